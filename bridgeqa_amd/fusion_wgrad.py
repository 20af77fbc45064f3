"""Native-GEMM helpers and the DEFERRED, grouped weight gradients of the fusion path (bridgeqa_amd/fusion_ops.py re-exports
everything here): a backward phase computes only the dX chain and parks (dY, X, weight, bias) records; one grouped launch per
tile class produces all dW / db of the phase at its end (reference: the autograd of nn.Linear, models/vit.py:30-32,51-53,
models/med.py:112-118,232,295,310)."""
import os

import torch
import torch.nn.functional as F

from .fusion_state import *  # noqa: F401,F403
from .fusion_state import __all__ as _state_all
# the weight-gradient tile classes live beside the GEMM tile policy; the cells keep their names here (tools flip them)
from .gemm_route import DW_TILE as _DW_TILE, SHORT_DW_MIN_ROWS as _SHORT_DW_MIN_ROWS  # noqa: F401
from .gemm_route import SHORT_DW_TILE as _SHORT_DW_TILE, wgrad_class

# ---- native GEMMs (csrc/gemm.hip through _ext.gemm_*) ------------------------------------------------------------
# Every nn.Linear of the fusion half on the bf16 CUDA path: forward (+bias, +GELU), input gradient (+GELU derivative,
# +bias gradient of the layer before), weight gradient (fp32).  BQ_TORCH_GEMM=1 is a MEASUREMENT knob only: it routes
# the same call sites to torch (hipBLASLt) so that bench.py can A/B the kernels inside the whole step.
_NATIVE_GEMM = [True]   # (tests / tools flip it to run the torch composition of the same node)


def _rows(t):
    """(M, K) bf16 view/copy the GEMM kernels accept: contiguous last dim, 16-B aligned rows"""
    t2 = t.reshape(-1, t.shape[-1])
    if t2.dtype != torch.bfloat16:
        t2 = t2.to(torch.bfloat16)
    if t2.stride(1) != 1 or t2.stride(0) % 8 or t2.data_ptr() % 16:
        t2 = t2.contiguous()
    return t2


def _native_ok(t, N, K):
    """forward y (M, N) = x (M, K) w^T: the contraction K is K-contiguous in both operands => K % 64"""
    return _NATIVE_GEMM[0] and t.is_cuda and compute_dtype() == torch.bfloat16 and K % 64 == 0 and N % 8 == 0


def _native_dx_ok(t, N, K):
    """input gradient dx (M, K) = dy (M, N) w: the contraction is N (K-contiguous in dy) => N % 64"""
    return _NATIVE_GEMM[0] and t.is_cuda and compute_dtype() == torch.bfloat16 and N % 64 == 0 and K % 8 == 0


def _f32_bias(bias):
    """the fp32 master bias itself when possible (no operand copy needed: the kernel adds fp32), else its shadow"""
    if bias is None:
        return None
    if bias.dtype == torch.float32 and bias.is_contiguous():
        return bias.detach()
    return _shadow(bias)


def _mm_f32(a, b):
    """a @ b for bf16 operands with an fp32 result (torch fallback of the weight gradient)"""
    return torch.mm(a.float(), b.float()) if not a.is_cuda else torch.mm(a, b, out_dtype=torch.float32)


def _dw_db(g2, x2, need_dw, need_db):
    """weight / bias gradient of one linear, now: dW = g2^T x2 (fp32), db = column sums of g2 (fp32)"""
    dw = db = None
    native = g2.is_cuda and g2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and g2.shape[1] % 8 == 0 \
        and x2.shape[1] % 8 == 0 and _NATIVE_GEMM[0]
    if need_dw:
        if native:
            from . import _ext
            dw = _ext.gemm_dw(_rows(g2), _rows(x2), tile=256 if wgrad_class(g2.shape[0]) == "big" else 64)
        else:
            dw = _mm_f32(g2.t(), x2)
    if need_db:
        if native:
            from . import _ext
            db = _ext.colsum_grouped([_rows(g2)])[0]
        else:
            db = g2.sum(0, dtype=torch.float32)
    return dw, db


# ---- deferred, grouped weight gradients ---------------------------------------------------------------------------
# dW / db are not on the critical path of a backward pass.  Inside a begin/flush scope the backward of every bf16
# linear computes ONLY dX and parks (dY, X, parameters); flush_deferred_wgrad() then produces ALL weight gradients
# of the scope with ONE grouped GEMM launch per tile class (12 ViT blocks x 4 linears = 48 problems, 1296 tiles of
# 256 x 256 with the full 16400-row contraction each -- instead of 48 launches of 27-36 tiles) and ALL bias gradients
# with one grouped column-sum launch.  MI355X has the HBM for it: the parked dY of config c3 are 2.7 GB.
_DEFER = [None]


def begin_deferred_wgrad():
    _DEFER[0] = []


def _accumulate_grad(p, g):
    if p is None or not p.requires_grad:
        return
    if p.grad is None:
        p.grad = g
    else:
        p.grad.add_(g)


def take_deferred_wgrad():
    """end the scope WITHOUT computing: returns the parked (dY, X, weights, biases) records for
    flush_deferred_items() -- pipeline.PhasedTrainStep produces the fusion phase's weight gradients on another stream,
    off the critical path between the fusion backward and the image / detector backward"""
    items, _DEFER[0] = _DEFER[0], None
    return items or []


def flush_deferred_wgrad():
    """compute the parked weight / bias gradients (current stream) and store them in the parameters' .grad"""
    flush_deferred_items(take_deferred_wgrad())


_PLAN_CACHE = {}
_PLAN_WGRAD = [True]
_QSUM = [True]
_QSUM64 = [True]
_TWO_SOURCE = [True]   # (tools / tests flip it: False = every second row source through the 64-tile adder launch, as before)


def plan_big_launches(tiles, cus, max_problems=36, moved_cost=0.011):
    """How to issue the 256 x 256-tile weight-gradient problems of one flush.  Every tile of such a launch runs the full
    contraction (all rows of the batch), so a launch costs ceil(tiles / cus) rounds of equal length -- 1296 tiles on 256 CUs
    are 5.06 rounds, i.e. SIX, for sixteen tiles.  Returns (groups, moved): `groups` = lists of problem indices, one grouped
    launch each (<= max_problems problems, the kernel-argument limit), `moved` = indices of small problems sent to the
    64 x 64-tile kernel instead, chosen so that rounds + moved_cost * (tiles moved) is smallest.  The problems come in a
    handful of distinct sizes, so the search walks the counts per size of the second launch (a few thousand cases, cached)."""
    key = (tuple(tiles), cus, max_problems)
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return hit
    n = len(tiles)
    rounds = lambda t: -(-t // cus) if t > 0 else 0
    order = sorted(range(n), key=lambda k: tiles[k])
    default = [list(range(n))[i:i + max_problems] for i in range(0, n, max_problems)]
    best = (sum(rounds(sum(tiles[k] for k in g)) for g in default), default, [])
    if n <= 2 * max_problems:
        for m in range(0, min(6, n)):
            moved = order[:m]
            rest = order[m:]
            cost_moved = moved_cost * sum(tiles[k] for k in moved)
            by_size = {}
            for k in rest:
                by_size.setdefault(tiles[k], []).append(k)
            sizes = sorted(by_size)
            if len(sizes) > 5:
                break
            total, cnt = sum(tiles[k] for k in rest), len(rest)
            combos = [[]]
            for sz in sizes:
                combos = [c + [x] for c in combos for x in range(len(by_size[sz]) + 1)]
                if len(combos) > 50000:
                    combos = None
                    break
            if combos is None:
                break
            for c in combos:
                nb = sum(c)
                if nb > max_problems or cnt - nb > max_problems:
                    continue
                tb = sum(x * sz for x, sz in zip(c, sizes))
                cost = rounds(tb) + rounds(total - tb) + cost_moved
                if cost < best[0] - 1e-9:
                    gb = [k for x, sz in zip(c, sizes) for k in by_size[sz][:x]]
                    ga = [k for x, sz in zip(c, sizes) for k in by_size[sz][x:]]
                    best = (cost, [g for g in (ga, gb) if g], list(moved))
    plan = (best[1], best[2])
    _PLAN_CACHE[key] = plan
    return plan


def split_for_table(group, two, max_entries=36):
    """One planned 256-tile launch whose problems `group` (longest contraction first) need more kernel-argument entries than a
    launch has -- a problem with a second row source takes two (two[k]) -- as the fewest launches that fit, the problems DEALT
    round-robin: every launch gets the same mix of long and short contractions.  Cutting the list where the table is full (what
    the library does with it) leaves all the long ones in the first launch: the twin K/V flush (12 x 257 and 12 x 64 K tiles,
    18 tiles each) then ran 324 tiles with 41 long ones on each of the first XCDs' 32 CUs -- two long rounds -- and a
    108-tile tail, 880 + 126 us under the profiler; dealt, each launch is 216 tiles, resident at once: 415 + 410 us
    (profiles/wgrad_two_source.md)."""
    entries = len(group) + sum(two)
    n = -(-entries // max_entries)
    if n <= 1:
        return [list(group)]
    chunks = [group[c::n] for c in range(n)]
    sizes = [len(group[c::n]) + sum(two[c::n]) for c in range(n)]
    if max(sizes) > max_entries:   # (an uneven deal of mixed problems: fall back to cutting the list in order)
        chunks, cur, used = [], [], 0
        for k, t in zip(group, two):
            if used + 1 + t > max_entries:
                chunks.append(cur)
                cur, used = [], 0
            cur.append(k)
            used += 1 + t
        chunks.append(cur)
    return [c for c in chunks if c]


def _nrows(t):
    """rows of a GEMM row operand: (rows, cols), or a (batch, rows, cols) batched-row view (_ext._mat_rows)"""
    return t.shape[0] if t.dim() == 2 else t.shape[0] * t.shape[1]


def flush_deferred_items(items):
    """items: (dY, X, weights, biases[, primary]) records.  `primary` (optional) = index of ANOTHER record of the same
    weights: this record's rows are a second row source of that weight gradient (the twin K/V projection reads image
    tokens and the other stream's states, _TwinKVFn): summed inside the primary's launch when that is the 256 x 256 kernel's,
    otherwise ADDED to it by a launch behind the primary one."""
    if not items:
        return
    from . import _ext
    flags = _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32
    items = [tuple(it) + (None,) * (5 - len(it)) for it in items]
    dws = [None] * len(items)
    prim = [k for k, it in enumerate(items) if it[4] is None]
    second = [k for k, it in enumerate(items) if it[4] is not None]
    # (mid = only the SHORT contractions: the planner's moved problems below -- full 16 400-row contractions of 9 tiles --
    # stay on the 64-tile kernel, whose cut contraction spreads them over the chip: the 256 x 128 form ran them at 5 % MFMA busy)
    cls = {k: wgrad_class(_nrows(items[k][0]), (items[k][0].shape[-1], items[k][1].shape[-1], items[k][0].dim() == 2))
           for k in prim}
    big, mid, small = ([k for k in prim if cls[k] == c] for c in ("big", "mid", "small"))
    if _PLAN_WGRAD[0]:
        # longest contractions first: a launch's workgroups start in tile order, so the long tiles (16 720-row image
        # tokens) run from the beginning and the short ones (4 416-row object tokens) fill in behind them (A/B x4: 40.88 vs
        # 40.91 ms -- inside the noise; kept because it cannot hurt)
        big.sort(key=lambda k: -_nrows(items[k][0]))
    groups = [big] if big else []
    if big and _PLAN_WGRAD[0]:
        tj = _DW_TILE[0]
        tiles = [-(-items[k][0].shape[-1] // tj) * -(-items[k][1].shape[-1] // 256) for k in big]
        cus = torch.cuda.get_device_properties(items[big[0]][0].device).multi_processor_count
        plan_groups, moved = plan_big_launches(tiles, cus * (256 // tj))
        groups = [[big[j] for j in g] for g in plan_groups]
        small = small + [big[j] for j in moved]
    # a second row source whose primary runs on the 256 x 256 kernel rides in that launch as a second contraction segment
    # (_ext.gemm_grouped P2 / Q2: its K tiles follow the primary's in the same workgroups, no pass over the stored gradient, no
    # atomics; one workgroup owns a tile, so the sum is fixed-order in every mode).  The planner above counted tiles without
    # them -- a segment adds none; the library splits a launch after 18 such pairs.
    attach = {}
    if _TWO_SOURCE[0] and _DW_TILE[0] == 256:
        on_big = {k for g in groups for k in g}
        for k in second:
            if items[k][4] in on_big and (items[k][3] is None or _QSUM[0]):   # (the bias gradient comes from the same launch)
                attach.setdefault(items[k][4], k)   # (a kernel problem carries ONE segment: further sources keep the adder)
        second = [k for k in second if attach.get(items[k][4]) != k]
        groups = [c for g in groups for c in split_for_table(g, [k in attach for k in g])]
    dbs = {}
    for tile, idx_groups in ((_DW_TILE[0], groups), (_SHORT_DW_TILE[0], [mid] if mid else []), (64, [small] if small else [])):
        for idx in idx_groups:
            probs = []
            for k in idx:
                g2, x2 = items[k][0], items[k][1]
                dws[k] = torch.empty(g2.shape[-1], x2.shape[-1], dtype=torch.float32, device=g2.device)
                pr = dict(P=x2, Q=g2, out=dws[k])
                if k in attach:
                    pr.update(P2=items[attach[k]][1], Q2=items[attach[k]][0])
                if items[k][3] is not None and _QSUM[0] and (tile != 64 or _QSUM64[0]):
                    # the bias gradient (column sums of dY) from the same launch: four more MFMAs per K tile in a third
                    # of the workgroups instead of a second pass over dY (csrc/gemm.hip, QSUM)
                    dbs[k] = torch.empty(g2.shape[-1], dtype=torch.float32, device=g2.device)
                    pr["colsum"] = dbs[k]
                probs.append(pr)
            _ext.gemm_grouped(probs, flags, _ext.EPI_NONE, tile)
    with_b = [k for k in prim if items[k][3] is not None and k not in dbs]
    if with_b:
        dbs.update(zip(with_b, _ext.colsum_grouped([items[k][0].reshape(-1, items[k][0].shape[-1]) for k in with_b])))
    if second:
        # second row sources: added onto the stored gradient of their primary record (same stream: ordered behind it) by
        # the small-tile kernel's atomic epilogue -- short contractions (B x 20 text rows).  ONE adder per element onto a value
        # an earlier launch of the same stream stored: bitwise reproducible as it is (the deterministic mode runs the same sum
        # with a plain load and store, gemm64_kernel_det)
        probs = []
        for k in second:
            g2, x2, pk = items[k][0], items[k][1], items[k][4]
            pr = dict(P=x2, Q=g2, out=dws[pk], accum=True)
            if items[pk][3] is not None:
                pr["colsum"] = dbs[pk]
            probs.append(pr)
        _ext.gemm_grouped(probs, flags, _ext.EPI_NONE, 64)
    for k in prim:
        g2, x2, ws, bs = items[k][:4]
        n = g2.shape[-1] // len(ws)
        for j, w in enumerate(ws):
            _accumulate_grad(w, dws[k][j * n:(j + 1) * n] if len(ws) > 1 else dws[k].view(w.shape))
            if bs is not None:
                _accumulate_grad(bs[j], dbs[k][j * n:(j + 1) * n] if len(ws) > 1 else dbs[k])


def _defer_ok(g2, x2):
    return (_DEFER[0] is not None and _NATIVE_GEMM[0] and g2.is_cuda and g2.dtype == torch.bfloat16
            and x2.dtype == torch.bfloat16 and g2.shape[1] % 8 == 0 and x2.shape[1] % 8 == 0)


def _park(g2, x2, ws, bs):
    _DEFER[0].append((_rows(g2), _rows(x2), ws, bs))


def _park_two(g_a, x_a, g_b, x_b, ws, bs):
    """one weight gradient from TWO row sources: dW = g_a^T x_a + g_b^T x_b (g_*: (rows, N) or batched-row views
    (batch, rows, N) read in place; x_*: (rows, K)); the second source is added behind the first (flush_deferred_items)"""
    d = _DEFER[0]
    d.append((g_a, _rows(x_a), ws, bs))
    d.append((g_b, _rows(x_b), ws, bs, len(d) - 1))



__all__ = [n for n in list(globals()) if not n.startswith("__")]
