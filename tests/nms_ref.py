"""Reference, conditions, inputs and a numpy emulation of the two kernels of csrc/nms.hip (nms_kernel, box_point_count_kernel
behind _ext.nms / _ext.box_point_count and ap_helper._decode_predictions), for tests/test_nms_bound_cpu.py and
tests/test_nms_bound_gpu.py.  Nothing here needs a GPU or the extension.

NMS REFERENCE.  float64 from the fp32 boxes the kernel reads, the reference project's utils/nms.py:40-152 (nms_2d_faster,
nms_3d_faster, nms_3d_faster_samecls) as the specification:
    volume   v = (x2 - x1) (y2 - y1) (z2 - z1)              (the 2-D form is the 3-D one with z = [0, 1])
    overlap  inter = prod max(0, min(hi_i, hi_j) - max(lo_i, lo_j)),  o = inter / (v_i + v_j - inter);  old type: o = inter / v_j
             with j the OTHER box, i the picked one;  same-class mode: o = 0 between boxes of different classes
    visit    the valid boxes in the order: NaN scores first (numpy's argsort places NaN last = picked first), then score
             descending with +0.0 == -0.0 and +-inf as numbers; equal scores, and NaNs among themselves, by increasing index
    greedy   a visited box that is still alive is kept and removes every other alive box with o > thr -- strictly, against the
             Python float thr (a double); a NaN overlap (0 / 0 of zero-volume boxes) never suppresses, as in numpy; an invalid
             box is neither visited nor suppressing
The kernel does the same double operations in the same order (every product, sum and quotient rounds once, nothing contracts:
-ffp-contract=off, and min / max of fp32 values are exact), so `keep` must EQUAL the reference's: tolerance 0.  A decision is
CONTESTED where 0 < |o - thr| <= 4 x 2^-52 thr; nms_reference counts them among the pairs it evaluates and every case must have
none.  o == thr exactly is a legitimate case: not suppressed.  nms_literal() is the np.argsort / np.delete form of the
specification (invalid boxes removed beforehand, as lib/ap_helper.py:116-120 does); numpy leaves the order of tied and NaN
scores to its sort, so it is compared only on runs without either.

POINT-IN-BOX REFERENCE.  float64 from the fp32 inputs: d = p - c, x = ct dx - st dz, y = dy, z = st dx + ct dz with ct = cos t,
st = sin t (local = roty(t)^T (p - c), the inverse of proposal_module.box_corners), inside iff |x| <= |l| / 2, |y| <= |w| / 2 and
|z| <= |h| / 2: the closed box of |size|, the hull of the eight corners.
What the kernel's fp32 values may differ by (u = 2^-24, every operation rounds once to nearest, -ffp-contract=off):
    difference  dx_f = fl(px - cx): e_d = u |dx|, and 0 where the exact difference IS an fp32 number (nothing rounds)
    trig        ct_f = cosf(t), st_f = sinf(t): |ct_f - ct| <= T = 16 u ABSOLUTE.  Nobody has measured OCML's sinf / cosf on this
                device; its documentation speaks of 1 to 2 ulp, and an ulp of a value below 1 is at most u, so T is 8 to 16 times
                that -- deliberately generous.  cosf(0) = 1 and sinf(0) = 0 are exact: T = 0 where the heading is exactly 0,
                and then both products (by 1 and by 0) and the add (of 0) are exact as well (r = 0 below, else r = u)
    product     a_f = fl(ct_f dx_f):  e_a0 = |ct| e_d + T |dx| + T e_d,   e_a = e_a0 + r (|ct dx| + e_a0)
    add         x_f = fl(a_f - b_f):  e_x = e_a + e_b + r (|x| + e_a + e_b);  z likewise;  y = dy_f: e_y = e_d
    half size   0.5f * size is exact for every normal fp32 number (a change of exponent), fabsf is exact; below 2^-125 the halving
                may round into the subnormals: e_h = 2^-149 there, 0 elsewhere
A coordinate is SURE inside where |size| / 2 - |coord| > e (or >= 0 where e = 0: the closed face), sure outside where it is < -e,
CONTESTED in between.  A (box, point) pair is sure inside where all three coordinates are, sure outside where any is, contested
otherwise.  The test demands, per box,  n_sure <= count <= n_sure + n_contested  (both clamped to cap where cap > 0), which is
equality wherever n_contested = 0.  A wide band can only enlarge the contested set, and that set is capped -- conditions, not
tolerances, asserted by count_conditions() on every case: contested pairs <= 1e-3 of all (box, point) pairs, at least 90 % of
the boxes have n_contested = 0, and no box's `>= 5` decision (the caller's cap = 5) is contested.

Against the issue: (1) it calls a pair contested where ANY | |coord| - half | lies within the error; here a pair that is surely
outside on another axis is sure, not contested -- a subset of the issue's set, so the interval is never wider than the issue's.
(2) The rounding of a difference is taken as 0 where the exact difference is an fp32 number, and the heading-0 products and add
as exact; this is what gives the lattice cases tolerance 0, which the issue demands of them.  (3) The halving of the size is
exact for normal numbers; the issue lists it as an error term, it contributes 2^-149 in the subnormal range only.  (4) The cap
defect `cap_ge` is read as the guard `cap > 0` written `cap >= 0` (cap = 0, "no clamp", then clamps every count to 0): `tot >=
cap ? cap : tot` equals the kernel's expression and could not be rejected.  (5) The defect "the picked box suppressing itself"
is read as a kernel that lets the picked box take part in its own suppression pass and reports the boxes still alive after it.
(6) Random NMS cases use 2 to 3 classes so that the same-class modes still suppress.  Nothing else differs.

EMULATION.  nms_emulate() restates the kernel's partition: the rank of box i = the number of boxes visited before it, order[rank]
= i, then K sequential passes whose suppression loop runs over j in strides of 256.  It raises PartitionError unless every slot
of `order` is written exactly once -- the ranks are a permutation of 0..K-1 -- for ANY scores, NaN and +-inf included; the
comparison the kernel used before (`sj > si || (sj == si && j < i)`, defect nan_blind) gives a NaN box rank 0 next to the true
best box and leaves slot K-1 unwritten.  count_emulate() restates the count in fp32 numpy: lane = i mod 256 sums its stride, 64
lanes fold into a wave partial, four partials add up.  `defect=` plants one wrong decision each (NMS_DEFECTS, COUNT_DEFECTS).

CASES (the smallest shapes that reach each mechanism; NMS cases run in the six MODES unless they fix the mode).
    one         B = K = 1
    strides     K = 255, 256, 257 with B = 3, a sixth of the boxes invalid: the tail of both stride loops, the scene offset
    full        B = 2, K = 1024, the limit of the kernel's LDS tables
    ties        K = 300, scores in {0, 0.5, 0.75, 1}: runs of exactly duplicated boxes, many scores 1.0, a (-0.0, +0.0) pair
    invalid     half invalid at random; the top-scored box invalid; a scene entirely invalid (keep all False); valid = None
    threshold   dyadic pairs with o = 0.25 and 0.5 exactly (kept) and one fp32 step above (suppressed); for thr in 0.2, 0.3, 0.7
                a pair whose overlap lies between thr and float32(thr) (old type against a unit cube: o = float32(thr) itself for
                0.2 and 0.3; for 0.7 three fp32 extents found by a seeded search)
    fp32_flip   pairs, found by a seeded search, whose overlap computed in fp32 falls on the other side of thr
    degenerate  zero-volume boxes (0 / 0), nested, identical and disjoint boxes, and the same scene translated by +1000
    asym        old-type pairs of very unequal volume in both score orders
    nonfinite   NaN, +inf, -inf among finite scores, K = 64 and 257, the NaN at index 0, K - 1 and in the middle
    lattice     heading 0, dyadic coordinates: points inside, on a face, an edge, a corner (counted), one fp32 step outside (not),
                boxes holding exactly 4, 5, 6 points, a zero size component, cap 0 and 5; tolerance 0
    tails       N = 1, 63, 64, 255, 256, 257, 513 with K = 7, B = 2, boxes that hold every point or about half of them
    random      B = 2, N = 1000, K = 40, ld = 3 and 7, headings over [-2 pi, 2 pi], sizes 0.1 to 1.6
    negative    one, two and three negative size components: the counts of |size|
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
EPS = 2.0 ** -52
TRIG = 16 * U          # absolute error granted to cosf / sinf (see above: generous, not measured)
CAP = 5                # ap_helper's `count >= 5`
PAIR_CAP = 1e-3
LANES, WAVE = 256, 64
NMS_MAX_K = 1024
f32, f64 = np.float32, np.float64

# name -> (two_d, same_cls, old_type, thr)
MODES = {"3d": (False, False, False, 0.25), "3d_old": (False, False, True, 0.2), "cls": (False, True, False, 0.25),
         "cls_old": (False, True, True, 0.3), "2d": (True, False, False, 0.3), "2d_old": (True, False, True, 0.25)}


class PartitionError(AssertionError):
    """the rank sort did not write every slot of `order` exactly once"""


# ---- NMS: reference -----------------------------------------------------------------------------------------------------------
def visit_order(score):
    """indices of a scene's boxes in visiting order (see the docstring); score (K,) fp32"""
    s = np.asarray(score, dtype=f64)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -np.where(nan, 0.0, s), ~nan))


def _overlap(lo, hi, vol, i, old_type):
    ext = [np.maximum(0.0, np.minimum(hi[i, a], hi[:, a]) - np.maximum(lo[i, a], lo[:, a])) for a in range(3)]
    inter = ext[0] * ext[1] * ext[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / vol if old_type else inter / (vol[i] + vol - inter)


def nms_reference(run):
    """-> keep (B, K) bool, info dict(contested, evaluated, kept, valid)"""
    box, score, cls, valid = run["box"].astype(f64), run["score"], run["cls"], run["valid"]
    thr, old_type, same_cls = run["thr"], run["old_type"], run["same_cls"]
    assert isinstance(thr, float) and box.dtype == f64 and run["box"].dtype == f32 and score.dtype == f32
    B, K = score.shape
    keep = np.zeros((B, K), dtype=bool)
    contested = evaluated = 0
    for b in range(B):
        lo, hi = box[b, :, :3], box[b, :, 3:]
        d = hi - lo
        vol = d[:, 0] * d[:, 1] * d[:, 2]
        alive = np.ones(K, dtype=bool) if valid is None else valid[b].astype(bool).copy()
        for i in visit_order(score[b]):
            if not alive[i]:
                continue
            keep[b, i] = True
            alive[i] = False
            o = _overlap(lo, hi, vol, i, old_type)
            if same_cls:
                o = np.where(cls[b] == cls[b, i], o, 0.0)
            with np.errstate(invalid="ignore"):
                contested += int((alive & (o != thr) & (np.abs(o - thr) <= 4 * EPS * thr)).sum())
                evaluated += int(alive.sum())
                alive &= ~(o > thr)
    n_valid = B * K if valid is None else int(valid.astype(bool).sum())
    return keep, dict(contested=contested, evaluated=evaluated, kept=int(keep.sum()), valid=n_valid)


def nms_literal(run):
    """the specification in its own form: ascending argsort, the last entry picked, np.delete of the suppressed positions;
    invalid boxes are taken out beforehand and the picks mapped back.  Defined only without tied or NaN scores."""
    box, score, cls, valid = run["box"].astype(f64), run["score"], run["cls"], run["valid"]
    thr, old_type, same_cls = run["thr"], run["old_type"], run["same_cls"]
    B, K = score.shape
    keep = np.zeros((B, K), dtype=bool)
    for b in range(B):
        sel = np.arange(K) if valid is None else np.nonzero(valid[b])[0]
        bx, c = box[b, sel], cls[b, sel]
        vol = (bx[:, 3] - bx[:, 0]) * (bx[:, 4] - bx[:, 1]) * (bx[:, 5] - bx[:, 2])
        I = np.argsort(score[b, sel])
        pick = []
        while I.size != 0:
            i, rest = I[-1], I[:-1]
            pick.append(i)
            l = np.maximum(0, np.minimum(bx[i, 3], bx[rest, 3]) - np.maximum(bx[i, 0], bx[rest, 0]))
            w = np.maximum(0, np.minimum(bx[i, 4], bx[rest, 4]) - np.maximum(bx[i, 1], bx[rest, 1]))
            h = np.maximum(0, np.minimum(bx[i, 5], bx[rest, 5]) - np.maximum(bx[i, 2], bx[rest, 2]))
            inter = l * w * h
            with np.errstate(invalid="ignore", divide="ignore"):
                o = inter / vol[rest] if old_type else inter / (vol[i] + vol[rest] - inter)
                if same_cls:
                    o = o * (c[i] == c[rest])
                gone = np.where(o > thr)[0]
            I = np.delete(I, np.concatenate(([I.size - 1], gone)).astype(np.int64))
        keep[b, sel[np.asarray(pick, dtype=np.int64)]] = True
    return keep


def has_ties_or_nan(run):
    s = run["score"]
    return bool(np.isnan(s).any()) or any(len(np.unique(row.astype(f64) + 0.0)) < len(row) for row in s)


# ---- NMS: emulation of the kernel's partition ----------------------------------------------------------------------------------
NMS_DEFECTS = ("ties_desc", "ge", "old_picked", "cls_ignored", "cls_always", "invalid_suppresses", "invalid_picked", "offset_cls",
               "offset_valid", "tail_rank", "tail_suppress", "fp32", "thresh_fp32", "self_suppress", "nan_blind")


def rank_sort(score, defect=None):
    """order (K,) of one scene as the kernel's rank sort forms it; PartitionError unless the ranks are a permutation"""
    s = np.asarray(score, dtype=f32)
    K = len(s)
    idx = np.arange(K)
    si, sj = s[:, None], s[None, :]
    ni, nj = np.isnan(si), np.isnan(sj)
    jl = (idx[None, :] > idx[:, None]) if defect == "ties_desc" else (idx[None, :] < idx[:, None])
    with np.errstate(invalid="ignore"):
        plain = (sj > si) | ((sj == si) & jl)
    first = plain if defect == "nan_blind" else np.where(nj, ~ni | jl, ~ni & plain)
    rank = first.sum(axis=1)
    ranked = idx[idx < LANES] if defect == "tail_rank" else idx            # tail_rank: `i = t` without the `i += 256` trips
    written = np.bincount(rank[ranked], minlength=K)
    if not (len(written) == K and bool((written == 1).all())):
        raise PartitionError("rank sort: %d slots of order[0..%d] unwritten, %d written more than once"
                             % (int((written[:K] == 0).sum()), K - 1, int((written > 1).sum())))
    order = np.empty(K, dtype=np.int64)
    order[rank] = idx
    return order


def nms_emulate(run, defect=None):
    score, cls, valid = run["score"], run["cls"], run["valid"]
    thr, old_type, same_cls = run["thr"], run["old_type"], run["same_cls"]
    wt = f32 if defect == "fp32" else f64
    box = run["box"].astype(wt)
    if defect == "thresh_fp32":
        thr = float(f32(thr))
    B, K = score.shape
    keep = np.zeros((B, K), dtype=bool)
    j_all = np.arange(K)
    for b in range(B):
        lo, hi = box[b, :, :3], box[b, :, 3:]
        d = hi - lo
        vol = d[:, 0] * d[:, 1] * d[:, 2]
        vb = valid[0 if defect == "offset_valid" else b] if valid is not None else None
        cb = cls[0 if defect == "offset_cls" else b]
        real = np.ones(K, dtype=bool) if vb is None else vb.astype(bool)
        alive = np.ones(K, dtype=bool) if defect in ("invalid_picked", "invalid_suppresses") else real.copy()
        order = rank_sort(score[b], defect)
        for pos in range(K):
            i = order[pos]
            if not alive[i]:
                continue
            ext = [np.maximum(wt(0), np.minimum(hi[i, a], hi[:, a]) - np.maximum(lo[i, a], lo[:, a])) for a in range(3)]
            inter = ext[0] * ext[1] * ext[2]
            with np.errstate(invalid="ignore", divide="ignore"):
                if old_type:
                    o = inter / (vol[i] if defect == "old_picked" else vol)
                else:
                    o = inter / (vol[i] + vol - inter)
            o = o.astype(f64)
            if (same_cls and defect != "cls_ignored") or defect == "cls_always":
                o = np.where(cb == cb[i], o, 0.0)
            with np.errstate(invalid="ignore"):
                hit = (o >= thr) if defect == "ge" else (o > thr)
            reach = alive & (j_all != i) if defect != "self_suppress" else alive.copy()
            if defect == "tail_suppress":
                reach &= j_all < LANES
            alive &= ~(reach & hit)
            if defect == "self_suppress":
                keep[b, i] = alive[i]                      # reports what is still alive after the pass
            else:
                keep[b, i] = real[i] if defect == "invalid_suppresses" else True
            alive[i] = False
    return keep


def nms_compare(keep, ref_keep):
    keep, ref_keep = np.asarray(keep).astype(bool), np.asarray(ref_keep).astype(bool)
    if keep.shape != ref_keep.shape:
        return ["keep has shape %s, the reference %s" % (keep.shape, ref_keep.shape)]
    bad = np.argwhere(keep != ref_keep)
    return ["keep[%d, %d] = %s, the reference says %s" % (b, k, keep[b, k], ref_keep[b, k]) for b, k in bad[:8]] + \
        (["... %d decisions differ" % len(bad)] if len(bad) > 8 else [])


# ---- NMS: inputs ----------------------------------------------------------------------------------------------------------------
def to_2d(box):
    """the bird's-eye form ap_helper hands over: (x1, z1, 0, x2, z2, 1)"""
    z, o = np.zeros_like(box[..., 0]), np.ones_like(box[..., 0])
    return np.stack([box[..., 0], box[..., 2], z, box[..., 3], box[..., 5], o], -1).astype(f32)


def _run(box, score, cls=None, valid=None, mode=None, thr=None, old_type=False, same_cls=False, two_d=False, tag=""):
    if mode is not None:
        two_d, same_cls, old_type, thr = MODES[mode]
        tag = (tag + " " + mode).strip()
    box = np.ascontiguousarray(box, dtype=f32)
    B, K = box.shape[:2]
    cls = np.zeros((B, K), dtype=np.int32) if cls is None else np.ascontiguousarray(cls, dtype=np.int32)
    return dict(box=to_2d(box) if two_d else box, score=np.ascontiguousarray(score, dtype=f32), cls=cls,
                valid=None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8), thr=float(thr),
                old_type=bool(old_type), same_cls=bool(same_cls), tag=tag, random=False)


def clustered(B, K, seed, n_cls=3):
    """boxes around a few hubs, as oracle/gen_golden_nms.py make_inputs places its proposals, so that suppression chains form;
    distinct scores (a permutation), classes 0..n_cls-1"""
    g = np.random.default_rng(seed)
    H = max(1, K // 5)
    hub = g.random((B, H, 3)) * (1.5 * H ** (1.0 / 3.0) + 0.5)
    c = hub[np.arange(B)[:, None], g.integers(0, H, (B, K))] + g.normal(size=(B, K, 3)) * 0.25
    s = g.random((B, K, 3)) * 0.8 + 0.4
    box = np.concatenate([c - s / 2, c + s / 2], -1).astype(f32)
    score = np.stack([(g.permutation(K) + 1.0) / (K + 1.0) for _ in range(B)]).astype(f32)
    return box, score, g.integers(0, n_cls, (B, K)).astype(np.int32), g


def _all_modes(box, score, cls, valid=None, tag="", random=True):
    runs = [_run(box, score, cls, valid, mode=m, tag=tag) for m in MODES]
    for r in runs:
        r["random"] = random
    return runs


def _next32(x, up=True):
    return f32(np.nextafter(f32(x), f32(np.inf if up else -np.inf)))


def _between(thr, seed=0):
    """three fp32 extents whose double product (x y) z lies strictly between float32(thr) and thr (thr = 0.7: below thr)"""
    t32 = float(f32(thr))
    lo, hi = min(t32, thr), max(t32, thr)
    g = np.random.default_rng(seed)
    for _ in range(100000):
        x, y = f32(g.uniform(0.8, 1.0)), f32(g.uniform(0.85, 1.0))
        z0 = f32(thr / (float(x) * float(y)))
        for z in (z0, _next32(z0), _next32(z0, False)):
            o = (float(x) * float(y)) * float(z)
            if lo < o < hi and z < 1:
                return x, y, z
    raise AssertionError("no extents found for thr = %r" % thr)


def _threshold_runs():
    runs = []
    unit = [0, 0, 0, 1, 1, 1]
    for thr in (0.25, 0.5):
        for step in (False, True):
            z = _next32(thr) if step else f32(thr)
            # 3-D: a slab of the unit cube: inter = z, union = 1; 2-D: the same slab in the bird's-eye plane (x, z)
            box = np.array([[unit, [0, 0, 0, 1, 1, z], [4, 4, 4, 5, 5, 5]]], dtype=f32)
            score = np.array([[0.9, 0.5, 0.1]], dtype=f32)
            for two_d in (False, True):
                for old in (False, True):
                    # old type: inter / the OTHER box's volume: the slab picked, the cube the other one
                    sc = score[:, [1, 0, 2]] if old else score
                    runs.append(_run(box, sc, thr=thr, old_type=old, two_d=two_d,
                                     tag="o %s %g %s%s" % ("one step above" if step else "==", thr, "2d" if two_d else "3d", " old" if old else "")))
    for thr in (0.2, 0.3):
        # old type against a unit cube: o = float32(thr) / 1, above thr
        box = np.array([[[0, 0, 0, 1, 1, f32(thr)], unit]], dtype=f32)
        runs.append(_run(box, [[0.9, 0.5]], thr=thr, old_type=True, tag="o = float32(%g) old" % thr))
        runs.append(_run(box, [[0.9, 0.5]], thr=thr, old_type=True, two_d=True, tag="o = float32(%g) old 2d" % thr))
        # IoU: the slab inside the cube: inter = slab, union = 1
        runs.append(_run(box[:, ::-1], [[0.9, 0.5]], thr=thr, tag="o = float32(%g) iou" % thr))
    x, y, z = _between(0.7)
    box = np.array([[[0, 0, 0, x, y, z], unit]], dtype=f32)
    runs.append(_run(box, [[0.9, 0.5]], thr=0.7, old_type=True, tag="float32(0.7) < o < 0.7 old"))
    runs.append(_run(box[:, ::-1], [[0.9, 0.5]], thr=0.7, tag="float32(0.7) < o < 0.7 iou"))
    return runs


def _o32(box, i, j, old_type):
    """the overlap of boxes i (picked) and j in fp32 arithmetic and in double"""
    out = []
    for wt in (f32, f64):
        b = box.astype(wt)
        ext = [np.maximum(wt(0), np.minimum(b[i, a + 3], b[j, a + 3]) - np.maximum(b[i, a], b[j, a])) for a in range(3)]
        inter = ext[0] * ext[1] * ext[2]
        v = [(b[k, 3] - b[k, 0]) * (b[k, 4] - b[k, 1]) * (b[k, 5] - b[k, 2]) for k in (i, j)]
        out.append(float(inter / v[1] if old_type else inter / (v[0] + v[1] - inter)))
    return out


def _fp32_flip_runs(per_mode=3, seed=1):
    """pairs whose overlap, computed in fp32, lies on the other side of thr than in double: box j's upper z is walked over the
    fp32 numbers next to the solution of o = thr"""
    runs = []
    g = np.random.default_rng(seed)
    for two_d, old, thr in ((False, False, 0.25), (False, True, 0.3), (True, False, 0.3), (True, True, 0.2)):
        found = 0
        for _ in range(20000):
            a = np.concatenate([g.random(3) * 0.3, 0.7 + g.random(3)]).astype(f32)          # picked
            c = np.concatenate([g.random(3) * 0.3 + 0.1, 0.5 + g.random(3)]).astype(f32)   # the other box
            if two_d:
                a[[1, 4]], c[[1, 4]] = (0, 1), (0, 1)
            # bisect box c's upper z (index 5) for o = thr in double, then look at the neighbouring fp32 numbers
            zl, zh = float(c[2]) + 1e-3, 3.0
            box = np.stack([a, c])
            f = lambda zz: _o32(np.stack([a, np.concatenate([c[:5], [f32(zz)]]).astype(f32)]), 0, 1, old)[1] - thr
            if not (f(zl) < 0 < f(zh) or f(zh) < 0 < f(zl)):
                continue
            up = f(zh) > 0
            for _ in range(60):
                zm = 0.5 * (zl + zh)
                if (f(zm) > 0) == up:
                    zh = zm
                else:
                    zl = zm
            z = f32(zl)
            for _ in range(4):
                z = _next32(z, False)
            for _ in range(9):
                box[1, 5] = z
                o32, o64 = _o32(box, 0, 1, old)
                if (o32 > thr) != (o64 > thr) and abs(o64 - thr) > 8 * EPS * thr:
                    b3 = box.copy()
                    if two_d:                                  # stored as a 3-D box whose (x, z) plane is the 2-D pair
                        b3 = np.stack([box[:, 0], np.zeros(2), box[:, 2], box[:, 3], np.ones(2), box[:, 5]], -1)
                    runs.append(_run(b3[None], [[0.9, 0.5]], thr=thr, old_type=old, two_d=two_d,
                                     tag="fp32 flips %s%s thr %g" % ("2d" if two_d else "3d", " old" if old else "", thr)))
                    found += 1
                    break
                z = _next32(z)
            if found == per_mode:
                break
        assert found == per_mode, "fp32_flip: search found %d pairs" % found
    return runs


def _ties_runs():
    box, _, cls, g = clustered(2, 300, 21, n_cls=2)
    score = g.choice(np.array([0.0, 0.5, 0.75, 1.0], dtype=f32), size=(2, 300), p=[0.2, 0.3, 0.3, 0.2])
    for b in range(2):
        for start in (10, 50, 120, 254, 290):                 # runs of exactly duplicated boxes with one score and one class
            box[b, start:start + 5], score[b, start:start + 5], cls[b, start:start + 5] = box[b, start], score[b, start], cls[b, start]
        # a (-0.0, +0.0) pair on duplicated boxes far from everything: the lower index must win
        box[b, 200:202], score[b, 200], score[b, 201], cls[b, 200:202] = [50, 50, 50, 51, 51, 51], -0.0, 0.0, 0
        score[b, 10:15] = 1.0
    assert (score == 1.0).sum() > 20 and np.signbit(score[0, 200]) and not np.signbit(score[0, 201])
    return _all_modes(box, score, cls, tag="ties")


def _invalid_runs():
    box, score, cls, g = clustered(4, 64, 31)
    valid = np.ones((4, 64), dtype=np.uint8)
    valid[0] = g.random(64) < 0.5
    valid[1, np.argmax(score[1])] = 0
    valid[2] = 0
    valid[3] = g.random(64) < 0.5
    runs = _all_modes(box, score, cls, valid, tag="invalid")
    runs += _all_modes(box, score, cls, None, tag="valid=None")
    return runs


def _degenerate_runs():
    box, score, cls, g = clustered(1, 40, 41)
    special = np.array([[1, 1, 1, 1, 2, 2], [1, 1, 1, 1, 2, 2], [1, 1, 1, 2, 1, 2], [3, 3, 3, 3, 3, 3],      # zero volume: 0 / 0
                        [0, 0, 0, 2, 2, 2], [0.5, 0.5, 0.5, 1.5, 1.5, 1.5], [0.75, 0.75, 0.75, 1, 1, 1],     # nested
                        [6, 6, 6, 7, 7, 7], [6, 6, 6, 7, 7, 7], [6, 6, 6, 7, 7, 7],                          # identical
                        [20, 0, 0, 21, 1, 1], [0, 20, 0, 1, 21, 1], [0, 0, 20, 1, 1, 21]], dtype=f32)         # disjoint
    n = len(special)
    box[0, :n] = special
    cls[0, :n] = 0
    box = np.concatenate([box, box + f32(1000.0)], 0).astype(f32)          # the scene again, translated by +1000
    score, cls = np.concatenate([score, score], 0), np.concatenate([cls, cls], 0)
    return _all_modes(box, score, cls, tag="degenerate", random=False)


def _asym_runs():
    big, small, far = [0, 0, 0, 8, 8, 8], [1, 1, 1, 1.5, 1.5, 1.5], [20, 20, 20, 21, 21, 21]
    box = np.array([[big, small, far], [big, small, far]], dtype=f32)
    score = np.array([[0.9, 0.5, 0.1], [0.5, 0.9, 0.1]], dtype=f32)        # the big box picked first / the small one
    return [_run(box, score, thr=thr, old_type=True, two_d=two_d, tag="asym %s thr %g" % ("2d" if two_d else "3d", thr))
            for two_d in (False, True) for thr in (0.2, 0.3)]


def _nonfinite_runs():
    runs = []
    for K in (64, 257):
        box, score, cls, g = clustered(3, K, 50 + K)
        nan, inf = f32(np.nan), f32(np.inf)
        score[0, 0] = nan
        score[1, K - 1] = nan
        score[2, K // 2], score[2, K // 2 + 3], score[2, 1] = nan, nan, nan
        for b in range(3):
            score[b, 5 + b], score[b, 20 + b], score[b, 30], score[b, 31] = inf, -inf, inf, -inf
        runs += _all_modes(box, score, cls, tag="nonfinite K=%d" % K, random=False)
    return runs


def _build_nms(name):
    if name == "one":
        return _all_modes(np.array([[[0, 0, 0, 1, 1, 1]]], dtype=f32), np.array([[0.5]], dtype=f32), np.zeros((1, 1)), random=False)
    if name == "strides":
        runs = []
        for K in (255, 256, 257):
            box, score, cls, g = clustered(3, K, K)
            runs += _all_modes(box, score, cls, (g.random((3, K)) > 1.0 / 6.0), tag="K=%d" % K)
        return runs
    if name == "full":
        box, score, cls, g = clustered(2, NMS_MAX_K, 7)
        return _all_modes(box, score, cls, tag="K=1024")
    return {"ties": _ties_runs, "invalid": _invalid_runs, "threshold": _threshold_runs, "fp32_flip": _fp32_flip_runs,
            "degenerate": _degenerate_runs, "asym": _asym_runs, "nonfinite": _nonfinite_runs}[name]()


NMS_CASES = ("one", "strides", "full", "ties", "invalid", "threshold", "fp32_flip", "degenerate", "asym", "nonfinite")


@functools.lru_cache(maxsize=None)
def nms_case(name):
    """-> tuple of runs (dicts of read-only arrays)"""
    runs = _build_nms(name)
    for r in runs:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tuple(runs)


@functools.lru_cache(maxsize=None)
def nms_reference_of(name):
    out = tuple(nms_reference(r) for r in nms_case(name))
    for keep, _ in out:
        keep.setflags(write=False)
    return out


def nms_conditions(run, keep, info):
    """the conditions the comparison rests on -> list of failures"""
    fails = []
    if info["contested"]:
        fails.append("%s: %d contested decisions" % (run["tag"], info["contested"]))
    if run["random"] and not 0.05 * info["valid"] <= info["kept"] <= 0.95 * info["valid"]:
        fails.append("%s: keeps %d of %d valid boxes" % (run["tag"], info["kept"], info["valid"]))
    if run["valid"] is not None and bool((keep & ~run["valid"].astype(bool)).any()):
        fails.append("%s: an invalid box is kept" % run["tag"])
    return fails


# ---- point count: reference -----------------------------------------------------------------------------------------------------
def count_reference(pc, center, size, heading):
    """-> dict(n_sure (B, K), n_contested (B, K), pairs); inputs fp32 arrays"""
    assert all(a.dtype == f32 for a in (pc, center, size, heading))
    p, c = pc[:, None, :, :3].astype(f64), center[:, :, None, :].astype(f64)
    d = p - c                                                             # (B, K, N, 3): exact in double
    ed = np.where(d.astype(f32).astype(f64) == d, 0.0, U * np.abs(d))
    t = heading.astype(f64)[:, :, None]
    ct, st = np.cos(t), np.sin(t)
    zero = heading[:, :, None] == 0
    T, r = np.where(zero, 0.0, TRIG), np.where(zero, 0.0, U)
    ct, st = np.where(zero, 1.0, ct), np.where(zero, 0.0, st)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    ex, ey, ez = ed[..., 0], ed[..., 1], ed[..., 2]

    def prod(cf, v, ev):
        e0 = np.abs(cf) * ev + T * np.abs(v) + T * ev
        return cf * v, e0 + r * (np.abs(cf * v) + e0)

    def add(a, ea, b, eb):
        return a + b, ea + eb + r * (np.abs(a + b) + ea + eb)
    x, e_x = add(*prod(ct, dx, ex), *prod(-st, dz, ez))
    z, e_z = add(*prod(st, dx, ex), *prod(ct, dz, ez))
    s = np.abs(size.astype(f64))[:, :, None, :]
    half = s / 2
    eh = np.where((s > 0) & (s < 2.0 ** -125), 2.0 ** -149, 0.0)
    sure_in, sure_out = True, False
    for a, (v, e) in enumerate(((x, e_x), (dy, ey), (z, e_z))):
        e = e + eh[..., a]
        m = half[..., a] - np.abs(v)
        sure_in = sure_in & ((m > e) | ((e == 0) & (m >= 0)))
        sure_out = sure_out | (m < -e)
    contested = ~sure_in & ~sure_out
    return dict(n_sure=sure_in.sum(-1), n_contested=contested.sum(-1), pairs=int(sure_in.size))


def count_compare(got, ref, cap=0):
    """n_sure <= count <= n_sure + n_contested per box, both ends clamped to cap > 0 -> list of failures"""
    got = np.asarray(got).astype(np.int64)
    lo, hi = ref["n_sure"], ref["n_sure"] + ref["n_contested"]
    if cap > 0:
        lo, hi = np.minimum(lo, cap), np.minimum(hi, cap)
    if got.shape != lo.shape:
        return ["count has shape %s, the reference %s" % (got.shape, lo.shape)]
    bad = np.argwhere((got < lo) | (got > hi))
    return ["count[%d, %d] = %d outside [%d, %d]" % (b, k, got[b, k], lo[b, k], hi[b, k]) for b, k in bad[:8]] + \
        (["... %d boxes differ" % len(bad)] if len(bad) > 8 else [])


def count_conditions(ref, tag=""):
    fails = []
    n, m = int(ref["n_contested"].sum()), ref["n_contested"].size
    if n > PAIR_CAP * ref["pairs"]:
        fails.append("%s: %d contested pairs of %d" % (tag, n, ref["pairs"]))
    if int((ref["n_contested"] == 0).sum()) < 0.9 * m:
        fails.append("%s: only %d of %d boxes are free of contested pairs" % (tag, int((ref["n_contested"] == 0).sum()), m))
    flip = (ref["n_sure"] < CAP) & (ref["n_sure"] + ref["n_contested"] >= CAP)
    if bool(flip.any()):
        fails.append("%s: the >= %d decision of %d boxes is contested" % (tag, CAP, int(flip.sum())))
    return fails


# ---- point count: emulation -----------------------------------------------------------------------------------------------------
COUNT_DEFECTS = ("drop_wave3", "drop_last_trip", "open_faces", "swap_wh", "sin_sign", "ld3", "signed_half", "cap_ge")


def count_emulate(pc, center, size, heading, cap=0, defect=None):
    """the kernel's fp32 arithmetic (numpy's cosf / sinf in place of the device's) and its partition of the sum"""
    B, N, ld = pc.shape
    K = center.shape[1]
    flat = pc.reshape(B, -1)
    row = np.arange(N) * (3 if defect == "ld3" else ld)
    lane = np.arange(N) % LANES
    trips = -(-N // LANES)
    out = np.zeros((B, K), dtype=np.int32)
    le = (lambda a, b: a < b) if defect == "open_faces" else (lambda a, b: a <= b)
    for b in range(B):
        px, py, pz = flat[b, row], flat[b, row + 1], flat[b, row + 2]
        for k in range(K):
            h = f32(0.5) * size[b, k]
            hl, hw, hh = h if defect == "signed_half" else np.abs(h)
            if defect == "swap_wh":
                hw, hh = hh, hw
            t = heading[b, k]
            ct, st = np.cos(t), np.sin(t)
            assert ct.dtype == f32
            if defect == "sin_sign":
                st = -st
            dx, dy, dz = px - center[b, k, 0], py - center[b, k, 1], pz - center[b, k, 2]
            x, z = ct * dx - st * dz, st * dx + ct * dz
            assert x.dtype == f32
            inside = le(np.abs(x), hl) & le(np.abs(dy), hw) & le(np.abs(z), hh)
            if defect == "drop_last_trip":
                inside &= np.arange(N) // LANES < trips - 1
            mine = np.bincount(lane[inside], minlength=LANES)              # what each of the 256 threads counted
            partial = mine.reshape(LANES // WAVE, WAVE).sum(axis=1)         # the 64-lane fold
            tot = int(partial[:3].sum() if defect == "drop_wave3" else partial.sum())
            clamp = cap >= 0 if defect == "cap_ge" else cap > 0
            out[b, k] = cap if clamp and tot > cap else tot
    return out


# ---- point count: inputs --------------------------------------------------------------------------------------------------------
def _crun(pc, center, size, heading, tag, expect=None, exact=False):
    r = dict(pc=np.ascontiguousarray(pc, dtype=f32), center=np.ascontiguousarray(center, dtype=f32),
             size=np.ascontiguousarray(size, dtype=f32), heading=np.ascontiguousarray(heading, dtype=f32), tag=tag,
             expect=None if expect is None else np.asarray(expect, dtype=np.int64), exact=exact)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _lattice_run():
    """heading 0 and dyadic coordinates: every decision exact.  Box 0 = centre (3, 2, 5), size (2, 1, 0.5); no coordinate or
    difference is subnormal, so a flush-to-zero mode could not matter."""
    c, h = np.array([3.0, 2.0, 5.0]), np.array([1.0, 0.5, 0.25])
    pts, inside0 = [], 0
    for q in ([0, 0, 0], [0.5, 0.25, 0.125], [-0.5, -0.25, 0.125], [0.75, 0, -0.125]):                 # strictly inside
        pts.append(c + q)
        inside0 += 1
    for sg in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],                     # faces
               [1, 1, 0], [-1, 0, 1], [0, -1, -1], [1, -1, 0],                                         # edges
               [1, 1, 1], [-1, -1, -1], [1, -1, 1], [-1, 1, -1]):                                      # corners
        pts.append(c + np.array(sg) * h)
        inside0 += 1
        for a in range(3):                                                                             # one fp32 step outside
            if sg[a]:
                q = (c + np.array(sg) * h).astype(f32)
                q[a] = _next32(q[a], up=sg[a] > 0)
                pts.append(q.astype(f64))
    # boxes 1, 2, 3 (unit cubes at x = 10, 20, 30) hold exactly 4, 5, 6 points, one of them on a face
    centers, sizes, expect = [c], [2 * h], [inside0]
    for n, x0 in ((4, 10.0), (5, 20.0), (6, 30.0)):
        centers.append(np.array([x0, 0.0, 0.0]))
        sizes.append(np.ones(3))
        expect.append(n)
        for i in range(n):
            pts.append(np.array([x0 + (0.5 if i == 0 else -0.25 + 0.0625 * i), 0.125 * i - 0.25, 0.25]))
        pts.append(np.array([float(_next32(x0 + 0.5)), 0.0, 0.0]))                                      # just outside
    # box 4: the size component w = 0 at x = 40: the points ON the plane y = 0 (3 of them), not the ones a step off it
    centers.append(np.array([40.0, 0.0, 0.0]))
    sizes.append(np.array([1.0, 0.0, 1.0]))
    expect.append(3)
    for q in ([40.0, 0.0, 0.0], [40.5, 0.0, 0.5], [39.75, -0.0, 0.25], [40.0, 2.0 ** -100, 0.0], [40.0, -2.0 ** -20, 0.0]):
        pts.append(np.array(q))
    # box 5: the same as box 0 with all three size components negative
    centers.append(c)
    sizes.append(-2 * h)
    expect.append(inside0)
    pts = np.array(pts)
    return _crun(pts[None], np.array(centers)[None], np.array(sizes)[None], np.zeros((1, len(centers))), "lattice",
                 expect=np.array(expect)[None], exact=True)


def _random_count(B, N, K, ld, seed, big=False, tag=""):
    g = np.random.default_rng(seed)
    pc = np.concatenate([g.random((B, N, 3)) * 4, g.normal(size=(B, N, ld - 3))], -1)
    center = g.random((B, K, 3)) * 4
    size = g.random((B, K, 3)) * 1.5 + 0.1
    if big:                                   # even boxes hold every point, odd ones about half (a face through the middle)
        size[:, 0::2] = 100.0
        size[:, 1::2] = (100.0, 100.0, 4.0)
        center[:, 1::2] = (2.0, 2.0, 0.0)
    heading = (g.random((B, K)) - 0.5) * 4 * math.pi
    return _crun(pc, center, size, heading, tag)


def _negative_run():
    r = _random_count(2, 300, 16, 4, 77, tag="negative")
    size = r["size"].copy()
    size[:, :, 1] *= 1.5                                                       # w != h on every box
    sign = np.ones((2, 16, 3), dtype=f32)
    for k in range(16):
        sign[:, k, [(k + j) % 3 for j in range(k % 3 + 1)]] = -1              # one, two and three negative components
    return _crun(r["pc"], r["center"], size * sign, r["heading"], "negative")


COUNT_CASES = ("lattice", "tails", "random", "negative")
TAIL_N = (1, 63, 64, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def count_case(name):
    if name == "lattice":
        return (_lattice_run(),)
    if name == "tails":
        return tuple(_random_count(2, N, 7, 3, 100 + N, big=True, tag="tails N=%d" % N) for N in TAIL_N)
    if name == "random":
        return tuple(_random_count(2, 1000, 40, ld, 200 + ld, tag="random ld=%d" % ld) for ld in (3, 7))
    if name == "negative":
        return (_negative_run(),)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def count_reference_of(name):
    return tuple(count_reference(r["pc"], r["center"], r["size"], r["heading"]) for r in count_case(name))
