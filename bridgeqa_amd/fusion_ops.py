"""Dense operators of the 2D-3D fusion path (ViT / MED-BERT twin encoder / LM decoder).

One narrow surface -- linear (+bias, +GELU), layer_norm (+residual), attention (additive mask,
optional probabilities), lm_loss -- so the modules in vit.py / med.py / blip_vqa_3d.py never
touch a kernel directly and every op has exactly one place where its MI355X implementation lives.

Precision policy ("bf16-in / fp32-accumulate allowed"): parameters stay fp32 (the
reference trains in fp32 and the state dict must round-trip); with `set_compute_dtype(bfloat16)`
GEMM operands are cast to bf16 and accumulate in fp32, softmax / LayerNorm statistics and the
residual stream stay fp32.  `float32` reproduces the reference arithmetic and is what the CPU
parity tests use.
"""
import math

import os

import torch
import torch.nn.functional as F

# the module is split in three (round 3): state + operand shadows, deferred weight gradients, and -- here -- the autograd
# nodes and the functional surface; the first two are re-exported so that `fusion_ops.X` keeps meaning what it meant
from .fusion_state import *  # noqa: F401,F403
from .fusion_wgrad import *  # noqa: F401,F403

# ---- gradient taps ------------------------------------------------------------------------------------------------
# A post-LN transformer sub-block reads its input twice: y = LN(x + f(x)).  Autograd therefore sums two gradients for x
# -- the residual one, which the LayerNorm backward produces first, and the input gradient of f's first linear -- with
# an accumulation kernel per site (~100 launches of 4-5 us in the text side of a c3 step).  A GradTap carries the first
# gradient to the node that produces the second, whose dX GEMM adds it in its epilogue (BQ_GEMM_EPI_ADD): the residual
# branch goes through tap(x, holder) (identity; its backward parks the incoming gradient in the holder and returns
# nothing), the linear receives tap=holder.  Autograd runs nodes in reverse creation order, so the tap -- created after the
# linear, just before the LayerNorm -- always fires before the linear's backward of the same pass.
# Should the consumer run first after all (its holder is then marked consumed), the tap simply returns its gradient to
# autograd, which accumulates it the ordinary way: the order is a performance assumption, never a correctness one.
class GradTap(object):
    __slots__ = ("grad", "consumed")

    def __init__(self):
        self.grad, self.consumed = None, False


class _TapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, holder):
        ctx.holder = holder
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        h = ctx.holder
        if h.consumed:
            return g, None
        h.grad = g if h.grad is None else h.grad + g
        return None, None


def tap(x, holder):
    """x for the residual branch; its gradient will reach x through the consumer that was given tap=holder"""
    if holder is None or not torch.is_tensor(x) or not x.requires_grad or not torch.is_grad_enabled():
        return x
    return _TapFn.apply(x, holder)


def _take_tap(holder, like_rows):
    """the parked gradient as (rows, K) bf16 rows laid out like the dX about to be produced, or None"""
    if holder is None:
        return None
    holder.consumed = True
    if holder.grad is None:
        return None
    g, holder.grad = holder.grad, None
    g2 = g.reshape(-1, g.shape[-1])
    if g2.dtype != torch.bfloat16:
        g2 = g2.to(torch.bfloat16)
    return g2 if g2.is_contiguous() else g2.contiguous()


# launches with fewer gradient rows read the transposed copy.  Round 4 first limited this to the text side (< 1024 rows: the
# latency chains, where the contraction-major read costs up to 2x); with the ViT's and the K/V projections' weights included
# the image backward window shrank by another 0.6 ms (A/B x2: 444.7 / 446.3 against 440.6 / 440.4 samples/s) for 0.1 ms more
# of transposes: in the step, beside the detector's backward, the contraction-major read loses more than alone (3-6 %)
_DX_T_ROWS = [1 << 30]


def _dx_wt(params, wb, rows):
    """the (K, N) transposed copy of the weight operand wb for a dX launch over `rows` gradient rows, or None: the launch then
    runs on the forward's K-contiguous operand form (fusion_state.transposed_shadow)"""
    if rows >= _DX_T_ROWS[0] or not wb.is_cuda:
        return None
    return transposed_shadow(tuple(params), wb)


def _dx_operands(param_groups, wops, rows):
    """(P operands, operand flag) of a GROUPED dX launch: every group's transposed copy and the K-contiguous form when all
    of them are small and have one, else the operands themselves read contraction-major"""
    from . import _ext
    if max(rows) < _DX_T_ROWS[0]:
        wts = [_dx_wt(ps, w, max(rows)) for ps, w in zip(param_groups, wops)]
        if all(t is not None for t in wts):
            return wts, 0
    return list(wops), _ext.GEMM_P_XC


class _LinearFn(torch.autograd.Function):
    """bf16-operand linear with fp32 master weights: the forward reads the bf16 shadow of W and the fp32 bias itself
    (bias / GELU in the GEMM epilogue), the backward produces dX with the same kernel family and dW / db in fp32
    (parked inside a deferred-wgrad scope)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gelu, tap_holder=None):
        wb = _shadow(weight)
        if wb.dim() > 2:  # a convolution whose stride equals its kernel (ViT patch embedding): (N, C, kh, kw) = (N, K)
            wb = wb.view(wb.shape[0], -1)
        N, K = wb.shape
        ctx.gelu, ctx.has_bias, ctx.x_dtype, ctx.x_shape = gelu, bias is not None, x.dtype, x.shape
        ctx.tap = tap_holder
        ctx.params = (weight, bias)
        if _native_ok(x, N, K):
            from . import _ext
            x2 = _rows(x)
            out = _ext.gemm_fwd(x2, wb, _f32_bias(bias), gelu=gelu)
            if gelu:
                ctx.save_for_backward(x2, wb, out[0])
                return out[1].view(*x.shape[:-1], N)
            ctx.save_for_backward(x2, wb)
            return out.view(*x.shape[:-1], N)
        bb = _shadow(bias) if bias is not None else None
        xb = x if x.dtype == compute_dtype() else x.to(compute_dtype())
        y = F.linear(xb, wb, bb)
        if gelu:
            ctx.save_for_backward(xb.reshape(-1, K), wb, y.reshape(-1, N))
            return F.gelu(y)
        ctx.save_for_backward(xb.reshape(-1, K), wb)
        return y

    @staticmethod
    def backward(ctx, g):
        if ctx.gelu:
            x2, wb, y = ctx.saved_tensors
            g2 = torch.ops.aten.gelu_backward(g.reshape(-1, g.shape[-1]), y)
        else:
            x2, wb = ctx.saved_tensors
            g2 = g.reshape(-1, g.shape[-1])
        N, K = wb.shape
        native = _native_dx_ok(g2, N, K)
        if g2.is_cuda and g2.dtype == torch.bfloat16:
            g2 = _rows(g2)
        w, b = ctx.params
        dw = db = None
        if _defer_ok(g2, x2) and ctx.needs_input_grad[1]:
            _park(g2, x2, [w], [b] if ctx.has_bias else None)
        else:
            dw, db = _dw_db(g2, x2, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        dx = None
        if ctx.needs_input_grad[0]:
            extra = _take_tap(ctx.tap, g2)
            if native:
                from . import _ext
                dx = _ext.gemm_dx(g2, wb, add=extra, wt=_dx_wt((w,), wb, g2.shape[0]))
            else:
                dx = torch.mm(g2, wb)
                if extra is not None:
                    dx = dx + extra
            dx = dx.view(ctx.x_shape).to(ctx.x_dtype)
        return dx, (dw.view(w.shape) if dw is not None else None), db, None, None


class _MlpFn(torch.autograd.Function):
    """fc2(gelu(fc1(x))) as ONE autograd node (reference models/vit.py:23-41 Mlp; models/med.py:292-317
    BertIntermediate + BertOutput.dense), so that the backward can fuse across the two layers:
      forward : GEMM(+b1, GELU epilogue: pre-activation and activation written by the same launch), GEMM(+b2)
      backward: dY1 = (dY2 W2) * gelu'(y1) in ONE launch (dGELU epilogue), dX = dY1 W1, dW1 / db1 / dW2 / db2 parked
                for the grouped launches (or computed at once outside a scope).  (The GEMM's fused column-sum epilogue
                for db1 was measured SLOWER in the step -- 235 vs 159 us per launch: 65 x 4 waves' fp32 atomics land on
                the same 12 KB -- than one more matrix in the grouped column-sum launch.)"""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, tap_holder=None):
        from . import _ext
        ctx.tap = tap_holder
        w1b, w2b = _shadow(w1), _shadow(w2)
        x2 = _rows(x)
        y1, h = _ext.gemm_fwd(x2, w1b, _f32_bias(b1), gelu=True)
        y2 = _ext.gemm_fwd(h, w2b, _f32_bias(b2))
        ctx.save_for_backward(x2, y1, h, w1b, w2b)
        ctx.params = (w1, b1, w2, b2)
        ctx.x_dtype, ctx.x_shape = x.dtype, x.shape
        return y2.view(*x.shape[:-1], w2b.shape[0])

    @staticmethod
    def backward(ctx, g):
        from . import _ext
        x2, y1, h, w1b, w2b = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        g2 = _rows(g)
        M = g2.shape[0]
        dy1 = _ext.gemm_dx(g2, w2b, pre_act=y1, wt=_dx_wt((w2,), w2b, M))
        dx = _ext.gemm_dx(dy1, w1b, add=_take_tap(ctx.tap, dy1), wt=_dx_wt((w1,), w1b, M)).view(ctx.x_shape).to(ctx.x_dtype) \
            if ctx.needs_input_grad[0] else None
        if _DEFER[0] is not None:
            _park(g2, h, [w2], [b2] if b2 is not None else None)
            _park(dy1, x2, [w1], [b1] if b1 is not None else None)
            dw1 = db1 = dw2 = db2 = None
        else:
            dw2, db2 = _dw_db(g2, h, True, b2 is not None)
            dw1, db1 = _dw_db(dy1, x2, True, b1 is not None)
        return dx, dw1, db1, dw2, db2, None


def mlp(x, fc1, fc2, tap=None):
    """fc2(gelu(fc1(x))) for two nn.Linear modules; one fused autograd node on the bf16 CUDA path.  tap: a GradTap whose
    parked gradient (of x, from the residual branch) is added to the input gradient by the last dX GEMM"""
    w1, w2 = fc1.weight, fc2.weight
    if (_native_ok(x, w1.shape[0], w1.shape[1]) and _native_ok(x, w2.shape[0], w2.shape[1])
            and _native_dx_ok(x, w1.shape[0], w1.shape[1]) and _native_dx_ok(x, w2.shape[0], w2.shape[1])
            and all(isinstance(t, torch.nn.Parameter) and t.dtype == torch.float32
                    for t in (w1, w2, fc1.bias, fc2.bias) if t is not None)):
        return _MlpFn.apply(x, w1, fc1.bias, w2, fc2.bias, tap)
    return linear(linear(x, w1, fc1.bias, act="gelu", tap=tap), w2, fc2.bias)


_CAT_CACHE = {}


def _cat_shadow(weights, biases):
    """bf16 [sum(N_i), K] / [sum(N_i)] concatenation of several linears' shadows.  Built once; afterwards the
    per-parameter shadows ARE row blocks of the concatenated buffers, so refreshing them (refresh_shadows, or the
    lazy path below) updates the fused operands in place -- no cat per step."""
    key = tuple(id(w) for w in weights)
    params = list(weights) + list(biases)
    hit = _CAT_CACHE.get(key)
    if (hit is not None and all(r() is w for r, w in zip(hit[0], params)) and hit[1].dtype == compute_dtype()
            and all(id(p) in _SHADOW and _SHADOW[id(p)][2].untyped_storage().data_ptr() ==
                    (hit[1] if p.dim() > 1 else hit[2]).untyped_storage().data_ptr() for p in params)):
        stale = [p for p in params if _SHADOW[id(p)][1] != p._version]
        if stale:
            with torch.no_grad():
                torch._foreach_copy_([_SHADOW[id(p)][2] for p in stale], [p.detach() for p in stale])
            for p in stale:
                ent = _SHADOW[id(p)]
                _SHADOW[id(p)] = (ent[0], p._version, ent[2])
        return hit[1], hit[2]
    import weakref
    with torch.no_grad():
        wc = torch.cat([w.detach().to(compute_dtype()) for w in weights], dim=0)
        bc = torch.cat([b.detach().to(compute_dtype()) for b in biases], dim=0)
    off = 0
    for w, b in zip(weights, biases):
        n = w.shape[0]
        _SHADOW[id(w)] = (weakref.ref(w), w._version, wc[off:off + n])
        _SHADOW[id(b)] = (weakref.ref(b), b._version, bc[off:off + n])
        off += n
    _CAT_CACHE[key] = ([weakref.ref(p) for p in params], wc, bc)
    return wc, bc


class _MultiLinearFn(torch.autograd.Function):
    """k linears over the SAME input evaluated as one GEMM (Q/K/V of self-attention, K/V of cross-attention):
    y[..., i, :] = x @ W_i^T + b_i.  One dX GEMM, one dW GEMM and one bias reduction in the backward; the
    per-layer gradients are row blocks (views) of the fused results."""

    @staticmethod
    def forward(ctx, x, tap_holder, *wb):
        k = len(wb) // 2
        weights, biases = wb[:k], wb[k:]
        wc, bc = _cat_shadow(weights, biases)
        ctx.k, ctx.x_dtype, ctx.x_shape = k, x.dtype, x.shape
        ctx.tap = tap_holder
        ctx.params = (weights, biases)
        if _native_ok(x, wc.shape[0], wc.shape[1]):
            from . import _ext
            x2 = _rows(x)
            y = _ext.gemm_fwd(x2, wc, bc)  # (bc is the bf16 concatenation of the k biases: bias_bf16 form)
            ctx.save_for_backward(x2, wc)
            return y.view(*x.shape[:-1], k, wc.shape[0] // k)
        xb = x if x.dtype == compute_dtype() else x.to(compute_dtype())
        y = F.linear(xb, wc, bc)
        ctx.save_for_backward(xb.reshape(-1, xb.shape[-1]), wc)
        return y.view(*y.shape[:-1], k, y.shape[-1] // k)

    @staticmethod
    def backward(ctx, g):
        x2, wc = ctx.saved_tensors
        k = ctx.k
        g2 = g.reshape(-1, g.shape[-2] * g.shape[-1])
        native = _native_dx_ok(g2, wc.shape[0], wc.shape[1])
        if g2.is_cuda and g2.dtype == torch.bfloat16:
            g2 = _rows(g2)
        elif not g2.is_contiguous():
            g2 = g2.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            extra = _take_tap(ctx.tap, g2)
            if native:
                from . import _ext
                dx = _ext.gemm_dx(g2, wc, add=extra, wt=_dx_wt(ctx.params[0], wc, g2.shape[0]))
            else:
                dx = torch.mm(g2, wc)
                if extra is not None:
                    dx = dx + extra
            dx = dx.view(ctx.x_shape).to(ctx.x_dtype)
        if _defer_ok(g2, x2):
            ws, bs = ctx.params
            _park(g2, x2, list(ws), list(bs))
            return (dx, None) + (None,) * (2 * k)
        dw, db = _dw_db(g2, x2, True, True)
        n = dw.shape[0] // k
        return (dx, None) + tuple(dw[i * n:(i + 1) * n] for i in range(k)) + tuple(db[i * n:(i + 1) * n] for i in range(k))


def multi_linear(x, linears, tap=None):
    """[lin_i(x)] stacked on a new second-to-last axis: (..., k, N).  Fused on the bf16 CUDA path.  tap: see mlp()."""
    ws, bs = [l.weight for l in linears], [l.bias for l in linears]
    if (compute_dtype() != torch.float32 and x.is_cuda and all(w.dtype == torch.float32 for w in ws)
            and all(b is not None for b in bs) and len({w.shape for w in ws}) == 1):
        return _MultiLinearFn.apply(x, tap, *ws, *bs)
    return torch.stack([linear(x, w, b, tap=(tap if i == 0 else None)) for i, (w, b) in enumerate(zip(ws, bs))], dim=-2)


class _AddTapFn(torch.autograd.Function):
    """fallback consumer of a GradTap for paths without a dX GEMM of their own: identity whose backward adds the parked
    gradient"""

    @staticmethod
    def forward(ctx, x, holder):
        ctx.holder = holder
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        h = ctx.holder
        h.consumed = True
        if h.grad is not None:
            g, h.grad = g + h.grad.to(g.dtype), None
        return g, None


def linear(x, weight, bias=None, act=None, tap=None):
    """y = act(x @ weight^T + bias); weight (out,in) as nn.Linear stores it.  Output in the compute dtype.
    tap: see mlp()."""
    if act not in (None, "gelu"):
        raise ValueError(act)
    if (compute_dtype() != torch.float32 and x.is_cuda and isinstance(weight, torch.nn.Parameter)
            and weight.dtype == torch.float32 and (bias is None or isinstance(bias, torch.nn.Parameter))):
        return _LinearFn.apply(x, weight, bias, act == "gelu", tap)
    if tap is not None and torch.is_tensor(x) and x.requires_grad and torch.is_grad_enabled():
        x = _AddTapFn.apply(x, tap)
    if weight.dim() > 2:
        weight = weight.reshape(weight.shape[0], -1)
    y = F.linear(_c(x), _c(weight), _c(bias) if bias is not None else None)
    if act == "gelu":
        y = F.gelu(y)  # exact (erf) GELU: vit.py act_layer=nn.GELU, med_config hidden_act "gelu"
    elif act is not None:
        raise ValueError(act)
    return y


def layer_norm(x, ln, residual=None):
    """LayerNorm(x [+ residual]) with fp32 statistics; output in the compute dtype."""
    if residual is None and _ln_kernel_ok(x, ln):
        return _DropAddLN.apply(x, None, ln.weight, ln.bias, ln.eps, 0.0, False)
    if residual is not None:
        x = x.float() + residual.float()
    y = F.layer_norm(x.float(), ln.normalized_shape, ln.weight, ln.bias, ln.eps)
    return _c(y)


def attention(q, k, v, mask, scale, return_probs=False, dropout_p=0.0):
    """softmax(q k^T * scale + mask) v.

    q (B,Lq,H,D), k/v (B,Lk,H,D) (any strides); mask None or additive fp32 broadcastable to
    (B,1,Lq,Lk).  Returns ctx (B,Lq,H,D) [compute dtype] and probs (B,H,Lq,Lk) fp32 or None.
    Order of operations follows med.py:179-217 (scores/sqrt(d) then + mask) and vit.py:75-83.
    """
    if compute_dtype() == torch.bfloat16 and _kernel_attention_ok(_c(q), _c(k), mask, return_probs):
        return _MaskedAttention.apply(_c(q), _c(k), _c(v), _mask_log2(mask, q.shape[0], k.shape[1]), scale,
                                      float(dropout_p)), None
    qh, kh, vh = _c(q).permute(0, 2, 1, 3), _c(k).permute(0, 2, 1, 3), _c(v).permute(0, 2, 1, 3)
    scores = torch.matmul(qh, kh.transpose(-1, -2)).float() * scale
    if mask is not None:
        scores = scores + mask
    probs = torch.softmax(scores, dim=-1)
    p = probs
    if dropout_p > 0.0:
        p = F.dropout(p, dropout_p, training=True)
    ctx = torch.matmul(p.to(vh.dtype), vh).permute(0, 2, 1, 3)
    return ctx, (probs if return_probs else None)


_STEP_SEED = {}
_CALL_SEED = [0]


def step_seed(device):
    """Device-resident step counter feeding the attention-dropout hash: bump it once per training step with
    new_step(); the increment is an ordinary kernel, so a replayed HIP graph draws fresh masks every replay."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _STEP_SEED:
        _STEP_SEED[key] = torch.full((1,), torch.initial_seed() & 0x7FFFFFFF, dtype=torch.int32, device=device)
    return _STEP_SEED[key]


def new_step(device):
    step_seed(device).add_(1)
    _CALL_SEED[0] = 0


def reset_seeds(seed, device=None):
    """the counters behind every dropout / drop-path mask of the HIP path back to the state a process seeded with `seed` starts
    in: the step counter of every device (and of `device`, created if it has none yet) filled in place, the call counter 0
    (bridgeqa_amd.manual_seed)"""
    v = int(seed) & 0x7FFFFFFF
    for t in _STEP_SEED.values():
        t.fill_(v)
    if device is not None:
        step_seed(torch.device(device)).fill_(v)
    _CALL_SEED[0] = 0


def set_deterministic(flag):
    """bridgeqa_amd.set_deterministic"""
    from . import set_deterministic as _set
    return _set(flag)


def is_deterministic():
    """bridgeqa_amd.is_deterministic"""
    from . import is_deterministic as _is
    return _is()


class _MaskedAttention(torch.autograd.Function):
    """softmax(q k^T * scale + key_mask) v with dropout on the probabilities, through csrc/attn.hip;
    q (B,Lq,H,64), k/v (B,Lk,H,64) bf16 (any strides with a contiguous head dim)."""

    @staticmethod
    def forward(ctx, q, k, v, mask_log2, scale, p_drop):
        from . import _ext
        _CALL_SEED[0] += 1
        seed, st = _CALL_SEED[0] * 7919, (step_seed(q.device) if p_drop > 0 else None)
        out, lse = _ext.attn_fwd(q, k, v, scale, mask_log2, p_drop, seed, st)
        ctx.save_for_backward(q, k, v, out, lse, mask_log2 if mask_log2 is not None else q.new_empty(0), 
                              st if st is not None else q.new_empty(0))
        ctx.cfg = (scale, p_drop, seed, mask_log2 is not None, st is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import _ext
        q, k, v, out, lse, mask_log2, st = ctx.saved_tensors
        scale, p_drop, seed, has_mask, has_st = ctx.cfg
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dkv = torch.empty((2,) + tuple(k.shape), dtype=k.dtype, device=k.device)
        kc, vc = (k, v) if k.stride() == v.stride() else (k.contiguous(), v.contiguous())
        if kc.stride() != dkv[0].stride():
            kc, vc = kc.contiguous(), vc.contiguous()
        qc = q if q.stride() == dq.stride() else q.contiguous()
        _ext.attn_bwd(qc, kc, vc, out, lse, grad_out, scale, dq, dkv[0], dkv[1], mask_log2 if has_mask else None,
                      p_drop, seed, st if has_st else None)
        return dq, dkv[0], dkv[1], None, None, None


_LN_BWD_FROM_SUM = [True]   # the backward of a dropout-free add + LayerNorm site reads its stored sum (bq_drop_add_ln_bwd_sum)


class _DropAddLN(torch.autograd.Function):
    """y = LayerNorm(dropout(x) + residual) in one kernel each way (csrc/ln.hip).  residual may be None (plain
    LayerNorm); with want_sum the bf16 sum dropout(x) + residual is a second output (the residual stream a pre-LN
    block carries on), and its gradient is folded into the same backward launch."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, p_drop, want_sum, p_path=0.0):
        from . import _ext
        _CALL_SEED[0] += 1
        seed, st = _CALL_SEED[0] * 104729, (step_seed(x.device) if (p_drop > 0 or p_path > 0) else None)
        rps = x.shape[-2] if x.dim() >= 3 else 1  # stochastic depth drops whole samples (B, L, H)
        need_grad = any(ctx.needs_input_grad[:4])
        y, s, mean, rstd, dgb = _ext.drop_add_ln_fwd(x, residual, weight, bias, eps, p_drop, seed, st, want_sum, p_path,
                                                     rps, need_grad)
        # a dropout-free site that wrote its sum (the ViT's residual update): the backward re-forms the normalised row from
        # that ONE stored tensor instead of from x and residual (round 6: 150 -> 125 / 100 MB per site at the ViT shape, and
        # neither x nor residual is kept alive for it)
        ctx.from_sum = bool(_LN_BWD_FROM_SUM[0] and want_sum and p_drop == 0.0 and residual is not None and s is not None)
        if ctx.from_sum:
            ctx.save_for_backward(s, x.new_empty(0), weight, mean, rstd, st if st is not None else x.new_empty(0))
        else:
            ctx.save_for_backward(x, residual if residual is not None else x.new_empty(0), weight, mean, rstd,
                                  st if st is not None else x.new_empty(0))
        ctx.cfg = (eps, p_drop, seed, st is not None, residual is not None, p_path, rps)
        ctx.dgb = dgb  # dgamma / dbeta accumulator, zeroed by the forward launch; consumed by the first backward
        if want_sum:
            return y, s
        return y

    @staticmethod
    def backward(ctx, dy, dsum=None):
        from . import _ext
        x, residual, weight, mean, rstd, st = ctx.saved_tensors
        eps, p_drop, seed, has_st, has_res, p_path, rps = ctx.cfg
        if dsum is not None and not dsum.is_contiguous():
            dsum = dsum.contiguous()
        dgb, ctx.dgb = ctx.dgb, None
        if ctx.from_sum:
            dx, dres, dg, db = _ext.drop_add_ln_bwd_sum(x, weight, dy.contiguous(), mean, rstd, eps, seed,
                                                        st if has_st else None, dsum, p_path, rps, dgb)
            return dx, dres, dg, db, None, None, None, None
        dx, dres, dg, db = _ext.drop_add_ln_bwd(x, residual if has_res else None, weight, dy.contiguous(), mean, rstd,
                                                eps, p_drop, seed, st if has_st else None, dsum, p_path, rps, dgb)
        return dx, dres, dg, db, None, None, None, None


def _ln_kernel_ok(x, ln):
    return (compute_dtype() == torch.bfloat16 and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 256 == 0
            and x.shape[-1] <= 1024 and x.is_contiguous() and ln.weight.dtype == torch.float32
            and tuple(ln.normalized_shape) == (x.shape[-1],))


def dropout_add_layer_norm(x, residual, ln, p_drop, training):
    """LayerNorm(dropout(x) + residual): BertSelfOutput / BertOutput tail (med.py:236-239, 313-317)."""
    p = float(p_drop) if training else 0.0
    if _ln_kernel_ok(x, ln) and residual.dtype == torch.bfloat16 and residual.is_contiguous():
        return _DropAddLN.apply(x, residual, ln.weight, ln.bias, ln.eps, p, False)
    h = F.dropout(x, p, training=True) if p > 0 else x
    return layer_norm(h, ln, residual=residual)


def add_layer_norm(x, residual, ln, drop_path=0.0):
    """(s, LayerNorm(s)) with s = drop_path(x) + residual: the residual update of one pre-LN sub-block fused with
    the next sub-block's norm (vit.py:106-109 `x = x + drop_path(f(norm(x)))` followed by the next `norm(x)`).
    drop_path = per-sample stochastic depth probability (0 in eval)."""
    if _ln_kernel_ok(x, ln) and residual.dtype == torch.bfloat16 and residual.is_contiguous():
        y, s = _DropAddLN.apply(x, residual, ln.weight, ln.bias, ln.eps, 0.0, True, float(drop_path))
        return s, y
    if drop_path > 0.0:
        keep = 1.0 - drop_path
        x = x.div(keep) * x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
    s = x + residual
    return s, layer_norm(s, ln)


_MASK_CACHE = {}


def _mask_log2(mask, B, Lk):
    """kernel-format key mask, converted once per mask tensor (the same extended mask serves all 12 layers)"""
    if mask is None:
        return None
    import weakref
    hit = _MASK_CACHE.get(id(mask))
    if hit is not None and hit[0]() is mask and hit[1] == mask._version:
        return hit[2]
    from . import _ext
    if len(_MASK_CACHE) > 64:
        _MASK_CACHE.clear()
    m = _ext.key_mask_log2(mask, B, Lk)
    _MASK_CACHE[id(mask)] = (weakref.ref(mask), mask._version, m)
    return m


def prime_masks(*masks):
    """Convert key masks to kernel format NOW, on the current stream.  Called before any fork so that side
    streams (which wait for the current stream when they fork) never see a half-written cached mask."""
    if compute_dtype() != torch.bfloat16:
        return
    for m in masks:
        if m is not None and m.is_cuda and m.dim() == 4 and m.shape[1] == 1 and m.shape[2] == 1:
            _mask_log2(m, m.shape[0], m.shape[3])


def _kernel_attention_ok(q, k, mask, return_probs):
    if return_probs or not q.is_cuda or q.dtype != torch.bfloat16 or q.shape[-1] != 64:
        return False
    if q.stride(-1) != 1 or k.stride(-1) != 1:
        return False
    return mask is None or (mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1)


def _seed_args(p_drop, device):
    _CALL_SEED[0] += 1
    return _CALL_SEED[0] * 7919, (step_seed(device) if p_drop > 0 else None)


class _PackedAttention(torch.autograd.Function):
    """softmax(q k^T * scale + key_mask) v on a fused-QKV tensor (B, L, 3, H, 64) through the MFMA kernels of
    csrc/attn.hip: no (L x L) tensor in HBM, forward or backward; the gradient comes back packed the same
    way, so the QKV projection's backward needs no concat."""

    @staticmethod
    def forward(ctx, qkv, scale, mask_log2, p_drop, causal=False, want_probs=False):
        from . import _ext
        seed, st = _seed_args(p_drop, qkv.device)
        out, lse = _ext.attn_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], scale, mask_log2, p_drop, seed, st, causal)
        ctx.save_for_backward(qkv, out, lse, mask_log2 if mask_log2 is not None else qkv.new_empty(0),
                              st if st is not None else qkv.new_empty(0))
        ctx.cfg = (scale, p_drop, seed, mask_log2 is not None, st is not None, causal)
        if want_probs:  # the softmax map BEFORE dropout (what med.py:202,223 returns), rebuilt from the LSE; DETACHED
            probs = _ext.attn_probs(qkv[:, :, 0], qkv[:, :, 1], lse, scale, mask_log2, causal=causal)
            ctx.mark_non_differentiable(probs)
            return out, probs
        return out

    @staticmethod
    def backward(ctx, grad_out, _gp=None):
        from . import _ext
        qkv, out, lse, mask_log2, st = ctx.saved_tensors
        scale, p_drop, seed, has_mask, has_st, causal = ctx.cfg
        dqkv = torch.empty_like(qkv)
        _ext.attn_bwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], out, lse, grad_out.contiguous(), scale,
                      dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], mask_log2 if has_mask else None, p_drop, seed,
                      st if has_st else None, causal)
        return dqkv, None, None, None, None, None


class _QKVAttention(torch.autograd.Function):
    """Cross-attention with q (B, Lq, H, 64) and a fused K/V tensor kv (B, Lk, 2, H, 64); dkv comes back packed."""

    @staticmethod
    def forward(ctx, q, kv, scale, mask_log2, p_drop, want_probs=False, sink=None):
        from . import _ext
        seed, st = _seed_args(p_drop, q.device)
        out, lse = _ext.attn_fwd(q, kv[:, :, 0], kv[:, :, 1], scale, mask_log2, p_drop, seed, st)
        ctx.save_for_backward(q, kv, out, lse, mask_log2 if mask_log2 is not None else q.new_empty(0),
                              st if st is not None else q.new_empty(0))
        ctx.cfg = (scale, p_drop, seed, mask_log2 is not None, st is not None, sink)
        if want_probs:
            probs = _ext.attn_probs(q, kv[:, :, 0], lse, scale, mask_log2)
            ctx.mark_non_differentiable(probs)
            return out, probs
        return out

    @staticmethod
    def backward(ctx, grad_out, _gp=None):
        from . import _ext
        q, kv, out, lse, mask_log2, st = ctx.saved_tensors
        scale, p_drop, seed, has_mask, has_st, sink = ctx.cfg
        qc = q if q.is_contiguous() else q.contiguous()
        dq = torch.empty_like(qc)
        # sink = (HoistedKV, slot): kv is this layer's column block of a hoisted projection and so is its gradient
        dkv = sink[0].grad_view(sink[1], kv) if sink is not None else torch.empty_like(kv)
        _ext.attn_bwd(qc, kv[:, :, 0], kv[:, :, 1], out, lse, grad_out.contiguous(), scale, dq, dkv[:, :, 0], dkv[:, :, 1],
                      mask_log2 if has_mask else None, p_drop, seed, st if has_st else None)
        if sink is not None:
            sink[0].push_dx(sink[1])
        return dq, dkv, None, None, None, None, None


# ---- the two text streams of the twin encoder as ONE batch ---------------------------------------------------------
# The twin encoder (reference med.py:549-614) runs two BertLayers per level -- `layer[i]` on the 2D stream, `layer_twin[i]`
# on the 3D stream -- that only exchange their PREVIOUS states.  Same shapes, different weights: every projection of a
# level is one grouped GEMM launch with one problem per stream (csrc/gemm.hip takes a problem list), every add +
# LayerNorm one launch over two row groups with their own gamma / beta (csrc/ln.hip), the self-attention one launch over
# the stacked batch.  The states travel stacked, (2B, L, D): rows [0, B) = 2D stream, [B, 2B) = 3D stream.

def _param_ok(*ps):
    return all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 for p in ps)


def _group_operands(ws, bs, G, k):
    """per group: the bf16 weight operand ((k N, K): the k linears' shadows are row blocks of one buffer) and its bias"""
    wops, bops = [], []
    for g in range(G):
        wg, bg = ws[g * k:(g + 1) * k], bs[g * k:(g + 1) * k]
        if k > 1:
            wc, bc = _cat_shadow(wg, bg)
        else:
            wc, bc = _shadow(wg[0]), _f32_bias(bg[0])
        wops.append(wc)
        bops.append(bc)
    return wops, bops


def _grouped_wgrad(g2s, x2s, ws, bs, k):
    """weight / bias gradients of G groups of k fused linears: parked inside a deferred scope (-> Nones), else now"""
    G = len(g2s)
    if all(_defer_ok(g2, x2) for g2, x2 in zip(g2s, x2s)):
        for g in range(G):
            _park(g2s[g], x2s[g], list(ws[g * k:(g + 1) * k]), list(bs[g * k:(g + 1) * k]))
        return (None,) * (2 * G * k)
    dws, dbs = [], []
    for g in range(G):
        dw, db = _dw_db(g2s[g], x2s[g], True, True)
        n = dw.shape[0] // k
        dws += [dw[j * n:(j + 1) * n] for j in range(k)]
        dbs += [db[j * n:(j + 1) * n] for j in range(k)]
    return tuple(dws) + tuple(dbs)


class _GroupedLinearFn(torch.autograd.Function):
    """G groups x k linears in ONE GEMM launch: group g applies its k linears (fused: one (k N, K) operand) to its own
    rows.  stacked: ONE input whose rows are G equal blocks and one output laid out the same way ((rows, k N)); else G
    inputs (any row counts: the image-side and the object-side K/V projections) and G outputs.  Backward: one grouped
    dX launch; dW / db parked per group for the phase's grouped launches."""

    @staticmethod
    def forward(ctx, G, k, stacked, tap_holder, *t):
        from . import _ext
        ctx.tap = tap_holder  # (stacked form only) the residual-branch gradient of the input, added by the dX launch
        nx = 1 if stacked else G
        xs, ws, bs = t[:nx], t[nx:nx + G * k], t[nx + G * k:]
        wops, bops = _group_operands(ws, bs, G, k)
        N = wops[0].shape[0]
        dev = xs[0].device
        if stacked:
            x2 = _rows(xs[0])
            M = x2.shape[0] // G
            xg = [x2[g * M:(g + 1) * M] for g in range(G)]
            y = torch.empty(x2.shape[0], N, dtype=torch.bfloat16, device=dev)
            yg = [y[g * M:(g + 1) * M] for g in range(G)]
            outs = (y.view(*xs[0].shape[:-1], N),)
        else:
            xg = [_rows(x) for x in xs]
            yg = [torch.empty(x2.shape[0], N, dtype=torch.bfloat16, device=dev) for x2 in xg]
            outs = tuple(y.view(*x.shape[:-1], N) for y, x in zip(yg, xs))
        _ext.gemm_grouped([dict(P=w, Q=x2, out=o, bias=b) for w, x2, o, b in zip(wops, xg, yg, bops)], 0, _ext.EPI_BIAS)
        ctx.save_for_backward(*xg, *wops)
        ctx.cfg = (G, k, stacked, [x.shape for x in xs], [x.dtype for x in xs])
        ctx.params = (ws, bs)
        return outs[0] if stacked else outs

    @staticmethod
    def backward(ctx, *grads):
        from . import _ext
        G, k, stacked, shapes, dtypes = ctx.cfg
        xg, wops = ctx.saved_tensors[:G], ctx.saved_tensors[G:]
        ws, bs = ctx.params
        N, K = wops[0].shape
        if stacked:
            g2 = _rows(grads[0].reshape(-1, N))
            M = g2.shape[0] // G
            gg = [g2[g * M:(g + 1) * M] for g in range(G)]
            dx = torch.empty(g2.shape[0], K, dtype=torch.bfloat16, device=g2.device)
            dxg = [dx[g * M:(g + 1) * M] for g in range(G)]
        else:
            gg = [_rows(g.reshape(-1, N)) for g in grads]
            dxg = [torch.empty(g2.shape[0], K, dtype=torch.bfloat16, device=g2.device) for g2 in gg]
        need = [i for i in range(1 if stacked else G) if ctx.needs_input_grad[4 + i]]
        if need:
            sel = range(G) if stacked else need
            extra = _take_tap(ctx.tap, g2) if stacked else None
            pops, pflag = _dx_operands([ws[g * k:(g + 1) * k] for g in range(G)], wops, [gg[g].shape[0] for g in sel])
            if extra is not None:
                _ext.gemm_grouped([dict(P=pops[g], Q=gg[g], out=dxg[g], aux=extra[g * M:(g + 1) * M]) for g in sel],
                                  pflag, _ext.EPI_ADD)
            else:
                _ext.gemm_grouped([dict(P=pops[g], Q=gg[g], out=dxg[g]) for g in sel], pflag, _ext.EPI_NONE)
        if stacked:
            dxs = (dx.view(shapes[0]).to(dtypes[0]) if need else None,)
        else:
            dxs = tuple(dxg[g].view(shapes[g]).to(dtypes[g]) if g in need else None for g in range(G))
        return (None, None, None, None) + dxs + _grouped_wgrad(gg, xg, ws, bs, k)


class _GroupedMlpFn(torch.autograd.Function):
    """fc2(gelu(fc1(x))) of G streams stacked along the rows, each with its own (fc1, fc2): the fused node of _MlpFn with
    every launch grouped -- forward 2 launches (GELU epilogue, bias epilogue), backward 2 (dGELU epilogue, plain) + parks."""

    @staticmethod
    def forward(ctx, G, tap_holder, x, *p):
        from . import _ext
        ctx.tap = tap_holder
        w1, b1, w2, b2 = p[0::4], p[1::4], p[2::4], p[3::4]
        w1o, w2o = [_shadow(w) for w in w1], [_shadow(w) for w in w2]
        x2 = _rows(x)
        M = x2.shape[0] // G
        I, D = w1o[0].shape[0], w2o[0].shape[0]
        y1 = torch.empty(x2.shape[0], I, dtype=torch.bfloat16, device=x.device)
        h = torch.empty_like(y1)
        y2 = torch.empty(x2.shape[0], D, dtype=torch.bfloat16, device=x.device)
        rows = lambda t, g: t[g * M:(g + 1) * M]
        _ext.gemm_grouped([dict(P=w1o[g], Q=rows(x2, g), out=rows(y1, g), out2=rows(h, g), bias=_f32_bias(b1[g]))
                           for g in range(G)], 0, _ext.EPI_BIAS_GELU)
        _ext.gemm_grouped([dict(P=w2o[g], Q=rows(h, g), out=rows(y2, g), bias=_f32_bias(b2[g])) for g in range(G)], 0,
                          _ext.EPI_BIAS)
        ctx.save_for_backward(x2, y1, h, *w1o, *w2o)
        ctx.params, ctx.G = (w1, b1, w2, b2), G
        ctx.x_dtype, ctx.x_shape = x.dtype, x.shape
        return y2.view(*x.shape[:-1], D)

    @staticmethod
    def backward(ctx, g):
        from . import _ext
        G = ctx.G
        x2, y1, h = ctx.saved_tensors[:3]
        w1o, w2o = ctx.saved_tensors[3:3 + G], ctx.saved_tensors[3 + G:]
        w1, b1, w2, b2 = ctx.params
        g2 = _rows(g.reshape(-1, g.shape[-1]))
        M = g2.shape[0] // G
        rows = lambda t, i: t[i * M:(i + 1) * M]
        dy1 = torch.empty_like(y1)
        p2, f2 = _dx_operands([(w,) for w in w2], w2o, [M] * G)
        _ext.gemm_grouped([dict(P=p2[i], Q=rows(g2, i), out=rows(dy1, i), aux=rows(y1, i)) for i in range(G)],
                          f2, _ext.EPI_DGELU)
        dx = None
        if ctx.needs_input_grad[2]:
            dx = torch.empty_like(x2)
            extra = _take_tap(ctx.tap, dy1)
            p1, f1 = _dx_operands([(w,) for w in w1], w1o, [M] * G)
            if extra is not None:
                _ext.gemm_grouped([dict(P=p1[i], Q=rows(dy1, i), out=rows(dx, i), aux=rows(extra, i)) for i in range(G)],
                                  f1, _ext.EPI_ADD)
            else:
                _ext.gemm_grouped([dict(P=p1[i], Q=rows(dy1, i), out=rows(dx, i)) for i in range(G)], f1, _ext.EPI_NONE)
            dx = dx.view(ctx.x_shape).to(ctx.x_dtype)
        gw2 = _grouped_wgrad([rows(g2, i) for i in range(G)], [rows(h, i) for i in range(G)], w2, b2, 1)
        gw1 = _grouped_wgrad([rows(dy1, i) for i in range(G)], [rows(x2, i) for i in range(G)], w1, b1, 1)
        out = []
        for i in range(G):
            out += [gw1[i], gw1[G + i], gw2[i], gw2[G + i]]
        return (None, None, dx) + tuple(out)


class _TwinDropAddLN(torch.autograd.Function):
    """LayerNorm_g(dropout(x) + residual) for the two row groups g of a stacked (2B, L, H) tensor, each with its own
    gamma / beta -- one launch each way (csrc/ln.hip, blockIdx.y = group)."""

    @staticmethod
    def forward(ctx, x, residual, wa, ba, wb, bb, eps, p_drop):
        from . import _ext
        _CALL_SEED[0] += 1
        seed, st = _CALL_SEED[0] * 104729, (step_seed(x.device) if p_drop > 0 else None)
        y, mean, rstd, dgb = _ext.twin_drop_add_ln_fwd(x, residual, wa, ba, wb, bb, eps, p_drop, seed, st,
                                                       any(ctx.needs_input_grad[:6]))
        ctx.save_for_backward(x, residual, wa, wb, mean, rstd, st if st is not None else x.new_empty(0))
        ctx.cfg = (eps, p_drop, seed, st is not None)
        ctx.dgb = dgb
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import _ext
        x, residual, wa, wb, mean, rstd, st = ctx.saved_tensors
        eps, p_drop, seed, has_st = ctx.cfg
        dgb, ctx.dgb = ctx.dgb, None
        dx, dres, dgb = _ext.twin_drop_add_ln_bwd(x, residual, wa, wb, dy.contiguous(), mean, rstd, eps, p_drop, seed,
                                                  st if has_st else None, dgb)
        return dx, dres, dgb[0, 0], dgb[0, 1], dgb[1, 0], dgb[1, 1], None, None


class _TwinMixFn(torch.autograd.Function):
    """keys / values source of the two cross-attentions of one twin level from the stacked states hs (2B, L, D):
    mix2d = cat(image tokens, 3D-stream states), mix3d = cat(object tokens, 2D-stream states) (reference med.py:549-562);
    the backward hands the states' gradient back STACKED (one cat) instead of two zero-filled slice gradients.
    (The torch composition: CPU / fp32 runs.  On the bf16 kernel path nothing is concatenated: _TwinKVFn.)"""

    @staticmethod
    def forward(ctx, enc2d, enc3d, hs):
        B = hs.shape[0] // 2
        ctx.cfg = (enc2d.shape[1], enc3d.shape[1])
        return torch.cat((enc2d, hs[B:]), dim=1), torch.cat((enc3d, hs[:B]), dim=1)

    @staticmethod
    def backward(ctx, g2d, g3d):
        P2, P3 = ctx.cfg
        return g2d[:, :P2], g3d[:, :P3], torch.cat((g3d[:, P3:], g2d[:, P2:]), dim=0)


class GradSink(object):
    """In-place accumulator for the gradient of ONE tensor that many nodes read (the image tokens / object tokens under the
    12 twin levels): every reader adds its share in the epilogue of its dX GEMM (out = acc + out) and returns nothing to
    autograd; the reader whose backward runs LAST hands the buffer over as the tensor's gradient.  `readers` counts the
    nodes created in the forward; a reader that never runs its backward would hold the gradient back -- twin levels
    always do (they form a chain)."""
    __slots__ = ("buf", "readers")

    def __init__(self):
        self.buf, self.readers = None, 0

    def opened(self):
        """called by the reader that allocates the buffer in a backward pass: at the END of that pass the buffer must have
        been handed over.  It is not when some reader never ran -- a loss on an intermediate level only
        (output_hidden_states), or a second backward over a retained graph --: the fixed tokens' gradient would silently be
        None (the reference's cat-based autograd has no such failure mode), so fail loudly instead."""
        def check():
            if self.buf is not None:
                n, self.buf, self.readers = self.readers, None, 0
                raise RuntimeError("GradSink: the backward pass ended with %d twin level(s) that never ran their backward; the "
                                   "image / object tokens' gradient would be lost.  The concatenation-free K/V node assumes ONE "
                                   "backward through ALL twin levels (no loss on intermediate levels only, no retain_graph "
                                   "re-runs): set fusion_ops._TWIN_KV[0] = False for such uses." % n)
        torch.autograd.Variable._execution_engine.queue_callback(check)


class _TwinKVFn(torch.autograd.Function):
    """Key / value projections of the two cross-attentions of one twin level WITHOUT the concatenations (reference
    med.py:549-562: layer[i] attends to cat(image tokens, 3D-stream states), layer_twin[i] to cat(object tokens, 2D-stream
    states); med.py:112-118 the projections).  One grouped GEMM of four problems writes each source's rows into its row
    range of the (B, P + L, 2 D) key/value tensor of its stream (batched-row output map, bq_gemm_desc.o_rpb); the backward
    reads its row range of the gradient in place (q_rpb): the fixed tokens' share is ADDED into the GradSink of enc2d /
    enc3d by the dX epilogue, the states' share comes back stacked with the gradient that reached the states through the
    level's other readers (tap) already added; the weight gradient has two row sources (fusion_wgrad._park_two).
    No cat, no strided slice gradients, no accumulation kernels (12 + 46 + 27 launches per c3 step)."""

    @staticmethod
    def forward(ctx, enc2d, enc3d, hs, sink2d, sink3d, tap_holder, *wb):
        from . import _ext
        ws, bs = wb[:4], wb[4:]
        wops, bops = _group_operands(ws, bs, 2, 2)
        B, L, D = hs.shape[0] // 2, hs.shape[1], hs.shape[2]
        P2, P3, N2 = enc2d.shape[1], enc3d.shape[1], wops[0].shape[0]
        kv2d = torch.empty(B, P2 + L, N2, dtype=torch.bfloat16, device=hs.device)
        kv3d = torch.empty(B, P3 + L, N2, dtype=torch.bfloat16, device=hs.device)
        _ext.gemm_grouped([dict(P=wops[0], Q=enc2d.view(B * P2, D), out=kv2d[:, :P2], bias=bops[0]),
                           dict(P=wops[1], Q=enc3d.view(B * P3, D), out=kv3d[:, :P3], bias=bops[1]),
                           dict(P=wops[0], Q=hs[B:].view(B * L, D), out=kv2d[:, P2:], bias=bops[0]),
                           dict(P=wops[1], Q=hs[:B].view(B * L, D), out=kv3d[:, P3:], bias=bops[1])], 0, _ext.EPI_BIAS)
        ctx.save_for_backward(enc2d, enc3d, hs, *wops)
        ctx.sinks, ctx.tap, ctx.params = (sink2d, sink3d), tap_holder, (ws, bs)
        sink2d.readers += 1
        sink3d.readers += 1
        return kv2d, kv3d

    @staticmethod
    def backward(ctx, g2d, g3d):
        from . import _ext
        enc2d, enc3d, hs, w2d, w3d = ctx.saved_tensors
        ws, bs = ctx.params
        B, L, D = hs.shape[0] // 2, hs.shape[1], hs.shape[2]
        P2, P3 = enc2d.shape[1], enc3d.shape[1]
        g2d, g3d = g2d.contiguous(), g3d.contiguous()
        outs = []
        for sink, enc in zip(ctx.sinks, (enc2d, enc3d)):
            if sink.readers <= 0:
                raise RuntimeError("GradSink: a twin level's backward ran a second time (retain_graph re-run?): the "
                                   "concatenation-free K/V node supports one backward per forward "
                                   "(fusion_ops._TWIN_KV[0] = False restores the cat-based composition)")
            if sink.buf is None:
                sink.buf = torch.zeros(enc.shape[0] * enc.shape[1], D, dtype=torch.bfloat16, device=hs.device)
                sink.opened()
            outs.append(sink.buf)
        dhs = torch.empty(2 * B * L, D, dtype=torch.bfloat16, device=hs.device)
        extra = _take_tap(ctx.tap, dhs)   # the states' gradient through the level's other readers, stacked rows
        if extra is None:
            extra = torch.zeros_like(dhs)
        (p2d, p3d), pflag = _dx_operands([ws[0:2], ws[2:4]], [w2d, w3d], [B * max(P2, P3)])
        _ext.gemm_grouped([dict(P=p2d, Q=g2d[:, :P2], out=outs[0], aux=outs[0]),
                           dict(P=p3d, Q=g3d[:, :P3], out=outs[1], aux=outs[1]),
                           dict(P=p2d, Q=g2d[:, P2:], out=dhs[B * L:], aux=extra[B * L:]),
                           dict(P=p3d, Q=g3d[:, P3:], out=dhs[:B * L], aux=extra[:B * L])], pflag, _ext.EPI_ADD)
        hs2 = hs.view(2 * B * L, D)
        src = ((g2d[:, :P2], enc2d.view(B * P2, D), g2d[:, P2:], hs2[B * L:]),
               (g3d[:, :P3], enc3d.view(B * P3, D), g3d[:, P3:], hs2[:B * L]))
        if _DEFER[0] is not None:
            for g, (ga, xa, gb, xb) in enumerate(src):
                _park_two(ga, xa, gb, xb, list(ws[2 * g:2 * g + 2]), list(bs[2 * g:2 * g + 2]))
            gw = (None,) * 8
        else:
            dws, dbs = [], []
            for g, (ga, xa, gb, xb) in enumerate(src):
                dw = torch.empty(ga.shape[-1], D, dtype=torch.float32, device=hs.device)
                db = torch.empty(ga.shape[-1], dtype=torch.float32, device=hs.device)
                f = _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32
                _ext.gemm_grouped([dict(P=xa, Q=ga, out=dw, colsum=db)], f, _ext.EPI_NONE,
                                  256 if (wgrad_class(B * ga.shape[1]) == "big" and ga.shape[1] >= 64) else 64)
                # (accum: ONE adder per element onto what the launch above stored on this stream -- bitwise reproducible as
                # it is, also in the deterministic mode, which runs it with plain loads and stores)
                _ext.gemm_grouped([dict(P=xb, Q=gb, out=dw, colsum=db, accum=True)], f, _ext.EPI_NONE, 64)
                n = dw.shape[0] // 2
                dws += [dw[:n], dw[n:]]
                dbs += [db[:n], db[n:]]
            gw = tuple(dws) + tuple(dbs)
        grads = []
        for sink in ctx.sinks:   # the last reader to run hands the accumulated gradient over
            sink.readers -= 1
            grads.append(None)
            if sink.readers == 0:
                grads[-1], sink.buf = sink.buf, None
        d2d = grads[0].view(enc2d.shape) if grads[0] is not None else None
        d3d = grads[1].view(enc3d.shape) if grads[1] is not None else None
        return (d2d, d3d, dhs.view(hs.shape), None, None, None) + gw


_TWIN_KV = [True]   # (tools/ab_bench.py flips it to time the concatenating composition inside the whole step)


def twin_kv_ok(enc2d, enc3d, hs):
    """the concatenation-free K/V node needs the kernel formats (bf16, CUDA, contiguous, widths the GEMM family takes) and
    segments the batched-row maps can address"""
    ok = lambda t: t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()
    return (_TWIN_KV[0] and compute_dtype() == torch.bfloat16 and _NATIVE_GEMM[0] and ok(enc2d) and ok(enc3d) and ok(hs)
            and hs.shape[-1] % 64 == 0 and max(enc2d.shape[1], enc3d.shape[1], hs.shape[1]) <= 65535)


def twin_kv(enc2d, enc3d, hs, lins_a, lins_b, sink2d, sink3d, tap=None):
    """-> kv2d (B, P2 + L, 2, D), kv3d (B, P3 + L, 2, D): [key; value] of stream a over (enc2d, 3D-stream states) and of
    stream b over (enc3d, 2D-stream states); lins_* = (key, value) linears; tap: a GradTap whose tap(hs, .) feeds the
    level's other readers of hs"""
    ws = [l.weight for l in lins_a] + [l.weight for l in lins_b]
    bs = [l.bias for l in lins_a] + [l.bias for l in lins_b]
    ya, yb = _TwinKVFn.apply(enc2d, enc3d, hs, sink2d, sink3d, tap, *ws, *bs)
    return ya.view(*ya.shape[:-1], 2, ya.shape[-1] // 2), yb.view(*yb.shape[:-1], 2, yb.shape[-1] // 2)


class _TwinSplitFn(torch.autograd.Function):
    """stacked (2B, ...) -> the two streams' states; backward = one cat"""

    @staticmethod
    def forward(ctx, hs):
        B = hs.shape[0] // 2
        return hs[:B].clone(), hs[B:].clone()

    @staticmethod
    def backward(ctx, ga, gb):
        return torch.cat((ga, gb), dim=0)


_ATTN_PAIR = [True]


class _TwinCrossAttention(torch.autograd.Function):
    """the two cross-attentions of one twin level: queries stacked (2B, L, H, 64), keys / values per stream as fused
    K/V tensors (B, Lk_g, 2, H, 64) of different lengths; context and dq come back stacked (no slice gradients)"""

    @staticmethod
    def forward(ctx, q, kva, kvb, scale, ma, mb, p_drop, want_probs=False):
        from . import _ext
        B = q.shape[0] // 2
        out = torch.empty_like(q)
        seeds, lses, probs = [], [], []
        pair = _ATTN_PAIR[0] and _ext.attn_pair_ok(q[:B], kva, q[B:], kvb)
        if pair:  # both cross-attentions in one launch: the 276-key one runs under the 1045-key one
            sides = []
            for g, (kv, m) in enumerate(((kva, ma), (kvb, mb))):
                seed, st = _seed_args(p_drop, q.device)
                seeds.append(seed)
                sides.append(dict(q=q[g * B:(g + 1) * B], k=kv[:, :, 0], v=kv[:, :, 1], out=out[g * B:(g + 1) * B],
                                  mask_log2=m, seed=seed))
            lses = _ext.attn_fwd_pair(sides, scale, p_drop, st)
        for g, (kv, m) in enumerate(((kva, ma), (kvb, mb))):
            if not pair:
                seed, st = _seed_args(p_drop, q.device)
                _, lse = _ext.attn_fwd(q[g * B:(g + 1) * B], kv[:, :, 0], kv[:, :, 1], scale, m, p_drop, seed, st,
                                       out=out[g * B:(g + 1) * B])
                seeds.append(seed)
                lses.append(lse)
            if want_probs:
                probs.append(_ext.attn_probs(q[g * B:(g + 1) * B], kv[:, :, 0], lses[g], scale, m))
        e = q.new_empty(0)
        ctx.save_for_backward(q, kva, kvb, out, lses[0], lses[1], ma if ma is not None else e, mb if mb is not None else e,
                              st if st is not None else e)
        ctx.cfg = (scale, p_drop, seeds, ma is not None, mb is not None, st is not None, pair)
        if want_probs:
            ctx.mark_non_differentiable(*probs)
            return out, probs[0], probs[1]
        return out

    @staticmethod
    def backward(ctx, grad_out, _ga=None, _gb=None):
        from . import _ext
        q, kva, kvb, out, lsa, lsb, ma, mb, st = ctx.saved_tensors
        scale, p_drop, seeds, has_a, has_b, has_st, pair = ctx.cfg
        B = q.shape[0] // 2
        grad_out = grad_out.contiguous()
        dq = torch.empty_like(q)
        dkvs, sides = [], []
        for g, (kv, lse, m, has) in enumerate(((kva, lsa, ma, has_a), (kvb, lsb, mb, has_b))):
            dkv = torch.empty_like(kv)
            r = slice(g * B, (g + 1) * B)
            if pair:
                sides.append(dict(q=q[r], k=kv[:, :, 0], v=kv[:, :, 1], out=out[r], lse=lse, grad_out=grad_out[r], dq=dq[r],
                                  dk=dkv[:, :, 0], dv=dkv[:, :, 1], mask_log2=m if has else None, seed=seeds[g]))
            else:
                _ext.attn_bwd(q[r], kv[:, :, 0], kv[:, :, 1], out[r], lse, grad_out[r], scale, dq[r], dkv[:, :, 0],
                              dkv[:, :, 1], m if has else None, p_drop, seeds[g], st if has_st else None)
            dkvs.append(dkv)
        if pair:
            _ext.attn_bwd_pair(sides, scale, p_drop, st if has_st else None)
        return dq, dkvs[0], dkvs[1], None, None, None, None, None


def twin_cross_attention(q, kva, kvb, scale, p_drop, mask_a, mask_b, return_probs=False):
    """q (2B, L, H, 64) stacked; kva (B, Lka, 2, H, 64), kvb (B, Lkb, 2, H, 64); masks (B,1,1,Lk) or None.
    return_probs: -> (context, probs_a, probs_b), the maps detached (attention_probs)"""
    B = q.shape[0] // 2
    return _TwinCrossAttention.apply(q.contiguous(), kva, kvb, scale, _mask_log2(mask_a, B, kva.shape[1]),
                                     _mask_log2(mask_b, B, kvb.shape[1]), float(p_drop), bool(return_probs))


def twin_kernel_ok(hs, linears):
    """the stacked twin path needs the kernel formats: bf16 compute, CUDA, width % 256 (LayerNorm kernel) and fp32
    master parameters with biases"""
    D = hs.shape[-1]
    return (compute_dtype() == torch.bfloat16 and _NATIVE_GEMM[0] and hs.is_cuda and hs.dtype == torch.bfloat16
            and D % 256 == 0 and D <= 1024 and hs.shape[0] % 2 == 0
            and all(l.bias is not None and _param_ok(l.weight, l.bias) and l.weight.shape[0] % 64 == 0
                    and l.weight.shape[1] % 64 == 0 for l in linears))


def twin_linear(hs, lin_a, lin_b, tap=None):
    """stacked states -> [lin_a(2D rows); lin_b(3D rows)], one launch (tap: a GradTap, see mlp())"""
    return _GroupedLinearFn.apply(2, 1, True, tap, hs, lin_a.weight, lin_b.weight, lin_a.bias, lin_b.bias)


def twin_multi_linear(hs, lins_a, lins_b, tap=None):
    """stacked states -> (..., k, N): the k fused projections (Q/K/V) of each stream, one launch"""
    k = len(lins_a)
    ws = [l.weight for l in lins_a] + [l.weight for l in lins_b]
    bs = [l.bias for l in lins_a] + [l.bias for l in lins_b]
    y = _GroupedLinearFn.apply(2, k, True, tap, hs, *ws, *bs)
    return y.view(*y.shape[:-1], k, y.shape[-1] // k)


def twin_multi_linear_var(xa, xb, lins_a, lins_b):
    """the k fused projections of stream a over xa and of stream b over xb (different row counts), one launch"""
    k = len(lins_a)
    ws = [l.weight for l in lins_a] + [l.weight for l in lins_b]
    bs = [l.bias for l in lins_a] + [l.bias for l in lins_b]
    ya, yb = _GroupedLinearFn.apply(2, k, False, None, xa, xb, *ws, *bs)
    return ya.view(*ya.shape[:-1], k, ya.shape[-1] // k), yb.view(*yb.shape[:-1], k, yb.shape[-1] // k)


def twin_mlp(hs, fc1_a, fc2_a, fc1_b, fc2_b, tap=None):
    return _GroupedMlpFn.apply(2, tap, hs, fc1_a.weight, fc1_a.bias, fc2_a.weight, fc2_a.bias,
                               fc1_b.weight, fc1_b.bias, fc2_b.weight, fc2_b.bias)


def twin_dropout_add_layer_norm(x, residual, ln_a, ln_b, p_drop, training):
    return _TwinDropAddLN.apply(x.contiguous(), residual.contiguous(), ln_a.weight, ln_a.bias, ln_b.weight, ln_b.bias,
                                ln_a.eps, float(p_drop) if training else 0.0)


def twin_mix(enc2d, enc3d, hs):
    return _TwinMixFn.apply(enc2d, enc3d, hs)


def twin_split(hs):
    return _TwinSplitFn.apply(hs)


# ---- hoisted K/V projections: several layers' cross-attentions over the SAME encoder states -------------------------
# The answer decoder's 12 cross-attentions read the same question states (reference med.py:112-118 per layer): their
# key / value projections are one GEMM (HoistedKV), each layer's dK/dV is written straight into its block of ONE gradient
# buffer, and the projection's backward is one dX chain + one parked weight-gradient record per layer.  (Rounds 1-3 also
# wired the twin encoder's image / object tokens through this class with a two-segment attention: measured neutral to
# slower three times, DESIGN.md changelog; round 4 replaced it by the concatenation-free _TwinKVFn above and deleted it.)

_HOIST_GROUPED = [True]      # single-stream path: the slots' projections as ONE grouped launch, their input gradients as one grouped launch + a sum
# ... and their input gradients as one grouped launch + a sum (take_dx).  OFF: it rounds the decoder's encoder-state gradient
# differently from the chained ADD epilogue (every upstream gradient moves by bf16 noise, 4e-3 .. 1e-2 rel-L2 -- expected), and
# with it the eager loop and the captured phases stop agreeing bit for bit on the DETECTOR's gradients (1e-7 at the top of the
# backbone's backward, amplified to 8e-3 at SA1 by six levels of bf16 gradient tensors, tools/bisect_graphed.py) although
# the object-token gradient they start from is identical; not understood, and worth ~0.1 ms at most
_HOIST_GROUPED_DX = [False]
_HOIST_BACKGROUND = [False]  # side-stream launches of the hoisted projections with one workgroup per CU (BQ_GEMM_BACKGROUND): measured slower


class HoistedKV(object):
    """K/V projections of `x` (B, L1, 768) -- the FIXED tokens of a cross-attention: image tokens / object tokens -- for
    several layers at once, LEVEL-MAJOR: layer slot i's [key_i; value_i](x) is the contiguous block Y[i] (B, L1, 2, H, 64)
    (the narrow attention kernels walk K / V rows 3 KB apart; the first version wrote ONE (B, L1, n * 1536) tensor whose
    rows were 36 KB apart, which cost the attention kernels what the hoisting saved, DESIGN.md §5 c).
    kv(i): that block.

    The projections depend on nothing the text levels compute, so on a GPU they run on a SIDE stream, one launch per
    layer slot with an event each: the text chain (launch-latency bound, a fraction of the CUs) runs beside them and level
    i's cross-attention waits for event i only.  Backward likewise: as soon as level i's attention backward has written
    d(Y[i]) the side stream accumulates  dx += d(Y[i]) W_i  (ADD epilogue of the dX GEMM); _HoistedKVFn.backward joins."""

    def __init__(self, x, selfattns, heads):
        self.selfattns = list(selfattns)  # BertSelfAttention modules of the cross-attentions, in layer order
        self.n = len(self.selfattns)
        self.heads = heads
        ws = [w for sa in self.selfattns for w in (sa.key.weight, sa.value.weight)]
        bs = [b for sa in self.selfattns for b in (sa.key.bias, sa.value.bias)]
        self.G = None          # (n, B, L1, 2 * 768) gradient of the hoisted projections, allocated by the first writer
        self.written = set()
        self.wc, self.bc = _cat_shadow(ws, bs)
        self.ws = tuple(ws)
        self.nb = self.wc.shape[0] // self.n
        self.x = x
        self.want_dx = bool(x.requires_grad)
        self.ready = None      # per-slot events of the side stream (forward)
        self.side = None       # the side stream, when one is used
        self.dx, self.pushed, self.pending = None, set(), None
        self.late = set()
        self.y_shape = (self.n,) + tuple(x.shape[:-1]) + (self.nb,)
        self.outs = _HoistedKVFn.apply(x, self, *ws, *bs)

    def kv(self, i):
        if self.ready is not None and self.ready[i] is not None:
            torch.cuda.current_stream(self.outs[i].device).wait_event(self.ready[i])
            self.ready[i] = None
        return self.outs[i]

    def block(self, i):
        """rows of the concatenated weight / bias that belong to layer slot i: [key_i; value_i]"""
        n = self.nb
        return self.wc[i * n:(i + 1) * n], self.bc[i * n:(i + 1) * n]

    def grad_view(self, i, like):
        """where layer slot i's attention backward writes d(kv(i)): block i of the shared gradient buffer"""
        if self.G is None:
            self.G = torch.empty(self.y_shape, dtype=like.dtype, device=like.device)
            self.written = set()
            self.dx, self.pushed, self.pending = None, set(), None
            self.late = set()
        self.written.add(i)
        return self.G[i].view(*self.y_shape[1:-1], 2, self.heads, like.shape[-1])

    def push_dx(self, i):
        """block i of the gradient buffer is complete: dx += d(Y[i]) W_i (on the side stream when there is one)"""
        if not self.want_dx or i in self.pushed:
            return
        self.pushed.add(i)
        if _HOIST_GROUPED[0] and _HOIST_GROUPED_DX[0] and self.n > 1 and self.G.is_cuda \
                and _native_dx_ok(self.G[i].view(-1, self.nb), self.nb, self.wc.shape[1]):
            # take_dx: ONE grouped launch for every slot + one sum, instead of a launch per level on the chain.  The same
            # arithmetic with and without a side stream: the eager loop (forks on) and the captured phases (forks off)
            # must round alike -- tests/test_graphed_gpu.py compares their gradients parameter by parameter
            self.late.add(i)
        elif self.side is not None:
            # (the launch itself is issued one push later -- _flush_pending: the text chain's next kernel is then the FIRST
            # successor of this level's attention backward in the captured graph and the GEMM a later one)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.G.device))
            pend, self.pending = self.pending, (i, ev)
            if pend is not None:
                self._launch_dx(*pend)
        else:
            self.dx = _dx2(self.G[i].view(-1, self.nb), self.block(i)[0], add=self.dx, wt=self.block_t(i))

    def block_t(self, i):
        """columns of the transposed concatenated weight that belong to layer slot i (the K-contiguous operand of its dX
        launch when the fixed tokens are few: the decoder's 320 question states), or None"""
        wt = _dx_wt(self.ws, self.wc, self.G[i].numel() // self.nb)
        return None if wt is None else wt[:, i * self.nb:(i + 1) * self.nb]

    def _launch_dx(self, i, ev):
        self.side.wait_event(ev)
        self.G.record_stream(self.side)
        with torch.cuda.stream(self.side):
            self.dx = _dx2(self.G[i].view(-1, self.nb), self.block(i)[0], add=self.dx, background=_HOIST_BACKGROUND[0])

    def take_dx(self, shape):
        if self.pending is not None:
            pend, self.pending = self.pending, None
            self._launch_dx(*pend)
        if self.late:
            from . import _ext
            idx = sorted(self.late)
            self.late = set()
            M = self.G[idx[0]].numel() // self.nb
            part = torch.empty(len(idx), M, self.wc.shape[1], dtype=self.G.dtype, device=self.G.device)
            # (K-contiguous transposed weight copies when every slot has one -- the captured phases, after t_refresh --, else
            # the weights themselves read contraction-major: the same products summed in the same order either way)
            wts = [self.block_t(i) for i in idx]
            xc = any(w is None for w in wts)
            _ext.gemm_grouped([dict(P=self.block(i)[0] if xc else wts[k], Q=_rows(self.G[i].view(-1, self.nb)), out=part[k])
                               for k, i in enumerate(idx)], _ext.GEMM_P_XC if xc else 0, _ext.EPI_NONE)
            tot = part.sum(0, dtype=torch.float32) if self.dx is None else part.sum(0, dtype=torch.float32) + self.dx.view(M, -1).float()
            self.dx = tot.to(self.G.dtype)
        dx, self.dx = self.dx, None
        if self.side is not None and dx is not None:
            main = torch.cuda.current_stream(dx.device)
            main.wait_stream(self.side)
            dx.record_stream(main)
        return None if dx is None else dx.view(shape)



def _fwd2(x2, w, b, out=None, background=False):
    """x2 @ w^T + b for bf16 (M, K) rows and an (N, K) bf16 operand (b bf16 or fp32), native kernels when eligible"""
    if _native_ok(x2, w.shape[0], w.shape[1]):
        from . import _ext
        return _ext.gemm_fwd(_rows(x2), w, b, out=out, background=background)
    y = F.linear(x2, w, b if b is None or b.dtype == x2.dtype else b.to(x2.dtype))
    if out is not None:
        out.copy_(y)
        return out
    return y


def _dx2(g2, w, add=None, background=False, wt=None):
    """g2 @ w (+ add); wt: w's transpose (see _ext.gemm_dx)"""
    if _native_dx_ok(g2, w.shape[0], w.shape[1]):
        from . import _ext
        return _ext.gemm_dx(_rows(g2), w, add=add, background=background, wt=wt)
    dx = torch.mm(g2, w)
    return dx if add is None else dx + add


class _HoistedKVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, hold, *wb):
        xb = x if x.dtype == compute_dtype() else x.to(compute_dtype())
        x2 = xb.reshape(-1, xb.shape[-1])
        n, nb = hold.n, hold.nb
        y = torch.empty(hold.y_shape, dtype=xb.dtype, device=xb.device)
        y2 = y.view(n, -1, nb)
        grouped = _HOIST_GROUPED[0] and xb.is_cuda and n > 1 and _native_ok(x2, nb, x2.shape[1])

        def all_slots():
            # one grouped launch for all layer slots (12 launches of ~8 us on the chain before round 6); the SAME launch with
            # and without a side stream, so that the eager loop and the captured phases round alike
            from . import _ext
            xr = _rows(x2)
            _ext.gemm_grouped([dict(P=hold.block(i)[0], Q=xr, out=y2[i], bias=hold.block(i)[1]) for i in range(n)], 0,
                              _ext.EPI_BIAS)
        if xb.is_cuda and overlap_enabled(xb) and _native_ok(x2, nb, x2.shape[1]):
            f = fork("hoist", xb)
            hold.side, hold.ready = f.side, []
            with f:
                f.uses(xb, y)
                if grouped:
                    all_slots()
                    ev = torch.cuda.Event()
                    ev.record(f.side)
                    hold.ready = [ev] * n
                else:
                    for i in range(n):
                        _fwd2(x2, *hold.block(i), out=y2[i], background=_HOIST_BACKGROUND[0])
                        ev = torch.cuda.Event()
                        ev.record(f.side)
                        hold.ready.append(ev)
            y.record_stream(f.main)
        elif grouped:
            all_slots()
        else:
            for i in range(n):
                _fwd2(x2, *hold.block(i), out=y2[i])
        ctx.save_for_backward(xb)
        ctx.hold, ctx.x_dtype, ctx.k = hold, x.dtype, len(wb) // 2
        y6 = y.view(*hold.y_shape[:-1], 2, hold.heads, -1)
        return tuple(y6[i] for i in range(n))

    @staticmethod
    def backward(ctx, *grads):
        hold = ctx.hold
        (xb,) = ctx.saved_tensors
        like = next(g for g in grads if g is not None)
        for i, g in enumerate(grads):
            if g is None:
                hold.grad_view(i, like).zero_()
            elif i not in hold.written or g.data_ptr() != hold.grad_view(i, like).data_ptr():
                hold.grad_view(i, like).copy_(g)  # the gradient did not come from attention_q_kv's in-place writer
        dx = None
        if ctx.needs_input_grad[0]:
            hold.want_dx = True
            for i in range(hold.n):
                hold.push_dx(i)      # (the blocks whose writer did not push them already)
            dx = hold.take_dx(xb.shape).to(ctx.x_dtype)
        G = hold.G
        hold.G = None
        x2 = xb.reshape(-1, xb.shape[-1])
        k, n, nb = ctx.k, hold.n, hold.nb
        if _defer_ok(G[0].view(-1, nb), x2):
            # inside a deferred-wgrad scope every slot's [key_i; value_i] block is ONE parked record (the flush splits its
            # rows evenly over the two weights)
            for i, sa in enumerate(hold.selfattns):
                _park(G[i].view(-1, nb), x2, [sa.key.weight, sa.value.weight], [sa.key.bias, sa.value.bias])
            return (dx, None) + (None,) * (2 * k)
        dws, dbs = [], []
        h = nb // 2
        for i in range(n):
            dw, db = _dw_db(G[i].view(-1, nb), x2, True, True)
            dws += [dw[:h], dw[h:]]
            dbs += [db[:h], db[h:]]
        return (dx, None) + tuple(dws) + tuple(dbs)


def _packed_ok(t, mask, strided=False):
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.shape[-1] == 64
            and (t.is_contiguous() or (strided and t.stride(-1) == 1 and all(st % 8 == 0 for st in t.stride()[:-1])))
            and (mask is None or (mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1)))


def packed_kernel_ok(qkv, key_mask):
    """True when attention_packed(qkv, ..., key_mask) runs on the fused kernels (needed by callers that can only
    hand over a causal mask in factored form: key mask + causal flag)"""
    return _packed_ok(qkv, key_mask)


def attention_packed(qkv, scale, dropout_p=0.0, mask=None, causal=False, return_probs=False):
    """Self-attention on the output of a fused QKV projection, qkv (B, L, 3, H, D) -> (B, L, H, D).
    bf16 / D=64 / CUDA goes to the fused kernels; anything else to the reference composition.  causal=True (kernel
    path only, see packed_kernel_ok): `mask` is the (B,1,1,L) key mask and keys after the query are hidden too."""
    if _packed_ok(qkv, mask):
        # return_probs: (context, probs f32 (B,H,L,L)).  On the kernel path the map is rebuilt from the forward's LSE
        # (csrc/attn.hip attn_probs_kernel) and is DETACHED: the reference's is part of the autograd graph, but nothing
        # on this path differentiates through it (a caller that does -- save_attention + attn_gradients hooks -- gets the
        # reference composition, med.BertSelfAttention)
        return _PackedAttention.apply(qkv, scale, _mask_log2(mask, qkv.shape[0], qkv.shape[1]), float(dropout_p),
                                      bool(causal), bool(return_probs))
    if causal:
        raise RuntimeError("attention_packed(causal=True) needs the kernel path; pass the full (B,1,L,L) mask instead")
    ctx, probs = attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, scale, return_probs=return_probs,
                           dropout_p=dropout_p)
    return (ctx, probs) if return_probs else ctx


def attention_q_kv(q, kv, scale, dropout_p=0.0, mask=None, return_probs=False, sink=None):
    """Cross-attention: q (B, Lq, H, D), kv (B, Lk, 2, H, D) from a fused K/V projection -> (B, Lq, H, D)
    (return_probs: see attention_packed).  sink = (HoistedKV, slot): kv is that projection's strided block for this
    layer (kernel path only) and its gradient is written in place into the projection's gradient buffer."""
    if sink is not None:
        if not (_packed_ok(kv, mask, strided=True) and q.is_cuda and q.dtype == torch.bfloat16 and q.stride(-1) == 1):
            raise RuntimeError("attention_q_kv: a hoisted K/V block needs the kernel path (bf16, D = 64, key-only mask)")
        return _QKVAttention.apply(q, kv, scale, _mask_log2(mask, kv.shape[0], kv.shape[1]), float(dropout_p),
                                   bool(return_probs), sink)
    if _packed_ok(kv, mask) and q.is_cuda and q.dtype == torch.bfloat16 and q.stride(-1) == 1:
        return _QKVAttention.apply(q, kv, scale, _mask_log2(mask, kv.shape[0], kv.shape[1]), float(dropout_p),
                                   bool(return_probs))
    ctx, probs = attention(q, kv[:, :, 0], kv[:, :, 1], mask, scale, return_probs=return_probs, dropout_p=dropout_p)
    return (ctx, probs) if return_probs else ctx


# ---- beam-search decoding on a static K/V cache (csrc/attn_decode.hip) ----------------------------------------------------------
# The reference's decode loop grows every layer's cache by torch.cat and reorders all of it with index_select after every
# step (models/med.py:196-214, :1466-1470).  Here the cache is ONE allocation that stays in place: slot s writes its step-t key /
# value row into KV[layer, s, t] and an ancestry table says which physical row holds position j of the hypothesis that
# currently sits in slot s.  Reordering the beams rewrites that table (Lmax x S int32), not the cache.

def reorder_ancestry(anc, t, beam_idx, identity=None):
    """The table update of one beam reorder, in place; pure torch (CPU tensors too).  anc: int (Lmax, S); t: positions already
    written (the NEXT step writes row t); beam_idx (S,): new slot s continues the hypothesis of old slot beam_idx[s].
    anc[:t] = anc[:t][:, beam_idx]; row t, where every slot is about to write its own row, becomes the identity."""
    if t > 0:
        anc[:t] = anc[:t].index_select(1, beam_idx)
    if t < anc.shape[0]:
        anc[t] = torch.arange(anc.shape[1], dtype=anc.dtype, device=anc.device) if identity is None else identity
    return anc


def gather_history(cache, anc, t):
    """(S, t, ...) history of every slot read through the ancestry table: what the decode kernel attends over, and what
    physically reordering the cache with index_select (models/med.py:1466-1470) would have left in rows [0, t)"""
    j = torch.arange(t, device=cache.device)
    return cache[anc[:t].long().t(), j[None, :]]


class DecodeLayer(object):
    """what BertSelfAttention needs of a DecodeCache for one layer (the `past_key_value` of the decode route)"""
    __slots__ = ("cache", "index")

    def __init__(self, cache, index):
        self.cache, self.index = cache, index

    def self_attention(self, qkv, scale):
        """qkv (S, 1, 3, H, 64) of the step's token -> context (S, 1, H, 64); writes the step's row of this layer's cache"""
        from . import _ext
        c = self.cache
        return _ext.attn_decode_self(qkv, c.kv[self.index], c.anc, scale, t=c.t, t_tensor=c.pos)

    def cross_attention(self, q, scale):
        """q (S, 1, H, 64) -> context over this layer's hoisted question keys / values (they belong to the slot)"""
        from . import _ext
        c = self.cache
        return _ext.attn_decode_cross(q, c.cross[self.index], scale, c.cross_mask)


class DecodeCache(object):
    """Static cache of one beam-search decode: kv bf16 (n_layers, S, Lmax, 2, H, 64) in one allocation, the ancestry table anc
    int32 (Lmax, S), the position as a device counter `pos` (read by the kernels: a captured step replays) mirrored by the host
    integer `t`, the HoistedKV of the encoder states (every layer's cross-attention K/V, projected ONCE for the whole decode)
    and the encoder key mask in kernel format.  advance() after every step, reorder(beam_idx) after the beams moved."""

    def __init__(self, n_layers, S, Lmax, heads, device, hoisted=None, cross_mask=None):
        self.n_layers, self.S, self.Lmax, self.heads = n_layers, S, Lmax, heads
        self.kv = torch.zeros(n_layers, S, Lmax, 2, heads, 64, dtype=torch.bfloat16, device=device)
        self.identity = torch.arange(S, dtype=torch.int32, device=device)
        self.anc = self.identity[None, :].repeat(Lmax, 1)
        self.pos = torch.zeros(1, dtype=torch.int32, device=device)
        self.t = 0
        self.hoisted = hoisted
        # (kv(i) waits for the side stream the hoisted projections may run on: done here, once, before any step or capture)
        self.cross = [hoisted.kv(i) for i in range(n_layers)] if hoisted is not None else None
        self.cross_mask = cross_mask

    def layer(self, i):
        return DecodeLayer(self, i)

    def advance(self):
        if self.t + 1 > self.Lmax:
            raise RuntimeError("DecodeCache: more than Lmax = %d steps" % self.Lmax)
        self.t += 1
        self.pos.add_(1)

    def reorder(self, beam_idx):
        reorder_ancestry(self.anc, self.t, beam_idx, self.identity)
        return self


class BeamState(object):
    """What generation.beam_search keeps between two steps, as static device buffers beside a DecodeCache (csrc/beam.hip,
    include/bqhip_beam.h): beam scores, the token table, the id buffer the next decoder step reads, done flags, the count of
    samples not yet done and the finished-hypothesis heaps (tokens included).  Everything but `ids` lies in ONE allocation, so
    host() is one copy.  step(logits) runs one whole iteration of the search on the device -- it reads cur_len from cache.pos
    (already incremented for the step) and reorders cache.anc in place -- and allocates, synchronises and copies nothing."""

    _LAYOUT = (("beam_score", torch.float32, "S"), ("tokens", torch.int32, "SL"), ("done", torch.int32, "B"),
               ("not_done", torch.int32, "H"), ("src", torch.int32, "S"), ("cand", torch.int64, "SK"),
               ("top_score", torch.float32, "BK"), ("top_index", torch.int32, "BK"), ("heap_len", torch.int32, "B"),
               ("heap_adds", torch.int32, "B"), ("heap_seq", torch.int32, "Bn"), ("heap_hyplen", torch.int32, "Bn"),
               ("heap_sum", torch.float32, "Bn"), ("heap_score", torch.float64, "Bn"), ("heap_worst", torch.float64, "B"),
               ("heap_tokens", torch.int32, "BnL"))

    def __init__(self, cache, prompt_ids, num_beams, max_length, eos_token_id, pad_token_id, min_length=0, length_penalty=1.0,
                 early_stopping=False):
        from . import _ext
        S, nb = prompt_ids.shape[0], int(num_beams)
        if prompt_ids.dim() != 2 or prompt_ids.shape[1] != 1 or S % nb or S != cache.S:
            raise RuntimeError("BeamState: one-token prompts for the cache's %d slots are needed" % cache.S)
        self.cache, self.B, self.nb, self.S, self.max_length = cache, S // nb, nb, S, int(max_length)
        self.eos, self.pad, self.min_length = int(eos_token_id), int(pad_token_id), int(min_length)
        self.length_penalty, self.early_stopping = length_penalty, bool(early_stopping)
        dev = prompt_ids.device
        self.shapes = {"S": (S,), "SL": (S, self.max_length), "B": (self.B,), "H": (_ext.BEAM_MAX_LEN + 2,), "SK": (S, 2 * nb),
                       "BK": (self.B, 2 * nb), "Bn": (self.B, nb), "BnL": (self.B, nb, self.max_length)}
        self.offsets, n = {}, 0
        for name, dtype, shape in self._LAYOUT:
            self.offsets[name] = n
            n += -(-_numel(self.shapes[shape]) * torch.empty(0, dtype=dtype).element_size() // 16) * 16
        self.arena = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.t = self._views(self.arena)
        self.t["beam_score"].view(self.B, nb)[:, 1:] = -1e9
        self.t["tokens"][:, 0] = prompt_ids[:, 0].to(torch.int32)
        self.t["not_done"].fill_(self.B)
        self.t["heap_worst"].fill_(1e9)
        self.ids = prompt_ids.to(torch.int64).clone(memory_format=torch.contiguous_format)
        # n ** length_penalty as Python computes it: the device never calls pow
        self.lenpow = torch.tensor([1.0] + [float(k ** length_penalty) for k in range(1, self.max_length + 1)],
                                   dtype=torch.float64).to(dev)
        self._desc = self._desc_key = None

    def _views(self, arena):
        out = {}
        for name, dtype, shape in self._LAYOUT:
            shp = self.shapes[shape]
            nbytes = _numel(shp) * torch.empty(0, dtype=dtype).element_size()
            out[name] = arena[self.offsets[name]:self.offsets[name] + nbytes].view(dtype).view(shp)
        return out

    def __getattr__(self, name):
        t = self.__dict__.get("t")
        if t is not None and name in t:
            return t[name]
        raise AttributeError(name)

    def step(self, logits):
        from . import _ext
        key = (logits.data_ptr(), logits.dtype, tuple(logits.shape), logits.stride())
        if key != self._desc_key:
            self._desc = _ext.beam_state_desc(logits, self.B, self.nb, self.max_length, self.eos, self.pad, self.min_length,
                                              self.early_stopping, pos=self.cache.pos, lenpow=self.lenpow, anc=self.cache.anc,
                                              ids=self.ids, **self.t)
            self._desc_key, self._logits = key, logits
        _ext.beam_step(self._desc, logits.device)

    def host(self):
        """{name: CPU tensor} of everything but ids, by ONE copy"""
        return self._views(self.arena.cpu())

    def hypotheses(self, host):
        """the heaps of host() as generation.BeamHypotheses, entries in list order -> (hyps, done)"""
        from .generation import BeamHypotheses
        hyps = []
        for b in range(self.B):
            h = BeamHypotheses(self.nb, self.length_penalty, self.early_stopping)
            n = int(host["heap_len"][b])
            for i in sorted(range(n), key=lambda i: int(host["heap_seq"][b, i])):
                h.beams.append((float(host["heap_score"][b, i]),
                                host["heap_tokens"][b, i, :int(host["heap_hyplen"][b, i])].tolist()))
            h.worst_score = float(host["heap_worst"][b])
            hyps.append(h)
        return hyps, [bool(d) for d in host["done"].tolist()]


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


# ---- answer ranking on the shared K/V of the question (csrc/attn_rank.hip) -------------------------------------------------------
# The reference re-scores k candidate answers per question against question states tiled k times (models/blip_vqa_3d.py:509-566)
# and every decoder layer projects the tiled rows to K / V.  The K / V of a question do not depend on the candidate: here they
# are projected ONCE from the untiled (Bq, Lq, 768) states and candidate sequence n reads question n // group.

class RankLayer(object):
    """what BertSelfAttention needs of a RankShared for one layer: the HoistedStates of the ranking route (`hoisted`, `slot`)
    plus `group`; handed to the layer as its encoder_hidden_states and to its self-attention as the `rank` argument"""
    __slots__ = ("shared", "slot")

    def __init__(self, shared, slot):
        self.shared, self.slot = shared, slot

    @property
    def hoisted(self):
        return self.shared.hoisted

    @property
    def group(self):
        return self.shared.group

    def self_attention(self, qkv, scale, key_mask):
        """qkv (N, La, 3, H, 64), key_mask the factored (N, 1, 1, La) additive mask -> causal context (N, La, H, 64)"""
        from . import _ext
        return _ext.attn_rank_self(qkv, scale, _mask_log2(key_mask, qkv.shape[0], qkv.shape[1]))

    def cross_attention(self, q, scale):
        """q (N, La, H, 64) -> context over this layer's keys / values of question n // group"""
        from . import _ext
        s = self.shared
        return _ext.attn_rank_cross(q, s.blocks[self.slot], scale, s.group, s.mask_log2)


class RankShared(object):
    """encoder_hidden_states of the ranking route: ONE HoistedKV over the untiled question states (Bq, Lq, 768) for all decoder
    layers, the question key mask in kernel format, and `group` -- how many consecutive decoder sequences read each question
    (1: the first-token pass, k: the re-score).  Built once per rank_answer call (BertLMHeadModel.rank_shared); inference only:
    there is no backward."""

    def __init__(self, states, selfattns, heads, key_mask=None):
        from . import _ext
        self.Bq, self.Lq = int(states.shape[0]), int(states.shape[1])
        self.hoisted = HoistedKV(_c(states), selfattns, heads)
        # (kv(i) waits for the side stream the hoisted projections may run on: done here, once)
        self.blocks = [self.hoisted.kv(i) for i in range(self.hoisted.n)]
        self.mask_log2 = None if key_mask is None else _ext.key_mask_log2(key_mask, self.Bq, self.Lq)
        self.group = 1

    def grouped(self, group):
        """a view of the same projections and mask for `group` consecutive sequences per question (this object is unchanged)"""
        import copy
        v = copy.copy(self)
        v.group = int(group)
        return v

    def layer(self, i):
        return RankLayer(self, i)


class _LMHeadCE(torch.autograd.Function):
    """Tied LM head + shifted label-smoothed cross entropy on the kernels (csrc/gemm.hip cross-entropy epilogue +
    csrc/lmhead.hip): logits computed tile by tile on the MFMA pipeline and stored once as bf16; the loss statistics
    come from the fp32 accumulators; no fp32 logits, no softmax / log-softmax / nll kernels.  hidden (B, L, D) bf16,
    weight (V, D) fp32 parameter (the word-embedding matrix), bias fp32 parameter (V,), labels (B, L) with -100 =
    ignore.  Returns (logits (B, L, V) bf16 view of the padded buffer, per-row loss (B, L) f32 with position t holding
    the loss of predicting labels[:, t+1]; last position 0)."""

    @staticmethod
    def forward(ctx, hidden, weight, bias, labels, label_smoothing):
        from . import _ext
        B, L, D = hidden.shape
        V = weight.shape[0]
        Vp = (V + 63) // 64 * 64
        wb = _shadow(weight)
        h2 = _rows(hidden)
        tgt = torch.full((B, L), -100, dtype=torch.int32, device=hidden.device)
        tgt[:, :-1] = labels[:, 1:].to(torch.int32)
        bias_pad = torch.zeros(Vp, dtype=torch.float32, device=hidden.device)
        if bias is not None:
            bias_pad[:V] = bias.detach()
        logits, loss, lse = _ext.lmhead_ce_fwd(h2, wb, bias_pad, tgt.view(-1), V, label_smoothing)
        ctx.save_for_backward(h2, wb, logits, lse, tgt)
        ctx.cfg = (B, L, D, V, Vp, float(label_smoothing), hidden.dtype, bias is not None)
        ctx.params = (weight, bias)
        out_logits = logits.view(B, L, Vp)[:, :, :V]   # NB consumed by the backward (turned into dlogits in place)
        ctx.mark_non_differentiable(out_logits)
        return out_logits, loss.view(B, L)

    @staticmethod
    def backward(ctx, _dlogits, dloss):
        from . import _ext
        h2, wb, logits, lse, tgt = ctx.saved_tensors
        B, L, D, V, Vp, eps, h_dtype, has_bias = ctx.cfg
        g = dloss.reshape(-1).to(torch.float32).contiguous()
        dl = _ext.lmhead_ce_dlogits(logits, lse, tgt.view(-1), g, V, eps)   # in place: the logits are consumed
        R = B * L
        # dH (R, D) = dlogits (R, Vp) W (V, D): a 30 528-long contraction for a small output -> cut into pieces (the rows
        # of W beyond V are out of bounds for the DMA: zeros); each piece stores its own slab and the slabs are summed in
        # piece order (_ext.gemm_grouped, fixed_order) IN EVERY MODE: dH is the one cut contraction whose result every
        # other gradient of the step descends from.  Accumulated with fp32 atomics, the arrival order of the pieces moved
        # the bf16 rounding of an element of dH now and then, and the bf16 backward behind it carried that into every
        # gradient upstream (1e-3 .. 1e-2 rel-L2 between two executions of one step from the same state, eager or replayed)
        dh = torch.zeros(R, D, dtype=torch.float32, device=h2.device)
        tiles = ((D + 63) // 64) * ((R + 31) // 32)
        ksplit = max(1, min(Vp // 64, (768 + tiles - 1) // tiles))
        _ext.gemm_grouped([dict(P=wb, Q=dl, out=dh, Kc=Vp, p_bytes=wb.shape[0] * wb.stride(0) * 2, ksplit=ksplit)],
                          _ext.GEMM_P_XC | _ext.GEMM_OUT_F32, _ext.EPI_NONE, 32, fixed_order=True)
        dhidden = dh.view(B, L, D).to(h_dtype)
        # dW (Vp, D) = dlogits^T h (fp32; its first V rows are the gradient of the tied embedding matrix)
        dw = torch.empty(Vp, D, dtype=torch.float32, device=h2.device)
        _ext.gemm_grouped([dict(P=h2, Q=dl, out=dw)], _ext.GEMM_P_XC | _ext.GEMM_Q_XC | _ext.GEMM_OUT_F32, _ext.EPI_NONE, 256)
        db = _ext.colsum_grouped([dl])[0][:V] if has_bias else None
        return dhidden, dw[:V], db, None, None


def lm_loss(hidden, decoder_weight, decoder_bias, labels, label_smoothing=0.1):
    """Tied LM head + shifted label-smoothed cross entropy, summed per sequence (med.py:1417-1432).

    hidden (B,L,D) = output of the prediction-head transform; labels (B,L) with -100 = ignore.
    Returns (logits (B,L,V), loss (B,)).
    """
    D = hidden.shape[-1]
    if (_NATIVE_GEMM[0] and hidden.is_cuda and compute_dtype() == torch.bfloat16 and D % 64 == 0
            and isinstance(decoder_weight, torch.nn.Parameter) and decoder_weight.dtype == torch.float32
            and decoder_weight.is_contiguous() and hidden.dim() == 3):
        logits, row_loss = _LMHeadCE.apply(hidden, decoder_weight, decoder_bias, labels, float(label_smoothing))
        return logits, row_loss.sum(1)
    logits = linear(hidden, decoder_weight, decoder_bias).float()
    B, L, V = logits.shape
    shifted = logits[:, :-1, :].reshape(-1, V)
    tgt = labels[:, 1:].reshape(-1)
    loss = F.cross_entropy(shifted, tgt, reduction="none", label_smoothing=label_smoothing)
    return logits, loss.view(B, -1).sum(1)


def gelu(x):
    return F.gelu(x)


SQRT_HEAD = math.sqrt
