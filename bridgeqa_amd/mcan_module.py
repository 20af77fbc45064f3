"""MCAN blocks used by the reference-object head of ScanQA's VQA branch and by the stage-1 question branch -- mirror of the
reference's models/mcan_module.py (FC :18-43, MLP :46-54, LayerNorm :57-69, AttFlat :74-133, MHAtt :138-224, FFN :229-245,
SA :250-273, SGA :278-311, MCAN_E :316-327, MCAN_ED :330-355) with its class names, constructor arguments, forward signatures and state-dict keys (linear_v / linear_k / linear_q /
linear_merge, mlp.fc.linear, mlp.linear, a_2 / b_2), so reference checkpoints load with strict=True.

SURVEY.md §8f rank 1 ("ScanQA.forward glue"): these blocks sit on the CALLER side of the hot path -- 2 layers over 256
proposals x 256 channels against 20 question states, < 0.1 % of the step's flop -- so they run on torch ops (fp32), no
kernels of their own.  AttFlat and the MCAN_E / MCAN_ED stacks belong to the non-BLIP question branch (qa_module.py:496-590;
hotpath.ScanQAHotPath(use_blip=False, lang_branch=True)): torch compositions over the same blocks.

Reference quirks kept on purpose (parity, not opinion):
  * LayerNorm divides by (std + eps) with the UNBIASED standard deviation (torch.std), not sqrt(var + eps);
  * masks are boolean with True = "hide this key" (scores.masked_fill(mask, -1e9)).

The fused route (set_fused / BQ_MCAN_FUSED=1, default off).  The two launch-bound compositions of these blocks -- LayerNorm,
always applied to a residual sum, ~11 launches forward; AttFlat's masked_fill / softmax / weighted sums / cat -- have kernels in
csrc/mcan.hip (include/bqhip_mcan.h states their arithmetic).  With the switch on, fp32 device tensors of an eligible size take
them through one autograd Function each; everything else, and everything with the switch off, runs the compositions below
unchanged.  nn.Dropout stays a torch op on both routes, so one seed gives both the same masks.

The fused attention route (set_fused_attention / BQ_MCAN_ATT=1, default off; independent of the switch above).  MHAtt's core --
scores, division, masked_fill, softmax, dropout, the product with V, transpose().contiguous(), 9 device kernels forward and
11 backward per site -- has kernels in csrc/mhatt.hip (include/bqhip_mhatt.h states their arithmetic): one launch forward, two
backward, reading the three linears' outputs in place and writing the layout linear_merge reads.  The dropout multiplier is
drawn by MHAtt.dropout itself on a tensor of ones of the composition's shape, at the same point of the random stream.
"""
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

_FUSED = os.environ.get("BQ_MCAN_FUSED", "0") == "1"


def set_fused(flag):
    """route LayerNorm and AttFlat's pooling through csrc/mcan.hip where eligible; returns the previous setting"""
    global _FUSED
    prev, _FUSED = _FUSED, bool(flag)
    return prev


def fused_enabled():
    return _FUSED


_FUSED_ATT = os.environ.get("BQ_MCAN_ATT", "0") == "1"


def set_fused_attention(flag):
    """route MHAtt's attention core through csrc/mhatt.hip where eligible; returns the previous setting"""
    global _FUSED_ATT
    prev, _FUSED_ATT = _FUSED_ATT, bool(flag)
    return prev


def fused_attention_enabled():
    return _FUSED_ATT


def _f32_cuda(*ts):
    return all(t.is_cuda and t.dtype == torch.float32 for t in ts)


class _ResidualLayerNormFn(torch.autograd.Function):
    """a_2 (z - mean) / (sigma + eps) + b_2 over z = x + s on bqm_mcan_ln_fwd / bqm_mcan_ln_bwd"""

    @staticmethod
    def forward(ctx, x, s, a2, b2, eps):
        from . import _ext
        H = x.shape[-1]
        x2 = x.detach().reshape(-1, H).contiguous()
        s2 = s.detach().reshape(-1, H).contiguous() if s is not None else None
        a2d = a2.detach().contiguous()
        y, mean, sigma = _ext.mcan_ln_fwd(x2, s2, a2d, b2.detach().contiguous(), eps)
        ctx.save_for_backward(x2, s2, a2d, mean, sigma)
        ctx.eps = eps
        return y.view(x.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from . import _ext
        x2, s2, a2d, mean, sigma = ctx.saved_tensors
        dz, dab = _ext.mcan_ln_bwd(dy.reshape(x2.shape).contiguous(), x2, s2, a2d, mean, sigma, ctx.eps)
        dz = dz.view(dy.shape)
        return dz, (dz if s2 is not None else None), dab[0], dab[1], None


class _AttFlatPoolFn(torch.autograd.Function):
    """softmax over the keys of the (masked) glimpse logits and the glimpses' weighted sums on bqm_attflat_pool_fwd / _bwd"""

    @staticmethod
    def forward(ctx, x, logits, hide):
        from . import _ext
        xc, lc = x.detach().contiguous(), logits.detach().contiguous()
        out, p = _ext.attflat_pool_fwd(xc, lc, hide)
        ctx.save_for_backward(xc, p, hide)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        from . import _ext
        xc, p, hide = ctx.saved_tensors
        dx, dlogits = _ext.attflat_pool_bwd(dout.contiguous(), xc, p, hide)
        return dx, dlogits, None


class _MHAttCoreFn(torch.autograd.Function):
    """softmax(hide ? -1e9 : q k^T / sqrt d) keep v per head on bqh_mhatt_fwd / bqh_mhatt_bwd; q, k, v and the result (B, N, H)"""

    @staticmethod
    def forward(ctx, q, k, v, hide, keep, heads):
        from . import _ext
        qd, kd, vd = q.detach(), k.detach(), v.detach()
        out, p = _ext.mhatt_fwd(qd, kd, vd, hide, keep, heads)
        ctx.save_for_backward(qd, kd, vd, p, hide, keep)
        ctx.heads = heads
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        from . import _ext
        qd, kd, vd, p, hide, keep = ctx.saved_tensors
        dq, dk, dv = _ext.mhatt_bwd(dout.contiguous(), qd, kd, vd, p, hide, keep, ctx.heads)
        return dq, dk, dv, None, None, None


class FC(nn.Module):
    def __init__(self, in_size, out_size, pdrop=0., use_gelu=True):
        super().__init__()
        self.pdrop, self.use_gelu = pdrop, use_gelu
        self.linear = nn.Linear(in_size, out_size)
        if use_gelu:
            self.gelu = nn.GELU()
        if pdrop > 0:
            self.dropout = nn.Dropout(pdrop)

    def forward(self, x):
        x = self.linear(x)
        if self.use_gelu:
            x = self.gelu(x)
        return self.dropout(x) if self.pdrop > 0 else x


class MLP(nn.Module):
    def __init__(self, in_size, mid_size, out_size, pdrop=0., use_gelu=True):
        super().__init__()
        self.fc = FC(in_size, mid_size, pdrop=pdrop, use_gelu=use_gelu)
        self.linear = nn.Linear(mid_size, out_size)

    def forward(self, x):
        return self.linear(self.fc(x))


class LayerNorm(nn.Module):
    """a_2 * (x - mean) / (std + eps) + b_2 with torch.std's unbiased estimate (mcan_module.py:57-69)"""

    def __init__(self, size, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.a_2 = nn.Parameter(torch.ones(size))
        self.b_2 = nn.Parameter(torch.zeros(size))

    def _fused_ok(self, x, residual):
        if not (_FUSED and _f32_cuda(x, self.a_2, self.b_2) and x.dim() >= 1 and x.numel() > 0):
            return False
        if residual is not None and not (_f32_cuda(residual) and residual.shape == x.shape and residual.device == x.device):
            return False
        from . import _ext
        return _ext.mcan_hidden_ok(x.shape[-1]) and self.a_2.shape == (x.shape[-1],) and self.a_2.device == x.device

    def forward(self, x, residual=None):
        """LayerNorm(x + residual); the sum is formed inside the kernel on the fused route"""
        if self._fused_ok(x, residual):
            return _ResidualLayerNormFn.apply(x, residual, self.a_2, self.b_2, self.eps)
        if residual is not None:
            x = x + residual
        centred = x - x.mean(-1, keepdim=True)
        n = x.shape[-1]
        std = centred.pow(2).sum(-1, keepdim=True).div(max(n - 1, 1)).sqrt()
        return self.a_2 * centred / (std + self.eps) + self.b_2


class MHAtt(nn.Module):
    def __init__(self, hidden_size, num_heads=8, pdrop=0.1):
        super().__init__()
        self.linear_v = nn.Linear(hidden_size, hidden_size)
        self.linear_k = nn.Linear(hidden_size, hidden_size)
        self.linear_q = nn.Linear(hidden_size, hidden_size)
        self.linear_merge = nn.Linear(hidden_size, hidden_size)
        self.hidden_size, self.num_heads = hidden_size, num_heads
        self.head_hidden_size = int(hidden_size / num_heads)
        self.dropout = nn.Dropout(pdrop)

    def _split(self, t, B):
        return t.view(B, -1, self.num_heads, self.head_hidden_size).transpose(1, 2)

    def _fused_ok(self, v, k, q, mask):
        if not (_FUSED_ATT and _f32_cuda(v, k, q) and q.dim() == 3 and k.dim() == 3 and v.shape == k.shape and q.numel() > 0):
            return False
        B, Nq, H = q.shape
        Nk = k.shape[1]
        if not (k.shape[0] == B and k.shape[2] == H == self.hidden_size == self.num_heads * self.head_hidden_size
                and k.device == q.device and v.device == q.device
                and q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and 0 <= self.dropout.p < 1):
            return False
        if mask is not None and not (mask.dtype == torch.bool and mask.is_cuda and mask.device == q.device
                                     and tuple(mask.shape) == (B, 1, 1, Nk)):
            return False
        from . import _ext
        return _ext.mhatt_ok(H, self.num_heads, Nq, Nk) and B * self.num_heads <= 65535

    def forward(self, v, k, q, mask, att_pdrop=0, att_drop_topk=100):
        B = q.size(0)
        v, k, q = self.linear_v(v), self.linear_k(k), self.linear_q(q)
        if self._fused_ok(v, k, q, mask):
            Nq, Nk = q.shape[1], k.shape[1]
            hide = mask.reshape(B, Nk).contiguous().view(torch.uint8) if mask is not None else None
            keep = None
            if self.dropout.training and self.dropout.p > 0:   # the composition's draw: same module, shape, dtype and point
                keep = self.dropout(torch.ones(B, self.num_heads, Nq, Nk, dtype=torch.float32, device=q.device))
            return self.linear_merge(_MHAttCoreFn.apply(q, k, v, hide, keep, self.num_heads))
        v, k, q = self._split(v, B), self._split(k, B), self._split(q, B)
        ctx = self.att(v, k, q, mask, att_pdrop, att_drop_topk)
        return self.linear_merge(ctx.transpose(1, 2).contiguous().view(B, -1, self.hidden_size))

    def att(self, value, key, query, mask, att_pdrop=0, att_drop_topk=100):
        # (att_pdrop / att_drop_topk: accepted and ignored, as in the reference -- its top-k masking is commented out)
        scores = torch.matmul(query, key.transpose(-2, -1)) / math.sqrt(query.size(-1))
        if mask is not None:
            scores = scores.masked_fill(mask, -1e9)
        return torch.matmul(self.dropout(F.softmax(scores, dim=-1)), value)


class FFN(nn.Module):
    def __init__(self, hidden_size, pdrop=0.1):
        super().__init__()
        self.mlp = MLP(in_size=hidden_size, mid_size=int(hidden_size * 4), out_size=hidden_size, pdrop=pdrop, use_gelu=True)

    def forward(self, x):
        return self.mlp(x)


class SA(nn.Module):
    """self-attention block, post-norm"""

    def __init__(self, hidden_size, num_heads=8, pdrop=0.1):
        super().__init__()
        self.mhatt = MHAtt(hidden_size, num_heads, pdrop)
        self.ffn = FFN(hidden_size, pdrop)
        self.dropout1, self.norm1 = nn.Dropout(pdrop), LayerNorm(hidden_size)
        self.dropout2, self.norm2 = nn.Dropout(pdrop), LayerNorm(hidden_size)

    def forward(self, x, x_mask):
        x = self.norm1(x, self.dropout1(self.mhatt(x, x, x, x_mask)))
        return self.norm2(x, self.dropout2(self.ffn(x)))


class SGA(nn.Module):
    """self-attention over x, then x attends to y (guided attention), then FFN; post-norm"""

    def __init__(self, hidden_size, num_heads=8, pdrop=0.1):
        super().__init__()
        self.mhatt1 = MHAtt(hidden_size, num_heads, pdrop)
        self.mhatt2 = MHAtt(hidden_size, num_heads, pdrop)
        self.ffn = FFN(hidden_size, pdrop)
        self.dropout1, self.norm1 = nn.Dropout(pdrop), LayerNorm(hidden_size)
        self.dropout2, self.norm2 = nn.Dropout(pdrop), LayerNorm(hidden_size)
        self.dropout3, self.norm3 = nn.Dropout(pdrop), LayerNorm(hidden_size)

    def forward(self, x, y, x_mask, y_mask, att_pdrop=None, att_drop_topk=None):
        x = self.norm1(x, self.dropout1(self.mhatt1(x, x, x, x_mask)))
        x = self.norm2(x, self.dropout2(self.mhatt2(y, y, x, y_mask, att_pdrop, att_drop_topk)))
        return self.norm3(x, self.dropout3(self.ffn(x)))


class AttFlat(nn.Module):
    """attention pooling over the tokens (mcan_module.py:74-133): softmax over MLP(x) per glimpse, masked keys at -1e9, the
    glimpses' weighted sums concatenated and merged.  x_mask (B, 1, 1, N) bool, True = hide.  The att_pdrop > 0 top-k masking
    has no flag in scripts/train.py (ScanQA's att_pdrop stays 0) and is not carried."""

    def __init__(self, hidden_size, flat_mlp_size=512, flat_glimpses=1, flat_out_size=1024, pdrop=0.1):
        super().__init__()
        self.mlp = MLP(in_size=hidden_size, mid_size=flat_mlp_size, out_size=flat_glimpses, pdrop=pdrop, use_gelu=True)
        self.flat_glimpses = flat_glimpses
        self.linear_merge = nn.Linear(hidden_size * flat_glimpses, flat_out_size)

    def _fused_ok(self, x, att, x_mask):
        if not (_FUSED and _f32_cuda(x, att) and x.dim() == 3 and x.numel() > 0):
            return False
        if x_mask is not None and not (x_mask.dtype == torch.bool and x_mask.is_cuda and x_mask.device == x.device
                                       and x_mask.numel() == x.shape[0] * x.shape[1]):
            return False
        from . import _ext
        return (_ext.mcan_hidden_ok(x.shape[2]) and 1 <= x.shape[1] <= _ext.MCAN_MAX_N
                and 1 <= self.flat_glimpses <= _ext.MCAN_MAX_G)

    def forward(self, x, x_mask, att_pdrop=0, att_drop_topk=100):
        if att_pdrop > 0:
            raise NotImplementedError("AttFlat: att_pdrop > 0 (top-k score masking) is not supported")
        att = self.mlp(x)
        if self._fused_ok(x, att, x_mask):
            hide = x_mask.reshape(x.shape[0], x.shape[1]).contiguous().view(torch.uint8) if x_mask is not None else None
            return self.linear_merge(_AttFlatPoolFn.apply(x, att, hide))
        if x_mask is not None:
            att = att.masked_fill(x_mask.squeeze(1).squeeze(1).unsqueeze(2), -1e9)
        att = F.softmax(att, dim=1)
        x_atted = torch.cat([torch.sum(att[:, :, i:i + 1] * x, dim=1) for i in range(self.flat_glimpses)], dim=1)
        return self.linear_merge(x_atted)


class MCAN_E(nn.Module):
    def __init__(self, hidden_size, num_heads=8, num_layers=6, pdrop=0.1):
        super().__init__()
        self.enc_list = nn.ModuleList([SA(hidden_size, num_heads, pdrop) for _ in range(num_layers)])

    def forward(self, x, x_mask):
        for enc in self.enc_list:
            x = enc(x, x_mask)
        return x


class MCAN_ED(nn.Module):
    """encoder over x (self-attention), then decoder over y guided by the encoded x (mcan_module.py:330-355)"""

    def __init__(self, hidden_size, num_heads=8, num_layers=6, pdrop=0.1):
        super().__init__()
        self.enc_list = nn.ModuleList([SA(hidden_size, num_heads, pdrop) for _ in range(num_layers)])
        self.dec_list = nn.ModuleList([SGA(hidden_size, num_heads, pdrop) for _ in range(num_layers)])

    def forward(self, x, y, x_mask, y_mask, att_pdrop=0, att_drop_topk=100):
        for enc in self.enc_list:
            x = enc(x, x_mask)
        for dec in self.dec_list:
            y = dec(y, x, y_mask, x_mask, att_pdrop, att_drop_topk)
        return x, y
