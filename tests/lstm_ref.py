"""References for the LSTM kernels of bridgeqa_amd/csrc/lstm.hip (tests only; numpy, no torch).

  lstm_ref(x, lens, params, ...)       fp64, the packed-sequence contract of nn.LSTM(batch_first=True) over
                                       pack_padded_sequence(enforce_sorted=False) + pad_packed_sequence: output (B, max(len), H dirs)
                                       with zeros beyond each length, h_n (layers dirs, B, H) = the last valid state of every
                                       (layer, direction) -- for the reverse direction the state after step 0.
  emu_direction / emu_direction_bwd    fp32 emulation of ONE (layer, direction) as the kernels sum it: four interleaved chains
                                       over k (k mod 4) added as (a0 + a1) + (a2 + a3), every product and sum rounded separately,
                                       the four gates' partial sums of the backward added as (p0 + p1) + (p2 + p3).  exp / tanh are
                                       numpy's fp32 routines (the device's expf / tanhf differ from them in the last place).
  emu_lstm(x, lens, params, ...)       the stacked / bidirectional loop of lang_module.lstm_fused over emu_direction, with the
                                       gradients of every parameter and of x for given dOut / dH_n (GEMMs in fp32 numpy).

params: {"weight_ih_l0": (4H, E), "weight_hh_l0": (4H, H), "bias_ih_l0": (4H,), "bias_hh_l0": (4H,), ..._reverse, ..._l1}: the
names of nn.LSTM.  Gate order i f g o.
"""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _sfx(layer, d):
    return "_l%d%s" % (layer, "_reverse" if d else "")


def ref_direction(x, lens, w_ih, w_hh, b_ih, b_hh, reverse, t_out):
    """fp64, one layer and direction: y (B, t_out, H), h_last (B, H)"""
    B, H = x.shape[0], w_hh.shape[1]
    y = np.zeros((B, t_out, H))
    h_last = np.zeros((B, H))
    for b in range(B):
        h, c = np.zeros(H), np.zeros(H)
        n = int(lens[b])
        for t in (range(n - 1, -1, -1) if reverse else range(n)):
            pre = w_ih @ x[b, t] + b_ih + w_hh @ h + b_hh
            i, f, g, o = _sig(pre[:H]), _sig(pre[H:2 * H]), np.tanh(pre[2 * H:3 * H]), _sig(pre[3 * H:])
            c = f * c + i * g
            h = o * np.tanh(c)
            y[b, t] = h
        h_last[b] = h
    return y, h_last


def lstm_ref(x, lens, params, num_layers=1, bidirectional=False):
    """fp64 reference of the whole nn.LSTM: out (B, max(len), H dirs), h_n (layers dirs, B, H)"""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    inp = np.asarray(x, dtype=np.float64)
    t_out = int(max(lens))
    h_n = []
    for layer in range(num_layers):
        outs = []
        for d in range(2 if bidirectional else 1):
            s = _sfx(layer, d)
            y, hl = ref_direction(inp, lens, p["weight_ih" + s], p["weight_hh" + s], p["bias_ih" + s], p["bias_hh" + s], bool(d),
                                  t_out)
            outs.append(y)
            h_n.append(hl)
        inp = np.concatenate(outs, -1)
    return inp, np.stack(h_n)


# ---- fp32 emulation of the kernels' summation order ---------------------------------------------------------------------------
f32 = np.float32


def _chains(prod):
    """prod (..., K) fp32 products -> their sum as the kernels form it: chain q adds k = q, q + 4, ... in order from zero,
    then (a0 + a1) + (a2 + a3)"""
    K = prod.shape[-1]
    a = np.zeros(prod.shape[:-1] + (4,), dtype=f32)
    for k in range(0, K, 4):
        a = (a + prod[..., k:k + 4]).astype(f32)
    return ((a[..., 0] + a[..., 1]).astype(f32) + (a[..., 2] + a[..., 3]).astype(f32)).astype(f32)


def emu_direction(gx, w_hh, lens, reverse, t_out):
    """gx (B, T, 4H) fp32 = x W_ih^T + b_ih + b_hh; returns y, h_last, gates (post-activation), cells as lstm_fwd_kernel"""
    gx, w_hh = gx.astype(f32), w_hh.astype(f32)
    B, H = gx.shape[0], w_hh.shape[1]
    y = np.zeros((B, t_out, H), f32)
    gates = np.zeros((B, t_out, 4 * H), f32)
    cells = np.zeros((B, t_out, H), f32)
    h_last = np.zeros((B, H), f32)
    one = f32(1.0)
    for b in range(B):
        h, c = np.zeros(H, f32), np.zeros(H, f32)
        n = min(max(int(lens[b]), 0), t_out)
        for t in (range(n - 1, -1, -1) if reverse else range(n)):
            pre = (gx[b, t] + _chains((w_hh * h[None, :]).astype(f32))).astype(f32)   # column j: sum_k h[k] W_hh[j, k]
            a = np.empty(4 * H, f32)
            for q in (0, 1, 3):
                a[q * H:(q + 1) * H] = (one / (one + np.exp(-pre[q * H:(q + 1) * H]).astype(f32)).astype(f32)).astype(f32)
            a[2 * H:3 * H] = np.tanh(pre[2 * H:3 * H]).astype(f32)
            c = ((a[H:2 * H] * c).astype(f32) + (a[:H] * a[2 * H:3 * H]).astype(f32)).astype(f32)
            h = (a[3 * H:] * np.tanh(c).astype(f32)).astype(f32)
            y[b, t], gates[b, t], cells[b, t] = h, a, c
        h_last[b] = h
    return y, h_last, gates, cells


def emu_direction_bwd(dy, dh_last, gates, cells, w_hh, lens, reverse):
    """dgx (B, t_out, 4H) as lstm_bwd_kernel forms it"""
    w_hh = w_hh.astype(f32)
    B, t_out, H = cells.shape
    dgx = np.zeros((B, t_out, 4 * H), f32)
    one = f32(1.0)
    for b in range(B):
        n = min(max(int(lens[b]), 0), t_out)
        dh_rec, dc = np.zeros(H, f32), np.zeros(H, f32)
        for s in range(n):
            sf = n - 1 - s
            t = n - 1 - sf if reverse else sf
            dh = (dy[b, t] + dh_rec).astype(f32) if dy is not None else dh_rec
            if s == 0 and dh_last is not None:
                dh = (dh + dh_last[b]).astype(f32)
            gi, gf, gg, go = (gates[b, t, q * H:(q + 1) * H] for q in range(4))
            cc = cells[b, t]
            cp = cells[b, t + 1 if reverse else t - 1] if sf > 0 else np.zeros(H, f32)
            tc = np.tanh(cc).astype(f32)
            d_o = (dh * tc).astype(f32)
            dc = (dc + ((dh * go).astype(f32) * (one - (tc * tc).astype(f32)).astype(f32)).astype(f32)).astype(f32)
            di, dg, df = (dc * gg).astype(f32), (dc * gi).astype(f32), (dc * cp).astype(f32)
            dc = (dc * gf).astype(f32)
            ai = ((di * gi).astype(f32) * (one - gi).astype(f32)).astype(f32)
            af = ((df * gf).astype(f32) * (one - gf).astype(f32)).astype(f32)
            ag = (dg * (one - (gg * gg).astype(f32)).astype(f32)).astype(f32)
            ao = ((d_o * go).astype(f32) * (one - go).astype(f32)).astype(f32)
            d = np.concatenate([ai, af, ag, ao]).astype(f32)
            dgx[b, t] = d
            if sf > 0:
                # thread (q, k): sum over the H rows r = q H + m of gate q of d[r] W_hh[r, k], four chains over m
                prod = (w_hh.reshape(4, H, H) * d.reshape(4, H, 1)).astype(f32)        # (q, m, k)
                part = _chains(np.transpose(prod, (0, 2, 1)))                          # (q, k)
                dh_rec = ((part[0] + part[1]).astype(f32) + (part[2] + part[3]).astype(f32)).astype(f32)
    return dgx


def emu_lstm(x, lens, params, num_layers=1, bidirectional=False, d_out=None, d_hn=None):
    """fp32 emulation of lang_module.lstm_fused (eval mode: no inter-layer dropout).  Returns out, h_n and, when d_out / d_hn
    ((B, max(len), H dirs) / (layers dirs, B, H)) are given, {"x": dX, parameter name: gradient}."""
    p = {k: np.asarray(v, dtype=f32) for k, v in params.items()}
    dirs = 2 if bidirectional else 1
    t_out = int(max(lens))
    inp = np.asarray(x, dtype=f32)[:, :t_out]
    B = inp.shape[0]
    saved, h_n = [], []
    for layer in range(num_layers):
        outs = []
        for d in range(dirs):
            s = _sfx(layer, d)
            bias = (p["bias_ih" + s] + p["bias_hh" + s]).astype(f32)
            gx = (inp.reshape(B * t_out, -1) @ p["weight_ih" + s].T + bias).astype(f32).reshape(B, t_out, -1)
            y, hl, gates, cells = emu_direction(gx, p["weight_hh" + s], lens, bool(d), t_out)
            saved.append((inp, y, gates, cells))
            outs.append(y)
            h_n.append(hl)
        inp = np.concatenate(outs, -1)
    out, h_n = inp, np.stack(h_n)
    if d_out is None and d_hn is None:
        return out, h_n
    H = h_n.shape[-1]
    grads = {}
    d_inp = np.asarray(d_out, dtype=f32) if d_out is not None else np.zeros_like(out)
    for layer in range(num_layers - 1, -1, -1):
        d_prev = None
        for d in range(dirs):
            s = _sfx(layer, d)
            xin, y, gates, cells = saved[layer * dirs + d]
            dy = np.ascontiguousarray(d_inp[..., d * H:(d + 1) * H])
            dhl = np.asarray(d_hn[layer * dirs + d], dtype=f32) if d_hn is not None else None
            dgx = emu_direction_bwd(dy, dhl, gates, cells, p["weight_hh" + s], lens, bool(d))
            d2 = dgx.reshape(B * t_out, 4 * H)
            hprev = np.zeros_like(y)
            if t_out > 1:
                if d:
                    hprev[:, :-1] = y[:, 1:]
                else:
                    hprev[:, 1:] = y[:, :-1]
            grads["weight_ih" + s] = (d2.T @ xin.reshape(B * t_out, -1)).astype(f32)
            grads["weight_hh" + s] = (d2.T @ hprev.reshape(B * t_out, H)).astype(f32)
            grads["bias_ih" + s] = grads["bias_hh" + s] = d2.sum(0, dtype=f32)
            dx = (d2 @ p["weight_ih" + s]).astype(f32).reshape(B, t_out, -1)
            d_prev = dx if d_prev is None else (d_prev + dx).astype(f32)
        d_inp = d_prev
    grads["x"] = d_inp
    return out, h_n, grads
