"""Shared cases, runners and the error bound of the LSTM tests (tests/test_lang_branch_cpu.py, tests/test_lstm_gpu.py).

A case is (name, lens, T, layers, bidirectional); with hidden size H and E = 20 it fixes, by seed, the nn.LSTM parameters, the
input x (B, T, E) and the two cotangents G_out (B, max(len), H dirs), G_emb (B, H dirs) of the scalar
    loss = sum(lang_out * G_out) + sum(lang_emb * G_emb)
so that gradient flows through BOTH outputs.  Every runner returns {"out", "emb", "x" (= dX), parameter name: gradient}.

The bound (the issue's): a tensor's error against the fp64 reference may be at most K times the error of torch's own fp32 CPU
nn.LSTM against the same reference plus one fp32 ulp of the reference's largest magnitude.  K was fixed BEFORE any device run:
twice the worst ratio that the fp32 emulation of the kernels' summation order (lstm_ref.emu_lstm) reaches over every case,
hidden size and tensor here, on the CPU (2.0844: H = 256, bidirectional, dX).  test_lang_branch_cpu.py recomputes the ratio and
holds the emulation itself to K (the CPU nn.LSTM's own summation order may differ between hosts, so not to K / 2).
"""
import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_ref

E = 20
LENS = [1, 9, 7, 2, 9]      # unsorted, a length of 1, a tie, max(len) < T
CASES = [
    ("uni", LENS, 12, 1, False),
    ("bidir", LENS, 12, 1, True),
    ("two_layers", LENS, 12, 2, False),
    ("two_layers_bidir", LENS, 12, 2, True),
    ("single_step", [1], 1, 1, False),
    ("single_step_bidir", [1], 1, 1, True),
]
# twice the emulation's worst ratio (EMU_WORST, measured on the CPU by emulation_worst_ratio(); profiles/lang_branch.md)
EMU_WORST = 2.0844
K = 2 * EMU_WORST


def make_case(case, H, seed=0):
    name, lens, T, layers, bidir = case
    g = torch.Generator().manual_seed(seed + 1000 * H + len(name))
    lstm = torch.nn.LSTM(E, H, batch_first=True, num_layers=layers, bidirectional=bidir)
    params = {}
    for n, p in lstm.named_parameters():
        # (larger than the default 1/sqrt(H) init: gates away from the linear regime of sigmoid / tanh)
        params[n] = (torch.rand(p.shape, generator=g, dtype=torch.float64) * 2 - 1) * (2.0 / H ** 0.5)
    B, t_out, D = len(lens), max(lens), H * (2 if bidir else 1)
    x = torch.randn(B, T, E, generator=g, dtype=torch.float64).float().double()
    params = {n: v.float().double() for n, v in params.items()}   # exactly representable in fp32: every runner sees the same
    return dict(name=name, lens=list(lens), T=T, layers=layers, bidir=bidir, H=H, params=params, x=x,
                g_out=torch.randn(B, t_out, D, generator=g, dtype=torch.float64).float().double(),
                g_emb=torch.randn(B, D, generator=g, dtype=torch.float64).float().double())


def emb_of(h_n, layers):
    """lang_emb from h_n (layers dirs, B, H): the last layer's final states, directions side by side (lang_module.py)"""
    L, B, H = h_n.shape
    return h_n.view(layers, -1, B, H)[-1].permute(1, 0, 2).contiguous().flatten(start_dim=1)


def run_torch(c, dtype):
    """torch's CPU nn.LSTM on packed input in `dtype`, gradients by autograd"""
    lstm = torch.nn.LSTM(E, c["H"], batch_first=True, num_layers=c["layers"], bidirectional=c["bidir"]).to(dtype)
    with torch.no_grad():
        for n, p in lstm.named_parameters():
            p.copy_(c["params"][n].to(dtype))
    x = c["x"].to(dtype).clone().requires_grad_(True)
    packed = pack_padded_sequence(x, torch.tensor(c["lens"]), batch_first=True, enforce_sorted=False)
    po, (h_n, _) = lstm(packed)
    out, _ = pad_packed_sequence(po, batch_first=True)
    emb = emb_of(h_n, c["layers"])
    ((out * c["g_out"].to(dtype)).sum() + (emb * c["g_emb"].to(dtype)).sum()).backward()
    res = {"out": out.detach(), "emb": emb.detach(), "x": x.grad}
    res.update({n: p.grad for n, p in lstm.named_parameters()})
    return {k: v.double().numpy() for k, v in res.items()}


def run_emulation(c):
    """the fp32 numpy emulation of the kernels' summation order (lstm_ref.emu_lstm)"""
    dirs = 2 if c["bidir"] else 1
    B, H, L = len(c["lens"]), c["H"], c["layers"]
    g_emb = c["g_emb"].numpy().astype(np.float32)
    d_hn = np.zeros((L * dirs, B, H), np.float32)
    for d in range(dirs):
        d_hn[(L - 1) * dirs + d] = g_emb[:, d * H:(d + 1) * H]
    p = {n: v.numpy() for n, v in c["params"].items()}
    out, h_n, grads = lstm_ref.emu_lstm(c["x"].numpy(), c["lens"], p, L, c["bidir"], d_out=c["g_out"].numpy(), d_hn=d_hn)
    res = {"out": out, "emb": emb_of(torch.from_numpy(h_n), L).numpy()}
    res.update(grads)
    return {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}


def run_module(c, device, lang_module_cls):
    """bridgeqa_amd's LangModule (fused route on a device) in fp32; returns the result dict and the module outputs"""
    m = lang_module_cls(18, use_lang_classifier=False, use_bidir=c["bidir"], num_layers=c["layers"], emb_size=E,
                        hidden_size=c["H"], pdrop=0.0).to(device).eval()
    with torch.no_grad():
        for n, p in m.lstm.named_parameters():
            p.copy_(c["params"][n].float())
    x = c["x"].float().to(device).clone().requires_grad_(True)
    dd = m({"lang_feat": x, "lang_len": torch.tensor(c["lens"])})
    ((dd["lang_out"] * c["g_out"].float().to(device)).sum() + (dd["lang_emb"] * c["g_emb"].float().to(device)).sum()).backward()
    res = {"out": dd["lang_out"].detach(), "emb": dd["lang_emb"].detach(), "x": x.grad[:, :max(c["lens"])]}
    res.update({n: p.grad for n, p in m.lstm.named_parameters()})
    return {k: v.double().cpu().numpy() for k, v in res.items()}, dd


def _max_diff(a, ref):
    """max |a - ref|; dX may be given for the first max(len) steps only: the reference is zero beyond them (asserted)"""
    if a.shape != ref.shape:
        assert a.ndim == 3 and a.shape[0] == ref.shape[0] and a.shape[2] == ref.shape[2] and a.shape[1] <= ref.shape[1]
        assert not ref[:, a.shape[1]:].any()
        ref = ref[:, :a.shape[1]]
    return float(np.abs(a - ref).max())


def errors(got, ref, cpu32):
    """per tensor: (error of `got`, error of the fp32 CPU nn.LSTM, one fp32 ulp of the reference's largest magnitude)"""
    out = {}
    for k in ref:
        ulp = float(np.spacing(np.float32(np.abs(ref[k]).max())))
        out[k] = (_max_diff(got[k], ref[k]), _max_diff(cpu32[k], ref[k]), ulp)
    return out


def ratio(err, err_cpu, ulp):
    """how many CPU-fp32 errors the error is, after the ulp allowance (the quantity K bounds)"""
    over = max(0.0, err - ulp)
    return 0.0 if over == 0.0 else (over / err_cpu if err_cpu > 0 else float("inf"))


def emulation_worst_ratio(hidden=(128, 256)):
    worst, where = 0.0, None
    for H in hidden:
        for case in CASES:
            c = make_case(case, H)
            ref, cpu32, emu = run_torch(c, torch.float64), run_torch(c, torch.float32), run_emulation(c)
            for k, e in errors(emu, ref, cpu32).items():
                r = ratio(*e)
                if r > worst:
                    worst, where = r, (H, case[0], k) + e
    return worst, where


if __name__ == "__main__":
    print(emulation_worst_ratio())
