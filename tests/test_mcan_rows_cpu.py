"""The row operators of the MCAN blocks (csrc/mcan.hip) without a GPU: the fp64 references of tests/mcan_ref.py equal the modules
of bridgeqa_amd/mcan_module.py run in double with autograd, the fp32 emulations of the kernels stay inside the per-element bounds,
planted defects break them, the interface exists from the header to the module switch, and with the switch off -- or on, with
host tensors -- the modules compute bit for bit what they computed before the switch existed."""
import pytest
import torch

import mcan_ref as R
from bridgeqa_amd import mcan_module

WORST = {}


def _ratio(name, out, ref, tol, rows=None):
    if rows is not None:
        out, ref, tol = out[rows], ref[rows], tol[rows]
    r, msg = R.excess(out, ref, tol)
    assert msg is None, "%s: %s" % (name, msg)
    WORST[name] = max(WORST.get(name, 0.0), r)
    return r


def _breaks(out, ref, tol, rows=None):
    if rows is not None:
        out, ref, tol = out[rows], ref[rows], tol[rows]
    return R.excess(out, ref, tol)[1] is not None


_old_layernorm, _old_attflat_tail = R.composition_layernorm, R.composition_attflat_tail


def _old_attflat(m, x, x_mask):
    return m.linear_merge(_old_attflat_tail(m.mlp(x), x, x_mask, m.flat_glimpses))


# ---- the references are the modules ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, H", [(5, 64), (7, 256)])
@pytest.mark.parametrize("with_s", [True, False])
def test_layernorm_reference_equals_the_module_in_double(M, H, with_s):
    d = R.ln_inputs(M, H)
    keep = R.regular_rows(M)
    x = d["x"][keep].double().requires_grad_(True)
    s = d["s"][keep].double().requires_grad_(True) if with_s else None
    dy = d["dy"][keep].double()
    m = mcan_module.LayerNorm(H, eps=R.eps32()).double()
    with torch.no_grad():
        m.a_2.copy_(d["a2"])
        m.b_2.copy_(d["b2"])
    y = m(x, s) if with_s else m(x)
    y.backward(dy)
    x32, s32 = d["x"][keep], (d["s"][keep] if with_s else None)
    ref = R.ln_forward(x32, s32, d["a2"], d["b2"])
    assert (ref["y"] - y.detach()).abs().max() <= 1e-11
    # the backward reference takes mean and sigma as given: hand it the exact ones (as fp64 tensors)
    bwd = R.ln_backward(d["dy"][keep], x32, s32, d["a2"], ref["mean"], ref["sigma"])
    assert (bwd["dz"] - x.grad).abs().max() <= 1e-11
    if with_s:
        assert torch.equal(x.grad, s.grad)
    assert (bwd["da2"] - m.a_2.grad).abs().max() <= 1e-11 and (bwd["db2"] - m.b_2.grad).abs().max() <= 1e-11


def test_constant_row_gives_b2_and_a_nan_gradient_in_the_module():
    """what the kernels must reproduce: sigma = 0 is not guarded"""
    H = 64
    m = mcan_module.LayerNorm(H)
    with torch.no_grad():
        m.b_2.copy_(torch.randn(H))
    x = torch.full((1, H), 1.5, requires_grad=True)
    y = m(x, torch.full((1, H), 0.5))
    assert torch.equal(y[0], m.b_2)
    y.sum().backward()
    assert torch.isnan(x.grad).all()
    y_emu, _, sigma = R.emulate_ln_forward(x.detach(), torch.full((1, H), 0.5), m.a_2.detach(), m.b_2.detach())
    assert torch.equal(y_emu[0], m.b_2) and float(sigma) == 0.0


@pytest.mark.parametrize("N, G, H", [(37, 2, 64), (1, 1, 64), (256, 2, 64)])
@pytest.mark.parametrize("kind", R.MASKS)
def test_pool_reference_equals_the_attflat_tail_in_double(N, G, H, kind):
    B = 3
    d = R.pool_inputs(B, N, G, H)
    hide = R.pool_hide(B, N, kind)
    x = d["x"].double().requires_grad_(True)
    logits = d["logits"].double().requires_grad_(True)
    mask = hide.view(B, 1, 1, N) if hide is not None else None
    out = _old_attflat_tail(logits, x, mask, G)
    out.backward(d["dout"].double())
    ref = R.pool_forward(d["x"], d["logits"], hide)
    assert (ref["out"] - out.detach()).abs().max() <= 1e-11
    if hide is not None:
        assert torch.allclose(ref["p"][1], torch.full((N, G), 1.0 / N, dtype=torch.float64), rtol=0, atol=1e-15)   # uniform
    bwd = R.pool_backward(d["dout"], d["x"], ref["p"], hide)           # p given: the exact one
    assert (bwd["dx"] - x.grad).abs().max() <= 1e-11
    assert (bwd["dl"] - logits.grad).abs().max() <= 1e-11              # the hidden positions included
    if hide is not None:
        assert (logits.grad[hide] == 0).all() and (bwd["dl"][hide] == 0).all()


# ---- the emulations stay inside the bounds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, H", R.LN_SHAPES)
@pytest.mark.parametrize("with_s", [True, False])
def test_layernorm_emulation_stays_within_the_bound(M, H, with_s):
    """Largest |err| / bound over all shapes, with and without s (fp32 emulation on the host):
        y 0.0558  mean 0.0104  sigma 0.0406  dz 0.0895  da2 0.663  db2 0.125
    -- far below 1 because the bounds hold for ANY order of a row's additions and this order (at most 16 serial terms, a
    6-level tree) is short; da2 and db2 come closest at M = 1, where nothing is summed and the roundings of one product are
    all there is."""
    d = R.ln_inputs(M, H)
    s = d["s"] if with_s else None
    rows = R.regular_rows(M)
    ref = R.ln_forward(d["x"], s, d["a2"], d["b2"])
    y, mean, sigma = R.emulate_ln_forward(d["x"], s, d["a2"], d["b2"])
    _ratio("ln_y", y, ref["y"], ref["tol_y"], rows)
    _ratio("ln_mean", mean, ref["mean"], ref["tol_mean"], rows)
    _ratio("ln_sigma", sigma, ref["sigma"], ref["tol_sigma"], rows)
    if M > R.CONST_ROW:
        assert torch.equal(y[R.CONST_ROW], d["b2"]) and float(sigma[R.CONST_ROW]) == 0.0
    b = R.ln_bwd_inputs(M, H, with_s)
    if b["x"].shape[0] == 0:
        return
    ref = R.ln_backward(b["dy"], b["x"], b["s"], b["a2"], b["mean"], b["sigma"])
    dz, da2, db2 = R.emulate_ln_backward(b["dy"], b["x"], b["s"], b["a2"], b["mean"], b["sigma"])
    assert torch.isfinite(dz).all()
    _ratio("ln_dz", dz, ref["dz"], ref["tol_dz"])
    _ratio("ln_da2", da2, ref["da2"], ref["tol_da2"])
    _ratio("ln_db2", db2, ref["db2"], ref["tol_db2"])


@pytest.mark.parametrize("B, N, G, H", R.POOL_SHAPES)
@pytest.mark.parametrize("kind", R.MASKS)
def test_pool_emulation_stays_within_the_bound(B, N, G, H, kind):
    """Largest |err| / bound over all shapes and both masks (fp32 emulation on the host):
        p 0.179  out 0.0689  dx 0.484  dl 0.00819
    (dx at G = 1 is one product held to 3 u)"""
    d = R.pool_inputs(B, N, G, H)
    hide = R.pool_hide(B, N, kind)
    ref = R.pool_forward(d["x"], d["logits"], hide)
    out, p = R.emulate_pool_forward(d["x"], d["logits"], hide)
    _ratio("pool_p", p, ref["p"], ref["tol_p"])
    _ratio("pool_out", out, ref["out"], ref["tol_out"])
    if hide is not None:
        assert (p[1] == p[1, 0, 0]).all() and abs(float(p[1, 0, 0]) - 1.0 / N) <= 2 * R.U / N      # uniform under a full mask
    p32 = R.pool_p32(d["logits"], hide)
    ref = R.pool_backward(d["dout"], d["x"], p32, hide)
    dx, dl = R.emulate_pool_backward(d["dout"], d["x"], p32, hide)
    _ratio("pool_dx", dx, ref["dx"], ref["tol_dx"])
    _ratio("pool_dl", dl, ref["dl"], ref["tol_dl"])
    if hide is not None:
        assert (dl[hide] == 0).all()


# ---- planted defects break the bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M, H", [(5, 64), (5, 1024), (67, 256)])
def test_planted_layernorm_defects_break_the_bound(M, H):
    d = R.ln_inputs(M, H)
    rows = R.regular_rows(M)
    ref = R.ln_forward(d["x"], d["s"], d["a2"], d["b2"])
    # divisor H instead of H - 1: sigma and y, on every row
    y, _, sigma = R.emulate_ln_forward(d["x"], d["s"], d["a2"], d["b2"], defect="divisor_H")
    assert _breaks(sigma, ref["sigma"], ref["tol_sigma"], rows) and _breaks(y, ref["y"], ref["tol_y"], rows)
    # sqrt(var + eps) instead of sigma + eps: row 2 (scaled by 1e-3) is the row built for it
    y, _, _ = R.emulate_ln_forward(d["x"], d["s"], d["a2"], d["b2"], defect="eps_in_sqrt")
    assert _breaks(y[2:3], ref["y"][2:3], ref["tol_y"][2:3])
    # a 16-bit rounding of c: forward and backward
    y, _, _ = R.emulate_ln_forward(d["x"], d["s"], d["a2"], d["b2"], defect="c_16bit")
    assert _breaks(y, ref["y"], ref["tol_y"], rows)
    b = R.ln_bwd_inputs(M, H)
    ref = R.ln_backward(b["dy"], b["x"], b["s"], b["a2"], b["mean"], b["sigma"])
    dz, da2, _ = R.emulate_ln_backward(b["dy"], b["x"], b["s"], b["a2"], b["mean"], b["sigma"], defect="c_16bit")
    assert _breaks(dz, ref["dz"], ref["tol_dz"]) and _breaks(da2, ref["da2"], ref["tol_da2"])


@pytest.mark.parametrize("N, G, H", [(37, 2, 64), (256, 1, 256)])
def test_planted_pool_defects_break_the_bound(N, G, H):
    B = 3
    d = R.pool_inputs(B, N, G, H)
    hide = R.pool_hide(B, N, "mixed")
    ref = R.pool_forward(d["x"], d["logits"], hide)
    # the fill as -inf: the fully hidden sample (1) is the input built for it
    out, p = R.emulate_pool_forward(d["x"], d["logits"], hide, defect="fill_inf")
    assert _breaks(p[1], ref["p"][1], ref["tol_p"][1]) and _breaks(out[1], ref["out"][1], ref["tol_out"][1])
    assert not _breaks(p[0], ref["p"][0], ref["tol_p"][0])            # a partly hidden sample does not tell the two fills apart
    # dlogits not zeroed under the mask: again the fully hidden sample, where p is 1 / N and not 0
    p32 = R.pool_p32(d["logits"], hide)
    ref = R.pool_backward(d["dout"], d["x"], p32, hide)
    _, dl = R.emulate_pool_backward(d["dout"], d["x"], p32, hide, defect="no_zero")
    assert _breaks(dl[1], ref["dl"][1], ref["tol_dl"][1])
    assert not _breaks(dl[0], ref["dl"][0], ref["tol_dl"][0])         # p = 0 there: the product hides the defect


# ---- the interface exists (fails without the feature) ---------------------------------------------------------------------------
def test_the_interface_exists_from_the_header_to_the_switch():
    from bridgeqa_amd import _cabi, _ext, build
    names = ["bqm_mcan_ln_fwd", "bqm_mcan_ln_bwd_slab_floats", "bqm_mcan_ln_bwd", "bqm_attflat_pool_fwd", "bqm_attflat_pool_bwd"]
    assert "bqhip_mcan.h" in _cabi.ADDITIVE_HEADERS and list(_cabi.MCAN_PROTOS) == names
    assert not set(names) & (set(_cabi.PROTOS) | set(_cabi.ADDITIVE_PROTOS) | set(_cabi.EXTENSION_PROTOS))
    assert _cabi.DEFINES["BQHIP_ABI_VERSION"] == 6
    vp, i, f = _cabi.ctypes.c_void_p, _cabi.ctypes.c_int, _cabi.ctypes.c_float
    assert _cabi.MCAN_PROTOS["bqm_mcan_ln_fwd"] == (i, [vp] * 7 + [i, i, f, vp])
    assert _cabi.MCAN_PROTOS["bqm_mcan_ln_bwd"] == (i, [vp] * 9 + [i, i, f, vp])
    assert _cabi.MCAN_PROTOS["bqm_mcan_ln_bwd_slab_floats"] == (_cabi.ctypes.c_long, [i, i])
    assert _cabi.MCAN_PROTOS["bqm_attflat_pool_fwd"] == (i, [vp] * 5 + [i] * 4 + [vp])
    assert _cabi.MCAN_PROTOS["bqm_attflat_pool_bwd"] == (i, [vp] * 6 + [i] * 4 + [vp])
    for n in names:
        assert getattr(_ext._lib, n).argtypes == _cabi.MCAN_PROTOS[n][1]
    for n in ("mcan_ln_fwd", "mcan_ln_bwd", "attflat_pool_fwd", "attflat_pool_bwd"):
        assert callable(getattr(_ext, n))
    assert callable(mcan_module.set_fused) and mcan_module.fused_enabled() in (False, True)
    # the slab: one (2, H) row per workgroup of 4 rows, capped
    assert _ext._lib.bqm_mcan_ln_bwd_slab_floats(67, 256) == 17 * 2 * 256
    assert _ext._lib.bqm_mcan_ln_bwd_slab_floats(100000, 64) == R.BWD_CAP * 2 * 64
    assert _ext._lib.bqm_mcan_ln_bwd_slab_floats(5, 96) == 0
    # ineligible sizes are BQ_EINVAL before any pointer is looked at
    assert _ext._lib.bqm_mcan_ln_fwd(None, None, None, None, None, None, None, 4, 96, 1e-6, None) == -1
    assert b"H 96" in _ext._lib.bq_last_error()
    assert _ext._lib.bqm_mcan_ln_bwd(None, None, None, None, None, None, None, None, None, 4, 1088, 1e-6, None) == -1
    assert _ext._lib.bqm_attflat_pool_fwd(None, None, None, None, None, 2, 1025, 1, 64, None) == -1
    assert _ext._lib.bqm_attflat_pool_bwd(None, None, None, None, None, None, 2, 8, 5, 64, None) == -1
    assert _ext._lib.bqm_attflat_pool_fwd(None, None, None, None, None, 2, 8, 1, 64, None) == -1        # null pointers
    build.build()
    res = build.kernel_resources()
    if res is None:
        return                                                             # (a prebuilt library: no remarks to read)
    mine = {k: v for k, v in res.items() if "mcan_" in k}
    assert len(mine) == 16 + 16 + 3                                        # LayerNorm forward / backward per H / 64, fold, 2 pool
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0, (k, v)
        assert v.get("lds", 0) <= 32768, (k, v)


def test_the_entry_points_are_exported_and_defined_against_their_declaration():
    """what tests/test_cabi_cpu.py holds the bq_ entry points to, for the bqm_ ones: the exported bqm_ symbols are the declared
    ones, and each definition is a plain `extern "C"` in a source that sees the header through bq_common.h"""
    import os
    import re
    import subprocess
    from bridgeqa_amd import _cabi, _ext
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output(["nm", "-D", "--defined-only", _ext.library_path()]).decode()
    exported = {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[2].startswith("bqm_")}
    assert exported == set(_cabi.MCAN_PROTOS)
    src = re.sub(r"//[^\n]*", "", open(os.path.join(root, "bridgeqa_amd", "csrc", "mcan.hip")).read())
    assert '#include "bq_common.h"' in src
    assert '#include "bqhip_mcan.h"' in open(os.path.join(root, "include", "bqhip_fusion.h")).read()
    for name in _cabi.MCAN_PROTOS:
        heads = re.findall(r"^([^\n;{}]*?)\b%s\s*\(" % name, src, flags=re.M)
        assert heads == ['extern "C" long ' if name.endswith("slab_floats") else 'extern "C" int '], (name, heads)


def test_cpu_tensors_raise_in_the_bindings():
    from bridgeqa_amd import _ext
    x, v = torch.zeros(4, 64), torch.zeros(64)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.mcan_ln_fwd(x, None, v, v, 1e-6)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.mcan_ln_bwd(x, x, None, v, torch.zeros(4), torch.zeros(4), 1e-6)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.attflat_pool_fwd(torch.zeros(2, 4, 64), torch.zeros(2, 4, 1), None)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.attflat_pool_bwd(torch.zeros(2, 64), torch.zeros(2, 4, 64), torch.zeros(2, 4, 1), None)


# ---- nothing changes with the switch off, or on the host with it on -------------------------------------------------------------
@pytest.fixture(params=[False, True], ids=["off", "on_cpu"])
def switch(request):
    prev = mcan_module.set_fused(request.param)
    yield request.param
    mcan_module.set_fused(prev)


def test_default_is_off():
    import os
    if os.environ.get("BQ_MCAN_FUSED", "0") != "1":
        assert mcan_module.fused_enabled() is False
    prev = mcan_module.set_fused(True)
    assert mcan_module.fused_enabled() is True
    mcan_module.set_fused(prev)
    assert mcan_module.fused_enabled() is prev


@pytest.mark.parametrize("H", [256, 96])
def test_layernorm_with_a_residual_is_bitwise_the_composition(switch, H):
    d = dict(R.ln_inputs(5, 256), **{k: R.ln_bwd_inputs(5, 256)[k] for k in ("x", "s")})   # (no constant row: NaN != NaN)
    x, s = d["x"][:, :H].clone().requires_grad_(True), d["s"][:, :H].clone().requires_grad_(True)
    m = mcan_module.LayerNorm(H)
    with torch.no_grad():
        m.a_2.copy_(d["a2"][:H])
        m.b_2.copy_(d["b2"][:H])
    y = m(x, s)
    y.sum().backward()
    x0 = x.detach().clone().requires_grad_(True)
    s0 = s.detach().clone().requires_grad_(True)
    ga = m.a_2.grad.clone()
    m.a_2.grad = None
    y0 = _old_layernorm(m, x0 + s0)
    y0.sum().backward()
    assert torch.equal(y, y0) and torch.equal(x.grad, x0.grad) and torch.equal(s.grad, s0.grad) and torch.equal(ga, m.a_2.grad)
    assert torch.equal(m(x.detach()), _old_layernorm(m, x.detach()))       # and without a residual


def test_attflat_and_the_blocks_are_bitwise_unchanged(switch):
    torch.manual_seed(3)
    B, N, H = 3, 37, 64
    m = mcan_module.AttFlat(H, flat_mlp_size=32, flat_glimpses=2, flat_out_size=48, pdrop=0.0)
    x = torch.randn(B, N, H)
    mask = R.pool_hide(B, N, "mixed").view(B, 1, 1, N)
    assert torch.equal(m(x, mask), _old_attflat(m, x, mask)) and torch.equal(m(x, None), _old_attflat(m, x, None))
    # one SGA layer in training mode: the residual handed to the norm is the dropout's output, drawn as before
    sga = mcan_module.SGA(H, num_heads=4, pdrop=0.1).train()
    y = torch.randn(B, 9, H)
    torch.manual_seed(11)
    out = sga(x, y, None, None)
    torch.manual_seed(11)
    t = _old_layernorm(sga.norm1, x + sga.dropout1(sga.mhatt1(x, x, x, None)))
    t = _old_layernorm(sga.norm2, t + sga.dropout2(sga.mhatt2(y, y, t, None, None, None)))
    t = _old_layernorm(sga.norm3, t + sga.dropout3(sga.ffn(t)))
    assert torch.equal(out, t)
    sa = mcan_module.SA(H, num_heads=4, pdrop=0.1).train()
    torch.manual_seed(12)
    out = sa(x, None)
    torch.manual_seed(12)
    t = _old_layernorm(sa.norm1, x + sa.dropout1(sa.mhatt(x, x, x, None)))
    t = _old_layernorm(sa.norm2, t + sa.dropout2(sa.ffn(t)))
    assert torch.equal(out, t)
