"""The stage-1 question branch without a GPU: the fp64 LSTM reference against torch, the fp32 emulation of the kernels against
the bound the device is held to, LangModule's fallback / AttFlat / MCAN_E / MCAN_ED / the branch of ScanQAHotPath against goldens
recorded from the reference's own modules (tools/gen_golden_lang.py -> tests/golden/lang_branch.npz; weights by
golden_util.fill_params, i.e. equal iff key names and shapes are), state-dict key parity, eligibility and errors, and the new
kernels' compile-time resources.

Tolerances: the modules here run the same torch CPU operators in the same order as the reference's, so the differences are
expected to be zero; what is ALLOWED is fp32 round-off: for the LSTM four times the reference's own fp32-vs-fp64 gap recorded in
the fixture (1.3e-7 / 8.8e-8), for the MCAN stacks 1e-5 absolute on outputs of magnitude <= 4 (a few hundred fp32 roundings of
2^-24 each through two layers)."""
import numpy as np
import pytest
import torch

import lstm_cases as lc
import lstm_ref
from golden_util import fill_params

MCAN_ATOL = 1e-5


def _keys(module, prefix=""):
    return ["%s%s %s" % (prefix, k, "x".join(map(str, v.shape))) for k, v in module.state_dict().items()]


@pytest.fixture(scope="module")
def G(golden):
    return golden("lang_branch.npz")


# ---- references -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES, ids=[c[0] for c in lc.CASES])
def test_fp64_reference_equals_torch_double_lstm(case):
    c = lc.make_case(case, 128)
    ref = lc.run_torch(c, torch.float64)
    out, h_n = lstm_ref.lstm_ref(c["x"].numpy(), c["lens"], {k: v.numpy() for k, v in c["params"].items()}, c["layers"], c["bidir"])
    emb = lc.emb_of(torch.from_numpy(h_n), c["layers"]).numpy()
    assert out.shape == ref["out"].shape == (len(c["lens"]), max(c["lens"]), 128 * (2 if c["bidir"] else 1))
    assert np.abs(out - ref["out"]).max() < 1e-14 and np.abs(emb - ref["emb"]).max() < 1e-14   # |h| < 1: a few ulps of double
    for b, n in enumerate(c["lens"]):
        assert not out[b, n:].any()


def test_emulation_of_the_kernels_holds_the_device_bound():
    """K is twice the emulation's worst ratio (lstm_cases.EMU_WORST, fixed before any device run); the emulation itself must
    stay inside K wherever it is recomputed"""
    assert lc.K == 2 * lc.EMU_WORST
    worst, where = lc.emulation_worst_ratio()
    print("emulation worst ratio %.4f at %s (recorded %.4f, K = %.4f)" % (worst, where, lc.EMU_WORST, lc.K))
    assert worst <= lc.K, where


# ---- LangModule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kw", [("uni", dict(use_bidir=False, num_layers=1)), ("bi2", dict(use_bidir=True, num_layers=2))])
def test_lang_module_fallback_matches_the_reference(G, tag, kw):
    from bridgeqa_amd import _ext
    from bridgeqa_amd.lang_module import LangModule
    m = LangModule(18, use_lang_classifier=True, emb_size=20, hidden_size=128, **kw).eval()
    assert _keys(m) == G["lm_%s_keys" % tag].tolist()
    fill_params(m, "lm_%s." % tag)
    before = list(_ext.LSTM_CALLS)
    lens = torch.from_numpy(G["lm_lang_len"])
    assert lens.tolist() == [1, 9, 7, 2, 9] and G["lm_lang_feat"].shape == (5, 12, 20)
    with torch.no_grad():
        d = m({"lang_feat": torch.from_numpy(G["lm_lang_feat"]), "lang_len": lens})
    assert _ext.LSTM_CALLS == before                                  # CPU: the held nn.LSTM
    D = 128 * (2 if kw["use_bidir"] else 1)
    assert d["lang_out"].shape == (5, 9, D) and d["lang_emb"].shape == (5, D)
    assert np.array_equal(d["lang_mask"].numpy(), G["lm_%s_lang_mask" % tag])
    assert d["lang_mask"].tolist() == [[t >= n for t in range(9)] for n in lens.tolist()]
    tol = 4 * float(G["lm_%s_gap64" % tag])
    for k in ("lang_out", "lang_emb", "lang_scores"):
        assert np.abs(d[k].numpy() - G["lm_%s_%s" % (tag, k)]).max() <= tol, k


def test_lang_module_eligibility_and_errors(monkeypatch):
    from bridgeqa_amd import _ext, lang_module
    from bridgeqa_amd.lang_module import LangModule
    before = list(_ext.LSTM_CALLS)
    m = LangModule(18, emb_size=20, hidden_size=100).eval()           # H = 100 is not built: fallback wherever it runs
    x = torch.randn(2, 6, 20)
    assert not lang_module.lstm_eligible(m.lstm, x) and not lang_module.lstm_eligible(LangModule(18, emb_size=20).lstm, x)
    assert not lang_module.lstm_eligible(LangModule(18, emb_size=20).double().lstm, x.double())
    d = m({"lang_feat": x, "lang_len": torch.tensor([6, 3])})
    assert d["lang_out"].shape == (2, 6, 100) and d["lang_scores"].shape == (2, 18) and _ext.LSTM_CALLS == before
    with pytest.raises(ValueError, match="at least 1"):
        m({"lang_feat": x, "lang_len": torch.tensor([6, 0])})
    with pytest.raises(NotImplementedError):
        LangModule(18, bert_model_name="bert-base-uncased")
    monkeypatch.setenv("BQ_LSTM_FUSED", "0")
    assert not lang_module.fused_enabled()
    monkeypatch.setenv("BQ_LSTM_FUSED", "1")
    assert lang_module.fused_enabled()
    monkeypatch.delenv("BQ_LSTM_FUSED")
    assert lang_module.fused_enabled() == lang_module.FUSED_DEFAULT


def test_wrappers_reject_host_tensors_without_launching():
    from bridgeqa_amd import _ext
    before = list(_ext.LSTM_CALLS)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.lstm_fwd(torch.zeros(1, 2, 512), torch.zeros(128, 512), torch.ones(1, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.lstm_bwd(None, None, torch.zeros(1, 2, 512), torch.zeros(1, 2, 128), torch.zeros(512, 128),
                      torch.ones(1, dtype=torch.int32))
    assert _ext.LSTM_CALLS == before
    # the library refuses an unsupported hidden size and null pointers with a status, before any launch
    assert _ext._lib.bq_lstm_fwd(None, None, None, None, None, None, None, 1, 2, 2, 100, 0, None) == -1
    assert b"hidden size 100" in _ext._lib.bq_last_error()
    assert _ext._lib.bq_lstm_fwd(None, None, None, None, None, None, None, 1, 2, 2, 128, 0, None) == -1
    assert _ext._lib.bq_lstm_bwd(None, None, None, None, None, None, None, 1, 2, 256, 0, None) == -1
    assert _ext._lib.bq_lstm_fwd(None, None, None, None, None, None, None, 0, 2, 2, 128, 0, None) == 0   # empty batch


# ---- AttFlat / MCAN_E / MCAN_ED ----------------------------------------------------------------------------------------------
def test_attflat_and_mcan_stacks_match_the_reference(G):
    from bridgeqa_amd.mcan_module import MCAN_E, MCAN_ED, AttFlat
    x, y = torch.from_numpy(G["mc_x"]), torch.from_numpy(G["mc_y"])
    x_mask, y_mask = torch.from_numpy(G["mc_x_mask"]), torch.from_numpy(G["mc_y_mask"])
    assert x_mask.any() and y_mask.any() and not x_mask.all() and not y_mask.all()      # both masks in use
    af = AttFlat(32, flat_mlp_size=48, flat_glimpses=2, flat_out_size=40, pdrop=0.1).eval()
    e = MCAN_E(32, num_heads=8, num_layers=2, pdrop=0.1).eval()
    ed = MCAN_ED(32, num_heads=8, num_layers=2, pdrop=0.1).eval()
    for m, tag in ((af, "af"), (e, "e"), (ed, "ed")):
        assert _keys(m) == G[tag + "_keys"].tolist()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        fill_params(m, tag + ".")
    with torch.no_grad():
        got = {"af_out_x": af(x, x_mask), "af_out_y": af(y, y_mask), "af_out_nomask": af(x, None), "e_out": e(y, y_mask)}
        got["ed_out_x"], got["ed_out_y"] = ed(x, y, x_mask, y_mask)
    for k, v in got.items():
        assert v.shape == G[k].shape and np.abs(G[k]).max() <= 4
        assert np.abs(v.numpy() - G[k]).max() <= MCAN_ATOL, k
    with pytest.raises(NotImplementedError):
        af(x, x_mask, att_pdrop=0.1)


# ---- ScanQAHotPath(lang_branch=True) ------------------------------------------------------------------------------------------
def test_hotpath_branch_keys_are_the_references_and_default_is_unchanged(G):
    from bridgeqa_amd.hotpath import ScanQAHotPath
    base = ScanQAHotPath(input_feature_dim=1, num_proposal=16, use_blip=False)
    base_keys = list(base.state_dict())
    full = ScanQAHotPath(input_feature_dim=1, num_proposal=16, use_blip=False, lang_branch=True, num_answers=30)
    keys = _keys(full)
    new = [k for k in keys if k.split(" ")[0] not in base_keys]
    assert new == G["branch_default_keys"].tolist()                   # names, shapes AND registration order (hidden 256 default)
    assert [k.split(" ")[0] for k in keys][:len(base_keys)] == base_keys
    assert [n for n, _ in full.named_children()][-9:] == ["object_cls", "lang_net", "lang_feat_linear", "lang_cls", "attflat_visual",
                                                         "attflat_lang", "answer_cls", "fusion_backbone", "fusion_norm"]
    # absent argument: the tree of before (no branch module, no flag attribute)
    assert [n for n, _ in base.named_children()] == ["detection_backbone", "voting_net", "proposal_net", "object_feat_linear"]
    assert not hasattr(base, "lang_branch") and not hasattr(base, "lang_net")
    with pytest.raises(ValueError):
        ScanQAHotPath(input_feature_dim=1, use_blip=False, lang_branch=True)              # num_answers has no default
    # a model with the branch is never handed to graph replay
    from bridgeqa_amd import graphed, pipeline
    runner = graphed.GraphedRunner.__new__(graphed.GraphedRunner)
    runner.model = full.train()
    assert not runner.usable({"point_clouds": torch.zeros(1), "images": None})
    with pytest.raises(ValueError, match="lang_branch"):
        pipeline.PhasedTrainStep(full, {}, None, None)


def test_branch_forward_matches_the_reference(G):
    """qa_module.py:501-587 on identical object_feat / bbox_mask / objectness_scores / language inputs"""
    from bridgeqa_amd import hotpath
    holder = torch.nn.Module()
    hotpath.build_lang_branch(holder, 128, 18, 30, mcan_flat_mlp_size=64, mcan_flat_out_size=96, lang_emb_size=20)
    holder.eval()
    assert _keys(holder) == G["branch_keys"].tolist()
    fill_params(holder, "branch.")
    inp = {k[6:]: torch.from_numpy(v) for k, v in G.items() if k.startswith("br_in_")}
    object_mask = (~inp["bbox_mask"].bool()).unsqueeze(1).unsqueeze(2)
    with torch.no_grad():
        d = hotpath.lang_branch_forward(holder, dict(inp), inp["object_feat"], object_mask, True, True, True)
    assert np.array_equal(d["lang_mask"].numpy(), G["br_out_lang_mask"])
    for k in ("lang_out", "lang_emb", "fuse_feat", "lang_scores", "cluster_ref", "answer_scores"):
        ref = G["br_out_" + k]
        assert d[k].shape == ref.shape
        assert np.abs(d[k].numpy() - ref).max() <= MCAN_ATOL * max(1.0, np.abs(ref).max() / 4), k
    with torch.no_grad():
        d2 = hotpath.lang_branch_forward(holder, dict(inp), inp["object_feat"], object_mask, False, False, False)
    assert "fuse_feat" in d2 and not {"lang_scores", "cluster_ref", "answer_scores"} & set(d2)


# ---- compile-time resources of the new kernels ----------------------------------------------------------------------------------
def test_lstm_kernels_have_no_scratch_and_the_recorded_lds():
    """tests/golden/kernel_resources.json predates these kernels; they are held here.  LDS as built: forward H + 4H floats,
    backward 4H + 4H floats."""
    from bridgeqa_amd import build
    build.build()
    res = build.kernel_resources()
    if res is None:
        pytest.skip("objects were not compiled by this checkout's build.py (prebuilt library)")
    mine = {k: v for k, v in res.items() if "lstm_" in k}
    lds = {}
    for k, v in mine.items():
        assert v.get("scratch", 0) == 0, k
        kind = "fwd" if "lstm_fwd_kernel" in k else "bwd" if "lstm_bwd_kernel" in k else None
        H = 128 if "ILi128E" in k else 256 if "ILi256E" in k else None
        lds[(kind, H)] = v.get("lds", 0)
    assert lds == {("fwd", 128): 2560, ("fwd", 256): 5120, ("bwd", 128): 4096, ("bwd", 256): 8192}
