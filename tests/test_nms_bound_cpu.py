"""tests/nms_ref.py checked without a GPU: the float64 NMS reference, fed by the float64 point count, reproduces the reference
project's own pred_mask (tests/golden/nms.npz, five variants) and equals the literal np.argsort / np.delete form wherever
numpy's order is defined; the numpy emulation of the kernels' partition equals the reference on every case (and its rank sort
is a permutation for every input); every planted defect of nms_ref.NMS_DEFECTS / COUNT_DEFECTS is rejected on a named case by
the comparison tests/test_nms_bound_gpu.py uses; and every case holds the conditions that comparison rests on (no contested NMS
decision, the keep share, the contested-pair caps).  Prints, per case, the keep share and the contested-pair share (pytest -s)."""
import types

import numpy as np
import pytest
import torch

import nms_ref as R

# the case on which each planted defect must be rejected (it may be rejected on others too)
NMS_DEFECT_CASE = dict(
    ties_desc="ties", ge="threshold", old_picked="asym", cls_ignored="strides", cls_always="strides", invalid_suppresses="invalid",
    invalid_picked="invalid", offset_cls="strides", offset_valid="strides", tail_rank="strides", tail_suppress="strides",
    fp32="fp32_flip", thresh_fp32="threshold", self_suppress="one", nan_blind="nonfinite")
COUNT_DEFECT_CASE = dict(drop_wave3="tails", drop_last_trip="tails", open_faces="lattice", swap_wh="random", sin_sign="random",
                         ld3="random", signed_half="negative", cap_ge="lattice")
PARTITION_DEFECTS = ("tail_rank", "nan_blind")          # rejected by the permutation assertion of the rank sort


def _decode_cpu(end, cfgd, cfg):
    """the decode of ap_helper._decode_predictions up to the two kernel calls, in fp32 torch on the CPU"""
    from bridgeqa_amd.loss_helper import _class2angle
    from bridgeqa_amd.proposal_module import box_corners
    center = end["center"].float().contiguous()
    hcls = torch.argmax(end["heading_scores"], -1)
    hres = torch.gather(end["heading_residuals"], 2, hcls.unsqueeze(-1)).squeeze(2).float()
    scls = torch.argmax(end["size_scores"], -1)
    sres = torch.gather(end["size_residuals"], 2, scls.unsqueeze(-1).unsqueeze(-1).repeat(1, 1, 1, 3)).squeeze(2).float()
    mean_size = torch.from_numpy(np.asarray(cfg.mean_size_arr, dtype=np.float32))
    heading = _class2angle(cfg, hcls, hres).contiguous()
    size = (mean_size[scls] + sres).contiguous()
    corners = box_corners(center, size, heading)
    lo, hi = corners.min(dim=2).values, corners.max(dim=2).values
    obj_prob = torch.softmax(end["objectness_scores"].float(), -1)[:, :, 1]
    cls = torch.argmax(end["sem_cls_scores"], -1)
    n = lambda t: np.ascontiguousarray(t.numpy())
    return n(center), n(size), n(heading), n(torch.cat([lo, hi], -1)), n(obj_prob), n(cls).astype(np.int32)


@pytest.mark.parametrize("v", range(5))
def test_reference_reproduces_the_golden_pred_mask(golden, v):
    from test_nms_gpu import VARIANTS
    g = golden("nms.npz")
    pre = "v%d_in_" % v
    end = {k[len(pre):]: torch.from_numpy(g[k]) for k in g if k.startswith(pre)}
    cfg = types.SimpleNamespace(num_heading_bin=int(g["v%d_NH" % v]), num_class=18, mean_size_arr=g["v%d_mean_size_arr" % v])
    cfgd = VARIANTS[v]
    center, size, heading, box, obj_prob, cls = _decode_cpu(end, cfgd, cfg)
    valid = None
    if cfgd["remove_empty_box"]:
        ref = R.count_reference(np.ascontiguousarray(end["point_clouds"].numpy()), center, size, heading)
        assert not R.count_conditions(ref)
        valid = ref["n_sure"] >= R.CAP
    same = bool(cfgd["use_3d_nms"] and cfgd.get("cls_nms", False))
    run = R._run(box, obj_prob, cls, valid, thr=cfgd["nms_iou"], old_type=cfgd["use_old_type_nms"], same_cls=same,
                 two_d=not cfgd["use_3d_nms"], tag="golden v%d" % v)
    keep, info = R.nms_reference(run)
    assert not info["contested"]
    assert np.array_equal(keep.astype(np.float64), g["v%d_pred_mask" % v])
    assert np.array_equal(R.nms_emulate(run), keep)


@pytest.mark.parametrize("name", R.NMS_CASES)
def test_nms_reference_equals_the_literal_form_and_the_emulation(name):
    literal = 0
    for run, (keep, info) in zip(R.nms_case(name), R.nms_reference_of(name)):
        assert not R.nms_compare(R.nms_emulate(run), keep), run["tag"]
        if not R.has_ties_or_nan(run):
            assert not R.nms_compare(R.nms_literal(run), keep), run["tag"]
            literal += 1
    assert literal > 0 or name in ("ties", "nonfinite")


@pytest.mark.parametrize("name", R.NMS_CASES)
def test_nms_case_holds_its_conditions(name):
    runs, refs = R.nms_case(name), R.nms_reference_of(name)
    assert len(runs) >= (6 if name not in ("threshold", "fp32_flip", "asym") else 4)
    for run, (keep, info) in zip(runs, refs):
        print("%s [%s]: keeps %d of %d valid boxes (%.3f), contested %d of %d evaluated pairs"
              % (name, run["tag"], info["kept"], info["valid"], info["kept"] / max(info["valid"], 1), info["contested"], info["evaluated"]))
        fails = R.nms_conditions(run, keep, info)
        assert not fails, fails
        assert run["box"].shape[1] <= R.NMS_MAX_K
    if name in ("strides", "full", "ties", "invalid"):
        assert all(r["random"] for r in runs)
    if name == "invalid":
        for run, (keep, _) in zip(runs, refs):
            if run["valid"] is not None:
                assert not keep[2].any() and not run["valid"][2].any()                    # the scene entirely invalid
                assert run["valid"][1, np.argmax(run["score"][1])] == 0 and keep[1].any()
    if name == "threshold":
        for run, (keep, _) in zip(runs, refs):
            want = 3 if "==" in run["tag"] else 2 if "<" in run["tag"] else 2 if "step" in run["tag"] else 1
            assert int(keep.sum()) == want, run["tag"]
    if name == "degenerate":
        for run, (keep, _) in zip(runs, refs):
            assert keep[0, [0, 1, 3]].all() and (keep[0, 2] or "2d" in run["tag"])        # zero volume: never suppressed
            assert np.array_equal(keep[0, :13], keep[1, :13])
            assert keep[0, 7:10].sum() == 1                                               # identical: the best one only
            assert keep[0, 10:13].all() or "2d" in run["tag"]                             # disjoint (in 3-D)
    if name == "ties":
        for run, (keep, _) in zip(runs, refs):
            assert keep[:, 200].all() and not keep[:, 201].any()                          # -0.0 == +0.0: the lower index wins
    if name == "nonfinite":
        for run, (keep, _) in zip(runs, refs):
            K = run["score"].shape[1]
            assert keep[0, 0] and keep[1, K - 1] and keep[2, 1]                           # the first-visited NaN box is kept


def test_rank_sort_is_a_permutation_for_any_scores():
    g = np.random.default_rng(3)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, 1.0, np.nan, 3e38, -3e38, 1e-45, -1e-45], dtype=np.float32)
    for K in (1, 2, 12, 255, 256, 257, 1024):
        for trial in range(4):
            s = g.choice(special, size=K) if trial < 2 else g.random(K).astype(np.float32)
            if trial == 3:
                s[g.integers(0, K, max(1, K // 7))] = np.nan
            order = R.rank_sort(s)
            assert sorted(order.tolist()) == list(range(K))
            assert np.array_equal(order, R.visit_order(s))
    with pytest.raises(R.PartitionError):
        R.rank_sort(np.array([0.5, np.nan, 0.25], dtype=np.float32), defect="nan_blind")


@pytest.mark.parametrize("defect", R.NMS_DEFECTS)
def test_planted_nms_defect_is_rejected(defect):
    name = NMS_DEFECT_CASE[defect]
    rejected = []
    for run, (keep, _) in zip(R.nms_case(name), R.nms_reference_of(name)):
        try:
            if R.nms_compare(R.nms_emulate(run, defect=defect), keep):
                rejected.append(run["tag"])
        except R.PartitionError:
            assert defect in PARTITION_DEFECTS
            rejected.append(run["tag"] + " (permutation)")
    assert rejected, "%s passes on %s" % (defect, name)
    if defect in PARTITION_DEFECTS:
        assert any(t.endswith("(permutation)") for t in rejected)
    if defect == "thresh_fp32":
        assert {t.split(" old")[0].split(" iou")[0] for t in rejected} == {"o = float32(0.2)", "o = float32(0.3)", "float32(0.7) < o < 0.7"}


@pytest.mark.parametrize("name", R.COUNT_CASES)
def test_count_case_holds_its_conditions_and_the_emulation_its_interval(name):
    for run, ref in zip(R.count_case(name), R.count_reference_of(name)):
        fails = R.count_conditions(ref, run["tag"])
        print("%s: contested %d of %d pairs (%.2e), %d of %d boxes free of them"
              % (run["tag"], int(ref["n_contested"].sum()), ref["pairs"], ref["n_contested"].sum() / ref["pairs"],
                 int((ref["n_contested"] == 0).sum()), ref["n_contested"].size))
        assert not fails, fails
        for cap in (0, R.CAP):
            got = R.count_emulate(run["pc"], run["center"], run["size"], run["heading"], cap=cap)
            assert not R.count_compare(got, ref, cap), run["tag"]
        if run["exact"]:
            assert not ref["n_contested"].any() and np.array_equal(ref["n_sure"], run["expect"])
            assert {4, 5, 6} <= set(run["expect"].ravel().tolist())
        if name == "tails":
            assert (ref["n_sure"][:, 0::2] == run["pc"].shape[1]).all()                  # every lane and wave contributes
        if name == "negative":
            assert (run["size"] < 0).any(axis=(0, 1)).all() and set((run["size"] < 0).sum(-1).ravel().tolist()) == {1, 2, 3}
            pos = R.count_reference(run["pc"], run["center"], np.abs(run["size"]), run["heading"])
            assert np.array_equal(pos["n_sure"], ref["n_sure"]) and ref["n_sure"].sum() > 20


@pytest.mark.parametrize("defect", R.COUNT_DEFECTS)
def test_planted_count_defect_is_rejected(defect):
    name = COUNT_DEFECT_CASE[defect]
    rejected = False
    for run, ref in zip(R.count_case(name), R.count_reference_of(name)):
        for cap in (0, R.CAP):
            got = R.count_emulate(run["pc"], run["center"], run["size"], run["heading"], cap=cap, defect=defect)
            rejected = rejected or bool(R.count_compare(got, ref, cap))
    assert rejected, "%s passes on %s" % (defect, name)


def test_every_defect_has_a_case():
    assert set(NMS_DEFECT_CASE) == set(R.NMS_DEFECTS) and set(NMS_DEFECT_CASE.values()) <= set(R.NMS_CASES)
    assert set(COUNT_DEFECT_CASE) == set(R.COUNT_DEFECTS) and set(COUNT_DEFECT_CASE.values()) <= set(R.COUNT_CASES)
