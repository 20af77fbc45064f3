"""tests/detloss_ref.py checked without a GPU: the fp64 reference reproduces the reference project's own numbers
(tests/golden/det_loss.npz) and its closed-form gradients equal fp64 autograd of loss_helper's composition; a plain fp32 emulation
of the kernels' partition (item -> thread -> wave -> block) and the fp32 torch composition stay within the bound on every case;
every planted defect of detloss_ref.DEFECTS is rejected by the comparison tests/test_detloss_bound_gpu.py uses; and every case
holds the conditions the bound rests on (no contested pick or threshold, contested signs <= 1e-3, all three label classes on
the random cases)."""
import pytest
import torch

import detloss_ref as R

# the case on which each planted defect must be rejected (it may be rejected on others too)
DEFECT_CASE = dict(
    drop_A="two_trips_A", drop_B="two_trips_B", drop_C="two_trips_C", batch_mod="two_trips_A", last_i1="ties", last_k2="ties",
    last_vote="ties", sign0="ties", labels_via_ic="bench_like", skip_padded="ties", huber_unclamped="bench_like",
    no_third="bench_like", weights_swapped="bench_like", share_div_npos="bench_like", partial_left_out="bench_like",
    neg_no_sub="bench_like", cl_stride3="limits", seed_i64_as_i32="limits", wrong_upstream="bench_like")


def test_reference_reproduces_the_golden_terms_and_labels(golden):
    from test_loss_cpu import load
    d, want, cfg = load(golden, torch.device("cpu"))
    ref = R.reference(d, cfg, check=False)
    for i, k in enumerate(R.TERMS):
        assert abs(float(ref["terms"][i]) - float(want[k])) <= 1e-6 * max(1.0, abs(float(want[k]))), (k, float(ref["terms"][i]), float(want[k]))
    for k in R.LABELS:
        assert torch.equal(ref[k], want[k]) and ref[k].dtype == want[k].dtype, k


@pytest.mark.parametrize("name", R.CASES)
def test_closed_form_gradients_equal_fp64_autograd(name):
    """the composition forms its masks and their sums through .float() also when run in fp64, so its denominators carry one fp32
    rounding u: held to 4 u of the tensor's largest element (a wrong pick, sign or factor is of the order of that element)"""
    t, cfg = R.tensors(name)
    ref, comp = R.reference_of(name), R.composition(t, cfg, dtype=torch.float64)
    assert torch.allclose(comp["terms"], ref["terms"], rtol=4 * R.U, atol=1e-12), (comp["terms"], ref["terms"])
    assert torch.allclose(comp["ratios"].double(), ref["ratios"], rtol=0.0, atol=4 * R.U)
    for k in R.LABELS:
        assert torch.equal(comp[k], ref[k]), k
    for i, n in enumerate(R.NAMES):
        want = ref["grads"][n] * R.TW[i]
        err = float((comp["grads"][n] - want).abs().max())
        assert err <= 4 * R.U * float(want.abs().max()), (n, err)


@pytest.mark.parametrize("name", R.CASES)
def test_emulation_and_fp32_composition_stay_within_the_bound(name):
    t, cfg = R.tensors(name)
    ref = R.reference_of(name)
    for what, out, slack in (("emulation", R.emulate(t, cfg), None), ("composition", R.composition(t, cfg), R.autograd_slack(ref))):
        worst, fails = R.compare(out, ref, slack=slack)
        assert not fails, "%s %s:\n%s" % (name, what, "\n".join(fails))
        print("%s %s: " % (name, what) + "  ".join("%s %.3g" % kv for kv in worst.items()))


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_is_rejected(defect):
    name = DEFECT_CASE[defect]
    t, cfg = R.tensors(name)
    _, fails = R.compare(R.emulate(t, cfg, defect=defect), R.reference_of(name))
    assert fails, "%s passes on %s" % (defect, name)


def test_every_defect_has_a_case():
    assert set(DEFECT_CASE) == set(R.DEFECTS) and set(DEFECT_CASE.values()) <= set(R.CASES)


@pytest.mark.parametrize("name", R.CASES)
def test_case_holds_the_conditions_of_the_bound(name):
    t, cfg = R.tensors(name)
    ref = R.reference(t, cfg, check=False)
    assert not any(ref["contested"].values()), ref["contested"]
    assert ref["sign_share"] <= R.SIGN_CAP
    pos, neg = (float(v) for v in ref["ratios"])
    if name in R.RANDOM_CASES:
        assert 0.02 < pos < 0.9 and neg > 0.02, (pos, neg)
    finite = all(bool(torch.isfinite(g).all()) for g in ref["grads"].values()) and bool(torch.isfinite(ref["terms"]).all())
    assert finite
    if name == "no_positive":
        assert pos == 0.0 and neg > 0.0 and float(ref["terms"][2:].abs().sum()) > 0.0 and float(ref["terms"][3:].abs().sum()) == 0.0
    if name == "all_grey":
        assert pos == 0.0 and neg == 0.0 and float(ref["terms"][1]) == 0.0
    if name == "no_vote_mask":
        assert float(ref["terms"][0]) == 0.0 and float(ref["grads"]["vote_xyz"].abs().sum()) == 0.0
    if name == "no_box":
        assert float(t["box_label_mask"].sum()) == 0.0 and pos > 0.0
    if name == "one":
        assert pos == 1.0 and all(float(ref["terms"][i]) == 0.0 for i in (3, 5, 7))
    if name == "limits":
        x = t["sem_cls_scores"]
        assert float((x.amax(-1, keepdim=True) - x).max()) > 60.0 and t["seed_inds"].dtype == torch.int64 and t["center_label"].shape[2] == 6
    if name.startswith("two_trips"):
        B, S = t["seed_xyz"].shape[:2]
        count = dict(A=B * S, B=B * t["center"].shape[1], C=B * t["center_label"].shape[1])[name[-1]]
        assert R.DL_ALL < count < 2 * R.DL_ALL


def test_the_ties_case_holds_its_ties():
    """the structures the issue lists are present in the reference's decisions, and every input is a small dyadic"""
    t, cfg = R.tensors("ties")
    ref = R.reference_of("ties")
    for k, v in t.items():
        if v.is_floating_point():
            assert torch.equal(v * 8, (v * 8).round()) and float(v.abs().max()) < 64, k
    gt, c, agg = t["center_label"], t["center"], t["aggregated_vote_xyz"]
    for b in range(gt.shape[0]):
        assert torch.equal(gt[b, 0], gt[b, 1]) and int(ref["i1"][b, 0]) == 0 and int(ref["objectness_label"][b, 0]) == 1   # duplicate real boxes
        assert int(t["heading_class_label"][b, 0]) != int(t["heading_class_label"][b, 1])
        assert int(ref["i1"][b, 1]) == 5 and float(t["box_label_mask"][b, 5]) == 0 and int(ref["objectness_label"][b, 1]) == 1   # a padded row assigned
        assert torch.equal(c[b, 4], c[b, 5]) and torch.equal(agg[b, 4], agg[b, 5]) and int(ref["k2"][b, 4]) == 4            # duplicate proposals
        assert int(ref["k2"][b, 2]) == 6 and int(ref["objectness_label"][b, 6]) == 1
        assert int(ref["objectness_mask"][b, 2]) == 0 and (int(ref["objectness_label"][b, 3]), int(ref["objectness_mask"][b, 3])) == (0, 1)
        v = t["vote_xyz"].view(gt.shape[0], -1, 3, 3)[b]
        assert torch.equal(v[0, 0], v[0, 1]) and torch.equal(v[0, 0], v[0, 2]) and (int(ref["bj"][b, 0]), int(ref["bv"][b, 0])) == (0, 0)
        assert (int(ref["bj"][b, 1]), int(ref["bv"][b, 1])) == (0, 1) and float(ref["grads"]["vote_xyz"].view(gt.shape[0], -1, 3, 3)[b, 1].abs().sum()) == 0.0
        assert int(ref["bv"][b, 2]) == 0 and (int(ref["bj"][b, 4]), int(ref["bv"][b, 4])) == (0, 0)
    # Huber errors at exactly 0, +-1, +-2 among the positives
    pos = ref["objectness_label"].bool()
    g = ref["grads"]["heading_residuals_normalized"].sum(-1)[pos] * (ref["npos"] + 1e-6)
    assert {-1.0, 0.0, 1.0} <= set(round(float(x), 9) for x in g)
    # exact arithmetic: the emulation's labels, assignment and signs equal the reference's with tolerance 0
    em = R.emulate(t, cfg, tw=(1.0,) * 8)
    for k in R.LABELS:
        assert torch.equal(em[k], ref[k]), k
    assert torch.equal(torch.sign(em["grads"]["vote_xyz"]).double(), torch.sign(ref["grads"]["vote_xyz"]))
    assert not bool(ref["sign_contested"].any())
