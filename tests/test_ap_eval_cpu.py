"""Detection evaluation without a GPU (bridgeqa_amd/ap_helper.py parse_groundtruths / APCalculator on its numpy path) and the
tests' own literal restatement (tests/ap_ref.py), both against golden vectors the reference's lib/ap_helper.py and
utils/eval_det.py produced (tools/gen_golden_ap.py -> tests/golden/ap_eval.npz).

Bounds.  rec / prec are quotients of exact integers: equal bit for bit.  AP is a sum of n_det non-negative terms that add up
to at most 1, so any order of summation stays within n_det * 2^-52 of any other.  Corners: the decode differs from numpy's
only in a few ulp of cos / sin on coordinates below 16, under 1e-14; 1e-12 leaves a 100x margin."""
import types

import numpy as np
import pytest
import torch

import ap_ref

THRESHOLDS = (0.25, 0.5)


def load_eval_case(g):
    cut = lambda a, n: np.split(a, np.cumsum(n)[:-1])
    pc, pb, ps = (cut(g["ev_pred_" + k], g["ev_pred_count"]) for k in ("cls", "corners", "score"))
    gc, gb = (cut(g["ev_gt_" + k], g["ev_gt_count"]) for k in ("cls", "corners"))
    preds = [[(int(c), b, float(s)) for c, b, s in zip(*scan)] for scan in zip(pc, pb, ps)]
    gts = [[(int(c), b) for c, b in zip(*scan)] for scan in zip(gc, gb)]
    assert tuple(g["ev_thresholds"]) == THRESHOLDS
    ap_ref.check_eval_case(preds, gts, THRESHOLDS)            # the generator's conditions, re-asserted on load
    return preds, gts


def golden_metrics(g, t):
    return dict(zip([str(k) for k in g["ev_t%d_metric_keys" % t]], g["ev_t%d_metric_values" % t]))


def check_metrics(got, g, t, n_det):
    want = golden_metrics(g, t)
    assert list(got.keys()) == list(want.keys())
    for k in want:
        if k.endswith("Recall"):
            assert got[k] == want[k], k
        else:
            assert abs(got[k] - want[k]) <= n_det * 2.0 ** -52, (k, got[k], want[k])


def check_curves(g, t, rec, prec, ap, n_det):
    assert sorted(ap) == g["ev_t%d_classes" % t].tolist()
    for c in sorted(ap):
        assert np.array_equal(rec[c], g["ev_t%d_c%d_rec" % (t, c)]), c
        assert np.array_equal(prec[c], g["ev_t%d_c%d_prec" % (t, c)]), c
        assert abs(ap[c] - float(g["ev_t%d_c%d_ap" % (t, c)])) <= n_det * 2.0 ** -52, c


def check_groundtruths(g, v, out, end):
    assert out is end["batch_gt_map_cls"]
    assert [len(lst) for lst in out] == g["gt%d_count" % v].tolist()
    cls = [c for lst in out for c, _ in lst]
    assert all(type(c) is int for c in cls) and cls == g["gt%d_cls" % v].tolist()
    corners = np.array([b for lst in out for _, b in lst]).reshape(-1, 8, 3)
    assert corners.dtype == np.float64
    assert np.abs(corners - g["gt%d_corners" % v]).max() <= 1e-12


def label_case(g, v, dev="cpu"):
    pre = "gt%d_in_" % v
    end = {k[len(pre):]: torch.from_numpy(g[k]).to(dev) for k in g if k.startswith(pre)}
    cfg = types.SimpleNamespace(num_heading_bin=int(g["gt%d_NH" % v]), num_class=18, mean_size_arr=g["gt%d_mean_size_arr" % v])
    return end, dict(dataset_config=cfg)


def test_case_builder_reproduces_the_fixture(golden):
    preds, gts = load_eval_case(golden("ap_eval.npz"))
    p2, g2 = ap_ref.build_eval_case(0)
    assert [len(p) for p in p2] == [len(p) for p in preds] and len(gts[3]) == 70 and not gts[1] and not preds[2]
    assert all(np.array_equal(a[1], b[1]) and a[0] == b[0] and a[2] == b[2] for x, y in zip(preds, p2) for a, b in zip(x, y))
    assert all(np.array_equal(a[1], b[1]) and a[0] == b[0] for x, y in zip(gts, g2) for a, b in zip(x, y))


@pytest.mark.parametrize("t", range(2))
def test_literal_restatement_vs_reference_golden(golden, t):
    g = golden("ap_eval.npz")
    preds, gts = load_eval_case(g)
    n_det = sum(len(p) for p in preds)
    rec, prec, ap = ap_ref.eval_all(dict(enumerate(preds)), dict(enumerate(gts)), THRESHOLDS[t])
    check_curves(g, t, rec, prec, ap, n_det)
    check_metrics(ap_ref.metrics(dict(enumerate(preds)), dict(enumerate(gts)), THRESHOLDS[t]), g, t, n_det)


@pytest.mark.parametrize("v", range(2))
def test_parse_groundtruths_vs_reference_golden(golden, v):
    from bridgeqa_amd.ap_helper import parse_groundtruths
    g = golden("ap_eval.npz")
    end, cfgd = label_case(g, v)
    check_groundtruths(g, v, parse_groundtruths(end, cfgd), end)


@pytest.mark.parametrize("t", range(2))
def test_calculator_on_host_lists_vs_reference_golden(golden, t):
    from bridgeqa_amd.ap_helper import APCalculator
    g = golden("ap_eval.npz")
    preds, gts = load_eval_case(g)
    n_det = sum(len(p) for p in preds)
    calc = APCalculator(THRESHOLDS[t])
    calc.step(preds[:3], gts[:3])
    calc.step(preds[3:], gts[3:])
    assert calc.scan_cnt == 8
    check_metrics(calc.compute_metrics(backend="numpy"), g, t, n_det)
    rec, prec, ap = calc.eval_det(backend="numpy")[THRESHOLDS[t]]
    check_curves(g, t, rec, prec, ap, n_det)
    named = APCalculator(THRESHOLDS[t], class2type_map={2: "chair", 5: "table", 7: "door", 11: "sink"})
    named.step(preds, gts)
    m = named.compute_metrics(backend="numpy")
    assert list(m)[:4] == ["chair Average Precision", "table Average Precision", "door Average Precision", "sink Average Precision"]
    assert m["sink Average Precision"] == 0 and m["sink Recall"] == 0          # predicted, never in the ground truth


def test_threshold_tuple_equals_single_threshold_calculators(golden):
    from bridgeqa_amd.ap_helper import APCalculator
    preds, gts = load_eval_case(golden("ap_eval.npz"))
    both = APCalculator(THRESHOLDS)
    both.step(preds, gts)
    m = both.compute_metrics(backend="numpy")
    assert list(m.keys()) == list(THRESHOLDS)
    for thr in THRESHOLDS:
        one = APCalculator(thr)
        one.step(preds, gts)
        assert m[thr] == one.compute_metrics(backend="numpy")
    with pytest.raises(ValueError):
        APCalculator((0.1, 0.2, 0.3, 0.4, 0.5))


def test_reset_forgets_every_step(golden):
    from bridgeqa_amd.ap_helper import APCalculator
    preds, gts = load_eval_case(golden("ap_eval.npz"))
    calc = APCalculator(0.25)
    calc.step(preds[:4], gts[:4])
    calc.reset()
    assert calc.scan_cnt == 0 and not calc.pred_map_cls and not calc.gt_map_cls
    calc.step(preds[4:], gts[4:])
    fresh = APCalculator(0.25)
    fresh.step(preds[4:], gts[4:])
    assert calc.compute_metrics(backend="numpy") == fresh.compute_metrics(backend="numpy")
    want = ap_ref.metrics(dict(enumerate(preds[4:])), dict(enumerate(gts[4:])), 0.25)
    got = calc.compute_metrics(backend="numpy")
    assert list(got) == list(want) and all(abs(got[k] - want[k]) <= 400 * 2.0 ** -52 for k in want)


def test_class_with_ground_truth_and_no_prediction_has_ap_and_recall_zero(golden):
    from bridgeqa_amd.ap_helper import APCalculator
    preds, gts = load_eval_case(golden("ap_eval.npz"))
    preds = [[d for d in p if d[0] != 5] for p in preds]          # class 5 keeps its ground truth, loses every detection
    calc = APCalculator(0.25)
    calc.step(preds, gts)
    m = calc.compute_metrics(backend="numpy")
    want = ap_ref.metrics(dict(enumerate(preds)), dict(enumerate(gts)), 0.25)
    assert list(m.keys()) == list(want.keys())
    assert m["5 Average Precision"] == 0 and m["5 Recall"] == 0
    assert want["7 Average Precision"] != 0                                 # the next class keeps its OWN result
    assert all(abs(m[k] - want[k]) <= 400 * 2.0 ** -52 for k in want) and m["AR"] == want["AR"]


def test_equal_scores_rank_by_scan_then_position():
    """two detections of one box with the same score: the earlier scan / earlier list position claims it"""
    from bridgeqa_amd.ap_helper import APCalculator
    box = ap_ref.corners_of((1, 1, 1), (1, 1, 1), 0.0)
    far = ap_ref.corners_of((5, 5, 5), (1, 1, 1), 0.0)
    preds = [[(0, far, 0.5), (0, box, 0.5), (0, box, 0.5)], [(0, box, 0.5)]]
    gts = [[(0, box)], [(0, box)]]
    calc = APCalculator(0.25)
    calc.step(preds, gts)
    rec, prec, ap = calc.eval_det(backend="numpy")[0.25]
    r2, p2, a2 = ap_ref.eval_all(dict(enumerate(preds)), dict(enumerate(gts)), 0.25)
    # rank order: (scan 0, pos 0) miss, (0, 1) hit, (0, 2) duplicate, (1, 0) hit
    assert np.array_equal(prec[0], np.array([0, 1 / 2, 1 / 3, 2 / 4])) and np.array_equal(prec[0], p2[0])
    assert np.array_equal(rec[0], r2[0]) and ap[0] == a2[0]


def test_packed_cpu_tensors_equal_host_lists():
    """the packing semantics without a GPU: fixed-shape packed objects on the CPU (per-class scores and single-class form, with
    invalid slots) give the metrics of the lists they stand for"""
    from bridgeqa_amd.ap_helper import APCalculator, PackedGroundTruths, PackedPredictions
    rng = np.random.default_rng(3)
    B, K, K2, C = 3, 12, 6, 4
    ext = torch.from_numpy(ap_ref.random_boxes(rng, B * K).reshape(B, K, 6))
    gext = ext[:, :K2] + torch.from_numpy(rng.normal(size=(B, K2, 6)) * 0.05)
    valid = torch.from_numpy(rng.random((B, K)) < 0.7)
    gvalid = torch.from_numpy(rng.random((B, K2)) < 0.8)
    gcls = torch.from_numpy(rng.integers(0, C, (B, K2)))
    score = torch.from_numpy(rng.random((B, K, C)).astype(np.float32))
    cls = torch.from_numpy(rng.integers(0, C, (B, K)))
    corners = lambda e: np.array([[e[i], e[j + 1], e[k + 2]] for i in (0, 3) for j in (0, 3) for k in (0, 3)], dtype=np.float64)
    gts = [[(int(gcls[b, j]), corners(gext[b, j].numpy())) for j in range(K2) if gvalid[b, j]] for b in range(B)]
    per_class = [[(c, corners(ext[b, k].numpy()), score[b, k, c].item()) for c in range(C) for k in range(K) if valid[b, k]]
                 for b in range(B)]
    single = [[(int(cls[b, k]), corners(ext[b, k].numpy()), score[b, k, 0].item()) for k in range(K) if valid[b, k]] for b in range(B)]
    for lists, packed in ((per_class, PackedPredictions(ext, score, None, valid, C)),
                          (single, PackedPredictions(ext, score[:, :, 0].contiguous(), cls, valid, C))):
        a, b = APCalculator(THRESHOLDS), APCalculator(THRESHOLDS)
        a.step(lists, gts)
        b.step(packed, PackedGroundTruths(gext, gcls, gvalid, C))
        b.step(packed, PackedGroundTruths(gext, gcls, gvalid, C))
        a.step(lists, gts)
        assert a.compute_metrics(backend="numpy") == b.compute_metrics(backend="numpy")
        want = ap_ref.metrics(dict(enumerate(lists + lists)), dict(enumerate(gts + gts)), 0.5)
        got = a.compute_metrics(backend="numpy")[0.5]
        assert list(got) == list(want) and all(abs(got[k] - want[k]) <= 2 * B * K * C * 2.0 ** -52 for k in want)
    with pytest.raises(TypeError):
        APCalculator().step(per_class, PackedGroundTruths(gext, gcls, gvalid, C))
