"""The two kernels of csrc/nms.hip (nms_kernel, box_point_count_kernel) held to the float64 decisions of tests/nms_ref.py through
_ext.nms and _ext.box_point_count: `keep` must EQUAL the reference's on every run of every case of nms_ref.NMS_CASES (tolerance
0: the kernel does the reference's double operations in its order), the counts must lie in [n_sure, n_sure + n_contested] per
box -- equality wherever nothing is contested, and the lattice cases contest nothing by construction.  One composition test
runs ap_helper._decode_predictions (decode, empty-box test, NMS) and holds its `keep` to the reference run on the extents, the
objectness, the classes and the point counts the same call produced.  Which mechanism each case reaches is said in the docstring
of tests/nms_ref.py; the conditions the comparisons rest on are asserted on the CPU by tests/test_nms_bound_cpu.py.

`nonfinite` (NaN and +-inf scores) is a test of DEFINED behaviour: the rank sort is a total order, so every slot of the kernel's
visiting table is written exactly once for any scores (nms_ref.rank_sort asserts the same of its restatement).

On an MI355X: `keep` equalled the reference on every run of every case (K = 1024, the ties, the NaN / inf scores, the pairs between
thr and float32(thr) and the fp32-flip pairs included); no (box, point) pair of any count case was contested, so every count was
EQUAL to the float64 count; the composition's `keep` equalled the reference in its three modes.  The kernel as it was before
this change was not run against these cases: by its code it compares the threshold in fp32 (`threshold`), takes the signed half
size (`negative`) and leaves a slot of its visiting table unwritten on a NaN score (`nonfinite`); nms_ref's emulation of each of
the three is rejected on that case by tests/test_nms_bound_cpu.py."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import nms_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
pytestmark = pytest.mark.gpu


def _nms(dev, run):
    from bridgeqa_amd import _ext
    t = lambda a: None if a is None else torch.from_numpy(np.array(a)).to(dev)
    return _ext.nms(t(run["box"]), t(run["score"]), run["thr"], cls=t(run["cls"]) if run["same_cls"] else None,
                    valid=t(run["valid"]), old_type=run["old_type"], same_cls=run["same_cls"]).cpu().numpy()


def _count(dev, run, cap=0):
    from bridgeqa_amd import _ext
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    return _ext.box_point_count(t(run["pc"]), t(run["center"]), t(run["size"]), t(run["heading"]), cap=cap).cpu().numpy()


@pytest.mark.parametrize("name", R.NMS_CASES)
def test_nms_keep_equals_the_fp64_reference(dev, name):
    fails = []
    for run, (keep, info) in zip(R.nms_case(name), R.nms_reference_of(name)):
        assert not info["contested"]
        got = _nms(dev, run)
        assert got.dtype == np.bool_
        fails += ["%s [%s]: %s" % (name, run["tag"], f) for f in R.nms_compare(got, keep)]
    assert not fails, "\n".join(fails[:20])


def test_nms_with_the_class_ids_passed_but_unused(dev):
    """same_cls off with class ids present: the class test must not be applied"""
    from bridgeqa_amd import _ext
    for run, (keep, _) in zip(R.nms_case("strides"), R.nms_reference_of("strides")):
        if not run["same_cls"]:
            t = lambda a: torch.from_numpy(np.array(a)).to(dev)
            got = _ext.nms(t(run["box"]), t(run["score"]), run["thr"], cls=t(run["cls"]), valid=t(run["valid"]),
                           old_type=run["old_type"], same_cls=False).cpu().numpy()
            assert not R.nms_compare(got, keep), run["tag"]


def test_the_float_entry_point_forwards_the_rounded_threshold(dev):
    """bq_nms keeps its signature (float thresh) and forwards (double)thresh: it must equal the reference run with float32(thr) --
    on the `threshold` runs that differs from the Python-float decision exactly where the overlap lies between the two"""
    from bridgeqa_amd import _ext
    differ = 0
    for run, (keep, _) in zip(R.nms_case("threshold"), R.nms_reference_of("threshold")):
        box, score = (torch.from_numpy(np.array(run[k])).to(dev) for k in ("box", "score"))
        B, K = score.shape
        got = torch.empty(B, K, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _ext._check(_ext._lib.bq_nms(_ext._p(box), _ext._p(score), None, None, _ext._p(got), B, K, run["thr"], int(run["old_type"]), 0,
                                         _ext._stream()), "nms")
        want, _ = R.nms_reference(dict(run, thr=float(np.float32(run["thr"]))))
        assert not R.nms_compare(got.cpu().numpy(), want), run["tag"]
        differ += int(not np.array_equal(want, keep))
    assert differ == 8                                    # the runs named "float32(thr)": 3 each for 0.2 and 0.3, 2 for 0.7


def test_nms_limit_of_k(dev):
    from bridgeqa_amd import _ext
    with pytest.raises(RuntimeError):
        _ext.nms(torch.zeros(1, R.NMS_MAX_K + 1, 6, device=dev), torch.zeros(1, R.NMS_MAX_K + 1, device=dev), 0.25)


@pytest.mark.parametrize("name", R.COUNT_CASES)
def test_point_count_within_the_fp64_interval(dev, name):
    fails = []
    for run, ref in zip(R.count_case(name), R.count_reference_of(name)):
        plain = _count(dev, run)
        capped = _count(dev, run, cap=R.CAP)
        contested = int(ref["n_contested"].sum())
        print("\n%s: contested %d of %d pairs, largest count %d" % (run["tag"], contested, ref["pairs"], int(plain.max())), end="")
        fails += ["%s: %s" % (run["tag"], f) for f in R.count_compare(plain, ref)]
        fails += ["%s cap: %s" % (run["tag"], f) for f in R.count_compare(capped, ref, R.CAP)]
        if not np.array_equal(capped, np.minimum(plain, R.CAP)):
            fails.append("%s: cap = %d is not clamp(max = %d) of cap = 0" % (run["tag"], R.CAP, R.CAP))
        if run["exact"] and not np.array_equal(plain, run["expect"]):
            fails.append("%s: counts %s, by hand %s" % (run["tag"], plain.tolist(), run["expect"].tolist()))
        if name == "negative":
            pos = dict(run, size=np.abs(run["size"]))
            if not np.array_equal(_count(dev, pos), plain):
                fails.append("negative: the count differs from that of |size|")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("variant", (0, 1, 2))
def test_decode_predictions_keep_equals_the_reference_on_its_own_operands(dev, variant, monkeypatch):
    """ap_helper._decode_predictions at B = 3, K = 256, N = 2000 with remove_empty_box on, in the three NMS modes: the operands it
    handed to the two kernels are recorded, and its `keep` must equal the reference run on them"""
    from gen_golden_nms import make_inputs
    from bridgeqa_amd import _ext, ap_helper
    cfgd = (dict(use_3d_nms=True, cls_nms=True, nms_iou=0.25, use_old_type_nms=False),
            dict(use_3d_nms=True, cls_nms=False, nms_iou=0.3, use_old_type_nms=True),
            dict(use_3d_nms=False, cls_nms=False, nms_iou=0.3, use_old_type_nms=False))[variant]
    NH = 4
    d, mean_size_arr = make_inputs(70 + variant, NH, B=3, K=256, N=2000)
    cfg = types.SimpleNamespace(num_heading_bin=NH, num_class=18, mean_size_arr=mean_size_arr)
    end = {k: v.to(dev) for k, v in d.items()}
    seen = {}
    real_count, real_nms = _ext.box_point_count, _ext.nms

    def spy_count(points, center, size, heading, cap=0):
        out = real_count(points, center, size, heading, cap=cap)
        seen["count"] = tuple(np.ascontiguousarray(t.cpu().numpy()) for t in (points, center, size, heading)) + (cap, out.cpu().numpy())
        return out

    def spy_nms(box, score, thresh, cls=None, valid=None, old_type=False, same_cls=False):
        seen["nms"] = dict(box=box.cpu().numpy(), score=score.cpu().numpy(), thr=thresh, cls=None if cls is None else cls.cpu().numpy(),
                           valid=valid.cpu().numpy(), old_type=old_type, same_cls=same_cls)
        return real_nms(box, score, thresh, cls=cls, valid=valid, old_type=old_type, same_cls=same_cls)
    monkeypatch.setattr(_ext, "box_point_count", spy_count)
    monkeypatch.setattr(_ext, "nms", spy_nms)
    corners, lo, hi, keep, obj_prob, pred_sem_cls, _ = ap_helper._decode_predictions(end, dict(cfgd, remove_empty_box=True, dataset_config=cfg))
    # the empty-box test: the counts within the interval, no `>= 5` decision contested, the mask handed on is that decision
    pc, center, size, heading, cap, count = seen["count"]
    ref = R.count_reference(pc, center, size, heading)
    assert cap == R.CAP and not R.count_conditions(ref, "decode") and not R.count_compare(count, ref, cap)
    n = seen["nms"]
    assert np.array_equal(n["valid"].astype(bool), ref["n_sure"] >= R.CAP) and 0.05 < n["valid"].mean() < 0.95
    # the operands: the extents of the call's own corners, its objectness and classes
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    box3 = np.concatenate([lo_h, hi_h], -1)
    assert np.array_equal(n["box"], R.to_2d(box3) if not cfgd["use_3d_nms"] else box3)
    assert np.array_equal(n["score"], obj_prob.cpu().numpy()) and n["thr"] == cfgd["nms_iou"]
    assert np.array_equal(corners.min(dim=2).values.cpu().numpy(), lo_h)
    run = R._run(box3, obj_prob.cpu().numpy(), pred_sem_cls.cpu().numpy(), n["valid"], thr=cfgd["nms_iou"], old_type=cfgd["use_old_type_nms"],
                 same_cls=bool(cfgd["use_3d_nms"] and cfgd["cls_nms"]), two_d=not cfgd["use_3d_nms"], tag="decode")
    want, info = R.nms_reference(run)
    assert not info["contested"] and 0.05 * info["valid"] <= info["kept"] <= 0.95 * info["valid"]
    assert not R.nms_compare(keep.cpu().numpy(), want)
