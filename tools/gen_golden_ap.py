"""Golden vectors for the detection evaluation (parse_groundtruths, APCalculator), produced by the REFERENCE's own
lib/ap_helper.py (:180-278) and utils/eval_det.py on the CPU of the build container.

TEST INFRASTRUCTURE.  Usage:  python tools/gen_golden_ap.py   -> tests/golden/ap_eval.npz   (data only)

The shims are oracle/gen_golden_loss.py's and the dataset config oracle/gen_golden_nms.py's; the seeded inputs come from
tests/ap_ref.py (build_label_case, build_eval_case), whose conditions (distinct scores per class, no IoU within 1e-9 of a
threshold, every ground-truth class predicted -- the reference's multiprocessing path is only well defined then) are asserted
here and again by the tests on load."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "ap_eval.npz")
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from gen_golden_loss import install_shims  # noqa: E402
from gen_golden_nms import ConfigShim  # noqa: E402
import ap_ref  # noqa: E402

THRESHOLDS = (0.25, 0.5)


def main():
    install_shims()
    import lib.ap_helper as ap
    from utils.eval_det import eval_det, get_iou_obb
    save = {}
    # ---- parse_groundtruths
    for v, NH in enumerate((1, 4)):
        d, mean_size_arr = ap_ref.build_label_case(20 + v, NH)
        for k, a in d.items():
            save["gt%d_in_%s" % (v, k)] = a
        save["gt%d_mean_size_arr" % v], save["gt%d_NH" % v] = mean_size_arr, np.array(NH)
        end = {k: torch.from_numpy(a) for k, a in d.items()}
        out = ap.parse_groundtruths(end, dict(dataset_config=ConfigShim(NH, 18, mean_size_arr)))
        assert out is end["batch_gt_map_cls"]
        save["gt%d_count" % v] = np.array([len(lst) for lst in out], dtype=np.int64)
        save["gt%d_cls" % v] = np.array([c for lst in out for c, _ in lst], dtype=np.int64)
        save["gt%d_corners" % v] = np.array([b for lst in out for _, b in lst], dtype=np.float64).reshape(-1, 8, 3)
        assert save["gt%d_corners" % v].max() < 16
        print("labels", v, "boxes per scene", save["gt%d_count" % v].tolist())
    # ---- the evaluation set
    preds, gts = ap_ref.build_eval_case(0)
    ap_ref.check_eval_case(preds, gts, THRESHOLDS)
    save["ev_pred_count"] = np.array([len(p) for p in preds], dtype=np.int64)
    save["ev_pred_cls"] = np.array([c for p in preds for c, _, _ in p], dtype=np.int64)
    save["ev_pred_corners"] = np.array([b for p in preds for _, b, _ in p], dtype=np.float64).reshape(-1, 8, 3)
    save["ev_pred_score"] = np.array([s for p in preds for _, _, s in p], dtype=np.float64)
    save["ev_gt_count"] = np.array([len(g) for g in gts], dtype=np.int64)
    save["ev_gt_cls"] = np.array([c for g in gts for c, _ in g], dtype=np.int64)
    save["ev_gt_corners"] = np.array([b for g in gts for _, b in g], dtype=np.float64).reshape(-1, 8, 3)
    save["ev_thresholds"] = np.array(THRESHOLDS)
    pred_all, gt_all = dict(enumerate(preds)), dict(enumerate(gts))
    for t, thr in enumerate(THRESHOLDS):
        rec, prec, apv = eval_det(pred_all, gt_all, ovthresh=thr, get_iou_func=get_iou_obb)
        save["ev_t%d_classes" % t] = np.array(sorted(apv), dtype=np.int64)
        for c in sorted(apv):
            save["ev_t%d_c%d_rec" % (t, c)], save["ev_t%d_c%d_prec" % (t, c)] = np.asarray(rec[c]), np.asarray(prec[c])
            save["ev_t%d_c%d_ap" % (t, c)] = np.array(apv[c], dtype=np.float64)
        calc = ap.APCalculator(thr)
        calc.step(preds[:3], gts[:3])
        calc.step(preds[3:], gts[3:])
        m = calc.compute_metrics()
        for c in sorted(apv):       # the multiprocessing path on its well-defined branch agrees with eval_det
            assert m["%d Average Precision" % c] == apv[c]
        save["ev_t%d_metric_keys" % t] = np.array(list(m.keys()))
        save["ev_t%d_metric_values" % t] = np.array([float(x) for x in m.values()], dtype=np.float64)
        print("threshold", thr, "mAP", m["mAP"], "AR", m["AR"], "detections", int(save["ev_pred_count"].sum()))
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
