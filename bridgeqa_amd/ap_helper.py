"""Post-processing of the detector's proposals -- mirror of the reference's lib/ap_helper.py:40-178 `parse_predictions`
(the evaluation path: lib/eval_helper.py:71, scripts/eval.py:495, scripts/predict.py): decode the
proposal boxes, drop the empty ones, run the (2-D / 3-D / per-class 3-D) greedy NMS, build `pred_mask` and
`batch_pred_map_cls`.  Same function name, arguments (`end_points`, `config_dict` with the reference's keys) and outputs.

What changes underneath: the reference loops over B x K proposals in Python with a device->host sync per scalar, tests
every box against all N points with a scipy Delaunay hull and runs numpy NMS per scene; here the decode is batched on the
device (proposal_module.box_corners), the point-in-box count and the NMS are HIP kernels (csrc/nms.hip), and the host sees
ONE copy of the small result tensors at the end (the list-of-tuples format of batch_pred_map_cls is host data by
definition).  `ScannetDatasetConfig` (absent from the reference checkout): num_heading_bin, num_class and mean_size_arr
are read from config_dict['dataset_config'] (class2angle / class2size restated as in loss_helper._class2angle).

The module's other two public pieces, as scripts/eval.py:442-507 imports them: `parse_groundtruths` (:180-223, one batched
float64 decode instead of a host loop with a sync per scalar) and `APCalculator` (:225-278 over utils/eval_det.py and
utils/box_util.py box3d_iou), whose matching and curves run on the device (csrc/ap_eval.hip).  `pack_predictions` /
`pack_groundtruths` are the device-resident forms of the two lists: fixed shapes, nothing compacted, nothing copied."""
import numpy as np
import torch

from . import _ext
from .loss_helper import _class2angle
from .proposal_module import box_corners


def softmax(x):
    """ap_helper.py:33-38 (numpy)"""
    probs = np.exp(x - np.max(x, axis=len(x.shape) - 1, keepdims=True))
    return probs / np.sum(probs, axis=len(x.shape) - 1, keepdims=True)


def _decode_predictions(end_points, config_dict):
    """the device half of parse_predictions: decode, empty-box test, NMS -- no device -> host transfer.  Returns corners
    (B, K, 8, 3) f32, their min / max (B, K, 3), keep (B, K) bool, obj_prob (B, K), pred_sem_cls (B, K), sem_probs (B, K, C)"""
    cfg = config_dict["dataset_config"]
    center = end_points["center"].detach().float().contiguous()                       # (B, K, 3)
    B, K = center.shape[:2]
    dev = center.device
    hcls = torch.argmax(end_points["heading_scores"], -1)
    hres = torch.gather(end_points["heading_residuals"], 2, hcls.unsqueeze(-1)).squeeze(2).detach().float()
    scls = torch.argmax(end_points["size_scores"], -1)
    sres = torch.gather(end_points["size_residuals"], 2,
                        scls.unsqueeze(-1).unsqueeze(-1).repeat(1, 1, 1, 3)).squeeze(2).detach().float()
    pred_sem_cls = torch.argmax(end_points["sem_cls_scores"], -1)
    sem_probs = torch.softmax(end_points["sem_cls_scores"].detach().float(), -1)
    mean_size = torch.from_numpy(np.asarray(cfg.mean_size_arr, dtype=np.float32)).to(dev)
    heading = _class2angle(cfg, hcls, hres).contiguous()            # class2angle(..., to_label_format=True)
    size = (mean_size[scls] + sres).contiguous()                    # class2size
    corners = box_corners(center, size, heading)                    # get_3d_box, (B, K, 8, 3)
    nonempty = torch.ones(B, K, dtype=torch.bool, device=dev)
    if config_dict["remove_empty_box"]:
        pc = end_points["point_clouds"]
        pc = pc if (pc.dtype == torch.float32 and pc.is_contiguous()) else pc.float().contiguous()
        nonempty = _ext.box_point_count(pc, center, size, heading, cap=5) >= 5       # ap_helper.py:98 `< 5` -> empty
    obj_prob = torch.softmax(end_points["objectness_scores"].detach().float(), -1)[:, :, 1]
    lo, hi = corners.min(dim=2).values, corners.max(dim=2).values   # (B, K, 3)
    if not config_dict["use_3d_nms"]:
        # bird's-eye boxes over the x and z axes (ap_helper.py:108-113)
        zero, one = torch.zeros_like(lo[..., 0]), torch.ones_like(lo[..., 0])
        box = torch.stack([lo[..., 0], lo[..., 2], zero, hi[..., 0], hi[..., 2], one], -1)
        keep = _ext.nms(box, obj_prob, config_dict["nms_iou"], valid=nonempty, old_type=config_dict["use_old_type_nms"])
    else:
        box = torch.cat([lo, hi], -1)
        same = bool(config_dict.get("cls_nms", False))
        keep = _ext.nms(box, obj_prob, config_dict["nms_iou"], cls=pred_sem_cls if same else None, valid=nonempty,
                        old_type=config_dict["use_old_type_nms"], same_cls=same)
    return corners, lo, hi, keep, obj_prob, pred_sem_cls, sem_probs


def parse_predictions(end_points, config_dict):
    cfg = config_dict["dataset_config"]
    corners, _, _, keep, obj_prob, pred_sem_cls, sem_probs = _decode_predictions(end_points, config_dict)
    B, K = keep.shape
    # ---- the one device -> host hand-over
    keep_h, obj_h, cls_h = keep.cpu().numpy(), obj_prob.cpu().numpy(), pred_sem_cls.cpu().numpy()
    corners_h, sem_h = corners.cpu().numpy().astype(np.float64), sem_probs.cpu().numpy()
    assert keep_h.any(axis=1).all()                                  # ap_helper.py:117 `assert(len(pick)>0)`
    end_points["pred_mask"] = keep_h.astype(np.float64)
    end_points["pred_mask_device"] = keep
    batch_pred_map_cls = []
    for i in range(B):
        sel = [j for j in range(K) if keep_h[i, j] and obj_h[i, j] > config_dict["conf_thresh"]]
        if config_dict["per_class_proposal"]:
            cur = []
            for ii in range(cfg.num_class):
                cur += [(ii, corners_h[i, j], sem_h[i, j, ii] * obj_h[i, j]) for j in sel]
            batch_pred_map_cls.append(cur)
        else:
            batch_pred_map_cls.append([(int(cls_h[i, j]), corners_h[i, j], obj_h[i, j]) for j in sel])
    end_points["batch_pred_map_cls"] = batch_pred_map_cls
    return batch_pred_map_cls


# ---- ground truth (ap_helper.py:180-223) -------------------------------------------------------------------------------
def _decode_groundtruths(end_points, config_dict):
    """all B x K2 label boxes decoded in one batch on the labels' device, in float64 as the reference's numpy loop does
    (class2angle, class2size, get_3d_box); masked rows are decoded too and dropped by the caller.  -> (B, K2, 8, 3) f64"""
    cfg = config_dict["dataset_config"]
    center = end_points["center_label"][:, :, 0:3].detach().double()
    dev = center.device
    hcls = end_points["heading_class_label"].detach().long()
    hres = end_points["heading_residual_label"].detach().double()
    scls = end_points["size_class_label"].detach().long()
    sres = end_points["size_residual_label"].detach().double()
    mean_size = torch.from_numpy(np.asarray(cfg.mean_size_arr, dtype=np.float64)).to(dev)
    heading = _class2angle(cfg, hcls, hres)
    size = mean_size[scls] + sres
    return box_corners(center, size, heading)


def parse_groundtruths(end_points, config_dict):
    """ap_helper.py:180-223: same keys, same return value and side effect (end_points['batch_gt_map_cls']): per scene the
    list of (int class, (8, 3) float64 corners) of the rows with box_label_mask == 1, in row order.  One batched float64
    decode on the device and one hand-over to the host instead of a device -> host copy per scalar."""
    corners = _decode_groundtruths(end_points, config_dict)
    corners_h = corners.cpu().numpy()
    mask_h = end_points["box_label_mask"].detach().cpu().numpy()
    cls_h = end_points["sem_cls_label"].detach().cpu().numpy()
    batch_gt_map_cls = []
    for i in range(corners_h.shape[0]):
        batch_gt_map_cls.append([(cls_h[i, j].item(), corners_h[i, j]) for j in range(corners_h.shape[1]) if mask_h[i, j] == 1])
    end_points["batch_gt_map_cls"] = batch_gt_map_cls
    return batch_gt_map_cls


# ---- device-resident forms ---------------------------------------------------------------------------------------------------
class PackedPredictions(object):
    """fixed-shape, device-resident form of batch_pred_map_cls: ext (B, K, 6) f64 = min / max of the fp32 corners; score
    (B, K, C) f32 = sem_prob * obj_prob (per-class proposals, entry (b, k, c) is a detection of class c) or score (B, K)
    f32 = obj_prob with cls (B, K); valid (B, K) bool = kept by NMS and obj_prob > conf_thresh.  Nothing is compacted."""

    def __init__(self, ext, score, cls, valid, num_class):
        self.ext, self.score, self.cls, self.valid, self.num_class = ext, score, cls, valid, int(num_class)


class PackedGroundTruths(object):
    """fixed-shape, device-resident form of batch_gt_map_cls: ext (B, K2, 6) f64, cls (B, K2), valid (B, K2) bool"""

    def __init__(self, ext, cls, valid, num_class):
        self.ext, self.cls, self.valid, self.num_class = ext, cls, valid, int(num_class)


def pack_predictions(end_points, config_dict):
    """parse_predictions without the host: the same decode / empty-box test / NMS, the result left on the device in fixed
    shapes (no nonzero, no synchronisation) for APCalculator.step.  The list form's entries are exactly the (b, k[, c])
    with valid[b, k], in the list's order (class-major, then k, for per-class proposals)."""
    cfg = config_dict["dataset_config"]
    _, lo, hi, keep, obj_prob, pred_sem_cls, sem_probs = _decode_predictions(end_points, config_dict)
    ext = torch.cat([lo, hi], -1).double()
    valid = keep & (obj_prob > config_dict["conf_thresh"])
    if config_dict["per_class_proposal"]:
        return PackedPredictions(ext, sem_probs[:, :, :cfg.num_class] * obj_prob.unsqueeze(-1), None, valid, cfg.num_class)
    return PackedPredictions(ext, obj_prob, pred_sem_cls, valid, cfg.num_class)


def pack_groundtruths(end_points, config_dict):
    """parse_groundtruths without the host: extents of the float64 corners of every label row, its class and its mask"""
    corners = _decode_groundtruths(end_points, config_dict)
    ext = torch.cat([corners.min(dim=2).values, corners.max(dim=2).values], -1)
    num_class = getattr(config_dict["dataset_config"], "num_class", None)
    if num_class is None:
        raise ValueError("pack_groundtruths: dataset_config.num_class is needed (classes are not read back from the device)")
    return PackedGroundTruths(ext, end_points["sem_cls_label"].detach().long(), end_points["box_label_mask"].detach() == 1,
                              num_class)


# ---- the segment algorithm on the host (numpy): the slow path ---------------------------------------------------------
_AP_CHUNK = 256          # = the workgroup of ap_curve_kernel: the AP sum below repeats its order of additions


def _np_iou_matrix(a, g):
    """box_util.py:112-123 for every pair: a (n, 6), g (m, 6) extents -> (n, m); the reference's operations in its order"""
    xA, yA, zA = (np.maximum(a[:, None, k], g[None, :, k]) for k in range(3))
    xB, yB, zB = (np.minimum(a[:, None, k + 3], g[None, :, k + 3]) for k in range(3))
    inter = np.maximum(xB - xA, 0) * np.maximum(yB - yA, 0) * np.maximum(zB - zA, 0)
    va = (a[:, 3] - a[:, 0]) * (a[:, 4] - a[:, 1]) * (a[:, 5] - a[:, 2])
    vg = (g[:, 3] - g[:, 0]) * (g[:, 4] - g[:, 1]) * (g[:, 5] - g[:, 2])
    return inter / (va[:, None] + vg[None, :] - inter + 1e-8)


def _np_match(box_tab, det_box, gt_tab, seg_det, seg_gt, thr):
    """what bq_ap_match computes, segment by segment"""
    D, T = len(det_box), len(thr)
    tp = np.zeros((T, D), dtype=np.uint8)
    ovmax = np.full(D, -np.inf)
    jmax = np.full(D, -1, dtype=np.int32)
    for s in np.nonzero((seg_det[1:] > seg_det[:-1]) & (seg_gt[1:] > seg_gt[:-1]))[0]:
        d0, d1, g0, g1 = seg_det[s], seg_det[s + 1], seg_gt[s], seg_gt[s + 1]
        iou = _np_iou_matrix(box_tab[det_box[d0:d1]], gt_tab[g0:g1])
        jm = np.argmax(iou, axis=1)                       # first maximum = lowest index
        ov = iou[np.arange(d1 - d0), jm]
        ovmax[d0:d1], jmax[d0:d1] = ov, jm
        for t in range(T):
            cand = np.nonzero(ov > thr[t])[0]             # in score order: the first claim of a box wins it
            if len(cand):
                tp[t, d0 + cand[np.unique(jm[cand], return_index=True)[1]]] = 1
    return tp, ovmax, jmax


def _np_curve(tp, cls_off, npos):
    """what bq_ap_curve computes, its order of additions included"""
    T, D = tp.shape
    C = len(npos)
    rec, prec = np.zeros((T, D)), np.zeros((T, D))
    ap, last = np.zeros((C, T)), np.zeros((C, T))
    for c in range(C):
        c0, c1 = cls_off[c], cls_off[c + 1]
        n = c1 - c0
        if n == 0:
            continue
        for t in range(T):
            x = tp[t, c0:c1].astype(np.float64)
            tpc, fpc = np.cumsum(x), np.cumsum(1.0 - x)
            r = tpc / (npos[c] + 1e-8)
            p = tpc / np.maximum(tpc + fpc, np.finfo(np.float64).eps)
            env = np.maximum(np.maximum.accumulate(p[::-1])[::-1], 0.0)
            rp = np.concatenate(([0.0], r[:-1]))
            term = np.where(r != rp, (r - rp) * env, 0.0)
            rows = np.zeros(-(-n // _AP_CHUNK) * _AP_CHUNK)
            rows[:n] = term
            rows = rows.reshape(-1, _AP_CHUNK)
            acc = np.zeros(_AP_CHUNK)
            for ch in range(rows.shape[0] - 1, -1, -1):
                acc = acc + rows[ch]
            s = _AP_CHUNK // 2
            while s > 0:
                acc[:s] = acc[:s] + acc[s:2 * s]
                s //= 2
            rec[t, c0:c1], prec[t, c0:c1], ap[c, t], last[c, t] = r, p, acc[0], r[-1]
    return rec, prec, ap, last


def _extents(corners):
    c = np.asarray(corners, dtype=np.float64).reshape(-1, 8, 3)
    return np.concatenate([c.min(axis=1), c.max(axis=1)], -1)


class APCalculator(object):
    """lib/ap_helper.py:225-278 APCalculator -- `step`, `compute_metrics`, `reset` with the reference's signatures and
    compute_metrics' dict ('<name> Average Precision' per class in sorted key order, 'mAP', '<name> Recall', 'AR'; names
    from class2type_map, else str(key)) -- over utils/eval_det.py's eval_det_cls / voc_ap (non-07 metric) with box3d_iou.

    `step` takes the reference's host lists (batch_pred_map_cls, batch_gt_map_cls) or the device-resident pair
    (pack_predictions, pack_groundtruths); scans are numbered in arrival order.  A packed step transfers nothing.
    `compute_metrics` groups the detections into (class, scene) segments with torch sorts, matches every segment in one
    bq_ap_match launch, forms every curve in one bq_ap_curve launch and copies the per-class results to the host ONCE.
    Without a GPU (host lists or CPU tensors) the same segment algorithm runs in numpy -- the slow path, bit for bit the
    same results.

    Meaning: eval_det's per-class one.  The class set is the union of predicted and ground-truth classes; a class with
    ground truth and no detection has AP 0 and Recall 0.  (The reference's eval_det_multiprocessing hands such a class the
    NEXT class's results to its successors -- `ret_values[i]` is indexed over all classes, filled over the predicted ones,
    utils/eval_det.py:225-229; that slip is not reproduced.)

    Ties: the reference's np.argsort(-confidence) leaves equal scores in unspecified order.  Here the order is defined:
    score descending, then scan number, then position in the scene's list.

    Extension: ap_iou_thresh may be a sequence of up to 4 thresholds; compute_metrics then returns {threshold: dict} from
    one matching pass."""

    def __init__(self, ap_iou_thresh=0.25, class2type_map=None):
        self.ap_iou_thresh = ap_iou_thresh
        self._multi = isinstance(ap_iou_thresh, (tuple, list, np.ndarray))
        self._thr = tuple(float(t) for t in ap_iou_thresh) if self._multi else (float(ap_iou_thresh),)
        if not 1 <= len(self._thr) <= 4:
            raise ValueError("APCalculator: 1 to 4 thresholds, got %d" % len(self._thr))
        self.class2type_map = class2type_map
        self.reset()

    def reset(self):
        self.gt_map_cls = {}      # {scan_id: [(classname, bbox)]}          (host-list steps, as the reference keeps them)
        self.pred_map_cls = {}    # {scan_id: [(classname, bbox, score)]}
        self._steps = []          # (first scan number, batch size, predictions, ground truths) in arrival order
        self.scan_cnt = 0

    def step(self, batch_pred_map_cls, batch_gt_map_cls):
        packed = isinstance(batch_pred_map_cls, PackedPredictions), isinstance(batch_gt_map_cls, PackedGroundTruths)
        if packed[0] != packed[1]:
            raise TypeError("APCalculator.step: predictions and ground truths must both be lists or both be packed")
        bsize = batch_pred_map_cls.ext.shape[0] if packed[0] else len(batch_pred_map_cls)
        assert bsize == (batch_gt_map_cls.ext.shape[0] if packed[0] else len(batch_gt_map_cls))
        self._steps.append((self.scan_cnt, bsize, batch_pred_map_cls, batch_gt_map_cls))
        if not packed[0]:
            for i in range(bsize):
                self.gt_map_cls[self.scan_cnt + i] = batch_gt_map_cls[i]
                self.pred_map_cls[self.scan_cnt + i] = batch_pred_map_cls[i]
        self.scan_cnt += bsize

    # ---- flat tables ----------------------------------------------------------------------------------------------------
    def _device(self, backend):
        devs = [p.ext.device for _, _, p, _ in self._steps if isinstance(p, PackedPredictions)]
        cuda = [d for d in devs if d.type == "cuda"]
        if backend == "numpy":
            return torch.device("cpu")
        if backend == "device" or cuda or (not devs and torch.cuda.is_available()):
            if not (cuda or torch.cuda.is_available()):
                raise RuntimeError("APCalculator: the device path needs a GPU")
            return cuda[0] if cuda else torch.device("cuda", torch.cuda.current_device())
        return torch.device("cpu")

    def _tables(self, dev):
        """every detection slot and ground-truth slot of every step as flat columns on `dev`, in arrival order (scan, then
        list position); class keys mapped to their rank among the sorted keys"""
        host_keys, n_packed = set(), 0
        for _, _, p, g in self._steps:
            if isinstance(p, PackedPredictions):
                n_packed = max(n_packed, p.num_class, g.num_class)
            else:
                host_keys.update(c for lst in p for c, _, _ in lst)
                host_keys.update(c for lst in g for c, _ in lst)
        keys = sorted(host_keys | set(range(n_packed)))
        rank = {k: i for i, k in enumerate(keys)}
        lut = torch.tensor([rank[c] for c in range(n_packed)], dtype=torch.int64, device=dev) if n_packed else None
        i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)
        det = dict(scene=[], cls=[], score=[], box=[], valid=[])
        gt = dict(scene=[], cls=[], ext=[], valid=[])
        boxes, n_box, max_gt = [], 0, 0
        for scan0, B, p, g in self._steps:
            if isinstance(p, PackedPredictions):
                K = p.ext.shape[1]
                scene = torch.arange(scan0, scan0 + B, device=dev)
                box = n_box + torch.arange(B * K, device=dev).view(B, K)
                if p.cls is None:
                    C = p.score.shape[2]
                    shape = (B, K, C)
                    cols = (scene.view(B, 1, 1), lut[:C].view(1, 1, C), p.score.to(dev).double(), box.view(B, K, 1),
                            p.valid.to(dev).view(B, K, 1))
                else:
                    shape = (B, K)
                    cols = (scene.view(B, 1), lut[p.cls.to(dev).long().clamp(0, n_packed - 1)], p.score.to(dev).double(), box,
                            p.valid.to(dev))
                for name, col in zip(("scene", "cls", "score", "box", "valid"), cols):
                    det[name].append(col.expand(shape).reshape(-1))
                boxes.append(p.ext.to(dev).reshape(-1, 6))
                n_box += B * K
                K2 = g.ext.shape[1]
                gt["scene"].append(scene.view(B, 1).expand(B, K2).reshape(-1))
                gt["cls"].append(lut[g.cls.to(dev).long().clamp(0, n_packed - 1)].reshape(-1))
                gt["ext"].append(g.ext.to(dev).reshape(-1, 6))
                gt["valid"].append(g.valid.to(dev).reshape(-1))
                max_gt = max(max_gt, K2)
            else:
                n = [len(lst) for lst in p]
                det["scene"].append(i64(np.repeat(np.arange(scan0, scan0 + B), n)))
                det["cls"].append(i64([rank[c] for lst in p for c, _, _ in lst]))
                det["score"].append(torch.as_tensor(np.asarray([s for lst in p for _, _, s in lst], dtype=np.float64)).to(dev))
                det["box"].append(n_box + torch.arange(sum(n), device=dev))
                det["valid"].append(torch.ones(sum(n), dtype=torch.bool, device=dev))
                boxes.append(torch.as_tensor(_extents([c for lst in p for _, c, _ in lst])).to(dev))
                n_box += sum(n)
                m = [len(lst) for lst in g]
                gt["scene"].append(i64(np.repeat(np.arange(scan0, scan0 + B), m)))
                gt["cls"].append(i64([rank[c] for lst in g for c, _ in lst]))
                gt["ext"].append(torch.as_tensor(_extents([c for lst in g for _, c in lst])).to(dev))
                gt["valid"].append(torch.ones(sum(m), dtype=torch.bool, device=dev))
                for lst in g:
                    cnt = {}
                    for c, _ in lst:
                        cnt[c] = cnt.get(c, 0) + 1
                    max_gt = max([max_gt] + list(cnt.values()))
        cat = lambda d: {k: torch.cat(v) for k, v in d.items()}
        return keys, cat(det), cat(gt), torch.cat(boxes), max_gt

    def _evaluate(self, backend=None):
        """-> (keys, device-or-numpy arrays): see compute_metrics / eval_det"""
        if not self._steps:
            raise ValueError("APCalculator: no step was taken")
        dev = self._device(backend)
        keys, det, gt, box_tab, max_gt = self._tables(dev)
        NC, NS = len(keys), self.scan_cnt
        S = NC * NS
        # detections: stable sorts -- arrival order already is (scan, position), so sorting by score and then by the
        # segment (or the class) leaves ties in (scan, position) order
        seg = torch.where(det["valid"], det["cls"] * NS + det["scene"], torch.full_like(det["cls"], S))
        clk = torch.where(det["valid"], det["cls"], torch.full_like(det["cls"], NC))
        p1 = torch.sort(det["score"], descending=True, stable=True).indices
        seg_sorted, pm = torch.sort(seg[p1], stable=True)
        cls_sorted, pc = torch.sort(clk[p1], stable=True)
        order_m, order_c = p1[pm], p1[pc]                       # match order: (segment, score); curve order: (class, score)
        D = order_m.numel()
        seg_det = torch.searchsorted(seg_sorted, torch.arange(S + 1, device=dev)).int()
        cls_off = torch.searchsorted(cls_sorted, torch.arange(NC + 1, device=dev)).int()
        det_box = det["box"][order_m].int()
        gseg = torch.where(gt["valid"], gt["cls"] * NS + gt["scene"], torch.full_like(gt["cls"], S))
        gseg_sorted, pg = torch.sort(gseg, stable=True)
        gt_tab = gt["ext"][pg].contiguous()
        seg_gt = torch.searchsorted(gseg_sorted, torch.arange(S + 1, device=dev)).int()
        npos = (seg_gt[1:] - seg_gt[:-1]).view(NC, NS).sum(1).double()
        inv_m = torch.empty(D, dtype=torch.int64, device=dev)
        inv_m[order_m] = torch.arange(D, device=dev)
        to_curve = inv_m[order_c]
        box_tab = box_tab.contiguous()
        if dev.type == "cuda":
            tp, _, _ = _ext.ap_match(box_tab, det_box, gt_tab, seg_det, seg_gt, self._thr, max_seg_gt=max_gt)
            rec, prec, ap, last = _ext.ap_curve(tp[:, to_curve].contiguous(), cls_off, npos)
            ndet = (cls_off[1:] - cls_off[:-1]).double()
            small = torch.cat([ap.reshape(-1), last.reshape(-1), ndet, npos]).cpu().numpy()   # the one device -> host copy
        else:
            n = lambda t: t.numpy()
            tp, _, _ = _np_match(n(box_tab), n(det_box), n(gt_tab), n(seg_det), n(seg_gt), self._thr)
            rec, prec, ap, last = _np_curve(np.ascontiguousarray(tp[:, n(to_curve)]), n(cls_off), n(npos))
            ndet = (n(cls_off)[1:] - n(cls_off)[:-1]).astype(np.float64)
            small = np.concatenate([ap.reshape(-1), last.reshape(-1), ndet, n(npos)])
        T = len(self._thr)
        ap, last = small[:NC * T].reshape(NC, T), small[NC * T:2 * NC * T].reshape(NC, T)
        ndet, npos = small[2 * NC * T:2 * NC * T + NC], small[2 * NC * T + NC:]
        present = [c for c in range(NC) if ndet[c] > 0 or npos[c] > 0]
        return keys, present, ap, last, (rec, prec, cls_off)

    def eval_det(self, backend=None):
        """{threshold: (rec, prec, ap)} with rec / prec {class: array over the class's detections in confidence order} and
        ap {class: float}, as utils/eval_det.py eval_det returns them (the curves are copied from the device: diagnostics)"""
        keys, present, ap, _, (rec, prec, cls_off) = self._evaluate(backend)
        if isinstance(rec, torch.Tensor):
            rec, prec, cls_off = rec.cpu().numpy(), prec.cpu().numpy(), cls_off.cpu().numpy()
        elif isinstance(cls_off, torch.Tensor):
            cls_off = cls_off.numpy()
        out = {}
        for t, thr in enumerate(self._thr):
            sl = {c: slice(cls_off[c], cls_off[c + 1]) for c in present}
            out[thr] = ({keys[c]: rec[t, sl[c]] for c in present}, {keys[c]: prec[t, sl[c]] for c in present},
                        {keys[c]: float(ap[c, t]) for c in present})
        return out

    def compute_metrics(self, backend=None):
        """Use accumulated predictions and groundtruths to compute Average Precision (the reference's dict; one dict per
        threshold, keyed by threshold, when ap_iou_thresh is a sequence).  backend: None = the device when the steps hold
        device tensors or a GPU is present, else numpy; 'numpy' / 'device' force one."""
        keys, present, ap, last, _ = self._evaluate(backend)
        out = {}
        for t, thr in enumerate(self._thr):
            ret_dict = {}
            name = lambda c: self.class2type_map[keys[c]] if self.class2type_map else str(keys[c])
            for c in present:
                ret_dict["%s Average Precision" % name(c)] = float(ap[c, t])
            ret_dict["mAP"] = np.mean([ap[c, t] for c in present])
            for c in present:
                ret_dict["%s Recall" % name(c)] = float(last[c, t])
            ret_dict["AR"] = np.mean([last[c, t] for c in present])
            out[thr] = ret_dict
        return out if self._multi else out[self._thr[0]]
