"""The definition of training-scene preparation in plain numpy: the yardstick of tests/test_scene_prep_cpu.py and
tests/test_scene_prep_gpu.py (and the host column of tools/bench_scene_prep.py).  Written from the reference's
ScannetQADataset.__getitem__ (lib/dataset.py:415-515, 537-573, 598-603, 803-816) and utils/pc_utils.py:275-313; it shares no
code with bridgeqa_amd/scene_data.py.

A scene is a dict: rows (P, D) fp32 with xyz first, instance_labels (P), semantic_labels (P), instance_bboxes (K, 8) fp64 =
cx cy cz dx dy dz nyu40id object-id.  A sample's parameters are a dict: choices (N), flip_x, flip_y in {1, -1}, angles
(ax, ay, az), translation (3) fp64 -- what scene_data.draw_params returns.  `augment=False` reads only `choices`.

Arithmetic, as the reference has it: the points are an fp32 array; a rotation is np.dot(xyz, R^T) in fp64 assigned back into the
fp32 array (rotate_points writes the order of the three products and two sums out; test_scene_prep_cpu.py holds it to np.dot
bit for bit); the translation is an in-place += of fp64 factors; the boxes are fp64 until the final astype(float32); the votes
are fp32."""
import numpy as np


def rotx(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def roty(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rotz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def dot_rt(v, R):
    """v . R^T for v (n, 3) and R (3, 3), in fp64: (x R^T[0][j] + y R^T[1][j]) + z R^T[2][j], each operation rounded on its own"""
    v = np.asarray(v, dtype=np.float64)
    Rt = np.transpose(np.asarray(R, dtype=np.float64))
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    return (x * Rt[0][None, :] + y * Rt[1][None, :]) + z * Rt[2][None, :]


def rotate_points(xyz32, R):
    """point_cloud[:, 0:3] = np.dot(point_cloud[:, 0:3], np.transpose(rot_mat)) on an fp32 array"""
    assert xyz32.dtype == np.float32
    return dot_rt(xyz32, R).astype(np.float32)


def rotate_aligned_boxes_along_axis(boxes, R, axis):
    """boxes (G, 6) fp64 -> (G, 6): the centre turns, the extent along `axis` stays, each of the other two becomes twice the
    largest coordinate of the four turned corners (+-e1/2, +-e2/2, 0 on the axis).  For axis 'z' this is VoteNet's
    rotate_aligned_boxes.  (The reference imports this helper from a file its tree does not hold: the x / y forms are this
    project's reading of it.)"""
    a = "xyz".index(axis)
    p, q = [k for k in range(3) if k != a]
    half = boxes[:, 3:6] / 2.0
    reach = np.zeros((boxes.shape[0], 4, 2))                   # per corner: its turned p and q coordinates
    for k, (sp, sq) in enumerate([(-1, -1), (1, -1), (1, 1), (-1, 1)]):
        corner = np.zeros((boxes.shape[0], 3))
        corner[:, p] = sp * half[:, p]
        corner[:, q] = sq * half[:, q]
        turned = dot_rt(corner, R)
        reach[:, k, 0], reach[:, k, 1] = turned[:, p], turned[:, q]
    out = np.empty_like(boxes)
    out[:, 0:3] = dot_rt(boxes[:, 0:3], R)
    out[:, 3 + a] = boxes[:, 3 + a]
    out[:, 3 + p] = 2.0 * reach[:, :, 0].max(axis=1)
    out[:, 3 + q] = 2.0 * reach[:, :, 1].max(axis=1)
    return out


def prepare_sample(scene, params, nyu40ids, nyu40id2class, mean_size_arr, max_boxes=128, augment=True, object_id=-1):
    """one sample's data dict (numpy, the dtypes of lib/dataset.py:551-603)"""
    G = max_boxes
    sizes = np.asarray(mean_size_arr, dtype=np.float64)
    pick = np.asarray(params["choices"])
    N = pick.shape[0]
    pts = scene["rows"][pick]                                  # a copy, fp32; the feature columns are never touched again
    assert pts.dtype == np.float32
    inst = np.asarray(scene["instance_labels"])[pick]
    sem = np.asarray(scene["semantic_labels"])[pick]
    raw = np.asarray(scene["instance_bboxes"], dtype=np.float64)
    n_box = min(raw.shape[0], G)
    boxes = np.full((G, 6), -100.0)                            # padding rows: an impossible position; they are augmented too
    boxes[:n_box] = raw[:n_box, 0:6]

    if augment:
        flip_x, flip_y = int(params["flip_x"]), int(params["flip_y"])
        for col, flip in ((0, flip_x), (1, flip_y)):
            if flip == -1:
                pts[:, col] = -1 * pts[:, col]
                boxes[:, col] = -1 * boxes[:, col]
        total = None
        for axis, make, angle in zip("xyz", (rotx, roty, rotz), params["angles"]):
            rot = make(angle)
            pts[:, 0:3] = rotate_points(pts[:, 0:3], rot)
            boxes = rotate_aligned_boxes_along_axis(boxes, rot, axis)
            total = rot if total is None else np.dot(rot, total)            # Rx, then Ry Rx, then Rz Ry Rx
        shift = np.array([params["translation"][0], params["translation"][1], params["translation"][2]], dtype=np.float64)
        pts[:, 0:3] += shift                                   # fp32 array += fp64 factors: the fp64 sum, rounded once
        boxes[:, 0:3] += shift

    # votes, after the augmentation: an instance votes iff its first sampled point carries a voting semantic label
    votes = np.zeros((N, 3))
    voting = np.zeros(N)
    for ident in np.unique(inst):
        members = np.flatnonzero(inst == ident)
        if sem[members[0]] not in nyu40ids:
            continue
        xyz = pts[members, 0:3]
        votes[members] = 0.5 * (xyz.min(axis=0) + xyz.max(axis=0)) - xyz    # fp32 arithmetic, stored into fp64 exactly
        voting[members] = 1

    classes = np.zeros(G)
    residuals = np.zeros((G, 3))
    cls = [nyu40id2class[int(i)] for i in raw[:n_box, 6]]
    classes[:n_box] = cls
    residuals[:n_box] = boxes[:n_box, 3:6] - sizes[cls]

    has_ref = object_id is not None and object_id >= 0
    is_ref = np.zeros(G)
    ref_center, ref_class, ref_residual = np.zeros(3), 0, np.zeros(3)
    if has_ref:
        for i in range(n_box):                                 # the LAST matching box leaves its labels
            if raw[i, 7] == object_id:
                is_ref[i] = 1
                ref_center, ref_class, ref_residual = boxes[i, 0:3], classes[i], residuals[i]

    mask = np.zeros(G)
    mask[:n_box] = 1
    d = {
        "point_clouds": pts.astype(np.float32),
        "vote_label": np.tile(votes, (1, 3)).astype(np.float32),
        "vote_label_mask": voting.astype(np.int64),
        "center_label": boxes.astype(np.float32)[:, 0:3],
        "target_bboxes": boxes.astype(np.float32),
        "size_residual_label": residuals.astype(np.float32),
        "heading_residual_label": np.zeros(G, dtype=np.float32),
        "box_label_mask": mask.astype(np.float32),
        "heading_class_label": np.zeros(G, dtype=np.int64),
        "size_class_label": classes.astype(np.int64),
        "sem_cls_label": classes.astype(np.int64),
        "ref_box_label": is_ref.astype(np.int64),
        "num_bbox": np.array(n_box).astype(np.int64),
        "ref_obj_mask": np.array(has_ref).astype(np.int64),
        "ref_center_label": np.asarray(ref_center).astype(np.float32),
        "ref_size_class_label": np.array(int(ref_class)).astype(np.int64),
        "ref_size_residual_label": np.asarray(ref_residual).astype(np.float32),
    }
    if augment:
        d.update(flip_x=np.array(flip_x).astype(np.int64), flip_y=np.array(flip_y).astype(np.int64),
                 rot_mat=total.astype(np.float32), translation=shift.astype(np.float32))
    return d


def prepare_batch(scenes, scene_index, params, nyu40ids, nyu40id2class, mean_size_arr, max_boxes=128, augment=True,
                  object_ids=None):
    """the default collate over prepare_sample: every key stacked along a new first axis"""
    object_ids = [-1] * len(scene_index) if object_ids is None else object_ids
    samples = [prepare_sample(scenes[s], p, nyu40ids, nyu40id2class, mean_size_arr, max_boxes, augment, o)
               for s, p, o in zip(scene_index, params, object_ids)]
    return {k: np.stack([d[k] for d in samples]) for k in samples[0]}
