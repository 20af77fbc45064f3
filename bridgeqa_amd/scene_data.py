"""Training scenes prepared where they are consumed: the scenes stay resident on the device, and a batch of detector inputs and
labels -- what ScannetQADataset.__getitem__ builds per sample with numpy and the loader then collates, pins and uploads (reference
lib/dataset.py:415-515, 537-573, 598-603, 803-816) -- is three launches of csrc/scene_prep.hip under the reference's data-dict keys.

    store = SceneStore(scenes, device, DC.nyu40ids, DC.nyu40id2class, DC.mean_size_arr)      # once
    batcher = SceneBatcher(store, num_points=40000, augment=True)
    batch = batcher.prepare(scene_index, object_ids, out=stager.next_batch)                  # per step, in place

A scene record is a dict: rows (P, D) fp32 with xyz first and the static features behind it (colour, normals, height, multiview:
the reference computes all of them before it samples, so they are only gathered), instance_labels (P), semantic_labels (P),
instance_bboxes (K, 8) = cx cy cz dx dy dz nyu40id object-id.

On a CPU device the same definition runs in numpy, operation for operation (the same bits): that is what the CPU tests hold
against tests/sceneprep_ref.py.  On a CUDA device there is no fallback: the kernels run or prepare() raises.

Out of scope, left with the caller: the split == 'test' branch, pcl_color, original_point_cloud, images, language, answers."""
import numpy as np
import torch

MAX_INSTANCE_ID = 2047     # = _ext.SCENE_MAX_IDS - 1: the per-workgroup LDS table of scene_sample_kernel holds ids 0 .. 2047
XF = 41                    # = _ext.SCENE_XF: flip_x, flip_y, Rx (9), Ry (9), Rz (9), t (3), Rz Ry Rx (9)
_STEPS = np.arange(-0.5, 0.501, 0.001)   # the translation factors of ScannetQADataset._translate


def _rotx(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def _roty(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)


def _rotz(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def draw_params(rng, P, N, augment=True):
    """one sample's random draws, the numpy calls of the reference in its order (utils/pc_utils.py:25-33, lib/dataset.py:448-491,
    807-809): a RandomState seeded like the reference's global one reproduces the reference's sample.  rng: np.random.RandomState
    (or the np.random module)."""
    params = {"choices": rng.choice(P, N, replace=P < N)}
    if not augment:
        return params
    params["flip_x"] = -1 if rng.random_sample() > 0.5 else 1
    params["flip_y"] = -1 if rng.random_sample() > 0.5 else 1
    params["angles"] = [(rng.random_sample() * np.pi / 18) - np.pi / 36 for _ in range(3)]
    params["translation"] = [rng.choice(_STEPS, size=1)[0] for _ in range(3)]
    return params


def pack_transform(params):
    """the XF doubles of one sample's augmentation as the kernels read them; the matrices hold numpy's cos / sin"""
    rx, ry, rz = (make(a) for make, a in zip((_rotx, _roty, _rotz), params["angles"]))
    xf = np.empty(XF, dtype=np.float64)
    xf[0], xf[1] = params["flip_x"], params["flip_y"]
    xf[2:11], xf[11:20], xf[20:29] = rx.ravel(), ry.ravel(), rz.ravel()
    xf[29:32] = np.asarray(params["translation"], dtype=np.float64)
    xf[32:41] = np.dot(rz, np.dot(ry, rx)).ravel()
    return xf


def out_spec(B, N, D, G, augment=True):
    """key -> (shape, dtype) of everything a batch holds: the reference's data-dict keys after the default collate"""
    f, i = torch.float32, torch.int64
    spec = {"point_clouds": ((B, N, D), f), "vote_label": ((B, N, 9), f), "vote_label_mask": ((B, N), i),
            "center_label": ((B, G, 3), f), "target_bboxes": ((B, G, 6), f), "size_residual_label": ((B, G, 3), f),
            "heading_residual_label": ((B, G), f), "box_label_mask": ((B, G), f), "heading_class_label": ((B, G), i),
            "size_class_label": ((B, G), i), "sem_cls_label": ((B, G), i), "ref_box_label": ((B, G), i), "num_bbox": ((B,), i),
            "ref_obj_mask": ((B,), i), "ref_center_label": ((B, 3), f), "ref_size_class_label": ((B,), i),
            "ref_size_residual_label": ((B, 3), f)}
    if augment:
        spec.update({"flip_x": ((B,), i), "flip_y": ((B,), i), "rot_mat": ((B, 3, 3), f), "translation": ((B, 3), f)})
    return spec


class SceneStore(object):
    """The scene records packed once into ragged tensors on `device` (scene s owns rows row_base[s] .. row_base[s + 1]).
    nyu40ids: the semantic ids whose instances vote; nyu40id2class: nyu40 id -> class index; mean_size_arr (num_class, 3):
    the dataset config's, taken as arguments as hotpath.ScanQAHotPath takes mean_size_arr.  max_boxes: the reference's
    MAX_NUM_OBJ.  Raises ValueError for instance ids outside [0, 2047], a box whose nyu40 id has no class, rows that are not
    fp32 (P >= 1, D >= 3), or records whose lengths disagree."""

    def __init__(self, scenes, device, nyu40ids, nyu40id2class, mean_size_arr, max_boxes=128):
        self.device = torch.device(device)
        scenes = list(scenes)
        if not scenes:
            raise ValueError("SceneStore: no scenes")
        G = self.max_boxes = int(max_boxes)
        if G < 1:
            raise ValueError("SceneStore: max_boxes must be positive")
        mean_size = np.ascontiguousarray(np.asarray(mean_size_arr, dtype=np.float64))
        if mean_size.ndim != 2 or mean_size.shape[1] != 3 or mean_size.shape[0] < 1:
            raise ValueError("SceneStore: mean_size_arr must be (num_class, 3)")
        NC = mean_size.shape[0]
        self.nyu40ids = np.asarray(nyu40ids).astype(np.int64).ravel()
        if self.nyu40ids.size and self.nyu40ids.min() < 0:
            raise ValueError("SceneStore: negative nyu40 id")
        self.nyu40id2class = dict(nyu40id2class)
        S = len(scenes)
        self.P, self.D, max_id, max_sem = [], None, 0, int(self.nyu40ids.max()) if self.nyu40ids.size else 0
        for s, sc in enumerate(scenes):
            rows = sc["rows"]
            rows = rows.numpy() if torch.is_tensor(rows) else np.asarray(rows)
            if rows.dtype != np.float32 or rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 3:
                raise ValueError("SceneStore: scene %d: rows must be a (P >= 1, D >= 3) float32 array, got %s %s"
                                 % (s, rows.dtype, rows.shape))
            if self.D is None:
                self.D = rows.shape[1]
            if rows.shape[1] != self.D:
                raise ValueError("SceneStore: scene %d has %d columns, scene 0 has %d" % (s, rows.shape[1], self.D))
            P = rows.shape[0]
            inst, sem = np.asarray(sc["instance_labels"]), np.asarray(sc["semantic_labels"])
            if inst.shape != (P,) or sem.shape != (P,):
                raise ValueError("SceneStore: scene %d: labels must be (%d,), got %s and %s" % (s, P, inst.shape, sem.shape))
            if inst.min() < 0 or inst.max() > MAX_INSTANCE_ID:
                raise ValueError("SceneStore: scene %d: instance ids span [%d, %d]; [0, %d] is supported"
                                 % (s, inst.min(), inst.max(), MAX_INSTANCE_ID))
            boxes = np.asarray(sc["instance_bboxes"], dtype=np.float64)
            if boxes.ndim != 2 or boxes.shape[1] != 8:
                raise ValueError("SceneStore: scene %d: instance_bboxes must be (K, 8), got %s" % (s, boxes.shape))
            max_id = max(max_id, int(inst.max()))
            max_sem = max(max_sem, int(sem.max()))
            self.P.append(P)
        self.max_instance_id = max_id
        row_base = np.zeros(S + 1, dtype=np.int64)
        row_base[1:] = np.cumsum(self.P)
        total = int(row_base[-1])
        dev = self.device
        self.rows = torch.empty(total, self.D, dtype=torch.float32, device=dev)
        self.inst = torch.empty(total, dtype=torch.int32, device=dev)
        self.sem = torch.empty(total, dtype=torch.int32, device=dev)
        boxes_all = np.zeros((S, G, 8), dtype=np.float64)
        num_bbox = np.zeros(S, dtype=np.int32)
        box_class = np.zeros((S, G), dtype=np.int32)
        for s, sc in enumerate(scenes):
            lo, hi = int(row_base[s]), int(row_base[s + 1])
            rows = sc["rows"]
            self.rows[lo:hi].copy_(rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows)))
            self.inst[lo:hi].copy_(torch.from_numpy(np.asarray(sc["instance_labels"]).astype(np.int32)))
            self.sem[lo:hi].copy_(torch.from_numpy(np.asarray(sc["semantic_labels"]).astype(np.int32)))
            boxes = np.asarray(sc["instance_bboxes"], dtype=np.float64)
            nb = min(boxes.shape[0], G)
            boxes_all[s, :nb] = boxes[:nb]
            num_bbox[s] = nb
            for i in range(nb):
                cls = self.nyu40id2class.get(int(boxes[i, 6]))
                if cls is None or not 0 <= int(cls) < NC:
                    raise ValueError("SceneStore: scene %d, box %d: nyu40 id %d has no class in [0, %d)"
                                     % (s, i, int(boxes[i, 6]), NC))
                box_class[s, i] = int(cls)
        votes_sem = np.zeros(max(max_sem, 0) + 1, dtype=np.uint8)
        votes_sem[self.nyu40ids] = 1
        up = lambda a: torch.from_numpy(a).to(dev)
        self.row_base, self.boxes, self.num_bbox, self.box_class = up(row_base), up(boxes_all), up(num_bbox), up(box_class)
        self.mean_size, self.votes_sem = up(mean_size), up(votes_sem)
        self._row_base_host = row_base

    def __len__(self):
        return len(self.P)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.rows, self.inst, self.sem, self.row_base, self.boxes,
                                                          self.num_bbox, self.box_class, self.mean_size, self.votes_sem))


def _dot_rt(v, R):
    """v (n, 3) . R^T in fp64 as (x R^T[0][j] + y R^T[1][j]) + z R^T[2][j] -- sp_rotate of csrc/scene_prep.hip"""
    return (v[:, 0:1] * R[None, :, 0] + v[:, 1:2] * R[None, :, 1]) + v[:, 2:3] * R[None, :, 2]


def _rotate_boxes_along_axis(center, extent, R, axis):
    """rotate_aligned_boxes_along_axis on fp64 (G, 3) centres and extents: the ONE host statement of it (the device's is
    sp_rotate_box).  The reference imports the helper from a file its tree does not hold; axis 2 is VoteNet's
    rotate_aligned_boxes, axes 0 and 1 the same construction about x and y."""
    p, q = (1, 2) if axis == 0 else ((0, 2) if axis == 1 else (0, 1))
    half_p, half_q = extent[:, p] / 2.0, extent[:, q] / 2.0
    best_p = best_q = None
    for sp, sq in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
        corner = np.zeros_like(center)
        corner[:, p], corner[:, q] = sp * half_p, sq * half_q
        turned = _dot_rt(corner, R)
        best_p = turned[:, p] if best_p is None else np.maximum(best_p, turned[:, p])
        best_q = turned[:, q] if best_q is None else np.maximum(best_q, turned[:, q])
    out = extent.copy()
    out[:, p], out[:, q] = 2.0 * best_p, 2.0 * best_q
    return _dot_rt(center, R), out


class SceneBatcher(object):
    """prepare() turns scene indices into the detector's inputs and labels for a batch, keyed and typed as the reference's
    collated data dict: point_clouds (B, N, D) f32, vote_label (B, N, 9) f32, vote_label_mask (B, N) i64, center_label,
    target_bboxes, size_residual_label, heading_residual_label, box_label_mask f32, heading_class_label, size_class_label,
    sem_cls_label, ref_box_label, num_bbox, ref_obj_mask, ref_size_class_label i64, ref_center_label, ref_size_residual_label
    f32 and, with augment, flip_x / flip_y i64, rot_mat (B, 3, 3) = Rz Ry Rx and translation (B, 3) f32.  augment=False is a pure
    gather: flips 1, no rotation, no translation, and the four augmentation keys are absent (lib/dataset.py:598).

    On a CUDA store a batch is three launches (_ext.SCENE_CALLS); the host waits for nothing, and with a complete `out` no
    tensor is allocated after the first batch of a given size."""

    def __init__(self, store, num_points, augment=True):
        self.store, self.num_points, self.augment = store, int(num_points), bool(augment)
        if self.num_points < 1:
            raise ValueError("SceneBatcher: num_points must be positive")
        self.last_params = None     # the parameters of the latest prepare(): a list of draw_params-style dicts
        self._work = {}             # B -> (choices, table) device buffers
        self._host_rng, self._host_seed = None, None

    def spec(self, B):
        """key -> (shape, dtype) of a batch of B samples"""
        return out_spec(B, self.num_points, self.store.D, self.store.max_boxes, self.augment)

    def empty(self, B):
        """a fresh dict of output tensors for B samples (what prepare() allocates without `out`)"""
        return {k: torch.empty(shape, dtype=dtype, device=self.store.device) for k, (shape, dtype) in self.spec(B).items()}

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def _host_draws(self, generator):
        """the host-side RandomState behind flips, angles and translations of params=None: seeded from the generator's (or
        torch's) initial seed the first time that seed is seen, then advancing"""
        seed = (generator.initial_seed() if generator is not None else torch.initial_seed()) % (2 ** 32)
        if self._host_rng is None or seed != self._host_seed:
            self._host_rng, self._host_seed = np.random.RandomState(seed), seed
        return self._host_rng

    def _draw(self, scene_index, generator):
        """params=None: per sample, choices = the first N of a random permutation of [0, P) (randint when P < N) from torch on
        the store's device; flips, angles and translation steps with the reference's distributions from the host (twelve numbers
        per sample).  Returns (choices (B, N) int64 on the device, list of parameter dicts without 'choices')."""
        dev, N = self.store.device, self.num_points
        rng = self._host_draws(generator)
        rows, params = [], []
        for s in scene_index:
            P = self.store.P[s]
            if P >= N:
                rows.append(torch.randperm(P, generator=generator, device=dev)[:N])
            else:
                rows.append(torch.randint(0, P, (N,), generator=generator, device=dev))
            p = {}
            if self.augment:
                p["flip_x"] = -1 if rng.random_sample() > 0.5 else 1
                p["flip_y"] = -1 if rng.random_sample() > 0.5 else 1
                p["angles"] = [(rng.random_sample() * np.pi / 18) - np.pi / 36 for _ in range(3)]
                p["translation"] = [_STEPS[rng.randint(0, _STEPS.shape[0])] for _ in range(3)]
            params.append(p)
        return torch.stack(rows), params

    # ---- the batch ----------------------------------------------------------------------------------------------------------
    def prepare(self, scene_index, object_ids=None, params=None, generator=None, out=None, check=False):
        """scene_index: B indices into the store; object_ids: B reference-object ids, -1 (or None) for none; params: B dicts as
        draw_params makes them, or None to draw here (`generator`: a torch.Generator on the store's device); out: a dict
        holding preallocated tensors under this batcher's keys (other keys are left alone; a missing key is allocated and
        added) -- written in place and returned; a shape, dtype, device or layout mismatch raises ValueError.  check=True also
        verifies on the device that every choice lies inside its scene (one host wait); otherwise the kernels clamp."""
        store, N = self.store, self.num_points
        scene_index = [int(s) for s in scene_index]
        B = len(scene_index)
        if B < 1:
            raise ValueError("SceneBatcher.prepare: an empty batch")
        for s in scene_index:
            if not 0 <= s < len(store):
                raise ValueError("SceneBatcher.prepare: scene index %d outside [0, %d)" % (s, len(store)))
        object_ids = [-1 if o is None else int(o) for o in (object_ids if object_ids is not None else [-1] * B)]
        if len(object_ids) != B:
            raise ValueError("SceneBatcher.prepare: %d object ids for %d scenes" % (len(object_ids), B))
        spec = self.spec(B)
        out = {} if out is None else out
        for k, (shape, dtype) in spec.items():
            if k not in out:
                continue
            t = out[k]
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
                raise ValueError("SceneBatcher.prepare: out[%r] must be %s %s, got %s" % (
                    k, dtype, tuple(shape), "%s %s" % (t.dtype, tuple(t.shape)) if torch.is_tensor(t) else type(t).__name__))
            if t.device != store.device or not t.is_contiguous():
                raise ValueError("SceneBatcher.prepare: out[%r] must be a contiguous tensor on %s" % (k, store.device))
        if params is None:
            choices, params = self._draw(scene_index, generator)
        else:
            params = list(params)
            if len(params) != B:
                raise ValueError("SceneBatcher.prepare: %d parameter sets for %d scenes" % (len(params), B))
            ch = np.stack([np.asarray(p["choices"]).astype(np.int64) for p in params])
            if ch.shape != (B, N):
                raise ValueError("SceneBatcher.prepare: choices must be (%d,) per sample, got %s" % (N, ch.shape[1:]))
            for s, row in zip(scene_index, ch):
                if row.min() < 0 or row.max() >= store.P[s]:
                    raise ValueError("SceneBatcher.prepare: choices outside [0, %d) for scene %d" % (store.P[s], s))
            choices = torch.from_numpy(ch)
            params = [{k: v for k, v in p.items() if k != "choices"} for p in params]
        xf = np.stack([pack_transform(p) for p in params]) if self.augment else None
        for k, (shape, dtype) in spec.items():
            if k not in out:
                out[k] = torch.empty(shape, dtype=dtype, device=store.device)
        if store.device.type == "cuda":
            self._prepare_device(scene_index, object_ids, choices, xf, out, check)
            reported = choices
        else:
            reported = choices = choices.cpu()
            self._prepare_host(scene_index, object_ids, choices.numpy(), xf, out)
        self.last_params = [dict(p, choices=reported[b]) for b, p in enumerate(params)]
        return out

    def _prepare_device(self, scene_index, object_ids, choices, xf, out, check):
        from . import _ext
        store, dev, B, N = self.store, self.store.device, len(scene_index), self.num_points
        if B not in self._work:
            self._work[B] = (torch.empty(B, N, dtype=torch.int32, device=dev),
                             torch.empty(B, store.max_instance_id + 1, _ext.SCENE_ENTRY, dtype=torch.int32, device=dev),
                             torch.empty(2, B, dtype=torch.int32, device=dev),
                             torch.empty(B, XF, dtype=torch.float64, device=dev))
        ch32, table, ids, xf_dev = self._work[B]
        with torch.cuda.device(dev):
            ch32.copy_(choices if choices.is_cuda else choices.pin_memory(), non_blocking=True)
            ids.copy_(torch.tensor([scene_index, object_ids], dtype=torch.int32).pin_memory(), non_blocking=True)
            if self.augment:
                xf_dev.copy_(torch.from_numpy(xf).pin_memory(), non_blocking=True)
            _ext.scene_prep(store, ids[0], ids[1], ch32, xf_dev if self.augment else None, out, table, augment=self.augment,
                            check=check)

    def _prepare_host(self, scene_index, object_ids, choices, xf, out):
        """the definition in numpy, one sample at a time, written into `out`"""
        st, N, G = self.store, self.num_points, self.store.max_boxes
        rows_all, inst_all, sem_all = st.rows.numpy(), st.inst.numpy(), st.sem.numpy()
        boxes_all, mean_size = st.boxes.numpy(), st.mean_size.numpy()
        o = {k: out[k].numpy() for k in self.spec(len(scene_index))}
        for b, (s, oid) in enumerate(zip(scene_index, object_ids)):
            lo = int(st._row_base_host[s])
            ch = choices[b] + lo
            pc = rows_all[ch]                                 # (N, D) fp32 copy
            xyz = pc[:, 0:3].copy()
            nb = int(st.num_bbox[s])
            center = np.full((G, 3), -100.0)
            extent = np.full((G, 3), -100.0)
            center[:nb], extent[:nb] = boxes_all[s, :nb, 0:3], boxes_all[s, :nb, 3:6]
            if self.augment:
                x = xf[b]
                if x[0] < 0:
                    xyz[:, 0], center[:, 0] = -xyz[:, 0], -center[:, 0]
                if x[1] < 0:
                    xyz[:, 1], center[:, 1] = -xyz[:, 1], -center[:, 1]
                for axis in range(3):
                    R = x[2 + 9 * axis:11 + 9 * axis].reshape(3, 3)
                    xyz = _dot_rt(xyz.astype(np.float64), R).astype(np.float32)
                    center, extent = _rotate_boxes_along_axis(center, extent, R, axis)
                xyz = (xyz.astype(np.float64) + x[None, 29:32]).astype(np.float32)
                center = center + x[None, 29:32]
                o["flip_x"][b], o["flip_y"][b] = (-1 if x[0] < 0 else 1), (-1 if x[1] < 0 else 1)
                o["rot_mat"][b] = x[32:41].reshape(3, 3).astype(np.float32)
                o["translation"][b] = x[29:32].astype(np.float32)
            pc[:, 0:3] = xyz
            o["point_clouds"][b] = pc
            # votes: per-instance min / max / first sample position by scatter, fp32
            inst = inst_all[ch]
            T = st.max_instance_id + 1
            first = np.full(T, N, dtype=np.int64)
            np.minimum.at(first, inst, np.arange(N))
            mn = np.full((T, 3), np.inf, dtype=np.float32)
            mx = np.full((T, 3), -np.inf, dtype=np.float32)
            np.minimum.at(mn, inst, xyz)
            np.maximum.at(mx, inst, xyz)
            seen = first < N
            decides = np.zeros(T, dtype=bool)
            decides[seen] = np.isin(sem_all[ch[first[seen]]], st.nyu40ids)
            mid = np.zeros((T, 3), dtype=np.float32)
            mid[seen] = np.float32(0.5) * (mn[seen] + mx[seen])
            mask = decides[inst]
            vote = np.where(mask[:, None], mid[inst] - xyz, np.float32(0)).astype(np.float32)
            o["vote_label"][b] = np.tile(vote, (1, 3))
            o["vote_label_mask"][b] = mask
            # boxes
            cls = st.box_class[s].numpy().astype(np.int64)
            valid = np.arange(G) < nb
            o["target_bboxes"][b] = np.concatenate([center, extent], 1).astype(np.float32)
            o["center_label"][b] = center.astype(np.float32)
            resid = np.where(valid[:, None], extent - mean_size[cls], 0.0)
            o["size_residual_label"][b] = resid.astype(np.float32)
            o["heading_residual_label"][b], o["heading_class_label"][b] = 0, 0
            o["box_label_mask"][b] = valid
            o["size_class_label"][b], o["sem_cls_label"][b] = cls, cls
            match = valid & (boxes_all[s, :, 7] == oid) & (oid >= 0)
            o["ref_box_label"][b] = match
            o["num_bbox"][b], o["ref_obj_mask"][b] = nb, int(oid >= 0)
            if match.any():
                last = int(np.nonzero(match)[0][-1])
                o["ref_center_label"][b] = center[last].astype(np.float32)
                o["ref_size_class_label"][b] = cls[last]
                o["ref_size_residual_label"][b] = resid[last].astype(np.float32)
            else:
                o["ref_center_label"][b], o["ref_size_class_label"][b], o["ref_size_residual_label"][b] = 0, 0, 0
