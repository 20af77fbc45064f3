"""bridgeqa_amd/scene_data.py on a CPU device against the numpy definition of tests/sceneprep_ref.py (points, labels and masks
bit for bit, votes numerically equal: only the sign of a zero is free), the explicit order of the rotation against np.dot,
draw_params against the reference's numpy calls written out, the key set and dtypes, the rejections, and the C header."""
import os
import subprocess

import numpy as np
import pytest
import torch

import sceneprep_cases as C
import sceneprep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = ("point_clouds", "vote_label", "center_label", "target_bboxes", "size_residual_label", "heading_residual_label",
       "box_label_mask", "ref_center_label", "ref_size_residual_label")
I64 = ("vote_label_mask", "heading_class_label", "size_class_label", "sem_cls_label", "ref_box_label", "num_bbox", "ref_obj_mask",
       "ref_size_class_label")
AUG = {"flip_x": torch.int64, "flip_y": torch.int64, "rot_mat": torch.float32, "translation": torch.float32}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def compare(got, want):
    """-> list of failures: every key of `want` present with its dtype and shape; vote_label np.array_equal, the rest bitwise"""
    fails = []
    if set(got) != set(want):
        fails.append("keys differ: %s" % sorted(set(got) ^ set(want)))
    for k, w in want.items():
        if k not in got:
            continue
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        if g.dtype != w.dtype or g.shape != w.shape:
            fails.append("%s: %s %s, expected %s %s" % (k, g.dtype, g.shape, w.dtype, w.shape))
        elif not np.isfinite(g.astype(np.float64)).all():
            fails.append("%s: not finite" % k)
        elif k == "vote_label":
            if not np.array_equal(g, w):
                fails.append("vote_label: %d elements differ" % int((g != w).sum()))
        elif not np.array_equal(_bits(g), _bits(w)):
            fails.append("%s: %d elements differ in their bits" % (k, int((_bits(g) != _bits(w)).sum())))
    return fails


def batch_cases():
    """(name, scenes, G, N, scene_index, object_ids, params) -- shared with the GPU test"""
    c = C.cases()
    return [("AB", c["scenes_ab"], C.G, C.N_AB, [0, 1], c["object_ids_ab"], c["params_ab"]),
            ("BA_noref", c["scenes_ab"], C.G, C.N_AB, [1, 0], None, c["params_ab"][::-1]),
            ("C", c["scenes_c"], C.G, C.N_C, [0], c["object_ids_c"], c["params_c"])]


def run_case(case, device, augment, **kw):
    from bridgeqa_amd.scene_data import SceneBatcher, SceneStore
    name, scenes, G, N, index, oids, params = case
    store = SceneStore(scenes, device, max_boxes=G, **C.config())
    got = SceneBatcher(store, N, augment=augment).prepare(index, oids, params=params, **kw)
    want = R.prepare_batch(scenes, index, params, max_boxes=G, augment=augment, object_ids=oids, **C.config())
    return got, want


def test_the_cases_hold_what_they_promise():
    c = C.cases()
    for sc, p in zip(c["scenes_ab"] + c["scenes_c"], c["params_ab"] + c["params_c"]):
        C.check_layout(sc, p["choices"])
    a, pa = c["scenes_ab"][0], c["params_ab"][0]
    assert (a["instance_labels"][pa["choices"]] == 13).sum() == 1 and len(set(pa["choices"])) == C.N_AB
    assert len(set(c["params_ab"][1]["choices"])) < C.N_AB                       # P < N: repeats
    assert a["instance_bboxes"].shape[0] == 11 > C.G > c["scenes_ab"][1]["instance_bboxes"].shape[0] == 5


@pytest.mark.parametrize("augment", (True, False))
@pytest.mark.parametrize("case", batch_cases(), ids=lambda c: c[0])
def test_cpu_path_equals_the_numpy_definition(case, augment):
    got, want = run_case(case, "cpu", augment)
    assert not compare(got, want), "\n".join(compare(got, want))
    # the definition itself shows the properties the cases were built for
    inst = np.stack([case[1][s]["instance_labels"][p["choices"]] for s, p in zip(case[4], case[6])])
    assert (want["vote_label_mask"][inst == 11] == 1).all() and (want["vote_label_mask"][inst == 12] == 0).all()
    assert (want["vote_label"][inst == 13] == 0).all() and (want["vote_label_mask"][inst == 13] == 1).all()
    pads = np.concatenate([want["target_bboxes"][b, nb:] for b, nb in enumerate(want["num_bbox"])])
    assert pads.size and bool((pads != -100).any()) == augment                              # the padding rows are transformed
    if not augment:
        rows = np.stack([case[1][s]["rows"][p["choices"]] for s, p in zip(case[4], case[6])])
        assert np.array_equal(_bits(got["point_clouds"].numpy()), _bits(rows))               # a pure gather


def test_last_matching_box_gives_the_reference_labels():
    got, want = run_case(batch_cases()[0], "cpu", True)
    assert want["ref_box_label"][0].sum() == 2 and want["ref_obj_mask"].tolist() == [1, 0]   # object id 4 sits on boxes 1 and 3
    assert np.array_equal(want["ref_center_label"][0], want["center_label"][0, 3])
    assert torch.equal(got["ref_center_label"][0], got["center_label"][0, 3]) and not got["ref_center_label"][1].any()


def test_explicit_rotation_order_equals_np_dot_on_the_fp32_array():
    """Bit equal on every point of the cases, through the three chained rotations.  One exception is known and held to numeric
    equality: a point with a NEGATIVE zero coordinate (the cases hold one such row on purpose, for the min / max encoding).
    Where every term of a sum is -0 the written-out order gives -0, while np.dot's matrix product starts its sum from +0 and
    gives +0 -- measured here: 1 element of 33 072, the x of (-0, 0, -0) under rotx."""
    c = C.cases()
    for sc, p in zip(c["scenes_ab"] + c["scenes_c"], c["params_ab"] + c["params_c"]):
        xyz = sc["rows"][p["choices"], 0:3].copy()
        plain = ~np.signbit(np.where(xyz == 0, xyz, np.float32(1))).any(1)      # rows without a negative zero
        assert plain.sum() >= 0.95 * len(plain) and not plain.all()
        for make, angle in zip((R.rotx, R.roty, R.rotz), p["angles"]):
            rot = make(angle)
            want = xyz.copy()
            want[:, 0:3] = np.dot(want[:, 0:3], np.transpose(rot))
            xyz = R.rotate_points(xyz, rot)
            assert np.array_equal(_bits(xyz[plain]), _bits(want[plain])) and np.array_equal(xyz, want)


def test_draw_params_makes_the_reference_calls_in_order():
    from bridgeqa_amd.scene_data import draw_params
    for P, N in ((50, 20), (7, 20)):
        got = draw_params(np.random.RandomState(11), P, N, True)
        rs = np.random.RandomState(11)
        choices = rs.choice(P, N, replace=(P < N))
        flip_x = -1 if rs.random_sample() > 0.5 else 1
        flip_y = -1 if rs.random_sample() > 0.5 else 1
        angles = [(rs.random_sample() * np.pi / 18) - np.pi / 36 for _ in range(3)]
        factor = [rs.choice(np.arange(-0.5, 0.501, 0.001), size=1)[0] for _ in range(3)]
        assert np.array_equal(got["choices"], choices) and (got["flip_x"], got["flip_y"]) == (flip_x, flip_y)
        assert list(got["angles"]) == angles and list(got["translation"]) == factor
        assert rs.random_sample() == draw_params_state_after(11, P, N)               # no further draw was made
    plain = draw_params(np.random.RandomState(11), 50, 20, False)
    assert set(plain) == {"choices"} and np.array_equal(plain["choices"], np.random.RandomState(11).choice(50, 20, replace=False))


def draw_params_state_after(seed, P, N):
    from bridgeqa_amd.scene_data import draw_params
    rs = np.random.RandomState(seed)
    draw_params(rs, P, N, True)
    return rs.random_sample()


def test_keys_and_dtypes():
    from bridgeqa_amd.scene_data import SceneBatcher, SceneStore
    c = C.cases()
    store = SceneStore(c["scenes_ab"], "cpu", max_boxes=C.G, **C.config())
    assert len(store) == 2 and store.D == 7 and store.max_instance_id == 2047
    assert store.nbytes >= (6000 + 97) * (7 * 4 + 8)
    for augment in (True, False):
        b = SceneBatcher(store, 64, augment=augment)
        out = b.prepare([0, 1, 1], generator=torch.Generator().manual_seed(1))
        want = {k: torch.float32 for k in F32}
        want.update({k: torch.int64 for k in I64})
        want.update(AUG if augment else {})
        assert {k: v.dtype for k, v in out.items()} == want
        assert out["point_clouds"].shape == (3, 64, 7) and out["vote_label"].shape == (3, 64, 9)
        assert out["target_bboxes"].shape == (3, C.G, 6) and out["num_bbox"].tolist() == [8, 5, 5]
        if augment:
            assert out["rot_mat"].shape == (3, 3, 3) and out["translation"].shape == (3, 3)
        # the drawn parameters are reported, and the definition reproduces the batch from them
        again = R.prepare_batch(c["scenes_ab"], [0, 1, 1], [dict(p, choices=p["choices"].numpy()) for p in b.last_params],
                                max_boxes=C.G, augment=augment, **C.config())
        assert not compare(out, again), "\n".join(compare(out, again))
        ch = b.last_params[0]["choices"].numpy()
        assert len(set(ch.tolist())) == 64 and ch.min() >= 0 and ch.max() < 6000


def test_out_is_written_in_place_and_mismatches_raise():
    from bridgeqa_amd.scene_data import SceneBatcher, SceneStore
    case = batch_cases()[0]
    store = SceneStore(case[1], "cpu", max_boxes=C.G, **C.config())
    b = SceneBatcher(store, C.N_AB)
    out = b.empty(2)
    out["images"] = "left alone"
    ptrs = {k: v.data_ptr() for k, v in out.items() if torch.is_tensor(v)}
    got = b.prepare(case[4], case[5], params=case[6], out=out)
    assert got is out and out["images"] == "left alone"
    assert {k: v.data_ptr() for k, v in out.items() if torch.is_tensor(v)} == ptrs
    want = R.prepare_batch(case[1], case[4], case[6], max_boxes=C.G, object_ids=case[5], **C.config())
    assert not compare({k: v for k, v in out.items() if k != "images"}, want)
    for key, bad in (("point_clouds", torch.empty(2, C.N_AB, 8)), ("vote_label_mask", torch.empty(2, C.N_AB, dtype=torch.int32)),
                     ("target_bboxes", torch.empty(2, 6, C.G).transpose(1, 2)), ("num_bbox", [8, 5])):
        with pytest.raises(ValueError, match=key):
            b.prepare(case[4], case[5], params=case[6], out=dict(out, **{key: bad}))
    with pytest.raises(ValueError):
        b.prepare([0, 2], params=case[6])
    with pytest.raises(ValueError, match="choices"):
        b.prepare([1, 0], params=case[6])                       # scene A's choices reach past scene B's 97 points


def test_store_rejects_what_the_kernels_do_not_hold():
    from bridgeqa_amd.scene_data import SceneStore
    a = C.cases()["scenes_ab"][0]
    mk = lambda **kw: SceneStore([dict(a, **kw)], "cpu", max_boxes=C.G, **C.config())
    hi, neg = a["instance_labels"].copy(), a["instance_labels"].copy()
    hi[3], neg[3] = 2048, -1
    for kw in (dict(instance_labels=hi), dict(instance_labels=neg), dict(rows=a["rows"].astype(np.float64)),
               dict(semantic_labels=a["semantic_labels"][:-1]),
               dict(instance_bboxes=np.concatenate([a["instance_bboxes"][:1] * [1, 1, 1, 1, 1, 1, 0, 1], a["instance_bboxes"][1:]]))):
        with pytest.raises(ValueError):
            mk(**kw)
    assert mk().max_instance_id == 2047


def test_header_is_c99_and_the_library_exports_the_entry_points(tmp_path):
    from bridgeqa_amd import _cabi, _ext
    names = ("bq_scene_boxes", "bq_scene_sample", "bq_scene_votes")
    assert "bqhip_scene.h" in _cabi.ADDITIVE_HEADERS
    for n in names:
        assert n in _cabi.ADDITIVE_PROTOS and n not in _cabi.PROTOS
        restype, argtypes = _cabi.ADDITIVE_PROTOS[n]
        assert restype is _cabi.ctypes.c_int and argtypes[-1] is _cabi.ctypes.c_void_p
        assert getattr(_ext._lib, n).argtypes == argtypes
    assert _cabi.DEFINES["BQHIP_ABI_VERSION"] == 6 and _ext.SCENE_MAX_IDS == 2048
    from bridgeqa_amd import scene_data                     # (states the two constants again so that its CPU path needs no library)
    assert (scene_data.XF, scene_data.MAX_INSTANCE_ID) == (_ext.SCENE_XF, _ext.SCENE_MAX_IDS - 1)
    assert '#include "bqhip_scene.h"' in open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    src = tmp_path / "t.c"
    src.write_text('#include "bqhip_scene.h"\nint main(void) { return BQ_SCENE_XF == 41 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = subprocess.run(["nm", "-D", "--defined-only", _ext.library_path()], capture_output=True, text=True).stdout
    for n in names:
        assert " T %s\n" % n in syms, n
