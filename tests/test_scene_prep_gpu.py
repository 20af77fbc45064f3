"""csrc/scene_prep.hip behind bridgeqa_amd.scene_data.SceneBatcher on the device, against the numpy definition of
tests/sceneprep_ref.py on the scenes of tests/sceneprep_cases.py (what each scene is built to hold is said there):
point_clouds, every label tensor and the masks BIT equal, vote_label equal under np.array_equal (numeric equality: only the
sign of a zero is free -- the min / max table orders -0 below +0, numpy's min / max take whichever zero comes first)."""
import types

import numpy as np
import pytest
import torch

import sceneprep_cases as C
import sceneprep_ref as R
from test_scene_prep_cpu import _bits, batch_cases, compare, run_case

pytestmark = pytest.mark.gpu


def _store(dev, scenes):
    from bridgeqa_amd.scene_data import SceneStore
    return SceneStore(scenes, dev, max_boxes=C.G, **C.config())


@pytest.mark.parametrize("augment", (True, False))
@pytest.mark.parametrize("case", batch_cases(), ids=lambda c: c[0])
def test_device_batch_equals_the_numpy_definition(dev, case, augment):
    from bridgeqa_amd import _ext
    before = list(_ext.SCENE_CALLS)
    got, want = run_case(case, dev, augment, check=True)
    assert all(v.is_cuda for v in got.values())
    launches = sum(_ext.SCENE_CALLS) - sum(before)
    assert 1 <= launches <= 5, launches
    fails = compare(got, want)
    assert not fails, "\n".join(fails)
    if not augment:
        rows = np.stack([case[1][s]["rows"][p["choices"]] for s, p in zip(case[4], case[6])])
        assert np.array_equal(_bits(got["point_clouds"].cpu().numpy()), _bits(rows))             # the bitwise gather


def test_two_runs_are_bitwise_equal_and_out_is_written_in_place(dev):
    from bridgeqa_amd.scene_data import SceneBatcher
    _, scenes, G, N, index, oids, params = batch_cases()[0]
    b = SceneBatcher(_store(dev, scenes), N)
    first = {k: v.clone() for k, v in b.prepare(index, oids, params=params).items()}
    out = b.empty(2)
    for v in out.values():
        v.fill_(7)                                       # whatever a previous batch left behind
    out["question"] = ["kept"]
    ptrs = {k: v.data_ptr() for k, v in out.items() if torch.is_tensor(v)}
    got = b.prepare(index, oids, params=params, out=out)
    assert got is out and out["question"] == ["kept"]
    assert {k: v.data_ptr() for k, v in out.items() if torch.is_tensor(v)} == ptrs
    for k, v in first.items():
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v,
                           out[k].view(torch.int32) if v.dtype == torch.float32 else out[k]), k
    with pytest.raises(ValueError, match="vote_label"):
        b.prepare(index, oids, params=params, out=dict(out, vote_label=torch.empty(2, N, 3, device=dev)))
    with pytest.raises(ValueError, match="point_clouds"):
        b.prepare(index, oids, params=params, out=dict(out, point_clouds=torch.empty(2, N, 7)))


@pytest.mark.parametrize("augment", (True, False))
def test_device_draws(dev, augment):
    """params=None: shapes and dtypes, a permutation prefix where P >= N, the reference's ranges, at most five launches, and the
    definition reproduces the batch from the parameters the batcher reports"""
    from bridgeqa_amd import _ext
    from bridgeqa_amd.scene_data import SceneBatcher
    scenes = C.cases()["scenes_ab"]
    N = 4096
    b = SceneBatcher(_store(dev, scenes), N, augment=augment)
    g = torch.Generator(device=dev).manual_seed(5)
    index, oids = [0, 1, 0, 0], [4, -1, 13, -1]
    before = sum(_ext.SCENE_CALLS)
    out = b.prepare(index, oids, generator=g)
    assert 1 <= sum(_ext.SCENE_CALLS) - before <= 5
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items()} == b.spec(4)
    params = [dict(p, choices=p["choices"].cpu().numpy()) for p in b.last_params]
    steps = np.arange(-0.5, 0.501, 0.001)
    for s, p in zip(index, params):
        ch = p["choices"]
        assert ch.shape == (N,) and ch.min() >= 0 and ch.max() < scenes[s]["rows"].shape[0]
        if scenes[s]["rows"].shape[0] >= N:
            assert len(np.unique(ch)) == N
        if augment:
            assert p["flip_x"] in (1, -1) and p["flip_y"] in (1, -1)
            assert all(-np.pi / 36 <= a < np.pi / 36 for a in p["angles"]) and all(t in steps for t in p["translation"])
    assert not np.array_equal(params[0]["choices"], params[2]["choices"])                        # a draw per sample
    want = R.prepare_batch(scenes, index, params, max_boxes=C.G, augment=augment, object_ids=oids, **C.config())
    fails = compare(out, want)
    assert not fails, "\n".join(fails)


def test_detector_and_fused_loss_consume_the_batch(dev):
    """scene C at N = 1024 through ScanQAHotPath(use_blip=False).detect and the fused detection loss: finite, and equal to the
    loss from the same tensors built by the numpy definition on the host and uploaded"""
    from bridgeqa_amd import loss_helper as lh
    from bridgeqa_amd.hotpath import ScanQAHotPath
    from bridgeqa_amd.scene_data import SceneBatcher
    _, scenes, G, N, index, oids, params = batch_cases()[2]
    index, oids, params = index * 2, oids * 2, params * 2
    cfg = types.SimpleNamespace(num_heading_bin=1, num_size_cluster=18, num_class=18, mean_size_arr=C.MEAN_SIZE_ARR)
    torch.manual_seed(0)
    # (eval mode: the forward keeps no state between the two passes, so equal inputs must give an equal loss)
    model = ScanQAHotPath(input_feature_dim=132, use_blip=False, mean_size_arr=C.MEAN_SIZE_ARR).to(dev).eval()
    batch = SceneBatcher(_store(dev, scenes), N).prepare(index, oids, params=params)
    host = R.prepare_batch(scenes, index, params, max_boxes=G, object_ids=oids, **C.config())
    losses = []
    for data in (batch, {k: torch.from_numpy(v).to(dev) for k, v in host.items()}):
        dd = model.detect(dict(data))
        assert lh._fused_ok(dd) is not None, "the fused detection loss declined the batch"
        loss, dd = lh.get_detection_loss(dd, cfg)
        losses.append(loss.detach().clone())
    assert bool(torch.isfinite(losses[0])) and losses[0].item() > 0
    assert torch.equal(losses[0], losses[1]), (losses[0].item(), losses[1].item())


def test_wrapper_rejections(dev):
    from bridgeqa_amd import _ext
    from bridgeqa_amd.scene_data import XF, SceneBatcher
    _, scenes, G, N, index, oids, params = batch_cases()[0]
    store = _store(dev, scenes)
    b = SceneBatcher(store, N)
    out = b.empty(2)
    T = store.max_instance_id + 1
    scene = torch.tensor(index, dtype=torch.int32, device=dev)
    oid = torch.tensor(oids, dtype=torch.int32, device=dev)
    ch = torch.from_numpy(np.stack([p["choices"] for p in params])).to(dev).int()
    xf = torch.zeros(2, XF, dtype=torch.float64, device=dev)
    table = torch.empty(2, T, _ext.SCENE_ENTRY, dtype=torch.int32, device=dev)
    before = list(_ext.SCENE_CALLS)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.scene_prep(store, scene, oid, ch.cpu(), xf, out, table)
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.scene_prep(store, scene, oid, ch, xf, dict(out, vote_label=out["vote_label"].cpu()), table)
    with pytest.raises(RuntimeError, match="choices must be a int32"):
        _ext.scene_prep(store, scene, oid, ch.long(), xf, out, table)
    with pytest.raises(RuntimeError, match="xf must be a float64"):
        _ext.scene_prep(store, scene, oid, ch, xf.float(), out, table)
    with pytest.raises(RuntimeError, match="contiguous"):
        _ext.scene_prep(store, scene, oid, ch.t().contiguous().t(), xf, out, table)
    bad = ch.clone()
    bad[1, 17] = 97                                                   # scene B holds points 0 .. 96
    with pytest.raises(RuntimeError, match="1 choices outside"):
        _ext.scene_prep(store, scene, oid, bad, xf, out, table, check=True)
    assert _ext.SCENE_CALLS == before                                 # every rejection came before the first launch
    # the library's own extent checks: a status and a text, no exit
    st = _ext._lib.bq_scene_sample(store.rows.data_ptr(), store.inst.data_ptr(), store.row_base.data_ptr(), scene.data_ptr(),
                                   ch.data_ptr(), xf.data_ptr(), out["point_clouds"].data_ptr(), table.data_ptr(), 2, 2, N, 2, T,
                                   1, None)
    assert st == _ext._D["BQ_EINVAL"] and b"D = 2" in _ext._lib.bq_last_error()
    st = _ext._lib.bq_scene_votes(store.inst.data_ptr(), store.sem.data_ptr(), store.votes_sem.data_ptr(),
                                  store.row_base.data_ptr(), scene.data_ptr(), ch.data_ptr(), out["point_clouds"].data_ptr(),
                                  table.data_ptr(), out["vote_label"].data_ptr(), out["vote_label_mask"].data_ptr(), 2, 2, N, 7,
                                  4096, 41, None)
    assert st == _ext._D["BQ_EINVAL"] and b"4096" in _ext._lib.bq_last_error()
