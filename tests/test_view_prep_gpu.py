"""csrc/view_prep.hip behind bridgeqa_amd.view_data on the device, against the numpy definition of tests/viewprep_ref.py on the
inputs recorded in tests/golden/viewprep/ (which that definition reproduces byte for byte from Pillow: the CPU test).  Every
comparison is bitwise against table[reference bytes]."""
import numpy as np
import pytest
import torch

import viewprep_ref as R
from test_view_prep_cpu import bits, expected, golden_cases

pytestmark = pytest.mark.gpu

_REF = {}


def ref(i, OH, OW):
    """table[ref bytes] of golden input i at (OH, OW), fp32 NCHW, computed once"""
    if (i, OH, OW) not in _REF:
        _REF[(i, OH, OW)] = R.preprocess(golden_cases()[i][2], OH, OW)
    return _REF[(i, OH, OW)]


@pytest.fixture(scope="module")
def store(dev):
    from bridgeqa_amd.view_data import ViewStore
    return ViewStore([a for _, _, a, _ in golden_cases()], dev)


@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: "%dx%d-%dx%d" % s[1:])
def test_every_size_and_content_equals_the_definition(dev, store, size):
    """growing with windows clamped at both borders, odd extents, shrinking with 13 and 11 taps, each pass skipped, windows
    shorter than ksize -- on random bytes, the 0 / 255 checkerboard and the ramp, fp32 NCHW and bf16 patches"""
    from bridgeqa_amd import _ext
    from bridgeqa_amd.view_data import ViewBatcher
    name, H, W, OH, OW = size
    pick = [i for i, c in enumerate(golden_cases()) if c[0] == name]
    assert [golden_cases()[i][1] for i in pick] == list(R.CONTENTS) and store.shapes[pick[0]] == (H, W)
    before = _ext.VIEW_CALLS[0]
    got = ViewBatcher(store, (OH, OW)).prepare(pick)["images"]
    assert _ext.VIEW_CALLS[0] == before + 1 and got.is_cuda and got.shape == (3, 1, 3, OH, OW)
    want = torch.stack([ref(i, OH, OW) for i in pick])
    assert torch.equal(bits(got[:, 0].cpu()), bits(want)), int((bits(got[:, 0].cpu()) != bits(want)).sum())
    # the recorded Pillow bytes themselves, through the table
    table = R.norm_table()
    for j, i in enumerate(pick):
        o = torch.from_numpy(np.array(golden_cases()[i][3])).permute(2, 0, 1).long()
        assert torch.equal(bits(got[j, 0].cpu()), bits(torch.gather(table, 1, o.reshape(3, -1)).reshape(3, OH, OW)))
    p = 8
    got = ViewBatcher(store, (OH, OW), dtype=torch.bfloat16, layout="patches", patch=p).prepare(pick)["images"]
    assert got.dtype == torch.bfloat16 and got.shape == (3, 1, (OH // p) * (OW // p), 3 * p * p)
    assert torch.equal(bits(got[:, 0].cpu()), bits(R.to_patches(want.to(torch.bfloat16), p)))


@pytest.mark.parametrize("OW", (48, 38), ids=("four_wide", "single"))
def test_row_tiles_and_a_ragged_last_tile(dev, store, OW):
    """output heights that take at least three row tiles with a shorter last one, at the tile height the host picks and at a
    forced small one; OW = 38 takes the one-pixel-per-thread kernels"""
    from bridgeqa_amd.view_data import ViewBatcher
    cases = golden_cases()
    pick = [i for i, c in enumerate(cases) if c[0] in ("grow", "shrink")]
    for OH, tile_rows in ((75, None), (52, 8)):
        b = ViewBatcher(store, (OH, OW), tile_rows=tile_rows)
        assert OH > 2 * b.tile_rows and OH % b.tile_rows != 0, (OH, b.tile_rows)
        got = b.prepare(pick)["images"][:, 0].cpu()
        want = torch.stack([ref(i, OH, OW) for i in pick])
        assert torch.equal(bits(got), bits(want)), (OH, OW, int((bits(got) != bits(want)).sum()))


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("layout", ("nchw", "patches"))
def test_a_batch_mixing_sizes_with_repeated_and_unordered_indices(dev, store, dtype, layout):
    from bridgeqa_amd.view_data import ViewBatcher
    idx = [[20, 0], [3, 3], [7, 19], [14, 6]]                    # V = 2: tiny, grow, odd, shrink and copy inputs
    b = ViewBatcher(store, 48, dtype=dtype, layout=layout, patch=16)
    want = torch.stack([ref(i, 48, 48) for row in idx for i in row]).to(dtype)
    want = R.to_patches(want, 16) if layout == "patches" else want
    for index in (idx, torch.tensor(idx, device=dev), torch.tensor(idx, device=dev, dtype=torch.int32)):
        got = b.prepare(index)["images"]
        assert got.shape[:2] == (4, 2) and got.dtype == dtype
        assert torch.equal(bits(got.reshape(want.shape).cpu()), bits(want))
    # an index outside the store is clamped by the kernel: a wrong view, no fault -- (B,) gives V = 1
    got = b.prepare(torch.tensor([-5, 400], device=dev))["images"]
    edge = torch.stack([ref(0, 48, 48), ref(20, 48, 48)]).to(dtype)
    edge = R.to_patches(edge, 16) if layout == "patches" else edge
    assert got.shape[:2] == (2, 1) and torch.equal(bits(got[:, 0].cpu()), bits(edge))


def test_bf16_patches_equal_unfold_and_cast_of_the_fp32_images(dev, store):
    from bridgeqa_amd.view_data import ViewBatcher
    idx = torch.tensor([[1, 4], [9, 16]], device=dev)
    x = ViewBatcher(store, 48).prepare(idx)["images"]                                          # (2, 2, 3, 48, 48) fp32
    got = ViewBatcher(store, 48, dtype=torch.bfloat16, layout="patches", patch=16).prepare(idx)["images"]
    B, V, C, H, W = x.shape
    unfold = x.reshape(B * V, C, 3, 16, 3, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, V, 9, C * 256)   # PatchEmbed.forward's
    assert got.shape == unfold.shape and torch.equal(bits(got), bits(unfold.to(torch.bfloat16)))


def test_vit_forward_from_bf16_patches_equals_the_forward_from_fp32_images(dev, store):
    from bridgeqa_amd import fusion_ops as ops
    from bridgeqa_amd import vit
    from bridgeqa_amd.view_data import ViewBatcher
    torch.manual_seed(0)
    m = vit.VisionTransformer(img_size=64, patch_size=16, embed_dim=256, depth=2, num_heads=4, drop_path_rate=0.1).to(dev).eval()
    idx = torch.tensor([[2, 5], [10, 17]], device=dev)
    images = ViewBatcher(store, 64).prepare(idx)["images"]
    patches = ViewBatcher(store, 64, dtype=torch.bfloat16, layout="patches").prepare(idx)["images"]
    prev = ops.set_compute_dtype(torch.bfloat16)
    try:
        with torch.no_grad():
            a, b = m(images[:, 0]), m(patches[:, 0])           # hotpath.py's data_dict["images"][:, 0], either layout
    finally:
        ops.set_compute_dtype(prev)
    assert a.dtype == b.dtype == torch.bfloat16 and a.shape == (2, 17, 256)     # the kernel path ran
    assert bool(torch.isfinite(a.float()).all()) and torch.equal(bits(a), bits(b))


def test_out_is_written_in_place(dev, store):
    from bridgeqa_amd.view_data import ViewBatcher
    b = ViewBatcher(store, 48)
    out = b.empty(2, 2)
    out["images"].fill_(7)
    out["question"] = ["kept"]
    ptr = out["images"].data_ptr()
    got = b.prepare([[0, 12], [12, 1]], out=out)
    assert got is out and out["question"] == ["kept"] and out["images"].data_ptr() == ptr
    want = torch.stack([ref(i, 48, 48) for i in (0, 12, 12, 1)])
    assert torch.equal(bits(out["images"].reshape(4, 3, 48, 48).cpu()), bits(want))
    with pytest.raises(ValueError, match="images"):
        b.prepare([[0, 12], [12, 1]], out={"images": torch.empty(2, 2, 3, 48, 48)})           # a host tensor
    with pytest.raises(ValueError, match="images"):
        b.prepare([[0, 12], [12, 1]], out={"images": torch.empty(2, 2, 3, 48, 40, device=dev)})


def test_a_captured_prepare_replays_with_the_index_tensor_of_the_moment(dev, store):
    from bridgeqa_amd.view_data import ViewBatcher
    b = ViewBatcher(store, 48)
    idx = torch.tensor([[0, 3], [6, 9]], device=dev)
    out = b.empty(2, 2)
    b.prepare(idx, out=out)                                       # warm: nothing is allocated inside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        b.prepare(idx, out=out)
    for new in ([[0, 3], [6, 9]], [[15, 1], [1, 18]]):
        idx.copy_(torch.tensor(new, device=dev))
        out["images"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        want = torch.stack([ref(i, 48, 48) for row in new for i in row])
        assert torch.equal(bits(out["images"].reshape(4, 3, 48, 48).cpu()), bits(want)), new


def test_encode_views_on_raw_frames_equals_encode_views_on_preprocessed_tensors(dev):
    from test_itm_cpu import build
    _, m, blip_itm = build(dev)                                   # image_size 64, as tests/test_itm_gpu.py builds it
    frames = np.stack([R.content(k, 24, 32, seed=i) for i, k in enumerate(R.CONTENTS + ("random",))])
    pre = torch.stack([R.preprocess(f, 64, 64) for f in frames])                               # blip_utils.preprocess
    want = blip_itm.encode_views(m, pre, batch_size=3)
    got = blip_itm.encode_views(m, torch.from_numpy(frames), batch_size=3)
    assert got.shape == want.shape == (4, 256) and torch.equal(bits(got), bits(want))


def test_wrapper_rejections(dev, store):
    from bridgeqa_amd import _ext
    from bridgeqa_amd.view_data import ViewBatcher
    b = ViewBatcher(store, 48)
    plan, idx = b.plan, torch.tensor([0, 1], device=dev)
    out = torch.empty(2, 3, 48, 48, device=dev)
    args = lambda **kw: dict(dict(pixels=store.pixels, views=plan.views, tab=plan.tab, desc=plan.desc, index=idx,
                                  norm=b.format.table, out=out, OH=48, OW=48, tile_rows=b.tile_rows, lds_rows=b.lds_rows), **kw)
    before = _ext.VIEW_CALLS[0]
    with pytest.raises(RuntimeError, match="CPU not supported"):
        _ext.view_prep(**args(pixels=store.pixels.cpu()))
    with pytest.raises(RuntimeError, match="index must be a int64"):
        _ext.view_prep(**args(index=idx.int()))
    with pytest.raises(RuntimeError, match="out must be a float32 tensor of shape"):
        _ext.view_prep(**args(out=out.bfloat16()))
    with pytest.raises(RuntimeError, match="patch = 5"):
        _ext.view_prep(**args(patch=5))
    assert _ext.VIEW_CALLS[0] == before                           # every rejection came before the launch
    with pytest.raises(RuntimeError, match="LDS"):
        _ext.view_prep(**args(lds_rows=4000))                     # the library's own check: a status and a text, no launch
