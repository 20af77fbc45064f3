"""bridgeqa_amd/view_data.py on a CPU device against the numpy definition of tests/viewprep_ref.py, bit for bit; that definition
against the Pillow outputs recorded in tests/golden/viewprep/ (tools/make_viewprep_golden.py) and against a live Pillow where one
is installed; the normalisation table against the ToTensor / Normalize composition; the rejections; the C header; the kernels'
resources."""
import os
import subprocess

import numpy as np
import pytest
import torch

import viewprep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "viewprep", "pillow.npz")
_CACHE = {}


def golden_cases():
    """[(name, kind, input, Pillow's output)] -- loaded once, shared with the GPU test, never modified"""
    if "cases" not in _CACHE:
        _CACHE["cases"] = R.golden_cases(np.load(GOLD, allow_pickle=False))
        for _, _, a, o in _CACHE["cases"]:
            a.setflags(write=False)
            o.setflags(write=False)
    return _CACHE["cases"]


def bits(t):
    """a float tensor as integers"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def expected(frames_and_sizes, dtype=torch.float32, layout="nchw", patch=16):
    """table[ref bytes] for [(frame, OH, OW)] of one output size, in the asked type and layout"""
    x = torch.stack([R.preprocess(f, OH, OW) for f, OH, OW in frames_and_sizes]).to(dtype)
    return R.to_patches(x, patch) if layout == "patches" else x


def test_reference_equals_the_recorded_pillow_outputs():
    cases = golden_cases()
    assert len(cases) == len(R.SIZES) * len(R.CONTENTS) == 21
    for name, kind, a, want in cases:
        got = R.resize(a, want.shape[0], want.shape[1])
        assert np.array_equal(got, want), (name, kind, int((got != want).sum()))
    # the checkerboards drive the clamp at both ends
    assert any(o.min() == 0 and o.max() == 255 for n, k, _, o in cases if k == "checker" and n in ("grow", "odd"))


def test_reference_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(7)
    sizes = [(240, 320, 480, 480)] + [tuple(int(v) for v in rng.randint(1, 90, 4)) for _ in range(12)]
    for H, W, OH, OW in sizes:
        for kind in R.CONTENTS:
            a = R.content(kind, H, W, seed=H + W)
            want = np.asarray(Image.fromarray(a).resize((OW, OH), Image.BICUBIC))
            assert np.array_equal(R.resize(a, OH, OW), want), (H, W, OH, OW, kind)


def test_coefficient_tables_equal_the_scalar_definition():
    from bridgeqa_amd import view_data as VD
    for i, o in ((24, 48), (32, 48), (37, 48), (29, 48), (131, 48), (97, 48), (31, 40), (1, 8), (7, 8), (5, 16), (3, 16),
                 (240, 480), (320, 480), (968, 480), (1296, 480), (968, 384), (1296, 384), (1000, 7)):
        (b, k), (rb, rk) = VD.coefficients(i, o), R.coefficients(i, o)
        assert b.dtype == k.dtype == np.int32 and np.array_equal(b, rb) and np.array_equal(k, rk), (i, o)
        assert int(np.abs(k.astype(np.int64)).sum(1).max()) * 255 < 1.4e9          # the int32 sum cannot overflow
    b, k = VD.coefficients(48, 48)                                                   # the skipped pass: the byte itself
    assert np.array_equal(b[:, 0], np.arange(48)) and (b[:, 1] == 1).all() and (k == 1 << 22).all() and k.shape == (48, 1)
    assert R.coefficients(131, 48)[1].shape[1] == 13 and R.coefficients(97, 48)[1].shape[1] == 11


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("layout", ("nchw", "patches"))
def test_cpu_path_equals_the_reference_bitwise(dtype, layout):
    from bridgeqa_amd.view_data import ViewBatcher, ViewStore
    cases = golden_cases()
    store = ViewStore([a for _, _, a, _ in cases], "cpu")
    assert len(store) == 21 and store.nbytes == sum(a.size for _, _, a, _ in cases) and store.base.dtype == np.int64
    for OH, OW in ((48, 48), (48, 40), (8, 8), (16, 16)):
        pick = [i for i, (_, _, _, o) in enumerate(cases) if o.shape[:2] == (OH, OW)]
        b = ViewBatcher(store, (OH, OW), dtype=dtype, layout=layout, patch=8)
        got = b.prepare(pick)["images"]
        want = expected([(cases[i][2], OH, OW) for i in pick], dtype, layout, 8)
        assert got.dtype == dtype and got.shape == (len(pick), 1) + want.shape[1:]
        assert torch.equal(bits(got[:, 0]), bits(want)), (OH, OW)
        if layout == "nchw" and dtype == torch.float32:                             # and so equals Pillow's bytes through the table
            table = R.norm_table()
            for j, i in enumerate(pick):
                o = torch.from_numpy(np.array(cases[i][3])).permute(2, 0, 1).long()
                assert torch.equal(bits(got[j, 0]), bits(torch.gather(table, 1, o.reshape(3, -1)).reshape(3, OH, OW)))
    # (B, V), repeated and out-of-order indices, views of different sizes in one batch
    idx = [[20, 0], [3, 3], [7, 19]]
    got = ViewBatcher(store, 48, dtype=dtype, layout=layout, patch=16).prepare(torch.tensor(idx))["images"]
    want = expected([(cases[i][2], 48, 48) for row in idx for i in row], dtype, layout, 16)
    assert got.shape[:2] == (3, 2) and torch.equal(bits(got.reshape(want.shape)), bits(want))


def test_preprocess_views_equals_the_reference():
    from bridgeqa_amd.view_data import preprocess_views
    frames = np.stack([R.content(k, 31, 48, seed=3) for k in R.CONTENTS])
    got = preprocess_views(torch.from_numpy(frames), (40, 48))
    assert torch.equal(bits(got), bits(expected([(f, 40, 48) for f in frames])))
    got = preprocess_views(torch.from_numpy(frames), 32, dtype=torch.bfloat16, layout="patches", patch=16)
    assert got.shape == (3, 4, 768)
    assert torch.equal(bits(got), bits(expected([(f, 32, 32) for f in frames], torch.bfloat16, "patches", 16)))


def test_all_768_table_entries_equal_totensor_and_normalize():
    from bridgeqa_amd import view_data as VD
    table = VD.norm_table()
    assert table.shape == (3, 256) and table.dtype == torch.float32
    m, s = torch.tensor(VD.CLIP_MEAN, dtype=torch.float32), torch.tensor(VD.CLIP_STD, dtype=torch.float32)
    for c in range(3):
        # ToTensor: HWC bytes -> CHW float / 255; Normalize: (x - mean[:, None, None]) / std[:, None, None]
        img = torch.arange(256, dtype=torch.uint8).reshape(16, 16, 1).expand(16, 16, 3).contiguous()
        x = img.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
        x = x.sub(m[:, None, None]).div(s[:, None, None])
        assert torch.equal(bits(table[c]), bits(x[c].reshape(256))), c
    assert VD.CLIP_MEAN == R.CLIP_MEAN == (0.48145466, 0.4578275, 0.40821073) and VD.CLIP_STD == R.CLIP_STD
    other = VD.norm_table((0.5, 0.4, 0.3), (0.2, 0.25, 0.5))
    assert torch.equal(bits(other), bits(R.norm_table((0.5, 0.4, 0.3), (0.2, 0.25, 0.5)))) and not torch.equal(other, table)


def test_out_is_written_in_place_and_argument_errors_raise():
    from bridgeqa_amd.view_data import ViewBatcher, ViewStore, preprocess_views
    frames = [R.content("random", 24, 32, 1), R.content("ramp", 37, 29, 2)]
    store = ViewStore(frames, "cpu")
    b = ViewBatcher(store, 48)
    out = b.empty(2, 2)
    out["images"].fill_(7)
    out["question"] = ["kept"]
    ptr = out["images"].data_ptr()
    got = b.prepare([[0, 1], [1, 1]], out=out)
    assert got is out and out["question"] == ["kept"] and out["images"].data_ptr() == ptr
    assert torch.equal(bits(out["images"].reshape(4, 3, 48, 48)), bits(expected([(frames[i], 48, 48) for i in (0, 1, 1, 1)])))
    assert b.spec(2, 2) == {"images": ((2, 2, 3, 48, 48), torch.float32)}
    for bad in (torch.empty(2, 2, 3, 48, 40), torch.empty(2, 2, 3, 48, 48, dtype=torch.bfloat16),
                torch.empty(2, 2, 3, 48, 96)[..., ::2], [1, 2]):
        with pytest.raises(ValueError, match="images"):
            b.prepare([[0, 1], [1, 1]], out={"images": bad})
    for idx in ([0, 2], [-1], [], [[[0]]], [0.5]):
        with pytest.raises(ValueError):
            b.prepare(idx)
    for kw in (dict(dtype=torch.float16), dict(layout="nhwc"), dict(layout="patches", patch=7), dict(size=0),
               dict(std=(1.0, 0.0, 1.0)), dict(mean=(0.5, 0.5))):
        with pytest.raises(ValueError):
            ViewBatcher(store, **dict(dict(size=48), **kw))
    for f in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            ViewStore([f], "cpu")
    with pytest.raises(ValueError):
        ViewStore([], "cpu")
    with pytest.raises(ValueError):
        preprocess_views(torch.zeros(2, 3, 8, 8), 8)
    # shrinking so far that one output row's input rows do not fit a workgroup's LDS: the limit is named
    with pytest.raises(ValueError, match="61440 bytes of LDS"):
        ViewBatcher(ViewStore([np.zeros((16000, 16, 3), np.uint8)], "cpu"), (8, 4000))


def test_tile_height_keeps_the_lds_image_inside_a_workgroup():
    from bridgeqa_amd import view_data as VD
    for (H, W), size in (((240, 320), 480), ((968, 1296), 480), ((968, 1296), 384), ((97, 131), 48)):
        plan = VD._Plan([(H, W)], [0], size, size, "cpu")
        assert 1 <= plan.tile_rows <= VD.TILE_ROWS and VD.NORM_BYTES + plan.lds_rows * 3 * size <= VD.LDS_BYTES
        bounds = plan.tables[(H, size)][0].astype(np.int64)
        for r0 in range(0, size, plan.tile_rows):
            t = bounds[r0:r0 + plan.tile_rows]
            assert (t[:, 0] + t[:, 1]).max() - t[:, 0].min() <= plan.lds_rows
    assert VD._Plan([(240, 320)], [0], 480, 480, "cpu").tile_rows == VD.TILE_ROWS
    assert VD._Plan([(968, 1296)], [0], 480, 480, "cpu").tile_rows < VD.TILE_ROWS     # LDS decides here


def test_consumers_accept_the_new_inputs_on_the_host():
    """vit.PatchEmbed takes the patch-major tensor and gives what it gives for the NCHW one; encode_views takes raw frames"""
    from bridgeqa_amd import vit
    from bridgeqa_amd.view_data import preprocess_views
    torch.manual_seed(0)
    frames = torch.from_numpy(np.stack([R.content("ramp", 24, 32, seed=i) for i in range(2)]))
    pe = vit.PatchEmbed(img_size=32, patch_size=16, embed_dim=8)
    with torch.no_grad():
        a = pe(preprocess_views(frames, 32))
        b = pe(preprocess_views(frames, 32, layout="patches", patch=16))
    assert a.shape == (2, 4, 8) and torch.equal(a, b)
    with pytest.raises(AssertionError):
        pe(torch.zeros(2, 4, 767))


def test_header_is_c99_additive_and_bound(tmp_path):
    from bridgeqa_amd import _cabi, _ext, view_data
    assert "bqhip_view.h" in _cabi.ADDITIVE_HEADERS
    assert "bq_view_prep" in _cabi.ADDITIVE_PROTOS and "bq_view_prep" not in _cabi.PROTOS
    restype, argtypes = _cabi.ADDITIVE_PROTOS["bq_view_prep"]
    assert restype is _cabi.ctypes.c_int and argtypes[-1] is _cabi.ctypes.c_void_p and len(argtypes) == 19
    assert _ext._lib.bq_view_prep.argtypes == argtypes
    assert _cabi.DEFINES["BQHIP_ABI_VERSION"] == 6 and len(_cabi.PROTOS) == 97
    assert (view_data.COLS, view_data.DESC, view_data.LDS_BYTES) == (_ext.VIEW_COLS, _ext.VIEW_DESC, _ext.VIEW_LDS_BYTES)
    assert view_data.PRECISION_BITS == _cabi.ADDITIVE_DEFINES["BQ_VIEW_PRECISION_BITS"] == R.PRECISION_BITS
    assert '#include "bqhip_view.h"' in open(os.path.join(ROOT, "include", "bqhip_fusion.h")).read()
    src = tmp_path / "t.c"
    src.write_text('#include "bqhip_view.h"\nint main(void) { return BQ_VIEW_COLS == 5 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    syms = subprocess.run(["nm", "-D", "--defined-only", _ext.library_path()], capture_output=True, text=True).stdout
    assert " T bq_view_prep\n" in syms
    # the library's own checks: a status and a text, no launch (no device is touched before them)
    st = _ext._lib.bq_view_prep(None, 3, None, 1, None, None, 1, 1, None, 1, None, None, 8, 8, 8, 8, 0, 0, None)
    assert st == _ext._D["BQ_EINVAL"] and b"null pointer" in _ext._lib.bq_last_error()
    st = _ext._lib.bq_view_prep(None, 3, None, 1, None, None, 1, 1, None, 1, None, None, 8, 8, 8, 8, 0, 3, None)
    assert st == _ext._D["BQ_EINVAL"] and b"patch = 3" in _ext._lib.bq_last_error()
    st = _ext._lib.bq_view_prep(None, 3, None, 1, None, None, 1, 1, None, 1, None, None, 480, 480, 32, 64, 0, 0, None)
    assert st == _ext._D["BQ_EINVAL"] and b"LDS" in _ext._lib.bq_last_error()


def test_view_kernels_use_no_scratch():
    from bridgeqa_amd import build
    res = build.kernel_resources()
    if res is None:
        pytest.skip("the library was not built by build.py here: no resource remarks")
    mine = {k: v for k, v in res.items() if "view_prep_kernel" in k}
    assert len(mine) == 8, sorted(mine)                       # fp32 / bf16 x four-wide / single x NCHW / patches
    for k, v in mine.items():
        assert v["scratch"] == 0 and v["lds"] == 0, (k, v)    # (the LDS image is dynamic: sized per launch)
