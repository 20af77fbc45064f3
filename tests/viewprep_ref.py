"""The definition bridgeqa_amd.view_data is held to, in plain numpy and independent of the package: Pillow's 8-bit bicubic
resize of an RGB image (horizontal pass, bytes, vertical pass; a = -0.5; the support widens when shrinking; coefficients in
IEEE double, rounded to 22 fractional bits) and the ToTensor / Normalize table.  tests/test_view_prep_cpu.py holds it to
the recorded Pillow outputs of tests/golden/viewprep/ and to a live Pillow where one is installed."""
import math
import zlib

import numpy as np

PRECISION_BITS = 22
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# (name, H, W, OH, OW) of the recorded goldens: every extent stays under 64 but the 131 of the shrinking case
SIZES = (("grow", 24, 32, 48, 48), ("odd", 37, 29, 48, 48), ("shrink", 97, 131, 48, 48), ("vskip", 48, 31, 48, 40),
         ("copy", 48, 48, 48, 48), ("row", 1, 7, 8, 8), ("tiny", 5, 3, 16, 16))
CONTENTS = ("random", "checker", "ramp")


def bicubic(t):
    t, a = abs(t), -0.5
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0
    if t < 2.0:
        return (((t - 5.0) * t + 8.0) * t - 4.0) * a
    return 0.0


def coefficients(in_size, out_size):
    """-> (bounds (out, 2) int32 = first input index and count, k (out, ksize) int32, zero behind the count)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    k = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = xmin, n
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
    return bounds, k


def _pass(img, out_size, axis):
    """one pass along `axis` (0 rows, 1 columns) of an (H, W, 3) byte image"""
    in_size = img.shape[axis]
    if in_size == out_size:
        return img                                       # skipped: no filter, no rounding
    bounds, k = coefficients(in_size, out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for xx in range(out_size):
        xmin, n = bounds[xx]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k[xx, :n].astype(np.int64), src[xmin:xmin + n], axes=(0, 0))
        assert np.abs(acc).max() < 2 ** 31
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, OH, OW):
    """(H, W, 3) uint8 -> (OH, OW, 3) uint8: Image.fromarray(img).resize((OW, OH), Image.BICUBIC)"""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    return np.ascontiguousarray(_pass(_pass(img, OW, 1), OH, 0))


def norm_table(mean=CLIP_MEAN, std=CLIP_STD):
    """(3, 256) fp32: ToTensor then Normalize of every byte, with torch's own fp32 operations"""
    import torch
    b = torch.arange(256, dtype=torch.uint8)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return b.to(torch.float32).div(255)[None, :].sub(m[:, None]).div(s[:, None])


def preprocess(img, OH, OW, mean=CLIP_MEAN, std=CLIP_STD):
    """-> (3, OH, OW) fp32 torch tensor = table[c][resized byte]"""
    import torch
    r = torch.from_numpy(np.array(resize(img, OH, OW))).permute(2, 0, 1).long()
    return torch.gather(norm_table(mean, std), 1, r.reshape(3, -1)).reshape(3, OH, OW)


def to_patches(x, p):
    """(..., 3, OH, OW) -> (..., (OH / p) (OW / p), 3 p p): the unfold of vit.PatchEmbed.forward"""
    lead, (C, H, W) = x.shape[:-3], x.shape[-3:]
    x = x.reshape(-1, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(-1, (H // p) * (W // p), C * p * p)
    return x.reshape(*lead, (H // p) * (W // p), C * p * p)


def content(kind, H, W, seed=0):
    """the pixel contents of the cases: random bytes, a 0 / 255 checkerboard (drives the clamp at both ends), a noisy ramp"""
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        a = (((y + x) & 1) * 255).astype(np.uint8)
        return np.stack([a, 255 - a, a], 2)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        a = (x * 255.0 / max(W - 1, 1) * 0.6 + y * 255.0 / max(H - 1, 1) * 0.4)[:, :, None] + rng.randint(-6, 7, (H, W, 3))
        return np.clip(a, 0, 255).astype(np.uint8)
    raise ValueError(kind)


def case_seed(name, kind):
    return zlib.crc32(("%s/%s" % (name, kind)).encode()) % 1000


def golden_cases(g):
    """the recorded file -> [(name, kind, input (H, W, 3), Pillow's output (OH, OW, 3))]; an input the file holds only as a
    checksum is regenerated from its seed and held to that checksum"""
    out = []
    for name, H, W, OH, OW in SIZES:
        for kind in CONTENTS:
            key = "%s/%s" % (name, kind)
            a = g["in/" + key] if "in/" + key in g else content(kind, H, W, seed=case_seed(name, kind))
            assert a.shape == (H, W, 3) and zlib.crc32(a.tobytes()) == int(g["crc/" + key]), key
            assert g["out/" + key].shape == (OH, OW, 3)
            out.append((name, kind, a, g["out/" + key]))
    return out
