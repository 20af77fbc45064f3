#!/usr/bin/env python
"""Records tests/golden/viewprep/pillow.npz: the inputs of tests/viewprep_ref.py's cases (the larger random ones as a checksum of
what viewprep_ref.content regenerates) and what the installed Pillow gives for them with
Image.fromarray(a).resize((OW, OH), Image.BICUBIC).  Run it where Pillow is installed; the version is stored.

    python tools/make_viewprep_golden.py
"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viewprep_ref as R  # noqa: E402


def main():
    import PIL
    from PIL import Image
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, H, W, OH, OW in R.SIZES:
        for kind in R.CONTENTS:
            a = R.content(kind, H, W, seed=R.case_seed(name, kind))
            got = np.asarray(Image.fromarray(a).resize((OW, OH), Image.BICUBIC))
            assert got.shape == (OH, OW, 3) and got.dtype == np.uint8
            # (inputs that do not compress are regenerated from their seed by viewprep_ref.golden_cases and held to this checksum)
            if H * W <= 1024 or kind == "checker":
                out["in/%s/%s" % (name, kind)] = a
            out["crc/%s/%s" % (name, kind)] = np.array(zlib.crc32(a.tobytes()), dtype=np.int64)
            out["out/%s/%s" % (name, kind)] = got
    d = os.path.join(ROOT, "tests", "golden", "viewprep")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "pillow.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
