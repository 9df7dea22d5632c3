"""Writes the fixtures of the device JPEG encoder's tests: tests/golden/jpeg_enc/<width>x<height>.npz.

    python tools/make_goldens_jpeg_enc.py

One archive per shape of tests/jpeg_enc_cpu_ref.py's case list (shapes x kinds x qualities x subsamplings).  It holds, as
uint8 arrays, `src_<kind>`: the (H, W, 3) source image, and `pil_<case name>`: the bytes of the file PIL writes for it,
`Image.fromarray(src).save(f, "JPEG", quality=q, subsampling=s)` -- libjpeg-turbo's baseline encoder at its defaults.  These
are PIL's outputs, recorded; the host tests compare them with a live PIL encode wherever PIL imports, so a stale fixture
cannot hide.
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg_enc")


def main():
    import jpeg_enc_cpu_ref as R
    if not features.check_feature("libjpeg_turbo"):
        raise SystemExit("the fixtures are libjpeg-turbo's output; this Pillow is built against another libjpeg")
    os.makedirs(OUT, exist_ok=True)
    per_shape = {}
    for name, kind, w, h, q, sub in R.cases():
        arrays = per_shape.setdefault((w, h), {})
        src = R.source(kind, w, h)
        arrays[f"src_{kind}"] = src
        f = io.BytesIO()
        Image.fromarray(src).save(f, "JPEG", quality=q, subsampling=sub)
        arrays[f"pil_{name}"] = np.frombuffer(f.getvalue(), dtype=np.uint8)
    for (w, h), arrays in per_shape.items():
        path = os.path.join(OUT, f"{w}x{h}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
    print(f"Pillow {Image.__version__}, libjpeg-turbo {features.version('jpg')}")


if __name__ == "__main__":
    main()
