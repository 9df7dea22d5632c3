"""Writes the JPEG fixtures of tests/golden/jpeg/ and tests/golden/g21_jpeg.npz (what PIL decodes from each of them).

    python tools/make_goldens_jpeg.py [--photos /root/reference/imgs/test_imgs]

The generated files are PIL encodes of one seeded image (a smooth gradient plus noise plus a few hard edges, so that every
coefficient position is exercised), cropped to the smallest shapes at which each rule of the decoder can go wrong; the two
photographs are copied from the reference's test images.  manifest.json records, per file, what the tests expect of it and
the sampling PIL reports.  The goldens are PIL's `Image.open(f).convert("RGB")`, i.e. libjpeg-turbo's default decode; the
host tests compare them with a live PIL decode wherever PIL imports, so a stale golden cannot hide.
"""
import argparse
import io
import json
import os
import shutil

import numpy as np
from PIL import Image, JpegImagePlugin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")
NPZ = os.path.join(ROOT, "tests", "golden", "g21_jpeg.npz")


def seeded_image(h=64, w=64, seed=21):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 3.0 * xx, 220 - 2.5 * yy, 60 + 1.5 * xx + 1.5 * yy], axis=2)
    img += g.normal(0.0, 12.0, img.shape)
    img[5:20, 8:30] = (250, 10, 10)                      # hard edges, not on the block grid
    img[22:35, 3:12] = (5, 5, 240)
    img[10:33, 41:50] = (255, 255, 255)
    img[30:36, 20:52] = (0, 0, 0)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise_image(h=64, w=64, seed=22):
    g = np.random.default_rng(seed)
    return (g.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)          # full contrast: the range limiter


# name, source, (w, h), mode, save options
CASES = [
    ("c444_53x37_q90", "seeded", (53, 37), "RGB", dict(quality=90, subsampling=0)),
    ("c420_53x37_q75", "seeded", (53, 37), "RGB", dict(quality=75, subsampling=2)),
    ("c422_53x37", "seeded", (53, 37), "RGB", dict(quality=75, subsampling=1)),
    ("c420_16x16", "seeded", (16, 16), "RGB", dict(quality=75, subsampling=2)),
    ("c420_1x1", "seeded", (1, 1), "RGB", dict(quality=75, subsampling=2)),
    ("c420_17x9", "seeded", (17, 9), "RGB", dict(quality=75, subsampling=2)),
    ("grey_40x24", "seeded", (40, 24), "L", dict(quality=75)),
    ("c420_64x48_rst3", "seeded", (64, 48), "RGB", dict(quality=75, subsampling=2, restart_marker_blocks=3)),
    ("c420_53x37_opt", "seeded", (53, 37), "RGB", dict(quality=75, subsampling=2, optimize=True)),
    ("c420_53x37_q100_noise", "noise", (53, 37), "RGB", dict(quality=100, subsampling=2)),
    ("c420_53x37_q5", "seeded", (53, 37), "RGB", dict(quality=5, subsampling=2)),
    # chroma planes of one or two columns take the replicating upsampler; one chroma row has no vertical neighbour
    ("c420_4x3", "seeded", (4, 3), "RGB", dict(quality=90, subsampling=2)),
    ("c422_3x4", "seeded", (3, 4), "RGB", dict(quality=90, subsampling=1)),
    ("c420_6x2", "seeded", (6, 2), "RGB", dict(quality=90, subsampling=2)),
    ("prog_53x37", "seeded", (53, 37), "RGB", dict(quality=75, subsampling=2, progressive=True)),
]
PHOTOS = [("photo_13", "13.jpg"), ("photo_8", "8.jpg")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--photos", default="/root/reference/imgs/test_imgs")
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    src = {"seeded": seeded_image(), "noise": noise_image()}
    manifest, golden = [], {}

    def record(name, kind):
        path = os.path.join(OUT, name + ".jpg")
        entry = {"file": name + ".jpg", "kind": kind}
        if kind != "corrupt":
            with Image.open(path) as im:
                entry["width"], entry["height"] = im.size
                entry["components"] = len(im.getbands())
                entry["sampling"] = JpegImagePlugin.get_sampling(im)       # 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, -1 = none (grey)
                golden[name] = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
        manifest.append(entry)

    for name, which, (w, h), mode, opts in CASES:
        im = Image.fromarray(src[which][:h, :w])
        if mode == "L":
            im = im.convert("L")
        im.save(os.path.join(OUT, name + ".jpg"), "JPEG", **opts)
        record(name, "unsupported" if opts.get("progressive") else "supported")
    whole = open(os.path.join(OUT, "c420_53x37_q75.jpg"), "rb").read()
    with open(os.path.join(OUT, "c420_53x37_q75_cut.jpg"), "wb") as f:
        f.write(whole[:len(whole) // 2])
    record("c420_53x37_q75_cut", "corrupt")
    for name, fn in PHOTOS:
        shutil.copyfile(os.path.join(args.photos, fn), os.path.join(OUT, name + ".jpg"))
        record(name, "supported")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")
    np.savez_compressed(NPZ, **golden)
    total = os.path.getsize(NPZ) + sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print(f"{len(manifest)} fixtures, {total} bytes in all ({os.path.getsize(NPZ)} in {os.path.basename(NPZ)})")


if __name__ == "__main__":
    main()
