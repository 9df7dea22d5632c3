"""The device JPEG encoder on the GPU (csrc/fdet_jpeg_enc.hip, fdet_amd/datasets/jpeg.py DeviceJpegEncoder) against the files
PIL wrote (tests/golden/jpeg_enc/, tools/make_goldens_jpeg_enc.py): zero differing bytes everywhere.  tests/test_jpeg_enc_host.py
shows on the CPU that the numpy restatement of the kernels (tests/jpeg_enc_cpu_ref.py) writes those same files, so the stage
checks here (coefficients, block bit lengths) say which kernel a difference comes from."""
import functools
import io
import os

import numpy as np
import pytest
import torch

import jpeg_enc_cpu_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_enc")
SUBS = {0: "4:4:4", 1: "4:2:2", 2: "4:2:0"}
SETTINGS = [(q, s) for q in R.QUALITIES for s in (0, 1, 2)]
SETTING_IDS = [f"q{q}-{SUBS[s].replace(':', '')}" for q, s in SETTINGS]
IMAGES = [(kind, w, h) for w, h in R.SHAPES for kind in R.KINDS]            # the 32 sources, the bank's order


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets import augment, jpeg
    return augment, jpeg


@functools.lru_cache(maxsize=None)
def _fixtures():
    out = {}
    for w, h in R.SHAPES:
        with np.load(os.path.join(GOLDEN, f"{w}x{h}.npz")) as z:
            out[(w, h)] = {k: z[k] for k in z.files}
    return out


def _sources():
    return [_fixtures()[(w, h)][f"src_{kind}"] for kind, w, h in IMAGES]


def _want(i, q, s) -> bytes:
    kind, w, h = IMAGES[i]
    return _fixtures()[(w, h)][f"pil_{kind}_{w}x{h}_q{q}_s{s}"].tobytes()


@functools.lru_cache(maxsize=None)
def _bank(lead=0):
    A, _ = _mods()
    return A.DeviceImageBank.from_arrays(_sources(), "cuda", lead_bytes=lead)


@functools.lru_cache(maxsize=None)
def _restated(q, s):
    """Per image (coefficients, block bit lengths) of the restatement: computed once per setting."""
    out = []
    for a in _sources():
        c = R.coefficients(a, q, s)
        out.append((c, R.block_bits(c, s)))
    return out


def _check(files, q, s, indices=None):
    idx = range(len(IMAGES)) if indices is None else indices
    assert len(files) == len(idx)
    for f, i in zip(files, idx):
        want = _want(i, q, s)
        kind, w, h = IMAGES[i]
        assert isinstance(f, bytes) and len(f) == len(want), f"{kind} {w}x{h} q{q} {SUBS[s]}: {len(f)} bytes, PIL wrote {len(want)}"
        assert f == want, f"{kind} {w}x{h} q{q} {SUBS[s]}: first difference at byte {next(k for k in range(len(f)) if f[k] != want[k])}"


@pytest.mark.parametrize("q,s", SETTINGS, ids=SETTING_IDS)
def test_files_equal_the_fixtures(q, s):
    _, J = _mods()
    enc = J.DeviceJpegEncoder("cuda", quality=q, subsampling=SUBS[s])
    files = enc.encode(_bank())
    assert enc.chunks == 1
    _check(files, q, s)
    assert enc.scan_bytes == sum(len(R.scan_bytes(c, s)) for c, _b in _restated(q, s))


@pytest.mark.parametrize("q,s", SETTINGS, ids=SETTING_IDS)
def test_coefficients_and_block_bits_equal_the_restatement(q, s):
    """The plan phase's workspace, stage by stage: k_enc_fdct's coefficients, k_enc_bits' lengths, k_enc_scan's offsets and totals."""
    _, J = _mods()
    got = J.DeviceJpegEncoder("cuda", quality=q, subsampling=SUBS[s]).plan_arrays(_bank())
    for (kind, w, h), (coef, bits, start, total), (rc, rb) in zip(IMAGES, got, _restated(q, s)):
        what = f"{kind} {w}x{h} q{q} {SUBS[s]}"
        assert coef.shape == rc.shape and coef.dtype == np.int16, what
        bad = np.argwhere(coef != rc)
        assert bad.size == 0, f"{what}: {len(bad)} coefficients differ, first at block {bad[0][0]} position {bad[0][1]}"
        assert np.array_equal(bits, rb), f"{what}: bit lengths differ at blocks {np.flatnonzero(bits != rb)[:8]}"
        assert np.array_equal(start, np.cumsum(rb, dtype=np.uint32) - rb), f"{what}: bit offsets are not the exclusive scan"
        assert total == int(rb.sum()), what


@pytest.mark.parametrize("s", [0, 1, 2], ids=["444", "422", "420"])
def test_images_at_odd_offsets_in_one_call(s):
    """lead_bytes=1: the bank's first image starts at byte 1, and the images' starts take every residue modulo 4."""
    _, J = _mods()
    bank = _bank(1)
    assert int(bank.table["offset"][0]) == 1 and len({int(o) % 4 for o in bank.table["offset"]}) == 4
    enc = J.DeviceJpegEncoder("cuda", quality=75, subsampling=SUBS[s])
    files = enc.encode(bank)
    assert enc.chunks == 1
    _check(files, 75, s)


def test_a_subset_with_a_repeated_index_in_reverse_order():
    _, J = _mods()
    enc = J.DeviceJpegEncoder("cuda")                        # the defaults: quality 75, 4:2:0
    idx = [31, 17, 17, 4, 0, 30, 17]
    _check(enc.encode(_bank(), idx), 75, 2, idx)
    _check(enc.encode(_bank(), iter(reversed(range(32)))), 75, 2, list(reversed(range(32))))
    assert enc.encode(_bank(), []) == []
    with pytest.raises(IndexError):
        enc.encode(_bank(), [32])
    with pytest.raises(IndexError):
        enc.encode(_bank(), [-1])


@pytest.mark.parametrize("chunk_bytes,chunks", [(1, 32), (40000, None)])
def test_tiny_chunks_return_the_same_bytes(chunk_bytes, chunks):
    _, J = _mods()
    enc = J.DeviceJpegEncoder("cuda", quality=100, subsampling="4:2:2", chunk_bytes=chunk_bytes)
    files = enc.encode(_bank(1))
    assert enc.chunks == chunks if chunks else 2 < enc.chunks < 32
    _check(files, 100, 1)


def test_an_image_of_a_thousand_blocks_with_flat_areas_equals_the_restatement():
    """More blocks than three passes of the scan kernel take, bit offsets beyond 2^16 and runs of all-EOB blocks, between two
    other images of the same call."""
    A, J = _mods()
    g = np.random.default_rng(77)
    big = g.integers(0, 256, (117, 165, 3), dtype=np.uint8)
    big[30:90, 40:120] = 255                                # a flat saturated area: runs of all-EOB blocks
    images = [_sources()[20], big, _sources()[31]]
    bank = A.DeviceImageBank.from_arrays(images, "cuda", lead_bytes=3)
    for q, s in ((100, 0), (75, 2)):
        files = J.DeviceJpegEncoder("cuda", quality=q, subsampling=SUBS[s]).encode(bank)
        for f, a in zip(files, images):
            assert f == R.encode(a, q, s), (q, s, a.shape)


@pytest.mark.parametrize("s", [0, 1, 2], ids=["444", "422", "420"])
def test_decoding_the_encoders_files_gives_what_pil_decodes_from_pils(s):
    Image = pytest.importorskip("PIL.Image")
    A, J = _mods()
    files = J.DeviceJpegEncoder("cuda", quality=75, subsampling=SUBS[s]).encode(_bank())
    got = J.DeviceJpegDecoder("cuda").decode_bytes(files)
    arrays = []
    for i in range(len(IMAGES)):
        with Image.open(io.BytesIO(_want(i, 75, s))) as im:
            arrays.append(np.asarray(im.convert("RGB")))
    want = A.DeviceImageBank.from_arrays(arrays, "cuda")
    assert np.array_equal(got.table, want.table) and torch.equal(got.data, want.data)


def test_files_equal_live_pil_at_settings_outside_the_fixtures():
    Image = pytest.importorskip("PIL.Image")
    _, J = _mods()
    src = _sources()
    for q, sub in ((1, "4:2:0"), (49, "4:2:2"), (50, "4:4:4"), (90, "4:2:0")):
        files = J.DeviceJpegEncoder("cuda", quality=q, subsampling=sub).encode(_bank())
        for a, f in zip(src, files):
            b = io.BytesIO()
            Image.fromarray(a).save(b, "JPEG", quality=q, subsampling=sub)
            assert f == b.getvalue(), (q, sub, a.shape)


def test_save_images_with_the_device_encoder_writes_pils_files(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import fdet_amd  # noqa: F401
    from fdet_amd.render import save_images
    bank = _bank(1)
    n = len(bank)
    ext = [".jpg", ".jpeg", ".JPG", ".png"]
    names = [f"d{i % 3}/{i:02d}{ext[i % 4]}" for i in range(n)]

    def read(root):
        return [(tmp_path / root / name).read_bytes() for name in names]
    save_images(bank, [tmp_path / "before" / name for name in names])                                 # the call as it always was
    src = _sources()
    for name, a, got in zip(names, src, read("before")):
        b = io.BytesIO()
        Image.fromarray(a).save(b, "PNG" if name.endswith(".png") else "JPEG")
        assert got == b.getvalue(), name
    save_images(bank, [tmp_path / "pil" / name for name in names], encoder="pil")
    save_images(bank, [tmp_path / "dev" / name for name in names], threads=3, encoder="device")
    assert read("pil") == read("before") and read("dev") == read("before")
    save_images(bank, [tmp_path / "pil90" / name for name in names], encoder="pil", quality=90, subsampling="4:4:4")
    save_images(bank, [tmp_path / "dev90" / name for name in names], encoder="device", quality=90, subsampling="4:4:4")
    assert read("pil90") == read("dev90") and read("pil90") != read("before")
    for name, a, got in zip(names, src, read("dev90")):
        b = io.BytesIO()
        if name.endswith(".png"):
            Image.fromarray(a).save(b, "PNG")
        else:
            Image.fromarray(a).save(b, "JPEG", quality=90, subsampling="4:4:4")
        assert got == b.getvalue(), name
    with pytest.raises(ValueError):
        save_images(bank, [tmp_path / "x.jpg"], encoder="device")                                    # one path for 32 images


def test_best_shots_saved_as_jpeg_by_either_encoder(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import fdet_amd  # noqa: F401
    from fdet_amd import chips as chips_mod, tracking
    A, _ = _mods()
    T, C = 5, 24
    g = np.random.default_rng(9)
    frames = [g.integers(0, 256, (60, 80, 3), dtype=np.uint8) for _ in range(T)]
    rows = np.zeros((T, 2, 5), np.float32)
    rows[:, 0] = [0.9, 20, 15, 24, 26]
    rows[:, 1] = [0.8, 50, 20, 20, 20]
    counts = np.full(T, 2, np.int32)
    res = tracking.FaceTracker(min_hits=1, max_misses=3, alpha=1.0).update(torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda())
    best = chips_mod.BestShots(size=C, capacity=8)
    best.update(A.DeviceImageBank.from_arrays(frames, "cuda"), res)
    _rec, pics = best.gallery()
    assert len(pics) == 2
    for enc, q in (("pil", 75), ("device", 75), ("pil", 60), ("device", 60)):
        paths = best.save(tmp_path / f"{enc}{q}", "jpg", encoder=enc, quality=q)
        assert [os.path.basename(p) for p in paths] == ["seq0_track1.jpg", "seq0_track2.jpg"]
        for p, a in zip(paths, pics):
            b = io.BytesIO()
            Image.fromarray(a).save(b, "JPEG", quality=q)
            assert open(p, "rb").read() == b.getvalue(), (enc, q, p)


def test_scripts_write_the_same_jpeg_files_with_the_device_encoder(tmp_path, monkeypatch):
    """detect_images --draw / --chips and track_frames --draw / --best-shots with JPEG output: --device-jpeg-encode changes no byte
    of any file."""
    Image = pytest.importorskip("PIL.Image")
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images, track_frames
    monkeypatch.chdir(tmp_path)
    g = np.random.default_rng(3)
    base = g.integers(0, 256, (12, 16, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)          # 96 x 128, blocky
    frames = tmp_path / "frames"
    frames.mkdir()
    for i in range(4):
        Image.fromarray(np.roll(base, 2 * i, axis=1)).save(frames / f"f{i:03d}.png")

    def tree(root):
        files = {os.path.relpath(p, root): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}
        assert files and all(n.endswith(".jpg") and b[:2] == b"\xff\xd8" for n, b in files.items())
        return files
    model = ["--model", "poolresnet", "--filters", "64", "--probability-threshold", "0.02"]
    for tag, extra in (("pil", []), ("dev", ["--device-jpeg-encode"])):
        torch.manual_seed(11)
        track_frames.main(model + ["--frames", str(frames), "--min-hits", "1", "--out", str(tmp_path / f"t_{tag}.txt"), "--draw",
                                   str(tmp_path / f"tdraw_{tag}"), "--draw-format", "jpg", "--anonymize", "pixelate", "--best-shots",
                                   str(tmp_path / f"tshots_{tag}"), "--chip-size", "24", "--chip-format", "jpg", "--jpeg-quality", "85"] + extra)
        torch.manual_seed(11)
        detect_images.main(model + ["--images", str(frames), "--tile", "--out", str(tmp_path / f"d_{tag}.txt"), "--draw",
                                    str(tmp_path / f"ddraw_{tag}"), "--draw-format", "jpg", "--chips", str(tmp_path / f"dchips_{tag}"),
                                    "--chip-format", "jpg", "--jpeg-quality", "85"] + extra)
    for root in ("tdraw", "tshots", "ddraw", "dchips"):
        assert tree(tmp_path / f"{root}_pil") == tree(tmp_path / f"{root}_dev"), root
    a = np.asarray(Image.open(tmp_path / "ddraw_dev" / "f000.jpg"))
    assert a.shape == (96, 128, 3)
