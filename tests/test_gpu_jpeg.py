"""The device JPEG decoder on the GPU (csrc/fdet_jpeg.hip fdet_jpeg_reconstruct, fdet_amd/datasets/jpeg.py): banks decoded
from the fixtures of tests/golden/jpeg/ against `DeviceImageBank.from_arrays` of what PIL decoded from them
(tests/golden/g21_jpeg.npz).  Zero differing bytes everywhere: tests/test_jpeg_host.py shows on the CPU that the numpy
restatement of the kernels' arithmetic reaches PIL's output for every fixture."""
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
JPEG_DIR = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(JPEG_DIR, "manifest.json")))
SUPPORTED = [e["file"][:-4] for e in MANIFEST if e["kind"] == "supported"]


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets import augment, jpeg
    return augment, jpeg


def _blob(name) -> bytes:
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def goldens():
    z = np.load(os.path.join(HERE, "golden", "g21_jpeg.npz"))
    return {k: z[k] for k in z.files}


def _same(bank, want):
    assert bank.table.dtype == want.table.dtype and np.array_equal(bank.table, want.table)
    assert torch.equal(bank.d_table, want.d_table)
    n = int(want.table["offset"][-1]) + int(want.table["h"][-1]) * int(want.table["w"][-1]) * 3
    lead = int(want.table["offset"][0])
    assert bank.data.numel() == want.data.numel()
    assert torch.equal(bank.data[lead:n], want.data[lead:n])
    assert not bank.data[:lead].any()


@pytest.mark.parametrize("lead", [0, 64])
def test_ragged_batch_of_every_supported_fixture_is_byte_identical(goldens, lead):
    A, J = _mods()
    dec = J.DeviceJpegDecoder("cuda")
    bank = dec.decode_bytes([_blob(n) for n in SUPPORTED], lead_bytes=lead)
    want = A.DeviceImageBank.from_arrays([goldens[n] for n in SUPPORTED], "cuda", lead_bytes=lead)
    assert dec.fallbacks == [] and dec.chunks == 1
    for i, n in enumerate(SUPPORTED):                        # per image first: a failure names the fixture
        o, size = int(want.table["offset"][i]), goldens[n].size
        diff = int((bank.data[o:o + size] != want.data[o:o + size]).sum())
        assert diff == 0, f"{n}: {diff} of {size} bytes differ"
    _same(bank, want)


def test_small_chunks_use_both_staging_buffers_and_the_reuse_event(goldens):
    A, J = _mods()
    order = SUPPORTED[::-1] + SUPPORTED                      # the photographs first, then everything again
    dec = J.DeviceJpegDecoder("cuda", workers=4, chunk_bytes=64 << 10)
    bank = dec.decode_bytes([_blob(n) for n in order])
    assert dec.chunks >= 3, dec.chunks
    _same(bank, A.DeviceImageBank.from_arrays([goldens[n] for n in order], "cuda"))
    one = J.DeviceJpegDecoder("cuda", workers=1, chunk_bytes=128)            # every image a chunk of its own
    bank = one.decode_bytes([_blob(n) for n in SUPPORTED])
    assert one.chunks == len(SUPPORTED)
    _same(bank, A.DeviceImageBank.from_arrays([goldens[n] for n in SUPPORTED], "cuda"))


def test_an_unsupported_file_falls_back_to_pil_in_its_slot(goldens, tmp_path):
    pytest.importorskip("PIL.Image")
    A, J = _mods()
    from PIL import Image
    order = SUPPORTED[:3] + ["prog_53x37"] + SUPPORTED[3:6]
    dec = J.DeviceJpegDecoder("cuda")
    bank = dec.decode_bytes([_blob(n) for n in order], lead_bytes=3)
    assert dec.fallbacks == [3]
    _same(bank, A.DeviceImageBank.from_arrays([goldens[n] for n in order], "cuda", lead_bytes=3))
    # a file that is no JPEG at all goes the same way (decode_files, by path)
    Image.fromarray(goldens["c420_17x9"]).save(tmp_path / "a.png")
    shutil.copyfile(os.path.join(JPEG_DIR, "c422_53x37.jpg"), tmp_path / "b.jpg")
    bank = dec.decode_files([tmp_path / "a.png", tmp_path / "b.jpg"])
    assert dec.fallbacks == [0]
    _same(bank, A.DeviceImageBank.from_arrays([goldens["c420_17x9"], goldens["c422_53x37"]], "cuda"))


def test_a_truncated_file_raises_and_the_decoder_goes_on_working(goldens, tmp_path):
    A, J = _mods()
    from fdet_amd import FdetError
    dec = J.DeviceJpegDecoder("cuda")
    with pytest.raises(FdetError, match="c420_53x37_q75_cut"):
        dec.decode_files([os.path.join(JPEG_DIR, n + ".jpg") for n in (SUPPORTED[0], "c420_53x37_q75_cut", SUPPORTED[1])])
    with pytest.raises(FdetError, match="image 1"):
        dec.decode_bytes([_blob(SUPPORTED[0]), b"\xff\xd8\xff\xe0 no jpeg behind the magic"])
    bank = dec.decode_bytes([_blob(n) for n in SUPPORTED])
    _same(bank, A.DeviceImageBank.from_arrays([goldens[n] for n in SUPPORTED], "cuda"))


def test_bank_from_files_with_the_device_decoder_equals_the_pil_bank():
    pytest.importorskip("PIL.Image")
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets.WIDERFace.annotations import bank_from_files
    paths = [os.path.join(JPEG_DIR, n + ".jpg") for n in SUPPORTED + ["prog_53x37"]]
    _same(bank_from_files(paths, "cuda", decoder="device"), bank_from_files(paths, "cuda"))


def test_reconstruct_rejects_a_descriptor_past_the_bank_before_it_writes(goldens):
    import fdet_amd  # noqa: F401
    from fdet_amd import FdetError, hotpath as hp
    d = np.zeros(1, hp.JPEG_DESC_DTYPE)
    d["width"], d["height"], d["ncomp"], d["hs"], d["vs"] = 16, 16, 3, 2, 2
    d["blocks_w"], d["blocks_h"], d["qt"] = [2, 1, 1], [2, 1, 1], 1
    d["coef_offset"], d["plane_offset"] = [0, 256, 320], [0, 256, 320]
    coef = torch.zeros(384, dtype=torch.int16, device="cuda")
    ws = torch.zeros(384, dtype=torch.uint8, device="cuda")
    bank = torch.full((1031,), 7, dtype=torch.uint8, device="cuda")
    d_d = torch.from_numpy(d.view(np.uint8).copy()).cuda()
    d["bank_offset"] = 1031 - 767
    with pytest.raises(FdetError, match="past the bank"):
        hp.jpeg_reconstruct(coef, d_d, d, ws, bank)
    torch.cuda.synchronize()
    assert bool((bank == 7).all())
    d["bank_offset"] = 1031 - 768                            # an odd offset; the bank's last byte is the image's last byte
    d_d = torch.from_numpy(d.view(np.uint8).copy()).cuda()
    hp.jpeg_reconstruct(coef, d_d, d, ws, bank)
    torch.cuda.synchronize()
    assert bool((bank[:263] == 7).all()) and bool((bank[263:] == 128).all())     # all-zero coefficients decode to mid grey


# ------------------------------------------------------------------------------------------------------- end to end
def _trained_small():
    from fdet_amd.models.PoolResnet import PoolResnet
    z = np.load(os.path.join(HERE, "golden", "g6_trained_small.npz"))
    P = {k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    model = PoolResnet(filters=32, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.02, iou_threshold=0.3)
    model.load_state_dict(P)
    return model.cuda().eval()


def test_tiled_detector_gives_the_same_rows_on_both_banks(goldens):
    A, J = _mods()
    from fdet_amd import tiling
    names = ["photo_13", "photo_8"]
    model = _trained_small()
    det = tiling.TiledDetector(model, tile_sizes=(320,), overlap=0.25, include_whole=True)
    a = det.detect(J.DeviceJpegDecoder("cuda").decode_bytes([_blob(n) for n in names]), [0, 1])
    b = det.detect(A.DeviceImageBank.from_arrays([goldens[n] for n in names], "cuda"), [0, 1])
    assert int(b[1].sum()) >= 1                              # cannot pass on empty output
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_detect_images_writes_the_same_files_with_and_without_device_jpeg(tmp_path, monkeypatch):
    pytest.importorskip("PIL.Image")
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images
    monkeypatch.chdir(tmp_path)
    torch.save(_trained_small().state_dict(), tmp_path / "small.pth")
    (tmp_path / "imgs" / "event").mkdir(parents=True)
    shutil.copyfile(os.path.join(JPEG_DIR, "photo_13.jpg"), tmp_path / "imgs" / "event" / "13.jpg")
    shutil.copyfile(os.path.join(JPEG_DIR, "photo_8.jpg"), tmp_path / "imgs" / "8.jpg")
    base = ["--model", "poolresnet", "--filters", "32", "--checkpoint", str(tmp_path / "small.pth"), "--images",
            str(tmp_path / "imgs"), "--tile", "320", "--probability-threshold", "0.02", "--iou-threshold", "0.3"]
    pil = detect_images.main(base + ["--out", str(tmp_path / "pil.txt")])
    dev = detect_images.main(base + ["--out", str(tmp_path / "dev.txt"), "--device-jpeg"])
    text = (tmp_path / "pil.txt").read_text()
    assert text.startswith("8.jpg\n") and "event/13.jpg\n" in text and int(pil["counts"].sum()) >= 1
    assert (tmp_path / "dev.txt").read_text() == text
    assert torch.equal(dev["rows"], pil["rows"]) and torch.equal(dev["counts"], pil["counts"])


def test_train_model_runs_an_epoch_on_a_miniature_wider_tree(tmp_path, monkeypatch):
    pytest.importorskip("PIL.Image")
    import fdet_amd  # noqa: F401
    from fdet_amd import train_model
    monkeypatch.chdir(tmp_path)
    root = tmp_path / "wider"
    (root / "wider_face_split").mkdir(parents=True)
    faces = {"photo_13": ["120 60 80 100 0 0 0 0 0 0"], "photo_8": ["200 90 60 70 0 0 0 0 0 0", "40 50 30 30 0 0 0 0 0 0"],
             "c420_64x48_rst3": ["0 0 0 0 0 0 0 0 0 0"],
             "c444_53x37_q90": ["1 1 9 9 0 0 0 0 0 0", "2 2 9 9 0 0 0 0 0 0", "3 3 9 9 0 0 0 0 0 0"]}      # three faces: filtered
    for split, names in (("train", ["photo_13", "photo_8", "c420_64x48_rst3", "c444_53x37_q90"]), ("val", ["photo_8", "photo_13"])):
        d = root / f"WIDER_{split}" / "images" / "0--Parade"
        d.mkdir(parents=True)
        lines = []
        for n in names:
            shutil.copyfile(os.path.join(JPEG_DIR, n + ".jpg"), d / f"{n}.jpg")
            lines += [f"0--Parade/{n}.jpg", str(0 if faces[n][0].startswith("0 0 0 0") else len(faces[n]))] + faces[n]
        (root / "wider_face_split" / f"wider_face_{split}_bbx_gt.txt").write_text("\n".join(lines) + "\n")
    common = ["--filters", "8", "--epochs", "1", "--batch-size", "2", "--wider-root", str(root)]
    for extra in ([], ["--device-jpeg"]):
        hist = train_model.main(common + extra)
        assert len(hist["train"]) == 1 and len(hist["val"]) == 1 and np.isfinite(float(hist["train"][-1]["loss"]))
