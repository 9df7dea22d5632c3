"""The host half of the JPEG decoder (csrc/fdet_jpeg.hip fdet_jpeg_info / fdet_jpeg_entropy_decode) and the numpy
restatement of its device half (tests/jpeg_cpu_ref.py), against what PIL decodes from the fixtures of tests/golden/jpeg/
(tools/make_goldens_jpeg.py).  No GPU.  The bound everywhere is zero differing bytes: both sides are integer pipelines."""
import ctypes
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_cpu_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
JPEG_DIR = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(JPEG_DIR, "manifest.json")))
SUPPORTED = [e for e in MANIFEST if e["kind"] == "supported"]
DECODABLE = [e for e in MANIFEST if e["kind"] != "corrupt"]
SAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), -1: (1, 1)}     # PIL's get_sampling -> luma (hs, vs)


def _bytes(entry) -> bytes:
    with open(os.path.join(JPEG_DIR, entry["file"]), "rb") as f:
        return f.read()


def _name(entry) -> str:
    return entry["file"][:-4]


@pytest.fixture(scope="module")
def goldens():
    z = np.load(os.path.join(HERE, "golden", "g21_jpeg.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def test_the_fixture_set_covers_the_cases():
    names = {_name(e) for e in MANIFEST}
    assert {"c444_53x37_q90", "c420_53x37_q75", "c422_53x37", "c420_16x16", "c420_1x1", "c420_17x9", "grey_40x24",
            "c420_64x48_rst3", "c420_53x37_opt", "c420_53x37_q100_noise", "c420_53x37_q5", "prog_53x37", "c420_53x37_q75_cut",
            "photo_13", "photo_8"} <= names
    assert len(SUPPORTED) >= 13


@pytest.mark.parametrize("entry", SUPPORTED, ids=_name)
def test_info_agrees_with_pil_on_size_and_sampling(hp, entry, goldens):
    rc, info, msg = hp.jpeg_info(_bytes(entry))
    assert rc == 0, msg
    assert (int(info["width"]), int(info["height"]), int(info["ncomp"])) == (entry["width"], entry["height"], entry["components"])
    assert goldens[_name(entry)].shape == (entry["height"], entry["width"], 3)
    hs, vs = SAMPLING[entry["sampling"]]
    assert (int(info["hs"][0]), int(info["vs"][0])) == (hs, vs)
    nc = int(info["ncomp"])
    assert all(int(info["hs"][c]) == 1 and int(info["vs"][c]) == 1 for c in range(1, nc))
    mx, my = -(-entry["width"] // (8 * hs)), -(-entry["height"] // (8 * vs))
    assert (int(info["mcus_x"]), int(info["mcus_y"])) == (mx, my)
    assert [int(v) for v in info["blocks_w"][:nc]] == [mx * hs] + [mx] * (nc - 1)
    assert [int(v) for v in info["blocks_h"][:nc]] == [my * vs] + [my] * (nc - 1)
    assert int(info["coef_count"]) == 64 * sum(int(info["blocks_w"][c]) * int(info["blocks_h"][c]) for c in range(nc))
    assert int(info["restart_interval"]) == (3 if "rst3" in entry["file"] else 0)
    assert int(info["qt"][:nc].min()) >= 1


@pytest.mark.parametrize("entry", SUPPORTED, ids=_name)
def test_entropy_decode_plus_restatement_equals_pil_byte_for_byte(entry, goldens):
    got = R.decode(_bytes(entry))
    want = goldens[_name(entry)]
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("entry", DECODABLE, ids=_name)
def test_the_golden_is_what_pil_decodes_today(entry, goldens):
    Image = pytest.importorskip("PIL.Image")
    with Image.open(os.path.join(JPEG_DIR, entry["file"])) as im:
        live = np.asarray(im.convert("RGB"), dtype=np.uint8)
    assert np.array_equal(live, goldens[_name(entry)])


def test_optimised_and_restart_fixtures_are_what_they_claim():
    """the optimised file carries Huffman tables of its own (not the standard ones of its sibling), the restart file a DRI"""
    files = {_name(e): _bytes(e) for e in MANIFEST}

    def dht(b):
        out, i = [], 2
        while i + 4 <= len(b) and b[i] == 0xFF and b[i + 1] != 0xDA:
            n = (b[i + 2] << 8) | b[i + 3]
            if b[i + 1] == 0xC4:
                out.append(b[i + 4:i + 2 + n])
            i += 2 + n
        return out
    assert dht(files["c420_53x37_opt"]) != dht(files["c420_53x37_q75"])
    assert b"\xff\xdd\x00\x04" in files["c420_64x48_rst3"] and b"\xff\xd0" in files["c420_64x48_rst3"]


def test_progressive_is_unsupported_and_truncated_is_an_error(hp):
    files = {_name(e): _bytes(e) for e in MANIFEST}
    rc, info, msg = hp.jpeg_info(files["prog_53x37"])
    assert rc == hp.JPEG_UNSUPPORTED == -4 and info is None and "progressive" in msg
    coef = np.zeros(1 << 16, np.int16)
    rc, msg = hp.jpeg_entropy_decode(files["prog_53x37"], coef.ctypes.data, coef.size)
    assert rc == hp.JPEG_UNSUPPORTED
    cut = files["c420_53x37_q75_cut"]
    rc, info, _ = hp.jpeg_info(cut)                          # the headers are whole: the size is known, the scan is not
    assert rc == 0 and (int(info["width"]), int(info["height"])) == (53, 37)
    rc, msg = hp.jpeg_entropy_decode(cut, coef.ctypes.data, coef.size)
    assert rc == hp.JPEG_ECORRUPT == -5 and "truncated" in msg
    for n in (2, 3, 20, 200, len(cut) - 1):                  # cut anywhere: an error, never a read past n
        rc, _ = hp.jpeg_entropy_decode(cut[:n], coef.ctypes.data, coef.size)
        assert rc < 0


def test_capacity_one_short_is_an_error_and_nothing_past_capacity_is_written(hp):
    data = _bytes(SUPPORTED[1])
    rc, info, _ = hp.jpeg_info(data)
    need = int(info["coef_count"])
    guard = 64
    buf = np.full(need + guard, 0x5555, dtype=np.int16)
    rc, msg = hp.jpeg_entropy_decode(data, buf.ctypes.data, need - 1)
    assert rc == -3 and "coefficients" in msg
    assert (buf == 0x5555).all()
    rc, msg = hp.jpeg_entropy_decode(data, buf.ctypes.data, need)
    assert rc == 0, msg
    assert (buf[need:] == 0x5555).all() and (buf[:need] != 0x5555).any()


def test_random_bytes_behind_a_valid_soi_are_an_error(hp):
    g = np.random.default_rng(5)
    coef = np.zeros(1 << 16, np.int16)
    for n in (4, 64, 1000, 20000):
        data = b"\xff\xd8" + g.integers(0, 256, n, dtype=np.uint8).tobytes()
        rc, info, msg = hp.jpeg_info(data)
        assert rc < 0 and info is None and msg
        assert hp.jpeg_entropy_decode(data, coef.ctypes.data, coef.size)[0] < 0
    # a good header in front of a random scan: whatever the bits say, the call returns (an error or 64 * blocks coefficients)
    good = _bytes(SUPPORTED[1])
    sos = good.index(b"\xff\xda")
    head = good[:sos + 14]
    for seed in range(8):
        noise = np.random.default_rng(seed).integers(0, 255, 4000, dtype=np.uint8).tobytes()      # no 0xFF: no marker ends it
        rc, _ = hp.jpeg_entropy_decode(head + noise, coef.ctypes.data, coef.size)
        assert rc in (0, hp.JPEG_ECORRUPT)


def test_eight_threads_give_the_coefficients_of_one(hp):
    blobs = [_bytes(e) for e in SUPPORTED]
    alone = [R.entropy_decode(b)[1] for b in blobs]
    jobs = [(i, b) for _ in range(6) for i, b in enumerate(blobs)]
    with ThreadPoolExecutor(max_workers=8) as ex:
        got = list(ex.map(lambda j: (j[0], R.entropy_decode(j[1])[1]), jobs))
    assert len(got) == 6 * len(blobs)
    for i, coef in got:
        assert np.array_equal(coef, alone[i])


def test_null_and_zero_size_arguments_return_einval(hp):
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    L = _native.lib()
    data = _bytes(SUPPORTED[0])
    info = np.zeros(1, hp.JPEG_INFO_DTYPE)
    coef = np.zeros(64, np.int16)
    for rc in (L.fdet_jpeg_info(None, 10, info.ctypes.data), L.fdet_jpeg_info(data, 0, info.ctypes.data),
               L.fdet_jpeg_info(data, len(data), None)):
        assert rc == -1 and b"jpeg_info" in L.fdet_last_error()
    for rc in (L.fdet_jpeg_entropy_decode(None, 10, coef.ctypes.data, 64), L.fdet_jpeg_entropy_decode(data, 0, coef.ctypes.data, 64),
               L.fdet_jpeg_entropy_decode(data, len(data), None, 64), L.fdet_jpeg_entropy_decode(data, len(data), coef.ctypes.data, 0)):
        assert rc == -1 and b"jpeg_entropy_decode" in L.fdet_last_error()
    # the device entry point validates on the host before anything is enqueued: no GPU is touched by these calls
    d = np.zeros(1, hp.JPEG_DESC_DTYPE)
    p = ctypes.c_void_p(0x1000)                              # never dereferenced: every call fails validation first
    h = d.ctypes.data
    for args in ((None, 64, p, h, 1, p, 64, p, 64), (p, 64, None, h, 1, p, 64, p, 64), (p, 64, p, None, 1, p, 64, p, 64),
                 (p, 64, p, h, 1, None, 64, p, 64), (p, 64, p, h, 1, p, 64, None, 64)):
        assert L.fdet_jpeg_reconstruct(*args, None) == -1 and b"null pointer" in L.fdet_last_error()
    for args in ((p, 64, p, h, 0, p, 64, p, 64), (p, 0, p, h, 1, p, 64, p, 64), (p, 64, p, h, 1, p, 0, p, 64),
                 (p, 64, p, h, 1, p, 64, p, 0), (p, 64, p, h, 65536, p, 64, p, 64)):
        assert L.fdet_jpeg_reconstruct(*args, None) == -1 and b"bad sizes" in L.fdet_last_error()


def _desc(hp, **kw):
    d = np.zeros(1, hp.JPEG_DESC_DTYPE)
    d["width"], d["height"], d["ncomp"], d["hs"], d["vs"] = 16, 16, 3, 2, 2
    d["blocks_w"], d["blocks_h"] = [2, 1, 1], [2, 1, 1]
    d["coef_offset"], d["plane_offset"] = [0, 256, 320], [0, 256, 320]
    d["qt"] = 1
    for k, v in kw.items():
        d[k] = v
    return d


@pytest.mark.parametrize("field,value,text", [
    ("blocks_w", [1, 1, 1], "do not cover"), ("blocks_h", [2, 0, 1], "do not cover"), ("width", 17, "do not cover"),
    ("bank_offset", 64 * 1024 - 767, "past the bank"), ("bank_offset", -1, "past the bank"), ("hs", 1, "supported set"),
    ("vs", 3, "supported set"), ("ncomp", 2, "supported set"), ("coef_offset", [0, 256, 328], "past the"),
    ("coef_offset", [4, 256, 320], "misaligned"), ("plane_offset", [0, 256, 324], "misaligned"),
    ("plane_offset", [0, 256, 100000], "past the workspace"), ("width", 0, "bad size")])
def test_reconstruct_rejects_inconsistent_descriptors_on_the_host(hp, field, value, text):
    from fdet_amd import _native
    L = _native.lib()
    p = ctypes.c_void_p(0x1000)
    ok_sizes = (384, 384, 64 * 1024)                        # coef_count, workspace_bytes, bank_bytes
    d = _desc(hp, **{field: value})
    if field == "hs":
        d["vs"] = 2                                          # 1x2 luma sampling
    rc = L.fdet_jpeg_reconstruct(p, ok_sizes[0], p, d.ctypes.data, 1, p, ok_sizes[1], p, ok_sizes[2], None)
    assert rc == -1 and text.encode() in L.fdet_last_error(), L.fdet_last_error()


def test_bank_from_files_rejects_an_unknown_decoder():
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets.WIDERFace.annotations import bank_from_files
    with pytest.raises(ValueError, match="decoder"):
        bank_from_files([], "cpu", decoder="nope")


def test_train_model_parser_accepts_wider_root_and_keeps_every_default():
    import fdet_amd  # noqa: F401
    from fdet_amd import train_model
    d = vars(train_model.build_parser().parse_args([]))
    assert d == dict(model="poolresnet", filters=128, patches=10, size=480, lr=1e-4, epochs=70, batch_size=8, steps_per_epoch=50,
                     val_steps=5, save=None, precision=32, augment=False, bank_size=None, wider_root=None, device_jpeg=False)
    a = train_model.build_parser().parse_args(["--wider-root", "/data/wider", "--device-jpeg"])
    assert a.wider_root == "/data/wider" and a.device_jpeg is True


def test_scripts_take_the_device_jpeg_switch():
    import inspect
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images, run_validation_epoch
    from fdet_amd.datasets.WIDERFace.annotations import bank_from_files
    assert inspect.signature(bank_from_files).parameters["decoder"].default == "pil"
    for mod in (detect_images, run_validation_epoch):
        assert '"--device-jpeg"' in inspect.getsource(mod.main)
