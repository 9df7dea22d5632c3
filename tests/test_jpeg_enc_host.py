"""Host half of the device JPEG encoder (csrc/fdet_jpeg_enc.hip: fdet_jpeg_quant_tables, fdet_jpeg_write_header, the argument
checks of the two device entry points) and the numpy restatement of its device half (tests/jpeg_enc_cpu_ref.py), against the
files PIL wrote (tests/golden/jpeg_enc/, tools/make_goldens_jpeg_enc.py) and against a live PIL.  No GPU.  The bound
everywhere is zero differing bytes: every stage is integer arithmetic."""
import ctypes
import io
import os

import numpy as np
import pytest

import jpeg_enc_cpu_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg_enc")
HEADER_BYTES = 623
SHAPE_IDS = [f"{w}x{h}" for w, h in R.SHAPES]


@pytest.fixture(scope="module")
def fixtures():
    """{(width, height): the archive's arrays}; every case of the list must be there."""
    out = {}
    for w, h in R.SHAPES:
        with np.load(os.path.join(GOLDEN, f"{w}x{h}.npz")) as z:
            out[(w, h)] = {k: z[k] for k in z.files}
    for name, kind, w, h, _q, _s in R.cases():
        assert f"pil_{name}" in out[(w, h)] and f"src_{kind}" in out[(w, h)], name
    return out


@pytest.fixture(scope="module")
def L():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    return _native.lib()


def _cases_of(shape):
    return [c for c in R.cases() if (c[2], c[3]) == shape]


def test_the_case_list_is_the_one_the_encoder_was_specified_with():
    assert R.SHAPES == [(1, 1), (8, 8), (16, 16), (17, 9), (53, 37), (100, 75), (33, 130), (99, 131)]
    assert R.KINDS == ("noise", "ramp", "saturated", "constant") and R.QUALITIES == (5, 75, 100)
    assert len(R.cases()) == 8 * 4 * 3 * 3


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_the_restatement_writes_the_fixture_files(shape, fixtures):
    for name, kind, w, h, q, sub in _cases_of(shape):
        src = fixtures[shape][f"src_{kind}"]
        assert np.array_equal(src, R.source(kind, w, h)), name
        assert R.encode(src, q, sub) == fixtures[shape][f"pil_{name}"].tobytes(), name


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_the_fixtures_and_the_restatement_are_what_pil_writes_today(shape, fixtures):
    Image = pytest.importorskip("PIL.Image")
    for name, kind, _w, _h, q, sub in _cases_of(shape):
        src = fixtures[shape][f"src_{kind}"]
        f = io.BytesIO()
        Image.fromarray(src).save(f, "JPEG", quality=q, subsampling=sub)
        assert f.getvalue() == fixtures[shape][f"pil_{name}"].tobytes(), name
    # a shape and settings outside the fixture set, and PIL's defaults
    src = np.random.default_rng(5).integers(0, 256, (45, 70, 3), dtype=np.uint8)
    for q, sub in ((1, 2), (33, 1), (50, 0), (90, 2)):
        f = io.BytesIO()
        Image.fromarray(src).save(f, "JPEG", quality=q, subsampling=sub)
        assert R.encode(src, q, sub) == f.getvalue(), (q, sub)
    f = io.BytesIO()
    Image.fromarray(src).save(f, "JPEG")
    assert R.encode(src) == f.getvalue()


def test_write_header_equals_the_fixtures_up_to_the_scan(L, fixtures):
    buf = ctypes.create_string_buffer(HEADER_BYTES + 8)
    n = ctypes.c_size_t(0)
    for name, _kind, w, h, q, sub in R.cases():
        buf.raw = b"\xaa" * (HEADER_BYTES + 8)
        assert L.fdet_jpeg_write_header(w, h, q, sub, buf, HEADER_BYTES, ctypes.byref(n)) == 0, L.fdet_last_error()
        assert n.value == HEADER_BYTES
        want = fixtures[(w, h)][f"pil_{name}"].tobytes()
        assert buf.raw[:HEADER_BYTES] == want[:HEADER_BYTES], name
        assert want[HEADER_BYTES - 14:HEADER_BYTES - 12] == b"\xff\xda"                    # the header ends with the SOS segment
        assert buf.raw[HEADER_BYTES:] == b"\xaa" * 8, "write_header wrote past its count"
        assert R.header(w, h, q, sub) == want[:HEADER_BYTES]
    # the largest size the format takes
    assert L.fdet_jpeg_write_header(65535, 65535, 75, 2, buf, HEADER_BYTES, ctypes.byref(n)) == 0
    assert buf.raw[:HEADER_BYTES] == R.header(65535, 65535, 75, 2)


def test_quant_tables_equal_pils_dqt_for_every_quality(L):
    Image = pytest.importorskip("PIL.Image")
    out = np.zeros((2, 64), dtype=np.uint16)
    for q in range(1, 101):
        assert L.fdet_jpeg_quant_tables(q, out.ctypes.data) == 0
        f = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(f, "JPEG", quality=q, subsampling=2)
        b = f.getvalue()
        assert b[20:25] == b"\xff\xdb\x00\x43\x00" and b[89:94] == b"\xff\xdb\x00\x43\x01"
        dqt = np.stack([np.frombuffer(b[25:89], np.uint8), np.frombuffer(b[94:158], np.uint8)])  # zigzag order in the file
        assert np.array_equal(out[:, R.ZIGZAG], dqt), q
        assert np.array_equal(out, R.quant_tables(q)), q


@pytest.mark.parametrize("shape", R.SHAPES, ids=SHAPE_IDS)
def test_the_restatements_coefficients_are_what_the_decoder_reads_out_of_pils_file(shape, L, fixtures):
    """Ties encoder and decoder together: fdet_jpeg_entropy_decode of PIL's file gives the quantised coefficients PIL coded,
    dummy blocks included."""
    from fdet_amd import hotpath as hp
    for name, kind, w, h, q, sub in _cases_of(shape):
        data = fixtures[shape][f"pil_{name}"].tobytes()
        rc, info, msg = hp.jpeg_info(data)
        assert rc == 0, msg
        coef = np.zeros(int(info["coef_count"]), np.int16)
        rc, msg = hp.jpeg_entropy_decode(data, coef.ctypes.data, coef.size)
        assert rc == 0, msg
        mine = R.coefficients(fixtures[shape][f"src_{kind}"], q, sub)
        assert mine.shape[0] * 64 == coef.size
        at = 0
        for c, plane in enumerate(R.to_planes(mine, w, h, sub)):
            assert plane.shape[:2] == (int(info["blocks_h"][c]), int(info["blocks_w"][c]))
            assert np.array_equal(plane.reshape(-1), coef[at:at + plane.size]), (name, c)
            at += plane.size


def test_block_bits_sum_to_the_scan_and_stay_within_the_bound(fixtures):
    for name, kind, w, h, q, sub in _cases_of((53, 37)) + _cases_of((1, 1)):
        coef = R.coefficients(fixtures[(w, h)][f"src_{kind}"], q, sub)
        bits = R.block_bits(coef, sub)
        assert int(bits.max()) <= 11 + 16 + 63 * 26
        assert (int(bits.sum()) + 7) // 8 == len(R.scan_bytes(coef, sub)), name


def test_host_entries_reject_bad_arguments(L):
    out = np.zeros((2, 64), dtype=np.uint16)
    for q in (0, 101, -5):
        assert L.fdet_jpeg_quant_tables(q, out.ctypes.data) == -1 and b"quality" in L.fdet_last_error()
    assert L.fdet_jpeg_quant_tables(75, None) == -1 and b"null pointer" in L.fdet_last_error()
    buf = ctypes.create_string_buffer(HEADER_BYTES)
    n = ctypes.c_size_t(0)
    for w, h, q, s, text in ((0, 8, 75, 2, b"bad size"), (8, 65536, 75, 2, b"bad size"), (8, 8, 0, 2, b"quality"),
                             (8, 8, 75, 3, b"subsampling"), (8, 8, 75, -1, b"subsampling")):
        assert L.fdet_jpeg_write_header(w, h, q, s, buf, HEADER_BYTES, ctypes.byref(n)) == -1 and text in L.fdet_last_error()
    assert L.fdet_jpeg_write_header(8, 8, 75, 2, None, HEADER_BYTES, ctypes.byref(n)) == -1
    assert L.fdet_jpeg_write_header(8, 8, 75, 2, buf, HEADER_BYTES, None) == -1
    buf.raw = b"\xaa" * HEADER_BYTES
    n.value = 0
    assert L.fdet_jpeg_write_header(8, 8, 75, 2, buf, HEADER_BYTES - 1, ctypes.byref(n)) == -3                # FDET_EWORKSPACE
    assert n.value == HEADER_BYTES and buf.raw == b"\xaa" * HEADER_BYTES, "a short buffer must stay untouched"
    assert L.fdet_jpeg_enc_ws_bytes(0, 1) == 0 and L.fdet_jpeg_enc_ws_bytes(6, 0) == 0 and L.fdet_jpeg_enc_ws_bytes(6, 65536) == 0
    assert L.fdet_jpeg_enc_ws_bytes(6, 1) == 6 * 136 + 4 and L.fdet_jpeg_enc_ws_bytes(1 << 33, 2) == (1 << 33) * 136 + 8


def _descs(hp, sizes, sub=2):
    hs, vs = R.LUMA_HV[sub]
    d = np.zeros(len(sizes), hp.JPEG_ENC_DESC_DTYPE)
    off = base = 0
    for i, (w, h) in enumerate(sizes):
        mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
        d[i] = (off, base, 0, w, h, mx, my, mx * my * (hs * vs + 2), 0)
        off += w * h * 3
        base += int(d[i]["n_blocks"])
    return d, off, base


PLAN_CASES = [
    (dict(n=0), "n_images"), (dict(quality=0), "quality"), (dict(quality=101), "quality"), (dict(sub=3), "subsampling"),
    (dict(field=("width", 1, 0)), "bad size"), (dict(field=("height", 0, 65536)), "bad size"),
    (dict(field=("mcus_x", 0, 3)), "MCU grid"), (dict(field=("mcus_y", 1, 1)), "MCU grid"),
    (dict(field=("n_blocks", 0, 5)), "n_blocks"), (dict(field=("block_base", 1, 6)), "does not continue"),
    (dict(field=("block_base", 0, 8)), "does not continue"), (dict(field=("bank_offset", 1, -1)), "past the bank"),
    (dict(bank_short=1), "past the bank"), (dict(ws_short=1), "workspace"), (dict(ws_align=8), "16-byte aligned"),
]


@pytest.mark.parametrize("change,text", PLAN_CASES, ids=[t + str(i) for i, (_c, t) in enumerate(PLAN_CASES)])
def test_plan_rejects_bad_arguments_on_the_host(L, change, text):
    """Every call fails validation before anything is enqueued: no GPU is touched and no pointer is dereferenced."""
    from fdet_amd import hotpath as hp
    d, bank_bytes, B = _descs(hp, [(17, 9), (53, 37)])
    if "field" in change:
        name, i, value = change["field"]
        d[name][i] = value
    p = ctypes.c_void_p(0x1000)
    ws = ctypes.c_void_p(0x1000 + change.get("ws_align", 0))
    rc = L.fdet_jpeg_enc_plan(p, bank_bytes - change.get("bank_short", 0), p, d.ctypes.data, change.get("n", 2),
                              change.get("quality", 75), change.get("sub", 2), ws, B * 136 + 8 - change.get("ws_short", 0), None)
    assert rc == (-3 if "ws_short" in change else -1) and text.encode() in L.fdet_last_error(), L.fdet_last_error()
    for k in range(4):                                       # a null pointer in any place
        a = [p, bank_bytes, p, d.ctypes.data, 2, 75, 2, p, B * 136 + 8, None]
        a[(0, 2, 3, 7)[k]] = None
        assert L.fdet_jpeg_enc_plan(*a) == -1 and b"null pointer" in L.fdet_last_error()


EMIT_CASES = [
    (dict(total=(0, 0)), "bit"), (dict(total=(1, 72 * 1665 + 1)), "bit"), (dict(offset=(1, 2)), "scan offset"),
    (dict(offset=(1, 0)), "scan offset"), (dict(offset=(1, 132)), "scan offset"), (dict(offset=(0, -4)), "scan offset"),
    (dict(scan_bytes=139), "scan offset"), (dict(field=("n_blocks", 1, 71)), "n_blocks"), (dict(ws_short=1), "workspace"),
    (dict(scan_align=2), "4-byte aligned"),
]


@pytest.mark.parametrize("change,text", EMIT_CASES, ids=[t.replace(" ", "_") + str(i) for i, (_c, t) in enumerate(EMIT_CASES)])
def test_emit_rejects_bad_totals_and_offsets_on_the_host(L, change, text):
    from fdet_amd import hotpath as hp
    d, _bank_bytes, B = _descs(hp, [(17, 9), (53, 37)])         # 12 and 72 blocks
    totals = np.array([801, 95], dtype=np.uint32)            # 101 -> 104 bytes, 12 bytes
    d["scan_offset"] = [0, 128]
    if "total" in change:
        totals[change["total"][0]] = change["total"][1]
    if "offset" in change:
        d["scan_offset"][change["offset"][0]] = change["offset"][1]
    if "field" in change:
        d[change["field"][0]][change["field"][1]] = change["field"][2]
    p = ctypes.c_void_p(0x1000)
    scan = ctypes.c_void_p(0x2000 + change.get("scan_align", 0))
    rc = L.fdet_jpeg_enc_emit(p, d.ctypes.data, totals.ctypes.data, 2, 2, p, B * 136 + 8 - change.get("ws_short", 0), scan,
                              change.get("scan_bytes", 140), None)
    assert rc == (-3 if "ws_short" in change else -1) and text.encode() in L.fdet_last_error(), L.fdet_last_error()


def test_python_layers_check_their_options_without_a_gpu():
    import inspect
    import fdet_amd  # noqa: F401
    from fdet_amd import detect_images, render, track_frames
    from fdet_amd.datasets.jpeg import DeviceJpegEncoder
    sig = inspect.signature(render.save_images).parameters
    assert [sig[k].default for k in ("threads", "encoder", "quality", "subsampling")] == [16, "pil", 75, "4:2:0"]
    with pytest.raises(ValueError, match="encoder"):
        render.save_images(None, [], encoder="nope")
    sig = inspect.signature(DeviceJpegEncoder.__init__).parameters
    assert [sig[k].default for k in ("quality", "subsampling", "chunk_bytes")] == [75, "4:2:0", 256 << 20]
    with pytest.raises(ValueError, match="quality"):
        DeviceJpegEncoder("cpu", quality=0)
    with pytest.raises(ValueError, match="subsampling"):
        DeviceJpegEncoder("cpu", subsampling="4:1:1")
    for mod in (detect_images, track_frames):
        src = inspect.getsource(mod.main)
        assert "add_jpeg_encode_arguments(ap)" in src and "check_jpeg_encode_arguments(ap, args)" in src
    import argparse
    ap = argparse.ArgumentParser()
    detect_images.add_draw_arguments(ap)
    detect_images.add_chip_arguments(ap, "--chips", "chips")
    detect_images.add_jpeg_encode_arguments(ap)
    a = ap.parse_args(["--draw", "d", "--draw-format", "jpg", "--device-jpeg-encode", "--jpeg-quality", "90"])
    detect_images.check_jpeg_encode_arguments(ap, a)
    assert detect_images.jpeg_encode_options(a) == {"encoder": "device", "quality": 90}
    assert detect_images.jpeg_encode_options(ap.parse_args([])) == {"encoder": "pil", "quality": 75}
    for bad in (["--device-jpeg-encode"], ["--jpeg-quality", "80"], ["--draw", "d", "--draw-format", "jpg", "--jpeg-quality", "0"]):
        with pytest.raises(SystemExit):
            detect_images.check_jpeg_encode_arguments(ap, ap.parse_args(bad))
