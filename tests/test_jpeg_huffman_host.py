"""The host half of the device Huffman decoder (csrc/fdet_jpeg.hip fdet_jpeg_scan_prepare) and the Python restatement of its
kernels (tests/jpeg_huff_cpu_ref.py) against the host decoder fdet_jpeg_entropy_decode.  No GPU.  Every check is an
equality: the coefficient planes are the host decoder's byte for byte, or the image is flagged where the host decoder
returns an error.  tests/test_gpu_jpeg_huffman.py holds the kernels to the same planes."""
import json
import os
import re

import numpy as np
import pytest

import jpeg_enc_cpu_ref as E
import jpeg_huff_cpu_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
JPEG_DIR = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(JPEG_DIR, "manifest.json")))
SUPPORTED = [e["file"][:-4] for e in MANIFEST if e["kind"] == "supported"]
SUB_BITS = (64, 128, 1024)
GENERATED = {"constant": ("constant", 320, 240, 75, 2), "noise": ("noise", 200, 120, 95, 0), "saturated": ("saturated", 96, 64, 50, 1)}


def _blob(name) -> bytes:
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        return f.read()


def generated(name) -> bytes:
    kind, w, h, q, sub = GENERATED[name]
    return E.encode(E.source(kind, w, h), q, sub)


@pytest.fixture(scope="module")
def hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def host_planes(hp, data):
    """-> (rc, int16 planes) of fdet_jpeg_entropy_decode."""
    rc, info, msg = hp.jpeg_info(data)
    assert rc == 0, msg
    want = np.zeros(int(info["coef_count"]), np.int16)
    rc, _msg = hp.jpeg_entropy_decode(data, want.ctypes.data, want.size)
    return rc, want, info


def restated_segments(data: bytes):
    """The three-line restatement of the unstuffing: the scan ends at the first marker that is no RSTn, splits at the RSTn
    and loses the 00 behind every FF."""
    body = data[R.scan_start(data):]
    end = re.search(rb"\xff[^\x00\xd0-\xd7]", body)
    return [p.replace(b"\xff\x00", b"\xff") for p in re.split(rb"\xff[\xd0-\xd7]", body[:end.start()] if end else body)]


# ------------------------------------------------------------------------------------------------------------ prepare
@pytest.mark.parametrize("name", SUPPORTED + ["c420_53x37_q75_cut"])
def test_prepare_unstuffs_into_aligned_zero_padded_segments(hp, name):
    data = _blob(name)
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
    assert rc == 0, msg
    want = restated_segments(data)
    assert len(segs) == len(want)
    _, info, _ = hp.jpeg_info(data)
    mcus = int(info["mcus_x"]) * int(info["mcus_y"])
    at = mcu = 0
    for s, w in zip(segs, want):
        o, n = int(s["byte_offset"]), int(s["byte_len"])
        assert o == at and o % 16 == 0
        assert scan[o:o + n].tobytes() == w
        at = o + (n + 15) // 16 * 16
        assert not scan[o + n:at].any()
        assert int(s["first_mcu"]) == mcu
        mcu += int(s["mcu_count"])
    assert at == len(scan) and mcu == mcus


def test_the_restart_fixture_gives_four_segments_of_three_mcus(hp):
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(_blob("c420_64x48_rst3"))
    assert rc == 0, msg
    assert [(int(s["first_mcu"]), int(s["mcu_count"])) for s in segs] == [(0, 3), (3, 3), (6, 3), (9, 3)]


@pytest.mark.parametrize("name", ["c420_53x37_q75", "c420_53x37_opt", "grey_40x24", "c444_53x37_q90"])
def test_the_tables_decode_every_code_of_the_files_dht(hp, name):
    data = _blob(name)
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
    assert rc == 0, msg
    dht, sel = R.dht_tables(data), R.scan_selectors(data)
    T = R._tables(tables)
    for c, (td, ta) in enumerate(sel):
        for cls, tid in ((0, td), (1, ta)):
            bits, vals = dht[(cls, tid)]
            look_nbits, look_sym, maxcode, valoffset, tvals, nvals = T[c][cls]
            assert nvals == len(vals) and tvals[:nvals] == vals
            for sym, (code, length) in E.huff_codes(bits, vals).items():
                if length <= 9:
                    for fill in (0, (1 << (9 - length)) - 1):
                        k = (code << (9 - length)) | fill
                        assert (look_nbits[k], look_sym[k]) == (length, sym)
                else:
                    assert look_nbits[code >> (length - 9)] == 0
                assert code <= maxcode[length] and tvals[valoffset[length] + code] == sym
                assert all(code >> (length - l) > maxcode[l] for l in range(1, length))


def test_progressive_is_unsupported_and_the_cut_file_is_a_stream_the_emit_flags(hp):
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(_blob("prog_53x37"))
    assert rc == hp.JPEG_UNSUPPORTED and "progressive" in msg
    data = _blob("c420_53x37_q75_cut")
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
    assert rc == 0 and len(segs) == 1                        # prepare takes it: the bytes merely end early
    hrc, _want, info = host_planes(hp, data)
    assert hrc == hp.JPEG_ECORRUPT
    for sb in SUB_BITS:
        out = R.decode(scan, segs, tables, info, sb)
        assert out["converged"] and out["flags"] & R.EXHAUSTED


def test_prepare_sends_irregular_restart_streams_to_the_host(hp):
    data = _blob("c420_64x48_rst3")
    a = R.scan_start(data)
    at = [i for i in range(a, len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(at) == 3

    def put(i, v):
        return data[:i + 1] + bytes([v]) + data[i + 2:]
    out_of_sequence = put(at[1], 0xD3)
    other_marker = put(at[1], 0xFE)
    too_few = data[:at[2]] + b"\xff\xd9"
    too_many = data[:-2] + b"\xff\xd3\x00\x00\xff\xd9"
    for bad in (out_of_sequence, other_marker, too_few, too_many):
        rc, *_ = hp.jpeg_scan_prepare_arrays(bad)
        assert rc == hp.JPEG_HUFF_HOST == 1
    coef = np.zeros(1 << 16, np.int16)
    for bad in (out_of_sequence, other_marker, too_few):     # what the host decoder refuses itself
        assert hp.jpeg_entropy_decode(bad, coef.ctypes.data, coef.size)[0] == hp.JPEG_ECORRUPT


def test_prepare_respects_its_capacities(hp):
    data = _blob("c420_64x48_rst3")
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
    assert rc == 0
    assert hp.jpeg_scan_prepare_arrays(data, seg_capacity=3)[0] == -3                # FDET_EWORKSPACE
    guard = np.full(len(scan) + 64, 0xAB, np.uint8)
    segbuf = np.zeros(4, hp.JPEG_HUFF_SEG_DTYPE)
    tab = np.zeros(1, hp.JPEG_HUFF_TABLES_DTYPE)
    for cap in (0, 1, 15, 16, len(scan) - 16, len(scan) - 1):
        guard[:] = 0xAB
        rc, used, n, msg = hp.jpeg_scan_prepare(data, guard.ctypes.data, cap, segbuf.ctypes.data, 4, tab.ctypes.data)
        assert rc == -3, (cap, rc)
        assert (guard[cap:] == 0xAB).all()
    rc, used, n, msg = hp.jpeg_scan_prepare(data, guard.ctypes.data, len(scan), segbuf.ctypes.data, 4, tab.ctypes.data)
    assert rc == 0 and used == len(scan) and n == 4 and (guard[len(scan):] == 0xAB).all()
    assert np.array_equal(guard[:used], scan)
    for cut in (1, 2, 3, 20, R.scan_start(data) - 1):         # no scan at all: the header parser's own refusals
        assert hp.jpeg_scan_prepare_arrays(data[:cut])[0] in (hp.JPEG_ECORRUPT, -1)


# -------------------------------------------------------------------------------------------------------- restatement
def _check_stream(hp, data, sub_bits, record):
    hrc, want, info = host_planes(hp, data)
    assert hrc == 0
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
    assert rc == 0, msg
    out = R.decode(scan, segs, tables, info, sub_bits)
    record(f"sub_bits {sub_bits}: {out['subs']} subsequences, {out['passes']} passes (cap {out['cap']}), {out['decodes']} decodes")
    assert out["converged"] and out["passes"] <= out["cap"]
    assert out["flags"] == 0
    assert out["coef"].dtype == np.int16 and np.array_equal(out["coef"], want)
    return out


@pytest.mark.parametrize("sub_bits", SUB_BITS)
@pytest.mark.parametrize("name", SUPPORTED)
def test_the_restatement_gives_the_host_decoders_planes(hp, name, sub_bits, capsys):
    with capsys.disabled():
        _check_stream(hp, _blob(name), sub_bits, lambda s: print(f"\n    {name} {s}", end=""))


@pytest.mark.parametrize("sub_bits", SUB_BITS)
@pytest.mark.parametrize("name", sorted(GENERATED))
def test_the_restatement_gives_the_host_decoders_planes_on_generated_streams(hp, name, sub_bits, capsys):
    with capsys.disabled():
        out = _check_stream(hp, generated(name), sub_bits, lambda s: print(f"\n    {name} {s}", end=""))
    if name == "constant" and sub_bits == 1024:
        assert 1800 / out["subs"] > 100                       # hundreds of blocks per subsequence: the scan and the DC sum
    if name == "noise" and sub_bits == 64:
        assert out["subs"] > 3 * 15 * 25 * 3                  # blocks that span several subsequences


def test_the_photograph_converges_in_the_passes_the_design_quotes(hp):
    data = _blob("photo_8")
    _, _, info = host_planes(hp, data)
    rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
    out = R.decode(scan, segs, tables, info, 1024)
    assert out["subs"] == 623 and out["passes"] <= 8


# ------------------------------------------------------------------------------------------------------------ corrupt
def corrupt_streams():
    base = _blob("c420_53x37_q75")
    return [(f"mutation {o}={v:#04x}", b) for o, v, b in R.mutations(base)] + [("cut", _blob("c420_53x37_q75_cut"))]


@pytest.mark.parametrize("sub_bits", (64, 1024))
def test_corrupt_streams_reproduce_the_host_planes_or_are_flagged_where_the_host_refuses(hp, sub_bits):
    outcomes = {"planes": 0, "flagged": 0, "host": 0}
    for label, data in corrupt_streams():
        hrc, want, info = host_planes(hp, data)
        rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
        if rc == hp.JPEG_HUFF_HOST:
            outcomes["host"] += 1
            continue
        assert rc == 0, (label, msg)
        out = R.decode(scan, segs, tables, info, sub_bits)    # no assert of the restatement fires
        assert out["converged"], label
        if out["flags"]:
            assert hrc == hp.JPEG_ECORRUPT, f"{label}: flagged {out['flags']} but the host decoder accepts the stream"
            outcomes["flagged"] += 1
        else:
            assert hrc == 0 and np.array_equal(out["coef"], want), label
            outcomes["planes"] += 1
    assert outcomes["flagged"] >= 1 and sum(outcomes.values()) == 17


@pytest.mark.parametrize("sub_bits", (64, 1024))
def test_corrupt_restart_streams_reproduce_the_host_planes_or_are_flagged_where_the_host_refuses(hp, sub_bits):
    """the same property per segment: the scan, the DC sum and what follows a segment's blocks.  The host decoder refills its
    window once behind an interval's blocks and wants the RSTn there, so more than 64 spare bits are its to refuse."""
    outcomes = {"planes": 0, "flagged": 0, "host": 0}
    seen = {}
    for label, data in R.restart_corruptions(_blob("c420_64x48_rst3")):
        hrc, want, info = host_planes(hp, data)
        rc, scan, segs, tables, msg = hp.jpeg_scan_prepare_arrays(data)
        if rc == hp.JPEG_HUFF_HOST:
            outcomes["host"] += 1
            continue
        assert rc == 0, (label, msg)
        out = R.decode(scan, segs, tables, info, sub_bits)
        assert out["converged"], label
        seen[label] = out["flags"]
        if out["flags"]:
            assert hrc == hp.JPEG_ECORRUPT, f"{label}: flagged {out['flags']} but the host decoder accepts the stream"
            outcomes["flagged"] += 1
        else:
            assert hrc == 0 and np.array_equal(out["coef"], want), f"{label}: host code {hrc}"
            outcomes["planes"] += 1
    assert seen["24 spare bytes 0x55"] & R.TRAILING and seen["1 spare bytes 0x55"] == 0 and seen["7 spare bytes 0x00"] == 0
    assert outcomes["flagged"] >= 3 and outcomes["planes"] >= 3 and sum(outcomes.values()) == 26, outcomes
    print(outcomes)


# ------------------------------------------------------------------------------------------------------------ surface
def test_the_decoder_refuses_unknown_huffman_settings():
    import fdet_amd  # noqa: F401
    from fdet_amd.datasets.jpeg import DeviceJpegDecoder
    from fdet_amd.datasets.WIDERFace.annotations import bank_from_files
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="huffman"):
            DeviceJpegDecoder("cpu", huffman=bad)
    for bad in (0, 32, 96 + 16, 1000):
        with pytest.raises(ValueError, match="sub_bits"):
            DeviceJpegDecoder("cpu", huffman="device", sub_bits=bad)
    with pytest.raises(ValueError, match="max_sync_passes"):
        DeviceJpegDecoder("cpu", huffman="device", max_sync_passes=0)
    dec = DeviceJpegDecoder("cpu")
    assert dec.huffman == "host" and dec.huffman_fallbacks == [] and dec.sync_passes == 0
    with pytest.raises(ValueError, match="huffman"):
        bank_from_files([], "cpu", decoder="device", huffman="gpu")
    with pytest.raises(ValueError, match="needs decoder='device'"):
        bank_from_files([], "cpu", decoder="pil", huffman="device")


@pytest.mark.parametrize("script", ["detect_images", "run_validation_epoch", "train_model"])
def test_the_huffman_flag_needs_the_device_decoder(script, capsys):
    import importlib
    import fdet_amd  # noqa: F401
    mod = importlib.import_module(f"fdet_amd.{script}")
    argv = {"detect_images": ["--images", "nowhere", "--out", "nowhere.txt"], "run_validation_epoch": [], "train_model": []}[script]
    with pytest.raises(SystemExit) as e:
        mod.main(argv + ["--device-jpeg-huffman"])
    assert e.value.code == 2
    assert "--device-jpeg-huffman needs --device-jpeg" in capsys.readouterr().err
