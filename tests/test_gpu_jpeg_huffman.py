"""The device Huffman decoder on the GPU (csrc/fdet_jpeg_huff.hip fdet_jpeg_huffman_sync / fdet_jpeg_huffman_emit, driven by
fdet_amd/datasets/jpeg.py with huffman="device"): its coefficient planes against the host decoder fdet_jpeg_entropy_decode,
`torch.equal` everywhere.  tests/test_jpeg_huffman_host.py shows on the CPU that the Python restatement of the kernels' rules
reaches the same planes for the same streams, and that the corrupt streams used here leave no index out of its range."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import jpeg_enc_cpu_ref as E
import jpeg_huff_cpu_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
JPEG_DIR = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(JPEG_DIR, "manifest.json")))
SUPPORTED = [e["file"][:-4] for e in MANIFEST if e["kind"] == "supported"]
SUB_BITS = (64, 128, 1024)
GENERATED = {"constant": ("constant", 320, 240, 75, 2), "noise": ("noise", 200, 120, 95, 0), "saturated": ("saturated", 96, 64, 50, 1)}


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    from fdet_amd.datasets import augment, jpeg
    return augment, jpeg, hotpath


def _blob(name) -> bytes:
    with open(os.path.join(JPEG_DIR, name + ".jpg"), "rb") as f:
        return f.read()


def _host_planes(hp, data) -> torch.Tensor:
    rc, info, msg = hp.jpeg_info(data)
    assert rc == 0, msg
    want = np.zeros(int(info["coef_count"]), np.int16)
    rc, msg = hp.jpeg_entropy_decode(data, want.ctypes.data, want.size)
    assert rc == 0, msg
    return torch.from_numpy(want)


@pytest.fixture(scope="module")
def streams():
    """name -> (file bytes, the host decoder's planes): computed once, shared, never modified."""
    _A, _J, hp = _mods()
    out = {n: _blob(n) for n in SUPPORTED}
    for name, (kind, w, h, q, sub) in GENERATED.items():
        out[name] = E.encode(E.source(kind, w, h), q, sub)
    return {n: (b, _host_planes(hp, b)) for n, b in out.items()}


@pytest.fixture(scope="module")
def goldens():
    z = np.load(os.path.join(HERE, "golden", "g21_jpeg.npz"))
    return {k: z[k] for k in z.files}


def _check(dec, streams, names):
    planes, todo = dec.coefficient_planes([streams[n][0] for n in names])
    assert todo == [], [names[k] for k in todo]
    for n, got in zip(names, planes):
        want = streams[n][1]
        assert got.dtype == torch.int16 and got.numel() == want.numel()
        diff = int((got.cpu() != want).sum())
        assert diff == 0, f"{n} at sub_bits {dec.sub_bits}: {diff} of {want.numel()} coefficients differ"
        assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------- kernel against host decoder
@pytest.mark.parametrize("sub_bits", SUB_BITS)
def test_every_supported_fixture_in_one_launch_gives_the_host_decoders_planes(streams, sub_bits):
    """mixed samplings and grey, a one-subsequence image, restart segments, tables of its own, 695 subsequences of noise at 64
    bits (several workgroups, codes longer than the lookahead, blocks over three subsequences), 623 of a photograph at 1024"""
    _A, J, _hp = _mods()
    dec = J.DeviceJpegDecoder("cuda", huffman="device", sub_bits=sub_bits)
    _check(dec, streams, SUPPORTED)
    assert dec.sync_passes >= 2 and dec.scan_bytes > 0
    print(f"sub_bits {sub_bits}: {dec.sync_passes} passes")


@pytest.mark.parametrize("sub_bits", SUB_BITS)
def test_every_supported_fixture_alone_gives_the_host_decoders_planes(streams, sub_bits):
    _A, J, _hp = _mods()
    dec = J.DeviceJpegDecoder("cuda", huffman="device", sub_bits=sub_bits)
    for n in SUPPORTED:
        _check(dec, streams, [n])
        if n == "c420_1x1":
            assert dec.sync_passes == 2                      # one subsequence: one pass decodes it, one sees nothing change


@pytest.mark.parametrize("sub_bits", SUB_BITS)
def test_generated_streams_give_the_host_decoders_planes(streams, sub_bits):
    """constant: 1800 six-bit blocks, about 170 per subsequence at 1024 bits, pin the block-count scan and the DC prefix sum;
    noise: blocks that span several subsequences; saturated: 4:2:2"""
    _A, J, _hp = _mods()
    dec = J.DeviceJpegDecoder("cuda", huffman="device", sub_bits=sub_bits)
    _check(dec, streams, sorted(GENERATED))
    _check(dec, streams, ["constant"])


# ------------------------------------------------------------------------------------------------------------ end to end
def _same(bank, want):
    assert bank.table.dtype == want.table.dtype and np.array_equal(bank.table, want.table)
    assert bank.data.numel() == want.data.numel() and torch.equal(bank.data, want.data)


def test_the_decoder_gives_the_same_bank_with_either_huffman_setting(goldens):
    pytest.importorskip("PIL.Image")
    A, J, _hp = _mods()
    order = SUPPORTED[:3] + ["prog_53x37"] + SUPPORTED[3:]
    blobs = [_blob(n) for n in order]                        # (a non-JPEG entry goes by path in the next test)
    dev = J.DeviceJpegDecoder("cuda", huffman="device")
    host = J.DeviceJpegDecoder("cuda")
    for lead in (0, 64):
        got = dev.decode_bytes(blobs, lead_bytes=lead)
        _same(got, host.decode_bytes(blobs, lead_bytes=lead))
        _same(got, A.DeviceImageBank.from_arrays([goldens[n] for n in order], "cuda", lead_bytes=lead))
        assert dev.fallbacks == host.fallbacks == [3] and dev.huffman_fallbacks == [] and dev.chunks == 1
        assert dev.sync_passes >= 2
    ptrs = {k: (v.data_ptr(), v.numel()) for k, v in dev._bufs.items()}
    _same(dev.decode_bytes(blobs), host.decode_bytes(blobs))  # a second call reuses the buffers
    assert ptrs == {k: (v.data_ptr(), v.numel()) for k, v in dev._bufs.items()}


def test_a_non_jpeg_file_and_small_chunks_go_the_same_way(goldens, tmp_path):
    pytest.importorskip("PIL.Image")
    A, J, _hp = _mods()
    from PIL import Image
    Image.fromarray(goldens["c420_17x9"]).save(tmp_path / "a.png")
    paths = [tmp_path / "a.png"] + [os.path.join(JPEG_DIR, n + ".jpg") for n in SUPPORTED]
    dev = J.DeviceJpegDecoder("cuda", huffman="device", workers=4, chunk_bytes=64 << 10)
    bank = dev.decode_files(paths)
    assert dev.fallbacks == [0] and dev.huffman_fallbacks == [] and dev.chunks >= 3
    _same(bank, A.DeviceImageBank.from_arrays([goldens["c420_17x9"]] + [goldens[n] for n in SUPPORTED], "cuda"))
    from fdet_amd.datasets.WIDERFace.annotations import bank_from_files
    _same(bank_from_files(paths, "cuda", decoder="device", huffman="device"), bank)


def test_a_pass_cap_of_one_sends_every_image_to_the_host_and_gives_the_same_bank(goldens):
    A, J, _hp = _mods()
    dec = J.DeviceJpegDecoder("cuda", huffman="device", max_sync_passes=1)
    bank = dec.decode_bytes([_blob(n) for n in SUPPORTED])
    assert dec.sync_passes == 1 and dec.huffman_fallbacks == list(range(len(SUPPORTED))) and dec.fallbacks == []
    _same(bank, A.DeviceImageBank.from_arrays([goldens[n] for n in SUPPORTED], "cuda"))


def test_an_image_prepare_sends_to_the_host_is_decoded_there_into_the_same_planes(goldens):
    """irregular restart markers: one stream the host decoder accepts (a restart marker too many), one it refuses"""
    A, J, _hp = _mods()
    data = _blob("c420_64x48_rst3")
    at = [i for i in range(R.scan_start(data), len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    too_many = data[:-2] + b"\xff\xd3\x00\x00\xff\xd9"
    out_of_sequence = data[:at[1] + 1] + b"\xd3" + data[at[1] + 2:]
    names = ["c420_53x37_q75", "c420_64x48_rst3", "grey_40x24"]
    blobs = [_blob(names[0]), too_many, _blob(names[2])]
    dev, host = J.DeviceJpegDecoder("cuda", huffman="device"), J.DeviceJpegDecoder("cuda")
    bank = dev.decode_bytes(blobs)
    assert dev.huffman_fallbacks == [1] and dev.fallbacks == []
    _same(bank, host.decode_bytes(blobs))
    _same(bank, A.DeviceImageBank.from_arrays([goldens[n] for n in names], "cuda"))
    blobs[1] = out_of_sequence
    a, b = _outcome(dev, blobs), _outcome(host, blobs)
    assert a[0] == b[0] == "error" and a[1] == b[1] and "RST" in a[1]


# ---------------------------------------------------------------------------------------------------------------- errors
def _outcome(dec, blobs):
    from fdet_amd import FdetError
    try:
        return "bank", dec.decode_bytes(blobs).data.cpu()
    except FdetError as e:
        return "error", str(e)


def test_the_cut_file_raises_the_same_error_under_both_settings():
    _A, J, _hp = _mods()
    blobs = [_blob(SUPPORTED[0]), _blob("c420_53x37_q75_cut"), _blob(SUPPORTED[1])]
    a = _outcome(J.DeviceJpegDecoder("cuda", huffman="device"), blobs)
    b = _outcome(J.DeviceJpegDecoder("cuda"), blobs)
    assert a[0] == b[0] == "error" and a[1] == b[1] and "image 1" in a[1]


def test_the_sixteen_mutations_give_the_host_paths_planes_or_its_error():
    """the flags at work, not a stress test: tests/test_jpeg_huffman_host.py runs the restatement, which asserts every
    index, over these very streams"""
    _A, J, _hp = _mods()
    dev, host = J.DeviceJpegDecoder("cuda", huffman="device"), J.DeviceJpegDecoder("cuda")
    good = _blob(SUPPORTED[0])
    kinds = set()
    for o, v, data in R.mutations(_blob("c420_53x37_q75")):
        a, b = _outcome(dev, [good, data]), _outcome(host, [good, data])
        assert a[0] == b[0], (o, v, a, b)
        assert torch.equal(a[1], b[1]) if a[0] == "bank" else a[1] == b[1], (o, v)
        kinds.add(a[0])
    assert kinds == {"bank", "error"}


def test_corrupt_restart_streams_give_the_host_paths_planes_or_its_error():
    """spare bytes in front of a restart marker (the host decoder accepts up to 64 spare bits and refuses more) and 16
    mutations of the restart fixture: segments under corruption.  tests/test_jpeg_huffman_host.py runs the restatement,
    which asserts every index, over these very streams."""
    _A, J, _hp = _mods()
    dev, host = J.DeviceJpegDecoder("cuda", huffman="device"), J.DeviceJpegDecoder("cuda")
    good = _blob(SUPPORTED[0])
    kinds = {}
    for label, data in R.restart_corruptions(_blob("c420_64x48_rst3")):
        a, b = _outcome(dev, [good, data]), _outcome(host, [good, data])
        assert a[0] == b[0], (label, a, b)
        assert torch.equal(a[1], b[1]) if a[0] == "bank" else a[1] == b[1], label
        kinds[label] = a[0]
        if a[0] == "bank":
            assert dev.huffman_fallbacks == [], label       # the device path vouched for what the host accepts
    assert kinds["24 spare bytes 0x55"] == "error" and kinds["1 spare bytes 0x55"] == "bank"
    assert set(kinds.values()) == {"bank", "error"}


# ------------------------------------------------------------------------------------------------------- C-ABI refusals
def test_the_entry_points_refuse_bad_arguments_before_they_write():
    _A, J, hp = _mods()
    from fdet_amd import FdetError
    names = ["c420_64x48_rst3", "grey_40x24"]
    blobs = [_blob(n) for n in names]
    dec = J.DeviceJpegDecoder("cuda", huffman="device", sub_bits=128)
    chunk = [(i, hp.jpeg_info(b)[1]) for i, b in enumerate(blobs)]
    descs, spans, used, _ws = dec._describe(chunk, np.zeros(2, dtype=J.IMAGE_DTYPE))
    with ThreadPoolExecutor(2) as pool:
        d_scan, d_tab, d_images, images, d_segs, segs, n_subs, host = dec.huffman_stage(pool, blobs, names, chunk, descs)
    assert host == set() and len(segs) == 5
    state = torch.full((3 * n_subs,), 7, dtype=torch.int64, device="cuda")
    changed = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    first = torch.full((n_subs,), 7, dtype=torch.int32, device="cuda")
    coef = torch.full((used,), 7, dtype=torch.int16, device="cuda")
    flags = torch.full((2,), 7, dtype=torch.int32, device="cuda")

    def both(match, images=images, segs=segs, sub_bits=128, scan=d_scan, coef=coef, only_emit=False):
        if not only_emit:
            with pytest.raises(FdetError, match=match):
                hp.jpeg_huffman_sync(scan, d_tab, d_images, images, d_segs, segs, sub_bits, state, changed)
        with pytest.raises(FdetError, match=match):
            hp.jpeg_huffman_emit(scan, d_tab, d_images, images, d_segs, segs, sub_bits, state, first, coef, flags)

    for sb in (32, 48, 100, 0, -64):
        both("sub_bits", sub_bits=sb)
    both("subsequence range", sub_bits=256)                  # a layout made for another size
    s = segs.copy()
    s["byte_offset"][4] = d_scan.numel()
    both("outside the scan buffer", segs=s)
    s = segs.copy()
    s["byte_len"][4] = d_scan.numel() - int(s["byte_offset"][4]) + 1
    both("outside the scan buffer", segs=s)
    s = segs.copy()
    s["byte_offset"][1] += 8
    both("misaligned", segs=s)
    s = segs.copy()
    s["first_mcu"][2] += 1
    both("MCU range", segs=s)
    both("16-byte aligned", scan=d_scan[4:])
    im = images.copy()
    im["coef_offset"][1][0] = used - 64
    both("past the", images=im, only_emit=True)
    im = images.copy()
    im["coef_offset"][0][1] += 4
    both("misaligned", images=im, only_emit=True)
    both("past the", coef=coef[:used - 8], only_emit=True)
    im = images.copy()
    im["hs"][0] = 4
    both("supported set", images=im)
    torch.cuda.synchronize()
    for t in (state, changed, first, coef, flags):
        assert bool((t == 7).all())                          # nothing was written
    # and the same arguments, unspoilt, decode
    state.zero_()
    for _ in range(int(segs["sub_count"].max()) + 1):
        changed.zero_()
        hp.jpeg_huffman_sync(d_scan, d_tab, d_images, images, d_segs, segs, 128, state, changed)
    flags.zero_()
    hp.jpeg_huffman_emit(d_scan, d_tab, d_images, images, d_segs, segs, 128, state, first, coef, flags)
    torch.cuda.synchronize()
    assert not changed.any() and not flags.any()
    for (a, c), b in zip(spans, blobs):
        assert torch.equal(coef[a:a + c].cpu(), _host_planes(hp, b))
