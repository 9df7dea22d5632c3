"""The pooled forward's two forms (csrc/fdet_conv3x3_ps.hip: one workgroup per CU with two chunk buffers; WG2 = two
workgroups per CU with one buffer each) compute the same bits.  FDET_PS_POOL_WG2 is read once per process, so each form
runs in a child of its own (tests/ps_pool_wg2_worker.py, two children for the whole module); the CPU reference of every
case is computed once here, from the PS-rounded inputs the child saved, with the bound of tests/test_gpu_ps.py."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ps_pool_wg2_worker import SENTINEL, SHAPES, case_inputs   # noqa: E402

CASES = [(s, t) for s in SHAPES for t in (True, False)]
IDS = [f"{'x'.join(map(str, s))}-{'train' if t else 'eval'}" for s, t in CASES]


def close(a, b, tol=1e-4):   # tests/test_gpu_ps.py
    a = a.cpu().double(); b = b.cpu().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"max err {err} vs scale {scale}"


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("ps_pool_wg2")
    out = {}
    for v in ("0", "1"):
        path = str(d / f"wg2_{v}.pt")
        env = dict(os.environ, FDET_PS_POOL_WG2=v)
        r = subprocess.run([sys.executable, os.path.join(HERE, "ps_pool_wg2_worker.py"), path], env=env, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, f"FDET_PS_POOL_WG2={v}: worker failed\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        out[v] = torch.load(path, weights_only=False)
        assert out[v]["wg2"] == v
    return out


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(case, got):
        if case not in cache:
            shape, train = case
            N, C, H, W = shape
            _, _, w, b, scale = case_inputs(shape, train)
            c = F.leaky_relu(F.conv2d(got["xr"], w, b, padding=1), 0.2)
            u = c * (scale[:, :, None, None] if train else 1.0) + got["sr"]
            cache[case] = (c, u, F.max_pool2d(u, 2))
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_new_form_equals_present_form_bit_for_bit(runs, case):
    a, b = runs["0"]["cases"][case], runs["1"]["cases"][case]
    for k in ("pool_f", "pool_ps_buf", "route", "only_f", "only_ps_buf"):
        if a.get(k) is None:
            assert b.get(k) is None
            continue
        assert bits_equal(a[k], b[k]), f"{k} differs between FDET_PS_POOL_WG2=0 and 1"
    assert bits_equal(a["xr"], b["xr"]) and bits_equal(a["sr"], b["sr"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("form", ["0", "1"])
def test_against_cpu_reference_and_buffer_hygiene(runs, refs, case, form):
    shape, train = case
    N, C, H, W = shape
    got = runs[form]["cases"][case]
    c, u, ref = refs(case, got)
    # every output element was written (the fp32 output started as NaN, the routing bytes as a sentinel no byte can equal:
    # bits 6-7 of a routing byte are zero)
    close(got["pool_f"], ref)
    close(got["only_f"], ref)
    assert bits_equal(got["only_f"], got["pool_f"])
    if got["pool_ps"] is not None:
        close(got["pool_ps"], ref)
        assert bits_equal(got["only_ps_buf"], got["pool_ps_buf"])
        words = got["pool_ps_buf"].view(torch.int16)
        assert not bool(((words != 0) & ~got["real_words"]).any()), "a halo / guard slot of pool_ps is no longer zero"
    assert got["repeat_equal"], "the second run on the same buffers differs from the first"
    if not train:
        assert got["route"] is None
        return
    route = got["route"]
    assert not bool((route == SENTINEL).any()) and not bool((route & 0xC0).any())
    if W > 62:
        return      # strips: routing bytes are per strip; compared bit for bit with the present form above
    rt = route.permute(0, 1, 4, 2, 3).reshape(N, C, H // 2, W // 2).int()
    win = F.unfold(u.reshape(N * C, 1, H, W), 2, stride=2).reshape(N, C, 4, H // 2, W // 2)
    top2 = win.topk(2, dim=2).values
    clear = (top2[:, :, 0] - top2[:, :, 1]) > 1e-3
    assert torch.equal(((rt >> 4) & 3)[clear], win.argmax(dim=2).int()[clear])
    cw = F.unfold(c.reshape(N * C, 1, H, W), 2, stride=2).reshape(N, C, 4, H // 2, W // 2)
    for k in range(4):
        sure = cw[:, :, k].abs() > 1e-3
        assert torch.equal(((rt >> k) & 1)[sure], (cw[:, :, k] > 0).int()[sure])


def test_two_training_steps_give_identical_parameters(runs):
    a, b = runs["0"]["train"], runs["1"]["train"]
    assert a["losses"] == b["losses"]
    assert a["params"].keys() == b["params"].keys()
    for k in a["params"]:
        assert bits_equal(a["params"][k], b["params"][k]), k
