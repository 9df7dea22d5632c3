"""Batch-size-dependent kernel choices of the engines against the library's own plan checks (CPU only).

The engines pick kernels per batch (ConvStack.plan(N): the PS blocks and chains, the stem decisions and the PS weight
gradient's workspace plan), and the C entry points refuse shapes whose 32-bit offsets a batch would overflow.  For every
deployed geometry and a sweep of batch sizes around each switch, every stage the engine routes a training step (and the
uint8 frame path) to must be accepted by the side-effect-free query of that entry point -- the same check function the entry
point runs before it launches anything.  Nothing here launches a kernel: the queries only read sizes, and the engines are
built without a device (wg_num_cus() falls back to the MI355X's 256 CUs)."""
import json
import os
import subprocess
import sys

import pytest

import fdet_amd  # noqa: F401
from fdet_amd import hotpath as hp
from fdet_amd import ps as psm
from fdet_amd.models.PoolResnet import PoolResnet
from fdet_amd.models.Resnet import Resnet
from fdet_amd.models.SSD import SSD

SWEEP = (1, 2, 7, 64, 256, 512)


def _around(*ts):
    return sorted({n for t in ts for n in (t - 1, t, t + 1) if n >= 1})


def conv_stack_stages(eng, N):
    """[(stage, accepted)] of one training step (forward + backward) at batch N: every stage of the engine's plan of the pass
    against the side-effect-free query of the entry points it is routed to."""
    plan = eng.plan(N)
    g = eng.geo
    F_ = g.filters
    out = []
    if plan.stem_ps:
        out.append(("stem_fwd_ps", hp.stem_fwd_ps_ok(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p, p16=plan.p16)))
        if eng.u8_frames_ok():
            out.append(("stem_fwd_ps_u8", hp.stem_fwd_ps_ok(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p, p16=plan.p16,
                                                            u8=True)))
    for st in plan.stages:
        k, hk, run = st.k, st.hk, st.run
        if st.kind == "ps_pool":
            out.append((f"block{k}@{hk} conv_ps", psm.conv3x3_ps_ok(N, F_, F_, hk, hk, 0)))
            out.append((f"block{k}@{hk} conv_ps_pool", psm.conv3x3_ps_ok(N, F_, F_, hk, hk, 2 if st.out_ps else 1)))
            out.append((f"block{k}@{hk} wgrad_ps", psm.conv3x3_wgrad_ps_ws_bytes(1, N, F_, hk, hk) > 0))
        elif st.kind in ("ps_chain", "chain"):
            ps = st.kind == "ps_chain"
            assert st.wgrad == ("ps" if ps else "batched")
            out.append((f"chain{k}@{hk} ps={ps}", hp.block_chain_ok(N, F_, hk, hk, ps)))
            if ps:
                out.append((f"chain{k}@{hk} wgrad_ps", psm.conv3x3_wgrad_ps_ws_bytes(min(16, 2 * run), N, F_, hk, hk) > 0))
            else:
                out.append((f"chain{k}@{hk} wgrad_batched", hp.conv3x3_wgrad_batched_ws_bytes(min(16, 2 * run), N, F_, F_, hk, hk) > 0))
        else:
            if st.fused_pool:
                out.append((f"block{k}@{hk} fwd_pool", hp.pool_fusion_supported(F_, F_, hk, hk, N)))
            if st.wgrad == "batched":
                out.append((f"block{k}@{hk} wgrad_batched", hp.conv3x3_wgrad_batched_ws_bytes(2, N, F_, F_, hk, hk) > 0))
            else:
                out.append((f"block{k}@{hk} wgrad", hp.conv3x3_wgrad_ws_bytes(N, F_, F_, hk, hk) > 0))
    x3, p16 = plan.stem_wgrad
    if x3:
        out.append((f"stem_wgrad p16={p16}", hp.stem_wgrad_x3_ok(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p, p16=p16)))
    out.append(("stem_ws", hp.stem_ws_bytes(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p) > 0))
    return out


def _refused(stages):
    return [s for s, ok in stages if not ok]


GEOMETRIES = {
    # (constructor, precision, batch-size switches of the host's plan functions)
    "poolresnet64_480": (lambda: PoolResnet(64, (3, 480, 480), 10), "bf16x3", (777, 2331)),
    "poolresnet64_480_p16": (lambda: PoolResnet(64, (3, 480, 480), 10), "bf16", (777, 2331)),
    "poolresnet128_480": (lambda: PoolResnet(128, (3, 480, 480), 10), "bf16x3", (777, 1166)),
    "poolresnet128_480_p16": (lambda: PoolResnet(128, (3, 480, 480), 10), "bf16", (777, 1166)),
    "resnet64_640": (lambda: Resnet(64, (3, 640, 640), 20), "bf16x3", (82, 328, 1311)),
}


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_every_stage_the_engine_picks_is_accepted_by_its_kernel(geo):
    ctor, prec, switches = GEOMETRIES[geo]
    eng = ctor().engine
    eng.set_precision(prec)
    bad = {}
    for N in sorted(set(SWEEP) | set(_around(*switches)) | {800, 2330, 2400}):
        r = _refused(conv_stack_stages(eng, N))
        if r:
            bad[N] = r
    assert not bad, f"{geo}: the engine routes these batch sizes to kernels that refuse them: {bad}"


def test_switches_sit_where_the_gpu_tests_expect_them():
    """tests/test_gpu_batch_sizes.py puts a batch and its halves on the two sides of these switches."""
    e = PoolResnet(64, (3, 480, 480), 10).engine
    for N, want in ((1200, True), (2330, True), (2331, False), (2400, False)):
        p = e.plan(N)
        assert (p.stages[0].kind == "ps_pool") == want and p.stem_ps == want, N
    r = Resnet(64, (3, 640, 640), 20).engine
    for N, want in ((42, True), (81, True), (82, False), (84, False)):
        p = r.plan(N)
        assert (p.stages[0].kind == "ps_pool") == want and p.stages[1].kind == "ps_pool", N


@pytest.mark.parametrize("N", sorted(set(SWEEP) | {776, 777, 800, 1165, 1166, 2330, 2331}))
def test_precision16_keeps_its_one_pass_stem_weight_gradient_at_every_batch(N):
    """precision16 must not switch the PoolResnet stem's weight gradient to bf16x3 when the batch grows."""
    for F_ in (64, 128):
        eng = PoolResnet(F_, (3, 480, 480), 10).engine
        eng.set_precision("bf16")
        assert eng.plan(N).stem_wgrad == (True, True), (F_, N)
        assert hp.stem_wgrad_x3_ok(N, 3, F_, 480, 480, 10, 8, 2, p16=True), (F_, N)


@pytest.mark.parametrize("N", sorted(set(SWEEP) | {777, 2330}))
def test_ssd_stages_are_accepted(N):
    """SSD F=16 at 480^2 (ssdstack.py): the batched / single weight-gradient plans and the stem's matrix-core weight gradient
    exist for every conv at every batch size the sweep covers."""
    model = SSD(filters=16, input_shape=(3, 480, 480))
    eng = model.engine
    hk = 480 // 2
    bad = []
    for name, ci, co, pool, head in eng.specs:
        for cin in (ci, co):
            if hp.conv3x3_wgrad_batched_ws_bytes(2, N, cin, co, hk, hk) <= 0 and hp.conv3x3_wgrad_ws_bytes(N, cin, co, hk, hk) <= 0:
                bad.append((name, cin, co, hk))
        hk = hk // 2 if pool else hk
    assert hp.stem_k3_wgrad_x3_supported(3, 16, 480, 480, 3, 2, 1)
    assert hp.stem_wgrad_x3_ok(N, 3, 16, 480, 480, 3, 2, 1) and hp.stem_wgrad_x3_ok(N, 3, 16, 480, 480, 3, 2, 1, p16=True)
    assert hp.stem_ws_bytes(N, 3, 16, 480, 480, 3, 2, 1) > 0
    assert not bad, bad


def test_stem_workspace_grows_with_the_chunks_of_a_large_batch():
    """Batches beyond one launch of the pipelined stem kernels: the weight-gradient workspace holds the partials of every
    chunk (one slab per workgroup, 256 per chunk), below that size it is what one launch needs."""
    per_slab = 64 * 321 * 4
    assert hp.stem_ws_bytes(776, 3, 64, 480, 480, 10, 8, 2) >= 256 * per_slab
    assert hp.stem_ws_bytes(777, 3, 64, 480, 480, 10, 8, 2) >= (256 + 60) * per_slab        # 776 images + 1 (60 rows)
    assert hp.stem_ws_bytes(2400, 3, 64, 480, 480, 10, 8, 2) >= 4 * 256 * per_slab
    assert hp.stem_ws_bytes(1, 3, 64, 480, 480, 10, 8, 2) >= 60 * per_slab


def test_queries_refuse_what_the_kernels_cannot_run():
    """The queries are not constant: shapes without a plan are refused."""
    assert not hp.stem_fwd_ps_ok(4, 3, 32, 480, 480, 10, 8, 2)              # the PoolResnet PS stem is built for 64 channels
    assert not hp.stem_fwd_ps_ok(0, 3, 64, 480, 480, 10, 8, 2)
    assert not hp.stem_wgrad_x3_ok(4, 3, 64, 352, 352, 10, 8, 2, p16=True)  # Wo = 44: no one-pass kernel
    assert hp.stem_wgrad_x3_ok(4, 3, 64, 352, 352, 10, 8, 2)                # ... the staged bf16x3 kernel covers it
    assert not psm.conv3x3_ps_ok(2331, 64, 64, 60, 60, 1)                   # pooled block: 32-bit offsets of fp32 tensors
    assert psm.conv3x3_ps_ok(2330, 64, 64, 60, 60, 1)
    assert not psm.conv3x3_ps_ok(4, 64, 64, 60, 60 + 1, 1)                  # odd map: no pooled block
    assert not hp.block_chain_ok(4, 64, 20, 20)                             # 20 x 24 positions > 256
    assert hp.block_chain_ok(4, 64, 15, 15, True) and hp.block_chain_ok(4, 64, 15, 15, False)
    assert not hp.block_chain_ok(150000, 64, 15, 15, False)


def test_weight_gradient_plan_ignores_the_retired_pack_switch():
    """FDET_WGRAD_PACK selected a packed narrow-row staging that is gone: in a child process with it set (the library reads
    its switches once per process), the plans of narrow maps (4..16 columns, where it applied) report pack == 0 and equal
    the plans of this process, whose environment is the child's without the switch."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shapes = [(2, 64, 64, 15, W) for W in (15, 4, 16)]
    code = ("import sys, json; sys.path.insert(0, sys.argv[1]); import fdet_amd; from fdet_amd import hotpath as hp; "
            "print(json.dumps([hp.conv3x3_wgrad_x3_plan(*s) for s in json.loads(sys.argv[2])]))")
    assert "FDET_WGRAD_PACK" not in os.environ, "this test needs a process started without the retired switch"
    r = subprocess.run([sys.executable, "-c", code, root, json.dumps(shapes)], env=dict(os.environ, FDET_WGRAD_PACK="1"),
                       capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    with_switch = json.loads(r.stdout.strip().splitlines()[-1])
    assert [p["pack"] for p in with_switch] == [0, 0, 0] and all(p["ok"] for p in with_switch), with_switch
    assert with_switch == [hp.conv3x3_wgrad_x3_plan(*s) for s in shapes]
