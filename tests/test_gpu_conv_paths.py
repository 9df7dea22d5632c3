"""Every dispatch path of the bf16x3 / precision16 3x3 convolution (csrc/fdet_conv3x3_x3*.hip, fdet_wgrad3x3_x3.hip)
against a float64 CPU reference of the same operation.

The runners choose among three kernel families (aligned-band small-tile "al", small-tile "sb", general persistent
"general"), and inside a family among vector widths (from W % 4 and the pointers' alignment), MT (Cout padded
to 32, CoP % 64), epilogue modes, column segmentation and the precision.  Each case below states the route it must reach
(`expected_route`, a restatement of those rules) and checks it through fdet_conv3x3_x3_last_route /
fdet_conv3x3_wgrad_bf16x3_plan, so a shape list that drifts off its branch fails instead of testing nothing.  Tile sizes
(NW / NT / R) are a cost model's choice and are not asserted; where the cost model also picks MT (sb) or decides
whether rows are segmented (general), any of the candidates the rules allow is accepted.

Bounds: bf16x3 max|got - ref| <= 1e-4 * max(1, max|ref|); precision16 reference on bf16-rounded operands, outputs
within close_bf16's bound (one bf16 rounding of the stored value), weight gradients within 1e-4 of the scale.
Outputs start as NaN inside a sentinel band that must survive; every launch runs twice and must repeat bit for bit.

The environment switches the runners read once per process (FDET_CONV_KERNEL, FDET_SB_AL, FDET_WGRAD_PIPE,
FDET_WGRAD_PK4) are covered by re-running subsets of this file in
child processes (test_switch_groups); FDET_CONV_TILE is read at every call and covered in-process."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_gpu_p16 import bf, close_bf16      # precision16 rounding and its output bound, shared with those tests

pytestmark = pytest.mark.gpu

EPI_GENERIC, EPI_FWD_FULL, EPI_FWD_BOTH, EPI_FWD_OUT, EPI_DGRAD_ACT, EPI_DGRAD_ADD, EPI_FWD_POOL, EPI_DGRAD_ADDPOOL = range(8)
SLOPE = 0.2
GUARD = 64                      # sentinel floats before and after every output (256 bytes: keeps the base alignment)
SENTINEL = -7.25e5


@pytest.fixture(scope="module")
def hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def close(got, ref, tol=1e-4, what=""):
    got = got.cpu().double(); ref = ref.cpu().double()
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


# ----------------------------------------------------------------------------------------------------------------------
# expected routes: a restatement of run_x3 / fdet_x3_sb_pool_run / fdet_x3_sb_run / plan_x3
# ----------------------------------------------------------------------------------------------------------------------
def _aligned(p, b):
    return p is None or p % b == 0


def _vw(W, x):
    """Vector width of the sb / al runners: from W and the input pointer only."""
    return 4 if W % 4 == 0 and _aligned(x, 16) else (2 if W % 2 == 0 and _aligned(x, 8) else 1)


def _nbs_small(vw):          # nbs_sb: staging slots per thread
    return 1 if vw == 4 else (2 if vw == 2 else 3)


def _nbs_general(nw, nt, vw):
    return (2 * (nw * nt * 32 + 184) // vw + nw * 64 - 1) // (nw * 64)


def _plain_mode(dgrad, p):
    """EPI_* of the pointer set, or None when no fused mode matches (p: name -> data_ptr or None)."""
    if not dgrad and p["bias"]:
        if p["y_full"] and not p["y_out"]:
            return EPI_FWD_FULL
        if p["y_full"] and p["y_out"] and p["skip"] and p["scale"]:
            return EPI_FWD_BOTH
        if not p["y_full"] and p["y_out"] and p["skip"] and not p["scale"]:
            return EPI_FWD_OUT
    elif dgrad:
        if p["act"] and not p["skip"]:
            return EPI_DGRAD_ACT
        if not p["act"] and p["skip"]:
            return EPI_DGRAD_ADD
    return None


def _route_al(N, ci, co, H, W, p, dgrad, pooled, p16):
    if W > 63 or co % 32 or ci % 16:
        return None
    if pooled and (W > 62 or W % 2 or H % 2):
        return None
    if not pooled and W < 17:
        return None
    WP = 32 if W <= 31 else 64
    vw = _vw(W, p["x"])
    mode = (EPI_DGRAD_ADDPOOL if dgrad else EPI_FWD_POOL) if pooled else _plain_mode(dgrad, p)
    if mode is None:
        return None
    R = 256 // WP
    if R > H:
        R = (H + 1) & ~1
    if 2 * (R + 2) * (W // vw) > _nbs_small(vw) * 256:
        return None
    return {("al", vw, 2 if co % 64 == 0 else 1, mode, 0, int(p16))}


def _route_sb(N, ci, co, H, W, p, dgrad, p16):
    WP = (W + 4) // 4 * 4
    vw = _vw(W, p["x"])
    cop = (co + 31) // 32 * 32
    mode = (_plain_mode(dgrad, p) if co % 32 == 0 else None)
    mode = EPI_GENERIC if mode is None else mode
    rows_total = N * (H + 1)
    mts = set()
    for mt in ((2, 1) if cop % 64 == 0 else (1,)):
        for nt in (2, 1):
            cap = 128 * nt
            if WP > cap:
                continue
            R = min(cap // WP, rows_total)
            if 2 * (R + 2) * (W // vw) > _nbs_small(vw) * 256:
                continue
            if (2 * 9 * 2 * mt * 32 + 4 * (cap + 2 * WP + 3)) * 16 > 80 * 1024:
                continue
            mts.add(mt)                     # which feasible (MT, NT) wins is the cost model's choice
    return {("sb", vw, mt, mode, 0, int(p16)) for mt in mts} or None


def _conv_tile_force():
    e = os.environ.get("FDET_CONV_TILE")
    if not e:
        return 0, 0
    try:
        nw, nt = (int(v) for v in e.split(",")[:2])
    except ValueError:
        return 0, 0
    return nw, nt


def _route_general(N, ci, co, H, W, p, dgrad, p16):
    cop = (co + 31) // 32 * 32
    mode = EPI_GENERIC
    if co % 32 == 0 or (co % 16 == 0 and dgrad):
        m = _plain_mode(dgrad, p)
        if m is not None and (co % 32 == 0 or m in (EPI_DGRAD_ACT, EPI_DGRAD_ADD)):
            mode = m
    if all(_aligned(p[k], 16) for k in ("x", "y_full", "y_out", "skip", "act")) and W % 4 == 0:
        vw = 4
    elif W % 2 == 0 and _aligned(p["x"], 8):
        vw = 2
    else:
        vw = 1
    mt = 2 if cop % 64 == 0 else 1
    cfgs = ((8, 1), (4, 4), (8, 2)) if mt == 2 else ((8, 1), (8, 2))
    fnw, fnt = _conv_tile_force()
    rows_total = N * (H + 1)
    segs = set()
    for nw, nt in cfgs:
        if fnt and (nt != fnt or nw != fnw):
            continue
        nthr, cap = nw * 64, nw * nt * 32
        for nseg in range(1, 65):
            cw = (W + nseg - 1) // nseg
            if nseg > 1:
                cw = (cw + 3) // 4 * 4
                if (nseg - 1) * cw >= W:
                    continue
            wp = ((cw + 2 if nseg > 1 else W + 1) + 3) // 4 * 4
            if wp > cap:
                continue
            R = min(cap // wp, rows_total)
            if (2 * (2 * 9 * 2 * mt * 32 + 4 * (cap + 2 * wp + 3)) + nthr) * 16 > 160 * 1024:
                continue
            if nseg > 1 and vw != 4:
                continue
            if 2 * (R + 2) * (cw // vw) > _nbs_general(nw, nt, vw) * nthr:
                continue
            if nseg > 1 and 4 * (R + 2) > nthr:
                continue
            segs.add(int(nseg > 1))         # the first segment count that fits this tile; the cost model picks the tile
            break
    return {("general", vw, mt, mode, s, int(p16)) for s in segs}


def expected_route(kind, N, ci, co, H, W, p, p16):
    """Acceptable (family, VW, MT, mode, seg, p16) routes of one launch; the empty set means the call must be refused.
    kind: fwd / dgrad / fwd_pool / dgrad_unpool; ci / co: channels the runner reads / writes (a data gradient reads the
    conv's output channels and writes its input channels); p: name -> data_ptr (None: not passed)."""
    dgrad = kind in ("dgrad", "dgrad_unpool")
    env = os.environ
    if kind in ("fwd_pool", "dgrad_unpool"):
        return _route_al(N, ci, co, H, W, p, dgrad, True, p16) or set()
    kc = env.get("FDET_CONV_KERNEL", "")[:1]
    if W <= 64 and kc != "g":
        e = env.get("FDET_SB_AL")
        sb_al = -1 if e is None else (1 if e[:1] == "1" else 0)
        if sb_al == 1 or (sb_al < 0 and W >= 33):
            r = _route_al(N, ci, co, H, W, p, dgrad, False, p16)
            if r:
                return r
        r = _route_sb(N, ci, co, H, W, p, dgrad, p16)
        if r:
            return r
    return _route_general(N, ci, co, H, W, p, dgrad, p16)


def expected_wgrad_plan(N, ci, co, H, W, L=1):
    """plan_x3's route fields: ok, pipe, lpr32, pk4, pack (reserved, always 0), vw, mtc, nseg."""
    env = os.environ
    vw = 4 if W % 4 == 0 else (2 if W % 2 == 0 else 1)
    nseg, cw = 1, W
    if W // vw > 16 and vw == 4:
        cw, nseg = 56, (W + 55) // 56
    P = 64 if nseg > 1 else (W + 1 + 7) // 8 * 8
    cop = (co + 31) // 32 * 32
    mtc = 2 if cop % 64 == 0 else 1
    ok = cw // vw <= 16
    rows_total = N * (H + 1)
    lpr32 = P == 32 and nseg == 1 and W <= 32
    rp = 32 // (4 * vw)
    pipe = (ok and mtc == 2 and nseg == 1 and ((vw != 2 and rp * P == 128) or lpr32) and rows_total >= 8
            and env.get("FDET_WGRAD_PIPE", "")[:1] != "0")
    lpr32 = pipe and lpr32
    pk4 = pipe and env.get("FDET_WGRAD_PK4", "")[:1] != "0" and (
        (not lpr32 and vw == 1 and 13 <= W <= 16 and P == 16) or (lpr32 and W >= 29 and P == 32))
    if pipe and vw == 1 and not lpr32 and not pk4:
        pipe = lpr32 = False
    return dict(ok=int(ok), pipe=int(pipe), lpr32=int(lpr32), pk4=int(pk4), pack=0, vw=vw, mtc=mtc, nseg=nseg)


# ----------------------------------------------------------------------------------------------------------------------
# buffers: contiguous views at an offset of 0, 1 or 2 floats into a larger buffer with sentinel bands
# ----------------------------------------------------------------------------------------------------------------------
class Placed:
    def __init__(self, shape, off, src=None, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        self.off, self.n = off, n
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, device="cuda")
        self.t = self.buf[GUARD + off:GUARD + off + n].view(*shape)
        if src is not None:
            self.t.copy_(src)
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (4 * off) % 16

    def guards_intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD + self.off] == SENTINEL).all()) and bool((b[GUARD + self.off + self.n:] == SENTINEL).all())


def _ptrs(**kw):
    keys = ("x", "bias", "y_full", "skip", "scale", "y_out", "act")
    return {k: (kw[k].data_ptr() if kw.get(k) is not None else None) for k in keys}


def _route_tuple(hp):
    r = hp.conv3x3_x3_last_route()
    return (r["family"], r["vw"], r["mt"], r["mode"], r["seg"], r["p16"])


ROUTES_SEEN = set()


@pytest.fixture(scope="module", autouse=True)
def _routes_report():
    """CONV_PATHS_ROUTES_OUT=<file>: append the distinct routes and weight-gradient plans this process reached."""
    yield
    path = os.environ.get("CONV_PATHS_ROUTES_OUT")
    if path and ROUTES_SEEN:
        switches = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("FDET_") and k != "FDET_LIB_PATH")
        with open(path, "a") as f:
            for r in sorted(ROUTES_SEEN, key=str):
                f.write(f"{switches or '(defaults)'}\t{r}\n")


def _twice(hp, launch, outs, what):
    """Run `launch` on NaN-filled outputs, check the sentinels, run it again: bit-identical results and the same route.
    Returns the first run's outputs and its route (checked by the caller after the values, see _check_route)."""
    launch()
    torch.cuda.synchronize()
    got = _route_tuple(hp)
    ROUTES_SEEN.add(got)
    first = [o.t.clone() for o in outs]
    for o in outs:
        assert o.guards_intact(), f"{what}: write outside the output (offset {o.off})"
        o.t.fill_(float("nan"))
    launch()
    torch.cuda.synchronize()
    assert _route_tuple(hp) == got
    for o, f in zip(outs, first):
        assert o.guards_intact(), f"{what}: write outside the output on the second run"
        assert torch.equal(o.t.view(torch.int32), f.view(torch.int32)), f"{what}: second run differs"
    return first, got


def _check_route(got, expected, what):
    assert got in expected, f"{what}: reached {got}, expected one of {sorted(expected)}"


def _refused(hp, launch, outs, what):
    from fdet_amd import FdetError
    with pytest.raises(FdetError):
        launch()
    torch.cuda.synchronize()
    assert hp.conv3x3_x3_last_route()["family"] is None, f"{what}: a refused call recorded a launch"
    for o in outs:
        assert o.guards_intact() and bool(o.t.isnan().all()), f"{what}: a refused call wrote its output"


# ----------------------------------------------------------------------------------------------------------------------
# the case table
# ----------------------------------------------------------------------------------------------------------------------
WIDTHS = [1, 2, 13, 16, 17, 28, 31, 32, 33, 34, 35, 44, 47, 60, 62, 63, 64, 65, 66, 67, 127, 130, 252, 254, 255, 256, 258, 260]
CHANNELS = (16, 32, 48, 64, 96, 128)
_HS = (1, 2, 3, 5, 7)
_NS = (1, 3, 5)
_OFFS = ((0, 0), (2, 1), (1, 2), (0, 2), (2, 0), (1, 0), (0, 1))


def _width_cases():
    """Each width at VW 4 / 2 / 1 (x offset 0 / 2 / 1 floats) and with outputs offset independently; MT = 2 (64 or 128
    channels) and MT = 1 (32, 96, or 48 -> 16 with a padded half tile) alternate."""
    out = []
    k = 0
    chans = ((64, 64), (32, 32), (48, 16), (96, 128), (16, 48), (128, 96), (64, 32), (32, 64))
    for W in WIDTHS:
        # (x offset, output offset): x and outputs aligned, then x aligned with outputs not, then x at 8 / 4 bytes
        offs = ((0, 0), (0, 1), (2, 2), (1, 0)) if W % 4 == 0 else (((0, 0), (1, 2)) if W % 2 == 0 else ((0, 0), (2, 1)))
        for xo, oo in offs:
            ci, co = chans[k % len(chans)]
            N, H = _NS[k % 3], _HS[k % 5]
            if W >= 127:
                N, H = min(N, 3), min(H, 3)
            out.append((N, ci, co, H, W, xo, oo))
            k += 1
    return out


def _pair_cases():
    """Every (Cin, Cout) pair of CHANNELS, square ones included, on AL / sb / general widths."""
    out = []
    k = 0
    for ci in CHANNELS:
        for co in CHANNELS:
            W = (35, 20, 66, 60, 17, 130)[k % 6]
            xo, oo = _OFFS[k % len(_OFFS)]
            out.append((_NS[k % 3], ci, co, (2, 3, 1)[k % 3], W, xo, oo))
            k += 1
    return out


def ssd_cases():
    """The SSD engine's (Cin, Cout, W) triples: block_specs(16) from the stem's 240 columns, halved after pooled blocks."""
    import fdet_amd  # noqa: F401
    from fdet_amd.ssdstack import PATCH_SIZES, block_specs
    hk = 4 * PATCH_SIZES[0]
    seen, out, heads = set(), [], []
    for name, ci, co, pool, head in block_specs(16):
        for t in ((ci, co, hk), (co, co, hk)):
            if t not in seen:
                seen.add(t)
                out.append((1, t[0], t[1], 2, t[2], 0, 0))
        hk = hk // 2 if pool else hk
        if head >= 0:
            heads.append(hk)                    # the heads read the block outputs
    assert tuple(heads) == tuple(PATCH_SIZES)
    return out


# the widest rows without column segments that still have a tiling (W % 4 != 0, or an input that is not 16-byte aligned):
# 170 columns for MT = 2, 202 (VW = 2) / 191 (VW = 1) for MT = 1; one column more is refused (REFUSED_CONV)
EDGE_CASES = [(1, 64, 64, 2, 170, 0, 0), (2, 32, 32, 2, 202, 0, 0), (1, 32, 32, 3, 191, 1, 0), (1, 64, 64, 1, 170, 1, 2)]
# the small-tile kernel with MT = 2: its cost model (512 workgroup slots per round) takes two 32-channel tiles per
# workgroup once a 128-channel output has enough bands -- as for 64 channels at 30x30 with bench.py's batch of 256.
# Forward (Cout = 128) at VW 4 / 1, data gradient (Cin = 128) at VW 2; these cases require MT = 2 where the rules give
# the small-tile kernel a choice (without switches: always).  No weight gradient here: the other tables cover it.
SB_MT2_CASES = [(640, 16, 128, 1, 32, 0, 0), (640, 16, 128, 1, 32, 1, 2), (640, 128, 16, 1, 32, 2, 1)]
CASES = _width_cases() + _pair_cases() + ssd_cases() + EDGE_CASES + SB_MT2_CASES


def _require_sb_mt2(case, exp):
    if case in SB_MT2_CASES and any(t[0] == "sb" and t[2] == 2 for t in exp):
        return {t for t in exp if t[2] == 2}
    return exp


def _cid(c):
    N, ci, co, H, W, xo, oo = c
    return f"N{N}-{ci}x{co}-H{H}-W{W}-x{xo}-o{oo}"


def _data(case, seed):
    N, ci, co, H, W, xo, oo = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) * (0.3 / ci ** 0.5 * 3)
    b = torch.randn(co, generator=g)
    skip = torch.randn(N, co, H, W, generator=g)
    scale = (torch.rand(N, co, generator=g) > 0.25).float() / 0.75
    dz = torch.randn(N, co, H, W, generator=g)
    act = torch.randn(N, ci, H, W, generator=g)
    add = torch.randn(N, ci, H, W, generator=g)
    return x, w, b, skip, scale, dz, act, add


def _pack(hp, w):
    co, ci = w.shape[:2]
    nf, nb = hp.packed_sizes(co, ci)
    wf = torch.empty(nf, device="cuda"); wb = torch.empty(nb, device="cuda")
    hp.pack_conv3x3_weights(w.cuda(), wf, wb, x3=True)
    return wf, wb


def _check(p16, got, ref, what):
    if p16:
        close_bf16(got, ref, what)
    else:
        close(got, ref, what=what)


@pytest.mark.parametrize("p16", [False, True], ids=["bf16x3", "p16"])
@pytest.mark.parametrize("case", CASES, ids=[_cid(c) for c in CASES])
def test_conv_path(hp, case, p16):
    _run_case(hp, case, p16)


def _run_case(hp, case, p16):
    N, ci, co, H, W, xo, oo = case
    x, w, b, skip, scale, dz, act, add = _data(case, N * 7919 + ci * 31 + co * 17 + H * 5 + W)
    wf, wb = _pack(hp, w)
    xr, wr = (bf(x), bf(w)) if p16 else (x, w)
    xr, wr = xr.double(), wr.double()
    bd, bc, xc = b.cuda(), b.double(), Placed(x.shape, xo, x.cuda())
    sk, sc = Placed(skip.shape, oo, skip.cuda()), scale.cuda()
    z = F.leaky_relu(F.conv2d(xr, wr, bc, padding=1), SLOPE)

    def fwd(**kw):
        hp.conv3x3_fwd(xc.t, wf, bd, co, slope=SLOPE, x3=True, p16=p16, **kw)

    # forward: conv1 flavour (FULL), training block tail (BOTH), eval block tail (OUT)
    yf = Placed((N, co, H, W), oo)
    o2 = (oo + 1) % 3 if oo else 0          # with outputs at offset 0, every pointer is aligned (the general kernel's VW 4)
    yf2, yo2 = Placed((N, co, H, W), oo), Placed((N, co, H, W), o2)
    yo3 = Placed((N, co, H, W), oo)
    flavours = (("fwd FULL", dict(y_full=yf), [yf], [z]),
                ("fwd BOTH", dict(y_full=yf2, skip=sk, drop_scale=sc, y_out=yo2), [yf2, yo2],
                 [z, z * scale.double()[:, :, None, None] + skip.double()]),
                ("fwd OUT", dict(skip=sk, y_out=yo3), [yo3], [z + skip.double()]))
    for what, kw, outs, refs in flavours:
        args = {k: v.t for k, v in kw.items() if isinstance(v, Placed)}
        args.update({k: v for k, v in kw.items() if not isinstance(v, Placed)})
        p = _ptrs(x=xc.t, bias=bd, y_full=args.get("y_full"), skip=args.get("skip"), scale=args.get("drop_scale"),
                  y_out=args.get("y_out"))
        exp = _require_sb_mt2(case, expected_route("fwd", N, ci, co, H, W, p, p16))
        what = f"{what} {_cid(case)}"
        if not exp:
            _refused(hp, lambda: fwd(**args), outs, what)
            continue
        got, route = _twice(hp, lambda: fwd(**args), outs, what)
        for g_, r_ in zip(got, refs):
            _check(p16, g_, r_, what)
        _check_route(route, exp, what)

    # data gradient x lrelu'(act), + add, and both (the generic epilogue)
    dzc = Placed(dz.shape, xo, dz.cuda())
    ac, adc = Placed(act.shape, oo, act.cuda()), Placed(add.shape, (oo + 2) % 3 if oo else 0, add.cuda())
    dzr = (bf(dz) if p16 else dz).double()
    base = F.conv_transpose2d(dzr, wr, padding=1)
    dact = torch.where(act > 0, 1.0, SLOPE).double()
    for what, a_, d_, ref in (("dgrad ACT", ac, None, base * dact), ("dgrad ADD", None, adc, base + add.double()),
                              ("dgrad ACT+ADD", ac, adc, base * dact + add.double())):
        dx = Placed((N, ci, H, W), oo)
        p = _ptrs(x=dzc.t, y_full=dx.t, act=a_.t if a_ else None, skip=d_.t if d_ else None)
        exp = _require_sb_mt2(case, expected_route("dgrad", N, co, ci, H, W, p, p16))
        what = f"{what} {_cid(case)}"

        def launch():
            hp.conv3x3_dgrad(dzc.t, wb, ci, dx.t, act=a_.t if a_ else None, add=d_.t if d_ else None, slope=SLOPE, x3=True,
                             p16=p16)
        if not exp:
            _refused(hp, launch, [dx], what)
            continue
        got, route = _twice(hp, launch, [dx], what)
        _check(p16, got[0], ref, what)
        _check_route(route, exp, what)

    # weight gradient, single and batched (L = 2)
    if case not in SB_MT2_CASES:
        _wgrad(hp, case, x, dz, p16)


def _wgrad(hp, case, x, dz, p16):
    from fdet_amd import FdetError
    N, ci, co, H, W, xo, oo = case
    for L in (1, 2):
        plan = hp.conv3x3_wgrad_x3_plan(N, ci, co, H, W, L)
        assert plan == expected_wgrad_plan(N, ci, co, H, W, L), f"wgrad plan L={L} {_cid(case)}: {plan}"
        ROUTES_SEEN.add(("wgrad",) + tuple(plan.values()))
        nbytes = hp.conv3x3_wgrad_batched_ws_bytes(L, N, ci, co, H, W)
        assert (nbytes > 0) == bool(plan["ok"])
        if L == 1:
            assert hp.wgrad_x3_supported(N, ci, co, H, W) == bool(plan["ok"])
        xs = [x] + ([torch.roll(x, 1, 0) * 0.5] if L == 2 else [])
        dzs = [dz] + ([torch.roll(dz, 1, 3) - 0.25] if L == 2 else [])
        xc = [Placed(t.shape, xo, t.cuda()) for t in xs]
        zc = [Placed(t.shape, (xo + 1) % 3, t.cuda()) for t in dzs]
        dW = [Placed((co, ci, 3, 3), oo) for _ in range(L)]
        db = [Placed((co,), (oo + l + 1) % 3) for l in range(L)]
        ws = torch.empty(max(nbytes, hp.conv3x3_wgrad_ws_bytes(N, ci, co, H, W)) // 4 + 1, device="cuda")

        def launch():
            if L == 1:
                hp.conv3x3_wgrad(xc[0].t, zc[0].t, dW[0].t, db[0].t, ws, x3=True, p16=p16)
            else:
                hp.conv3x3_wgrad_batched([t.t for t in xc], [t.t for t in zc], [t.t for t in dW], [t.t for t in db], ws,
                                         p16=p16)
        what = f"wgrad L={L} {_cid(case)}"
        if not plan["ok"]:
            with pytest.raises(FdetError):
                launch()
            torch.cuda.synchronize()
            assert all(t.guards_intact() and bool(t.t.isnan().all()) for t in dW + db), f"{what}: refused call wrote"
            continue
        launch()
        torch.cuda.synchronize()
        first = [t.t.clone() for t in dW + db]
        assert all(t.guards_intact() for t in dW + db), f"{what}: write outside dW / db"
        for t in dW + db:
            t.t.fill_(float("nan"))
        launch()
        torch.cuda.synchronize()
        for t, f_ in zip(dW + db, first):
            assert t.guards_intact() and torch.equal(t.t.view(torch.int32), f_.view(torch.int32)), f"{what}: second run"
        for l in range(L):
            xr = (bf(xs[l]) if p16 else xs[l]).double()
            zr = (bf(dzs[l]) if p16 else dzs[l]).double()
            close(dW[l].t, torch.nn.grad.conv2d_weight(xr, (co, ci, 3, 3), zr, padding=1), what=what + " dW")
            close(db[l].t, zr.sum(dim=(0, 2, 3)), what=what + " db")


# weight-gradient plans: the pipelined kernel's float4 rows (P = 64), 16-lane one-float rows with float4 quads (13, 15),
# the 32-lane rows (24..32 columns, VW 4 / 2: odd rows that wide exceed 16 lanes and are refused; float4 quads from 29), the staged kernel at VW 4 / 2 / 1 with MTC 1 / 2, column
# segments (rows wider than 64 floats)
WGRAD_CASES = [(3, 64, 64, 3, 60, 0, 0), (2, 64, 128, 5, 56, 1, 2), (3, 64, 64, 3, 13, 0, 1), (5, 128, 64, 2, 15, 2, 0),
               (3, 64, 64, 3, 28, 0, 0), (3, 32, 64, 2, 24, 1, 1), (3, 64, 64, 3, 30, 2, 2), (3, 96, 64, 2, 26, 0, 0),
               (1, 64, 64, 5, 9, 0, 0), (3, 64, 32, 3, 60, 0, 1), (1, 48, 96, 3, 14, 2, 0), (2, 64, 64, 1, 11, 0, 0),
               (1, 64, 64, 3, 120, 0, 0), (2, 32, 48, 2, 236, 1, 0), (5, 64, 64, 2, 4, 0, 2), (3, 16, 64, 3, 8, 0, 0),
               (3, 64, 64, 1, 16, 1, 0)]


@pytest.mark.parametrize("p16", [False, True], ids=["bf16x3", "p16"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[_cid(c) for c in WGRAD_CASES])
def test_wgrad_path(hp, case, p16):
    N, ci, co, H, W, xo, oo = case
    g = torch.Generator().manual_seed(N * 61 + ci + co + H + W)
    _wgrad(hp, case, torch.randn(N, ci, H, W, generator=g), torch.randn(N, co, H, W, generator=g), p16)


# ----------------------------------------------------------------------------------------------------------------------
# explicit refusals: shapes with no tiling must raise FdetError, and the plan queries must agree
# ----------------------------------------------------------------------------------------------------------------------
# (N, Cin, Cout, H, W, x offset): rows too wide for one unsegmented tile whose width (W % 4 != 0) or input pointer
# (not 16-byte aligned) rules out column segments
REFUSED_CONV = [(1, 64, 64, 2, 171, 0), (1, 64, 64, 2, 174, 0), (1, 32, 32, 2, 203, 0), (1, 32, 32, 2, 193, 0),
                (1, 64, 64, 2, 254, 0), (1, 32, 32, 2, 255, 0), (1, 64, 64, 2, 258, 0), (1, 32, 64, 1, 258, 2),
                (1, 64, 64, 2, 256, 1), (1, 64, 64, 2, 260, 2)]
# weight gradients of rows wider than 16 vector lanes without column segments (odd rows wider than 16, W % 4 == 2
# rows wider than 32)
REFUSED_WGRAD = [(2, 64, 64, 3, 17), (2, 32, 64, 3, 33), (1, 64, 64, 2, 34), (1, 64, 32, 2, 62), (1, 64, 64, 2, 255),
                 (1, 16, 16, 1, 130)]


@pytest.mark.parametrize("p16", [False, True], ids=["bf16x3", "p16"])
@pytest.mark.parametrize("shape", REFUSED_CONV, ids=[f"W{s[4]}-x{s[5]}" for s in REFUSED_CONV])
def test_conv_refusals(hp, shape, p16):
    N, ci, co, H, W, xo = shape
    x = Placed((N, ci, H, W), xo, torch.randn(N, ci, H, W, device="cuda"))
    dz = Placed((N, co, H, W), xo, torch.randn(N, co, H, W, device="cuda"))
    wf, wb = _pack(hp, torch.randn(co, ci, 3, 3) * 0.1)
    b = torch.randn(co, device="cuda")
    y = Placed((N, co, H, W), 0)
    dx = Placed((N, ci, H, W), 0)
    assert not expected_route("fwd", N, ci, co, H, W, _ptrs(x=x.t, bias=b, y_full=y.t), p16)
    assert not expected_route("dgrad", N, co, ci, H, W, _ptrs(x=dz.t, y_full=dx.t, skip=dx.t), p16)
    _refused(hp, lambda: hp.conv3x3_fwd(x.t, wf, b, co, y_full=y.t, x3=True, p16=p16), [y], "fwd")
    add = torch.zeros(N, ci, H, W, device="cuda")
    _refused(hp, lambda: hp.conv3x3_dgrad(dz.t, wb, ci, dx.t, add=add, x3=True, p16=p16), [dx], "dgrad")


@pytest.mark.parametrize("shape", REFUSED_WGRAD, ids=[f"W{s[4]}" for s in REFUSED_WGRAD])
def test_wgrad_refusals(hp, shape):
    N, ci, co, H, W = shape
    assert not expected_wgrad_plan(N, ci, co, H, W)["ok"]
    g = torch.Generator().manual_seed(W)
    _wgrad(hp, (N, ci, co, H, W, 0, 0), torch.randn(N, ci, H, W, generator=g), torch.randn(N, co, H, W, generator=g), False)
    assert hp.conv3x3_wgrad_x3_plan(N, ci, co, H, W)["ok"] == 0


def test_tables_reach_their_branches():
    """Without switches the width table reaches every family the defaults use, VW 4 / 2 / 1 in each, both MT, and
    segmented rows; every listed refusal is refused by the rules (checked on the GPU by test_*_refusals)."""
    for k in ("FDET_CONV_KERNEL", "FDET_SB_AL", "FDET_CONV_TILE"):
        if k in os.environ:
            pytest.skip("the defaults only")
    reach = set()
    for N, ci, co, H, W, xo, oo in _width_cases():
        base = 0x10000 + 4 * xo
        p = {"x": base, "bias": 1, "y_full": 0x20000 + 4 * oo, "skip": None, "scale": None, "y_out": None, "act": None}
        r = expected_route("fwd", N, ci, co, H, W, p, False)
        assert r or W >= 252, f"W={W} x{xo}: no route"
        reach |= {(t[0], t[1], t[2], t[4]) for t in r}
    for fam in ("al", "sb", "general"):
        for vw in (4, 2, 1):
            assert any(t[0] == fam and t[1] == vw for t in reach), (fam, vw)
        for mt in (1, 2):
            assert any(t[0] == fam and t[2] == mt for t in reach), (fam, mt)
    assert any(t[0] == "general" and t[3] for t in reach)


# ----------------------------------------------------------------------------------------------------------------------
# pooled-block modes (fdet_conv3x3_fwd_pool / fdet_conv3x3_dgrad_unpool): even maps of <= 62 columns
# ----------------------------------------------------------------------------------------------------------------------
# (N, Cin, Cout, H, W, x offset, out offset)
POOL_CASES = [(2, 64, 64, 4, 60, 0, 0), (1, 32, 32, 6, 62, 0, 1), (3, 64, 64, 2, 30, 1, 0), (2, 16, 32, 4, 44, 2, 2),
              (5, 96, 64, 2, 18, 0, 0), (2, 128, 128, 4, 16, 0, 1), (1, 64, 32, 2, 2, 1, 1), (3, 32, 96, 2, 34, 2, 0),
              (1, 48, 64, 8, 36, 1, 2), (2, 64, 128, 2, 48, 0, 2), (1, 32, 32, 2, 64, 0, 0)]


@pytest.mark.parametrize("p16", [False, True], ids=["bf16x3", "p16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=[_cid(c) for c in POOL_CASES])
def test_pooled_path(hp, case, p16):
    N, ci, co, H, W, xo, oo = case
    Ho, Wo = H // 2, W // 2
    g = torch.Generator().manual_seed(N * 131 + ci + co + W)
    x = torch.randn(N, ci, H, W, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) * 0.1
    b = torch.randn(co, generator=g)
    skip = torch.randn(N, co, H, W, generator=g)
    scale = (torch.rand(N, co, generator=g) > 0.25).float() / 0.75
    wf, wb = _pack(hp, w)
    xc, sk = Placed(x.shape, xo, x.cuda()), Placed(skip.shape, oo, skip.cuda())
    out = Placed((N, co, Ho, Wo), oo)
    route = torch.full((N, co, Ho, Wo), 255, dtype=torch.uint8, device="cuda")
    fusion_fwd = hp.pool_fusion_supported(co, ci, H, W, N)

    def fwd():
        hp.conv3x3_fwd_pool(xc.t, wf, b.cuda(), sk.t, scale.cuda(), out.t, route, slope=SLOPE, p16=p16)
    exp = expected_route("fwd_pool", N, ci, co, H, W, _ptrs(x=xc.t, bias=b, skip=sk.t, scale=scale), p16)
    if not exp:
        assert not fusion_fwd, "fdet_conv3x3_pool_fusion_ok accepts a shape the pooled forward refuses"
        _refused(hp, fwd, [out], f"fwd_pool {_cid(case)}")
    else:
        (got,), kr = _twice(hp, fwd, [out], f"fwd_pool {_cid(case)}")
        _check_route(kr, exp, f"fwd_pool {_cid(case)}")
        xr, wr = ((bf(x), bf(w)) if p16 else (x, w))
        c = F.leaky_relu(F.conv2d(xr.double(), wr.double(), b.double(), padding=1), SLOPE)
        e = c * scale.double()[:, :, None, None] + skip.double()
        _check(p16, got, F.max_pool2d(e, 2), f"fwd_pool {_cid(case)}")
        # the routing byte's argmax, wherever the window's decision is not within the rounding
        r = route.cpu().int()
        arg = (r >> 4) & 3
        ew = e.unfold(2, 2, 2).unfold(3, 2, 2).reshape(N, co, Ho, Wo, 4)
        top2 = ew.topk(2, dim=-1).values
        # (precision16 takes the max and the routing bits on the fp32 values, before the stored value is rounded)
        decided = (top2[..., 0] - top2[..., 1]) > 1e-4 * max(1.0, float(e.abs().max()))
        assert float(decided.float().mean()) > 0.99
        assert torch.equal(arg[decided], ew.argmax(-1)[decided].int())
        cw = c.unfold(2, 2, 2).unfold(3, 2, 2).reshape(N, co, Ho, Wo, 4)
        for k in range(4):                  # lrelu sign bits of the window's four elements, ATen scan order
            clear = cw[..., k].abs() > 1e-4 * max(1.0, float(c.abs().max()))
            assert torch.equal(((r >> k) & 1)[clear].bool(), (cw[..., k] > 0)[clear])
        assert int((r >> 6).max()) == 0
        # eval flavour: no routing bytes, no dropout scale
        out_e = Placed((N, co, Ho, Wo), oo)

        def fwd_eval():
            hp.conv3x3_fwd_pool(xc.t, wf, b.cuda(), sk.t, None, out_e.t, None, slope=SLOPE, p16=p16)
        (got_e,), kr_e = _twice(hp, fwd_eval, [out_e], f"fwd_pool eval {_cid(case)}")
        _check(p16, got_e, F.max_pool2d(c + skip.double(), 2), f"fwd_pool eval {_cid(case)}")
        _check_route(kr_e, exp, f"fwd_pool eval {_cid(case)}")

    # data gradient + unpool(dout) through routing bytes (the arg field: bits 4-5); the runner writes Cin channels
    dz = torch.randn(N, co, H, W, generator=g)
    dout = torch.randn(N, ci, Ho, Wo, generator=g)
    arg = torch.randint(0, 4, (N, ci, Ho, Wo), generator=g)
    rin = ((arg << 4) | torch.randint(0, 16, (N, ci, Ho, Wo), generator=g)).to(torch.uint8)
    dzc, doc = Placed(dz.shape, xo, dz.cuda()), Placed(dout.shape, oo, dout.cuda())
    dx = Placed((N, ci, H, W), (oo + 1) % 3)
    fusion_bwd = hp.pool_fusion_supported(ci, co, H, W, N)

    def bwd():
        hp.conv3x3_dgrad_unpool(dzc.t, wb, ci, doc.t, rin.cuda(), dx.t, slope=SLOPE, p16=p16)
    exp = expected_route("dgrad_unpool", N, co, ci, H, W, _ptrs(x=dzc.t, y_full=dx.t), p16) if ci % 32 == 0 else set()
    if not exp:
        assert not fusion_bwd, "fdet_conv3x3_pool_fusion_ok accepts a shape the pooled data gradient refuses"
        _refused(hp, bwd, [dx], f"dgrad_unpool {_cid(case)}")
        return
    (got,), kr = _twice(hp, bwd, [dx], f"dgrad_unpool {_cid(case)}")
    _check_route(kr, exp, f"dgrad_unpool {_cid(case)}")
    de = torch.zeros(N, ci, Ho, Wo, 4, dtype=torch.float64)
    de.scatter_(-1, arg.unsqueeze(-1), dout.double().unsqueeze(-1))
    de_full = de.reshape(N, ci, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, ci, H, W)
    dzr, wr = ((bf(dz), bf(w)) if p16 else (dz, w))
    _check(p16, got, F.conv_transpose2d(dzr.double(), wr.double(), padding=1) + de_full, f"dgrad_unpool {_cid(case)}")


# ----------------------------------------------------------------------------------------------------------------------
# FDET_CONV_TILE (read at every call): the general kernel's three MT = 2 and two MT = 1 tile configurations
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["8,1", "4,4", "8,2"])
@pytest.mark.parametrize("chans", [(64, 64), (32, 96)], ids=["MT2", "MT1"])
def test_conv_tile_configs(hp, monkeypatch, tile, chans):
    """{4,4} exists only for MT = 2: forcing it on an MT = 1 layer leaves no tiling, and the call is refused."""
    monkeypatch.setenv("FDET_CONV_TILE", tile)
    ci, co = chans
    for W, xo in ((130, 0), (66, 2), (256, 0)):
        for p16 in (False, True):
            _run_case(hp, (2, ci, co, 3, W, xo, 0), p16)


# ----------------------------------------------------------------------------------------------------------------------
# switches read once per process: one child process per group, a -k subset of this file
# ----------------------------------------------------------------------------------------------------------------------
SWITCH_GROUPS = [
    ({"FDET_CONV_KERNEL": "general", "FDET_WGRAD_PIPE": "0"}, "test_conv_path and (W6 or W3 or W1-)"),
    ({"FDET_SB_AL": "0", "FDET_WGRAD_PK4": "0"}, "test_conv_path and (W3 or W4 or W1)"),
    ({"FDET_SB_AL": "1"}, "test_conv_path and (W1 or W2 or W3)"),
]


def test_switch_groups():
    """Each group re-runs a subset of this file in a fresh process with its switches set; expected_route and
    expected_wgrad_plan read the same environment, so every case there also proves the switch took effect.  A child
    that fails, times out or dies on a signal fails this test at once (no retries, no further children)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for extra, sel in SWITCH_GROUPS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("FDET_") or k == "FDET_LIB_PATH"}
        env.update(extra)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                            os.path.join(root, "tests", "test_gpu_conv_paths.py"), "-k", sel], env=env, capture_output=True,
                           text=True, timeout=600, cwd=root)
        tail = r.stdout[-3000:] + r.stderr[-2000:]
        assert r.returncode == 0 and " passed" in r.stdout, f"{extra}: exit {r.returncode}\n{tail}"
