"""Every dispatch path of the stem convolution (csrc/fdet_stem.hip, fdet_stem_mfma.hip, fdet_stem_x3.hip,
fdet_stem_k3.hip: 3 -> F channels, k10 s8 p2 for PoolResnet, k3 s2 p1 for Resnet / SSD / SeparableCNN) against a float64
CPU reference of the same operation (F.conv2d, torch.nn.grad.conv2d_weight, dy.sum), at shapes chosen for the edges:
bottom / right padding that is really read, H != W, widths at the limits of each kernel, channel counts that pad
(F = 8, 100, 72) or take two channel blocks (F = 128, 72), the smallest maps, and batches whose rows outnumber the
persistent grids.

Each case runs EVERY stem entry point on its shape.  `expected_stem_route` -- a restatement of stem_plan, stem_mfma_ok,
the pipelined / single-tile choices, stem3_wgrad_ok, stem3_fwd_ps_ok, the scalar-fed condition and the three
process-wide switches -- says which kernel family must run (checked through fdet_stem_last_route, with the work items
and the grid of the launch) or that the call must be refused (FdetError, outputs untouched, an empty record).  A case
that drifts off its route fails.  tests/test_stem_paths_host.py checks on the CPU that the case list reaches every
route the library builds.

Bounds (the project's existing ones): fp32 and bf16x3 max|got - ref| <= 1e-4 * max(1, max|ref|); precision16 outputs
within close_bf16 of the reference on bf16-rounded operands and got == bf(got) (the k3 PS forward is fp32 VALU
arithmetic in either precision and rounds only what it stores: its reference keeps the fp32 operands, the bound is the
same); precision16 weight gradients within 1e-4 of the scale of the reference on bf(x), bf(dy); the bias gradient of
the k10 kernels is summed from the fp32 dy, that of the k3 matrix-core kernel from bf(dy) (its ones column multiplies the rounded operand: fdet_stem_k3.hip,
test_p16_ssd_stem_wgrad).  The uint8 forms are bit-equal to fdet_u8_to_f32_norm + the float form.
Plain outputs and the workspace sit inside 64-float sentinel bands that must survive, outputs start as NaN, PS outputs
must leave every halo / zero slot zero, x and dy sit between NaN bands (a read past an input shows even where only its
product with a zero reaches the result), and every launch runs twice and must repeat bit for bit.  Every case runs on
x = rand and on an input whose only non-zero pixels are in the last row and last column.

Observed on an MI355X: the worst error as a fraction of its bound, per route, over every case, loop case and switch
child of one run (STEM_PATHS_ERRORS_OUT=<file> writes them):
    valu_k10         fwd 0.004   wgrad 0.003          valu_k3_generic  fwd 0.001   wgrad 0.004
    valu_k3_scalar   wgrad 0.003                      mfma             fwd 0.006   wgrad 0.003
    x3_single        fwd 0.030   wgrad 0.132          k3_matrix        wgrad 0.136   precision16 wgrad 0.001
    x3_pipe          fwd 0.030   wgrad 0.097   precision16 wgrad 0.002
    x3_pipe PS fwd   0.058   uint8 0.074   precision16 0.986   uint8 + precision16 0.986
    k3_ps_fwd        0.067   precision16 0.988
The precision16 outputs sit at their bound by construction: rounding a value just above a power of two to bf16 moves
it by up to 2^-8 of itself, which is the bound; the fp32-grade routes leave a factor of 7 or more.

The switches read once per process (FDET_STEM_VALU, FDET_STEM_PIPE, FDET_STEM_K3_GENERIC) are covered by re-running
subsets of this file in child processes (test_switch_groups)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_paths import GUARD, Placed     # outputs inside sentinel bands, shared with those tests
from test_gpu_p16 import bf, close_bf16                     # precision16 rounding and its output bound

pytestmark = pytest.mark.gpu

K10, K3 = (10, 8, 2), (3, 2, 1)
ROUTE_KEYS = ("family", "pass", "p16", "u8", "ps")


@pytest.fixture(scope="module")
def env():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, ps
    return hotpath, ps


# ----------------------------------------------------------------------------------------------------------------------
# expected routes: a restatement of the dispatch code
# ----------------------------------------------------------------------------------------------------------------------
def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def stem_plan(N, F_, H, W, k, s, p):
    """stem_plan (fdet_stem.hip): None when the fp32 entry points refuse the shape."""
    if (k, s, p) not in (K10, K3):
        return None
    Ho, Wo = out_hw(H, W, k, s, p)
    wo64 = (Wo + 63) // 64 * 64
    BXS = wo64 + (k + s - 1) // s + 1
    XS = W + 2 * p + s + 4
    DS = Wo | 1
    lds_fwd = 3 * k * s * BXS * 4
    lds_wg = (3 * k * XS + 64 * DS) * 4
    if lds_fwd > 160 * 1024 or lds_wg > 160 * 1024:
        return None
    return dict(Ho=Ho, Wo=Wo, nblk=min(N * Ho, 1024 if k == 3 else 512), lds_fwd=lds_fwd, lds_wg=lds_wg)


def stem_mfma_ok(F_, H, W, k, s, p):
    if (k, s, p) != K10:
        return False
    Wo = out_hw(H, W, k, s, p)[1]
    return W % 4 == 0 and W <= 512 and Wo % 4 == 0 and Wo <= 64 and F_ >= 1


def ps_wp(W):
    return 16 if W + 1 <= 16 else (32 if W + 1 <= 32 else (64 if W + 1 <= 64 else 0))


def ps_geo_ok(N, C, H, W):
    wp = ps_wp(W)
    if wp == 0 or C % 8 or N < 1 or H < 1:
        return False
    return (N + 2) * 2 * (C // 8) * ((H + 2) & ~1) * wp < (1 << 31)


def ps_strips(W):
    """(S, Ws, Wlast) of ps_geo_strips, or None."""
    if W <= 63:
        return 1, W, W
    if W & 1:
        return None
    S = (W + 61) // 62
    Ws = ((W + S - 1) // S + 1) & ~1
    Wlast = W - (S - 1) * Ws
    if Wlast <= 0 or Ws > 62:
        return None
    return S, Ws, Wlast


def ps_geo_strips_ok(N, C, H, W):
    st = ps_strips(W)
    if st is None:
        return False
    S, Ws, _ = st
    if S == 1:
        return ps_geo_ok(N, C, H, W)
    return N * S < (1 << 20) and ps_geo_ok(N * S, C, H, Ws) and ps_wp(Ws) == 64


def stem3_wgrad_ok(F_, H, W, k, s, p):
    if (k, s, p) != K3 or F_ <= 0 or F_ % 8:
        return False
    Wo = out_hw(H, W, k, s, p)[1]
    return H % 2 == 0 and W % 4 == 0 and Wo % 16 == 0 and Wo <= 320


def stem3_fwd_ps_ok(F_, H, W, k, s, p):
    return (k, s, p) == K3 and F_ % 8 == 0 and H % 2 == 0 and W % 2 == 0


def _pipe_on(env):
    return env.get("FDET_STEM_PIPE", "")[:1] != "0"


def stem_x3_wgrad_pipe_ok(N, F_, H, W, env):
    Wo = out_hw(H, W, *K10)[1]
    return _pipe_on(env) and N > 0 and F_ > 0 and H >= 10 and 48 < Wo <= 60


def _route(family, pass_, p16, u8, ps_, items, grid):
    return dict(zip(ROUTE_KEYS, (family, pass_, int(p16), int(u8), int(ps_))), items=items, grid=grid, launches=1)


def expected_stem_route(entry, N, F_, H, W, k, s, p, p16=False, u8=False, env=None, ncu=256):
    """The record fdet_stem_last_route must hold after `entry` (fwd, fwd_x3, fwd_ps, wgrad, wgrad_x3) on this shape, or
    None when the library must refuse the call.  env: the process environment (the switches are read from it)."""
    env = os.environ if env is None else env
    valu = "FDET_STEM_VALU" in env                       # FDET_ENV_ONCE: set at all, whatever the value
    k3_generic = "FDET_STEM_K3_GENERIC" in env
    Ho, Wo = out_hw(H, W, k, s, p)
    nrows = N * Ho
    mfma = stem_mfma_ok(F_, H, W, k, s, p)
    if entry == "fwd":
        pl = stem_plan(N, F_, H, W, k, s, p)
        if pl is None:
            return None
        if mfma and not valu:
            return _route("mfma", "fwd", 0, 0, 0, nrows, min(nrows, 256))
        return _route("valu_k10" if k == 10 else "valu_k3_generic", "fwd", 0, 0, 0, nrows, nrows)
    if entry == "fwd_x3":
        if not mfma:
            return None
        return _route("x3_pipe" if _pipe_on(env) else "x3_single", "fwd", 0, 0, 0, nrows, min(nrows, 256))
    if entry == "fwd_ps":
        if not u8 and stem3_fwd_ps_ok(F_, H, W, k, s, p):
            if not ps_geo_strips_ok(N, F_, H // 2, W // 2):
                return None
            return _route("k3_ps_fwd", "fwd", p16, 0, 1, nrows, nrows)
        if F_ == 64 and mfma and H >= 10 and ps_geo_ok(N, F_, Ho, Wo):
            return _route("x3_pipe", "fwd", p16, u8, 1, nrows, min(nrows, 256))
        return None
    if entry == "wgrad":
        pl = stem_plan(N, F_, H, W, k, s, p)
        if pl is None:
            return None
        if mfma and not valu:
            return _route("mfma", "wgrad", 0, 0, 0, nrows, min(nrows, 256))
        if k == 10:
            return _route("valu_k10", "wgrad", 0, 0, 0, nrows, pl["nblk"])
        if H % 2 == 0 and W % 2 == 0 and Wo % 4 == 0 and not k3_generic:
            nitems = nrows * ((Wo + 63) // 64)
            return _route("valu_k3_scalar", "wgrad", 0, 0, 0, nitems, min(nitems, 4 * ncu, pl["nblk"]))
        return _route("valu_k3_generic", "wgrad", 0, 0, 0, nrows, pl["nblk"])
    if entry == "wgrad_x3":
        if stem3_wgrad_ok(F_, H, W, k, s, p):
            return _route("k3_matrix", "wgrad", p16, 0, 0, nrows, min(nrows, 3 * ncu))
        if not (mfma and W % 16 == 0):
            return None
        if stem_x3_wgrad_pipe_ok(N, F_, H, W, env):
            return _route("x3_pipe", "wgrad", p16, 0, 0, nrows, min(nrows, 256))
        if p16:
            return None                                   # precision16 has the pipelined kernel only
        return _route("x3_single", "wgrad", 0, 0, 0, nrows, min(nrows, 256))
    raise ValueError(entry)


# every (entry, p16, u8) form a case is run through
ENTRIES = [("fwd", False, False), ("fwd_x3", False, False), ("fwd_ps", False, False), ("fwd_ps", True, False),
           ("fwd_ps", False, True), ("fwd_ps", True, True), ("wgrad", False, False), ("wgrad_x3", False, False),
           ("wgrad_x3", True, False)]

# ----------------------------------------------------------------------------------------------------------------------
# the case table: (k, N, F, H, W, x offset in floats)
# ----------------------------------------------------------------------------------------------------------------------
K10_CASES = [
    (10, 2, 64, 478, 484, 0),    # MFMA fwd + wgrad, pipelined fwd, PS fwd at WP 64: bottom pad, 4 unused right columns; x3 wgrad refused
    (10, 2, 100, 96, 480, 0),    # Ho << Wo, pipelined wgrad (both precisions) with FP = 128 > F; PS refused (F != 64)
    (10, 2, 8, 486, 96, 0),      # Ho >> Wo: single-tile x3 wgrad at Wo = 12 with 61 rows per image; precision16 wgrad refused
    (10, 2, 64, 62, 416, 0),     # pipelined wgrad at its lower edge (Wo = 52), PS fwd at Wo = 52
    (10, 1, 128, 94, 352, 0),    # single-tile x3 wgrad at Wo = 44, two channel blocks, one image; precision16 wgrad refused
    (10, 2, 64, 70, 512, 0),     # Wo = 64, W = 512 (j < jmax, the last bx); PS refused (no 64-slot row holds 64 columns)
    (10, 2, 32, 22, 32, 0),      # smallest maps (3 x 4); PS refused (F = 32)
    (10, 2, 64, 10, 36, 0),      # Ho = 1; PS fwd at WP 16; x3 wgrad refused (W % 16)
    (10, 2, 64, 102, 224, 0),    # PS fwd at WP 32 in all four forms
    (10, 2, 64, 478, 478, 0),    # VALU k10: right and bottom pad; the uint8 form refused (W % 4)
    (10, 2, 100, 94, 38, 0),     # VALU k10, Wo = 5
    (10, 1, 8, 13, 12, 0),       # VALU k10, a 1 x 1 map
    (10, 2, 128, 100, 640, 0),   # VALU k10 beyond W = 512: two 64-column passes, more than 64 KiB of LDS
    (10, 2, 8, 54, 516, 0),      # VALU k10 at W = 516, Wo = 64
]
K3_CASES = [
    (3, 2, 16, 64, 40, 0),       # scalar-fed wgrad, W % 16 != 0, partial last chunk (Wo = 20)
    (3, 1, 8, 8, 24, 0),         # ... Wo = 12, one image
    (3, 2, 64, 30, 136, 0),      # scalar-fed with 2 segments (Wo = 68), PS fwd with 2 strips
    (3, 2, 72, 32, 488, 0),      # scalar-fed with 4 segments (Wo = 244), PS fwd with 4 strips, last strip 58 columns; FP 128
    (3, 2, 16, 64, 32, 4),       # scalar-fed with W % 16 == 0 on a base that is not 64-byte aligned
    (3, 2, 72, 33, 47, 0),       # generic wgrad, VALU fwd: odd H and odd W
    (3, 2, 8, 21, 30, 0),        # generic: odd H
    (3, 1, 64, 32, 31, 0),       # generic: odd W
    (3, 2, 64, 50, 64, 0),       # k3 matrix-core wgrad, 2 k-steps, odd Ho
    (3, 2, 16, 48, 96, 0),       # ... 3 k-steps
    (3, 2, 72, 20, 640, 0),      # ... 20 k-steps (every wave 5), PS fwd with 6 strips
    (3, 2, 8, 6, 1280, 0),       # PS fwd with 11 strips; matrix-core wgrad refused (Wo = 640); fp32 plan: LDS bound
]
CASES = K10_CASES + K3_CASES


def loop_cases(ncu=256):
    """(entries, case): batches whose work items exceed the persistent grid and are no multiple of it."""
    g4 = min(4 * ncu, 1024)
    return [
        ((("fwd", False, False), ("fwd_x3", False, False), ("fwd_ps", False, False), ("wgrad", False, False),
          ("wgrad_x3", False, False), ("wgrad_x3", True, False)), (10, 5, 64, 478, 480, 0)),      # 300 rows on 256 workgroups
        ((("fwd_x3", False, False), ("wgrad_x3", False, False)), (10, 9, 64, 246, 96, 0)),          # 279 rows, single-tile wgrad
        ((("wgrad", False, False),), (10, 9, 64, 470, 38, 0)),                                      # 531 rows on 512
        ((("wgrad", False, False),), (3, 33, 16, 63, 30, 0)),                                       # 1056 rows on 1024
        # the scalar-fed grid is min(items, 4 CUs, rows, 1024): more rows than that, two segments per row -> ipw = 3, idle tail workgroups
        ((("wgrad", False, False),), (3, g4 // 32 + 1, 16, 64, 136, 0)),
        ((("wgrad_x3", False, False), ("wgrad_x3", True, False)), (3, 3 * ncu // 32 + 1, 16, 64, 32, 0)),
    ]


def case_id(c):
    k, N, F_, H, W, off = c
    even = "-even" if k == 3 and H % 2 == 0 and W % 2 == 0 else ""
    return f"k{k}-{H}x{W}-F{F_}-N{N}" + (f"-off{off}" if off else "") + even


# ----------------------------------------------------------------------------------------------------------------------
# references (float64, CPU), computed once per (case, input kind) and shared by the forms of that case
# ----------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self, case, kind):
        k, N, F_, H, W, _ = case
        self.k, self.s, self.p = k, *(K10[1:] if k == 10 else K3[1:])
        Ho, Wo = out_hw(H, W, k, self.s, self.p)
        g = torch.Generator().manual_seed(((k * 131 + N) * 131 + F_) * 1000003 + H * 2003 + W + (7 if kind == "corner" else 0))
        self.fr = torch.randint(0, 256, (N, 3, H, W), dtype=torch.uint8, generator=g)
        self.x = torch.rand(N, 3, H, W, generator=g)
        if kind == "corner":                               # one non-zero pixel per plane: last row, last column
            v = torch.rand(N, 3, generator=g) + 0.5
            self.x = torch.zeros(N, 3, H, W)
            self.x[:, :, H - 1, W - 1] = v
            self.fr = torch.zeros(N, 3, H, W, dtype=torch.uint8)
            self.fr[:, :, H - 1, W - 1] = torch.randint(1, 256, (N, 3), dtype=torch.uint8, generator=g)
        self.w = torch.randn(F_, 3, k, k, generator=g) * (0.05 if k == 10 else 0.1)
        self.b = torch.randn(F_, generator=g)
        self.dy = torch.randn(N, F_, Ho, Wo, generator=g)
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def y(self, p16=False, u8=False):
        x = self.fr.float() / 255.0 if u8 else self.x
        x, w = (bf(x), bf(self.w)) if p16 else (x, self.w)
        return self._get(("y", p16, u8), lambda: F.conv2d(x.double(), w.double(), self.b.double(), stride=self.s, padding=self.p))

    def dW(self, p16=False):
        x, dy = (bf(self.x), bf(self.dy)) if p16 else (self.x, self.dy)
        return self._get(("dW", p16), lambda: torch.nn.grad.conv2d_weight(x.double(), tuple(self.w.shape), dy.double(),
                                                                          stride=self.s, padding=self.p))

    def db(self, rounded=False):
        dy = bf(self.dy) if rounded else self.dy
        return dy.double().sum(dim=(0, 2, 3))


ERRORS = {}        # route -> worst observed error / bound


def _key(r):
    return "%s/%s%s%s%s" % (r["family"], r["pass"], "/p16" if r["p16"] else "", "/u8" if r["u8"] else "", "/ps" if r["ps"] else "")


def close(got, ref, route, what, tol=1e-4):
    got = got.cpu().double(); ref = ref.cpu().double()
    scale = max(1.0, float(ref.abs().max()))
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = float((got - ref).abs().max())
    ERRORS[_key(route)] = max(ERRORS.get(_key(route), 0.0), err / (tol * scale))
    print(f"{what}: max err {err:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs bound {tol * scale:.3e}"


def close16(got, ref, route, what):
    """close_bf16 (the bound that decides), with the worst error / bound recorded; the ratio restates that bound only
    to report it, and a NaN, which no comparison flags, fails on its own."""
    g, r = got.cpu().double(), ref.cpu().double()
    assert bool(torch.isfinite(g).all()), f"{what}: non-finite output"
    bound = r.abs() * 2.0 ** -8 + 2e-5 * max(1.0, float(r.abs().max()))
    ratio = float(((g - r).abs() / bound).max())
    ERRORS[_key(route)] = max(ERRORS.get(_key(route), 0.0), ratio)
    print(f"{what}: worst error / bound {ratio:.3f}")
    close_bf16(got, ref, what)
    assert ratio <= 1.0, f"{what}: worst error / bound {ratio:.3f}"
    assert torch.equal(got.cpu(), bf(got.cpu())), f"{what}: a precision16 output is not a bf16 value"


@pytest.fixture(scope="module", autouse=True)
def _report():
    """STEM_PATHS_ERRORS_OUT=<file>: append the worst error / bound of every route this process reached."""
    yield
    path = os.environ.get("STEM_PATHS_ERRORS_OUT")
    if path and ERRORS:
        switches = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("FDET_STEM_"))
        with open(path, "a") as f:
            for r in sorted(ERRORS):
                f.write(f"{switches or '(defaults)'}\t{r}\t{ERRORS[r]:.4f}\n")


# ----------------------------------------------------------------------------------------------------------------------
# runners
# ----------------------------------------------------------------------------------------------------------------------
def _check_route(got, exp, what):
    for f in ROUTE_KEYS + ("launches", "items", "grid"):
        assert got[f] == exp[f], f"{what}: route record {got}, expected {exp}"


def _twice(hp, launch, outs, ws, what):
    """NaN-filled outputs, launch, sentinels, launch again: the same bits and the same route.  Returns the first outputs."""
    launch()
    torch.cuda.synchronize()
    got = hp.stem_last_route()
    first = [o.t.clone() for o in outs]
    for o in outs + [ws]:
        assert o.guards_intact(), f"{what}: write outside a buffer"
    for o in outs:
        o.t.fill_(float("nan"))
    launch()
    torch.cuda.synchronize()
    assert hp.stem_last_route() == got, f"{what}: the second run took another route"
    for o, f in zip(outs, first):
        assert o.guards_intact(), f"{what}: write outside the output on the second run"
        assert torch.equal(o.t.view(torch.int32), f.view(torch.int32)), f"{what}: second run differs"
    assert ws.guards_intact(), f"{what}: write outside the workspace"
    return first, got


def _refused(hp, launch, outs, what):
    from fdet_amd import FdetError
    with pytest.raises(FdetError):
        launch()
    torch.cuda.synchronize()
    r = hp.stem_last_route()
    assert r["family"] is None and r["launches"] == 0, f"{what}: a refused call recorded a launch: {r}"
    for o in outs:
        assert o.guards_intact() and bool(o.t.isnan().all()), f"{what}: a refused call wrote its output"


def _ps_zero_slots_ok(ps, y):
    """Every unit that holds no real element (zero slots, zero rows, guard images) is still zero."""
    N, C, H, W = y.shape
    real = ps.PsTensor.from_f32(torch.full((N, C, H, W), 1.0 + 2.0 ** -9, device="cuda"))     # hi and lo both non-zero
    if y.strips > 1:
        ps.halo_exchange(real)
    outside = real.buf.view(torch.int16) == 0
    return int((y.buf.view(torch.int16)[outside] != 0).sum()) == 0


def run_entry(env, case, ref, entry, p16, u8, dev):
    """One entry point on one case: its expected route and values, or its refusal."""
    hp, ps = env
    from fdet_amd import FdetError
    k, N, F_, H, W, off = case
    s, p = ref.s, ref.p
    Ho, Wo = out_hw(H, W, k, s, p)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    exp = expected_stem_route(entry, N, F_, H, W, k, s, p, p16, u8, ncu=ncu)
    what = f"{case_id(case)} {entry}{' p16' if p16 else ''}{' u8' if u8 else ''}"
    xd, wd, bd, ws = dev["x"], dev["w"], dev["b"], dev["ws"]
    if entry in ("fwd", "fwd_x3"):
        y = Placed((N, F_, Ho, Wo), 0)
        launch = lambda: hp.stem_fwd(xd, wd, bd, y.t, ws.t, k, s, p, x3=entry == "fwd_x3")       # noqa: E731
        if exp is None:
            return _refused(hp, launch, [y], what)
        (got,), r = _twice(hp, launch, [y], ws, what)
        close(got, ref.y(), exp, what)
        return _check_route(r, exp, what)
    if entry == "fwd_ps":
        xin = dev["fr"] if u8 else xd
        try:
            ys = [ps.PsTensor(N, F_, Ho, Wo, "cuda") for _ in range(2)]
        except FdetError:
            ys = None                                     # no PS layout for the output at all
        if exp is None:
            # the plan query must refuse too: a call the library wrongly took would write a PS tensor over the stand-in
            assert not hp.stem_fwd_ps_ok(N, 3, F_, H, W, k, s, p, p16=p16, u8=u8), f"{what}: fdet_stem_fwd_ps_ok accepts it"
            dummy = Placed((1 << 20,), 0)
            ydata = ys[0].data if ys else hp.ptr(dummy.t)
            fn = (lambda: hp.check(hp.lib().fdet_stem_fwd_ps_u8(hp.ptr(xin, torch.uint8), hp.ptr(wd), hp.ptr(bd), ydata, N, 3, F_, H, W,
                                                                  k, s, p, int(p16), hp.stream()), "fdet_stem_fwd_ps_u8")) if u8 else \
                 (lambda: hp.check(getattr(hp.lib(), "fdet_stem_fwd_ps" + ("_p16" if p16 else ""))(
                     hp.ptr(xd), hp.ptr(wd), hp.ptr(bd), ydata, N, 3, F_, H, W, k, s, p, hp.stream()), "fdet_stem_fwd_ps"))
            _refused(hp, fn, [dummy], what)
            if ys:
                assert int((ys[0].buf.view(torch.int32) != 0).sum()) == 0, f"{what}: a refused call wrote its output"
            return None
        assert ys is not None, f"{what}: no PS tensor for an output the route expects"
        routes = []
        for y in ys:
            if not p16:                                   # real elements (and strip halos) start as NaN; precision16 leaves lo planes alone
                ps.PsTensor.from_f32(torch.full((N, F_, Ho, Wo), float("nan"), device="cuda"), out=y)
            ps.stem_fwd_ps(xin, wd, bd, y, k, s, p, p16=p16)
            torch.cuda.synchronize()
            routes.append(hp.stem_last_route())
            assert _ps_zero_slots_ok(ps, y), f"{what}: a halo / zero slot of the PS output was written"
        assert routes[0] == routes[1] and torch.equal(ys[0].buf.view(torch.int32), ys[1].buf.view(torch.int32)), f"{what}: second run differs"
        got = ys[0].to_f32()
        if ys[0].strips > 1:                              # the halo slots it wrote are what the exchange writes
            before = ys[0].buf.view(torch.int32).clone()
            ps.halo_exchange(ys[0], p16=p16)
            assert torch.equal(ys[0].buf.view(torch.int32), before), f"{what}: strip halos differ from the exchange's"
        if u8:                                            # bit-equal to the normalisation kernel + the float form
            yr = ps.PsTensor(N, F_, Ho, Wo, "cuda")
            ps.stem_fwd_ps(hp.u8_to_f32_norm(xin), wd, bd, yr, k, s, p, p16=p16)
            assert torch.equal(yr.buf.view(torch.int32), ys[0].buf.view(torch.int32)), f"{what}: differs from u8_to_f32_norm + the float form"
        # the k3 PS forward stays fp32 VALU arithmetic on the unrounded operands in precision16 (ssdstack.py): only the stored value is bf16
        (close16 if p16 else close)(got, ref.y(p16 and exp["family"] != "k3_ps_fwd", u8), exp, what)
        return _check_route(routes[0], exp, what)
    # weight gradients
    dW, db = Placed((F_, 3, k, k), 0), Placed((F_,), 0)
    launch = lambda: hp.stem_wgrad(xd, dev["dy"], dW.t, db.t, ws.t, k, s, p, x3=entry == "wgrad_x3", p16=p16)      # noqa: E731
    if exp is None:
        return _refused(hp, launch, [dW, db], what)
    (gW, gb), r = _twice(hp, launch, [dW, db], ws, what)
    close(gW, ref.dW(p16), exp, what + " dW")
    close(gb, ref.db(rounded=p16 and exp["family"] == "k3_matrix"), exp, what + " db")
    return _check_route(r, exp, what)


def _guarded(src, off=0):
    """A device copy of `src` between NaN bands: a read past the input shows even where its product with a zero is all that
    reaches the result.  off: floats by which the copy is shifted off its 256-byte aligned base."""
    pl = Placed(tuple(src.shape), off, src=src.cuda())
    pl.buf[:GUARD + off] = float("nan")
    pl.buf[GUARD + off + pl.n:] = float("nan")
    return pl.t


def _device_inputs(hp, case, ref):
    k, N, F_, H, W, off = case
    nb = hp.stem_ws_bytes(N, 3, F_, H, W, k, ref.s, ref.p)
    plan = stem_plan(N, F_, H, W, k, ref.s, ref.p)
    assert (nb > 0) == (plan is not None), f"{case_id(case)}: fdet_stem_ws_bytes = {nb}, plan {plan}"
    assert nb % 4 == 0
    ws = Placed((max(nb // 4, 256),), 0)                  # exactly what the library asks for, inside sentinel bands
    return dict(x=_guarded(ref.x, off), fr=ref.fr.cuda(), w=ref.w.cuda(), b=ref.b.cuda(), dy=_guarded(ref.dy), ws=ws)


def run_case(env, case, entries=ENTRIES, kinds=("rand", "corner")):
    hp, _ = env
    for kind in kinds:
        ref = Ref(case, kind)
        dev = _device_inputs(hp, case, ref)
        for entry, p16, u8 in entries:
            run_entry(env, case, ref, entry, p16, u8, dev)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_stem_path(env, case):
    run_case(env, case)


LOOP_IDS = ["rows300on256", "singletile279", "valuk10_531", "generick3_1056", "scalark3_idle", "k3matrix"]      # of loop_cases()


@pytest.mark.parametrize("idx", range(len(LOOP_IDS)), ids=LOOP_IDS)
def test_persistent_loop(env, idx):
    """Work items outnumber the persistent grid and are no multiple of it: the second trip of every row loop, the odd row
    count of the pipelined kernels, workgroups whose share is empty and that must still write a zero slab."""
    hp, _ = env
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    entries, case = loop_cases(ncu)[idx]
    k, N, F_, H, W, _ = case
    s, p = (K10 if k == 10 else K3)[1:]
    for entry, p16, u8 in entries:
        exp = expected_stem_route(entry, N, F_, H, W, k, s, p, p16, u8, ncu=ncu)
        assert exp is not None, f"{case_id(case)} {entry}: refused"
        assert exp["items"] > exp["grid"] and exp["items"] % exp["grid"] != 0, f"{case_id(case)} {entry}: would not loop: {exp}"
    run_case(env, case, entries, kinds=("rand",))
    r = hp.stem_last_route()                               # the record of the last entry, from the library itself
    assert r["items"] > r["grid"] and r["items"] % r["grid"] != 0, f"{case_id(case)}: the last launch did not loop: {r}"


# ----------------------------------------------------------------------------------------------------------------------
# switches read once per process: one child process per switch, a subset of this file
# ----------------------------------------------------------------------------------------------------------------------
_K10_SUBSET = [c for c in K10_CASES if c[3:5] in ((478, 484), (96, 480), (62, 416))]
# (switch, cases of test_stem_path, ids of test_persistent_loop)
SWITCH_GROUPS = [
    ({"FDET_STEM_VALU": "1"}, _K10_SUBSET, []),
    ({"FDET_STEM_PIPE": "0"}, _K10_SUBSET, ["singletile279"]),
    ({"FDET_STEM_K3_GENERIC": "1"}, [c for c in K3_CASES if c[3] % 2 == 0 and c[4] % 2 == 0], []),
]


def test_switch_groups():
    """Each switch re-runs a subset of this file in a fresh process; expected_stem_route reads the same environment, so
    every case there also proves the switch took effect.  A child that fails, times out or dies on a signal fails this
    test at once (no retries, no further children)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "tests", "test_gpu_stem_paths.py")
    for extra, cases, loops in SWITCH_GROUPS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("FDET_") or k == "FDET_LIB_PATH"}
        env.update(extra)
        nodes = [f"{path}::test_stem_path[{case_id(c)}]" for c in cases] + [f"{path}::test_persistent_loop[{i}]" for i in loops]
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider"] + nodes, env=env,
                           capture_output=True, text=True, timeout=600, cwd=root)
        tail = r.stdout[-3000:] + r.stderr[-2000:]
        assert r.returncode == 0 and f"{len(nodes)} passed" in r.stdout, f"{extra}: exit {r.returncode}\n{tail}"
