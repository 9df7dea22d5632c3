"""GPU tests of precision16 on the fp32-I/O conv kernels (the `_bf16` entries of include/fdet.h): the kernels PoolResnet-large
(F=128, the reference's own training recipe, train_model.py:15-17,50) runs, and every other width that is a multiple of 16.

Kernel level: against torch CPU ops on operands rounded to bf16 (activations as loaded, weights as the hi half of the packed
panel): the only differences left are fp32 summation order and ONE bf16 rounding of each stored value -- bound
2^-8 |ref| + 2e-5 scale, and every stored value is a bf16 number.  Weight / bias gradients are fp32 sums of bf16 products:
the usual 1e-4 of the tensor's scale against conv2d_weight of the rounded operands.
Model level: the fixture g18 = the reference PoolResnet(filters=128) train step under torch.autocast("cpu", bfloat16)
(tools/make_goldens_r5.py), with the tolerances of the F=64 fixture g17 (tests/test_gpu_p16.py)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, C, H, W): 60 / 30 / 15 columns of F=128 (odd batch included), a 32-channel map, a 16-channel one (GENERIC epilogue),
# and rows wider than 64 columns (the general persistent kernel, float4 and float2 rows)
UNPOOLED = [(2, 128, 60, 60), (3, 128, 30, 30), (5, 128, 15, 15), (7, 128, 15, 15), (2, 32, 30, 30), (3, 16, 60, 60),
            (2, 32, 10, 96), (2, 16, 6, 70)]
POOLED = [(2, 128, 60, 60), (3, 128, 30, 30)]
WGRAD = [s for s in UNPOOLED if s != (2, 16, 6, 70)]      # (rows of 35 float2 lanes have no bf16x3 weight-gradient plan)


@pytest.fixture(scope="module")
def hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def close_bf16(got, ref, what=""):
    """`got` holds bf16-rounded values of (approximately) `ref`."""
    got = got.cpu().double(); ref = ref.cpu().double()
    assert torch.equal(got.float(), bf(got.float())), f"{what}: stored values are not bf16 numbers"
    scale = max(1.0, float(ref.abs().max()))
    err = (got - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 2e-5 * scale
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries off, worst {float((err - bound).max()):.3e} over the bound"


def close(a, b, tol=1e-4):
    a = a.cpu().double(); b = b.cpu().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"max err {err} vs scale {scale}"


def _pack(hp, w):
    cout, cin = w.shape[:2]
    nf, nb = hp.packed_sizes(cout, cin)
    wf = torch.empty(nf, device="cuda"); wb = torch.empty(nb, device="cuda")
    hp.pack_conv3x3_weights(w.cuda(), wf, wb, x3=True)
    return wf, wb


def _data(shape, seed):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    t = lambda *s: torch.randn(*s, generator=g)
    return g, t(N, C, H, W), t(C, C, 3, 3) * (0.3 / C ** 0.5), t(C)


@pytest.mark.parametrize("shape", UNPOOLED)
def test_p16_fwd_modes(hp, shape):
    N, C, H, W = shape
    g, x, w, b = _data(shape, N * 1000 + C + H + W)
    skip = torch.randn(N, C, H, W, generator=g)
    sc = torch.where(torch.rand(N, C, generator=g) < 0.5, 0.0, 2.0)
    wf, _ = _pack(hp, w)
    z = F.leaky_relu(F.conv2d(bf(x).double(), bf(w).double(), b.double(), padding=1), 0.2)
    xc, bc, sk = x.cuda(), b.cuda(), skip.cuda()
    y = torch.full((N, C, H, W), float("nan"), device="cuda")
    hp.conv3x3_fwd(xc, wf, bc, C, y_full=y, slope=0.2, x3=True, p16=True)                           # lrelu(conv + b)
    close_bf16(y, z, "y_full")
    y2, o2 = torch.full_like(y, float("nan")), torch.full_like(y, float("nan"))
    hp.conv3x3_fwd(xc, wf, bc, C, y_full=y2, skip=sk, drop_scale=sc.cuda(), y_out=o2, slope=0.2, x3=True, p16=True)
    close_bf16(y2, z, "y_full (training tail)")
    close_bf16(o2, z * sc.double()[:, :, None, None] + skip.double(), "y_out (training tail)")
    o3 = torch.full_like(y, float("nan"))
    hp.conv3x3_fwd(xc, wf, bc, C, skip=sk, y_out=o3, slope=0.2, x3=True, p16=True)                   # eval tail
    close_bf16(o3, z + skip.double(), "y_out (eval tail)")


@pytest.mark.parametrize("shape", UNPOOLED)
def test_p16_dgrad_modes(hp, shape):
    N, C, H, W = shape
    g, dz, w, _ = _data(shape, N * 77 + C + H + W)
    act = torch.randn(N, C, H, W, generator=g)
    add = torch.randn(N, C, H, W, generator=g)
    _, wb = _pack(hp, w)
    t = F.conv_transpose2d(bf(dz).double(), bf(w).double(), padding=1)
    dx = torch.full((N, C, H, W), float("nan"), device="cuda")
    hp.conv3x3_dgrad(dz.cuda(), wb, C, dx, act=act.cuda(), slope=0.2, x3=True, p16=True)
    close_bf16(dx, t * torch.where(act > 0, 1.0, 0.2).double(), "dx (lrelu')")
    dx2 = torch.full_like(dx, float("nan"))
    hp.conv3x3_dgrad(dz.cuda(), wb, C, dx2, add=add.cuda(), slope=0.2, x3=True, p16=True)
    close_bf16(dx2, t + add.double(), "dx (+ add)")


@pytest.mark.parametrize("shape", WGRAD)
def test_p16_wgrad_single_and_batched(hp, shape):
    N, C, H, W = shape
    assert hp.wgrad_x3_supported(N, C, C, H, W)
    g = torch.Generator().manual_seed(N * 31 + C + H + W)
    L = 2
    xs = [torch.randn(N, C, H, W, generator=g) for _ in range(L)]
    dzs = [torch.randn(N, C, H, W, generator=g) for _ in range(L)]
    refs = [(torch.nn.grad.conv2d_weight(bf(x).double(), (C, C, 3, 3), bf(z).double(), padding=1), bf(z).double().sum(dim=(0, 2, 3)))
            for x, z in zip(xs, dzs)]
    ws = torch.empty(hp.conv3x3_wgrad_ws_bytes(N, C, C, H, W) // 4 + 4, device="cuda")
    dW = torch.full((C, C, 3, 3), float("nan"), device="cuda"); db = torch.full((C,), float("nan"), device="cuda")
    hp.conv3x3_wgrad(xs[0].cuda(), dzs[0].cuda(), dW, db, ws, x3=True, p16=True)
    close(dW, refs[0][0]); close(db, refs[0][1])
    wsb = torch.empty(hp.conv3x3_wgrad_batched_ws_bytes(L, N, C, C, H, W) // 4 + 4, device="cuda")
    dWs = [torch.full((C, C, 3, 3), float("nan"), device="cuda") for _ in range(L)]
    dbs = [torch.full((C,), float("nan"), device="cuda") for _ in range(L)]
    hp.conv3x3_wgrad_batched([x.cuda() for x in xs], [z.cuda() for z in dzs], dWs, dbs, wsb, p16=True)
    for l in range(L):
        close(dWs[l], refs[l][0]); close(dbs[l], refs[l][1])


def _unpool(dout, route):
    """dx contribution of the pooled gradient: window (i, j) sends dout to element arg = (route >> 4) & 3 of its 2x2 block."""
    arg = (route.long() >> 4) & 3
    N, C, Hp, Wp = dout.shape
    out = torch.zeros(N, C, Hp, 2, Wp, 2, dtype=dout.dtype)
    for a in range(4):
        out[:, :, :, a // 2, :, a % 2] = torch.where(arg == a, dout, torch.zeros_like(dout))
    return out.reshape(N, C, 2 * Hp, 2 * Wp)


@pytest.mark.parametrize("shape", POOLED)
def test_p16_pooled_pair(hp, shape):
    N, C, H, W = shape
    g, x, w, b = _data(shape, N * 13 + C + H + W)
    x, w = bf(x), bf(w)                                   # bf16-valued operands: the bf16x3 kernel sees the same products
    skip = torch.randn(N, C, H, W, generator=g)
    sc = torch.where(torch.rand(N, C, generator=g) < 0.5, 0.0, 2.0)
    wf, wb = _pack(hp, w)
    args = (x.cuda(), wf, b.cuda(), skip.cuda(), sc.cuda())
    out = torch.full((N, C, H // 2, W // 2), float("nan"), device="cuda")
    route = torch.empty(N, C, H // 2, W // 2, dtype=torch.uint8, device="cuda")
    hp.conv3x3_fwd_pool(*args, out, route, 0.2, p16=True)
    out3, route3 = torch.empty_like(out), torch.empty_like(route)
    hp.conv3x3_fwd_pool(*args, out3, route3, 0.2)
    assert torch.equal(route.cpu(), route3.cpu()), "routing bytes differ from the bf16x3 kernel's"
    assert torch.equal(out.cpu(), bf(out3.cpu())), "pooled output is not the bf16 rounding of the bf16x3 kernel's"
    v = F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), padding=1), 0.2) * sc.double()[:, :, None, None] + skip.double()
    close_bf16(out, F.max_pool2d(v, 2), "pooled forward")
    # un-pool data gradient: dx = conv^T(dz) + unpool(dout) through those routing bytes
    dz = torch.randn(N, C, H, W, generator=g)
    dout = torch.randn(N, C, H // 2, W // 2, generator=g)
    dx = torch.full((N, C, H, W), float("nan"), device="cuda")
    hp.conv3x3_dgrad_unpool(dz.cuda(), wb, C, dout.cuda(), route, dx, 0.2, p16=True)
    ref = F.conv_transpose2d(bf(dz).double(), w.double(), padding=1) + _unpool(dout.double(), route.cpu())
    close_bf16(dx, ref, "un-pool data gradient")


# ---------------------------------------------------------------------------------------------------------------- model
def _redraw_u8(B, size, seed, checksum):
    x_u8 = torch.randint(0, 256, (B, 3, size, size), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    assert int(x_u8.long().sum()) == int(checksum)
    return x_u8


def test_p16_F128_train_step_vs_reference_autocast_fixture(golden):
    """g18: the reference PoolResnet(filters=128), one train step at B=2 under torch.autocast("cpu", bfloat16).  The engine in
    precision16 on the same inputs, parameters (by seed) and dropout masks: y within 2e-2 absolute (sigmoid outputs),
    loss within 2 %, every gradient tensor's norm within 5 % and its direction (cosine on the fixture's sample) >= 0.99."""
    import fdet_amd  # noqa: F401
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    g = golden("g18_poolresnet_F128_ac")
    torch.manual_seed(int(g["param_seed"]))
    model = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10, num_of_residual_blocks=10).cuda().train()
    eng = model.engine
    eng.set_precision("bf16")
    assert eng.p16 and eng.x3 and not eng.ps
    mm = ModelMeta(model=model, lr=1e-4)
    mm.configure_optimizers()
    x_u8 = _redraw_u8(2, 480, int(g["x_seed"]), g["x_sum"])
    model.set_dropout_masks({k[len("mask/"):]: v for k, v in g.items() if k.startswith("mask/")})
    lsum, y_hat, _ = mm.fused_train_step((x_u8.float() / 255.0).cuda(), g["y"].cuda())
    assert float((y_hat.cpu() - g["y_train"]).abs().max()) <= 2e-2
    assert abs(float(lsum) - float(g["loss"])) <= 2e-2 * float(g["loss"])
    sp = mm.opt.space
    names, _ = model.named_stack_params()
    for i, n in enumerate(names):
        got = sp.view(sp.grad, i).detach().cpu().double().reshape(-1)
        ref = g["grad/" + n].double()
        idx = g["idx/" + n].long()
        assert abs(float(got.norm()) - float(g["grad_norm"][i])) <= 5e-2 * float(g["grad_norm"][i]), n
        cos = float((got[idx] * ref).sum() / (got[idx].norm() * ref.norm()).clamp_min(1e-30))
        assert cos >= 0.99, (n, cos)


def _F128_step(mode, B=2, seed=4):
    import oracle as O
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    spec = O.poolresnet_spec(128, (3, 480, 480), 10)
    P = O.init_params(spec, seed=seed)
    x = torch.rand(B, 3, 480, 480, generator=torch.Generator().manual_seed(8)).cuda()
    y = torch.stack([O.encode_targets(b, (480, 480), 10) for b in O.synthetic_boxes(B, 480, seed=6)]).cuda()
    masks = O.make_dropout_masks(spec, B, seed=5)
    model = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().train()
    model.engine.set_precision(mode)
    mm = ModelMeta(model=model, lr=1e-4); mm.configure_optimizers()
    model.set_dropout_masks(masks)
    lsum, y_hat, _ = mm.fused_train_step(x, y)
    return float(lsum), y_hat.clone(), mm.opt.space.grad.clone()


def test_p16_F128_equals_fp32_grade_path_within_bf16():
    """The same F=128 step in the default bf16x3 arithmetic and in precision16: loss within 2 %, outputs within 2e-2,
    gradient cosine >= 0.995."""
    import fdet_amd  # noqa: F401
    (la, ya, ga), (lb, yb, gb) = _F128_step("bf16x3"), _F128_step("bf16")
    assert abs(la - lb) <= 2e-2 * abs(la), (la, lb)
    assert float((ya - yb).abs().max()) <= 2e-2
    assert not torch.equal(ga, gb)                         # the one-pass kernels did run
    cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
    assert cos >= 0.995, cos


def test_fdet_precision_env_selects_p16_at_F128():
    """FDET_PRECISION=bf16 is read when the engine is built: checked in a child process."""
    code = ("import fdet_amd\nfrom fdet_amd.models.PoolResnet import PoolResnet\n"
            "e = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10).cuda().engine\n"
            "print('P16', int(e.p16), int(e.x3), int(e.ps))\n")
    env = dict(os.environ, FDET_PRECISION="bf16")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "P16 1 1 0" in r.stdout, r.stdout


def test_set_precision_between_forward_and_backward_is_honoured():
    """A pass saved in one precision is differentiated in that precision, whatever set_precision() says by then."""
    import fdet_amd  # noqa: F401
    import oracle as O
    from fdet_amd.models.PoolResnet import PoolResnet
    B = 2
    model = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10)
    model.load_state_dict({k: v.clone() for k, v in O.init_params(O.poolresnet_spec(128, (3, 480, 480), 10), seed=2).items()})
    model = model.cuda().train()
    eng = model.engine
    P = {k: v.detach().contiguous() for k, v in model.state_dict().items()}
    x = torch.rand(B, 3, 480, 480, generator=torch.Generator().manual_seed(3)).cuda()
    dy = (torch.randn(B, 5, 10, 10, generator=torch.Generator().manual_seed(4)) * 1e-2).cuda()

    def grads(fwd_mode, bwd_mode):
        eng.set_precision(fwd_mode)
        _, saved = eng.forward(x, P, None, save=True)
        eng.set_precision(bwd_mode)
        G = {k: torch.full_like(v, float("nan")) for k, v in P.items()}
        eng.backward(saved, dy, P, G)
        torch.cuda.synchronize()
        return torch.cat([G[k].reshape(-1) for k in sorted(G)])

    for fwd_mode, other in (("bf16", "bf16x3"), ("bf16x3", "bf16")):
        same = grads(fwd_mode, fwd_mode)
        switched = grads(fwd_mode, other)
        assert eng.p16 == (other == "bf16")               # the setting itself is kept for the next pass
        assert torch.isfinite(switched).all()
        assert torch.allclose(switched, same, rtol=1e-6, atol=1e-9), fwd_mode
    eng.set_precision("bf16x3")


def test_reference_recipe_train_model_precision16(monkeypatch, tmp_path):
    """train_model.py --precision 16 with its defaults (F=128, S=10, batch 8): the reference's own recipe.  Finite losses,
    parameters moved, and the one-pass kernels ran (p16 launches counted at the hot-path layer)."""
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, train_model, trainer
    monkeypatch.chdir(tmp_path)
    calls = {"p16": 0, "x3": 0}

    def counting(fn):
        def wrapped(*a, **k):
            calls["p16" if k.get("p16") else "x3"] += 1
            return fn(*a, **k)
        return wrapped
    for name in ("conv3x3_fwd", "conv3x3_fwd_pool", "conv3x3_dgrad", "conv3x3_dgrad_unpool", "conv3x3_wgrad_batched"):
        monkeypatch.setattr(hotpath, name, counting(getattr(hotpath, name)))
    seen = {}
    real_fit = trainer.fit

    def fit(model_meta, *a, **k):
        m = model_meta.model
        seen["engine"] = m.engine
        seen["before"] = {n: p.detach().clone() for n, p in m.named_parameters()}
        out = real_fit(model_meta, *a, **k)
        seen["after"] = {n: p.detach().clone() for n, p in m.named_parameters()}
        return out
    monkeypatch.setattr(trainer, "fit", fit)
    hist = train_model.main(["--precision", "16", "--epochs", "1", "--steps-per-epoch", "3", "--val-steps", "1"])
    eng = seen["engine"]
    assert eng.geo.filters == 128 and eng.p16 and not eng.ps
    losses = [float(h["loss"]) for h in hist["train"]]
    assert losses and all(torch.isfinite(torch.tensor(losses))), losses
    moved = [n for n in seen["before"] if not torch.equal(seen["before"][n], seen["after"][n])]
    assert len(moved) == len(seen["before"]), f"parameters unchanged: {set(seen['before']) - set(moved)}"
    assert calls["p16"] > 0 and calls["x3"] == 0, calls
