"""GPU tests of precision16 on the SSD engine: the one-pass pointwise GEMMs (fdet_pointwise_*_bf16) and SSDStack in
precision16, the arithmetic of the reference's SSD recipe (train_model_ssd.py:13-15,46-55: SSD(filters=16), 480x480,
Trainer(precision=16)).

Kernel level: against torch on operands rounded to bf16 (activations as loaded, weights as the hi half of the packed panel):
what is left is fp32 summation order and ONE bf16 rounding of each stored value -- one bf16 ulp of the rounded reference plus
1e-6 of the tensor's scale, and every stored value is a bf16 number.  Weight / bias gradients are fp32 sums of bf16
products: 1e-4 of the tensor's scale.
Model level: the fixture g19 = the reference SSD(filters=16) train step under torch.autocast("cpu", bfloat16)
(tools/make_goldens_r6.py), with the output and loss bounds of the F=128 fixture g18 (tests/test_gpu_p16_wide.py) and
wider per-tensor gradient bounds (the fixture's own bf16 noise; see the test's docstring)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZE = 480

# (N, Cin, Cout, H, W): the four skip convs of SSD(16), the four Linear(C,5) heads, an odd plane (P = 37) and odd channels
PW_SHAPES = [(2, 16, 32, 240, 240), (2, 32, 64, 60, 60), (2, 64, 128, 60, 60), (2, 128, 256, 60, 60),
             (2, 128, 5, 60, 60), (3, 256, 5, 30, 30), (3, 256, 5, 15, 15), (3, 256, 5, 7, 7),
             (3, 40, 24, 1, 37)]


@pytest.fixture(scope="module")
def hp():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath
    return hotpath


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def bf16_ulp(v):
    """Spacing of bf16 numbers at |v| (8 significant bits)."""
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), e - 8)


def close_bf16(got, ref, what=""):
    """`got` holds bf16 numbers, each within one bf16 ulp of bf16(ref) plus 1e-6 of the tensor's scale."""
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    assert torch.equal(got.float(), bf(got.float())), f"{what}: stored values are not bf16 numbers"
    rr = bf(ref.float()).double()
    scale = max(1.0, float(ref.abs().max()))
    err = (got - rr).abs()
    bound = bf16_ulp(rr) + 1e-6 * scale
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} entries off, worst {float((err - bound).max()):.3e} over the bound"


def close(a, b, tol=1e-4, what=""):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * scale, f"{what}: max err {err} vs scale {scale}"


def _pw_data(shape, seed):
    N, ci, co, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ci, H, W, generator=g)
    w = torch.randn(co, ci, generator=g) / ci ** 0.5
    b = torch.randn(co, generator=g)
    return g, x, w, b


def _gemm(w, x):
    """(co,ci) x (N,ci,H,W) -> (N,co,H,W) in float64."""
    return torch.einsum("oc,nchw->nohw", w.double(), x.double())


@pytest.mark.parametrize("shape", PW_SHAPES)
def test_p16_pointwise_fwd(hp, shape):
    N, ci, co, H, W = shape
    g, x, w, b = _pw_data(shape, N * 1000 + ci + co + H)
    wf, _ = hp.pointwise_pack(w.cuda())
    xc = x.cuda()
    z = _gemm(bf(w), bf(x))
    for bias, slope in ((b, 1.0), (None, 1.0), (b, 0.2)):
        ref = z + (bias.double()[None, :, None, None] if bias is not None else 0.0)
        ref = torch.where(ref > 0, ref, ref * slope)
        y = torch.full((N, co, H, W), float("nan"), device="cuda")
        hp.pointwise_fwd(xc, wf, bias.cuda() if bias is not None else None, y, slope=slope, p16=True)
        close_bf16(y, ref, f"y (bias {bias is not None}, slope {slope})")
        # the bf16x3 entry of the same call is unchanged: fp32-grade against the unrounded operands
        y3 = torch.full_like(y, float("nan"))
        hp.pointwise_fwd(xc, wf, bias.cuda() if bias is not None else None, y3, slope=slope)
        r3 = _gemm(w, x) + (bias.double()[None, :, None, None] if bias is not None else 0.0)
        close(y3, torch.where(r3 > 0, r3, r3 * slope), 2e-5, "bf16x3 y")
        assert not torch.equal(y, y3)


@pytest.mark.parametrize("shape", PW_SHAPES)
def test_p16_pointwise_dgrad(hp, shape):
    N, ci, co, H, W = shape
    g, _, w, _ = _pw_data(shape, N * 77 + ci + co + H)
    dz = torch.randn(N, co, H, W, generator=g)
    add = torch.randn(N, ci, H, W, generator=g)
    _, wb = hp.pointwise_pack(w.cuda())
    t = _gemm(bf(w).t(), bf(dz))
    for a in (None, add):
        dx = torch.full((N, ci, H, W), float("nan"), device="cuda")
        hp.pointwise_dgrad(dz.cuda(), wb, dx, add=a.cuda() if a is not None else None, p16=True)
        close_bf16(dx, t + (a.double() if a is not None else 0.0), f"dx (add {a is not None})")
        dx3 = torch.full_like(dx, float("nan"))
        hp.pointwise_dgrad(dz.cuda(), wb, dx3, add=a.cuda() if a is not None else None)
        close(dx3, _gemm(w.t(), dz) + (a.double() if a is not None else 0.0), 2e-5, "bf16x3 dx")


@pytest.mark.parametrize("shape", PW_SHAPES)
def test_p16_pointwise_wgrad(hp, shape):
    N, ci, co, H, W = shape
    g = torch.Generator().manual_seed(N * 31 + ci + co + H)
    x = torch.randn(N, ci, H, W, generator=g)
    dz = torch.randn(N, co, H, W, generator=g)
    dW_ref = torch.einsum("nohw,nchw->oc", bf(dz).double(), bf(x).double())
    db_ref = bf(dz).double().sum(dim=(0, 2, 3))
    for want_b in (True, False):
        dW = torch.full((co, ci), float("nan"), device="cuda")
        db = torch.full((co,), float("nan"), device="cuda") if want_b else None
        hp.pointwise_wgrad(x.cuda(), dz.cuda(), dW, db, p16=True)
        close(dW, dW_ref, 1e-4, "dW")
        if want_b:
            close(db, db_ref, 1e-4, "db")
    dW3 = torch.full((co, ci), float("nan"), device="cuda"); db3 = torch.full((co,), float("nan"), device="cuda")
    hp.pointwise_wgrad(x.cuda(), dz.cuda(), dW3, db3)
    close(dW3, torch.einsum("nohw,nchw->oc", dz.double(), x.double()), 2e-5, "bf16x3 dW")
    close(db3, dz.double().sum(dim=(0, 2, 3)), 2e-5, "bf16x3 db")


def test_p16_ssd_stem_wgrad(hp):
    """The SSD stem (Conv(3,16,3,s2,p1) at 480^2) weight gradient in precision16: fdet_stem_wgrad_bf16 on the k3 matrix-core
    kernel, fp32 sums of bf16 products (1e-4 of the scale); the bf16x3 call is unchanged (fp32-grade)."""
    N, F_, S = 2, 16, SIZE
    assert hp.stem_k3_wgrad_x3_supported(3, F_, S, S, 3, 2, 1)
    g = torch.Generator().manual_seed(17)
    x = torch.rand(N, 3, S, S, generator=g)
    dy = torch.randn(N, F_, S // 2, S // 2, generator=g)
    ws = torch.empty(hp.stem_ws_bytes(N, 3, F_, S, S, 3, 2, 1) // 4 + 4, device="cuda")
    res = {}
    for p16 in (True, False):
        dW = torch.full((F_, 3, 3, 3), float("nan"), device="cuda"); db = torch.full((F_,), float("nan"), device="cuda")
        hp.stem_wgrad(x.cuda(), dy.cuda(), dW, db, ws, 3, 2, 1, x3=True, p16=p16)
        xr, dr = (bf(x), bf(dy)) if p16 else (x, dy)
        close(dW, torch.nn.grad.conv2d_weight(xr.double(), (F_, 3, 3, 3), dr.double(), stride=2, padding=1), 1e-4 if p16 else 2e-5, "dW")
        close(db, dr.double().sum(dim=(0, 2, 3)), 1e-4 if p16 else 2e-5, "db")
        res[p16] = dW.cpu()
    assert not torch.equal(res[True], res[False])


# ---------------------------------------------------------------------------------------------------------------- model
def _ssd_model(P, mode, log_path="out.log"):
    from fdet_amd.models.ModelMetaSSD import ModelMetaSSD
    from fdet_amd.models.SSD import SSD
    model = SSD(filters=16, input_shape=(3, SIZE, SIZE))
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().train()
    model.engine.set_precision(mode)
    mm = ModelMetaSSD(model=model, lr=1e-4, log_path=log_path)
    mm.configure_optimizers()
    return model, mm


def _grads(mm, model):
    sp = mm.opt._space()
    names, _ = model.named_stack_params()
    return {n: sp.view(sp.grad, i).detach().clone() for i, n in enumerate(names)}


def test_p16_ssd_train_step_vs_reference_autocast_fixture(golden):
    """g19: the reference SSD(filters=16), one train step at B=2 with ssd_loss(..., 10) under torch.autocast("cpu", bfloat16).
    The engine in precision16 on the same inputs, parameters (by seed) and dropout masks, through fused_train_step: score
    column within 2e-2 absolute, box columns within 2e-2 of their scale, loss within 2 % (g18's bounds).

    Per-tensor gradient bounds WIDENED from g18's (norm 5 %, cosine 0.99) to norm 12 %, cosine 0.97, plus a cosine >= 0.995
    of all sampled entries together.  Reason: the fixture's own bf16 noise.  The exact-fp32 gradient of the same step (the
    CPU oracle, oracle/ssd_model_oracle.py, same inputs, parameters and masks) is itself only at cosine 0.985 to the fixture
    on feature_extractor.2.conv1.weight, and 4 tensors differ from the fixture's norms by more than 5 % (up to 7.5 %, the
    32-channel 60x60 blocks feature_extractor.5 / .6), while its loss (1e-4), outputs (2e-3) and sampled entries taken
    together (cosine 0.9989) agree.  Hard-negative selection is not the cause: the losses agree to 1e-4.  g18's bounds would
    reject the exact answer; the widened ones admit it with a margin for the engine's own bf16 rounding."""
    import fdet_amd  # noqa: F401
    from oracle import ssd_model_oracle as SM
    g = golden("g19_ssd_F16_ac")
    P = SM.init_params(int(g["filters"]), int(g["param_seed"]))
    names = [str(n) for n in g["names"]]
    assert [float(P[n].double().sum()) for n in names] == pytest.approx(list(g["param_sum"]), rel=1e-6, abs=1e-6)
    model, mm = _ssd_model(P, "bf16")
    assert model.engine.p16
    x_u8 = torch.randint(0, 256, (2, 3, SIZE, SIZE), generator=torch.Generator().manual_seed(int(g["x_seed"])), dtype=torch.uint8)
    assert int(x_u8.long().sum()) == int(g["x_sum"])
    model.set_dropout_masks({k[len("mask/"):]: v for k, v in g.items() if k.startswith("mask/")})
    loss, y_hat = mm.fused_train_step((x_u8.float() / 255.0).cuda(), g["y"].cuda())
    y_hat, ref = y_hat.cpu(), g["y_train"]
    assert float((y_hat[..., 0] - ref[..., 0]).abs().max()) <= 2e-2
    box_scale = max(1.0, float(ref[..., 1:].abs().max()))
    assert float((y_hat[..., 1:] - ref[..., 1:]).abs().max()) <= 2e-2 * box_scale
    assert abs(float(loss) - float(g["loss"])) <= 2e-2 * float(g["loss"])
    G = _grads(mm, model)
    sa, sb = [], []
    for i, n in enumerate(names):
        got = G[n].cpu().double().reshape(-1)
        gr = g["grad/" + n].double()
        idx = g["idx/" + n].long()
        assert abs(float(got.norm()) - float(g["grad_norm"][i])) <= 0.12 * float(g["grad_norm"][i]), n
        cos = float((got[idx] * gr).sum() / (got[idx].norm() * gr.norm()).clamp_min(1e-30))
        assert cos >= 0.97, (n, cos)
        sa.append(got[idx]); sb.append(gr)
    sa, sb = torch.cat(sa), torch.cat(sb)
    assert float((sa * sb).sum() / (sa.norm() * sb.norm())) >= 0.995


def _ssd_step(mode, B=2):
    from oracle import ssd_model_oracle as SM
    from oracle import ssd_oracle as S
    import oracle as O
    P = SM.init_params(16, seed=4)
    model, mm = _ssd_model(P, mode)
    x = torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(8)).cuda()
    boxes = O.synthetic_boxes(B, SIZE, seed=6, max_faces=5)
    y = torch.stack([S.ssd_encode(b if b.numel() else torch.tensor([]), (SIZE, SIZE)) for b in boxes]).cuda()
    model.set_dropout_masks(SM.make_dropout_masks(16, B, seed=5))
    loss, y_hat = mm.fused_train_step(x, y)
    return float(loss), y_hat.clone(), mm.opt._space().grad.clone()


def test_p16_ssd_equals_fp32_grade_path_within_bf16():
    """The same SSD step in the default bf16x3 arithmetic and in precision16: loss within 2 %, outputs within 2e-2 of their
    scale, gradient cosine >= 0.995, and the gradients differ (the one-pass kernels did run)."""
    import fdet_amd  # noqa: F401
    (la, ya, ga), (lb, yb, gb) = _ssd_step("bf16x3"), _ssd_step("bf16")
    assert abs(la - lb) <= 2e-2 * abs(la), (la, lb)
    assert float((ya - yb).abs().max()) <= 2e-2 * max(1.0, float(ya.abs().max()))
    assert not torch.equal(ga, gb)
    cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
    assert cos >= 0.995, cos


def test_ssd_set_precision_between_forward_and_backward_is_honoured():
    """A pass saved in one precision is differentiated in that precision, whatever set_precision() says by then."""
    import fdet_amd  # noqa: F401
    from oracle import ssd_model_oracle as SM
    from fdet_amd.ssdstack import SSDStack
    B = 2
    P = {k: v.cuda().contiguous() for k, v in SM.init_params(16, seed=2).items()}
    eng = SSDStack(16)
    masks = {k: v.cuda() for k, v in SM.make_dropout_masks(16, B, seed=7).items()}
    x = torch.rand(B, 3, SIZE, SIZE, generator=torch.Generator().manual_seed(3)).cuda()
    dy = (torch.randn(B, eng.P, 5, generator=torch.Generator().manual_seed(4)) * 1e-2).cuda()

    def grads(fwd_mode, bwd_mode):
        eng.set_precision(fwd_mode)
        _, saved = eng.forward(x, P, masks, save=True)
        eng.set_precision(bwd_mode)
        G = {k: torch.full_like(v, float("nan")) for k, v in P.items()}
        eng.backward(saved, dy, P, G)
        torch.cuda.synchronize()
        return torch.cat([G[k].reshape(-1) for k in sorted(G)])

    res = {}
    for fwd_mode, other in (("bf16", "bf16x3"), ("bf16x3", "bf16")):
        same = grads(fwd_mode, fwd_mode)
        switched = grads(fwd_mode, other)
        assert eng.p16 == (other == "bf16")               # the setting itself is kept for the next pass
        assert torch.isfinite(switched).all()
        assert torch.allclose(switched, same, rtol=1e-6, atol=1e-9), fwd_mode
        res[fwd_mode] = same
    assert not torch.equal(res["bf16"], res["bf16x3"])


def test_reference_recipe_train_model_ssd_precision16(monkeypatch, tmp_path):
    """train_model_ssd.py --precision 16 with its defaults (SSD(16), 480x480, batch 24): the reference's recipe.  Finite
    losses, every parameter moved, every conv / pointwise launch at the hot-path layer ran in precision16, and the --save
    TorchScript file is written."""
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, train_model_ssd, trainer
    monkeypatch.chdir(tmp_path)
    calls = {"p16": 0, "x3": 0}

    def counting(fn):
        def wrapped(*a, **k):
            calls["p16" if k.get("p16") else "x3"] += 1
            return fn(*a, **k)
        return wrapped
    for name in ("conv3x3_fwd", "conv3x3_dgrad", "conv3x3_wgrad", "conv3x3_wgrad_batched", "pointwise_fwd", "pointwise_dgrad",
                 "pointwise_wgrad", "stem_wgrad"):
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
    save = tmp_path / "ssd.pt"
    hist = train_model_ssd.main(["--precision", "16", "--epochs", "1", "--steps-per-epoch", "3", "--val-steps", "1",
                                 "--save", str(save)])
    eng = seen["engine"]
    assert eng.filters == 16 and eng.p16
    losses = [float(h["loss"]) for h in hist["train"] + hist["val"]]
    assert losses and all(torch.isfinite(torch.tensor(losses))), losses
    moved = [n for n in seen["before"] if not torch.equal(seen["before"][n], seen["after"][n])]
    assert len(moved) == len(seen["before"]), f"parameters unchanged: {set(seen['before']) - set(moved)}"
    assert calls["p16"] > 0 and calls["x3"] == 0, calls
    assert save.exists() and save.stat().st_size > 0
    assert (tmp_path / "logs" / "out_ssd_16_480x480_sam_adam.log").exists()


def test_trainer_fit_drives_modelmeta_ssd(tmp_path):
    """trainer.fit on a ModelMetaSSD (default precision): uint8 host frames through U8BatchFeeder, targets (B,4774,5); the
    first step's loss equals a direct fused_train_step on the same batch, parameters and dropout masks."""
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    from fdet_amd.trainer import fit
    from oracle import ssd_model_oracle as SM
    import oracle as O
    B = 2
    P = SM.init_params(16, seed=9)
    masks = SM.make_dropout_masks(16, B, seed=10)
    x_u8 = torch.randint(0, 256, (B, 3, SIZE, SIZE), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    boxes = O.synthetic_boxes(B, SIZE, seed=12, max_faces=4)
    y = hp.ssd_encode_targets(boxes, (SIZE, SIZE)).cpu()
    assert tuple(y.shape) == (B, 4774, 5)

    model_a, mm_a = _ssd_model(P, "bf16x3", tmp_path / "out.log")
    model_a.set_dropout_masks(masks)
    steps = []
    hist = fit(mm_a, [(x_u8, y, boxes)], [(x_u8, y, boxes)], epochs=1,
               on_step=lambda i, train, out: steps.append((train, float(out["loss"]))))
    assert [t for t, _ in steps] == [True, False]
    assert set(hist["train"][0]) >= {"loss", "total_iou", "total_recall", "total_precision", "f1_score"}
    assert len(hist["val"]) == 1

    model_b, mm_b = _ssd_model(P, "bf16x3")
    model_b.set_dropout_masks(masks)
    x = hp.u8_to_f32_norm(x_u8.cuda())
    loss, _ = mm_b.fused_train_step(x, y.cuda())
    assert abs(steps[0][1] - float(loss)) <= 1e-6 * abs(float(loss)), (steps[0][1], float(loss))
