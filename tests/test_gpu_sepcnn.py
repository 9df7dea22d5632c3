"""SeparableCNN on the GPU: the fused separable-block kernel against a float64 restatement, against the composed launches
it replaces, and the model surface against the reference's numbers (fixture g20, tools/make_goldens_r7.py).
Bounds: bf16x3 paths within 1e-4 of the reference's scale (the close() rule of tests/test_gpu_conv_paths.py); gradients
and Adam as tests/test_gpu_model.py holds g15 to."""
import pytest
import torch

import sepcnn_cpu_ref as SR

pytestmark = pytest.mark.gpu

LEVELS = [(60, True), (30, True), (15, False), (16, False), (64, True)]


def close(got, ref, tol=1e-4, what=""):
    got = got.detach().cpu().double(); ref = ref.detach().cpu().double()
    err = float((got - ref).abs().max())
    bound = tol * max(1.0, float(ref.abs().max()))
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def block_inputs(F_, H, N, train, seed=0):
    gen = torch.Generator().manual_seed(1000 * F_ + 10 * H + N + seed)
    x = torch.randn(N, F_, H, H, generator=gen)
    w1 = torch.randn(F_, F_, 1, 1, generator=gen) / F_ ** 0.5
    wd = torch.randn(F_, 1, 3, 3, generator=gen) / 3.0
    w2 = torch.randn(F_, F_, 1, 1, generator=gen) / F_ ** 0.5
    sc = None
    if train:                                             # Dropout2d(0.25) scales, exact zeros included
        sc = (torch.rand(N, F_, generator=gen) >= 0.25).float() / 0.75
        sc[0, 0] = 0.0
    return x, w1, wd, w2, sc


def decided_windows(e, tol):
    """(windows whose two largest values differ by more than tol, float64 argmax in scan order)."""
    N, F_, H, W = e.shape
    ew = e.reshape(N, F_, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, F_, H // 2, W // 2, 4)
    top2 = ew.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) > tol, ew.argmax(-1)


def run_fused(x, w1, wd, w2, sc, pool, train):
    from fdet_amd import hotpath as hp, sepstack as ss
    N, F_, H, _ = x.shape
    xg = x.cuda()
    p1, p2 = hp.pointwise_pack(w1.cuda())[0], hp.pointwise_pack(w2.cuda())[0]
    out = torch.full((N, F_, H // pool, H // pool), float("nan"), device="cuda")
    a = torch.full_like(xg, float("nan")) if train else None
    b = torch.full_like(xg, float("nan")) if train else None
    route = torch.zeros(N, F_, H // 2, H // 2, dtype=torch.uint8, device="cuda") if (train and pool == 2) else None
    ss.sepblock_fwd(xg, p1, wd.cuda(), p2, sc.cuda() if sc is not None else None, out, a, b, route, pool)
    torch.cuda.synchronize()
    return out, a, b, route


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,pool", LEVELS)
@pytest.mark.parametrize("F_", [16, 64, 128])
def test_fused_block_against_float64(F_, H, pool, N, train):
    from fdet_amd import sepstack as ss
    assert ss.sepblock_plan(F_, H, H, 2 if pool else 1) is not None
    x, w1, wd, w2, sc = block_inputs(F_, H, N, train)
    a64, b64, e64, o64 = SR.block_parts(x.double(), w1.double(), wd.double(), w2.double(), None if sc is None else sc.double(), pool)
    out, a, b, route = run_fused(x, w1, wd, w2, sc, 2 if pool else 1, train)
    close(out, o64, what=f"out F{F_} H{H} N{N}")
    if train:
        close(a, a64, what="a")
        close(b, b64, what="b")
    if train and pool:
        tol = 1e-4 * max(1.0, float(e64.abs().max()))
        decided, arg = decided_windows(e64, tol)
        undecided = 1.0 - float(decided.float().mean())
        print(f"undecided windows {undecided:.4%}")
        assert undecided < 0.01
        r = route.cpu()
        assert torch.equal((r & 15)[decided], torch.full_like(r, 15)[decided])
        assert torch.equal((r >> 4)[decided].long(), arg[decided])


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("H,pool", LEVELS)
@pytest.mark.parametrize("F_", [16, 64, 128])
def test_fused_equals_composed_block(F_, H, pool, train, monkeypatch):
    """The same block through SepStack.block_forward with the switch on and off; the counters say which path ran."""
    from fdet_amd import sepstack as ss
    from fdet_amd.convstack import StackGeometry
    x, w1, wd, w2, sc = block_inputs(F_, H, 2, train, seed=7)
    outs = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("FDET_SEP", flag)
        # a one-block stack whose stem output is HxH: input 8H, stem k10 s8 p2; S = 16 sets the pooling rule H > 16
        eng = ss.SepStack(StackGeometry("separablecnn", F_, 3, 8 * H, 8 * H, 16, 1, 10, 8, 2, 1, 0, pool_mult=1, strict_grid=False))
        assert eng.lv == [(H, 2 if pool else 1)]
        P = {"residual_blocks.0.pointwise_conv1.weight": w1.cuda(), "residual_blocks.0.depthwise_conv.weight": wd.cuda(),
             "residual_blocks.0.pointwise_conv2.weight": w2.cuda()}
        eng._ensure_packed(P)
        out, sv = eng.block_forward(0, x.cuda(), P, sc.cuda() if sc is not None else None, save=train)
        torch.cuda.synchronize()
        assert eng.counters == ({"fused": 1, "composed": 0} if flag == "1" else {"fused": 0, "composed": 1})
        outs[flag] = (out, sv)
    close(outs["1"][0], outs["0"][0], what=f"fused vs composed F{F_} H{H}")
    if train:
        close(outs["1"][1][1], outs["0"][1][1], what="a")
        close(outs["1"][1][2], outs["0"][1][2], what="b")


def _golden_model(g, **kw):
    from fdet_amd.models.SeparableCNN import SeparableCNN
    model = SeparableCNN(filters=16, input_shape=(3, 480, 480), **kw)
    model.load_state_dict({k[len("param/"):]: v.clone() for k, v in g.items() if k.startswith("param/")}, strict=True)
    return model.cuda()


def _redraw(g):
    x_u8 = torch.randint(0, 256, (2, 3, 480, 480), generator=torch.Generator().manual_seed(int(g["x_seed"])), dtype=torch.uint8)
    assert int(x_u8.long().sum()) == int(g["x_sum"]) and torch.equal(x_u8[:, :, ::97, ::89], g["x_probe"])
    return x_u8


@pytest.mark.parametrize("switch,paths", [(None, {"fused": 0, "composed": 10}), ("1", {"fused": 10, "composed": 0}),
                                          ("0", {"fused": 0, "composed": 10})])
@pytest.mark.parametrize("key,kw", [("y_eval_default", {}), ("y_eval_pad3", {"output_padding": 3})])
def test_model_eval_forward_and_boxes_against_g20(golden, key, kw, switch, paths, monkeypatch):
    """Default dispatch: F=16 is not among the widths the fused kernel was measured faster at (sepstack.FUSED_MEASURED_FASTER),
    so every block takes the composed launches; FDET_SEP=1 / 0 force one path everywhere.  (The default at F=64, where the
    eight whole-map blocks do take the fused kernel, is asserted in test_batch_sizes_eval.)"""
    if switch is None:
        monkeypatch.delenv("FDET_SEP", raising=False)
    else:
        monkeypatch.setenv("FDET_SEP", switch)
    g = golden("g20_separablecnn_F16")
    model = _golden_model(g, **kw).eval()
    x = (_redraw(g).float() / 255.0).cuda()
    with torch.no_grad():
        y = model(x)
    assert tuple(y.shape) == tuple(g[key].shape)
    assert model.engine.counters == paths
    close(y, g[key], what=key)
    got = model.non_max_suppression(y)
    ref = model.non_max_suppression(g[key].cuda())
    assert len(got) == len(ref) == 2
    for a, b in zip(got, ref):
        assert a.shape == b.shape and torch.equal(a[:, 1:].cpu(), b[:, 1:].cpu())
        assert torch.allclose(a[:, 0].cpu(), b[:, 0].cpu(), atol=1e-4)


@pytest.mark.parametrize("switch", [None, "1"])
def test_model_train_step_against_g20(golden, switch, monkeypatch):
    from fdet_amd.models import ModelMeta
    if switch is None:
        monkeypatch.delenv("FDET_SEP", raising=False)
    else:
        monkeypatch.setenv("FDET_SEP", switch)
    g = golden("g20_separablecnn_F16")
    model = _golden_model(g, output_padding=3).train()
    mm = ModelMeta(model=model, lr=1e-4)
    (opt,), _ = mm.configure_optimizers()
    model.set_dropout_masks({k[len("mask/"):]: v for k, v in g.items() if k.startswith("mask/")})
    x = (_redraw(g).float() / 255.0).cuda()
    y = g["y"].cuda()
    out = mm.training_step((x, y, None), 0)
    loss = out["loss"]
    ref_loss = float(g["loss"])
    print("loss", float(loss.detach()), "ref", ref_loss)
    assert abs(float(loss) - ref_loss) <= 1e-4 * max(1.0, ref_loss)
    y_hat = mm(x)
    close(y_hat, g["y_train"], what="y_train")
    loss.backward()
    for n, p in model.named_parameters():
        got, ref = p.grad.detach().cpu().double().reshape(-1), g["grad/" + n].double().reshape(-1)
        rel_l2 = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        worst = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        print(f"grad {n}: rel L2 {rel_l2:.3e}, worst entry {worst:.3e} of scale")
        assert rel_l2 <= 2e-3, (n, rel_l2)
        assert worst <= 2e-2, (n, worst)
    opt.step()
    for n, p in model.named_parameters():
        d = (p.detach().cpu() - g["param_after/" + n]).abs()
        assert float(d.max()) <= 2.1e-4, n
        assert float((d > 1e-6).float().mean()) < 0.02, n


def _f64_model(seed=0):
    from fdet_amd.models.SeparableCNN import SeparableCNN
    torch.manual_seed(seed)
    return SeparableCNN(filters=64, input_shape=(3, 480, 480), output_padding=3).cuda()


@pytest.mark.parametrize("B", [1, 7, 64])
def test_batch_sizes_eval(B, monkeypatch):
    monkeypatch.delenv("FDET_SEP", raising=False)
    model = _f64_model().eval()
    x = torch.rand(B, 3, 480, 480, generator=torch.Generator().manual_seed(B))
    with torch.no_grad():
        y = model(x.cuda())
    # default dispatch at F=64 in eval: the eight 15x15 blocks (one tile per image) fused, the two banded levels composed
    assert model.engine.counters == {"fused": 8, "composed": 2}
    assert tuple(y.shape) == (B, 5, 16, 16) and bool(torch.isfinite(y).all())
    if B == 64:
        with torch.no_grad():
            halves = torch.cat([model(x[:32].cuda()), model(x[32:].cuda())])
        assert torch.equal(y, halves)
    P = {n: p.detach().cpu() for n, p in model.named_parameters()}
    sub = list(range(min(B, 4)))
    with torch.no_grad():
        close(y[sub], SR.forward(P, x[sub], head_pad=3), what=f"B={B} subset vs CPU")


def test_second_step_on_recycled_buffers_equals_a_fresh_engine():
    from fdet_amd.models import ModelMeta
    import oracle as O
    B = 7
    xs = [torch.rand(B, 3, 480, 480, generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2)]
    y = torch.stack([O.encode_targets(b, (480, 480), 16) for b in O.synthetic_boxes(B, 480, seed=3)]).cuda()
    masks = {f"residual_blocks.{k}": (torch.rand(B, 64, generator=torch.Generator().manual_seed(k)) >= 0.25).float() / 0.75 for k in range(10)}
    masks["head"] = (torch.rand(B, 64, generator=torch.Generator().manual_seed(99)) >= 0.5).float() / 0.5

    def steps(fresh_before_second):
        model = _f64_model(seed=5).train()
        model.set_dropout_masks(masks)
        mm = ModelMeta(model=model, lr=1e-4)
        mm.configure_optimizers()
        l1, _, _ = mm.fused_train_step(xs[0], y)
        if fresh_before_second:
            model._engine = None
        l2, _, _ = mm.fused_train_step(xs[1], y)
        return float(l1), float(l2)
    a, b = steps(False), steps(True)
    print("losses", a, b)
    assert all(map(lambda v: v == v and abs(v) != float("inf"), a + b))
    assert a == b


def test_surface_predict_graph_tiles_and_precision():
    from fdet_amd._native import FdetError
    model = _f64_model().eval()
    u8 = torch.randint(0, 256, (2, 3, 480, 480), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        det = model(u8, predict=torch.tensor(1))
        maps = model.forward_frames(u8)
        ref = model.reduce_bounding_boxes(maps[0])
        assert det.shape == ref.shape and torch.equal(det.cpu(), ref.cpu())
        maps_f = model.forward_frames(u8.float())
        assert torch.allclose(maps_f, maps, atol=1e-6)
    gp = model.graphed_predict(u8)
    eager = model.non_max_suppression(maps)
    for a, b in zip(gp(u8), eager):
        assert a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    with pytest.raises(FdetError):
        model.engine.set_precision("bf16")
    from fdet_amd.models import ModelMeta
    for export in (model.to_torchscript, ModelMeta(model=model).to_torchscript):     # the second is what trainer.fit calls
        with pytest.raises(FdetError, match="TorchScript export is not built for SeparableCNN"):
            export()


def test_tiled_detector_and_evaluator_run():
    import numpy as np
    from fdet_amd.datasets import augment as A
    from fdet_amd.datasets.synthetic import synthetic_boxes
    from fdet_amd.evaluation import DetectionEvaluator
    from fdet_amd.tiling import TiledDetector
    model = _f64_model().eval()
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((600, 700), (480, 480), (500, 900), (640, 480))]
    bank = A.DeviceImageBank.from_arrays(imgs, "cuda")
    ev = DetectionEvaluator()
    rows, counts = TiledDetector(model, reducer=ev.reducer_for(model)).detect(bank, [0, 1, 2, 3])
    assert rows.shape[0] == 4 and counts.shape == (4,)
    ev.update(rows, counts, synthetic_boxes(4, 480, seed=2))
    torch.cuda.synchronize()


@pytest.mark.parametrize("F_", [16, 64])
def test_head_k1_model_at_512_forward_and_train_step_against_cpu(F_):
    """512x512 with output_kernel_size=1: maps 64 -> 32 -> 16 and the 1x1 head (k_head_fwd<1> / k_head_bwd<1>).  Eval forward
    within 1e-4 of the CPU restatement; one training step with injected masks: output, loss and every gradient (out.weight /
    out.bias from the head's backward, all others through its dx) against the CPU autograd at the g15 bounds."""
    import oracle as O
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.SeparableCNN import SeparableCNN
    B = 2
    torch.manual_seed(11 + F_)
    model = SeparableCNN(filters=F_, input_shape=(3, 512, 512), output_kernel_size=1).cuda()
    assert tuple(model.out.weight.shape) == (5, F_, 1, 1) and model.engine.lv[:3] == [(64, 2), (32, 2), (16, 1)]
    P = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    x = torch.rand(B, 3, 512, 512, generator=torch.Generator().manual_seed(4))
    model.eval()
    with torch.no_grad():
        y_eval = model(x.cuda())
        assert tuple(y_eval.shape) == (B, 5, 16, 16)
        close(y_eval, SR.forward(P, x), what=f"eval F{F_} 512 k1")
    masks = {f"residual_blocks.{k}": (torch.rand(B, F_, generator=torch.Generator().manual_seed(k)) >= 0.25).float() / 0.75
             for k in range(10)}
    masks["head"] = (torch.rand(B, F_, generator=torch.Generator().manual_seed(77)) >= 0.5).float() / 0.5
    y = torch.stack([O.encode_targets(b, (512, 512), 16) for b in O.synthetic_boxes(B, 512, seed=6)])
    ref_y, ref_loss, ref_grads, _ = SR.train_step(P, x, y, masks)
    model.train()
    model.set_dropout_masks(masks)
    mm = ModelMeta(model=model, lr=1e-4)
    mm.configure_optimizers()
    out = mm.training_step((x.cuda(), y.cuda(), None), 0)
    loss = out["loss"]
    print("loss", float(loss.detach()), "ref", float(ref_loss))
    assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(1.0, float(ref_loss))
    close(mm(x.cuda()), ref_y, what="y_train")
    loss.backward()
    for n, p in model.named_parameters():
        got, ref = p.grad.detach().cpu().double().reshape(-1), ref_grads[n].double().reshape(-1)
        rel_l2 = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        worst = float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)
        print(f"grad {n}: rel L2 {rel_l2:.3e}, worst entry {worst:.3e} of scale")
        assert rel_l2 <= 2e-3, (n, rel_l2)
        assert worst <= 2e-2, (n, worst)


def test_reassigned_num_of_patches_decodes_the_default_10x10_grid(golden):
    """The pattern of the reference's pruner.py:32-38 on the default constructor (10x10 head, num_of_patches=16): assign
    num_of_patches and rebuild reduce_bounding_boxes; decode / NMS, predict and ModelMeta's step metrics then follow the
    10x10 grid (compared with the oracle's reducer on the same maps), and the blocks keep pooling down to 15x15."""
    import oracle as O
    from fdet_amd.datasets.utils import ReduceBoundingBoxes
    from fdet_amd.models import ModelMeta
    g = golden("g20_separablecnn_F16")
    model = _golden_model(g).eval()
    with torch.no_grad():
        model.out.bias[0] += 0.5                          # confident cells, so the decode has boxes to suppress
    model.num_of_patches = 10
    model.reduce_bounding_boxes = ReduceBoundingBoxes(0.5, 0.5, model.input_shape, model.num_of_patches)
    assert model.engine.lv == [(60, 2), (30, 2)] + [(15, 1)] * 8
    u8 = _redraw(g).cuda()
    x = u8.float() / 255.0
    with torch.no_grad():
        y_hat = model(x)
    assert tuple(y_hat.shape) == (2, 5, 10, 10)
    ref_red = O.ReduceBoundingBoxes(0.5, 0.5, (3, 480, 480), 10)
    got = model.non_max_suppression(y_hat)
    assert sum(b.shape[0] for b in got) > 0
    for n in range(2):
        ref = ref_red(y_hat[n])
        assert got[n].shape == ref.shape and torch.equal(got[n][:, 1:].cpu(), ref[:, 1:])
        assert torch.allclose(got[n][:, 0].cpu(), ref[:, 0], atol=1e-6)
    _, boxes0 = model.predict(u8)                         # rebuilds the reducer from model.num_of_patches
    assert model.reduce_bounding_boxes.num_of_patches == 10
    assert boxes0.shape == got[0].shape and torch.equal(boxes0[:, 1:].cpu(), got[0][:, 1:].cpu())
    y = torch.stack([O.encode_targets(b, (480, 480), 10) for b in O.synthetic_boxes(2, 480, seed=9)])
    mm = ModelMeta(model=model, lr=1e-4)
    with torch.no_grad():
        out = mm.validation_step((x, y.cuda(), None), 0)
    ref_m = O.step_metrics(y_hat.cpu(), y, ref_red)
    print("metrics", [float(out[k]) for k in ("total_iou", "total_recall", "total_precision")], "ref", ref_m)
    assert bool(torch.isfinite(out["loss"]))
    assert abs(float(out["total_iou"]) - ref_m[0]) <= 1e-4 * max(1.0, abs(ref_m[0]))     # the bounds of tests/test_gpu_model.py
    assert abs(float(out["total_recall"]) - ref_m[1]) <= 1e-6
    assert abs(float(out["total_precision"]) - ref_m[2]) <= 1e-6
