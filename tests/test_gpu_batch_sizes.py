"""Training and inference at small, odd, deployed and switch-crossing batch sizes.

The engines pick their kernels per batch (ConvStack.plan(N): the stem, PS block and PS chain routes; the PS weight gradient's
slab plan; the 32-bit offset limits of the C plans).  Small and odd batches are compared with the oracle; batches on the
far side of a switch are compared with their halves (which sit on the near side): forward and loss bit-exact where both run the same
kernels, else within 1e-4.  Gradients add up to 1e-4 of each tensor's scale where both sides run the same kernels.  Where
they do not (fp32-I/O vs pre-split activations, which keep 16 significant bits), the gradient is a discontinuous function
of the activations (pool routing, LeakyReLU kinks), so the two sides are compared with test_gpu_model's bounds for one step
in two arithmetics (measured on Resnet-64 640^2, B=84 vs 42: relative L2 <= 1.7e-4, entries <= 5.2e-4 of the scale; forward
3.6e-6).  tests/test_batch_plans.py checks on the CPU that every stage is accepted by its kernel at these sizes."""
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu

GiB = 1 << 30


def _need(gib):
    free, _ = torch.cuda.mem_get_info()
    if free < gib * GiB:
        pytest.skip(f"needs ~{gib} GiB of free device memory, {free / GiB:.1f} GiB free (short by {gib - free / GiB:.1f} GiB)")


def _yolo_model(kind, F_, size, S, nb, seed, prec="bf16x3"):
    import fdet_amd  # noqa: F401
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.models.Resnet import Resnet
    spec = (O.poolresnet_spec if kind == "poolresnet" else O.resnet_spec)(F_, (3, size, size), S, nb)
    P = O.init_params(spec, seed=seed)
    cls = PoolResnet if kind == "poolresnet" else Resnet
    model = cls(filters=F_, input_shape=(3, size, size), num_of_patches=S, num_of_residual_blocks=nb)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda()
    model.engine.set_precision(prec)
    return spec, P, model


def _inputs(spec, B, size, S, seed, device_x=True):
    from fdet_amd import hotpath as hp
    g = torch.Generator(device="cuda" if device_x else "cpu").manual_seed(seed)
    x = torch.rand(B, 3, size, size, generator=g, device="cuda" if device_x else "cpu")
    y = hp.encode_targets(O.synthetic_boxes(B, size, seed=seed + 1), (size, size), S)
    masks = O.make_dropout_masks(spec, B, seed=seed + 2)
    return x, y, masks


def _step(model, x, y, masks, sl=slice(None)):
    """Forward + yolo_loss + backward of the engine on x[sl] -> (y_hat, loss per image, loss sum, {name: grad})."""
    from fdet_amd import hotpath as hp
    eng = model.engine
    names, params = model.named_stack_params()
    Pd = {n: p.data for n, p in zip(names, params)}
    m_ = {k: v[sl].contiguous().cuda() for k, v in masks.items()} if masks is not None else None
    yh, saved = eng.forward(x[sl].contiguous(), Pd, m_, save=True)
    lpi, lsum, dy = hp.yolo_loss_fwd_bwd(yh, y[sl].contiguous(), want_grad=True)
    G = {n: torch.empty_like(p) for n, p in Pd.items()}
    eng.backward(saved, dy, Pd, G)
    del saved
    return yh, lpi, lsum, G


def _rel_close(a, b, tol):
    a = a.detach().cpu().double(); b = b.detach().cpu().double()
    scale = max(1e-30, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert err <= tol * max(scale, 1e-3), f"max err {err:.3e}, scale {scale:.3e}"


def _grads_across_arithmetics(G, G_ref):
    # test_gpu_model.test_fused_train_steps_vs_oracle's step-1 bounds (pool routing / LeakyReLU kinks make single gradient
    # entries jumpy between two arithmetics: L2 within 5e-3, entries within 5e-2 of the tensor's scale)
    for n, ref in G_ref.items():
        got = G[n].detach().cpu().double()
        ref = ref.double()
        rel_l2 = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        assert rel_l2 <= 5e-3, (n, rel_l2)
        _rel_close(got, ref, 5e-2)


def _halves_match(full, a, b, same_kernels):
    """A batch is the concatenation of its halves (test_gpu_fullsize.test_batch_is_concatenation_of_its_halves)."""
    y_all, lpi_all, lsum_all, G_all = full
    y_a, lpi_a, lsum_a, G_a = a
    y_b, lpi_b, lsum_b, G_b = b
    y_cat, lpi_cat = torch.cat([y_a, y_b]), torch.cat([lpi_a, lpi_b])
    if same_kernels:
        assert torch.equal(y_all, y_cat)
        assert torch.equal(lpi_all, lpi_cat)
    else:
        assert float((y_all - y_cat).abs().max()) <= 1e-4
        assert torch.allclose(lpi_all, lpi_cat, rtol=1e-4, atol=1e-4)
    ls = float(lsum_all)
    assert abs(ls - float(lsum_a) - float(lsum_b)) <= 1e-4 * max(1.0, abs(ls))
    assert abs(ls - float(lpi_all.double().sum())) <= 1e-4 * max(1.0, abs(ls))
    if not same_kernels:
        _grads_across_arithmetics(G_all, {n: G_a[n].double() + G_b[n].double() for n in G_all})
        return
    for n in G_all:
        tot = G_a[n].double() + G_b[n].double()
        scale = max(1e-6, float(tot.abs().max()))
        assert float((G_all[n].double() - tot).abs().max()) <= 1e-4 * scale, n


def _to_cpu(res):
    yh, lpi, lsum, G = res
    return yh.cpu(), lpi.cpu(), lsum.cpu(), {n: v.cpu() for n, v in G.items()}


# ---------------------------------------------------------------------------------------------- small and odd batches
ORACLE_CASES = [("poolresnet", 64, 480, 10, 10, 1), ("poolresnet", 64, 480, 10, 10, 7),
                ("resnet", 64, 320, 10, 6, 1), ("resnet", 64, 320, 10, 6, 5),
                ("poolresnet", 128, 480, 10, 10, 1), ("poolresnet", 128, 480, 10, 10, 3)]


@pytest.mark.parametrize("kind,F_,size,S,nb,B", ORACLE_CASES)
def test_small_and_odd_batches_match_the_oracle(kind, F_, size, S, nb, B):
    """Training forward, loss and parameter gradients at batches 1 and odd (one line per workgroup in the PS weight gradient's
    plan, odd band counts of the PS conv and chain kernels) against the oracle's train_step."""
    spec, P, model = _yolo_model(kind, F_, size, S, nb, seed=30 + B)
    x, y, masks = _inputs(spec, B, size, S, seed=40 + B, device_x=False)
    model.train()
    yh, lpi, lsum, G = _step(model, x.cuda(), y, masks)
    state = {"exp_avg": {k: torch.zeros_like(v) for k, v in P.items()}, "exp_avg_sq": {k: torch.zeros_like(v) for k, v in P.items()}}
    loss_ref, y_ref, G_ref = O.train_step(spec, {k: v.clone() for k, v in P.items()}, state, 1, x, y.cpu(), masks)
    assert torch.allclose(yh.cpu(), y_ref, atol=1e-4)
    assert abs(float(lsum) - float(loss_ref)) <= 1e-4 * max(1.0, float(loss_ref))
    _grads_across_arithmetics(G, G_ref)
    model.eval()
    with torch.no_grad():
        ye = model(x.cuda()).cpu()
    assert torch.allclose(ye, O.model_forward(spec, P, x, None), atol=1e-4)


@pytest.mark.parametrize("F_,B", [(64, 1), (64, 7), (128, 1), (128, 3)])
def test_small_and_odd_batches_precision16_vs_the_engines_bf16x3(F_, B):
    """precision16 at batches 1 and odd against the engine's own fp32-grade run (test_gpu_p16's bounds)."""
    res = {}
    for prec in ("bf16x3", "bf16"):
        spec, P, model = _yolo_model("poolresnet", F_, 480, 10, 10, seed=50 + B, prec=prec)
        x, y, masks = _inputs(spec, B, 480, 10, seed=60 + B)
        model.train()
        yh, _, lsum, G = _step(model, x, y, masks)
        names, _ = model.named_stack_params()
        res[prec] = (float(lsum), yh, torch.cat([G[n].flatten() for n in names]))
    (la, ya, ga), (lb, yb, gb) = res["bf16x3"], res["bf16"]
    assert abs(la - lb) <= 2e-2 * abs(la), (la, lb)
    assert float((ya - yb).abs().max()) <= 2e-2
    cos = float((ga.double() * gb.double()).sum() / (ga.double().norm() * gb.double().norm()))
    assert cos >= 0.995, cos


@pytest.mark.parametrize("B", [1, 5])
def test_ssd_small_and_odd_batches_match_the_oracle(B):
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    from fdet_amd.models.SSD import SSD
    from oracle import ssd_model_oracle as SM
    from oracle import ssd_oracle as SO
    fil, size = 16, 480
    P = SM.init_params(fil, seed=70 + B)
    model = SSD(filters=fil, input_shape=(3, size, size))
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().train()
    eng = model.engine
    names, params = model.named_stack_params()
    Pd = {n: p.data for n, p in zip(names, params)}
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(71 + B))
    boxes = O.synthetic_boxes(B, size, seed=72 + B, max_faces=5)
    tgt = torch.stack([SO.ssd_encode(b if b.numel() else torch.tensor([]), (size, size)) for b in boxes])
    masks = SM.make_dropout_masks(fil, B, seed=73 + B)
    loss_ref, y_ref, G_ref = SM.loss_and_grads(fil, P, x, tgt, masks)
    y, saved = eng.forward(x.cuda(), Pd, {k: v.cuda() for k, v in masks.items()}, save=True)
    loss, dy, _ = hp.ssd_loss_fwd_bwd(y, tgt.cuda(), 10, want_grad=True)
    G = {n: torch.empty_like(p) for n, p in Pd.items()}
    eng.backward(saved, dy, Pd, G)
    assert torch.allclose(y.cpu(), y_ref, rtol=1e-4, atol=1e-4)
    assert abs(float(loss) - float(loss_ref)) <= 1e-4 * max(1.0, abs(float(loss_ref)))
    for n in names:
        got, ref = G[n].detach().cpu().double(), G_ref[n].double()
        rel = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
        assert rel <= 5e-3, (n, rel)                    # test_gpu_ssd's bound (pool-argmax routing makes entries jumpy)


# ---------------------------------------------------------------------------------------------- config 2's literal batch
def test_config2_batch64_subset_matches_oracle_and_equals_its_halves():
    """BASELINE config 2 (PoolResnet-medium 480^2, bs=64): a 4-image subset against the oracle, and the batch against its
    halves (forward bit-exact, gradients adding up)."""
    B = 64
    spec, P, model = _yolo_model("poolresnet", 64, 480, 10, 10, seed=81)
    x, y, masks = _inputs(spec, B, 480, 10, seed=82)
    sub = [0, 13, 32, 63]
    model.train()
    full = _to_cpu(_step(model, x, y, masks))
    ms = {k: v[sub] for k, v in masks.items()}
    y_ref = O.model_forward(spec, P, x[sub].cpu(), ms)
    assert torch.allclose(full[0][sub], y_ref, atol=1e-4)
    a = _to_cpu(_step(model, x, y, masks, slice(0, B // 2)))
    b = _to_cpu(_step(model, x, y, masks, slice(B // 2, B)))
    _halves_match(full, a, b, same_kernels=True)


# ---------------------------------------------------------------------------------------------- batch-size sequences
def test_batch_size_sequence_on_one_engine_is_reproducible():
    """7 -> 1 -> 7 -> 64 -> 7 on one engine: the PS pool is cleared on every change of N and recycled buffers come back;
    each repeated batch size reproduces its first forward + backward bit for bit, and the uint8 frame path equals the fp32
    path at every N."""
    spec, P, model = _yolo_model("poolresnet", 64, 480, 10, 10, seed=91)
    first = {}
    for N in (7, 1, 7, 64, 7):
        x, y, masks = _inputs(spec, N, 480, 10, seed=92 + N)
        model.train()
        res = _to_cpu(_step(model, x, y, masks))
        if N in first:
            r0 = first[N]
            assert torch.equal(res[0], r0[0]) and torch.equal(res[1], r0[1]) and torch.equal(res[2], r0[2]), N
            for n in r0[3]:
                assert torch.equal(res[3][n], r0[3][n]), (N, n)
        else:
            first[N] = res
        model.eval()
        fr = torch.randint(0, 256, (N, 3, 480, 480), dtype=torch.uint8, generator=torch.Generator(device="cuda").manual_seed(N),
                           device="cuda")
        with torch.no_grad():
            a = model.forward_frames(fr)
            b = model._stack_forward(model._preprocess(fr))
        assert torch.equal(a, b), N


# ---------------------------------------------------------------------------------------------- across the switches
def _stem_launch_images():
    """Images per launch of the PoolResnet stem's pipelined kernels at 480^2 (32-bit offsets: 3*480*480*N < 2^29)."""
    return (2 ** 29 - 1) // (3 * 480 * 480)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_poolresnet64_batch800_stem_runs_in_chunks(prec):
    """B = 800 (halves 400): the stem's pre-split forward and its weight gradient run as more than one launch at 800 and as one
    at 400; everything else takes the same kernels, so the forward is bit-exact."""
    B = 800
    _need(60)
    spec, P, model = _yolo_model("poolresnet", 64, 480, 10, 10, seed=101, prec=prec)
    eng = model.engine
    assert B // 2 <= _stem_launch_images() < B
    for n in (B, B // 2):
        assert eng.plan(n).stem_ps and eng.plan(n).stem_wgrad == (True, prec == "bf16"), n
    x, y, masks = _inputs(spec, B, 480, 10, seed=102)
    model.train()
    full = _to_cpu(_step(model, x, y, masks))
    a = _to_cpu(_step(model, x, y, masks, slice(0, B // 2)))
    b = _to_cpu(_step(model, x, y, masks, slice(B // 2, B)))
    _halves_match(full, a, b, same_kernels=True)


@pytest.mark.timeout(1200)
def test_poolresnet64_forward_frames_batch800():
    B = 800
    _need(40)
    spec, P, model = _yolo_model("poolresnet", 64, 480, 10, 10, seed=111)
    model.eval()
    fr = torch.randint(0, 256, (B, 3, 480, 480), dtype=torch.uint8, generator=torch.Generator(device="cuda").manual_seed(112),
                       device="cuda")
    with torch.no_grad():
        a = model.forward_frames(fr)
        b = model._stack_forward(model._preprocess(fr))
        h = torch.cat([model.forward_frames(fr[: B // 2].contiguous()), model.forward_frames(fr[B // 2:].contiguous())])
    assert torch.equal(a, b)
    assert torch.equal(a, h)
    sub = [0, 399, 400, 799]
    ref = O.model_forward(spec, P, fr[sub].cpu().float() / 255.0, None)
    assert torch.allclose(a[sub].cpu(), ref, atol=1e-4)


@pytest.mark.timeout(1200)
def test_resnet64_640_batch84_level320_leaves_ps():
    """Config 3's geometry (Resnet-64 640^2, S=20), B = 84 (halves 42): level 320 runs the fp32-I/O kernels at 84 and column
    strips at 42, levels 160 and below stay on PS (mixed hand-offs in forward and backward)."""
    B = 84
    _need(40)
    spec, P, model = _yolo_model("resnet", 64, 640, 20, 10, seed=121)
    eng = model.engine
    assert [st.kind == "ps_pool" for st in eng.plan(B).stages[:2]] == [False, True]
    assert [st.kind == "ps_pool" for st in eng.plan(B // 2).stages[:2]] == [True, True]
    x, y, masks = _inputs(spec, B, 640, 20, seed=122)
    model.train()
    full = _to_cpu(_step(model, x, y, masks))
    a = _to_cpu(_step(model, x, y, masks, slice(0, B // 2)))
    b = _to_cpu(_step(model, x, y, masks, slice(B // 2, B)))
    _halves_match(full, a, b, same_kernels=False)


@pytest.mark.timeout(1800)
def test_poolresnet64_batch2400_level60_leaves_ps():
    """B = 2400 (halves 1200): level 60 and the stem leave the pre-split path at 2400 (fp32-I/O blocks, the staged fp32-output
    stem), both stay on it at 1200."""
    B = 2400
    _need(120)
    spec, P, model = _yolo_model("poolresnet", 64, 480, 10, 10, seed=131)
    eng = model.engine
    full, half = eng.plan(B), eng.plan(B // 2)
    assert full.stages[0].kind != "ps_pool" and not full.stem_ps and full.stages[1].kind == "ps_pool"
    assert half.stages[0].kind == "ps_pool" and half.stem_ps
    x, y, masks = _inputs(spec, B, 480, 10, seed=132)
    model.train()
    full = _to_cpu(_step(model, x, y, masks))
    a = _to_cpu(_step(model, x, y, masks, slice(0, B // 2)))
    b = _to_cpu(_step(model, x, y, masks, slice(B // 2, B)))
    _halves_match(full, a, b, same_kernels=False)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_poolresnet128_batch1166_staged_wgrad60(prec):
    """PoolResnet-128 480^2, B = 1166 (halves 583): the 60x60 weight gradient leaves its pipelined kernel (32-bit offsets:
    N * 128 * 60 * 60 < 2^29, fdet_wgrad3x3_x3.hip) and the stem forward its pipelined kernel; precision16 keeps its one-pass
    stem weight gradient on both sides."""
    B = 1166
    _need(120)
    spec, P, model = _yolo_model("poolresnet", 128, 480, 10, 10, seed=141, prec=prec)
    eng = model.engine
    assert (B // 2) * 128 * 60 * 60 < 2 ** 29 <= B * 128 * 60 * 60
    from fdet_amd import hotpath as hp
    for n in (B, B // 2):
        assert hp.wgrad_x3_supported(n, 128, 128, 60, 60) and eng.plan(n).stem_wgrad == (True, prec == "bf16"), n
    x, y, masks = _inputs(spec, B, 480, 10, seed=142)
    model.train()
    full = _to_cpu(_step(model, x, y, masks))
    a = _to_cpu(_step(model, x, y, masks, slice(0, B // 2)))
    b = _to_cpu(_step(model, x, y, masks, slice(B // 2, B)))
    _halves_match(full, a, b, same_kernels=False)
