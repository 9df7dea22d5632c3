"""GPU parity of the detection math (encode, loss, decode, NMS, metrics, normalise, Adam),
called through the C-ABI and checked against the oracle / golden fixtures.
Bit-exact for index/integer-valued work; fp32 loss within 1e-4 (north-star tolerance)."""
import math
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hp():
    import fdet_amd
    from fdet_amd import hotpath
    return hotpath


def test_single_hip_runtime(hp):
    from fdet_amd import _native
    _native.lib()
    assert len(_native.hip_runtimes_mapped()) == 1, _native.hip_runtimes_mapped()


def test_encode_golden_bit_exact(hp, golden):
    g = golden("g2_encode")
    for c in range(g["size"].shape[0]):
        size, S, n = int(g["size"][c]), int(g["S"][c]), int(g["n"][c])
        out = hp.encode_targets([g["boxes"][c, :n]], (size, size), S).cpu()
        assert torch.equal(out[0], g["maps"][c, :, :S, :S]), c


def test_encode_random_batch_bit_exact(hp):
    for S, size in [(10, 480), (15, 480), (20, 640)]:
        boxes = O.synthetic_boxes(64, size, seed=S, max_faces=5)
        boxes[3] = torch.zeros(0, 5)
        boxes[5] = torch.tensor([[1., 10, 10, 20, 20], [1., 12, 13, 5, 6]])       # same cell: last wins
        boxes[6] = torch.tensor([[1., float(size), float(size), 5, 5], [1., -7, 3, 5, 5]])  # clamp
        out = hp.encode_targets(boxes, (size, size), S).cpu()
        for n, b in enumerate(boxes):
            assert torch.equal(out[n], O.encode_targets(b, (size, size), S)), (S, n)


@pytest.mark.parametrize("S", [10, 15])
def test_loss_golden(hp, golden, S):
    g = golden(f"g1_loss_S{S}")
    lpi, lsum, grad = hp.yolo_loss_fwd_bwd(g["pred"].cuda(), g["gt"].cuda())
    lpi, grad = lpi.cpu(), grad.cpu()
    ref = g["loss"]
    assert torch.allclose(lpi, ref, rtol=1e-4, atol=1e-4)                 # tolerance: 1e-4 (north star)
    assert abs(float(lsum.cpu()) - float(ref.sum())) <= 1e-4 * max(1.0, float(ref.sum()))
    gr = g["grad"]
    assert torch.equal(torch.isnan(grad), torch.isnan(gr))
    assert torch.equal(torch.isinf(grad), torch.isinf(gr))
    inf = torch.isinf(gr)
    assert torch.equal(grad[inf], gr[inf])
    fin = torch.isfinite(gr)
    assert torch.allclose(grad[fin], gr[fin], rtol=1e-4, atol=1e-5)


def test_loss_vs_oracle_large_batch(hp):
    g = torch.Generator().manual_seed(0)
    B, S = 256, 10
    pred = torch.rand(B, 5, S, S, generator=g) * 0.98 + 0.01
    y = torch.stack([O.encode_targets(b, (480, 480), S) for b in O.synthetic_boxes(B, 480, seed=1)])
    lpi, lsum, grad = hp.yolo_loss_fwd_bwd(pred.cuda(), y.cuda())
    ref = torch.stack([O.yolo_loss(pred[n], y[n]) for n in range(B)])
    assert torch.allclose(lpi.cpu(), ref, rtol=1e-4, atol=1e-4)
    assert abs(float(lsum) - float(ref.sum())) <= 1e-4 * float(ref.sum())
    _, gr = O.yolo_loss_and_grad(pred[7], y[7])
    assert torch.allclose(grad[7].cpu(), gr, rtol=1e-4, atol=1e-6)


def test_decode_and_reduce_golden_bit_exact(hp, golden):
    g = golden("g3_decode")
    for c in range(g["size"].shape[0]):
        size, S = int(g["size"][c]), int(g["S"][c])
        pt, iou = float(g["pt"][c]), float(g["iou"][c])
        x = g["x"][c, :, :S, :S].contiguous()
        xb = torch.stack([x, x]).cuda()
        scores, boxes, counts = hp.decode(xb, pt, size, size)
        K = int(g["K"][c])
        assert counts.cpu().tolist() == [K, K]
        assert torch.equal(scores[1, :K].cpu(), g["pre"][c, :K, 0])
        assert torch.equal(boxes[1, :K].cpu(), g["pre"][c, :K, 1:])
        out, oc = hp.reduce_bounding_boxes(xb, pt, iou, size, size)
        Ko = int(g["Kout"][c])
        assert oc.cpu().tolist() == [Ko, Ko]
        assert torch.equal(out[0, :Ko].cpu(), g["out"][c, :Ko]), c


def _multi_chunk_maps(S):
    """(3,5,S,S) maps for the 256-wide compaction chunks of decode: scores from a set of 20 values (k/20, so equal scores
    are frequent and 10/20 sits exactly on the threshold 0.5).  Map 0 mixes hits and misses, map 1 has every cell above
    the threshold, map 2 none (its largest score equals the threshold: the comparison is strict)."""
    g = torch.Generator().manual_seed(100 + S)
    x = torch.rand(3, 5, S, S, generator=g)
    x[:, 3:] = x[:, 3:] * 0.28 + 0.02                      # boxes of 2..30 % of the image: plenty of overlap
    x[0, 0] = torch.randint(0, 20, (S, S), generator=g).float() / 20
    x[1, 0] = torch.randint(11, 20, (S, S), generator=g).float() / 20
    x[2, 0] = torch.randint(0, 11, (S, S), generator=g).float() / 20
    return x


@pytest.mark.parametrize("S", [16, 17, 23])
def test_decode_and_reduce_multi_chunk_bit_exact(hp, S):
    """decode and reduce_bounding_boxes past one 256-cell compaction chunk: 256 cells (exactly one full chunk), 289 (a
    second chunk that ends inside a wave) and 529 (three chunks), bit for bit against the oracle's decode_pre_nms
    followed by its nms."""
    from oracle import yolo_oracle as Y
    size, pt, iou, C = 480, 0.5, 0.3, S * S
    x = _multi_chunk_maps(S)
    ref = [Y.decode_pre_nms(x[n], pt, (3, size, size), S)[:2] for n in range(3)]
    # the oracle alone, before anything is compared with it: the counts these inputs were built for
    hit = (x[0, 0] > pt).flatten()
    assert [r[0].numel() for r in ref] == [int(hit.sum()), C, 0] and 0 < int(hit.sum()) < C
    for w0 in range(0, C, 64):                              # hits and misses in every wave of every chunk
        assert 0 < int(hit[w0:w0 + 64].sum()) < hit[w0:w0 + 64].numel(), w0
    assert ref[0][0].unique().numel() < ref[0][0].numel() and float(x[2, 0].max()) == pt
    keeps = [Y.nms(rb, rs, iou) for rs, rb in ref]
    assert all(0 < keeps[n].numel() < ref[n][0].numel() for n in (0, 1)) and keeps[2].numel() == 0   # the NMS has work

    xb = x.cuda()
    scores, boxes, counts = hp.decode(xb, pt, size, size)
    out, oc = hp.reduce_bounding_boxes(xb, pt, iou, size, size)
    assert counts.cpu().tolist() == [r[0].numel() for r in ref]
    assert oc.cpu().tolist() == [k.numel() for k in keeps]
    for n, ((rs, rb), keep) in enumerate(zip(ref, keeps)):
        K = rs.numel()
        assert torch.equal(scores[n, :K].cpu(), rs) and torch.equal(boxes[n, :K].cpu(), rb), (S, n)
        want = torch.cat([rs.view(-1, 1), rb.view(-1, 4)], 1)[keep]
        want[:, 3] -= want[:, 1]                            # utils.py:148-149
        want[:, 4] -= want[:, 2]
        assert torch.equal(out[n, :keep.numel()].cpu(), want), (S, n)


@pytest.mark.parametrize("thr", [0.01, 0.3, 0.5])
def test_nms_keep_sets_bit_exact(hp, thr):
    """torchvision.ops.nms semantics are restated (PARITY UNPINNED by the reference); the HIP
    kernel must return exactly the oracle's keep list, ties and zero-area boxes included."""
    g = torch.Generator().manual_seed(17)
    for K in (1, 2, 63, 64, 65, 100, 400, 1024, 3000):
        xy = torch.randint(0, 400, (K, 2), generator=g).float()
        wh = torch.randint(0, 90, (K, 2), generator=g).float()
        boxes = torch.cat([xy, xy + wh], 1)
        scores = torch.randint(0, 50, (K,), generator=g).float() / 50
        keep = hp.nms(boxes=boxes.cuda(), scores=scores.cuda(), iou_threshold=thr).cpu()
        assert keep.tolist() == O.nms(boxes, scores, thr).tolist(), K
    assert hp.nms(torch.zeros(0, 4).cuda(), torch.zeros(0).cuda(), thr).numel() == 0


def _config5_candidates(B, K, seed=2, size=480):
    """K candidates per image, scores U(0,1), centres uniform, sizes log-uniform 8..128 px."""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(B, K, 2, generator=g) * size
    wh = torch.exp(torch.rand(B, K, 2, generator=g) * (math.log(128.0) - math.log(8.0)) + math.log(8.0))
    boxes = torch.cat([c - wh / 2, c + wh / 2], 2).round()
    scores = torch.rand(B, K, generator=g)
    return boxes, scores


@pytest.mark.parametrize("K", [1024, 4096])
def test_batched_nms_config5(hp, K):
    """Batched greedy NMS at K >= 1000 candidates per image (config 5's synthetic distribution), ragged counts:
    every image's keep list equals the oracle's (restated torchvision semantics, PARITY UNPINNED by the reference)."""
    B = 6
    boxes, scores = _config5_candidates(B, K)
    counts = torch.tensor([K, K - 1, K // 2, 1, 0, K], dtype=torch.int32)
    keep, kc = hp.nms_batched(boxes.cuda(), scores.cuda(), counts.cuda(), 0.5)
    keep, kc = keep.cpu(), kc.cpu()
    for b in range(B):
        n = int(counts[b])
        ref = O.nms(boxes[b, :n], scores[b, :n], 0.5).tolist() if n else []
        assert keep[b, : int(kc[b])].tolist() == ref, (K, b)


def test_reduce_roundtrip_full_batch(hp):
    """size-independent property at the bench batch size: decode(encode(b)) == b for integer
    boxes in distinct cells (reference's own commented-out check, dataset.py:125-139)."""
    B, S, size = 256, 10, 480
    ps = size // S
    g = torch.Generator().manual_seed(2)
    boxes = []
    for n in range(B):
        cells = torch.randperm(S * S, generator=g)[: n % 5]
        rows = [[1.0, (int(c) // S) * ps + int(torch.randint(0, ps, (1,), generator=g)),
                 (int(c) % S) * ps + int(torch.randint(0, ps, (1,), generator=g)),
                 int(torch.randint(1, 150, (1,), generator=g)), int(torch.randint(1, 150, (1,), generator=g))]
                for c in cells]
        boxes.append(torch.tensor(rows, dtype=torch.float32).reshape(-1, 5))
    y = hp.encode_targets(boxes, (size, size), S)
    out, cnt = hp.reduce_bounding_boxes(y, 0.5, 1.1, size, size)
    out, cnt = out.cpu(), cnt.cpu()
    for n in range(B):
        k = int(cnt[n])
        assert k == boxes[n].shape[0]
        if k:
            a = boxes[n][torch.argsort(boxes[n][:, 1] * 10000 + boxes[n][:, 2])]
            d = out[n, :k][torch.argsort(out[n, :k, 1] * 10000 + out[n, :k, 2])]
            assert torch.equal(a, d)


def test_step_metrics_vs_oracle(hp):
    B, S, size = 32, 10, 480
    g = torch.Generator().manual_seed(4)
    y = torch.stack([O.encode_targets(b, (size, size), S) for b in O.synthetic_boxes(B, size, seed=3)])
    y_hat = (y + 0.08 * torch.rand(B, 5, S, S, generator=g)).clamp(0, 1)
    y_hat[:, 0] = torch.where(torch.rand(B, S, S, generator=g) > 0.97, torch.ones(()), y_hat[:, 0])
    red = O.ReduceBoundingBoxes(0.5, 0.5, (3, size, size), S)
    ref = O.step_metrics(y_hat, y, red)
    gt, gc = hp.reduce_bounding_boxes(y.cuda(), 0.5, 0.5, size, size)
    pr, pc = hp.reduce_bounding_boxes(y_hat.cuda(), 0.5, 0.5, size, size)
    per, tot = hp.step_metrics(gt, gc, pr, pc)
    tot = tot.cpu()
    assert abs(float(tot[0]) - ref[0]) <= 1e-4 * max(1.0, abs(ref[0]))
    assert abs(float(tot[1]) - ref[1]) <= 1e-6
    assert abs(float(tot[2]) - ref[2]) <= 1e-6


def test_u8_norm_bit_exact(hp):
    g = torch.Generator().manual_seed(0)
    for n in (16 * 7, 3 * 480 * 480 * 2, 1000003):
        x = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
        assert torch.equal(hp.u8_to_f32_norm(x.cuda()).cpu(), x / 255.0)
    every = torch.arange(256, dtype=torch.uint8).repeat(3)       # every value (the kernel multiplies by 1/255 and corrects)
    assert torch.equal(hp.u8_to_f32_norm(every.cuda()).cpu(), every / 255.0)


def test_adam_vs_oracle(hp):
    g = torch.Generator().manual_seed(0)
    n = 769349
    p = torch.randn(n, generator=g) * 0.05
    m = torch.zeros(n); v = torch.zeros(n)
    pd, md, vd = p.cuda(), m.cuda(), v.cuda()
    for step in range(1, 4):
        gr = torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-6, 2, (1,), generator=g)))
        O.adam_step([p], [gr], [m], [v], step)
        hp.adam_step(pd, gr.cuda(), md, vd, step)
        # fp32 elementwise update; ATen fuses some of these mul-adds, so allow a few ulp of the
        # tensor's scale (tolerance 1e-6 relative to max|.|)
        assert torch.allclose(pd.cpu(), p, rtol=1e-6, atol=1e-7)
        assert torch.allclose(md.cpu(), m, rtol=1e-5, atol=1e-6 * float(m.abs().max()))
        assert torch.allclose(vd.cpu(), v, rtol=1e-5, atol=1e-6 * float(v.abs().max()))


def test_cpu_tensor_is_refused(hp):
    from fdet_amd import FdetError
    with pytest.raises(FdetError):
        hp.yolo_loss_fwd_bwd(torch.rand(1, 5, 10, 10), torch.rand(1, 5, 10, 10))


@pytest.mark.parametrize("shape", [(2, 3, 640, 640), (1, 3, 333, 500), (2, 3, 100, 160), (1, 3, 1080, 1920), (1, 3, 480, 640)])
def test_resize_bilinear_u8_norm(hp, shape):
    """`resize(x) / 255.0` of models/PoolResnet.py:95 for frames that are not at the model resolution.
    Oracle: oracle.preprocess_u8 = torch CPU F.interpolate(bilinear, align_corners=False) + round + /255
    (torchvision 0.11.2's tensor Resize; torchvision itself is absent -> parity unpinned at that boundary).
    The interpolated value is fp32 with an ulp-level dependence on FMA contraction in the CPU build, so a
    pixel that lands within an ulp of .5 may round the other way: at most 0.05 % of the pixels may differ,
    and then by exactly one uint8 level."""
    import oracle as O
    g = torch.Generator().manual_seed(shape[2])
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    ref = O.preprocess_u8(x, (480, 480))
    got = hp.resize_bilinear_norm(x.cuda(), (480, 480)).cpu()
    assert got.shape == ref.shape
    lv = torch.round((got - ref) * 255.0).abs()
    assert float(lv.max()) <= 1.0
    assert float((lv > 0).float().mean()) <= 5e-4
    same = lv == 0
    assert torch.equal(got[same], ref[same])


def test_resize_bilinear_f32_and_identity(hp):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 200, 300, generator=g) * 255.0
    ref = F.interpolate(x, size=(480, 480), mode="bilinear", align_corners=False) / 255.0
    got = hp.resize_bilinear_norm(x.cuda(), (480, 480)).cpu()
    assert torch.allclose(got, ref, atol=1e-6, rtol=1e-6)
    u8 = torch.randint(0, 256, (1, 3, 480, 480), dtype=torch.uint8, generator=g)
    assert torch.equal(hp.resize_bilinear_norm(u8.cuda(), (480, 480)).cpu(), u8 / 255.0)   # Q17: identity round trip
