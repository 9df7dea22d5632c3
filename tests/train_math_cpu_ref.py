"""CPU references and input builders for the kernels that close a training step around the conv stack: the dropout
generator, Adam, the residual-block tail, the SSD head pack, the SSD loss with hard-negative mining and the step metrics.
TEST INFRASTRUCTURE ONLY.

Every reference is written from the contract in include/fdet.h and the reference lines the kernels cite, in float64 (or
in exact integer arithmetic for the generator), with torch autograd for the gradients.  Index-like decisions (the mining
mask, the max-pool routing) are taken on the float32 values the kernels see, by the float32 oracle or ATen.
tests/test_train_math_host.py proves the references and the inputs fair on the CPU; tests/test_gpu_train_math.py holds
the kernels to them."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O
from oracle import ssd_oracle as S

M64 = (1 << 64) - 1
SIZE = 480
SSD_P = sum(ps * ps for ps in S.PATCH_SIZES)                       # 4774
SSD_START = {60: 0, 30: 3600, 15: 4500, 7: 4725}                   # first prior of each scale, (scale, i, j) order
LO32 = float(np.float32(1e-7))                                     # the clamp of CustomBCELoss as fp32 numbers
HI32 = float(np.float32(1) - np.float32(1e-7))


# ------------------------------------------------------------------------------------------
# the float64 rule
# ------------------------------------------------------------------------------------------
def dist(a: torch.Tensor, ref64: torch.Tensor) -> float:
    """max |a - ref| over the positions where the reference is finite."""
    fin = torch.isfinite(ref64)
    if not bool(fin.any()):
        return 0.0
    return float((a.double()[fin] - ref64[fin]).abs().max())


def rule_tol(fp32_eval: torch.Tensor, ref64: torch.Tensor) -> float:
    """Bound for a kernel the project has no bound for: 4 x the distance of a plain fp32 torch evaluation from the float64
    reference on the same inputs, with a floor of 1e-6 of the tensor's scale.  Never looks at the kernel's output."""
    fin = torch.isfinite(ref64)
    scale = float(ref64[fin].abs().max()) if bool(fin.any()) else 0.0
    return max(4.0 * dist(fp32_eval, ref64), 1e-6 * scale)


# ------------------------------------------------------------------------------------------
# dropout generator (include/fdet.h: fdet_dropout_scales, fdet_dropout_scales_layers)
# ------------------------------------------------------------------------------------------
def _u64(v) -> np.ndarray:
    return np.array([int(v) & M64], dtype=np.uint64)


def u01(seed: int, ctr) -> np.ndarray:
    """splitmix64 finaliser of counter `ctr` (uint64 array) under `seed`: the top 24 bits times 2^-24, float32 in [0, 1).
    All arithmetic wraps mod 2^64 (numpy uint64 arrays)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    z = _u64(seed) + _u64(0x9E3779B97F4A7C15) * (ctr + _u64(1))
    z = (z ^ (z >> np.uint64(30))) * _u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * _u64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_scale(p: float) -> np.float32:
    return np.float32(1) / (np.float32(1) - np.float32(p))


def dropout_scales(n: int, p: float, seed: int, offset: int) -> np.ndarray:
    """(n,) float32: value i is 0 when u01(seed, offset + i) < p, else 1 / (1 - p); compared and scaled in float32."""
    u = u01(seed, _u64(offset) + np.arange(n, dtype=np.uint64))
    return np.where(u >= np.float32(p), keep_scale(p), np.float32(0)).astype(np.float32)


def dropout_layers(n: int, channels, p, seed: int, base: int, first_image: int):
    """One (n, C_k) float32 array per layer.  counter(image g, layer k, channel c) = base + g * LS + pre_k + c with
    LS = sum C_k, pre_k = sum_{j<k} C_j and g = first_image + i.  The kernel's buffer is these arrays, each dense,
    concatenated: layer k starts at float offset n * pre_k."""
    ls = int(sum(channels))
    out, pre = [], 0
    for C, pk in zip(channels, p):
        img = (_u64(first_image) + np.arange(n, dtype=np.uint64)) * _u64(ls)
        ctr = _u64(base) + img[:, None] + _u64(pre) + np.arange(C, dtype=np.uint64)[None, :]
        u = u01(seed, ctr)
        out.append(np.where(u >= np.float32(pk), keep_scale(pk), np.float32(0)).astype(np.float32))
        pre += int(C)
    return out


# ------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------
def adam64(p, g, m, v, step, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """oracle.adam_step on doubles, the gradient multiplied by grad_scale first.  Returns new (p, m, v); inputs untouched."""
    p, m, v = p.double().clone(), m.double().clone(), v.double().clone()
    O.adam_step([p], [g.double() * grad_scale], [m], [v], step, lr=lr, beta1=b1, beta2=b2, eps=eps)
    return p, m, v


def adam32(p, g, m, v, step, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, grad_scale=1.0):
    """The fp32 oracle on the same inputs (grad_scale is a power of two in every case, so g * grad_scale is exact)."""
    p, m, v = p.clone(), m.clone(), v.clone()
    O.adam_step([p], [g * grad_scale], [m], [v], step, lr=lr, beta1=b1, beta2=b2, eps=eps)
    return p, m, v


ADAM_LENGTHS = (1, 3, 4, 5, 1023, 1024, 1027, 2097152, 2097157)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_GRAD_SCALES = (1.0, 0.5, 0.125)


def adam_combos(n: int):
    """(index, step, grad_scale) of the combinations run at length n: all twelve for the short buffers, every fifth for
    the two that reach the grid-stride loop.  The seed of a combination's inputs is 100 * index + n % 97."""
    combos = [(s, q) for s in ADAM_STEPS for q in ADAM_GRAD_SCALES]
    return [(ci, s, q) for ci, (s, q) in enumerate(combos) if n <= 4096 or ci % 5 == 0]


def adam_case(n: int, seed: int):
    """Non-zero starting state: p ~ 0.05 N(0,1); m ~ 0.01 N(0,1); v uniform in [0, 1e-2] with exact zeros; two gradients
    (for `step` and `step + 1`) of magnitude 10^k, k in [-6, 1] as test_adam_vs_oracle draws them.  Every seventh entry
    (3, 10, ...) has g == m == v == 0 in both gradients."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.05
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-2
    v[torch.rand(n, generator=gen) < 0.1] = 0.0
    ks = [int(torch.randint(-6, 2, (1,), generator=gen)) for _ in range(2)]
    gs = [torch.randn(n, generator=gen) * (10.0 ** k) for k in ks]
    dead = torch.arange(n) % 7 == 3
    m[dead] = 0.0
    v[dead] = 0.0
    for g in gs:
        g[dead] = 0.0
    return p, m, v, gs, dead


# ------------------------------------------------------------------------------------------
# residual-block tail
# ------------------------------------------------------------------------------------------
def tail_eval(c, x, scale, pool, slope, dout, dtype):
    """out = maxpool_pool(c * scale + x) (floor), dz2 = d/dz2 and de = d/de of <out, dout> where c = leaky_relu(z2, slope).
    dout None: forward only."""
    c, x = c.to(dtype), x.to(dtype)
    sc = 1.0 if scale is None else scale.to(dtype)[:, :, None, None]
    e = c * sc + x
    out = F.max_pool2d(e, 2) if pool == 2 else e
    if dout is None:
        return out, None, None
    z2 = (c.clone() if slope == 1.0 else torch.where(c > 0, c, c / slope)).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    c2 = z2 if slope == 1.0 else F.leaky_relu(z2, slope)
    # route the gradient through the windows of the forward's own e: the max is taken on c, not on lrelu(c / slope)
    e2 = (c2 - c2.detach() + c) * sc + xr
    r2 = F.max_pool2d(e2, 2) if pool == 2 else e2
    gz, gx = torch.autograd.grad(r2, [z2, xr], dout.to(dtype))
    return out, gz, gx


def tail64(c, x, scale, pool, slope, dout):
    return tail_eval(c, x, scale, pool, slope, dout, torch.float64)


def tail_case(shape, seed, scale_kind="drop"):
    """c, x ~ N(0,1); scale: 'drop' = Dropout2d planes of p = 0.25 with channel (0, 1) dropped and (0, 0) kept,
    'none' = no scale."""
    gen = torch.Generator().manual_seed(seed)
    N, C, H, W = shape
    c = torch.randn(N, C, H, W, generator=gen)
    x = torch.randn(N, C, H, W, generator=gen)
    scale = None
    if scale_kind == "drop":
        scale = (torch.rand(N, C, generator=gen) > 0.25).float() / 0.75
        scale[0, 0] = 1 / 0.75
        if C > 1:
            scale[0, 1] = 0.0
    return c, x, scale, gen


# ------------------------------------------------------------------------------------------
# SSD head pack
# ------------------------------------------------------------------------------------------
def head_pack_eval(z, ps, prior_start, P, dy, dtype):
    """y (N,P,5): rows prior_start + i*ps + j = (sigmoid(z0), z1/ps + i/ps, z2/ps + j/ps, z3, z4), NaN elsewhere;
    dz (N,CP,ps,ps) = autograd of <y, dy> (zeros in channels 5..CP-1), None without dy."""
    zr = z.to(dtype).clone().requires_grad_(True)
    N = z.shape[0]
    i = torch.arange(ps, dtype=dtype).view(1, ps, 1)
    j = torch.arange(ps, dtype=dtype).view(1, 1, ps)
    rows = torch.stack([torch.sigmoid(zr[:, 0]), zr[:, 1] / ps + i / ps, zr[:, 2] / ps + j / ps, zr[:, 3], zr[:, 4]], -1)
    rows = rows.reshape(N, ps * ps, 5)
    y = torch.full((N, P, 5), math.nan, dtype=dtype)
    y[:, prior_start:prior_start + ps * ps] = rows.detach()
    dz = None
    if dy is not None:
        (dz,) = torch.autograd.grad(rows, zr, dy[:, prior_start:prior_start + ps * ps].to(dtype))
    return y, dz


def head_pack64(z, ps, prior_start, P, dy=None):
    return head_pack_eval(z, ps, prior_start, P, dy, torch.float64)


def head_pack_case(N, CP, ps, seed):
    """z ~ N(0,1) with z0 of the first cells set to +100, -100 (fp32 sigmoid saturates to exactly 1 and 0) and 0."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(N, CP, ps, ps, generator=gen)
    z[0, 0, 0, 0], z[0, 0, 0, 1], z[0, 0, 0, 2] = 100.0, -100.0, 0.0
    z[-1, 0, -1, -1], z[-1, 0, -1, -2] = -100.0, 100.0
    dy = torch.randn(N, SSD_P, 5, generator=gen)
    return z, dy


# ------------------------------------------------------------------------------------------
# SSD loss with hard-negative mining
# ------------------------------------------------------------------------------------------
def ssd_mask32(pred, target, ratio):
    """The mining mask of the fp32 oracle: ties are decided on the fp32 losses the kernel sees."""
    return S.hard_negative_mining(-torch.log(pred[:, :, 0].float()), target[:, :, 0].float(), ratio)


def ssd_loss64(pred, target, ratio):
    """losses/SSDLoss.py:56-86 in float64 given the fp32 oracle's mask.  Returns a dict: mask (B,P) bool, bce, sl1, npos,
    loss (float64 scalars) and grad (B,P,5) float64 = d loss / d pred."""
    mask = ssd_mask32(pred, target, ratio)
    labels = target[:, :, 0].double()
    conf = pred[:, :, 0].double().clone().requires_grad_(True)
    loc = pred[:, :, 1:].double().clone().requires_grad_(True)
    c = conf[mask].clamp(LO32, HI32)
    lm = torch.round(labels[mask])
    bce = torch.sum(-1 * (lm * torch.log(c) + (1 - lm) * torch.log(1 - c)))
    pos = labels > 0
    pl = loc[pos, :].reshape(-1, 4)
    gl = target[:, :, 1:].double()[pos, :].reshape(-1, 4)
    sl1 = F.smooth_l1_loss(pl, gl, reduction="sum")
    npos = int(pos.sum())
    loss = (sl1 + bce) / npos if npos else (sl1 + bce) / torch.zeros((), dtype=torch.float64)
    gc, gl_ = torch.autograd.grad(loss, [conf, loc], allow_unused=True)
    gc = torch.zeros_like(conf) if gc is None else gc
    gl_ = torch.zeros_like(loc) if gl_ is None else gl_
    return {"mask": mask, "bce": bce.detach(), "sl1": sl1.detach(), "npos": npos, "loss": loss.detach(),
            "grad": torch.cat([gc.unsqueeze(-1), gl_], -1)}


def mining_stats(pred, target, ratio):
    """What the fp32 oracle alone says about a batch, per image: npos, P_neg, kk = min(npos*ratio, P_neg), the number of
    selected / unselected negatives whose loss equals the smallest selected loss, whether the unselected ones all lie
    behind the selected ones, and how many 256-prior sweeps the selected ties come from."""
    mask = ssd_mask32(pred, target, ratio)
    loss = -torch.log(pred[:, :, 0].float())
    out = []
    for n in range(pred.shape[0]):
        pos = target[n, :, 0] > 0
        neg = ~pos
        npos, pneg = int(pos.sum()), int(neg.sum())
        sel = mask[n] & neg
        st = {"npos": npos, "P_neg": pneg, "kk": min(npos * ratio, pneg), "selected": int(sel.sum()),
              "tie_sel": 0, "tie_unsel": 0, "ordered": True, "tie_sweeps": 0}
        if 0 < st["kk"] < pneg:
            thr = loss[n][sel].min()
            at = neg & (loss[n] == thr)
            ts, tu = torch.nonzero(at & sel).flatten(), torch.nonzero(at & ~sel).flatten()
            st["tie_sel"], st["tie_unsel"] = ts.numel(), tu.numel()
            st["ordered"] = bool(tu.numel() == 0 or int(ts.max()) < int(tu.min()))
            st["tie_sweeps"] = int((ts // 256).unique().numel())
        out.append(st)
    return out


SSD_TIE_SEED = 5


def ssd_tie_boxes():
    """synthetic_boxes(4, 480, seed, max_faces=6) with the boxes of image 2 taken away: one image has no positive."""
    boxes = O.synthetic_boxes(4, SIZE, seed=SSD_TIE_SEED, max_faces=6)
    boxes[2] = torch.zeros(0, 5)
    return boxes


def ssd_tie_case():
    """B = 4, P = 4774: confidences on the 63 levels k/64, so dozens of negatives share the threshold loss; locations
    uniform in (0, 1); targets are the reference's multi-scale encode of ssd_tie_boxes()."""
    gen = torch.Generator().manual_seed(SSD_TIE_SEED)
    boxes = ssd_tie_boxes()
    target = torch.stack([S.ssd_encode(b if b.numel() else torch.tensor([]), (SIZE, SIZE)) for b in boxes])
    pred = torch.rand(4, SSD_P, 5, generator=gen) * 0.98 + 0.01
    pred[:, :, 0] = torch.randint(1, 64, (4, SSD_P), generator=gen).float() / 64
    return pred, target


SSD_SMALL_P = (1, 63, 255, 256, 257, 300)


def ssd_small_case(P: int):
    """B = 3, ratio 3, hand-made targets (label 0.94 at a few priors): npos * 3 below, at (or, where P is no multiple of 4,
    just above) and far above P_neg in images 0, 1, 2.  P = 1: a positive image and two negative-only ones."""
    gen = torch.Generator().manual_seed(1000 + P)
    pred = torch.rand(3, P, 5, generator=gen) * 0.98 + 0.01
    pred[:, :, 0] = torch.randint(1, 64, (3, P), generator=gen).float() / 64
    target = torch.zeros(3, P, 5)
    counts = (1, 0, 0) if P == 1 else (max(1, P // 16), (P + 3) // 4, (P + 1) // 2)
    for n, k in enumerate(counts):
        idx = torch.randperm(P, generator=gen)[:k]
        target[n, idx, 0] = 0.94
        target[n, idx, 1:] = torch.rand(k, 4, generator=gen)
    return pred, target


def ssd_saturated_case():
    """B = 3, P = 300, ratio 10.  Image 0: 10 positives (kk = 100 < 290); image 1: 2 positives and exactly 20 negatives of
    confidence 0 (loss +inf: the 20 that must be mined); image 2: 40 positives (kk = 400 > 260: every negative kept, the
    saturated ones included).  Negatives at 0, 1, the two clamp bounds, their neighbours outside the clamp and 1e-8;
    positives at 0 and 1."""
    gen = torch.Generator().manual_seed(77)
    P = 300
    pred = torch.rand(3, P, 5, generator=gen) * 0.98 + 0.01
    pred[:, :, 0] = torch.randint(1, 64, (3, P), generator=gen).float() / 64
    target = torch.zeros(3, P, 5)
    lo, hi = np.float32(1e-7), np.float32(1) - np.float32(1e-7)
    special = [0.0, 1.0, float(lo), float(hi), float(np.nextafter(lo, np.float32(0))), float(np.nextafter(hi, np.float32(1))), 1e-8]
    for n, k in enumerate((10, 2, 40)):
        perm = torch.randperm(P, generator=gen)
        pos, neg = perm[:k], perm[k:]
        target[n, pos, 0] = 0.94
        target[n, pos, 1:] = torch.rand(k, 4, generator=gen)
        pred[n, pos[0], 0], pred[n, pos[1], 0] = 0.0, 1.0
        if n == 1:
            pred[n, neg[:20], 0] = 0.0
            pred[n, neg[20:26], 0] = torch.tensor(special[1:], dtype=torch.float32)
        else:
            pred[n, neg[:7], 0] = torch.tensor(special, dtype=torch.float32)
            pred[n, neg[7:14], 0] = torch.tensor(special, dtype=torch.float32)
    return pred, target


SL1_D = (0.0, 1.0, -1.0, float(np.nextafter(np.float32(1), np.float32(0))), -float(np.nextafter(np.float32(1), np.float32(0))),
         1.5, -1.5, 0.25)


def ssd_label_case():
    """B = 2, P = 300, ratio 3: positives with labels 0.3 and 0.5 (positive for mining, 0 for the BCE: rint, half to even)
    and 0.94; their location targets are 0 and the predictions the differences SL1_D, |d| = 1 exactly included."""
    gen = torch.Generator().manual_seed(78)
    P = 300
    pred = torch.rand(2, P, 5, generator=gen) * 0.98 + 0.01
    pred[:, :, 0] = torch.randint(1, 64, (2, P), generator=gen).float() / 64
    target = torch.zeros(2, P, 5)
    d = torch.tensor(SL1_D, dtype=torch.float32)
    for n in range(2):
        idx = torch.randperm(P, generator=gen)[:12]
        target[n, idx, 0] = torch.tensor([0.3, 0.5, 0.94] * 4)
        for r, i in enumerate(idx.tolist()):
            pred[n, i, 1:] = d[(torch.arange(4) + 2 * r + n) % len(SL1_D)]
    return pred, target


def ssd_all_negative_case():
    gen = torch.Generator().manual_seed(79)
    pred = torch.rand(2, 300, 5, generator=gen) * 0.98 + 0.01
    return pred, torch.zeros(2, 300, 5)


# ------------------------------------------------------------------------------------------
# yolo loss
# ------------------------------------------------------------------------------------------
def yolo_case(B: int, S_: int, seed: int):
    """pred uniform in (0.01, 0.99); gt = the reference's encode of synthetic boxes (at least one box in image 0)."""
    gen = torch.Generator().manual_seed(seed)
    boxes = O.synthetic_boxes(B, SIZE, seed=seed, max_faces=3)
    boxes[0] = torch.tensor([[1.0, 100.0, 200.0, 50.0, 80.0]])
    gt = torch.stack([O.encode_targets(b, (SIZE, SIZE), S_) for b in boxes])
    pred = torch.rand(B, 5, S_, S_, generator=gen) * 0.98 + 0.01
    return pred, gt


def yolo64(pred, gt):
    """oracle.yolo_loss per image on doubles: (loss_per_image (B,), grad (B,5,S,S)) in float64."""
    losses, grads = [], []
    for n in range(pred.shape[0]):
        l, g = O.yolo_loss_and_grad(pred[n].double(), gt[n].double())
        losses.append(l)
        grads.append(g)
    return torch.stack(losses), torch.stack(grads)


def yolo_nan_case():
    """S = 8.  Image 0: zeros with +0.25, -0.25 and one NaN in the confidence plane: nansum == 0, no nan_to_num, the loss is
    NaN.  Image 1: the same NaN in an otherwise ordinary map: nan -> 0.1 and a finite loss."""
    pred, gt = yolo_case(2, 8, 41)
    pred[0] = 0.0
    pred[0, 0, 0, 0], pred[0, 0, 0, 1], pred[0, 0, 3, 5] = 0.25, -0.25, math.nan
    pred[1, 0, 3, 5] = math.nan
    return pred, gt


def yolo_zero_wh_case():
    """S = 8: predicted w exactly 0 under the object cell of image 0 (gradient -inf), predicted h exactly 0 under an empty
    cell (0 * inf = NaN), and both 0 where the target's w is 0 too."""
    pred, gt = yolo_case(2, 8, 42)
    i, j = [int(t[0]) for t in torch.where(gt[0, 0] > 0)]
    pred[0, 3, i, j] = 0.0
    ei, ej = [int(t[0]) for t in torch.where(gt[0, 0] == 0)]
    pred[0, 4, ei, ej] = 0.0
    pred[1, 3, ei, ej] = 0.0
    pred[1, 4, ei, ej] = 0.0
    return pred, gt


# ------------------------------------------------------------------------------------------
# step metrics
# ------------------------------------------------------------------------------------------
def metrics_per_image(gt_rows, gt_counts, pred_rows, pred_counts, dtype=torch.float64):
    """oracle.step_metrics (models/ModelMeta.py:199-214) kept per image: (B,3) = iou sum, recall, precision of each image,
    zeros for an image without predictions.  rows (B,Kmax,5) [score,x,y,w,h]."""
    B = gt_rows.shape[0]
    out = torch.zeros(B, 3, dtype=torch.float64)
    for n in range(B):
        gt = gt_rows[n, :int(gt_counts[n]), 1:].to(dtype).clone()
        pred = pred_rows[n, :int(pred_counts[n]), 1:].to(dtype).clone()
        if pred.shape[0] > 0:                                     # :199
            gt[:, 2] = gt[:, 2] + gt[:, 0]                        # :201-202
            gt[:, 3] = gt[:, 3] + gt[:, 1]
            pred[:, 2] = pred[:, 2] + pred[:, 0]                  # :204-205
            pred[:, 3] = pred[:, 3] + pred[:, 1]
            iou = torch.nan_to_num(O.box_iou(gt, pred), 0)        # :206
            hits = int((iou > 0.5).sum())
            if gt.shape[0] == 0:
                recall = 1.0 if pred.shape[0] == 0 else 0.0       # :207-208
            else:
                recall = hits / gt.shape[0]                       # :210
            out[n, 0] = float(torch.sum(iou))                     # :214
            out[n, 1] = recall
            out[n, 2] = hits / pred.shape[0]                      # :212
    return out


METRIC_COUNTS = ((0, 0), (0, 3), (3, 0), (1, 1), (12, 12), (5, 7))


def metrics_case():
    """B = 6, Kmax = 12, integer boxes: predictions are the ground truth shifted by a few pixels (so some pairs pass 0.5),
    the (1,1) image holds two identical boxes, and the two large images carry zero-area boxes on both sides (iou 0/0)."""
    gen = torch.Generator().manual_seed(9)
    B, K = len(METRIC_COUNTS), 12
    gt, pr = torch.zeros(B, K, 5), torch.zeros(B, K, 5)
    for t in (gt, pr):
        t[:, :, 0] = 1.0
        t[:, :, 1:3] = torch.randint(0, 300, (B, K, 2), generator=gen).float()
        t[:, :, 3:] = torch.randint(8, 120, (B, K, 2), generator=gen).float()
    for n, (G, P) in enumerate(METRIC_COUNTS):
        k = min(G, P)
        pr[n, :k, 1:] = gt[n, :k, 1:] + torch.randint(-6, 7, (k, 4), generator=gen).float()
    pr[3, 0] = gt[3, 0]
    for n in (4, 5):
        gt[n, 1, 3:] = 0.0
        pr[n, 2, 3:] = 0.0
        pr[n, 2, 1:3] = gt[n, 1, 1:3]                              # the same point on both sides: 0 / 0
    gc = torch.tensor([c[0] for c in METRIC_COUNTS], dtype=torch.int32)
    pc = torch.tensor([c[1] for c in METRIC_COUNTS], dtype=torch.int32)
    return gt, gc, pr, pc
