"""Int8 post-training quantisation of PoolResnet and Resnet for inference (include/fdet.h "Int8 inference").

    qp = calibrate(model, frames_iter)                  # float engine over a few frames -> activation scales
    m8 = Int8PoolResnet(model, qp)                      # int8 weights, int32 biases, fp32 multipliers, once
    m8 = Int8PoolResnet(model, qp, stem="integer")      # (opt-in: the integer uint8-frame stem, fdet_stem10_fwd_q8_u8)
    m8 = Int8Resnet(model, qp)                          # (a Resnet; quantize_model picks the class)
    rows, counts = m8.reduce_bounding_boxes.forward_batch(m8.forward_frames(frames))

The residual trunk (every 3x3 conv, both LeakyReLUs, the skip add and the 2x2 max-pool) runs on the integer matrix cores
(fdet_q8_conv3x3; the un-pooled blocks at the end as one fdet_q8_chain launch); the head keeps its float kernel, and the
stem reads uint8 frames and writes the quantised layout itself (fdet_stem_fwd_q8_u8) where it takes the shape.  Resnet's
3x3 / stride 2 stem is an integer kernel of its own (fdet_stem3_fwd_q8_u8): the uint8 frame is its quantised input (scale
1 / 255), so that network is integer from the frame bytes to the head's input and has one arithmetic for every input.  The
reference has no quantised path (its deployment tools are pruner.py and the ONNX / TorchScript exports); the arithmetic is
this project's own contract, restated in numpy by tests/q8_cpu_ref.py, tests/q8_resnet_cpu_ref.py and
tests/q8_pool_stem_cpu_ref.py, and the kernels equal those restatements bit for bit.  Int8PoolResnet(stem="integer") gives
PoolResnet the same kind of stem (fdet_stem10_fwd_q8_u8) in place of the float one; it is opt-in because it changes the
stem's bytes.

    m8 = Int8SeparableCNN(model, qp)                    # (a SeparableCNN: qp carries s_b; quantize_model picks the class)

SeparableCNN enters through that integer stem and runs every separable block as one launch of fdet_q8_sepblock
(the un-pooled tail as one fdet_q8_sepchain launch where measured faster); tests/q8_sep_cpu_ref.py restates the block.

    m8 = Int8SSD(model, calibrate_ssd(model, frames_iter))                  # (an SSD(filters=16); SSD.quantize does both)

SSD has its own scales (SSDQuantParams), calibration (calibrate_ssd) and entries (csrc/fdet_q8.hip: the
Cin -> Cout conv with a floor pool, the 1x1 skip conv, the Linear(C,5) head; csrc/fdet_stem_q8.hip: the 16-filter stem);
tests/q8_ssd_cpu_ref.py
restates them.  `calibrate`, `QuantParams` and `quantize_model` are what they were and refuse an SSD.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import hotpath as hp
from ._native import FdetError

F32 = torch.float32
NPF = np.float32
METHODS = ("absmax", "percentile", "explicit")

# Defaults of the two int8 paths that replace several launches by one (FDET_Q8_CHAIN / FDET_Q8_STEM = "auto"): on only where
# tools/q8_throughput.py measured the new path faster than the launches it replaces by more than the run-to-run spread
# (profiles/r15_q8_chain.json); "1" forces a path wherever its kernel takes the shape, "0" the launches.
CHAIN_MEASURED_FASTER = True
STEM_Q8_MEASURED_FASTER = True
# Int8SeparableCNN's un-pooled tail as one fdet_q8_sepchain launch (FDET_Q8_SEPCHAIN = "auto"): by the same rule, from
# profiles/r19_q8_sep.json
SEPCHAIN_MEASURED_FASTER = True


# ---------------------------------------------------------------------------------------------------------- scales
class QuantParams:
    """Activation scales of the int8 trunk, on the CPU: s_h[k] of block k's input (k = 0..nb; s_h[nb] is the head's input)
    and s_a[k] of block k's first-conv output.  Symmetric, per tensor, float32.  A SeparableCNN has a third list, s_b[k] of
    block k's depthwise output (s_a[k] is its first pointwise output); it is None for the 3x3 models, and files and objects
    without it are what they were."""

    def __init__(self, s_h: Sequence[float], s_a: Sequence[float], method: str = "explicit", percentile: Optional[float] = None,
                 images_seen: int = 0, s_b: Optional[Sequence[float]] = None):
        self.s_h = np.asarray(s_h, dtype=NPF).reshape(-1).copy()
        self.s_a = np.asarray(s_a, dtype=NPF).reshape(-1).copy()
        self.s_b = None if s_b is None else np.asarray(s_b, dtype=NPF).reshape(-1).copy()
        if self.s_a.size < 1 or self.s_h.size != self.s_a.size + 1:
            raise ValueError(f"QuantParams: {self.s_h.size} block-input scales need {self.s_h.size - 1} first-conv scales, "
                             f"got {self.s_a.size}")
        if self.s_b is not None and self.s_b.size != self.s_a.size:
            raise ValueError(f"QuantParams: {self.s_a.size} blocks need {self.s_a.size} depthwise scales, got {self.s_b.size}")
        for name, s in (("s_h", self.s_h), ("s_a", self.s_a)) + ((("s_b", self.s_b),) if self.s_b is not None else ()):
            if not (np.all(np.isfinite(s)) and np.all(s > 0)):
                raise ValueError(f"QuantParams: every scale in {name} must be positive and finite")
        if method not in METHODS:
            raise ValueError(f"QuantParams: method must be one of {METHODS}")
        self.method = method
        self.percentile = None if percentile is None else float(percentile)
        self.images_seen = int(images_seen)

    @property
    def num_blocks(self) -> int:
        return int(self.s_a.size)

    def save(self, path) -> None:
        extra = {} if self.s_b is None else {"s_b": self.s_b}
        np.savez(path, s_h=self.s_h, s_a=self.s_a, method=np.array(self.method),
                 percentile=np.array(np.nan if self.percentile is None else self.percentile, dtype=np.float64),
                 images_seen=np.array(self.images_seen, dtype=np.int64), **extra)

    @classmethod
    def load(cls, path) -> "QuantParams":
        with np.load(path, allow_pickle=False) as z:
            pct = float(z["percentile"])
            return cls(z["s_h"], z["s_a"], str(z["method"]), None if np.isnan(pct) else pct, int(z["images_seen"]),
                       z["s_b"] if "s_b" in z.files else None)

    def __eq__(self, other):
        return (isinstance(other, QuantParams) and np.array_equal(self.s_h, other.s_h) and np.array_equal(self.s_a, other.s_a)
                and (self.s_b is None) == (other.s_b is None) and (self.s_b is None or np.array_equal(self.s_b, other.s_b))
                and (self.method, self.percentile, self.images_seen) == (other.method, other.percentile, other.images_seen))

    def __repr__(self):
        return (f"QuantParams(blocks={self.num_blocks}, method={self.method!r}, percentile={self.percentile}, "
                f"images_seen={self.images_seen})")


class ActivationObserver:
    """Running range of the trunk's activations over calibration batches (torch reductions: offline work).  "absmax": the
    largest magnitude seen.  "percentile": per batch the given percentile of the magnitudes, the largest over the batches."""

    def __init__(self, num_blocks: int, method: str = "absmax", percentile: Optional[float] = None, with_b: bool = False):
        if method not in ("absmax", "percentile"):
            raise ValueError("calibration method must be 'absmax' or 'percentile'")
        if method == "percentile" and not (percentile is not None and 50.0 <= float(percentile) <= 100.0):
            raise ValueError("percentile calibration needs percentile in [50, 100], e.g. 99.99")
        if method == "absmax" and percentile is not None:
            raise ValueError("percentile is given: use method='percentile'")
        self.method, self.percentile = method, (None if percentile is None else float(percentile))
        self.h = [0.0] * (num_blocks + 1)
        self.a = [0.0] * num_blocks
        self.b = [0.0] * num_blocks if with_b else None    # (SeparableCNN: the depthwise outputs)
        self.images = 0

    def _range(self, t: torch.Tensor) -> float:
        m = t.detach().abs().reshape(-1).float()
        if self.method == "absmax" or m.numel() == 1:
            return float(m.max())
        k = min(m.numel(), max(1, int(np.ceil(self.percentile / 100.0 * m.numel()))))
        return float(m.kthvalue(k).values)

    def observe(self, h: List[torch.Tensor], a: List[torch.Tensor], b: Optional[List[torch.Tensor]] = None) -> None:
        """h: the nb + 1 block inputs (the last one is the head's input), a: the nb first-conv outputs, of one batch; b: the nb
        depthwise outputs where the observer was made with_b."""
        if len(h) != len(self.h) or len(a) != len(self.a) or (b is None) != (self.b is None) or (b is not None and len(b) != len(self.b)):
            raise ValueError("ActivationObserver.observe: wrong number of tensors")
        for i, t in enumerate(b or ()):
            self.b[i] = max(self.b[i], self._range(t))
        for i, t in enumerate(h):
            self.h[i] = max(self.h[i], self._range(t))
        for i, t in enumerate(a):
            self.a[i] = max(self.a[i], self._range(t))
        self.images += int(h[0].shape[0])

    def params(self) -> QuantParams:
        if self.images == 0:
            raise ValueError("calibration saw no image")

        def scale(v):                                      # an all-zero tensor quantises with scale 1
            return NPF(1.0) if v == 0.0 else NPF(v) / NPF(127.0)
        return QuantParams([scale(v) for v in self.h], [scale(v) for v in self.a], self.method, self.percentile, self.images,
                           None if self.b is None else [scale(v) for v in self.b])


def _check_model(model):
    from .models.PoolResnet import PoolResnet
    if type(model) is not PoolResnet:
        raise TypeError(f"int8 inference covers PoolResnet only, got {type(model).__name__}")


def _check_resnet(model):
    from .models.Resnet import Resnet
    if type(model) is not Resnet:
        raise TypeError(f"Int8Resnet covers Resnet only, got {type(model).__name__}")


def _check_separable(model):
    from .models.SeparableCNN import SeparableCNN
    if type(model) is not SeparableCNN:
        raise TypeError(f"Int8SeparableCNN covers SeparableCNN only, got {type(model).__name__}")


def _check_calibratable(model):
    from .models.PoolResnet import PoolResnet
    from .models.Resnet import Resnet
    from .models.SeparableCNN import SeparableCNN
    if type(model) not in (PoolResnet, Resnet, SeparableCNN):
        raise TypeError(f"int8 calibration covers SeparableCNN, Resnet and PoolResnet only, got {type(model).__name__}")


STEM_IN_SCALE = NPF(1.0) / NPF(255.0)                   # the scale of a uint8 frame as the integer stem's input code


@torch.no_grad()
def calibrate(model, frames_iter: Iterable[torch.Tensor], method: str = "absmax", percentile: Optional[float] = None) -> QuantParams:
    """Run the float engine (eval arithmetic: no dropout) over the calibration frames and reduce the intermediates it keeps
    for backward to activation scales.  frames_iter yields batches of FRAMES exactly as `forward_frames` takes them: (N,3,H,W)
    with values 0..255, uint8 or float, any size -- they go through the model's own preprocessing (resize, / 255).  Images
    that are already normalised to [0,1] are not frames: passing them would calibrate on nearly black input.
    A PoolResnet, a Resnet or a SeparableCNN (whose engine keeps (x, a, b) per block: the result carries s_b).  Resnet's engine keeps maps wider than 62 columns as column strips; PsTensor.to_f32 undoes
    the strips (fdet_ps_to_f32 plans them from the full width and reads real columns only), so what is observed is plain
    NCHW at every level."""
    from .ps import PsTensor
    _check_calibratable(model)
    if percentile is not None and method == "absmax":
        method = "percentile"
    eng = model.engine
    if eng.p16:
        raise FdetError("calibrate: run the calibration on the bf16x3 engine, not in precision16")
    nb = len(model.residual_blocks)
    sep = model._geometry().kind == "separablecnn"
    obs = ActivationObserver(nb, method, percentile, with_b=sep)
    dev = next(model.parameters()).device
    names, params = model.named_stack_params()
    P = {n: p.detach() for n, p in zip(names, params)}

    def f32(t):
        return t.to_f32() if isinstance(t, PsTensor) else t
    for frames in frames_iter:
        x = model._preprocess(torch.as_tensor(frames).to(dev))
        _, saved = eng.forward(x, P, None, save=True)
        blocks = saved["blocks"]
        obs.observe([f32(b[0]) for b in blocks] + [f32(saved["h_last"])], [f32(b[1]) for b in blocks],
                    [b[2] for b in blocks] if sep else None)
        if not sep:
            saved["ps_scope"].release()
    return obs.params()


def bank_frames(bank, out_hw, max_images: Optional[int] = None, batch_size: int = 16):
    """Calibration frames from a device image bank: its first `max_images` images, each resized whole to out_hw as the
    validation transform does (datasets.augment.default_transform), in batches of uint8 frames (values 0..255, what
    `calibrate` and `forward_frames` take; the transform's second output, not its normalised fp32 images)."""
    from .datasets.augment import DeviceBoxes, default_transform
    n = len(bank) if max_images is None else min(len(bank), int(max_images))
    if n < 1:
        raise ValueError("bank_frames: no calibration image")
    tf = default_transform(tuple(out_hw))
    boxes = DeviceBoxes([np.array([[1.0, 0.0, 0.0, 1.0, 1.0]], dtype=np.float32)] * len(bank), bank.device)   # (the transform wants boxes)
    for a in range(0, n, batch_size):
        yield tf(bank, np.arange(a, min(a + batch_size, n)), boxes, 0)[1]


# ---------------------------------------------------------------------------------------------------------- weights
def prepare_conv(w: np.ndarray, b: np.ndarray, s_in, s_out):
    """One conv's integers: (w_q int8 [Co,Ci,3,3], b_q int32 [Co], mul float32 [Co]).
    s_w[co] = absmax(w[co]) / 127 (1 for a channel of zeros), w_q = clamp(rint(w / s_w)), b_q = rint(b / (s_w * s_in)) in
    float64, mul = (s_w * s_in) / s_out in float32, one rounding per operation."""
    w = np.asarray(w, dtype=NPF)
    m = np.abs(w).reshape(w.shape[0], -1).max(axis=1).astype(NPF)
    s_w = np.where(m == 0, NPF(1.0), m / NPF(127.0)).astype(NPF)
    w_q = np.clip(np.rint(w / s_w[:, None, None, None]), -127, 127).astype(np.int8)
    b_q = np.rint(np.asarray(b, dtype=np.float64) / (s_w.astype(np.float64) * np.float64(NPF(s_in))))
    b_q = np.clip(b_q, -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    mul = ((s_w * NPF(s_in)) / NPF(s_out)).astype(NPF)
    return w_q, b_q, mul


class _Q8Conv:
    def __init__(self, w, b, s_in, s_out, dev):
        w_q, b_q, mul = prepare_conv(w, b, s_in, s_out)
        self.wpk = hp.q8_pack_weights(torch.from_numpy(w_q).to(dev))
        self.bias = torch.from_numpy(b_q).to(dev)
        self.mul = torch.from_numpy(mul).to(dev)


# ---------------------------------------------------------------------------------------------------------- the model
class _Int8Trunk:
    """What Int8PoolResnet and Int8Resnet share: the int8 residual trunk (2 x blocks fdet_q8_conv3x3 launches, or the
    un-pooled tail as one fdet_q8_chain launch that also dequantises -- the same bytes), the float head, the pooled Q8
    buffers and the model surface that the rest of the package asks for (TiledDetector, DetectionEvaluator, GraphedPredict,
    render / tracking / chips).  A subclass supplies the way into the trunk: `_check`, `_init_stem`, `_forward_f32`
    (float images in [0,1] at the model resolution -> maps) and `forward_frames`.  Inference only; weights and scales are
    those at construction.  Int8SeparableCNN replaces the block as well (`_check_levels`, `_init_blocks`, `_trunk`) and keeps
    the rest: buffers, timer, the float head (`_head`), the integer 10x10 stem (`_init_stem10`, `_stem10_u8`), the one-input
    rule and the model surface."""

    training = False
    _check = staticmethod(_check_model)
    COUNTERS = ("chain", "layers", "stem_q8", "stem_f32")

    def __init__(self, model, qparams: QuantParams):
        me = type(self).__name__
        self._check(model)
        if not isinstance(qparams, QuantParams):
            raise TypeError(f"{me}: qparams must be a QuantParams")
        nb = len(model.residual_blocks)
        if qparams.num_blocks != nb:
            raise ValueError(f"{me}: the model has {nb} residual blocks, the scales are for {qparams.num_blocks}")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise FdetError(f"{me} runs on the GPU only (no CPU fallback): move the model to cuda first")
        self.geo = model._geometry()
        self.h0, self.lv = self.geo.levels()
        F_ = int(model.filters)
        self._check_levels(F_)
        self.input_shape = model.input_shape
        self.num_of_patches = model.num_of_patches
        self.filters = F_
        self.probability_threshold = model.probability_threshold
        self.iou_threshold = model.iou_threshold
        self.reduce_bounding_boxes = model.reduce_bounding_boxes
        self.qparams = qparams
        self.device = dev
        self.slope = 0.2
        self._preprocess = model._preprocess               # resize / 255 exactly as the float model
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        self.counters = {k: 0 for k in self.COUNTERS}
        self._init_blocks(sd)
        self._init_stem(model, sd)
        self.head_w = model.out.weight.detach().to(F32).contiguous().clone()
        self.head_b = model.out.bias.detach().to(F32).contiguous().clone()
        self._ws = None
        self._pool = {}                                    # (N,C,H,W) -> free Q8Tensors; kept for the life of the model
        self.timer = None                                  # a convstack.KernelTimer: per-kernel times (tools/q8_throughput.py)

    def _check_levels(self, F_: int) -> None:
        for hk, _ in self.lv:
            if not hp.q8_supported(F_, hk, hk):
                raise FdetError(f"{type(self).__name__}: {F_} channels at {hk}x{hk} are outside the int8 kernels' range "
                                "(fdet_q8_supported: a multiple of 64 up to 256)")

    def _tail_first(self) -> int:
        """Index of the first block of the maximal run of un-pooled blocks at the end of the trunk."""
        first = len(self.lv)
        while first > 0 and self.lv[first - 1][1] != 2:
            first -= 1
        return first

    def _init_blocks(self, sd) -> None:
        nb, dev, F_ = len(self.lv), self.device, self.filters
        s_h, s_a = self.qparams.s_h, self.qparams.s_a
        self.blocks = []
        for k in range(nb):
            n = f"residual_blocks.{k}"
            c1 = _Q8Conv(sd[n + ".conv1.weight"], sd[n + ".conv1.bias"], s_h[k], s_a[k], dev)
            c2 = _Q8Conv(sd[n + ".conv2.weight"], sd[n + ".conv2.bias"], s_a[k], s_h[k + 1], dev)
            self.blocks.append((c1, c2, float(NPF(s_h[k]) / NPF(s_h[k + 1]))))
        # the maximal run of un-pooled blocks at the end of the trunk: one fdet_q8_chain launch where the kernel takes the map
        # (64 channels, at most 16 x 16, 1..16 blocks); its host pointer arrays are built here, once
        self.chain = os.environ.get("FDET_Q8_CHAIN", "auto")          # "0" launch by launch, "1" the chain wherever it runs, else measured
        first = self._tail_first()
        self._chain_first, self._chain_w = nb, None
        if first < nb and nb - first <= hp.Q8_CHAIN_MAX_BLOCKS and hp.q8_chain_supported(F_, self.lv[first][0], self.lv[first][0]):
            tail = self.blocks[first:]
            self._chain_first = first
            self._chain_w = hp.Q8ChainWeights([(c1.wpk, c1.bias, c1.mul) for c1, _, _ in tail],
                                              [(c2.wpk, c2.bias, c2.mul) for _, c2, _ in tail], [sm for _, _, sm in tail], F_)

    # ------------------------------------------------------------------ nn.Module-shaped odds and ends
    def eval(self):
        return self

    def train(self, mode: bool = True):
        if mode:
            raise FdetError(f"{type(self).__name__} is inference only")
        return self

    # ------------------------------------------------------------------ buffers
    def _take(self, N, H, W) -> hp.Q8Tensor:
        free = self._pool.setdefault((N, self.filters, H, W), [])
        return free.pop() if free else hp.Q8Tensor(N, self.filters, H, W, self.device)

    def _give(self, t: hp.Q8Tensor) -> None:
        self._pool.setdefault(t.shape, []).append(t)

    def _t(self, kind, h, flops=0.0, nbytes=0.0):
        from .convstack import _NOSPAN
        return _NOSPAN if self.timer is None else self.timer.span(f"{kind}@{h}x{h}", flops, nbytes)

    # ------------------------------------------------------------------ forward
    def chain_on(self) -> bool:
        """The un-pooled tail runs as one fdet_q8_chain launch."""
        if self._chain_w is None or self.chain == "0":
            return False
        return self.chain == "1" or CHAIN_MEASURED_FASTER

    def _trunk(self, h: hp.Q8Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        """The quantised stem output (taken from the pool; given back here) -> the (N,5,S,S) maps."""
        g, F_, dev = self.geo, self.filters, self.device
        N = h.shape[0]
        s_h = self.qparams.s_h
        if trace is not None:
            trace["blocks"] = []
        chain = self.chain_on()
        nlayer = self._chain_first if chain else len(self.lv)
        for k, (hk, pool) in enumerate(self.lv[:nlayer]):
            c1, c2, skip_mul = self.blocks[k]
            flops = 2.0 * N * F_ * F_ * 9 * hk * hk
            a = self._take(N, hk, hk)
            with self._t("q8_conv3x3", hk, flops, 2.0 * N * F_ * hk * hk):
                hp.q8_conv3x3(h, c1.wpk, c1.bias, c1.mul, a, slope=self.slope)
            out = self._take(N, hk // pool, hk // pool)
            with self._t("q8_conv3x3_pool" if pool == 2 else "q8_conv3x3_skip", hk, flops, (2.0 + 1.0 / (pool * pool)) * N * F_ * hk * hk):
                hp.q8_conv3x3(a, c2.wpk, c2.bias, c2.mul, out, skip=h, skip_mul=skip_mul, pool=pool == 2, slope=self.slope)
            self._give(h)
            self._give(a)
            h = out
            if trace is not None:
                trace["blocks"].append(h.nchw())
        hl = h.shape[2]
        hd = torch.empty(N, F_, hl, hl, dtype=F32, device=dev)
        if chain:
            nb = self._chain_w.nblocks
            outs = [self._take(N, hl, hl) for _ in range(nb)] if trace is not None else None
            with self._t("q8_chain", hl, 2.0 * nb * 2.0 * N * F_ * F_ * 9 * hl * hl, 5.0 * hd.numel()):
                hp.q8_chain(h, self._chain_w, outs=outs, out_f32=hd, out_scale=float(s_h[-1]), slope=self.slope)
            for t in outs or ():
                trace["blocks"].append(t.nchw())
                self._give(t)
            self.counters["chain"] += 1
        else:
            with self._t("q8_dequantize", hl, 0.0, 5.0 * hd.numel()):
                hp.q8_dequantize(h, float(s_h[-1]), out=hd)
            self.counters["layers"] += 1
        self._give(h)
        return self._head(hd, trace)

    def _head(self, hd: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        """The float head on the dequantised last map (N,F,hl,hl) -> (N,5,S,S); S is what the head's kernel and padding leave
        of hl (num_of_patches for PoolResnet and Resnet, whose geometry demands it)."""
        g = self.geo
        N, hl = hd.shape[0], hd.shape[2]
        S = hl + 2 * g.head_p - g.head_k + 1
        y = torch.empty(N, 5, S, S, dtype=F32, device=hd.device)
        with self._t("head_fwd", hl):
            hp.head_fwd(hd, None, self.head_w, self.head_b, y, g.head_k, g.head_p)
        if trace is not None:
            trace["y"] = y
        return y

    # ------------------------------------------------------------------ the integer 10x10 / stride 8 / pad 2 stem
    def _init_stem10(self, sd) -> None:
        g, F_, me = self.geo, self.filters, type(self).__name__
        if (g.stem_k, g.stem_s, g.stem_p) != (10, 8, 2) or not hp.stem10_fwd_q8_ok(1, g.in_ch, F_, g.H, g.W):
            raise FdetError(f"{me}: a {g.in_ch} -> {F_} channel k{g.stem_k} s{g.stem_s} p{g.stem_p} stem on {g.H}x{g.W} "
                            "frames is outside the integer stem's range (fdet_stem10_fwd_q8_ok: 3 channels, k10 s8 p2, F a "
                            "multiple of 64 up to 256, H and W in 6..4096)")
        w_q, b_q, mul = prepare_conv(sd["conv1.weight"], sd["conv1.bias"], STEM_IN_SCALE, self.qparams.s_h[0])
        self.stem_wpk = hp.q8_pack_stem10_weights(torch.from_numpy(w_q).to(self.device))
        self.stem_bias = torch.from_numpy(b_q).to(self.device)
        self.stem_mul = torch.from_numpy(mul).to(self.device)

    def _stem10_u8(self, frames: torch.Tensor, trace: Optional[dict] = None) -> hp.Q8Tensor:
        """uint8 codes at the model resolution -> the integer stem (fdet_stem10_fwd_q8_u8)."""
        g, me = self.geo, type(self).__name__
        if not frames.is_cuda:
            raise FdetError(f"{me} runs on the GPU only (no CPU fallback): move the input to cuda")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (g.in_ch, g.H, g.W):
            raise ValueError(f"expected input (N,{g.in_ch},{g.H},{g.W}), got {tuple(frames.shape)}")
        N, h0 = frames.shape[0], self.h0
        if not hp.stem10_fwd_q8_ok(N, g.in_ch, self.filters, g.H, g.W):
            raise FdetError(f"{me}: {N} images of {g.H}x{g.W} pass the int8 layout's 2 GiB per tensor: use smaller batches")
        h = self._take(N, h0, h0)
        with self._t("stem10_fwd_q8", h0, 2.0 * N * self.filters * 300 * h0 * h0, float(frames.numel()) + N * self.filters * h0 * h0):
            hp.stem10_fwd_q8_u8(frames.contiguous(), self.stem_wpk, self.stem_bias, self.stem_mul, h)
        self.counters["stem_q8"] += 1
        if trace is not None:
            trace["stem"] = h.nchw()
        return h

    # ------------------------------------------------------------------ the one-input rule of the integer stems
    @staticmethod
    def _codes(x: torch.Tensor) -> torch.Tensor:
        """float images in [0,1] -> the uint8 codes of the stem's input scale 1 / 255 (torch ops; NaN -> 0)."""
        return torch.nan_to_num(x.to(F32)).mul(255.0).round_().clamp_(0.0, 255.0).to(torch.uint8)

    def _forward_any(self, x: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        """Frames of any kind through an integer stem (`_stem_u8`): uint8 frames on the GPU at the model resolution as they
        are, everything else through `_preprocess` and `_codes`."""
        g = self.geo
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.is_cuda and x.dtype == torch.uint8 and x.dim() == 4 and tuple(x.shape[1:]) == (g.in_ch, g.H, g.W):
            return self._trunk(self._stem_u8(x, trace), trace)
        return self._forward_f32(self._preprocess(x), trace)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, predict: torch.Tensor = torch.tensor(0)):
        """The float model's forward: float images in [0,1] at the model resolution -> maps; predict=1: frames -> boxes of
        image 0."""
        if predict == 1:
            return self.single_non_max_suppression(self.forward_frames(x)[0])
        return self._forward_f32(x)

    forward = __call__

    def non_max_suppression(self, x):
        from .models.BaseModel import split_rows
        if len(x.shape) == 4:
            return split_rows(*self.reduce_bounding_boxes.forward_batch(x))
        return self.reduce_bounding_boxes(x)

    def single_non_max_suppression(self, x):
        return self.reduce_bounding_boxes(x)

    @torch.no_grad()
    def predict(self, x, probability_threshold=0.5, iou_threshold=0.5):
        from .datasets.utils import ReduceBoundingBoxes
        self.reduce_bounding_boxes = ReduceBoundingBoxes(
            probability_threshold=probability_threshold, iou_threshold=iou_threshold,
            input_shape=self.input_shape, num_of_patches=self.num_of_patches)
        image = self._preprocess(x)
        return image, self.non_max_suppression(self._forward_f32(image))[0]

    def graphed_predict(self, example: torch.Tensor):
        from .models.BaseModel import GraphedPredict
        return GraphedPredict(self, example)


class Int8PoolResnet(_Int8Trunk):
    """A trained PoolResnet with its residual trunk in int8: existing stem -> quantise -> 2 x blocks int8 convs ->
    dequantise -> existing head; or, where switched on (FDET_Q8_STEM / FDET_Q8_CHAIN, `counters`), the quantising stem on
    the uint8 frames and the un-pooled tail of the trunk as one launch that also dequantises -- the same bytes.  Inference
    only; weights and scales are those at construction.  It offers what the rest of the package asks of a model
    (TiledDetector, DetectionEvaluator, GraphedPredict, render / tracking / chips).

    stem="float" (the default) is the path above.  stem="integer" replaces the float stem by the integer kernel
    fdet_stem10_fwd_q8_u8: the uint8 frame is the stem's quantised input (scale 1 / 255), its weights are prepared as a trunk
    conv's, and Int8Resnet's one-input rule holds -- uint8 frames on the GPU at the model resolution go to the kernel as they
    are, everything else through `_preprocess` and `_codes` to the same kernel.  No float stem, no `/ 255` pass, no quantise
    launch and no FDET_Q8_STEM lookup; the stem's bytes differ from the float stem's (by at most one code on the trained
    archive), which is why it is opt-in.  F = 128 and 256 models are accepted (their trunk runs launch by launch)."""

    STEMS = ("float", "integer")

    def __init__(self, model, qparams: QuantParams, stem: str = "float"):
        if stem not in self.STEMS:
            raise ValueError(f"Int8PoolResnet: stem must be one of {self.STEMS}, got {stem!r}")
        self.stem = stem
        super().__init__(model, qparams)

    def _init_stem(self, model, sd) -> None:
        g, F_ = self.geo, self.filters
        if self.stem == "integer":
            self._init_stem10(sd)
            return
        self.stem_w = model.conv1.weight.detach().to(F32).contiguous().clone()
        self.stem_b = model.conv1.bias.detach().to(F32).contiguous().clone()
        self._stem_x3 = hp.x3_supported(F_, F_) and hp.stem_x3_supported(g.in_ch, g.W, g.stem_k, g.stem_s, g.stem_p)
        self.stem_q8 = os.environ.get("FDET_Q8_STEM", "auto")         # "0" float stem + quantise, "1" the quantising stem wherever it runs

    def stem_q8_on(self, N: int) -> bool:
        """uint8 frames at the model resolution go through the quantising stem (fdet_stem_fwd_q8_u8)."""
        g = self.geo
        if self.stem == "integer":                                    # (that stem has one route and no switch)
            return False
        if self.stem_q8 == "0" or not (self.stem_q8 == "1" or STEM_Q8_MEASURED_FASTER):
            return False
        return hp.stem_fwd_q8_ok(N, g.in_ch, self.filters, g.H, g.W, g.stem_k, g.stem_s, g.stem_p)

    def _stem_f32(self, x: torch.Tensor, trace: Optional[dict] = None) -> hp.Q8Tensor:
        """fp32 images in [0,1] -> float stem -> quantise."""
        g, F_ = self.geo, self.filters
        if not x.is_cuda:
            raise FdetError("Int8PoolResnet runs on the GPU only (no CPU fallback): move the input to cuda")
        if x.dim() != 4 or tuple(x.shape[1:]) != (g.in_ch, g.H, g.W):
            raise ValueError(f"expected input (N,{g.in_ch},{g.H},{g.W}), got {tuple(x.shape)}")
        if x.dtype != F32 or not x.is_contiguous():
            x = x.to(F32).contiguous()
        N, dev = x.shape[0], x.device
        nws = hp.stem_ws_bytes(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p)
        if self._ws is None or self._ws.numel() * 4 < nws:
            self._ws = torch.empty(max((nws + 3) // 4, 4), dtype=F32, device=dev)
        h0 = self.h0
        hf = torch.empty(N, F_, h0, h0, dtype=F32, device=dev)
        with self._t("stem_fwd", h0):
            hp.stem_fwd(x, self.stem_w, self.stem_b, hf, self._ws, g.stem_k, g.stem_s, g.stem_p, x3=self._stem_x3)
        h = self._take(N, h0, h0)
        with self._t("q8_quantize", h0, 0.0, 5.0 * hf.numel()):
            hp.q8_quantize(hf, float(self.qparams.s_h[0]), out=h)
        self.counters["stem_f32"] += 1
        if trace is not None:
            trace["stem"] = hf
        return h

    def _stem_i8(self, frames: torch.Tensor, trace: Optional[dict] = None) -> hp.Q8Tensor:
        """stem="integer": uint8 codes at the model resolution -> the integer stem."""
        return self._stem10_u8(frames, trace)

    def _stem_u8(self, frames: torch.Tensor, trace: Optional[dict] = None) -> hp.Q8Tensor:
        """uint8 frames at the model resolution -> the quantising stem: no fp32 image, no fp32 stem output (stem="integer":
        the integer stem)."""
        if self.stem == "integer":
            return self._stem_i8(frames, trace)
        g = self.geo
        N, h0 = frames.shape[0], self.h0
        h = self._take(N, h0, h0)
        with self._t("stem_fwd_q8", h0, 0.0, float(frames.numel()) + N * self.filters * h0 * h0):
            hp.stem_fwd_q8_u8(frames, self.stem_w, self.stem_b, float(self.qparams.s_h[0]), h, g.stem_k, g.stem_s, g.stem_p)
        self.counters["stem_q8"] += 1
        return h

    def _forward_f32(self, x: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        if self.stem == "integer":
            if not x.is_cuda:
                raise FdetError("Int8PoolResnet runs on the GPU only (no CPU fallback): move the input to cuda")
            return self._trunk(self._stem_i8(self._codes(x), trace), trace)
        return self._trunk(self._stem_f32(x, trace), trace)

    @torch.no_grad()
    def forward_frames(self, x: torch.Tensor) -> torch.Tensor:
        """frames (uint8 or float, any size) -> the (N,5,S,S) maps, as BaseModel.forward_frames.  uint8 frames on the GPU
        that are already at the model resolution go to the quantising stem as they are (where it is switched on and takes
        the shape): no `/ 255` pass, no fp32 stem output, no quantise launch, the same bytes.  stem="integer": every input
        reaches the integer stem (`_forward_any`)."""
        if self.stem == "integer":
            return self._forward_any(x)
        g = self.geo
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if (x.is_cuda and x.dtype == torch.uint8 and x.dim() == 4 and tuple(x.shape[1:]) == (g.in_ch, g.H, g.W)
                and self.stem_q8_on(x.shape[0])):
            return self._trunk(self._stem_u8(x.contiguous()))
        return self._forward_f32(self._preprocess(x))

    @torch.no_grad()
    def trace(self, frames: torch.Tensor) -> dict:
        """{"stem": fp32 stem output (N,F,h0,h0) -- stem="integer": the int8 stem output --, "blocks": [int8 (N,F,h,h) output
        of every block], "y": (N,5,S,S)}"""
        out = {}
        if self.stem == "integer":
            self._forward_any(frames, trace=out)
        else:
            self._forward_f32(self._preprocess(frames), trace=out)
        return out


class Int8Resnet(_Int8Trunk):
    """A trained Resnet (3x3 / stride 2 stem, pooling while the map is larger than S) in int8 from the frame bytes to the
    head's input: the integer stem on the uint8 frames (fdet_stem3_fwd_q8_u8; the frame is its quantised input, scale
    1 / 255, and s_h[0] its output scale), the shared int8 trunk, the float head.  ONE input rule and one arithmetic: uint8
    frames on the GPU at the model resolution go to the stem as they are; everything else (other sizes, float frames, float
    images in [0,1] through `__call__`) goes through the model's `_preprocess` and is turned into codes by
    clamp(rint(nan_to_num(x) * 255), 0, 255) with torch ops -- for images that came from uint8 frames that recovers the
    bytes -- and goes to the same stem.  There is no float stem here and so no second set of bytes."""

    _check = staticmethod(_check_resnet)

    def _init_stem(self, model, sd) -> None:
        g, F_ = self.geo, self.filters
        if (g.stem_k, g.stem_s, g.stem_p) != (3, 2, 1) or not hp.stem3_fwd_q8_ok(1, g.in_ch, F_, g.H, g.W):
            raise FdetError(f"Int8Resnet: a {g.in_ch} -> {F_} channel stem on {g.H}x{g.W} frames is outside the integer stem's "
                            "range (fdet_stem3_fwd_q8_ok: 3 channels, F a multiple of 64 up to 256, even H and W up to 4096)")
        w_q, b_q, mul = prepare_conv(sd["conv1.weight"], sd["conv1.bias"], STEM_IN_SCALE, self.qparams.s_h[0])
        self.stem_wpk = hp.q8_pack_stem_weights(torch.from_numpy(w_q).to(self.device))
        self.stem_bias = torch.from_numpy(b_q).to(self.device)
        self.stem_mul = torch.from_numpy(mul).to(self.device)

    def _stem_u8(self, frames: torch.Tensor, trace: Optional[dict] = None) -> hp.Q8Tensor:
        """uint8 codes at the model resolution -> the integer stem."""
        g = self.geo
        if not frames.is_cuda:
            raise FdetError("Int8Resnet runs on the GPU only (no CPU fallback): move the input to cuda")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (g.in_ch, g.H, g.W):
            raise ValueError(f"expected input (N,{g.in_ch},{g.H},{g.W}), got {tuple(frames.shape)}")
        N, h0 = frames.shape[0], self.h0
        if not hp.stem3_fwd_q8_ok(N, g.in_ch, self.filters, g.H, g.W):
            raise FdetError(f"Int8Resnet: {N} images of {g.H}x{g.W} pass the int8 layout's 2 GiB per tensor: use smaller batches")
        h = self._take(N, h0, h0)
        with self._t("stem3_fwd_q8", h0, 2.0 * N * self.filters * 27 * h0 * h0, float(frames.numel()) + N * self.filters * h0 * h0):
            hp.stem3_fwd_q8_u8(frames.contiguous(), self.stem_wpk, self.stem_bias, self.stem_mul, h)
        self.counters["stem_q8"] += 1
        if trace is not None:
            trace["stem"] = h.nchw()
        return h

    def _forward_f32(self, x: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        if not x.is_cuda:
            raise FdetError("Int8Resnet runs on the GPU only (no CPU fallback): move the input to cuda")
        return self._trunk(self._stem_u8(self._codes(x), trace), trace)

    @torch.no_grad()
    def forward_frames(self, x: torch.Tensor) -> torch.Tensor:
        """frames (uint8 or float, any size) -> the (N,5,S,S) maps, as BaseModel.forward_frames."""
        return self._forward_any(x)

    @torch.no_grad()
    def trace(self, frames: torch.Tensor) -> dict:
        """{"stem": int8 stem output (N,F,h0,h0), "blocks": [int8 (N,F,h,h) output of every block], "y": (N,5,S,S)}"""
        out = {}
        self._forward_any(frames, trace=out)
        return out


def prepare_sepblock(w1, wd, w2, s_in, s_a, s_b, s_out):
    """One separable block's integers (include/fdet.h, "Int8 inference: the separable block"): (w1_q int8 [C,C,1,1], mul1,
    wd_q int8 [C,1,3,3], mul2, w2_q int8 [C,C,1,1], mul3, skip_mul), each conv prepared as `prepare_conv` does, without a bias."""
    zero = np.zeros(np.asarray(w1).shape[0], NPF)
    w1_q, _, mul1 = prepare_conv(w1, zero, s_in, s_a)
    wd_q, _, mul2 = prepare_conv(wd, zero, s_a, s_b)
    w2_q, _, mul3 = prepare_conv(w2, zero, s_b, s_out)
    return w1_q, mul1, wd_q, mul2, w2_q, mul3, NPF(NPF(s_in) / NPF(s_out))


class Int8SeparableCNN(_Int8Trunk):
    """A SeparableCNN in int8 from the frame bytes to the head's input: the integer 10x10 stem on the uint8 frames
    (fdet_stem10_fwd_q8_u8, PoolResnet's integer stem: conv1 is the same conv), every separable block as one launch of
    fdet_q8_sepblock (pw1, LeakyReLU, depthwise 3x3, LeakyReLU, pw2, skip and the 2x2 max, requantised after each stage), the
    un-pooled blocks at the end as one fdet_q8_sepchain launch where that is switched on (FDET_Q8_SEPCHAIN: "0" launch by
    launch, "1" the chain wherever it runs, otherwise SEPCHAIN_MEASURED_FASTER) -- the same bytes --, the float head.  One
    input rule and one arithmetic, as Int8Resnet: there is no float stem.  F = 128 models run launch by launch (the chain is
    built for 64 channels).  `qparams` carries s_b (calibrate on a SeparableCNN gives it).  `counters`: "sepchain" chain
    launches, "sepblocks" fdet_q8_sepblock launches, "stem_q8" stem launches.  Accuracy is pinned on seeded random models
    only: no trained SeparableCNN archive exists."""

    _check = staticmethod(_check_separable)
    COUNTERS = ("sepchain", "sepblocks", "stem_q8")

    def __init__(self, model, qparams: QuantParams):
        if isinstance(qparams, QuantParams) and qparams.s_b is None:
            _check_separable(model)
            raise ValueError("Int8SeparableCNN: the scales lack s_b (the depthwise outputs): calibrate on the SeparableCNN")
        super().__init__(model, qparams)

    def _check_levels(self, F_: int) -> None:
        for hk, _ in self.lv:
            if not hp.q8_sepblock_supported(F_, hk, hk):
                raise FdetError(f"Int8SeparableCNN: {F_} channels at {hk}x{hk} are outside the int8 block's range "
                                "(fdet_q8_sepblock_supported: 64 or 128 channels, maps up to 4096 a side)")

    def _init_blocks(self, sd) -> None:
        nb, dev, F_ = len(self.lv), self.device, self.filters
        q = self.qparams
        self.blocks = []
        for k in range(nb):
            n = f"residual_blocks.{k}"
            w1_q, mul1, wd_q, mul2, w2_q, mul3, sm = prepare_sepblock(
                sd[n + ".pointwise_conv1.weight"], sd[n + ".depthwise_conv.weight"], sd[n + ".pointwise_conv2.weight"],
                q.s_h[k], q.s_a[k], q.s_b[k], q.s_h[k + 1])

            def t(a):
                return torch.from_numpy(a).to(dev)
            self.blocks.append((hp.q8_pack_sep_pw(t(w1_q)), t(mul1), hp.q8_pack_sep_dw(t(wd_q)), t(mul2), hp.q8_pack_sep_pw(t(w2_q)),
                                t(mul3), float(sm)))
        self.chain = os.environ.get("FDET_Q8_SEPCHAIN", "auto")
        first = self._tail_first()
        self._chain_first, self._chain_w = nb, None
        if first < nb and nb - first <= hp.Q8_CHAIN_MAX_BLOCKS and hp.q8_sepchain_supported(F_, self.lv[first][0], self.lv[first][0]):
            self._chain_first = first
            self._chain_w = hp.Q8SepChainWeights([b[:6] for b in self.blocks[first:]], [b[6] for b in self.blocks[first:]], F_)

    def _init_stem(self, model, sd) -> None:
        self._init_stem10(sd)

    def chain_on(self) -> bool:
        """The un-pooled tail runs as one fdet_q8_sepchain launch."""
        if self._chain_w is None or self.chain == "0":
            return False
        return self.chain == "1" or SEPCHAIN_MEASURED_FASTER

    def _trunk(self, h: hp.Q8Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        """The quantised stem output (taken from the pool; given back here) -> the head's maps."""
        F_, dev = self.filters, self.device
        N = h.shape[0]
        if trace is not None:
            trace["blocks"] = []
        chain = self.chain_on()
        nlayer = self._chain_first if chain else len(self.lv)
        for k, (hk, pool) in enumerate(self.lv[:nlayer]):
            *w, skip_mul = self.blocks[k]
            out = self._take(N, hk // pool, hk // pool)
            # 2 F + 9 MACs per channel and position; compulsory bytes: x in, y out
            with self._t("q8_sepblock_pool" if pool == 2 else "q8_sepblock", hk, 2.0 * N * F_ * (2 * F_ + 9) * hk * hk,
                         (1.0 + 1.0 / (pool * pool)) * N * F_ * hk * hk):
                hp.q8_sepblock(h, *w, skip_mul, out, pool=pool == 2, slope=self.slope)
            self.counters["sepblocks"] += 1
            self._give(h)
            h = out
            if trace is not None:
                trace["blocks"].append(h.nchw())
        hl = h.shape[2]
        hd = torch.empty(N, F_, hl, hl, dtype=F32, device=dev)
        s_last = float(self.qparams.s_h[-1])
        if chain:
            nb = self._chain_w.nblocks
            outs = [self._take(N, hl, hl) for _ in range(nb)] if trace is not None else None
            with self._t("q8_sepchain", hl, nb * 2.0 * N * F_ * (2 * F_ + 9) * hl * hl, 5.0 * hd.numel()):
                hp.q8_sepchain(h, self._chain_w, outs=outs, out_f32=hd, out_scale=s_last, slope=self.slope)
            for t in outs or ():
                trace["blocks"].append(t.nchw())
                self._give(t)
            self.counters["sepchain"] += 1
        else:
            with self._t("q8_dequantize", hl, 0.0, 5.0 * hd.numel()):
                hp.q8_dequantize(h, s_last, out=hd)
        self._give(h)
        return self._head(hd, trace)

    def _stem_u8(self, frames: torch.Tensor, trace: Optional[dict] = None) -> hp.Q8Tensor:
        return self._stem10_u8(frames, trace)

    def _forward_f32(self, x: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        if not x.is_cuda:
            raise FdetError("Int8SeparableCNN runs on the GPU only (no CPU fallback): move the input to cuda")
        return self._trunk(self._stem_u8(self._codes(x), trace), trace)

    @torch.no_grad()
    def forward_frames(self, x: torch.Tensor) -> torch.Tensor:
        """frames (uint8 or float, any size) -> the head's maps, as BaseModel.forward_frames."""
        return self._forward_any(x)

    @torch.no_grad()
    def trace(self, frames: torch.Tensor) -> dict:
        """{"stem": int8 stem output (N,F,h0,h0), "blocks": [int8 (N,F,h,h) output of every block], "y": the head's maps}"""
        out = {}
        self._forward_any(frames, trace=out)
        return out


# ---------------------------------------------------------------------------------------------------------- SSD
SSD_QPARAMS_VERSION = 1


class SSDQuantParams:
    """Activation scales of the int8 SSD, on the CPU: s_h[k] of block k's input (k = 0..nb; s_h[nb] is the last
    head's input), s_a[k] of block k's first-conv output, and s_k[j] of the 1x1 skip conv's output of the j-th block whose
    width changes (in block order).  Symmetric, per tensor, float32.  Its own class and its own versioned file (its arrays carry
    their own names, so neither class reads the other's file): QuantParams and its files are what they were."""

    def __init__(self, s_h: Sequence[float], s_a: Sequence[float], s_k: Sequence[float], method: str = "explicit",
                 percentile: Optional[float] = None, images_seen: int = 0):
        self.s_h = np.asarray(s_h, dtype=NPF).reshape(-1).copy()
        self.s_a = np.asarray(s_a, dtype=NPF).reshape(-1).copy()
        self.s_k = np.asarray(s_k, dtype=NPF).reshape(-1).copy()
        if self.s_a.size < 1 or self.s_h.size != self.s_a.size + 1:
            raise ValueError(f"SSDQuantParams: {self.s_h.size} block-input scales need {self.s_h.size - 1} first-conv scales, "
                             f"got {self.s_a.size}")
        if self.s_k.size > self.s_a.size:
            raise ValueError(f"SSDQuantParams: {self.s_k.size} skip-conv scales for {self.s_a.size} blocks")
        for name, s in (("s_h", self.s_h), ("s_a", self.s_a), ("s_k", self.s_k)):
            if not (np.all(np.isfinite(s)) and np.all(s > 0)):
                raise ValueError(f"SSDQuantParams: every scale in {name} must be positive and finite")
        if method not in METHODS:
            raise ValueError(f"SSDQuantParams: method must be one of {METHODS}")
        self.method = method
        self.percentile = None if percentile is None else float(percentile)
        self.images_seen = int(images_seen)

    @property
    def num_blocks(self) -> int:
        return int(self.s_a.size)

    def save(self, path) -> None:
        np.savez(path, kind=np.array("ssd"), version=np.array(SSD_QPARAMS_VERSION, dtype=np.int64), ssd_s_h=self.s_h,
                 ssd_s_a=self.s_a, ssd_s_k=self.s_k, method=np.array(self.method),
                 percentile=np.array(np.nan if self.percentile is None else self.percentile, dtype=np.float64),
                 images_seen=np.array(self.images_seen, dtype=np.int64))

    @classmethod
    def load(cls, path) -> "SSDQuantParams":
        with np.load(path, allow_pickle=False) as z:
            if "kind" not in z.files or str(z["kind"]) != "ssd":
                raise ValueError("SSDQuantParams.load: not an SSD scale file")
            if int(z["version"]) != SSD_QPARAMS_VERSION:
                raise ValueError(f"SSDQuantParams.load: file version {int(z['version'])}, this code reads {SSD_QPARAMS_VERSION}")
            pct = float(z["percentile"])
            return cls(z["ssd_s_h"], z["ssd_s_a"], z["ssd_s_k"], str(z["method"]), None if np.isnan(pct) else pct, int(z["images_seen"]))

    def __eq__(self, other):
        return (isinstance(other, SSDQuantParams) and np.array_equal(self.s_h, other.s_h) and np.array_equal(self.s_a, other.s_a)
                and np.array_equal(self.s_k, other.s_k)
                and (self.method, self.percentile, self.images_seen) == (other.method, other.percentile, other.images_seen))

    def __repr__(self):
        return (f"SSDQuantParams(blocks={self.num_blocks}, skips={self.s_k.size}, method={self.method!r}, "
                f"percentile={self.percentile}, images_seen={self.images_seen})")


def _check_ssd(model, me: str):
    from .models.SSD import SSD
    if type(model) is not SSD:
        raise TypeError(f"{me} covers SSD only, got {type(model).__name__}")


def _ssd_preprocess(model, x: torch.Tensor) -> torch.Tensor:
    """Frames -> float images in [0,1] at the model resolution: the preprocessing of SSD.forward(x, predict=1)."""
    if x.dim() == 3:
        x = x.unsqueeze(0)
    size = tuple(model.input_shape[1:])
    return hp.resize_bilinear_norm(x, size) if tuple(x.shape[-2:]) != size or x.dtype == torch.uint8 else x.float() / 255.0


@torch.no_grad()
def calibrate_ssd(model, frames_iter: Iterable[torch.Tensor], method: str = "absmax",
                  percentile: Optional[float] = None) -> SSDQuantParams:
    """`calibrate` for an SSD: the float bf16x3 engine (eval arithmetic) over frames as `forward_frames` takes them, its saved
    block inputs, skip-conv outputs, first-conv outputs and head inputs reduced to scales by ActivationObserver's range rule."""
    _check_ssd(model, "calibrate_ssd")
    if percentile is not None and method == "absmax":
        method = "percentile"
    eng = model.engine
    if eng.p16:
        raise FdetError("calibrate_ssd: run the calibration on the bf16x3 engine, not in precision16")
    specs = eng.specs
    nb = len(specs)
    obs = ActivationObserver(nb, method, percentile)
    wide = [k for k, s in enumerate(specs) if s[1] != s[2]]
    k_range = [0.0] * len(wide)
    dev = next(model.parameters()).device
    names, params = model.named_stack_params()
    P = {n: p.detach() for n, p in zip(names, params)}
    nheads = len(model.patch_sizes)
    for frames in frames_iter:
        x = _ssd_preprocess(model, torch.as_tensor(frames).to(dev))
        _, saved = eng.forward(x, P, None, save=True)
        blocks = saved["blocks"]
        obs.observe([b[0] for b in blocks] + [saved["heads"][nheads - 1]], [b[2] for b in blocks])
        for j, k in enumerate(wide):
            k_range[j] = max(k_range[j], obs._range(blocks[k][1]))
        for i in range(nheads - 1):                        # (heads 0..2 read the inputs of the blocks after them: the same tensors)
            k_in = nb - (nheads - 1) + i
            obs.h[k_in] = max(obs.h[k_in], obs._range(saved["heads"][i]))
    q = obs.params()
    return SSDQuantParams(q.s_h, q.s_a, [NPF(1.0) if v == 0.0 else NPF(v) / NPF(127.0) for v in k_range], q.method, q.percentile,
                          q.images_seen)


def prepare_head(w: np.ndarray, b: np.ndarray, s_in):
    """One Linear(C,5) head's integers: (w_q int8 [5,C], b_q int32 [5], m float32 [5]) with s_w[o] = absmax(w[o]) / 127 (1 for
    a row of zeros), b_q = rint(b / (s_w * s_in)) in float64 and m = s_w * s_in, one float32 multiply."""
    w = np.asarray(w, dtype=NPF)
    w_q, b_q, _ = prepare_conv(w.reshape(w.shape[0], -1, 1, 1), b, s_in, NPF(1.0))
    a = np.abs(w).max(axis=1).astype(NPF)
    s_w = np.where(a == 0, NPF(1.0), a / NPF(127.0)).astype(NPF)
    return w_q.reshape(w.shape), b_q, (s_w * NPF(s_in)).astype(NPF)


class _Q8XConv:
    def __init__(self, w, b, s_in, s_out, dev):
        w_q, b_q, mul = prepare_conv(w, b, s_in, s_out)
        self.wpk = hp.q8x_pack_weights(torch.from_numpy(w_q).to(dev))
        self.bias = torch.from_numpy(b_q).to(dev)
        self.mul = torch.from_numpy(mul).to(dev)


class Int8SSD:
    """An SSD(filters=16) at 480x480 in int8 from the frame bytes to the heads' outputs: the integer stem on the
    uint8 frames (fdet_stem3_fwd_q8x_u8), thirteen residual blocks on the integer matrix cores (fdet_q8x_conv3x3 with the
    skip add and the floor pool in its epilogue; fdet_q8x_pointwise for the 1x1 skip conv of the blocks whose width changes),
    the four Linear(C,5) heads as integer dot products (fdet_q8x_head_f32), and the float sigmoid-and-priors kernel
    (fdet_ssd_head_pack_fwd).  One input rule, as Int8Resnet: uint8 frames on the GPU at the model resolution go to the stem
    as they are; everything else goes through the model's preprocessing and `_codes` to the same stem.

    Inference only, GPU only, eval arithmetic; weights and scales are those at construction.  The Q8 buffers of a batch size
    are made (zero-filled) on the first call with it and the (N,4774,5) output is preallocated: a later call with the same N
    allocates nothing, runs on one stream without a host synchronisation and can be captured in a HIP graph.  The returned
    tensor is that buffer: the next call with the same N overwrites it.  Accuracy on trained weights is unpinned (no trained
    SSD archive exists); the tests pin the arithmetic and the quantisation error of a seeded model."""

    training = False
    COUNTERS = ("stem_q8", "convs", "pointwise", "heads")

    def __init__(self, model, qparams: SSDQuantParams):
        _check_ssd(model, "Int8SSD")
        if not isinstance(qparams, SSDQuantParams):
            raise TypeError("Int8SSD: qparams must be an SSDQuantParams")
        if int(model.filters) != 16 or tuple(model.input_shape) != (3, 480, 480):
            raise ValueError(f"Int8SSD: filters=16 at 480x480 only, got filters={model.filters} at {tuple(model.input_shape)}: a "
                             "wider model exceeds the 256 channels of the int8 kernels")
        from .ssdstack import PATCH_SIZES, block_specs
        self.specs = block_specs(16)
        nb = len(self.specs)
        self.wide = [k for k, s in enumerate(self.specs) if s[1] != s[2]]
        if qparams.num_blocks != nb or qparams.s_k.size != len(self.wide):
            raise ValueError(f"Int8SSD: the model has {nb} blocks, {len(self.wide)} of them with a skip conv; the scales are for "
                             f"{qparams.num_blocks} and {qparams.s_k.size}")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise FdetError("Int8SSD runs on the GPU only (no CPU fallback): move the model to cuda first")
        self.input_shape = model.input_shape
        self.patch_sizes = tuple(model.patch_sizes)
        self.filters = 16
        self.size = 480
        self.probability_threshold = model.probability_threshold
        self.iou_threshold = model.iou_threshold
        self.reduce_bounding_boxes = model.reduce_bounding_boxes
        self.qparams = qparams
        self.device = dev
        self.slope = 0.2
        self.starts = [0]
        for ps in PATCH_SIZES:
            self.starts.append(self.starts[-1] + ps * ps)
        self.P = self.starts[-1]
        self.counters = {k: 0 for k in self.COUNTERS}
        self.timer = None                                  # a convstack.KernelTimer: per-kernel times (tools/q8_throughput.py)
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        s_h, s_a, s_k = qparams.s_h, qparams.s_a, qparams.s_k
        w_q, b_q, mul = prepare_conv(sd["input_normalizer.weight"], sd["input_normalizer.bias"], STEM_IN_SCALE, s_h[0])
        self.stem_wpk = hp.q8x_pack_stem_weights(torch.from_numpy(w_q).to(dev))
        self.stem_bias = torch.from_numpy(b_q).to(dev)
        self.stem_mul = torch.from_numpy(mul).to(dev)
        self.blocks, self.heads = [], {}
        for k, (name, ci, co, pool, head) in enumerate(self.specs):
            c1 = _Q8XConv(sd[name + ".conv1.weight"], sd[name + ".conv1.bias"], s_h[k], s_a[k], dev)
            c2 = _Q8XConv(sd[name + ".conv2.weight"], sd[name + ".conv2.bias"], s_a[k], s_h[k + 1], dev)
            if ci != co:
                sk = s_k[self.wide.index(k)]
                cs = _Q8XConv(sd[name + ".pointwise_conv_skip.weight"], sd[name + ".pointwise_conv_skip.bias"], s_h[k], sk, dev)
                skip_mul = float(NPF(sk) / NPF(s_h[k + 1]))
            else:
                cs, skip_mul = None, float(NPF(s_h[k]) / NPF(s_h[k + 1]))
            self.blocks.append((c1, c2, cs, skip_mul))
            if head >= 0:
                hn = f"extracting_layers.{head}.0"
                hw, hb, hm = prepare_head(sd[hn + ".weight"], sd[hn + ".bias"], s_h[k + 1])
                self.heads[k] = (head, torch.from_numpy(hw).to(dev).contiguous(), torch.from_numpy(hb).to(dev),
                                 torch.from_numpy(hm).to(dev))
        self._model_preprocess = lambda x: _ssd_preprocess(model, x)
        self._plans = {}                                   # N -> the buffers of one pass; kept for the life of the model

    # ------------------------------------------------------------------ nn.Module-shaped odds and ends
    def eval(self):
        return self

    def train(self, mode: bool = True):
        if mode:
            raise FdetError("Int8SSD is inference only")
        return self

    _codes = staticmethod(_Int8Trunk._codes)

    def _preprocess(self, x: torch.Tensor) -> torch.Tensor:
        return self._model_preprocess(x)

    def _t(self, kind, h, ci, co, flops=0.0, nbytes=0.0):
        from .convstack import _NOSPAN
        return _NOSPAN if self.timer is None else self.timer.span(f"{kind}@{h}x{h}:{ci}->{co}", flops, nbytes)

    # ------------------------------------------------------------------ buffers
    def _plan(self, N: int) -> dict:
        """The buffers of a pass over N images, made once: per block its input, first-conv output, skip-conv output (or None)
        and output.  Buffers of one shape are shared where their lives do not overlap."""
        plan = self._plans.get(N)
        if plan is not None:
            return plan
        if not hp.stem3_fwd_q8x_ok(N, 3, 16, self.size, self.size) or not hp.q8x_act_bytes(N, 32, 240, 240):
            raise FdetError(f"Int8SSD: {N} images pass the int8 layout's 2 GiB per tensor: use smaller batches")
        dev, free = self.device, {}

        def take(C, H):
            lst = free.setdefault((C, H), [])
            return lst.pop() if lst else hp.Q8XTensor(N, C, H, H, dev)

        def give(t):
            free.setdefault((t.shape[1], t.shape[2]), []).append(t)
        h = take(16, self.size // 2)
        steps = []
        for name, ci, co, pool, head in self.specs:
            hk = h.shape[2]
            sk = take(co, hk) if ci != co else None
            a = take(co, hk)
            out = take(co, hk // 2 if pool else hk)
            steps.append((h, a, sk, out))
            give(h)
            give(a)
            if sk is not None:
                give(sk)
            h = out
        z = [torch.empty(N, 5, ps, ps, dtype=F32, device=dev) for ps in self.patch_sizes]
        y = torch.empty(N, self.P, 5, dtype=F32, device=dev)
        plan = {"steps": steps, "z": z, "y": y}
        self._plans[N] = plan
        return plan

    # ------------------------------------------------------------------ forward
    def _forward_u8(self, frames: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        """uint8 codes (N,3,480,480) on the GPU -> the (N,4774,5) rows."""
        if not frames.is_cuda:
            raise FdetError("Int8SSD runs on the GPU only (no CPU fallback): move the input to cuda")
        if frames.dim() != 4 or tuple(frames.shape[1:]) != (3, self.size, self.size) or frames.dtype != torch.uint8:
            raise ValueError(f"expected uint8 input (N,3,{self.size},{self.size}), got {frames.dtype} {tuple(frames.shape)}")
        N = frames.shape[0]
        plan = self._plan(N)
        steps, y = plan["steps"], plan["y"]
        h0 = steps[0][0]
        with self._t("stem3_fwd_q8x", 240, 3, 16, 2.0 * N * 16 * 27 * 240 * 240, float(frames.numel()) + N * 16 * 240 * 240):
            hp.stem3_fwd_q8x_u8(frames.contiguous(), self.stem_wpk, self.stem_bias, self.stem_mul, h0)
        self.counters["stem_q8"] += 1
        if trace is not None:
            trace["stem"] = h0.nchw()
            trace["blocks"], trace["z"] = [], []
        for k, ((name, ci, co, pool, head), (h, a, sk, out), (c1, c2, cs, skip_mul)) in enumerate(zip(self.specs, steps, self.blocks)):
            hk = h.shape[2]
            px = float(N * hk * hk)
            if cs is not None:
                with self._t("q8x_pointwise", hk, ci, co, 2.0 * px * ci * co, px * (ci + co)):
                    hp.q8x_pointwise(h, cs.wpk, cs.bias, cs.mul, sk)
                self.counters["pointwise"] += 1
            with self._t("q8x_conv3x3", hk, ci, co, 2.0 * px * 9 * ci * co, px * (ci + co)):
                hp.q8x_conv3x3(h, c1.wpk, c1.bias, c1.mul, a, slope=self.slope)
            with self._t("q8x_conv3x3_pool" if pool else "q8x_conv3x3_skip", hk, co, co, 2.0 * px * 9 * co * co,
                         px * co * (2.0 + (0.25 if pool else 1.0))):
                hp.q8x_conv3x3(a, c2.wpk, c2.bias, c2.mul, out, skip=sk if cs is not None else h, skip_mul=skip_mul, pool=bool(pool),
                               slope=self.slope)
            self.counters["convs"] += 2
            if trace is not None:
                trace["blocks"].append(out.nchw())
            if head >= 0:
                _, hw, hb, hm = self.heads[k]
                z = plan["z"][head]
                ho = out.shape[2]
                with self._t("q8x_head", ho, co, 5, 2.0 * N * ho * ho * co * 5, float(N * ho * ho * (co + 40))):
                    hp.q8x_head_f32(out, hw, hb, hm, z)
                    hp.ssd_head_pack_fwd(z, self.patch_sizes[head], self.starts[head], y)
                self.counters["heads"] += 1
                if trace is not None:
                    trace["z"].append(z.clone())
        if trace is not None:
            trace["y"] = y
        return y

    def _forward_f32(self, x: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        """float images in [0,1] at the model resolution -> codes -> the integer stem."""
        if not x.is_cuda:
            raise FdetError("Int8SSD runs on the GPU only (no CPU fallback): move the input to cuda")
        if x.dim() == 3:
            x = x.unsqueeze(0)
        return self._forward_u8(self._codes(x), trace)

    def _forward_any(self, x: torch.Tensor, trace: Optional[dict] = None) -> torch.Tensor:
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.is_cuda and x.dtype == torch.uint8 and x.dim() == 4 and tuple(x.shape[1:]) == (3, self.size, self.size):
            return self._forward_u8(x, trace)
        if not x.is_cuda:
            raise FdetError("Int8SSD runs on the GPU only (no CPU fallback): move the input to cuda")
        return self._forward_f32(self._preprocess(x), trace)

    @torch.no_grad()
    def forward_frames(self, x: torch.Tensor) -> torch.Tensor:
        """frames (uint8 or float, values 0..255, any size) -> the (N,4774,5) rows [score, x, y, w, h] of SSD.forward."""
        return self._forward_any(x)

    @torch.no_grad()
    def __call__(self, x: torch.Tensor, predict: torch.Tensor = torch.tensor(0)):
        """SSD.forward: float images in [0,1] at the model resolution -> rows; predict=1: frames -> boxes per image."""
        if predict == 1:
            return self.non_max_suppression(self.forward_frames(x))
        return self._forward_f32(x)

    forward = __call__

    @torch.no_grad()
    def trace(self, frames: torch.Tensor) -> dict:
        """{"stem": int8 (N,16,240,240), "blocks": [int8 output of every block], "z": [fp32 (N,5,ps,ps) of every head before
        sigmoid and priors], "y": (N,4774,5)}"""
        out = {}
        self._forward_any(frames, trace=out)
        return out

    def non_max_suppression(self, x):
        from .models.BaseModel import split_rows
        if len(x.shape) == 3:
            return split_rows(*self.reduce_bounding_boxes.forward_batch(x))
        return self.reduce_bounding_boxes(x)

    def single_non_max_suppression(self, x):
        return self.reduce_bounding_boxes(x)


def quantize_ssd(model, frames_iter, **kw) -> Int8SSD:
    """calibrate_ssd + Int8SSD (what SSD.quantize does)."""
    _check_ssd(model, "quantize_ssd")
    if int(model.filters) != 16 or tuple(model.input_shape) != (3, 480, 480):
        raise ValueError(f"Int8SSD: filters=16 at 480x480 only, got filters={model.filters} at {tuple(model.input_shape)}: a wider "
                         "model exceeds the 256 channels of the int8 kernels")
    return Int8SSD(model, calibrate_ssd(model, frames_iter, **kw))


def quantize_model(model, frames_iter, stem: str = "float", **kw):
    """calibrate + the int8 class of the model: Int8PoolResnet, Int8Resnet or Int8SeparableCNN (what the models' `quantize`
    do).  `stem` is Int8PoolResnet's ("float" or "integer"); a Resnet and a SeparableCNN have their integer stem only and
    their calls leave `stem` alone."""
    from .models.Resnet import Resnet
    from .models.SeparableCNN import SeparableCNN
    if type(model) is SeparableCNN:
        if stem != "float":
            raise ValueError("quantize_model: stem= selects PoolResnet's stem; Int8SeparableCNN has its integer stem only")
        return Int8SeparableCNN(model, calibrate(model, frames_iter, **kw))
    if type(model) is Resnet:
        if stem != "float":
            raise ValueError("quantize_model: stem= selects PoolResnet's stem; Int8Resnet has its integer stem only")
        return Int8Resnet(model, calibrate(model, frames_iter, **kw))
    if stem not in Int8PoolResnet.STEMS:
        raise ValueError(f"quantize_model: stem must be one of {Int8PoolResnet.STEMS}, got {stem!r}")
    return Int8PoolResnet(model, calibrate(model, frames_iter, **kw), stem=stem)
