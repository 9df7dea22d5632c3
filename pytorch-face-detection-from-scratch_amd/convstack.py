"""Conv-stack engine: the PoolResnet / Resnet forward and hand-written backward as a fixed
sequence of HIP kernel launches (no autograd graph inside).

Reference: models/PoolResnet.py:11-105, models/Resnet.py:10-99 (forward); the backward is the
autograd of that forward, restated kernel by kernel:

    stem -> [ conv1+lrelu -> conv2+lrelu -> dropout2d*skip-add (-> maxpool) ] x blocks
         -> dropout2d(0.5) -> head conv -> sigmoid

Activations saved for backward per block: a (conv1 output), c (conv2 output, pre-dropout) and
the block input; everything else is recomputed in the fused tails.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch

from . import hotpath as hp
from . import ps as psm

F32 = torch.float32


@dataclass
class StackGeometry:
    kind: str
    filters: int
    in_ch: int
    H: int
    W: int
    S: int
    num_blocks: int
    stem_k: int
    stem_s: int
    stem_p: int
    head_k: int
    head_p: int
    pool_mult: int          # pool iff H > pool_mult*S  (PoolResnet.py:41: 2, Resnet.py:38: 1)
    strict_grid: bool = True   # False: the head's grid may differ from S (models/SeparableCNN.py fixes S = 16 and returns what comes)

    def levels(self):
        """[(H_in, pool)] per block and the stem output size."""
        h0 = (self.H + 2 * self.stem_p - self.stem_k) // self.stem_s + 1
        w0 = (self.W + 2 * self.stem_p - self.stem_k) // self.stem_s + 1
        if h0 != w0:
            raise ValueError("square inputs only (reference swaps width/height, datasets/utils.py:107)")
        out, h = [], h0
        for _ in range(self.num_blocks):
            pool = 2 if h > self.pool_mult * self.S else 1
            if pool == 2 and h % 2:
                raise ValueError(f"cannot 2x2-pool an odd {h}x{h} map")
            out.append((h, pool))
            h //= pool
        s_out = h + 2 * self.head_p - self.head_k + 1
        if s_out != self.S and self.strict_grid:
            # the reference only fails later, in yolo_loss, with a shape mismatch
            raise ValueError(f"input {self.H}x{self.W} with this stem/head reaches a {s_out}x{s_out} grid, "
                             f"not num_of_patches={self.S}")
        if s_out <= 0:
            raise ValueError(f"input {self.H}x{self.W} with this stem/head leaves no output grid")
        return h0, out


PARAM_ORDER_DOC = "conv1.{weight,bias}, residual_blocks.k.conv{1,2}.{weight,bias}, out.{weight,bias}"


class KernelTimer:
    """HIP-event timing of kernel classes on the stream they are launched on (torch's current
    stream).  Events are only recorded while a timer is attached to the engine; nothing
    synchronises until summary()."""

    def __init__(self):
        self.rec = {}          # name -> [list of (start, end)], flops/launch, bytes/launch

    def span(self, name, flops=0.0, nbytes=0.0):
        return _Span(self, name, flops, nbytes)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, (evs, flops, nbytes) in self.rec.items():
            out[name] = (len(evs), sum(a.elapsed_time(b) for a, b in evs), flops / len(evs), nbytes / len(evs))
        return out


class _Span:
    def __init__(self, timer, name, flops, nbytes):
        self.t, self.name, self.flops, self.nbytes = timer, name, flops, nbytes

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()

    def __exit__(self, *exc):
        self.b.record()
        rec = self.t.rec.setdefault(self.name, [[], 0.0, 0.0])
        rec[0].append((self.a, self.b))
        rec[1] += self.flops
        rec[2] += self.nbytes


class _NoSpan:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NOSPAN = _NoSpan()


class _PsScope(list):
    """PS buffers leased by one forward pass: [(pool key, PsTensor)]; they go back to the engine's pool when the scope
    is released explicitly or dropped (CPython: as soon as the saved state of the pass is)."""

    def __init__(self, pool):
        super().__init__()
        self.pool = pool

    def release(self):
        for key, t in self:
            self.pool.setdefault(key, []).append(t)
        self.clear()

    def __del__(self):
        self.release()


@dataclass(frozen=True)
class Stage:
    """`run` consecutive blocks from block `k` on, all at one resolution, that a pass runs as one unit."""
    kind: str             # "ps_pool": pooled block on PS; "ps_chain" / "chain": one-launch run (PS / fp32 I/O); "block": per layer
    k: int
    run: int
    hk: int
    pool: int
    strips: bool          # the PS maps of the level are column strips
    out_ps: bool          # hands its output on as a PS tensor (else fp32 NCHW)
    fused_pool: bool      # pooling inside the conv epilogues: routing bytes are saved, not c
    wgrad: str            # weight gradients: "ps" / "batched" (one launch per level, PS / fp32 operands) or "single" (per layer)
    closes_level: bool    # backward: the level's queued weight gradients go out and after_block fires for its blocks


@dataclass(frozen=True)
class PassPlan:
    """Every route decision of one forward + backward pass (ConvStack.plan)."""
    N: int
    p16: bool
    stem_ps: bool         # the stem writes the first block's PS input itself
    stem_x3: bool         # else: the bf16x3 stem forward
    stem_wgrad: tuple     # (x3, p16) of the stem weight gradient
    head_fused: bool      # head + loss + their gradients in one launch, where the caller gives targets
    stages: tuple


class _WgradQueue:
    """(x, dz, weight name) of one backward pass's convs awaiting their level's batched weight-gradient launch, by route."""

    def __init__(self, eng, N, p16, G, dev, after_block):
        self.eng, self.N, self.p16, self.G, self.dev, self.after_block = eng, N, p16, G, dev, after_block
        self.items = {"ps": [], "batched": []}
        self.blocks = []                                   # blocks whose gradients are enqueued once the level closes

    def add(self, route, x, dz, name):
        self.items[route].append((x, dz, name))

    def launch(self, hk):
        e, N, F_, G = self.eng, self.N, self.eng.geo.filters, self.G
        for route, items in self.items.items():
            for i0 in range(0, len(items), 16):            # weight gradients of same-resolution convs: 16 to a launch
                grp = items[i0:i0 + 16]
                ops = [p[0] for p in grp], [p[1] for p in grp], [G[p[2] + ".weight"] for p in grp], [G[p[2] + ".bias"] for p in grp]
                if route == "ps":
                    ws = e._workspace("wgrad_ps", psm.conv3x3_wgrad_ps_ws_bytes(len(grp), N, F_, hk, hk), self.dev)
                else:
                    ws = e._workspace("wgrad_batched", hp.conv3x3_wgrad_batched_ws_bytes(len(grp), N, F_, F_, hk, hk), self.dev)
                with e._t("conv3x3_wgrad", N, hk, e._conv_flops(N, hk) * len(grp), e._act_bytes(N, hk, 2) * len(grp)):
                    (psm.conv3x3_wgrad_ps_batched if route == "ps" else hp.conv3x3_wgrad_batched)(*ops, ws, p16=self.p16)
            items.clear()

    def close(self, hk):
        """The level is done: launch what is queued, then report its blocks (data-parallel bucket launch)."""
        self.launch(hk)
        if self.after_block is not None:
            for k in sorted(self.blocks):
                self.after_block(k)
        self.blocks.clear()


class ConvStack:
    """Owns packed weights, workspaces and saved activations; parameters are passed in as a
    dict of GPU tensors named like the reference's state_dict."""

    def __init__(self, geo: StackGeometry):
        self.geo = geo
        self.h0, self.lv = geo.levels()
        self._packed_key = None
        self._wpk: Dict[str, torch.Tensor] = {}
        self._ws: Dict[str, torch.Tensor] = {}
        self.slope = 0.2
        self.timer: Optional[KernelTimer] = None
        # conv arithmetic: "bf16x3" (bf16 hi/lo split on the bf16 matrix cores, fp32 accumulate,
        # ~1e-5 of fp32) where the channel count allows, else "f32" (exact fp32 MFMA chain).
        # FDET_PRECISION=f32 forces the exact path.
        import os
        want = os.environ.get("FDET_PRECISION", "bf16x3")
        self.x3 = (want in ("bf16x3", "bf16")) and hp.x3_supported(geo.filters, geo.filters)
        # pooled blocks: dropout*skip*maxpool (and its backward) inside the conv epilogues (FDET_POOL_FUSION=0: the
        # separate elementwise tail kernels of round 1)
        self.pool_fusion = self.x3 and os.environ.get("FDET_POOL_FUSION", "1") != "0"
        # pre-split (PS) activations for the pooled 64-channel blocks (ps.py, csrc/fdet_ps.h): stem output, conv outputs
        # and their gradients live as bf16 hi|lo units, staged by LDS-DMA (FDET_PS=0: the fp32-I/O kernels of round 2)
        self.ps = self.pool_fusion and geo.filters == 64 and os.environ.get("FDET_PS", "1") != "0"
        self._ps_pool: Dict[tuple, list] = {}
        self.ps_strips = self.ps and os.environ.get("FDET_PS_STRIPS", "1") != "0"
        # precision16 (FDET_PRECISION=bf16 or set_precision("bf16")): the conv kernels run ONE bf16 MFMA pass (bf16
        # activations and weights, fp32 accumulation / epilogues / master weights, every stored activation and activation
        # gradient rounded to bf16) -- the arithmetic of the reference's Trainer(precision=16), train_model.py:50, with bf16
        # as the 16-bit type.  Wherever the bf16x3 kernels run: the PS kernels (64 channels) and the fp32-I/O kernels (any
        # multiple of 16 channels, e.g. PoolResnet-large F=128).  The stem forward, the head, the pooled-gradient routing and
        # the fp32-I/O block chain (64 channels with FDET_PS=0) keep their fp32-grade kernels.
        self.p16 = self.x3 and want == "bf16"
        self._ps_pool_N = None                             # the batch size _ps_pool was filled for
        # runs of un-pooled blocks as one LDS-resident launch (FDET_CHAIN=0: the per-layer kernels)
        self.chain = self.x3 and os.environ.get("FDET_CHAIN", "1") != "0"
        self._plans: Dict[tuple, PassPlan] = {}
        # training head fused with the loss (fdet_head_loss_fused: forward + yolo_loss + their gradients in one kernel on
        # the matrix cores); FDET_HEAD_FUSED=0 keeps the separate head_fwd / yolo_loss / head_bwd launches
        self.head_fused = self.x3 and os.environ.get("FDET_HEAD_FUSED", "1") != "0"
        self._zero_ws: Dict[str, torch.Tensor] = {}

    def set_precision(self, name: str) -> None:
        """"bf16x3" (fp32-grade, default) or "bf16" (precision16: one MFMA pass; needs the bf16 matrix-core kernels).  A
        pass saved by forward(save=True) keeps the precision it ran in: backward() follows it, not this setting."""
        if name not in ("bf16x3", "bf16"):
            raise ValueError("precision must be 'bf16x3' or 'bf16'")
        if name == "bf16" and not self.x3:
            raise ValueError("precision16 needs the bf16 matrix-core conv kernels: this engine runs the exact-fp32 path "
                             f"(FDET_PRECISION=f32, or {self.geo.filters} channels is not a multiple of 16)")
        self.p16 = name == "bf16"
        self._ps_pool.clear()                              # a bf16x3 pass may have left lo planes in pooled buffers

    def u8_frames_ok(self) -> bool:
        """forward(..., u8_frames=True) is available: the PoolResnet stem writes the first block's PS input itself, so it can
        read the uint8 frames directly (x / 255 fused into its staging)."""
        g = self.geo
        return bool(self.ps and self.x3 and self.lv and 30 <= self.h0 <= 62 and self.lv[0][1] == 2 and g.W % 4 == 0 and
                    hp.stem_x3_supported(g.in_ch, g.W, g.stem_k, g.stem_s, g.stem_p) and g.filters == 64)

    def head_loss_fusable(self) -> bool:
        """The fused training head (forward + loss + backward of the head in one launch) covers this geometry."""
        g = self.geo
        hl = self.lv[-1][0] // self.lv[-1][1] if self.lv else self.h0
        return self.head_fused and hp.head_loss_fused_supported(g.filters, hl, hl, g.head_k, g.head_p)

    def _t(self, kind: str, N: int, h: int, flops: float = 0.0, nbytes: float = 0.0):
        if self.timer is None:
            return _NOSPAN
        return self.timer.span(f"{kind}@{h}x{h}", flops, nbytes)

    def _conv_flops(self, N: int, h: int) -> float:
        F_ = self.geo.filters
        return 2.0 * N * F_ * F_ * 9 * h * h

    def _act_bytes(self, N: int, h: int, tensors: float) -> float:
        """Algorithmic HBM bytes of `tensors` activation-sized fp32 tensors (SURVEY.md 8d:
        every input read once, every output written once; weights are L2-resident)."""
        return 4.0 * N * self.geo.filters * h * h * tensors

    # ------------------------------------------------------------------ weights
    def _ensure_packed(self, P: Dict[str, torch.Tensor], force: bool = False):
        key = (self.x3,) + tuple((P[k].data_ptr(), P[k]._version) for k in sorted(P) if k.endswith("weight"))
        if not force and key == self._packed_key:
            return
        F_ = self.geo.filters
        nf, nb = hp.packed_sizes(F_, F_)
        dev = P["conv1.weight"].device
        names = [f"residual_blocks.{k}.conv{j}" for k in range(self.geo.num_blocks) for j in (1, 2)]
        for name in names:
            if name + ".f" not in self._wpk:
                self._wpk[name + ".f"] = torch.empty(nf, dtype=F32, device=dev)
                self._wpk[name + ".b"] = torch.empty(nb, dtype=F32, device=dev)
        if self.x3:                                        # every layer in one launch
            hp.pack_conv3x3_weights_batched([P[nm + ".weight"] for nm in names], [self._wpk[nm + ".f"] for nm in names],
                                            [self._wpk[nm + ".b"] for nm in names])
        else:
            for name in names:
                hp.pack_conv3x3_weights(P[name + ".weight"], self._wpk[name + ".f"], self._wpk[name + ".b"], x3=False)
        self._packed_key = key

    def mark_params_dirty(self):
        """Call after the parameters were updated behind torch's back (fdet_adam_step)."""
        self._packed_key = None

    def _workspace(self, name: str, nbytes: int, dev) -> torch.Tensor:
        n = (nbytes + 3) // 4
        t = self._ws.get(name)
        if t is None or t.numel() < n or t.device != dev:
            t = torch.empty(max(n, 4), dtype=F32, device=dev)
            self._ws[name] = t
        return t

    # ------------------------------------------------------------------ plan
    def plan(self, N: int, p16: Optional[bool] = None) -> PassPlan:
        """Every route of a pass at batch size N in precision p16 (default: the engine's): a pure function of the geometry, the
        engine's switches, N and p16, and the only place that asks the library's routing queries.  forward() runs it and
        saves it, backward() runs the saved one, tests read it."""
        p16 = self.p16 if p16 is None else bool(p16)
        key = (N, p16, self.x3, self.pool_fusion, self.ps, self.ps_strips, self.chain, self.head_fused)
        if key not in self._plans:
            self._plans[key] = self._derive_plan(N, p16)
        return self._plans[key]

    def _derive_plan(self, N: int, p16: bool) -> PassPlan:
        g, F_, lv = self.geo, self.geo.filters, self.lv

        def fits32(hk):       # (the batch-dependent limit of run_ps: 32-bit byte offsets of the fp32 tensors the PS kernels touch)
            return N * F_ * hk * hk * 4 < 2 ** 31

        def wgrad_ps(hk):     # the PS weight gradient has a slab plan for this batch
            return psm.conv3x3_wgrad_ps_ws_bytes(1, N, F_, hk, hk) > 0

        def route(k):         # (kind, run) of the stage that starts at block k
            if k >= len(lv):
                return None, 0
            hk, pool = lv[k]
            # a pooled block runs on pre-split activations when its even map is 30..62 columns wide, or wider and kept as
            # column strips (csrc/fdet_ps.h; FDET_PS_STRIPS=0: the round-2 kernels for wide maps)
            if self.ps and pool == 2 and hk % 2 == 0 and hk >= 30 and fits32(hk) and \
                    ((self.ps_strips and psm.strips_of(hk)[0] > 1 and wgrad_ps(hk)) if hk > 62 else
                     hp.pool_fusion_supported(F_, F_, hk, hk, N)):
                return "ps_pool", 1
            # consecutive un-pooled blocks that can run as one LDS-resident chain (bf16x3, 64 channels, small maps), with
            # their per-block tensors in PS where the PS weight gradient takes them
            run = 0
            if self.chain and pool == 1 and hp.block_chain_supported(F_, hk, hk):
                run = 1
                while k + run < len(lv) and lv[k + run] == (hk, 1) and run < 16:
                    run += 1
            if run > 1:
                return ("ps_chain" if self.ps and wgrad_ps(hk) and fits32(hk) else "chain"), run
            return "block", 1

        stages, k = [], 0
        while k < len(lv):
            hk, pool = lv[k]
            kind, run = route(k)
            strips = kind == "ps_pool" and hk > 62
            # (a strip level hands its pooled output on as fp32 NCHW; the next level's converter writes its halos)
            out_ps = kind == "ps_pool" and not strips and route(k + 1)[0] in ("ps_pool", "ps_chain")
            fused = kind == "ps_pool" or (kind == "block" and pool == 2 and self.pool_fusion and
                                          hp.pool_fusion_supported(F_, F_, hk, hk, N))
            if kind == "block":
                wgrad = "batched" if self.x3 and hp.wgrad_x3_supported(N, F_, F_, hk, hk) else "single"
            else:
                wgrad = "batched" if kind == "chain" else "ps"
            # weight gradients of a run of same-resolution blocks go out in one launch, behind the level's first block
            closes = wgrad == "single" or not stages or stages[-1].hk != hk
            stages.append(Stage(kind, k, run, hk, pool, strips, out_ps, fused, wgrad, closes))
            k += run
        # the stem writes the first block's PS input itself: the PoolResnet stem (k10 s8 p2, plain layout) or the Resnet stem
        # (k3 s2 p1, column strips included)
        stem = (g.in_ch, g.W, g.stem_k, g.stem_s, g.stem_p)
        stem_k3 = (g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p)
        stem_ps = bool(stages) and stages[0].kind == "ps_pool" and self.x3 and \
            ((not stages[0].strips and hp.stem_x3_supported(*stem)) or hp.stem_k3_fwd_ps_supported(*stem_k3))
        # the stem weight gradient: the matrix-core kernel where one exists for the stem's shape, in precision16 where the
        # pass runs it and the PoolResnet stem's kernel has its one-pass form (48 < Wo <= 60)
        wg_x3 = self.x3 and ((g.W % 16 == 0 and hp.stem_x3_supported(*stem)) or hp.stem_k3_wgrad_x3_supported(*stem_k3))
        return PassPlan(N, p16, stem_ps, self.x3 and hp.stem_x3_supported(*stem), (wg_x3, p16 and wg_x3 and 48 < self.h0 <= 60),
                        self.head_loss_fusable(), tuple(stages))

    # ------------------------------------------------------------------ PS buffers
    def _ps_take(self, scope: "_PsScope", N: int, C: int, H: int, W: int, dev) -> "psm.PsTensor":
        """A zero-haloed PS buffer from the engine's pool; it returns to the pool when `scope` (kept alive by the saved
        state of a forward pass, or released at the end of an inference call) goes away.  Producers write real elements
        only, so a recycled buffer still has zero halos."""
        key = (N, C, H, W, str(dev))
        free = self._ps_pool.setdefault(key, [])
        t = free.pop() if free else psm.PsTensor(N, C, H, W, dev)
        scope.append((key, t))
        return t

    def _as_ps(self, t, r, hk: int) -> "psm.PsTensor":
        """`t` as a PS tensor of the pass `r`: an fp32 NCHW map (a level handed on in fp32, or a saved tensor that a caller
        replaced) is converted into a leased buffer."""
        if isinstance(t, psm.PsTensor):
            return t
        return psm.PsTensor.from_f32(t.to(F32).contiguous(), out=self._ps_take(r.scope, r.N, self.geo.filters, hk, hk, r.dev))

    @staticmethod
    def _names(st: Stage) -> List[str]:
        return [f"residual_blocks.{q}" for q in range(st.k, st.k + st.run)]

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, P: Dict[str, torch.Tensor], masks: Optional[Dict[str, torch.Tensor]] = None,
                save: bool = False, loss_targets: Optional[torch.Tensor] = None, G: Optional[Dict[str, torch.Tensor]] = None,
                u8_frames: bool = False):
        """x (N,C,H,W) f32 on the GPU -> y (N,5,S,S).  masks: per-(n,c) dropout scales
        {"residual_blocks.k": (N,F), "head": (N,F)} or None (eval).  save=True keeps what
        backward needs and returns it as the second value.
        loss_targets (N,5,S,S) + G (gradient views): the head runs FUSED with yolo_loss and its own backward
        (head_loss_fusable()): saved["loss"] = (loss_per_image, loss_sum), G["out.*"] are written, and backward() is
        called with dy=None."""
        g = self.geo
        if x.dim() != 4 or tuple(x.shape[1:]) != (g.in_ch, g.H, g.W):
            raise ValueError(f"expected input (N,{g.in_ch},{g.H},{g.W}), got {tuple(x.shape)}")
        if u8_frames:
            # inference on the uint8 frames themselves: x / 255 happens inside the stem (fdet_stem_fwd_ps_u8)
            if x.dtype != torch.uint8 or save or not self.u8_frames_ok():
                raise ValueError("u8_frames: uint8 input, inference only, PoolResnet stem on the pre-split path")
            x = x.contiguous()
        elif x.dtype != F32 or not x.is_contiguous():
            x = x.to(F32).contiguous()
        self._ensure_packed(P)
        N, F_, dev = x.shape[0], g.filters, x.device
        if N != self._ps_pool_N:
            # PS buffers are sized per batch: a pool filled for another N (a last partial batch, a validation batch) would
            # only pile up ~260 MB sets outside the caching allocator -- drop it
            self._ps_pool.clear()
            self._ps_pool_N = N
        plan = self.plan(N, self.p16)
        ws = self._workspace("stem", hp.stem_ws_bytes(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p), dev)
        if u8_frames and not plan.stem_ps:                 # (a batch too large for the pre-split path: the separate x / 255)
            x = hp.u8_to_f32_norm(x)
        scope = _PsScope(self._ps_pool)
        # r: the running state of the pass -- h / h_ps: the current activation as fp32 NCHW or PS (the other is None)
        r = SimpleNamespace(N=N, dev=dev, p16=plan.p16, P=P, masks=masks, scope=scope, h=None, h_ps=None, blocks=[] if save else None)
        stem_flops = 2.0 * N * F_ * g.in_ch * g.stem_k * g.stem_k * self.h0 * self.h0
        with self._t("stem_fwd", N, self.h0, stem_flops, 4.0 * N * (g.in_ch * g.H * g.W + F_ * self.h0 * self.h0)):
            if plan.stem_ps:
                r.h_ps = self._ps_take(scope, N, F_, self.h0, self.h0, dev)
                psm.stem_fwd_ps(x, P["conv1.weight"], P["conv1.bias"], r.h_ps, g.stem_k, g.stem_s, g.stem_p, p16=plan.p16)
            else:
                r.h = torch.empty(N, F_, self.h0, self.h0, dtype=F32, device=dev)
                hp.stem_fwd(x, P["conv1.weight"], P["conv1.bias"], r.h, ws, g.stem_k, g.stem_s, g.stem_p, x3=plan.stem_x3)
        for st in plan.stages:
            getattr(self, "_fwd_" + st.kind)(st, r)
        # (plan and precision are stamped into the saved state: backward() runs the pass its forward ran)
        saved = {"x": x, "blocks": r.blocks, "masks": masks, "ps_scope": scope, "p16": plan.p16, "plan": plan} if save else None
        h = r.h
        y = torch.empty(N, 5, g.S, g.S, dtype=F32, device=dev)
        if loss_targets is not None and save and G is not None and plan.head_fused:
            if tuple(loss_targets.shape) != tuple(y.shape):
                raise ValueError(f"loss targets {tuple(loss_targets.shape)} != head output {tuple(y.shape)}")
            tg = loss_targets if (loss_targets.dtype == F32 and loss_targets.is_contiguous()) else loss_targets.to(F32).contiguous()
            hl = h.shape[2]
            nb = hp.head_loss_fused_ws_bytes(N, F_, hl, hl, g.head_k, g.head_p)
            ws = self._zero_ws.get("head_fused")
            if ws is None or ws.numel() * 4 != ((nb + 3) // 4) * 4 or ws.device != dev:
                ws = self._zero_ws["head_fused"] = torch.zeros((nb + 3) // 4, dtype=F32, device=dev)   # ticket counter starts at zero
            lpi = torch.empty(N, dtype=F32, device=dev)
            lsum = torch.empty(1, dtype=F32, device=dev)
            dout = torch.empty_like(h)
            macs = N * F_ * g.head_k ** 2 * (2 * 5 * g.S ** 2 + 5 * hl * hl)          # forward + dW + dx
            with self._t("head_loss_fused", N, hl, 2.0 * macs, self._act_bytes(N, hl, 2)):
                hp.head_loss_fused(h, masks["head"] if masks is not None else None, P["out.weight"], P["out.bias"], tg, y, lpi, lsum,
                                   dout, G["out.weight"], G["out.bias"], ws, g.head_k, g.head_p)
            saved["loss"] = (lpi, lsum)
            saved["head_dout"] = dout
        else:
            with self._t("head_fwd", N, h.shape[2], 2.0 * N * 5 * F_ * g.head_k ** 2 * g.S ** 2, self._act_bytes(N, h.shape[2], 1)):
                hp.head_fwd(h, masks["head"] if masks is not None else None, P["out.weight"], P["out.bias"], y, g.head_k, g.head_p)
        if save:
            saved["h_last"] = h
            saved["y"] = y
        else:
            scope.release()                                # inference: every PS buffer of the pass is free again
        return y, saved

    def _fwd_ps_pool(self, st: Stage, r) -> None:
        """Pooled block on pre-split activations: conv1 -> a (PS); conv2 + tail -> pooled output (PS when the next stage
        takes PS, else fp32 NCHW) + channel-innermost routing bytes."""
        N, F_, hk, dev, P, save = r.N, self.geo.filters, st.hk, r.dev, r.P, r.blocks is not None
        name = f"residual_blocks.{st.k}"
        x_ps = r.h_ps if r.h_ps is not None else self._as_ps(r.h, r, hk)
        a_ps = self._ps_take(r.scope, N, F_, hk, hk, dev)
        with self._t("conv3x3_fwd", N, hk, self._conv_flops(N, hk), self._act_bytes(N, hk, 2)):
            psm.conv3x3_ps_fwd(x_ps, self._wpk[name + ".conv1.f"], P[name + ".conv1.bias"], a_ps, self.slope, p16=r.p16)
            psm.halo_exchange(a_ps, p16=r.p16)             # strips: conv2 (and the weight gradient) read a's edge columns
        out_ps = self._ps_take(r.scope, N, F_, hk // 2, hk // 2, dev) if st.out_ps else None
        out = None if st.out_ps else torch.empty(N, F_, hk // 2, hk // 2, dtype=F32, device=dev)
        route = psm.route8_like(N, F_, hk, hk, dev) if save else None
        with self._t("conv3x3_fwd_pool", N, hk, self._conv_flops(N, hk), self._act_bytes(N, hk, 2 + 0.25 + (1 / 16 if save else 0))):
            psm.conv3x3_ps_fwd_pool(a_ps, self._wpk[name + ".conv2.f"], P[name + ".conv2.bias"], x_ps,
                                    r.masks[name] if r.masks is not None else None, out_ps, out, route, self.slope, p16=r.p16)
        if save:
            r.blocks.append((x_ps, a_ps, route))
        r.h, r.h_ps = out, out_ps

    def _fwd_chain_args(self, st: Stage, r):
        names = self._names(st)
        return ([self._wpk[nm + ".conv1.f"] for nm in names], [r.P[nm + ".conv1.bias"] for nm in names],
                [self._wpk[nm + ".conv2.f"] for nm in names], [r.P[nm + ".conv2.bias"] for nm in names],
                [r.masks[nm] for nm in names] if r.masks is not None else None)

    def _fwd_ps_chain(self, st: Stage, r) -> None:
        """The blocks of the run keep their activation on the CU: one launch (fdet_block_chain_fwd_ps); what backward needs is
        kept in PS (a_k, block outputs: operands of the weight gradients; c_k: hi plane = its signs)."""
        N, F_, hk, run, dev, save = r.N, self.geo.filters, st.hk, st.run, r.dev, r.blocks is not None
        x_ps = r.h_ps if r.h_ps is not None else self._as_ps(r.h, r, hk)
        a_l, c_l, o_l = ([self._ps_take(r.scope, N, F_, hk, hk, dev) for _ in range(n)] if save else None for n in (run, run, run - 1))
        out = torch.empty(N, F_, hk, hk, dtype=F32, device=dev)
        with self._t("chain_fwd", N, hk, 2 * run * self._conv_flops(N, hk), self._act_bytes(N, hk, 1 + (2.5 * run if save else 1))):
            psm.block_chain_fwd_ps(x_ps, *self._fwd_chain_args(st, r), a_l, c_l, o_l, out, self.slope, p16=r.p16)
        if save:
            r.blocks.extend((x_ps if i == 0 else o_l[i - 1], a_l[i], c_l[i]) for i in range(run))
        r.h, r.h_ps = out, None

    def _fwd_chain(self, st: Stage, r) -> None:
        """The same with fp32 NCHW tensors (fdet_block_chain_fwd_bf16x3)."""
        N, F_, hk, run, dev, save = r.N, self.geo.filters, st.hk, st.run, r.dev, r.blocks is not None
        a_l, c_l = ([torch.empty(N, F_, hk, hk, dtype=F32, device=dev) for _ in range(run)] if save else None for _ in (1, 2))
        o_l = [torch.empty(N, F_, hk, hk, dtype=F32, device=dev) if (save or i == run - 1) else None for i in range(run)]
        with self._t("chain_fwd", N, hk, 2 * run * self._conv_flops(N, hk), self._act_bytes(N, hk, 1 + (3 * run if save else 1))):
            hp.block_chain_fwd(r.h, *self._fwd_chain_args(st, r), a_l, c_l, o_l, self.slope)
        if save:
            r.blocks.extend((r.h if i == 0 else o_l[i - 1], a_l[i], c_l[i]) for i in range(run))
        r.h = o_l[-1]

    def _fwd_block(self, st: Stage, r) -> None:
        """One block, layer by layer, on fp32 NCHW tensors: pooling fused into conv2, as a separate tail, or none."""
        N, F_, hk, pool, dev, P, save = r.N, self.geo.filters, st.hk, st.pool, r.dev, r.P, r.blocks is not None
        name, h, x3, p16 = f"residual_blocks.{st.k}", r.h, self.x3, r.p16
        sc = r.masks[name] if r.masks is not None else None
        fl, w2, b2 = self._conv_flops(N, hk), self._wpk[name + ".conv2.f"], P[name + ".conv2.bias"]
        a = torch.empty(N, F_, hk, hk, dtype=F32, device=dev)
        with self._t("conv3x3_fwd", N, hk, fl, self._act_bytes(N, hk, 2)):
            hp.conv3x3_fwd(h, self._wpk[name + ".conv1.f"], P[name + ".conv1.bias"], F_, y_full=a, slope=self.slope, x3=x3, p16=p16)
        out = torch.empty(N, F_, hk // pool, hk // pool, dtype=F32, device=dev)
        if st.fused_pool:
            # conv2 + lrelu + dropout*skip + maxpool in one kernel; c is never written, backward gets one
            # routing byte per pooling window instead
            c = torch.empty(N, F_, hk // 2, hk // 2, dtype=torch.uint8, device=dev) if save else None
            with self._t("conv3x3_fwd_pool", N, hk, fl, self._act_bytes(N, hk, 2 + 0.25 + (1 / 16 if save else 0))):
                hp.conv3x3_fwd_pool(a, w2, b2, h, sc, out, c, self.slope, p16=p16)
        elif pool == 2:
            c = torch.empty_like(a)
            with self._t("conv3x3_fwd", N, hk, fl, self._act_bytes(N, hk, 2)):
                hp.conv3x3_fwd(a, w2, b2, F_, y_full=c, slope=self.slope, x3=x3, p16=p16)
            with self._t("tail_fwd", N, hk, 0.0, self._act_bytes(N, hk, 2.25)):
                hp.block_tail_fwd(c, h, sc, out, 2)
        else:
            c = torch.empty_like(a) if save else None
            with self._t("conv3x3_fwd", N, hk, fl, self._act_bytes(N, hk, 4 if save else 3)):
                hp.conv3x3_fwd(a, w2, b2, F_, y_full=c, skip=h, drop_scale=sc, y_out=out, slope=self.slope, x3=x3, p16=p16)
        if save:
            r.blocks.append((h, a, c))
        r.h = out

    # ------------------------------------------------------------------ backward
    def backward(self, saved, dy: torch.Tensor, P: Dict[str, torch.Tensor], G: Dict[str, torch.Tensor],
                 after_block=None) -> None:
        """dy = d loss / d y (N,5,S,S).  Writes every parameter gradient into G[name]
        (overwrites; same names/shapes as P).  `after_block(k)` is called once block k's
        gradients have been enqueued (data-parallel bucket launch).  Runs the plan of the forward pass (saved["plan"]): its
        routes and its precision, whatever set_precision() said since."""
        g, F_, plan = self.geo, self.geo.filters, saved["plan"]
        x, masks = saved["x"], saved["masks"]
        N, dev = plan.N, x.device
        h_last, y = saved["h_last"], saved["y"]
        if saved.get("head_dout") is not None:
            dout = saved["head_dout"]                      # the fused head already ran its backward (G["out.*"] written)
        else:
            if dy is None or tuple(dy.shape) != tuple(y.shape):
                raise ValueError(f"dy shape {None if dy is None else tuple(dy.shape)} != y shape {tuple(y.shape)}")
            dy = dy.to(F32).contiguous()
            hl = h_last.shape[2]
            ws = self._workspace("head", hp.head_bwd_ws_bytes(N, F_, hl, hl, g.head_k, g.head_p), dev)
            dout = torch.empty_like(h_last)
            with self._t("head_bwd", N, hl, 4.0 * N * 5 * F_ * g.head_k ** 2 * g.S ** 2, self._act_bytes(N, hl, 2)):
                hp.head_bwd(h_last, masks["head"] if masks is not None else None, P["out.weight"], y, dy, dout,
                            G["out.weight"], G["out.bias"], ws, g.head_k, g.head_p)
        if saved.get("ps_scope") is None:
            saved["ps_scope"] = _PsScope(self._ps_pool)
        r = SimpleNamespace(N=N, dev=dev, p16=plan.p16, P=P, G=G, masks=masks, scope=saved["ps_scope"], blocks=saved["blocks"],
                            dout=dout, wq=_WgradQueue(self, N, plan.p16, G, dev, after_block))
        for st in reversed(plan.stages):
            getattr(self, "_bwd_" + st.kind)(st, r)
            r.wq.blocks.extend(range(st.k, st.k + st.run))
            if st.closes_level:
                r.wq.close(st.hk)
        ws = self._workspace("stem", hp.stem_ws_bytes(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p), dev)
        stem_flops = 2.0 * N * F_ * g.in_ch * g.stem_k * g.stem_k * self.h0 * self.h0
        with self._t("stem_wgrad", N, self.h0, stem_flops, 4.0 * N * (g.in_ch * g.H * g.W + F_ * self.h0 * self.h0)):
            hp.stem_wgrad(x, r.dout, G["conv1.weight"], G["conv1.bias"], ws, g.stem_k, g.stem_s, g.stem_p,
                          x3=plan.stem_wgrad[0], p16=plan.stem_wgrad[1])
        saved["ps_scope"].release()                        # the saved PS activations / gradients are dead: back to the pool
        saved["blocks"] = []

    def _bwd_ps_chain(self, st: Stage, r) -> None:
        """The run comes back through the backward chain (fdet_block_chain_bwd_ps)."""
        N, F_, hk, run, names = r.N, self.geo.filters, st.hk, st.run, self._names(st)
        x_l, a_l, c_l = ([self._as_ps(r.blocks[q][j], r, hk) for q in range(st.k, st.k + run)] for j in range(3))
        dz1_l = [self._ps_take(r.scope, N, F_, hk, hk, r.dev) for _ in names]
        dz2_l = [self._ps_take(r.scope, N, F_, hk, hk, r.dev) for _ in names]
        dx = torch.empty_like(r.dout)
        with self._t("chain_bwd", N, hk, 2 * run * self._conv_flops(N, hk), self._act_bytes(N, hk, 2 + 3 * run)):
            psm.block_chain_bwd_ps(r.dout, [self._wpk[nm + ".conv1.b"] for nm in names], [self._wpk[nm + ".conv2.b"] for nm in names],
                                   [r.masks[nm] for nm in names] if r.masks is not None else None, a_l, c_l, dz1_l, dz2_l, dx,
                                   self.slope, p16=r.p16)
        for i in reversed(range(run)):
            r.wq.add("ps", a_l[i], dz2_l[i], names[i] + ".conv2")
            r.wq.add("ps", x_l[i], dz1_l[i], names[i] + ".conv1")
        r.dout = dx

    def _bwd_chain(self, st: Stage, r) -> None:
        """The same with fp32 NCHW tensors (fdet_block_chain_bwd_bf16x3)."""
        N, hk, run, names = r.N, st.hk, st.run, self._names(st)
        x_l, a_l, c_l = ([r.blocks[q][j] for q in range(st.k, st.k + run)] for j in range(3))
        dz1_l = [torch.empty_like(a) for a in a_l]
        dz2_l = [torch.empty_like(a) for a in a_l]
        dx = torch.empty_like(r.dout)
        with self._t("chain_bwd", N, hk, 2 * run * self._conv_flops(N, hk), self._act_bytes(N, hk, 2 + 4 * run)):
            hp.block_chain_bwd(r.dout, [self._wpk[nm + ".conv1.b"] for nm in names], [self._wpk[nm + ".conv2.b"] for nm in names],
                               [r.masks[nm] for nm in names] if r.masks is not None else None, a_l, c_l, dz1_l, dz2_l, dx, self.slope)
        for i in reversed(range(run)):
            r.wq.add("batched", a_l[i], dz2_l[i], names[i] + ".conv2")
            r.wq.add("batched", x_l[i], dz1_l[i], names[i] + ".conv1")
        r.dout = dx

    def _bwd_ps_pool(self, st: Stage, r) -> None:
        """Pooled block on pre-split activations (a caller may have replaced saved tensors by fp32 / NCHW ones)."""
        N, F_, hk, dev, p16, dout = r.N, self.geo.filters, st.hk, r.dev, r.p16, r.dout
        name = f"residual_blocks.{st.k}"
        sc = r.masks[name] if r.masks is not None else None
        xin, a, c = r.blocks[st.k]
        xin, a = self._as_ps(xin, r, hk), self._as_ps(a, r, hk)
        if c.dim() == 4:                                   # routing bytes in NCHW -> channel-innermost
            if st.strips:
                raise ValueError("routing bytes of a strip level are per strip (ps.route8_shape)")
            c = c.view(N, F_ // 8, 8, hk // 2, hk // 2).permute(0, 1, 3, 4, 2).contiguous()
        fl = self._conv_flops(N, hk)

        def wgrad(x_, dz_, nm_, clean=False):
            # strips: the weight gradient wants ZERO halo slots in dz (a halo is not a position of its strip), the
            # data-gradient conv behind it the neighbour columns -- so each layer's weight gradient runs right
            # here, between the two halo passes, instead of in the level's batched launch (clean: the producer
            # cleared the halo slots itself)
            if st.strips and not clean:
                psm.halo_exchange(dz_, zero_only=True, p16=p16)
            r.wq.add("ps", x_, dz_, nm_)
            if st.strips:
                r.wq.launch(hk)
                psm.halo_exchange(dz_, p16=p16)
        dz2 = self._ps_take(r.scope, N, F_, hk, hk, dev)
        with self._t("pool_route_bwd", N, hk, 0.0, self._act_bytes(N, hk, 1 + 0.25 + 1 / 16)):
            psm.pool_route_bwd_ps(dout, c, sc, dz2, self.slope, p16=p16)
        if st.strips:
            wgrad(a, dz2, name + ".conv2", clean=True)     # fdet_pool_route_bwd_ps clears dz2's halo slots
        dz1 = self._ps_take(r.scope, N, F_, hk, hk, dev)
        with self._t("conv3x3_dgrad", N, hk, fl, self._act_bytes(N, hk, 3)):
            psm.conv3x3_ps_dgrad_act(dz2, self._wpk[name + ".conv2.b"], a, dz1, self.slope, p16=p16)
        if st.strips:
            wgrad(xin, dz1, name + ".conv1")
        dx = torch.empty(N, F_, hk, hk, dtype=F32, device=dev)
        with self._t("conv3x3_dgrad_unpool", N, hk, fl, self._act_bytes(N, hk, 2 + 0.25 + 1 / 16)):
            psm.conv3x3_ps_dgrad_unpool(dz1, self._wpk[name + ".conv1.b"], dout, c, dx, self.slope, p16=p16)
        if not st.strips:
            wgrad(a, dz2, name + ".conv2")
            wgrad(xin, dz1, name + ".conv1")
        r.dout = dx

    def _bwd_block(self, st: Stage, r) -> None:
        """One block, layer by layer, on fp32 NCHW tensors."""
        N, F_, hk, pool, p16, G, dout = r.N, self.geo.filters, st.hk, st.pool, r.p16, r.G, r.dout
        name, x3, batched = f"residual_blocks.{st.k}", self.x3, st.wgrad == "batched"
        sc = r.masks[name] if r.masks is not None else None
        xin, a, c = r.blocks[st.k]
        dz2 = torch.empty_like(a)
        de = torch.empty_like(a) if (pool == 2 and not st.fused_pool) else None
        if st.fused_pool:                                  # forward kept routing bytes instead of c
            with self._t("pool_route_bwd", N, hk, 0.0, self._act_bytes(N, hk, 1 + 0.25 + 1 / 16)):
                hp.pool_route_bwd(dout, c, sc, dz2, self.slope)
        else:
            with self._t("tail_bwd", N, hk, 0.0, self._act_bytes(N, hk, 4.25 if pool == 2 else 3)):
                hp.block_tail_bwd(dout, c, xin, sc, dz2, de, pool, self.slope)
        if pool == 1:
            de = dout
        fl = self._conv_flops(N, hk)
        if not batched:
            wws = self._workspace("wgrad", hp.conv3x3_wgrad_ws_bytes(N, F_, F_, hk, hk), r.dev)
            with self._t("conv3x3_wgrad", N, hk, fl, self._act_bytes(N, hk, 2)):
                hp.conv3x3_wgrad(a, dz2, G[name + ".conv2.weight"], G[name + ".conv2.bias"], wws)
        dz1 = torch.empty_like(a)
        with self._t("conv3x3_dgrad", N, hk, fl, self._act_bytes(N, hk, 3)):
            hp.conv3x3_dgrad(dz2, self._wpk[name + ".conv2.b"], F_, dz1, act=a, slope=self.slope, x3=x3, p16=p16)
        if not batched:
            with self._t("conv3x3_wgrad", N, hk, fl, self._act_bytes(N, hk, 2)):
                hp.conv3x3_wgrad(xin, dz1, G[name + ".conv1.weight"], G[name + ".conv1.bias"], wws)
        dx = torch.empty_like(a) if batched else dz2       # batched: dz2 stays alive until the level's launch
        if st.fused_pool:
            with self._t("conv3x3_dgrad_unpool", N, hk, fl, self._act_bytes(N, hk, 2 + 0.25 + 1 / 16)):
                hp.conv3x3_dgrad_unpool(dz1, self._wpk[name + ".conv1.b"], F_, dout, c, dx, self.slope, p16=p16)
        else:
            with self._t("conv3x3_dgrad", N, hk, fl, self._act_bytes(N, hk, 3)):
                hp.conv3x3_dgrad(dz1, self._wpk[name + ".conv1.b"], F_, dx, add=de, slope=self.slope, x3=x3, p16=p16)
        if batched:
            r.wq.add("batched", a, dz2, name + ".conv2")
            r.wq.add("batched", xin, dz1, name + ".conv1")
        r.dout = dx


def param_names(num_blocks: int) -> List[str]:
    """State-dict order of the reference modules (models/PoolResnet.py:70-89)."""
    names = ["conv1.weight", "conv1.bias"]
    for k in range(num_blocks):
        for j in (1, 2):
            names += [f"residual_blocks.{k}.conv{j}.weight", f"residual_blocks.{k}.conv{j}.bias"]
    names += ["out.weight", "out.bias"]
    return names


class ConvStackFn(torch.autograd.Function):
    """Autograd bridge: makes `loss.backward()` work on the model surface (Lightning-style
    callers).  Forward saves activations inside the engine-owned dict; backward returns one
    gradient per parameter."""

    @staticmethod
    def forward(ctx, engine: ConvStack, masks, names, x, *params):
        P = {n: p.detach() for n, p in zip(names, params)}
        y, saved = engine.forward(x.detach(), P, masks, save=True)
        ctx.engine, ctx.saved, ctx.names, ctx.P = engine, saved, names, P
        return y

    @staticmethod
    def backward(ctx, dy):
        G = {n: torch.empty_like(p) for n, p in ctx.P.items()}
        ctx.engine.backward(ctx.saved, dy, ctx.P, G)
        ctx.saved = None
        return (None, None, None, None) + tuple(G[n] for n in ctx.names)
