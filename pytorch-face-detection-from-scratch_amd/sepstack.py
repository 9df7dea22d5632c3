"""Separable-stack engine: the SeparableCNN forward and hand-written backward as a fixed sequence of HIP launches
(reference: models/SeparableCNN.py:10-112; the backward is the autograd of that forward, restated launch by launch):

    stem -> [ pw1 -> lrelu -> dw3x3 -> lrelu -> pw2 -> dropout2d -> + skip (-> maxpool) ] x blocks
         -> dropout2d(0.5) -> head conv -> sigmoid

The stem and the head are the conv stack's (fp32 NCHW entries).  A block runs as ONE kernel (fdet_sepblock_fwd,
"fused") or as the launches it replaces (fdet_pointwise_fwd_bf16x3, fdet_mbt_dw_fwd, fdet_sepblock_lrelu,
fdet_block_tail_fwd: "composed").  By default a level takes the fused kernel where it was measured faster -- maps that fit
one workgroup whole -- and the composed launches elsewhere; FDET_SEP=0 forces the composed forward, FDET_SEP=1
the fused kernel wherever it has a tiling.  `counters` says which one ran.

Saved for backward per block: the block input x, a = lrelu(pw1 x), b = lrelu(dw a), and either the routing bytes of the
pooled maximum (fused, pooled) or c = pw2 b (composed).  Nothing else is needed: no activation follows pw2, so
d c = unpool(d out) * drop_scale, and lrelu' of both activations is read off the sign of the saved post-activation values.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional

import torch

from . import hotpath as hp
from ._native import FdetError, check, lib, ptr, stream
from .convstack import KernelTimer, StackGeometry, _NOSPAN

F32 = torch.float32


# (filters, training) for which the fused kernel on a whole-map tile (15x15, 16x16) was measured faster than the composed
# launches by more than the run-to-run spread (tools/bench_sepcnn.py at bs 256, profiles/r07_sepcnn.json)
FUSED_MEASURED_FASTER = frozenset({(64, False)})


def sepblock_plan(F_: int, H: int, W: int, pool: int):
    """(rows, columns, bands, column segments, LDS bytes, haloed positions) of the fused kernel's tile, or None."""
    out = (ctypes.c_int * 6)()
    ok = lib().fdet_sepblock_plan(int(F_), int(H), int(W), int(pool), out, 6)
    return tuple(out) if ok else None


def sepblock_fwd(x, w1_pk, wd, w2_pk, drop_scale, out, a_save=None, b_save=None, route=None, pool: int = 1,
                 slope: float = 0.2) -> None:
    """The fused block (fdet_sepblock_fwd).  Raises FdetError for shapes it has no tiling for."""
    N, F_, H, W = x.shape
    if tuple(out.shape) != (N, F_, H // pool, W // pool) or tuple(wd.shape) != (F_, 1, 3, 3):
        raise ValueError("sepblock_fwd: shapes disagree")
    for t in (a_save, b_save):
        if t is not None and tuple(t.shape) != tuple(x.shape):
            raise ValueError("sepblock_fwd: a_save / b_save must have x's shape")
    if route is not None and tuple(route.shape) != (N, F_, H // 2, W // 2):
        raise ValueError("sepblock_fwd: route shape")
    if drop_scale is not None and tuple(drop_scale.shape) != (N, F_):
        raise ValueError("sepblock_fwd: drop_scale shape")
    check(lib().fdet_sepblock_fwd(ptr(x), ptr(w1_pk), ptr(wd), ptr(w2_pk), ptr(drop_scale), ptr(out), ptr(a_save), ptr(b_save),
                                  ptr(route, torch.uint8), N, F_, H, W, int(pool), float(slope), stream()), "fdet_sepblock_fwd")


def gate_bwd(g, act, drop_scale, out, slope: float = 0.2) -> None:
    """out = g * drop_scale[n,c] * lrelu'(act) (either factor optional; out may be g)."""
    N, F_ = g.shape[0], g.shape[1]
    P = g.numel() // (N * F_)
    if out.shape != g.shape or (act is not None and act.shape != g.shape):
        raise ValueError("gate_bwd: shapes disagree")
    check(lib().fdet_sepblock_gate_bwd(ptr(g), ptr(act), ptr(drop_scale), ptr(out), N, F_, P, float(slope), stream()),
          "fdet_sepblock_gate_bwd")


def lrelu_(z, slope: float = 0.2) -> None:
    check(lib().fdet_sepblock_lrelu(ptr(z), ptr(z), z.numel(), float(slope), stream()), "fdet_sepblock_lrelu")


def dw_fwd(x, w, z) -> None:
    N, C, H, W = x.shape
    check(lib().fdet_mbt_dw_fwd(ptr(x), ptr(w), ptr(z), N, C, H, W, 3, 1, stream()), "fdet_mbt_dw_fwd")


def dw_bwd(x, dz, w, dx, dW, ws) -> None:
    N, C, H, W = x.shape
    check(lib().fdet_mbt_dw_bwd(ptr(x), ptr(dz), ptr(w), ptr(dx), ptr(dW), ptr(ws), ws.numel() * 4, N, C, H, W, 3, 1, stream()),
          "fdet_mbt_dw_bwd")


def param_names(num_blocks: int):
    """State-dict order of the reference modules (models/SeparableCNN.py:77-96)."""
    names = ["conv1.weight", "conv1.bias"]
    for k in range(num_blocks):
        names += [f"residual_blocks.{k}.{c}.weight" for c in ("pointwise_conv1", "depthwise_conv", "pointwise_conv2")]
    return names + ["out.weight", "out.bias"]


class SepStack:
    """Owns packed weights and workspaces; parameters come in as a dict of GPU tensors named like the state dict.

    Inference runs any multiple of 8 filters from 8 up.  Training needs a multiple of 16 (or 8): the head's backward
    (fdet_head_bwd) works in groups of 16 channels; `forward(save=True)` refuses other widths before anything runs."""

    def __init__(self, geo: StackGeometry):
        if geo.filters < 8 or geo.filters % 8:
            raise FdetError(f"SeparableCNN needs a multiple of 8 filters (>= 8), got {geo.filters}")
        self.geo = geo
        self.h0, self.lv = geo.levels()
        hl = self.lv[-1][0] // self.lv[-1][1] if self.lv else self.h0
        self.s_out = hl + 2 * geo.head_p - geo.head_k + 1          # the head's grid; may differ from num_of_patches (reference quirk)
        self.slope = 0.2
        self.timer: Optional[KernelTimer] = None
        self.fused = os.environ.get("FDET_SEP", "auto")     # "0" composed, "1" fused wherever it has a tiling, else measured dispatch
        self.counters = {"fused": 0, "composed": 0}
        self.p16 = False
        self._packed_key = None
        self._wpk: Dict[str, tuple] = {}
        self._ws: Dict[str, torch.Tensor] = {}

    # ------------------------------------------------------------------ surface shared with ConvStack
    def set_precision(self, name: str) -> None:
        if name == "bf16x3":
            return
        raise FdetError("SeparableCNN runs in bf16x3 (fp32-grade) arithmetic only: precision16 is not built for the separable block")

    def u8_frames_ok(self) -> bool:
        return False

    def head_loss_fusable(self) -> bool:
        return False

    def mark_params_dirty(self):
        self._packed_key = None

    def _t(self, kind: str, h: int):
        return _NOSPAN if self.timer is None else self.timer.span(f"{kind}@{h}x{h}")

    def _workspace(self, name: str, nbytes: int, dev) -> torch.Tensor:
        n = (nbytes + 3) // 4
        t = self._ws.get(name)
        if t is None or t.numel() < n or t.device != dev:
            t = self._ws[name] = torch.empty(max(n, 4), dtype=F32, device=dev)
        return t

    def _ensure_packed(self, P):
        key = tuple((P[k].data_ptr(), P[k]._version) for k in sorted(P) if "pointwise" in k)
        if key == self._packed_key:
            return
        for k in range(self.geo.num_blocks):
            for c in ("pointwise_conv1", "pointwise_conv2"):
                nm = f"residual_blocks.{k}.{c}"
                self._wpk[nm] = hp.pointwise_pack(P[nm + ".weight"])
        self._packed_key = key

    def fused_ok(self, hk: int, pool: int, train: bool = False) -> bool:
        """The fused kernel runs this level.  Default: only the (F, mode) pairs of FUSED_MEASURED_FASTER, and there only
        where one workgroup holds the whole map; every other shape, measured slower or not measured, takes the composed
        launches."""
        if self.fused == "0":
            return False
        plan = sepblock_plan(self.geo.filters, hk, hk, pool)
        if plan is None:
            return False
        if self.fused == "1":
            return True
        return plan[2] * plan[3] == 1 and (self.geo.filters, bool(train)) in FUSED_MEASURED_FASTER

    # ------------------------------------------------------------------ forward
    def block_forward(self, k: int, h, P, sc, save: bool):
        """One residual block: -> (out, saved tuple or None)."""
        hk, pool = self.lv[k]
        N, F_, dev = h.shape[0], self.geo.filters, h.device
        nm = f"residual_blocks.{k}"
        w1f, w2f = self._wpk[nm + ".pointwise_conv1"][0], self._wpk[nm + ".pointwise_conv2"][0]
        wd = P[nm + ".depthwise_conv.weight"]
        out = torch.empty(N, F_, hk // pool, hk // pool, dtype=F32, device=dev)
        if self.fused_ok(hk, pool, save):
            a = torch.empty_like(h) if save else None
            b = torch.empty_like(h) if save else None
            route = torch.empty(N, F_, hk // 2, hk // 2, dtype=torch.uint8, device=dev) if (save and pool == 2) else None
            with self._t("sepblock_fused", hk):
                sepblock_fwd(h, w1f, wd, w2f, sc, out, a, b, route, pool, self.slope)
            self.counters["fused"] += 1
            return out, ((h, a, b, route) if save else None)
        a = torch.empty_like(h)
        b = torch.empty_like(h)
        c = torch.empty_like(h)
        with self._t("sepblock_composed", hk):
            hp.pointwise_fwd(h, w1f, None, a, slope=self.slope)
            dw_fwd(a, wd, b)
            lrelu_(b, self.slope)
            hp.pointwise_fwd(b, w2f, None, c, slope=1.0)
            hp.block_tail_fwd(c, h, sc, out, pool)
        self.counters["composed"] += 1
        return out, ((h, a, b, c) if save else None)

    def forward(self, x, P, masks=None, save: bool = False, loss_targets=None, G=None, u8_frames: bool = False):
        """x (N,C,H,W) f32 on the GPU -> y (N,5,s_out,s_out); masks as ConvStack.forward."""
        g = self.geo
        if u8_frames:
            raise FdetError("SeparableCNN has no uint8 stem: frames are normalised by the preprocessing kernel")
        if x.dim() != 4 or tuple(x.shape[1:]) != (g.in_ch, g.H, g.W):
            raise ValueError(f"expected input (N,{g.in_ch},{g.H},{g.W}), got {tuple(x.shape)}")
        if save and g.filters > 16 and g.filters % 16:
            raise FdetError(f"SeparableCNN trains with 8 or a multiple of 16 filters (the head's backward), got {g.filters}; "
                            "inference runs any multiple of 8")
        if x.dtype != F32 or not x.is_contiguous():
            x = x.to(F32).contiguous()
        self._ensure_packed(P)
        N, F_, dev = x.shape[0], g.filters, x.device
        ws = self._workspace("stem", hp.stem_ws_bytes(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p), dev)
        h = torch.empty(N, F_, self.h0, self.h0, dtype=F32, device=dev)
        with self._t("stem_fwd", self.h0):
            hp.stem_fwd(x, P["conv1.weight"], P["conv1.bias"], h, ws, g.stem_k, g.stem_s, g.stem_p, x3=False)
        saved = {"x": x, "blocks": [], "masks": masks} if save else None
        for k in range(len(self.lv)):
            sc = masks[f"residual_blocks.{k}"] if masks is not None else None
            h, sv = self.block_forward(k, h, P, sc, save)
            if save:
                saved["blocks"].append(sv)
        y = torch.empty(N, 5, self.s_out, self.s_out, dtype=F32, device=dev)
        with self._t("head_fwd", h.shape[2]):
            hp.head_fwd(h, masks["head"] if masks is not None else None, P["out.weight"], P["out.bias"], y, g.head_k, g.head_p)
        if save:
            saved["h_last"], saved["y"] = h, y
        return y, saved

    # ------------------------------------------------------------------ backward
    def backward(self, saved, dy, P, G, after_block=None) -> None:
        """dy = d loss / d y.  Writes every parameter gradient into G[name] (overwrites)."""
        if after_block is not None:
            raise FdetError("data-parallel training is not built for SeparableCNN (the gradient buckets follow the conv stack's layout)")
        g = self.geo
        F_ = g.filters
        x, masks = saved["x"], saved["masks"]
        N, dev = x.shape[0], x.device
        h_last, y = saved["h_last"], saved["y"]
        if dy is None or tuple(dy.shape) != tuple(y.shape):
            raise ValueError(f"dy shape {None if dy is None else tuple(dy.shape)} != y shape {tuple(y.shape)}")
        dy = dy.to(F32).contiguous()
        hl = h_last.shape[2]
        ws = self._workspace("head", hp.head_bwd_ws_bytes(N, F_, hl, hl, g.head_k, g.head_p), dev)
        dout = torch.empty_like(h_last)
        with self._t("head_bwd", hl):
            hp.head_bwd(h_last, masks["head"] if masks is not None else None, P["out.weight"], y, dy, dout,
                        G["out.weight"], G["out.bias"], ws, g.head_k, g.head_p)
        taps = self._workspace("dw_taps", int(lib().fdet_mbt_taps_ws_bytes(F_, 3)), dev)
        for k in reversed(range(g.num_blocks)):
            hk, pool = self.lv[k]
            nm = f"residual_blocks.{k}"
            xin, a, b, last = saved["blocks"][k]
            sc = masks[nm] if masks is not None else None
            w1b, w2b = self._wpk[nm + ".pointwise_conv1"][1], self._wpk[nm + ".pointwise_conv2"][1]
            with self._t("sepblock_bwd", hk):
                # d c = unpool(d out) * scale, d e = unpool(d out) (the skip's share)
                dc = torch.empty_like(a)
                if last is not None and last.dtype == torch.uint8:
                    de = torch.empty_like(a)
                    hp.pool_route_bwd(dout, last, sc, dc, self.slope)       # bits 0-3 of the bytes are set: no lrelu' factor
                    hp.pool_route_bwd(dout, last, None, de, self.slope)
                elif pool == 2:
                    de = torch.empty_like(a)
                    hp.block_tail_bwd(dout, last, xin, sc, dc, de, 2, 1.0)  # slope 1: no activation follows pw2
                else:
                    de = dout
                    gate_bwd(dout, None, sc, dc, self.slope)
                hp.pointwise_wgrad(b, dc, G[nm + ".pointwise_conv2.weight"])
                db = torch.empty_like(a)
                hp.pointwise_dgrad(dc, w2b, db)
                gate_bwd(db, b, None, db, self.slope)                       # through lrelu #2: d (dw a)
                da = dc                                                     # (dc is dead: reuse it)
                dw_bwd(a, db, P[nm + ".depthwise_conv.weight"], da, G[nm + ".depthwise_conv.weight"], taps)
                gate_bwd(da, a, None, da, self.slope)                       # through lrelu #1: d (pw1 x)
                hp.pointwise_wgrad(xin, da, G[nm + ".pointwise_conv1.weight"])
                dx = torch.empty_like(a)
                hp.pointwise_dgrad(da, w1b, dx, add=de)
            dout = dx
            if after_block is not None:
                after_block(k)
        ws = self._workspace("stem", hp.stem_ws_bytes(N, g.in_ch, F_, g.H, g.W, g.stem_k, g.stem_s, g.stem_p), dev)
        with self._t("stem_wgrad", self.h0):
            hp.stem_wgrad(x, dout, G["conv1.weight"], G["conv1.bias"], ws, g.stem_k, g.stem_s, g.stem_p, x3=False)
        saved["blocks"] = []
