#!/usr/bin/env python3
"""The fused separable-block kernel (fdet_sepblock_fwd) against the composed forward it replaces, and SeparableCNN end to
end.  One process, warm-up, HIP events.  Prints ONE JSON line (and writes it to --out):

  * per level (60x60 pooled, 30x30 pooled, 15x15, 16x16) and F in {16, 32, 48, 64, 128} at bs 256, in eval and in training
    mode (dropout scales; the fused kernel also stores a, b and the routing bytes): ms of the fused kernel and of the
    composed launches (fdet_pointwise_fwd_bf16x3, fdet_mbt_dw_fwd, fdet_block_tail_fwd -- entries that predate the kernel --
    plus the elementwise fdet_sepblock_lrelu between the depthwise conv and the second GEMM, which no older entry
    offers), five repeats of `--iters` launches each: median, min-max spread, their ratio, and the fused kernel's
    achieved GB/s over its compulsory bytes (one read of x, one write of the output);
  * the whole eval forward and the whole training step (fused_train_step) in ms and img/s, per F.

    python tools/bench_sepcnn.py [--iters 20] [--batch 256] [--out profiles/r07_sepcnn.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, iters, repeats=5, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    out.sort()
    return {"ms": round(out[len(out) // 2], 4), "min": round(out[0], 4), "max": round(out[-1], 4),
            "spread": round((out[-1] - out[0]) / out[len(out) // 2], 4)}


def block_leg(F_, H, pool, B, iters, train=False):
    from fdet_amd import hotpath as hp, sepstack as ss
    gen = torch.Generator().manual_seed(F_ + H)
    x = torch.randn(B, F_, H, H, generator=gen).cuda()
    w1 = (torch.randn(F_, F_, 1, 1, generator=gen) / F_ ** 0.5).cuda()
    w2 = (torch.randn(F_, F_, 1, 1, generator=gen) / F_ ** 0.5).cuda()
    wd = (torch.randn(F_, 1, 3, 3, generator=gen) / 3).cuda()
    p1, p2 = hp.pointwise_pack(w1)[0], hp.pointwise_pack(w2)[0]
    out = torch.empty(B, F_, H // pool, H // pool, device="cuda")
    a, b, c = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    sc = ((torch.rand(B, F_, generator=gen) >= 0.25).float() / 0.75).cuda() if train else None
    route = torch.empty(B, F_, H // 2, H // 2, dtype=torch.uint8, device="cuda") if (train and pool == 2) else None

    def fused():
        if train:
            ss.sepblock_fwd(x, p1, wd, p2, sc, out, a, b, route, pool)
        else:
            ss.sepblock_fwd(x, p1, wd, p2, None, out, None, None, None, pool)

    def composed():
        hp.pointwise_fwd(x, p1, None, a, slope=0.2)
        ss.dw_fwd(a, wd, b)
        ss.lrelu_(b, 0.2)
        hp.pointwise_fwd(b, p2, None, c, slope=1.0)
        hp.block_tail_fwd(c, x, sc, out, pool)

    fu, co = timed(fused, iters), timed(composed, iters)
    nbytes = 4.0 * B * F_ * H * H * (1 + 1.0 / (pool * pool))
    spread = max(0.03, fu["spread"], co["spread"])
    ratio = co["ms"] / fu["ms"]
    return {"F": F_, "H": H, "pool": pool, "batch": B, "mode": "train" if train else "eval", "plan": ss.sepblock_plan(F_, H, H, pool), "fused": fu, "composed": co,
            "composed_over_fused": round(ratio, 3), "spread": round(spread, 4), "fused_faster": bool(ratio > 1 + spread),
            "fused_gbs_compulsory": round(nbytes / fu["ms"] / 1e6, 1)}


def model_leg(F_, B, iters):
    from fdet_amd import hotpath as hp
    from fdet_amd.datasets.synthetic import synthetic_boxes
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.SeparableCNN import SeparableCNN
    torch.manual_seed(0)
    model = SeparableCNN(filters=F_, input_shape=(3, 480, 480), output_padding=3).cuda()
    x = torch.rand(B, 3, 480, 480, generator=torch.Generator().manual_seed(3)).cuda()
    y = hp.encode_targets(synthetic_boxes(B, 480, seed=4), (480, 480), 16, device=x.device)
    model.eval()

    def ev():
        with torch.no_grad():
            model(x)
    e = timed(ev, iters)
    model.train()
    mm = ModelMeta(model=model, lr=1e-4)
    mm.configure_optimizers()
    t = timed(lambda: mm.fused_train_step(x, y), max(2, iters // 4))
    res = {"F": F_, "batch": B, "eval_forward": {**e, "img_per_s": round(B / e["ms"] * 1e3, 1)},
           "train_step": {**t, "img_per_s": round(B / t["ms"] * 1e3, 1)}, "paths": dict(model.engine.counters)}
    del model, mm, x, y
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    import fdet_amd  # noqa: F401
    res = {"metric": "separablecnn_fused_block", "device": torch.cuda.get_device_name(0),
           "blocks": [block_leg(F_, H, pool, a.batch, a.iters, train) for F_ in (16, 32, 48, 64, 128)
                      for H, pool in ((60, 2), (30, 2), (15, 1), (16, 1)) for train in (False, True)]}
    if not a.blocks_only:
        res["models"] = [model_leg(F_, a.batch, a.iters) for F_ in (64, 128)]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
