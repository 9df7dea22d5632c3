#!/usr/bin/env python3
"""precision16 vs bf16x3 on SSD(filters=16) at 480x480 (4774 priors): the reference's SSD recipe (train_model_ssd.py,
Trainer(precision=16), batch 24) and bench.py's config 4 (batch 64).  Prints ONE JSON line:

  * ms/step of the full training step (fwd + ssd_loss + bwd + Adam) at bs 24 and bs 64, in bf16x3 and in precision16 --
    both precisions on the same model in the same process, timed in alternating blocks after warm-up of both;
  * the SSDStack.timer per-launch table (HIP events, ms) of one step in each precision at bs 64;
  * the floors of bench.py's config-4 leg (3 x 14.36 GFLOP per image, dense bf16 MFMA peak), with one MFMA pass per
    product in precision16 and three in bf16x3.

    python tools/bench_p16_ssd.py [--rounds 4] [--steps 5] [--warmup 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# bench.py's constants (MI355X dense bf16 MFMA peak; SSD forward 14.36 GFLOP per image, backward twice that)
PEAK_BF16_MFMA_TFLOPS = 2500.0
GFLOP_PER_IMAGE_SSD = 3 * 14.36


def mfma_floor(gflop, passes, ms):
    t = passes * gflop / (PEAK_BF16_MFMA_TFLOPS * 1e3) * 1e3
    return {"algorithmic_gflop": round(gflop, 1), "mfma_floor_ms": round(t, 3), "frac_of_mfma_floor": round(t / ms, 4)}


def leg(B, rounds, steps, warm, timers):
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    from fdet_amd.convstack import KernelTimer
    from fdet_amd.datasets.synthetic import synthetic_boxes
    from fdet_amd.models.ModelMetaSSD import ModelMetaSSD
    from fdet_amd.models.SSD import SSD
    size = 480
    torch.manual_seed(0)
    model = SSD(filters=16, input_shape=(3, size, size)).cuda().train()
    mm = ModelMetaSSD(model=model, lr=1e-4)
    mm.configure_optimizers()
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(3)).cuda()
    y = hp.ssd_encode_targets(synthetic_boxes(B, size, seed=4), (size, size), device=x.device)
    eng = model.engine
    modes = ("bf16x3", "bf16")
    loss = {}
    for m in modes:                                        # warm-up of both precisions before anything is timed
        eng.set_precision(m)
        for _ in range(warm):
            loss[m] = mm.fused_train_step(x, y)[0]
    torch.cuda.synchronize()
    t = {m: [] for m in modes}
    for r in range(rounds):                                # alternating blocks (ABAB..., then BABA... next round)
        for m in (modes if r % 2 == 0 else modes[::-1]):
            eng.set_precision(m)
            mm.fused_train_step(x, y)                      # one untimed step after the switch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss[m] = mm.fused_train_step(x, y)[0]
            torch.cuda.synchronize()
            t[m].append((time.perf_counter() - t0) / steps * 1e3)
    out = {"batch": B}
    for m in modes:
        ms = sorted(t[m])[len(t[m]) // 2]
        key = "bf16x3" if m == "bf16x3" else "p16"
        out[key] = {"ms_per_step": round(ms, 3), "ms_blocks": [round(v, 3) for v in t[m]], "imgs_per_s": round(B / ms * 1e3, 1),
                    "finite_loss": bool(torch.isfinite(loss[m]).all()),
                    **mfma_floor(B * GFLOP_PER_IMAGE_SSD, 3.0 if m == "bf16x3" else 1.0, ms)}
    out["speedup_p16"] = round(out["bf16x3"]["ms_per_step"] / out["p16"]["ms_per_step"], 3)
    if timers:
        for m in modes:
            eng.set_precision(m)
            timer = KernelTimer()
            eng.timer = timer
            mm.fused_train_step(x, y)
            eng.timer = None
            per = timer.summary()
            key = "bf16x3" if m == "bf16x3" else "p16"
            out[key]["kernels_ms_per_step"] = {k: round(tot, 4) for k, (n_l, tot, fl, nb) in
                                               sorted(per.items(), key=lambda kv: -kv[1][1])}
            out[key]["kernels_sum_ms"] = round(sum(tot for (n_l, tot, fl, nb) in per.values()), 3)
    eng.set_precision("bf16x3")
    del model, mm, x, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    res = {"metric": "ssd_F16_p16_vs_bf16x3", "device": torch.cuda.get_device_name(0),
           "bs64": leg(64, a.rounds, a.steps, a.warmup, timers=True),
           "bs24": leg(24, a.rounds, 2 * a.steps, a.warmup, timers=False)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
