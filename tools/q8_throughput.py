"""Inference throughput of the int8 post-training-quantised PoolResnet beside the two float modes, and with
`--model resnet` of the int8 Resnet (see `main_resnet` below).

    python tools/q8_throughput.py [--images 256] [--launches 100] [--calls 10] [--out profiles/r15_q8_chain.json]
    python tools/q8_throughput.py --model resnet [--images 32] [--out profiles/r17_q8_resnet.json]
    python tools/q8_throughput.py --model separablecnn [--out profiles/r19_q8_sep.json]      (`main_separablecnn`)
    python tools/q8_throughput.py --model ssd [--images 64] [--out profiles/r20_q8_ssd.json]  (`main_ssd`)

Workload: the inference leg's -- --images uint8 480x480 frames on the device (the three stored frames of
tests/golden/g6_trained_small.npz, repeated) through the medium PoolResnet (64 filters, the trained weights of
tests/golden/g16_trained_medium.npz) to boxes: `reduce_bounding_boxes.forward_batch(model.forward_frames(frames))`.
Seven models in ONE process, every one warmed up, alternated sample by sample; a sample is --calls back-to-back calls between
two device events, reported per call; median / min / max, the 5th / 95th percentile and their distance (`spread_ms`) over
--launches samples:

  bf16x3            the default engine (three bf16 MFMA passes)
  precision16       engine.set_precision("bf16") (one bf16 pass)
  int8-layers       quantize.Int8PoolResnet, calibrated (abs-max) on the first 16 frames, FDET_Q8_CHAIN=0 FDET_Q8_STEM=0: the
                    float stem, a quantise launch, twenty conv launches, a dequantise launch (the baseline of the two below)
  int8-chain        the sixteen 15x15 convs and the dequantise as one fdet_q8_chain launch
  int8-chain+stem   and the quantising stem on the uint8 frames (fdet_stem_fwd_q8_u8)
  int8              the model as constructed with no switch set (the measured defaults)
  int8-integer-stem Int8PoolResnet(stem="integer"): the integer uint8-frame stem (fdet_stem10_fwd_q8_u8) in front of the same
                    trunk; compared with `int8` of the same run (`faster.integer_stem`)

Then, in a second phase with a KernelTimer attached (device events around every kernel class, so launch gaps inside a class
count as its time), the per-kernel times of the three int8 modes and of precision16, and from them per class: the 15x15 tail
(sixteen launches plus dequantise against the chain), the stem (stem plus quantise against the quantising stem; the `/ 255`
pass that the float stem needs before it is counted in the end-to-end times only) and the 20-conv trunk.  `*_floor_share` is
a class's MACs over the dense int8 MFMA peak (2 x the 2.5 PF bf16 peak = 2.5e15 MAC/s) over its measured time.  `faster` says
for each new path whether it beat what it replaces by more than the larger of the two spreads: the rule of its default
(quantize.CHAIN_MEASURED_FASTER / STEM_Q8_MEASURED_FASTER).  `stem_alone` times the integer stem on its own beside the
quantising float stem, the float stem + quantise pair and a plain device copy of the integer stem's bytes (frames read + int8
output written).  Prints one JSON line and, with --out, writes it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INT8_PEAK_MACS = 2.5e15


def _stats(v):
    import numpy as np
    a = np.sort(np.asarray(v))
    p05, p95 = float(np.percentile(a, 5)), float(np.percentile(a, 95))
    return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4),
            "p05_ms": round(p05, 4), "p95_ms": round(p95, 4), "spread_ms": round(p95 - p05, 4)}


def _alternate(fns, launches, calls):
    """{name: callable} -> {name: [ms per call]}: samples alternated between the callables, `calls` back-to-back calls between
    two device events per sample."""
    import torch
    ms = {k: [] for k in fns}
    for _ in range(launches):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / calls)
    return ms


def main_resnet(args):
    """`--model resnet`: --images uint8 480x480 frames (the three stored frames, repeated) through the medium Resnet (64
    filters, ten blocks, S = 15; the trained weights of tests/golden/g22_trained_resnet_medium*.npz) to boxes, for bf16x3,
    precision16 and quantize.Int8Resnet (calibrated, abs-max, on the first 16 frames) -- the protocol above: one process, every
    model warmed up, alternated sample by sample, --calls back-to-back calls per sample, median and 5th / 95th percentile.  The
    default is 32 frames, the batch the float Resnet engine is run and tested at (config 3).  Then the per-kernel-class table of
    the int8 model and of precision16 (stem, each level, tail, head), and the integer stem on its own beside the launches it
    stands in for -- the float 3x3 / stride 2 stem on the normalised fp32 images followed by fdet_q8_quantize at 240 x 240 (the
    `/ 255` pass before them is not counted) -- and beside a plain device copy that moves the stem's bytes (frames read + int8
    output written)."""
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    from fdet_amd.convstack import KernelTimer
    from fdet_amd.models.Resnet import Resnet
    from fdet_amd.quantize import Int8Resnet, calibrate
    if not torch.cuda.is_available():
        raise SystemExit("q8_throughput needs a GPU")
    gold = os.path.join(ROOT, "tests", "golden")
    P = {}
    for part in ("", "_b", "_c", "_d"):
        g = np.load(os.path.join(gold, f"g22_trained_resnet_medium{part}.npz"))
        P.update({k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    images = torch.from_numpy(np.load(os.path.join(gold, "g6_trained_small.npz"))["images"])
    n = args.images
    frames = images[torch.arange(n) % images.shape[0]].contiguous().cuda()

    def build(p16):
        m = Resnet(filters=64, input_shape=(3, 480, 480), num_of_patches=15, probability_threshold=0.7, iou_threshold=0.01)
        m.load_state_dict({k: v.clone() for k, v in P.items()})
        m = m.cuda().eval()
        if p16:
            m.engine.set_precision("bf16")
        return m
    m32, m16 = build(False), build(True)
    m8 = Int8Resnet(m32, calibrate(m32, [frames[:min(16, n)]]))
    models = {"bf16x3": m32, "precision16": m16, "int8": m8}

    def run(m):
        with torch.no_grad():
            return m.reduce_bounding_boxes.forward_batch(m.forward_frames(frames))
    boxes = {}
    for k, m in models.items():
        for _ in range(args.warmup):
            rows, counts = run(m)
        boxes[k] = int(counts.sum())
    torch.cuda.synchronize()
    e2e = {k: _stats(v) for k, v in _alternate({k: (lambda m=m: run(m)) for k, m in models.items()}, args.launches, args.calls).items()}

    def kernel_times(m, holder):
        holder.timer = KernelTimer()
        for _ in range(args.kernel_runs):
            run(m)
        s = holder.timer.summary()
        holder.timer = None
        return {name: {"launches_per_call": cnt // args.kernel_runs, "ms_per_call": round(total / args.kernel_runs, 4)}
                for name, (cnt, total, _, _) in sorted(s.items())}
    k8, k16 = kernel_times(m8, m8), kernel_times(m16, m16.engine)

    def classes(ks):
        out = {}
        for name, v in ks.items():
            kind, at = name.split("@")
            cls_ = "stem" if kind.startswith("stem") else "head" if kind.startswith("head") else \
                ("tail@" if at.startswith("15x") else "level@") + at
            out[cls_] = round(out.get(cls_, 0.0) + v["ms_per_call"], 4)
        return out

    # the stem on its own: the integer stem | the float stem + quantise it stands in for | a copy of the same bytes
    x32 = hp.u8_to_f32_norm(frames)
    w32, b32 = m32.conv1.weight.detach().contiguous(), m32.conv1.bias.detach().contiguous()
    hf = torch.empty(n, 64, 240, 240, dtype=torch.float32, device="cuda")
    ws = torch.empty(max((hp.stem_ws_bytes(n, 3, 64, 480, 480, 3, 2, 1) + 3) // 4, 4), dtype=torch.float32, device="cuda")
    x3 = hp.x3_supported(64, 64) and hp.stem_x3_supported(3, 480, 3, 2, 1)
    q_a, q_b = hp.Q8Tensor(n, 64, 240, 240, "cuda"), hp.Q8Tensor(n, 64, 240, 240, "cuda")
    s0 = float(m8.qparams.s_h[0])
    stem_bytes = frames.numel() + n * 64 * 240 * 240
    src = torch.empty(stem_bytes // 2, dtype=torch.uint8, device="cuda").fill_(7)
    dst = torch.empty_like(src)

    def float_pair():
        hp.stem_fwd(x32, w32, b32, hf, ws, 3, 2, 1, x3=x3)
        hp.q8_quantize(hf, s0, out=q_b)
    stem_fns = {"stem3_fwd_q8_u8": lambda: hp.stem3_fwd_q8_u8(frames, m8.stem_wpk, m8.stem_bias, m8.stem_mul, q_a),
                "float_stem+quantize": float_pair, "float_stem": lambda: hp.stem_fwd(x32, w32, b32, hf, ws, 3, 2, 1, x3=x3),
                "q8_quantize": lambda: hp.q8_quantize(hf, s0, out=q_b), "device_copy_same_bytes": lambda: dst.copy_(src)}
    for fn in stem_fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    stem = {k: _stats(v) for k, v in _alternate(stem_fns, args.launches, args.calls).items()}
    code_diff = (q_a.nchw()[:3].to(torch.int16) - q_b.nchw()[:3].to(torch.int16)).abs()    # integer stem against the quantised float stem
    pair_bytes = 4 * frames.numel() + 4 * hf.numel() + 4 * hf.numel() + n * 64 * 240 * 240
    gbs = {"stem3_fwd_q8_u8": round(stem_bytes / stem["stem3_fwd_q8_u8"]["median_ms"] / 1e6, 1),
           "device_copy_same_bytes": round(stem_bytes / stem["device_copy_same_bytes"]["median_ms"] / 1e6, 1),
           "float_stem+quantize": round(pair_bytes / stem["float_stem+quantize"]["median_ms"] / 1e6, 1)}
    macs = float(n) * 64 * 64 * 9 * (2 * 240 * 240 + 2 * 120 * 120 + 2 * 60 * 60 + 2 * 30 * 30 + 12 * 15 * 15)
    res = {"tool": "q8_throughput", "model": "resnet", "device_name": torch.cuda.get_device_name(0), "images": n,
           "launches": args.launches, "calls_per_sample": args.calls, "end_to_end": e2e,
           "images_per_s": {k: round(n / (v["median_ms"] * 1e-3), 1) for k, v in e2e.items()}, "boxes": boxes,
           "counters": dict(m8.counters),
           "over_precision16": round(e2e["precision16"]["median_ms"] / e2e["int8"]["median_ms"], 3),
           "over_bf16x3": round(e2e["bf16x3"]["median_ms"] / e2e["int8"]["median_ms"], 3),
           "int8_kernels": k8, "precision16_kernels": k16, "int8_classes_ms": classes(k8), "precision16_classes_ms": classes(k16),
           "trunk_gmac": round(macs / 1e9, 2), "int8_trunk_floor_ms": round(macs / INT8_PEAK_MACS * 1e3, 4),
           "stem_alone": stem, "stem_bytes": stem_bytes, "float_pair_bytes": pair_bytes, "stem_gb_per_s": gbs,
           "stem_share_of_copy_rate": round(gbs["stem3_fwd_q8_u8"] / gbs["device_copy_same_bytes"], 3),
           "stem_codes_vs_quantized_float_stem": {"max_abs_diff": int(code_diff.max()), "share_off_by_one": round(float((code_diff == 1).float().mean()), 4)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


def main_separablecnn(args):
    """`--model separablecnn`: --images uint8 480x480 frames (seeded random bytes) through a seeded random
    SeparableCNN(filters=64, output_padding=3) to boxes, for the float engine (bf16x3), quantize.Int8SeparableCNN with the
    un-pooled tail as one fdet_q8_sepchain launch, launch by launch, and as constructed -- the protocol above: one process,
    every model warmed up, alternated sample by sample, --calls back-to-back calls per sample, median and 5th / 95th
    percentile.  `faster.sepchain` is the rule of quantize.SEPCHAIN_MEASURED_FASTER.  Then the per-kernel-class table of the
    two int8 modes and of the float engine, and the block kernel on its own at the model's three levels: time, compulsory
    bytes (x read + y written) per second beside a plain device copy of the same bytes, MACs over the dense int8 peak, and at
    60x60 the planner's tile (budget: two workgroups per CU) beside a forced 20x30 tile (one workgroup per CU)."""
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    from fdet_amd.convstack import KernelTimer
    from fdet_amd.models.SeparableCNN import SeparableCNN
    from fdet_amd.quantize import Int8SeparableCNN, calibrate
    if not torch.cuda.is_available():
        raise SystemExit("q8_throughput needs a GPU")
    n = args.images
    torch.manual_seed(190)
    m32 = SeparableCNN(filters=64, input_shape=(3, 480, 480), output_padding=3).cuda().eval()
    frames = torch.randint(0, 256, (n, 3, 480, 480), dtype=torch.uint8, generator=torch.Generator().manual_seed(1190)).cuda()
    qp = calibrate(m32, [frames[:min(16, n)]])

    def build8(chain):
        m = Int8SeparableCNN(m32, qp)
        if chain is not None:
            m.chain = chain                                    # (the switch FDET_Q8_SEPCHAIN sets at construction)
        return m
    int8 = {"int8-blocks": build8("0"), "int8-chain": build8("1"), "int8": build8(None)}
    models = {"bf16x3": m32, **int8}

    def run(m):
        with torch.no_grad():
            return m.reduce_bounding_boxes.forward_batch(m.forward_frames(frames))
    boxes, maps = {}, {}
    for k, m in models.items():
        for _ in range(args.warmup):
            rows, counts = run(m)
        boxes[k] = int(counts.sum())
        with torch.no_grad():
            maps[k] = m.forward_frames(frames)
    identical = all(torch.equal(maps[k], maps["int8-blocks"]) for k in int8)
    dy = (maps["int8"] - maps["bf16x3"]).abs()
    torch.cuda.synchronize()
    e2e = {k: _stats(v) for k, v in _alternate({k: (lambda m=m: run(m)) for k, m in models.items()}, args.launches, args.calls).items()}

    def kernel_times(m, holder):
        holder.timer = KernelTimer()
        for _ in range(args.kernel_runs):
            run(m)
        s = holder.timer.summary()
        holder.timer = None
        return {name: {"launches_per_call": cnt // args.kernel_runs, "ms_per_call": round(total / args.kernel_runs, 4)}
                for name, (cnt, total, _, _) in sorted(s.items())}
    k8 = {k: kernel_times(m, m) for k, m in int8.items() if k != "int8"}
    k32 = kernel_times(m32, m32.engine)

    def classes(ks):
        out = {}
        for name, v in ks.items():
            kind, at = name.split("@")
            cls_ = "stem" if kind.startswith("stem") else "head" if kind.startswith("head") else \
                ("tail@" if at.startswith("15x") else "level@") + at
            out[cls_] = round(out.get(cls_, 0.0) + v["ms_per_call"], 4)
        return out

    # the block kernel on its own
    mb = int8["int8-blocks"]
    alone, fns, info = {}, {}, {}
    for k, (h, pool, tile) in {"60x60_pool": (60, True, (0, 0)), "60x60_pool_tile20x30": (60, True, (20, 30)), "30x30_pool": (30, True, (0, 0)),
                               "15x15": (15, False, (0, 0))}.items():
        blk = {60: 0, 30: 1, 15: 2}[h]
        x, y = hp.Q8Tensor(n, 64, h, h, "cuda"), hp.Q8Tensor(n, 64, h // (2 if pool else 1), h // (2 if pool else 1), "cuda")
        x.storage.random_(-127, 128)
        *w, sm = mb.blocks[blk]
        fns[k] = lambda x=x, y=y, w=w, sm=sm, pool=pool, tile=tile: hp.q8_sepblock(x, *w, sm, y, pool=pool, tile=tile)
        nbytes = n * 64 * h * h * (1.25 if pool else 2.0)
        cp = torch.empty(int(nbytes) // 2, dtype=torch.uint8, device="cuda").fill_(7)
        cd = torch.empty_like(cp)
        fns["copy_" + k] = lambda cp=cp, cd=cd: cd.copy_(cp)
        plan = hp.q8_sepblock_plan(64, h, h, pool)
        info[k] = {"bytes": int(nbytes), "macs": float(n) * 64 * (2 * 64 + 9) * h * h,
                   "tile": list(tile) if tile[0] else list(plan[:2]), "lds_bytes": plan[2] if not tile[0] else None}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    st = {k: _stats(v) for k, v in _alternate(fns, args.launches, args.calls).items()}
    for k, v in info.items():
        ms, cms = st[k]["median_ms"], st["copy_" + k]["median_ms"]
        alone[k] = {**v, **st[k], "gb_per_s": round(v["bytes"] / ms / 1e6, 1), "copy_same_bytes_ms": cms,
                    "copy_gb_per_s": round(v["bytes"] / cms / 1e6, 1), "share_of_copy_rate": round(cms / ms, 3),
                    "int8_peak_share": round(v["macs"] / INT8_PEAK_MACS * 1e3 / ms, 4)}

    def faster(new, old):
        gain = e2e[old]["median_ms"] - e2e[new]["median_ms"]
        spread = max(e2e[old]["spread_ms"], e2e[new]["spread_ms"])
        return {"gain_ms": round(gain, 4), "spread_ms": spread, "faster": bool(gain > spread)}
    from fdet_amd import quantize as Q
    res = {"tool": "q8_throughput", "model": "separablecnn", "device_name": torch.cuda.get_device_name(0), "images": n,
           "launches": args.launches, "calls_per_sample": args.calls, "end_to_end": e2e,
           "images_per_s": {k: round(n / (v["median_ms"] * 1e-3), 1) for k, v in e2e.items()}, "boxes": boxes,
           "int8_maps_identical": identical, "counters": {k: dict(m.counters) for k, m in int8.items()},
           "faster": {"sepchain": faster("int8-chain", "int8-blocks")}, "sepchain_default": bool(Q.SEPCHAIN_MEASURED_FASTER),
           "over_bf16x3": {k: round(e2e["bf16x3"]["median_ms"] / e2e[k]["median_ms"], 3) for k in int8},
           "dy_vs_float_engine": {"max": round(float(dy.max()), 6), "mean": round(float(dy.mean()), 6)},
           "int8_kernels": k8, "float_kernels": k32, "int8_classes_ms": {k: classes(v) for k, v in k8.items()},
           "float_classes_ms": classes(k32), "float_counters": dict(m32.engine.counters), "block_alone": alone}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


def main_ssd(args):
    """`--model ssd`: uint8 480x480 frames (seeded smooth random images) through a seeded random SSD(filters=16) to boxes, for
    the float engine (bf16x3), precision16 and quantize.Int8SSD (calibrated, abs-max, on the first 16 frames) -- the protocol
    above: one process, every model warmed up, alternated sample by sample, --calls back-to-back calls per sample, median and
    5th / 95th percentile -- at --images frames (default 64) and at 24, the recipe's batch.  The float models take the frames
    as TiledDetector hands them over (resize_bilinear_norm, then the stack); the int8 model takes the bytes.  `faster` is the
    rule of the other int8 models: int8 against precision16 by more than the larger of the two spreads.  `frames_to_rows` times
    the same calls without the reducer.  The model is untrained (no trained SSD archive exists) and scores every prior near
    0.5, so at the default threshold of 0.5 the reducer would sort and suppress all 4774 priors of every image and hide the
    network; --threshold (default 0.9) is the reducer's threshold of the three models, at which it keeps what a trained
    detector's would, a few candidates at the most.  Then the per-kernel
    table of the int8 model and of precision16 at --images frames, with each int8 class's MACs over the dense int8 peak."""
    import torch
    import torch.nn.functional as F
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    from fdet_amd.convstack import KernelTimer
    from fdet_amd.models.SSD import SSD
    from fdet_amd.quantize import Int8SSD, calibrate_ssd
    if not torch.cuda.is_available():
        raise SystemExit("q8_throughput needs a GPU")

    def build(p16):
        torch.manual_seed(200)
        m = SSD(16, (3, 480, 480), probability_threshold=args.threshold).cuda().eval()
        if p16:
            m.engine.set_precision("bf16")
        return m
    m32, m16 = build(False), build(True)
    batches = [args.images] + ([24] if args.images != 24 else [])
    nmax = max(batches)
    low = torch.rand(nmax, 3, 30, 30, generator=torch.Generator().manual_seed(1200))
    all_frames = F.interpolate(low, size=(480, 480), mode="bilinear", align_corners=False).mul(255.0).round().clamp(0, 255).to(torch.uint8).cuda()
    m8 = Int8SSD(m32, calibrate_ssd(m32, [all_frames[:min(16, nmax)]]))
    models = {"bf16x3": m32, "precision16": m16, "int8": m8}

    def rows_of(m, frames):
        with torch.no_grad():
            return m.forward_frames(frames) if hasattr(m, "forward_frames") else m(hp.resize_bilinear_norm(frames, (480, 480)))

    def run(m, frames):
        with torch.no_grad():
            return m.reduce_bounding_boxes.forward_batch(rows_of(m, frames))
    per_batch = {}
    for n in batches:
        frames = all_frames[:n].contiguous()
        boxes, ys = {}, {}
        for k, m in models.items():
            for _ in range(args.warmup):
                rows, counts = run(m, frames)
            boxes[k] = int(counts.sum())
            ys[k] = rows_of(m, frames).clone()
        torch.cuda.synchronize()
        fns = {k: (lambda m=m: run(m, frames)) for k, m in models.items()}
        fns.update({k + ":rows": (lambda m=m: rows_of(m, frames)) for k, m in models.items()})
        st = {k: _stats(v) for k, v in _alternate(fns, args.launches, args.calls).items()}
        e2e = {k: v for k, v in st.items() if not k.endswith(":rows")}
        net = {k[:-5]: v for k, v in st.items() if k.endswith(":rows")}

        def faster(t):
            gain = t["precision16"]["median_ms"] - t["int8"]["median_ms"]
            spread = max(t["precision16"]["spread_ms"], t["int8"]["spread_ms"])
            return {"gain_ms": round(gain, 4), "spread_ms": spread, "faster": bool(gain > spread)}
        ds = (ys["int8"][..., 0] - ys["bf16x3"][..., 0]).abs()
        per_batch[str(n)] = {"end_to_end": e2e, "frames_to_rows": net,
                             "images_per_s": {k: round(n / (v["median_ms"] * 1e-3), 1) for k, v in e2e.items()},
                             "boxes": boxes, "over_precision16": round(e2e["precision16"]["median_ms"] / e2e["int8"]["median_ms"], 3),
                             "over_bf16x3": round(e2e["bf16x3"]["median_ms"] / e2e["int8"]["median_ms"], 3),
                             "rows_over_precision16": round(net["precision16"]["median_ms"] / net["int8"]["median_ms"], 3),
                             "rows_over_bf16x3": round(net["bf16x3"]["median_ms"] / net["int8"]["median_ms"], 3),
                             "faster_than_precision16": faster(e2e), "rows_faster_than_precision16": faster(net),
                             "dscore_vs_float_engine": {"max": round(float(ds.max()), 6), "mean": round(float(ds.mean()), 6)}}
    n = args.images
    frames = all_frames[:n].contiguous()

    def kernel_times(m, holder):
        holder.timer = KernelTimer()
        for _ in range(args.kernel_runs):
            run(m, frames)
        s = holder.timer.summary()
        holder.timer = None
        return {name: {"launches_per_call": cnt // args.kernel_runs, "ms_per_call": round(total / args.kernel_runs, 4)}
                for name, (cnt, total, _, _) in sorted(s.items())}
    k8, k16 = kernel_times(m8, m8), kernel_times(m16, m16.engine)
    # MACs of an int8 conv class over the dense int8 peak, from the class name "kind@HxH:ci->co"
    share = {}
    for name, v in k8.items():
        kind, rest = name.split("@")
        at, io = rest.split(":")
        h = int(at.split("x")[0])
        ci, co = (int(t) for t in io.split("->"))
        taps = 9 if kind.startswith(("q8x_conv3x3", "stem")) else 1        # (the stem: 9 taps x 3 input channels)
        macs = float(n) * h * h * taps * ci * co * v["launches_per_call"]
        share[name] = {"gmac": round(macs / 1e9, 3), "int8_peak_share": round(macs / INT8_PEAK_MACS * 1e3 / v["ms_per_call"], 4) if v["ms_per_call"] > 0 else None}
    res = {"tool": "q8_throughput", "model": "ssd", "device_name": torch.cuda.get_device_name(0), "images": n, "batches": batches,
           "probability_threshold": args.threshold, "launches": args.launches, "calls_per_sample": args.calls, "by_batch": per_batch, "counters": dict(m8.counters),
           "int8_kernels": k8, "precision16_kernels": k16, "int8_kernel_macs": share,
           "int8_sum_ms": round(sum(v["ms_per_call"] for v in k8.values()), 4),
           "precision16_sum_ms": round(sum(v["ms_per_call"] for v in k16.values()), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("poolresnet", "resnet", "separablecnn", "ssd"), default="poolresnet")
    ap.add_argument("--images", type=int, default=None, help="frames per call (default 256; resnet: 32; ssd: 64)")
    ap.add_argument("--launches", type=int, default=100, help="timed samples per mode")
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls per sample")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-runs", type=int, default=50)
    ap.add_argument("--threshold", type=float, default=0.9, help="ssd: the reducer's probability threshold (see main_ssd)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.images is None:
        args.images = 32 if args.model == "resnet" else 64 if args.model == "ssd" else 256
    if args.model == "ssd":
        return main_ssd(args)
    if args.model == "resnet":
        return main_resnet(args)
    if args.model == "separablecnn":
        return main_separablecnn(args)
    import numpy as np
    import torch
    import fdet_amd  # noqa: F401
    from fdet_amd.convstack import KernelTimer
    from fdet_amd.models.PoolResnet import PoolResnet
    from fdet_amd.quantize import Int8PoolResnet, calibrate
    if not torch.cuda.is_available():
        raise SystemExit("q8_throughput needs a GPU")
    gold = os.path.join(ROOT, "tests", "golden")
    g = np.load(os.path.join(gold, "g16_trained_medium.npz"))
    P = {k[len("param/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    images = torch.from_numpy(np.load(os.path.join(gold, "g6_trained_small.npz"))["images"])
    n = args.images
    frames = images[torch.arange(n) % images.shape[0]].contiguous().cuda()

    def build(p16):
        m = PoolResnet(filters=64, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.7, iou_threshold=0.01)
        m.load_state_dict({k: v.clone() for k, v in P.items()})
        m = m.cuda().eval()
        if p16:
            m.engine.set_precision("bf16")
        return m
    m32, m16 = build(False), build(True)
    qp = calibrate(m32, [frames[:16]])

    def build8(chain, stem):
        m = Int8PoolResnet(m32, qp)
        if chain is not None:
            m.chain, m.stem_q8 = chain, stem                  # (the switches FDET_Q8_CHAIN / FDET_Q8_STEM set at construction)
        return m
    int8 = {"int8-layers": build8("0", "0"), "int8-chain": build8("1", "0"), "int8-chain+stem": build8("1", "1"),
            "int8": build8(None, None)}
    mi = Int8PoolResnet(m32, qp, stem="integer")
    models = {"bf16x3": m32, "precision16": m16, **int8, "int8-integer-stem": mi}

    def run(m):
        with torch.no_grad():
            return m.reduce_bounding_boxes.forward_batch(m.forward_frames(frames))
    boxes, maps = {}, {}
    for k, m in models.items():
        for _ in range(args.warmup):
            rows, counts = run(m)
        boxes[k] = int(counts.sum())
        if k in int8:
            with torch.no_grad():
                maps[k] = m.forward_frames(frames)
    identical = all(torch.equal(v, maps["int8-layers"]) for v in maps.values())
    torch.cuda.synchronize()
    ms = {k: [] for k in models}
    for _ in range(args.launches):
        for k, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                run(m)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.calls)

    def stats(v):
        a = np.sort(np.asarray(v))
        p05, p95 = float(np.percentile(a, 5)), float(np.percentile(a, 95))
        return {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a[0]), 4), "max_ms": round(float(a[-1]), 4),
                "p05_ms": round(p05, 4), "p95_ms": round(p95, 4), "spread_ms": round(p95 - p05, 4)}

    # per-kernel times (a phase of its own: the events slow the host side down a little)
    def kernel_times(m, holder):
        holder.timer = KernelTimer()
        for _ in range(args.kernel_runs):
            run(m)
        s = holder.timer.summary()
        holder.timer = None
        return {name: {"launches_per_call": cnt // args.kernel_runs, "ms_per_call": round(total / args.kernel_runs, 4)}
                for name, (cnt, total, _, _) in sorted(s.items())}
    k8 = {k: kernel_times(m, m) for k, m in int8.items() if k != "int8"}
    k16 = kernel_times(m16, m16.engine)
    ki = kernel_times(mi, mi)

    def cls(ks, names):
        return round(sum(v["ms_per_call"] for k, v in ks.items() if k.split("@")[0] in names), 4)
    at15 = {k: {n_: v for n_, v in ks.items() if n_.endswith("@15x15")} for k, ks in k8.items()}
    tail = {"int8-layers": cls(at15["int8-layers"], ("q8_conv3x3", "q8_conv3x3_skip", "q8_dequantize")),
            "int8-chain": cls(at15["int8-chain"], ("q8_chain",)), "int8-chain+stem": cls(at15["int8-chain+stem"], ("q8_chain",))}
    stem = {"int8-layers": cls(k8["int8-layers"], ("stem_fwd", "q8_quantize")), "int8-chain": cls(k8["int8-chain"], ("stem_fwd", "q8_quantize")),
            "int8-chain+stem": cls(k8["int8-chain+stem"], ("stem_fwd_q8",)), "int8-integer-stem": cls(ki, ("stem10_fwd_q8",)),
            "precision16": cls(k16, ("stem_fwd",))}
    trunk8 = {k: cls(ks, ("q8_conv3x3", "q8_conv3x3_skip", "q8_conv3x3_pool", "q8_chain", "q8_dequantize")) for k, ks in k8.items()}
    trunk16 = sum(v["ms_per_call"] for k, v in k16.items() if k.startswith(("conv3x3_fwd", "chain_fwd")))
    # (blocks 0 and 1 are pooled: 2 convs at 60x60, 2 at 30x30; then 8 blocks = 16 convs at 15x15)
    tail_macs = float(n) * 64 * 64 * 9 * 16 * 15 * 15
    trunk_macs = float(n) * 64 * 64 * 9 * (2 * 60 * 60 + 2 * 30 * 30 + 16 * 15 * 15)
    floor_ms, tail_floor_ms = trunk_macs / INT8_PEAK_MACS * 1e3, tail_macs / INT8_PEAK_MACS * 1e3
    e2e = {k: stats(v) for k, v in ms.items()}

    # the stem on its own: the integer stem | the quantising float stem | the float stem + quantise | a copy of the same bytes
    from fdet_amd import hotpath as hp
    x32 = hp.u8_to_f32_norm(frames)
    w32, b32 = m32.conv1.weight.detach().contiguous(), m32.conv1.bias.detach().contiguous()
    hf = torch.empty(n, 64, 60, 60, dtype=torch.float32, device="cuda")
    ws = torch.empty(max((hp.stem_ws_bytes(n, 3, 64, 480, 480, 10, 8, 2) + 3) // 4, 4), dtype=torch.float32, device="cuda")
    x3 = hp.x3_supported(64, 64) and hp.stem_x3_supported(3, 480, 10, 8, 2)
    q_a, q_b, q_c = (hp.Q8Tensor(n, 64, 60, 60, "cuda") for _ in range(3))
    s0 = float(qp.s_h[0])
    stem_bytes = frames.numel() + n * 64 * 60 * 60
    src = torch.empty(stem_bytes // 2, dtype=torch.uint8, device="cuda").fill_(7)
    dst = torch.empty_like(src)

    def float_pair():
        hp.stem_fwd(x32, w32, b32, hf, ws, 10, 8, 2, x3=x3)
        hp.q8_quantize(hf, s0, out=q_b)
    stem_fns = {"stem10_fwd_q8_u8": lambda: hp.stem10_fwd_q8_u8(frames, mi.stem_wpk, mi.stem_bias, mi.stem_mul, q_a),
                "float_stem+quantize": float_pair, "device_copy_same_bytes": lambda: dst.copy_(src)}
    if hp.stem_fwd_q8_ok(n, 3, 64, 480, 480, 10, 8, 2):
        stem_fns["stem_fwd_q8_u8"] = lambda: hp.stem_fwd_q8_u8(frames, w32, b32, s0, q_c, 10, 8, 2)
    for fn in stem_fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    stem_alone = {k: _stats(v) for k, v in _alternate(stem_fns, args.launches, args.calls).items()}
    code_diff = (q_a.nchw()[:3].to(torch.int16) - q_b.nchw()[:3].to(torch.int16)).abs()    # integer stem against the quantised float stem
    gbs = {k: round(stem_bytes / stem_alone[k]["median_ms"] / 1e6, 1) for k in ("stem10_fwd_q8_u8", "device_copy_same_bytes")}

    def faster(new, old):
        gain = e2e[old]["median_ms"] - e2e[new]["median_ms"]
        spread = max(e2e[old]["spread_ms"], e2e[new]["spread_ms"])
        return {"gain_ms": round(gain, 4), "spread_ms": spread, "faster": bool(gain > spread)}
    res = {"tool": "q8_throughput", "device_name": torch.cuda.get_device_name(0), "images": n, "launches": args.launches,
           "calls_per_sample": args.calls, "end_to_end": e2e, "images_per_s": {k: round(n / (v["median_ms"] * 1e-3), 1) for k, v in e2e.items()},
           "boxes": boxes, "int8_maps_identical": identical,
           "counters": {k: dict(m.counters) for k, m in int8.items()},
           "faster": {"chain": faster("int8-chain", "int8-layers"), "stem": faster("int8-chain+stem", "int8-chain"),
                      "integer_stem": faster("int8-integer-stem", "int8")},
           "over_precision16": {k: round(e2e["precision16"]["median_ms"] / e2e[k]["median_ms"], 3) for k in (*int8, "int8-integer-stem")},
           "over_bf16x3": {k: round(e2e["bf16x3"]["median_ms"] / e2e[k]["median_ms"], 3) for k in (*int8, "int8-integer-stem")},
           "int8_kernels": k8, "int8_integer_stem_kernels": ki, "integer_stem_counters": dict(mi.counters), "precision16_kernels": k16,
           "stem_alone": stem_alone, "stem_bytes": stem_bytes, "stem_gb_per_s": gbs,
           "stem_share_of_copy_rate": round(gbs["stem10_fwd_q8_u8"] / gbs["device_copy_same_bytes"], 3),
           "stem_codes_vs_quantized_float_stem": {"max_abs_diff": int(code_diff.max()),
                                                  "share_that_differ": round(float((code_diff != 0).float().mean()), 4)},
           "tail_15x15_ms": tail, "stem_ms": stem,
           "trunk_20_convs_ms": {**trunk8, "precision16": round(trunk16, 4)},
           "tail_gmac": round(tail_macs / 1e9, 2), "int8_tail_floor_ms": round(tail_floor_ms, 4),
           "int8_tail_floor_share": {k: round(tail_floor_ms / v, 4) if v > 0 else None for k, v in tail.items()},
           "trunk_gmac": round(trunk_macs / 1e9, 2), "int8_trunk_floor_ms": round(floor_ms, 4),
           "int8_trunk_floor_share": {k: round(floor_ms / v, 4) if v > 0 else None for k, v in trunk8.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
