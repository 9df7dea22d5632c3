"""Launch trace of ConvStack.forward / backward without a GPU (helper of tests/test_convstack_trace.py).

A recording proxy stands in front of `_native.lib()` and the pass runs on `device="meta"` tensors:
  * an entry of `_native.SIGNATURES` without a pointer argument is a host query and goes to the real library, and so do the
    entries that take pointers but only write host memory (FORWARDED) -- the engine's decisions hang on their answers;
  * every other entry is recorded and returns 0.
A record is [name, arg, ...]: integers and floats as they were passed, a pointer as the ordinal of its tensor's first
appearance within the step (0 = NULL; `PsTensor.data` counts as its buffer), a pointer array as the list of its elements'
ordinals.  So a trace pins the dataflow as well as the order, whichever pooled buffer was recycled.  Interleaved with the
launches: ["@span", name, flops, bytes] where a KernelTimer span opens, ["@after_block", k] for the data-parallel callback,
and ["@ps_alloc", n] at the end of a step for the PsTensors it allocated (the pool at work).

`python tests/convstack_trace.py --write` records tests/golden/convstack_trace/trace.json (pack(): per step the sequence of
its launches and a digest over all their arguments); `--show CASE` prints a case's full trace."""
import ctypes
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import fdet_amd  # noqa: E402,F401
from fdet_amd import _native, hotpath as hp, ps as psm  # noqa: E402
from fdet_amd.convstack import ConvStack, StackGeometry, param_names  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "convstack_trace", "trace.json")
FORWARDED = {"fdet_conv3x3_wgrad_bf16x3_plan", "fdet_sepblock_plan", "fdet_conv3x3_x3_last_route", "fdet_stem_last_route"}
F32 = torch.float32
_SPACING = 40                                              # fake addresses: (tensor index + 1) << 40, offsets stay below


class Recorder:
    """Stands in for lib(), ptr(), stream() and the engine's timer; `events` is the trace of the current step."""

    def __init__(self):
        self.real = _native.lib()
        self.events = []
        self._base = {}                                    # storage -> fake base address
        self._keep = []                                    # (keeps every storage alive, so that no key is reused)
        self._ordinal = {}
        self._ps_allocs = 0

    # ---- what the wrappers call
    def lib(self):
        return self

    def stream(self):
        return 0

    def ptr(self, t, dtype=F32):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"expected a torch.Tensor, got {type(t)}")
        if t.dtype != dtype:
            raise TypeError(f"expected dtype {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise TypeError("expected a contiguous tensor")
        st = t.untyped_storage()
        key = st._cdata
        if key not in self._base:
            self._keep.append(st)
            self._base[key] = len(self._keep) << _SPACING
        return self._base[key] + t.storage_offset() * t.element_size()

    def __getattr__(self, name):
        if name not in _native.SIGNATURES:
            raise AttributeError(name)
        argtypes = _native.SIGNATURES[name][1]
        if name in FORWARDED or ctypes.c_void_p not in argtypes:
            return getattr(self.real, name)

        def launch(*args):
            if len(args) != len(argtypes):
                raise TypeError(f"{name}: {len(args)} arguments, the C-ABI takes {len(argtypes)}")
            self.events.append([name] + [self._arg(ty, v) for ty, v in zip(argtypes, args)])
            return 0
        launch.__name__ = name
        return launch

    # ---- the engine's timer
    def span(self, name, flops=0.0, nbytes=0.0):
        self.events.append(["@span", name, float(flops), float(nbytes)])
        return _Null()

    # ---- records
    def _ord(self, addr):
        if not addr:
            return 0
        return self._ordinal.setdefault(addr >> _SPACING, len(self._ordinal) + 1)

    def _arg(self, ty, v):
        if ty is ctypes.c_void_p:
            if isinstance(v, ctypes.Array):
                return [self._ord(a) for a in v]
            return self._ord(v)
        if ty in (ctypes.c_float, ctypes.c_double):
            return float(v)
        return int(v)

    def end_step(self):
        ev, self.events, self._ordinal = self.events, [], {}
        ev.append(["@ps_alloc", self._ps_allocs])
        self._ps_allocs = 0
        return ev


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def install(monkeypatch):
    """Patch lib / ptr / stream where the wrappers look them up (they import them by name); returns the Recorder."""
    rec = Recorder()
    for mod in (_native, hp, psm):
        for name in ("lib", "ptr", "stream"):
            monkeypatch.setattr(mod, name, getattr(rec, name))
    init = psm.PsTensor.__init__

    def counted(self, *a, **kw):
        rec._ps_allocs += 1
        init(self, *a, **kw)
    monkeypatch.setattr(psm.PsTensor, "__init__", counted)
    return rec


# ------------------------------------------------------------------------------------------------------------- cases
def _geo(kind, F_, size, S):
    if kind == "poolresnet":
        return StackGeometry("poolresnet", F_, 3, size, size, S, 10, 10, 8, 2, 6, 0, pool_mult=2)
    return StackGeometry("resnet", F_, 3, size, size, S, 10, 3, 2, 1, 3, 1, pool_mult=1)


def _case(kind, F_, size, S, N, prec="bf16x3", mode="train", env=None, strips=None):
    return {"kind": kind, "F": F_, "size": size, "S": S, "N": N, "prec": prec, "mode": mode, "env": env or {}, "strips": strips}


def cases():
    """id -> case; together they take every branch of ConvStack.forward / backward."""
    out = {}
    for prec in ("bf16x3", "bf16"):
        for N in (2, 7, 256, 776, 777, 2330, 2331, 2400):
            out[f"pool64_480_N{N}_{prec}"] = _case("poolresnet", 64, 480, 10, N, prec)
        for N in (2, 1165, 1166):
            out[f"pool128_480_N{N}_{prec}"] = _case("poolresnet", 128, 480, 10, N, prec)
        out[f"pool16_480_N2_{prec}"] = _case("poolresnet", 16, 480, 10, 2, prec)
        out[f"pool64_480_N2_{prec}_flipped"] = _case("poolresnet", 64, 480, 10, 2, prec, mode="flip")
        out[f"pool64_480_N2_{prec}_replaced"] = _case("poolresnet", 64, 480, 10, 2, prec, mode="replace")
    for var in ("FDET_PS", "FDET_CHAIN", "FDET_POOL_FUSION", "FDET_HEAD_FUSED"):
        out[f"pool64_480_N2_{var}=0"] = _case("poolresnet", 64, 480, 10, 2, env={var: "0"})
        out[f"pool64_480_N2_{var}=0_fused_head"] = _case("poolresnet", 64, 480, 10, 2, mode="fused_head", env={var: "0"})
    out["pool64_480_N2_f32"] = _case("poolresnet", 64, 480, 10, 2, prec=None, env={"FDET_PRECISION": "f32"})
    out["pool64_480_N2_f32_replaced"] = _case("poolresnet", 64, 480, 10, 2, prec=None, mode="replace", env={"FDET_PRECISION": "f32"})
    out["pool8_480_N2"] = _case("poolresnet", 8, 480, 10, 2, prec=None)
    for N in (2, 42, 81, 82, 84):
        out[f"res64_640_N{N}"] = _case("resnet", 64, 640, 20, N)
    out["res64_640_N42_no_strips"] = _case("resnet", 64, 640, 20, 42, strips=False)
    out["res64_640_N42_bf16"] = _case("resnet", 64, 640, 20, 42, "bf16")
    out["res64_256_N5"] = _case("resnet", 64, 256, 8, 5)
    out["res64_256_N5_bf16"] = _case("resnet", 64, 256, 8, 5, "bf16")
    for N in (2, 2400):
        out[f"pool64_480_N{N}_infer"] = _case("poolresnet", 64, 480, 10, N, mode="infer")
        out[f"pool64_480_N{N}_infer_u8"] = _case("poolresnet", 64, 480, 10, N, mode="infer_u8")
    out["pool64_480_N2_bf16_infer_u8"] = _case("poolresnet", 64, 480, 10, 2, "bf16", mode="infer_u8")
    out["res64_640_N2_infer"] = _case("resnet", 64, 640, 20, 2, mode="infer")
    out["pool128_480_N2_infer"] = _case("poolresnet", 128, 480, 10, 2, mode="infer")
    for prec in ("bf16x3", "bf16"):
        out[f"pool64_480_N2_{prec}_fused_head"] = _case("poolresnet", 64, 480, 10, 2, prec, mode="fused_head")
    out["res64_640_N2_fused_head"] = _case("resnet", 64, 640, 20, 2, mode="fused_head")
    out["pool64_480_steps_4_4_3"] = _case("poolresnet", 64, 480, 10, (4, 4, 3), mode="steps")
    return out


def _meta(*shape, dtype=F32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def _params(g):
    shapes = {"conv1.weight": (g.filters, g.in_ch, g.stem_k, g.stem_k), "conv1.bias": (g.filters,),
              "out.weight": (5, g.filters, g.head_k, g.head_k), "out.bias": (5,)}
    P = {}
    for n in param_names(g.num_blocks):
        P[n] = _meta(*shapes.get(n, (g.filters, g.filters, 3, 3) if n.endswith("weight") else (g.filters,)))
    return P


def _step(rec, eng, P, N, mode):
    """One pass of `mode` at batch N; returns its events."""
    g = eng.geo
    F_ = g.filters
    if mode in ("infer", "infer_u8"):
        x = _meta(N, g.in_ch, g.H, g.W, dtype=torch.uint8 if mode == "infer_u8" else F32)
        eng.forward(x, P, None, save=False, u8_frames=mode == "infer_u8")
        return rec.end_step()
    x = _meta(N, g.in_ch, g.H, g.W)
    masks = {f"residual_blocks.{k}": _meta(N, F_) for k in range(g.num_blocks)}
    masks["head"] = _meta(N, F_)
    G = {n: torch.empty_like(p) for n, p in P.items()}
    if mode == "fused_head":
        y, saved = eng.forward(x, P, masks, save=True, loss_targets=_meta(N, 5, g.S, g.S), G=G)
        dy = None if saved.get("head_dout") is not None else torch.empty_like(y)
    else:
        y, saved = eng.forward(x, P, masks, save=True)
        dy = torch.empty_like(y)
    if mode == "flip":                                     # backward follows the precision of its forward, not this
        eng.set_precision("bf16x3" if eng.p16 else "bf16")
    if mode == "replace":                                  # a caller puts fp32 NCHW tensors in place of the saved ones
        for k, (hk, pool) in enumerate(eng.lv):
            xin, a, third = saved["blocks"][k]
            if isinstance(a, psm.PsTensor) and pool == 2:  # pooled PS block: a and NCHW routing bytes
                saved["blocks"][k] = (xin, _meta(N, F_, hk, hk), _meta(N, F_, hk // 2, hk // 2, dtype=torch.uint8))
            elif isinstance(a, psm.PsTensor):              # PS chain block: a and c
                saved["blocks"][k] = (xin, _meta(N, F_, hk, hk), _meta(N, F_, hk, hk))
            else:                                          # fp32 route: all three
                saved["blocks"][k] = (_meta(N, F_, hk, hk), _meta(N, F_, hk, hk), _meta(*third.shape, dtype=third.dtype))
    eng.backward(saved, dy, P, G, after_block=lambda k: rec.events.append(["@after_block", int(k)]))
    return rec.end_step()


def run_case(case, monkeypatch):
    """The steps of one case, each a list of events.  `monkeypatch` carries the recorder and the case's environment."""
    for k in ("FDET_PRECISION", "FDET_PS", "FDET_CHAIN", "FDET_POOL_FUSION", "FDET_HEAD_FUSED", "FDET_PS_STRIPS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    rec = install(monkeypatch)
    eng = ConvStack(_geo(case["kind"], case["F"], case["size"], case["S"]))
    if case["prec"] is not None:
        eng.set_precision(case["prec"])
    if case["strips"] is not None:
        eng.ps_strips = case["strips"]
    eng.timer = rec
    P = _params(eng.geo)
    Ns = case["N"] if case["mode"] == "steps" else (case["N"],)
    return [_step(rec, eng, P, N, "train" if case["mode"] == "steps" else case["mode"]) for N in Ns]


SAMPLE = "pool64_480_N2_bf16x3"                            # the case the fixture also holds in full, to be read


def _label(e):
    """An event without its arguments: the entry point, "@span <name>", "@after_block <k>", "@ps_alloc <n>"."""
    return e[0] if not e[0].startswith("@") else f"{e[0]} {e[1]}"


def digest(step):
    return hashlib.sha256(json.dumps(step, separators=(",", ":")).encode()).hexdigest()[:16]


def pack(traces):
    """The fixture's form of {case: steps}.  A step is [outline, events, digest]: its outline is the sequence of its events'
    labels (indices into "names"; steps with the same sequence share one), its digest covers every event with all its
    arguments.  The SAMPLE case is there in full as well."""
    names, outlines, cases_ = [], [], {}
    for cid in sorted(traces):
        cases_[cid] = []
        for step in traces[cid]:
            for e in step:
                if _label(e) not in names:
                    names.append(_label(e))
            o = [names.index(_label(e)) for e in step]
            if o not in outlines:
                outlines.append(o)
            cases_[cid].append([outlines.index(o), len(step), digest(step)])
    return {"names": names, "outlines": outlines, "cases": cases_, "sample": traces[SAMPLE]}


def dumps(packed):
    """One line per name table, outline, case and sample event."""
    one = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    rows = lambda vs: "[\n  " + ",\n  ".join(one(v) for v in vs) + "\n ]"  # noqa: E731
    cases_ = "{\n  " + ",\n  ".join(f"{json.dumps(c)}: {one(v)}" for c, v in packed["cases"].items()) + "\n }"
    sample = "[" + ", ".join(rows(st) for st in packed["sample"]) + "]"
    return (f'{{\n "names": {one(packed["names"])},\n "outlines": {rows(packed["outlines"])},\n "cases": {cases_},\n'
            f' "sample": {sample}\n}}\n')


def record(only=None):
    import pytest
    traces = {}
    for cid, case in cases().items():
        if only is None or cid == only:
            with pytest.MonkeyPatch.context() as mp:
                traces[cid] = run_case(case, mp)
    return traces


if __name__ == "__main__":
    if "--show" in sys.argv:                               # the full trace of one case, to diff between two commits
        cid = sys.argv[sys.argv.index("--show") + 1]
        for step in record(cid)[cid]:
            print("\n".join(json.dumps(e, separators=(",", ":")) for e in step))
        sys.exit(0)
    text = dumps(pack(record()))
    if "--write" in sys.argv:
        os.makedirs(os.path.dirname(FIXTURE), exist_ok=True)
        with open(FIXTURE, "w") as f:
            f.write(text)
    print(f"{len(cases())} cases, {len(text)} bytes")
