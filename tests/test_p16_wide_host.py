"""precision16 on the fp32-I/O conv kernels (PoolResnet-large, F=128), host side (no GPU):

* every one-pass `_bf16` entry is declared in include/fdet.h, listed in the ctypes table and exported by the built library;
* the one-pass instantiations of the register-staged pipelined weight gradient (k_wgrad3x3_x3_pipe<..., P16 = true>) keep
  the asm-load protocol: zero touches of an in-flight destination (tools/audit_asm_loads.py), audited by their full
  mangled prefix next to their bf16x3 twins (test_asm_audit.py audits only the first symbol behind each of its prefixes).
"""
import importlib.util
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-face-detection-from-scratch_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

P16_ENTRIES = ["fdet_conv3x3_fwd_bf16", "fdet_conv3x3_dgrad_bf16", "fdet_conv3x3_fwd_pool_bf16",
               "fdet_conv3x3_dgrad_unpool_bf16", "fdet_conv3x3_wgrad_bf16", "fdet_conv3x3_wgrad_bf16_batched"]

# <VW, DBG, LPR, PK4, P16>: the four pipelined forms the planner builds, in both precisions
PIPE = "_ZN12_GLOBAL__N_118k_wgrad3x3_x3_pipeILi"
PIPE_FORMS = ["4ELi0ELi16ELi0E", "4ELi0ELi16ELi1E", "4ELi0ELi32ELi1E", "1ELi0ELi32ELi0E"]


def _native():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_one_pass_entries_are_declared_tabled_and_exported():
    N = _native()
    declared = set(N.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in P16_ENTRIES:
        assert name in declared, f"{name} not declared in include/fdet.h"
        assert name in N.SIGNATURES, f"{name} missing from the ctypes table"
        assert name in exported, f"{name} not exported by {os.path.basename(N.LIB_PATH)}"
        twin = name.replace("_bf16", "_bf16x3")
        assert N.SIGNATURES[name] == N.SIGNATURES[twin], f"{name}: arguments differ from {twin}"


def test_hotpath_takes_p16_on_every_fp32_io_conv():
    import inspect
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    for fn in (hp.conv3x3_fwd, hp.conv3x3_dgrad, hp.conv3x3_fwd_pool, hp.conv3x3_dgrad_unpool, hp.conv3x3_wgrad,
               hp.conv3x3_wgrad_batched):
        prm = inspect.signature(fn).parameters
        assert "p16" in prm and prm["p16"].default is False, fn.__name__


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_one_pass_pipelined_weight_gradient_keeps_the_asm_load_protocol(tmp_path):
    spec = importlib.util.spec_from_file_location("audit_asm_loads", os.path.join(ROOT, "tools", "audit_asm_loads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "fdet_wgrad3x3_x3.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, "fdet_wgrad3x3_x3.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    for form in PIPE_FORMS:
        for p16 in (1, 0):
            k = f"{PIPE}{form}Lb{p16}E"
            nload, bad, foreign = mod.audit(k, str(out), verbose=False)
            assert nload > 0, f"{k}: no asm buffer loads found (instantiation not built?)"
            print(f"{k}: {nload} asm loads, {bad} touches, {foreign} foreign vector-memory ops")
            assert bad == 0, f"{k}: {bad} instructions touch an in-flight asm load destination: {mod.audit.last_touches[:4]}"


def test_precision16_is_available_at_F128():
    """set_precision("bf16") and FDET_PRECISION=bf16 reach the fp32-I/O kernels: PoolResnet-large (F=128) is no longer
    refused (set_precision) or silently ignored (the environment variable, read when the engine is built)."""
    import fdet_amd  # noqa: F401
    from fdet_amd.models.PoolResnet import PoolResnet
    eng = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10).engine
    assert eng.x3 and not eng.ps and not eng.p16
    eng.set_precision("bf16")
    assert eng.p16
    eng.set_precision("bf16x3")
    assert not eng.p16
    code = ("import fdet_amd\nfrom fdet_amd.models.PoolResnet import PoolResnet\n"
            "e = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10).engine\n"
            "print('P16', int(e.p16))\n")
    for env_val, want in (("bf16", "P16 1"), ("bf16x3", "P16 0")):
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, FDET_PRECISION=env_val),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert want in r.stdout, (env_val, r.stdout)


def test_precision16_refused_on_the_exact_fp32_path(monkeypatch):
    import fdet_amd  # noqa: F401
    from fdet_amd.models.PoolResnet import PoolResnet
    monkeypatch.setenv("FDET_PRECISION", "f32")
    eng = PoolResnet(filters=128, input_shape=(3, 480, 480), num_of_patches=10).engine
    assert not eng.x3 and not eng.p16
    with pytest.raises(ValueError, match="exact-fp32"):
        eng.set_precision("bf16")
