"""Host-side checks of the int8 chain and the quantising stem (no GPU): the conditions on the chain cases' data, the plan
queries and argument refusals of the new entry points, and the asm-load audit of the new stem instantiation."""
import ctypes
import importlib.util
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_chain_cases as CC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-face-detection-from-scratch_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.parametrize("i", range(len(CC.CHAIN_CASES)), ids=CC.CHAIN_IDS)
def test_chain_cases_are_neither_saturated_nor_dead(i):
    """Conditions on the inputs, so that saturation or a dead signal cannot hide a wrong kernel: every intermediate tensor of
    the restatement has at most 1.5 % of its values at +-127, at most 15 % zeros and a standard deviation of at least 8
    (with this generator: at most 0.81 %, 12.5 % -- the 1x1 case, 8 of 64 values -- and at least 10.1)."""
    ref = CC.chain_ref(i)
    assert len(ref) == CC.CHAIN_CASES[i][3]
    for k, (a, h) in enumerate(ref):
        for name, t in (("a", a), ("h", h)):
            sat, zero, std = float(np.mean(np.abs(t.astype(np.int32)) == 127)), float(np.mean(t == 0)), float(t.astype(np.float64).std())
            print(f"block {k} {name}: {100 * sat:.2f} % at +-127, {100 * zero:.2f} % zeros, std {std:.1f}")
            assert t.dtype == np.int8 and t.shape == CC.make_chain_case(i)["shape"]
            assert sat <= 0.015 and zero <= 0.15 and std >= 8.0, (k, name, sat, zero, std)


def test_ties_case_holds_exact_ties():
    """At least 5 % of the values before rounding are exact ties (x.5), in every conv of the ties chain, and most of them
    lie inside the int8 range (rounded half to even, not clamped)."""
    d = CC.make_ties_case()
    for n, t in enumerate(CC.pre_rounding(d)):
        tie = np.abs(t - np.floor(t)) == 0.5
        inside = tie & (np.abs(t) < 127)
        print(f"conv {n}: {100 * float(tie.mean()):.1f} % ties, {100 * float(inside.mean()):.1f} % inside the range")
        assert float(tie.mean()) >= 0.05 and float(inside.mean()) >= 0.05


def test_plan_queries_and_argument_refusals_need_no_gpu():
    from fdet_amd import _native
    L = _native.lib()
    assert [L.fdet_q8_chain_supported(*s) for s in ((64, 15, 15), (64, 16, 16), (64, 1, 1))] == [1, 1, 1]
    assert [L.fdet_q8_chain_supported(*s) for s in ((128, 15, 15), (64, 17, 15), (64, 15, 17), (64, 0, 15))] == [0, 0, 0, 0]
    assert L.fdet_stem_fwd_q8_ok(256, 3, 64, 480, 480, 10, 8, 2) == 1
    assert L.fdet_stem_fwd_q8_ok(256, 3, 128, 480, 480, 10, 8, 2) == 0
    assert L.fdet_stem_fwd_q8_ok(256, 3, 64, 480, 480, 3, 8, 2) == 0
    assert L.fdet_stem_fwd_q8_ok(2, 3, 64, 478, 478, 10, 8, 2) == 0          # W % 4
    assert L.fdet_stem_fwd_q8_ok(0, 3, 64, 480, 480, 10, 8, 2) == 0
    # host addresses: only ever compared with NULL or tested for alignment, nothing is enqueued
    buf = ctypes.create_string_buffer(256)
    p16 = (ctypes.addressof(buf) + 15) & ~15
    arr = (ctypes.c_void_p * 17)(*[p16 + 16] * 17)
    sm = (ctypes.c_float * 17)(*[0.75] * 17)
    outs = (ctypes.c_void_p * 17)(*[p16 + 32] * 17)

    def call(x=p16, out=outs, f32=None, nb=2, C=64, H=15, W=15, a=arr, scale=1.0):
        return L.fdet_q8_chain(x, a, a, a, a, a, a, sm, out, f32, scale, nb, 1, C, H, W, 0.2, None)
    assert call(nb=0) == -1 and b"nblocks" in L.fdet_last_error()
    assert call(nb=17) == -1 and b"nblocks" in L.fdet_last_error()
    none_last = (ctypes.c_void_p * 17)(*([p16 + 32] + [None] * 16))
    assert call(out=none_last, nb=2) == -1 and b"output" in L.fdet_last_error()
    assert call(out=None, nb=2) == -1 and b"output" in L.fdet_last_error()
    assert call(C=128) == -1 and call(H=17) == -1 and call(W=0) == -1
    assert call(x=p16 + 4) == -1 and b"aligned" in L.fdet_last_error()
    assert call(a=(ctypes.c_void_p * 17)(*[p16 + 24] * 17)) == -1 and b"aligned" in L.fdet_last_error()
    assert call(out=(ctypes.c_void_p * 17)(*[p16] * 17)) == -1 and b"alias" in L.fdet_last_error()
    assert call(out=None, f32=p16 + 64, scale=0.0) == -1 and b"out_scale" in L.fdet_last_error()
    assert L.fdet_stem_fwd_q8_u8(None, None, None, 1.0, None, 1, 3, 64, 480, 480, 10, 8, 2, None) == -1
    assert L.fdet_stem_fwd_q8_u8(p16, p16, p16, 0.0, p16, 1, 3, 64, 480, 480, 10, 8, 2, None) == -1 and b"scale" in L.fdet_last_error()
    assert L.fdet_stem_fwd_q8_u8(p16, p16, p16, 1.0, p16, 1, 3, 128, 480, 480, 10, 8, 2, None) == -1
    assert L.fdet_stem_fwd_q8_u8(p16, p16, p16, 1.0, p16 + 8, 1, 3, 64, 480, 480, 10, 8, 2, None) == -1


def test_wrappers_check_their_arguments():
    import torch
    from fdet_amd import hotpath as hp
    w = torch.zeros(9 * 64 * 64, dtype=torch.int8)
    b, m = torch.zeros(64, dtype=torch.int32), torch.zeros(64)
    with pytest.raises(ValueError):
        hp.Q8ChainWeights([], [], [])
    with pytest.raises(ValueError):
        hp.Q8ChainWeights([(w, b, m)] * 17, [(w, b, m)] * 17, [0.5] * 17)
    with pytest.raises(ValueError):
        hp.Q8ChainWeights([(w[:-1], b, m)], [(w, b, m)], [0.5])
    with pytest.raises(ValueError):
        hp.q8_chain(torch.zeros(4), None)
    with pytest.raises(ValueError):
        hp.stem_fwd_q8_u8(torch.zeros(1, 3, 16, 16), torch.zeros(64, 3, 10, 10), torch.zeros(64), 1.0, None)


Q8_STEM = "_ZN12_GLOBAL__N_118k_stem_fwd_x3_pipeILb1ELb0ELb1ELb1EEEvNS_10StemX3ArgsE"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_asm_load_audit_of_the_quantising_stem(tmp_path):
    """The Q8 instantiation of the pipelined stem, named in full, issues its register-staged loads cleanly: no instruction
    touches an in-flight destination on any path (tools/audit_asm_loads.py, as tests/test_asm_audit.py drives it)."""
    spec = importlib.util.spec_from_file_location("audit_asm_loads", os.path.join(ROOT, "tools", "audit_asm_loads.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    out = tmp_path / "fdet_stem_x3.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                    "-S", "--cuda-device-only", os.path.join(CSRC, "fdet_stem_x3.hip"), "-o", str(out)], check=True,
                   capture_output=True, timeout=600)
    nload, bad, foreign = mod.audit(Q8_STEM, str(out), verbose=False)
    print(f"{Q8_STEM}: {nload} asm loads, {bad} touches of in-flight destinations, {foreign} compiler-issued vector-memory ops beside them")
    assert nload > 0
    assert bad == 0, mod.audit.last_touches[:4]
    # the four-parameter names keep every prefix of tests/test_asm_audit.py on the instantiation it was written for: the
    # first label a prefix matches is the <.., Q8 = false> form
    text = open(out).read()
    for prefix in ("_ZN12_GLOBAL__N_118k_stem_fwd_x3_pipeILb1ELb0ELb1E", "_ZN12_GLOBAL__N_118k_stem_fwd_x3_pipeILb1ELb0ELb0E"):
        first = next(ln for ln in text.split("\n") if ln.startswith(prefix))
        assert first.startswith(prefix + "Lb0EEEv"), first[:90]
