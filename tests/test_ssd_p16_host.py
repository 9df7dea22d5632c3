"""precision16 for the SSD engine, host side (no GPU):

* the one-pass pointwise GEMM entries (fdet_pointwise_{fwd,dgrad,wgrad}_bf16) are declared in include/fdet.h, listed in the
  ctypes table with the arguments of their _bf16x3 twins, and exported by the built library;
* hotpath.pointwise_{fwd,dgrad,wgrad} take `p16` (default off);
* SSDStack.set_precision accepts "bf16" / "bf16x3" and nothing else; FDET_PRECISION=bf16 selects precision16 when the
  engine is built, unset does not;
* train_model_ssd's parser carries the reference recipe's defaults (train_model_ssd.py:13-15,48-55).
"""
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PW_ENTRIES = ["fdet_pointwise_fwd_bf16", "fdet_pointwise_dgrad_bf16", "fdet_pointwise_wgrad_bf16"]


def _native():
    import fdet_amd  # noqa: F401
    from fdet_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native


def test_one_pass_pointwise_entries_are_declared_tabled_and_exported():
    N = _native()
    declared = set(N.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in PW_ENTRIES:
        assert name in declared, f"{name} not declared in include/fdet.h"
        assert name in N.SIGNATURES, f"{name} missing from the ctypes table"
        assert name in exported, f"{name} not exported by {os.path.basename(N.LIB_PATH)}"
        twin = name + "x3"
        assert N.SIGNATURES[name] == N.SIGNATURES[twin], f"{name}: arguments differ from {twin}"


def test_hotpath_pointwise_takes_p16():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath as hp
    for fn in (hp.pointwise_fwd, hp.pointwise_dgrad, hp.pointwise_wgrad):
        prm = inspect.signature(fn).parameters
        assert "p16" in prm and prm["p16"].default is False, fn.__name__


def test_ssdstack_set_precision(monkeypatch):
    import fdet_amd  # noqa: F401
    from fdet_amd.ssdstack import SSDStack
    monkeypatch.delenv("FDET_PRECISION", raising=False)
    eng = SSDStack(16)
    assert eng.p16 is False
    eng.set_precision("bf16")
    assert eng.p16 is True
    eng.set_precision("bf16x3")
    assert eng.p16 is False
    for bad in ("fp16", "f32", "BF16", "", None):
        with pytest.raises(ValueError):
            eng.set_precision(bad)
    assert eng.p16 is False


@pytest.mark.parametrize("env_val,want", [("bf16", "P16 1"), (None, "P16 0"), ("bf16x3", "P16 0"), ("f32", "P16 0")])
def test_fdet_precision_env_selects_p16_for_ssd(env_val, want):
    code = ("import fdet_amd\nfrom fdet_amd.models.SSD import SSD\n"
            "e = SSD(filters=16, input_shape=(3, 480, 480)).engine\n"
            "print('P16', int(e.p16))\n")
    env = dict(os.environ)
    env.pop("FDET_PRECISION", None)
    if env_val is not None:
        env["FDET_PRECISION"] = env_val
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert want in r.stdout, (env_val, r.stdout)


def test_train_model_ssd_parser_has_reference_defaults():
    import fdet_amd  # noqa: F401
    from fdet_amd import train_model_ssd
    a = train_model_ssd.parser().parse_args([])
    assert (a.filters, a.size, a.lr, a.epochs, a.batch_size) == (16, 480, 1e-4, 70, 24)
    assert a.precision == 32 and a.save is None
    assert a.steps_per_epoch > 0 and a.val_steps > 0
    assert train_model_ssd.parser().parse_args(["--precision", "16"]).precision == 16
    with pytest.raises(SystemExit):
        train_model_ssd.parser().parse_args(["--precision", "8"])
