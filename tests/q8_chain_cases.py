"""Cases of the int8 chain kernel (fdet_q8_chain) and their restatement: a loop over tests/q8_cpu_ref.py's `block`.  Shared by
tests/test_q8_chain_host.py (conditions on the data) and tests/test_gpu_q8_chain.py (equality on the GPU)."""
import functools

import numpy as np

import q8_cpu_ref as R

F32 = np.float32
C = 64

# (N, H, W, nblocks): a map that is all halo; the real depth (8 blocks: both parities of the weight double buffer, many times);
# a full 16-pixel row with no masked lane; non-square maps; single rows and columns; odd image counts; more images than a
# launch has workgroups (one per CU); a single block
CHAIN_CASES = [(1, 1, 1, 2), (3, 15, 15, 8), (2, 16, 16, 3), (2, 5, 16, 2), (5, 10, 10, 3), (600, 4, 4, 1), (1, 16, 1, 2),
               (1, 1, 16, 2), (2, 15, 15, 1)]
CHAIN_IDS = ["x".join(str(v) for v in c) for c in CHAIN_CASES]
TIES_CASE = (1, 4, 4, 2)


def _conv(rng):
    w = rng.integers(-127, 128, (C, C, 3, 3)).astype(np.int8)
    b = rng.integers(-40000, 40001, C).astype(np.int32)
    mul = np.exp2(rng.uniform(-12.3, -10.8, C)).astype(F32)
    return w, b, mul


@functools.lru_cache(maxsize=None)
def make_chain_case(i):
    """x over the full range -127..127 with both ends planted; per conv full-range int8 weights, biases in +-40000 and
    per-channel multipliers 2^-12.3 .. 2^-10.8 (log-uniform); skip_mul 0.75."""
    N, H, W, nb = CHAIN_CASES[i]
    rng = np.random.default_rng(2000 + i)
    x = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8)
    x.reshape(-1)[:2] = (127, -127)
    blocks = [(_conv(rng), _conv(rng)) for _ in range(nb)]
    return dict(shape=(N, C, H, W), x=x, blocks=blocks, skip_mul=[F32(0.75)] * nb, slope=R.SLOPE)


@functools.lru_cache(maxsize=None)
def make_ties_case():
    """The "ties" construction of q8_cpu_ref.make_case on a chain: sparse weights of -1 / 0 / 1, multipliers 0.5, skip_mul 0.5,
    small biases -- every odd accumulator (first conv) and every odd acc + skip (second conv) sits exactly on .5.  The
    sparsity keeps |acc| / 2 mostly inside the int8 range, so the ties are rounded, not clamped away."""
    N, H, W, nb = TIES_CASE
    rng = np.random.default_rng(2100)
    x = rng.integers(-127, 128, (N, C, H, W)).astype(np.int8)
    x.reshape(-1)[:2] = (127, -127)

    def conv():
        w = (rng.integers(-1, 2, (C, C, 3, 3)) * (rng.random((C, C, 3, 3)) < 0.005)).astype(np.int8)
        return w, rng.integers(-9, 10, C).astype(np.int32), np.full(C, 0.5, F32)
    blocks = [(conv(), conv()) for _ in range(nb)]
    return dict(shape=(N, C, H, W), x=x, blocks=blocks, skip_mul=[F32(0.5)] * nb, slope=R.SLOPE)


def restate(d):
    """-> [(a_k, h_{k+1})] of every block: q8_cpu_ref.block, un-pooled, one after the other."""
    h, out = d["x"], []
    for (c1, c2), sm in zip(d["blocks"], d["skip_mul"]):
        a, h = R.block(h, c1, c2, sm, pool=False, slope=d["slope"])
        out.append((a, h))
    return out


@functools.lru_cache(maxsize=None)
def chain_ref(i):
    return restate(make_chain_case(i))


def pre_rounding(d):
    """The float32 values before rint of every conv of the chain (for the share of exact ties)."""
    h, out = d["x"], []
    for (c1, c2), sm in zip(d["blocks"], d["skip_mul"]):
        t1 = R.epilogue_float(R.conv_acc(h, c1[0], c1[1]), c1[2], slope=d["slope"])
        a = R.rint_clamp(t1)
        t2 = R.epilogue_float(R.conv_acc(a, c2[0], c2[1]), c2[2], h, sm, slope=d["slope"])
        h = R.rint_clamp(t2)
        out += [t1, t2]
    return out
