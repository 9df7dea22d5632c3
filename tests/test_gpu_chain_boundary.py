"""GPU tests of the PS block chain (fdet_block_chain_{fwd,bwd}_ps) at its layer boundary: what one layer hands to the next
(group 0 at once, groups 1..3 behind the next layer's MFMAs) for first, last, odd and even layers, a single block, pad
positions in every wave (5x5, 7x3) and an empty last wave, with and without dropout scales, in bf16x3 and precision16.

Reference: float64 torch CPU of plain conv, LeakyReLU, scale and add, staged the way the kernels see their operands
(bf16x3: the input as its PS tensor holds it; precision16: every conv operand rounded to bf16, the skip sum kept unrounded).
Bounds are the ones the chain already has: 1e-4 of the tensor's scale in bf16x3 (tests/test_gpu_ps.py), 1e-2 of the scale in
precision16 (tests/test_gpu_p16.py, test_p16_block_chain_forward: a rounding that falls the other way moves a later
activation by one bf16 ulp).  The hi plane of c is a bf16 truncation or rounding of c: 2^-8 of the value on top of that."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C = 64
SLOPE = 0.2


@pytest.fixture(scope="module")
def env():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, ps
    return hotpath, ps


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def close(got, ref, tol, what):
    got = got.cpu().double(); ref = ref.cpu().double()
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"{what}: max err {err:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err} vs scale {scale}"


def _lrelu_d(v):
    return torch.where(v > 0, 1.0, SLOPE).double()


def _reference(x0, Ws, scales, dout, rnd):
    """float64 forward and backward of the chain; `rnd` rounds a conv operand (identity or bf16)."""
    nb = len(Ws)
    r = lambda t: rnd(t.float()).double()
    h = x0.double()
    a_ref, c_ref, o_ref = [], [], []
    for k in range(nb):
        w1, b1, w2, b2 = Ws[k]
        a = F.leaky_relu(F.conv2d(r(h), r(w1), b1.double(), padding=1), SLOPE)
        c = F.leaky_relu(F.conv2d(r(a), r(w2), b2.double(), padding=1), SLOPE)
        h = (c * scales[k][:, :, None, None].double() if scales is not None else c) + h
        a_ref.append(a); c_ref.append(c); o_ref.append(h)
    g = dout.double()
    dz1 = [None] * nb; dz2 = [None] * nb
    for k in range(nb - 1, -1, -1):
        w1, _, w2, _ = Ws[k]
        z2 = g * _lrelu_d(c_ref[k])
        if scales is not None:
            z2 = z2 * scales[k][:, :, None, None].double()
        z1 = F.conv_transpose2d(r(z2), r(w2), padding=1) * _lrelu_d(a_ref[k])
        g = F.conv_transpose2d(r(z1), r(w1), padding=1) + g
        dz1[k] = z1; dz2[k] = z2
    return a_ref, c_ref, o_ref, dz1, dz2, g


def _setup(hp, ps, N, H, W, nb, use_scale, p16, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    Ws = [(torch.randn(C, C, 3, 3, generator=g) * 0.05, torch.randn(C, generator=g) * 0.1,
           torch.randn(C, C, 3, 3, generator=g) * 0.05, torch.randn(C, generator=g) * 0.1) for _ in range(nb)]
    scales = [((torch.rand(N, C, generator=g) > 0.25).float() / 0.75) for _ in range(nb)] if use_scale else None
    dout = torch.randn(N, C, H, W, generator=g)
    x_ps = ps.PsTensor.from_f32((bf(x) if p16 else x).cuda())
    x0 = x_ps.to_f32().cpu()                                  # the input as its PS tensor holds it
    nf, nbk = hp.packed_sizes(C, C)
    wf1, wb1, wf2, wb2 = [], [], [], []
    for (w1, _, w2, _) in Ws:
        for w, lf, lb in ((w1, wf1, wb1), (w2, wf2, wb2)):
            f_ = torch.empty(nf, device="cuda"); b_ = torch.empty(nbk, device="cuda")
            hp.pack_conv3x3_weights(w.cuda(), f_, b_, x3=True)
            lf.append(f_); lb.append(b_)
    dev = dict(x_ps=x_ps, wf1=wf1, wb1=wb1, wf2=wf2, wb2=wb2, b1=[w[1].cuda() for w in Ws], b2=[w[3].cuda() for w in Ws],
               sc=[s.cuda() for s in scales] if use_scale else None, dout=dout.cuda())
    ref = _reference(x0, Ws, scales, dout, bf if p16 else (lambda t: t))
    return dev, ref


def _mkps(ps, n, N, H, W):
    return [ps.PsTensor(N, C, H, W, "cuda") for _ in range(n)]


def _nan(N, H, W):
    return torch.full((N, C, H, W), float("nan"), device="cuda")


def _run_fwd(ps, d, N, H, W, nb, p16, bufs=None):
    a_p, c_p, o_p = bufs if bufs is not None else (_mkps(ps, nb, N, H, W), _mkps(ps, nb, N, H, W), _mkps(ps, nb - 1, N, H, W))
    last = _nan(N, H, W)
    ps.block_chain_fwd_ps(d["x_ps"], d["wf1"], d["b1"], d["wf2"], d["b2"], d["sc"], a_p[:nb], c_p[:nb], o_p[:nb - 1], last,
                          slope=SLOPE, p16=p16)
    return a_p, c_p, o_p, last


def _run_bwd(ps, d, a_t, c_t, N, H, W, nb, p16, bufs=None):
    z1, z2 = bufs if bufs is not None else (_mkps(ps, nb, N, H, W), _mkps(ps, nb, N, H, W))
    dx = _nan(N, H, W)
    ps.block_chain_bwd_ps(d["dout"], d["wb1"], d["wb2"], d["sc"], a_t, c_t, z1[:nb], z2[:nb], dx, slope=SLOPE, p16=p16)
    return z1, z2, dx


def _outside(ps, N, H, W):
    real = ps.PsTensor.from_f32(torch.full((N, C, H, W), 1.0 + 2.0 ** -9, device="cuda"))
    return real.buf.view(torch.int16) == 0


@pytest.mark.parametrize("p16", [False, True], ids=["bf16x3", "p16"])
@pytest.mark.parametrize("nb", [1, 2, 3])
@pytest.mark.parametrize("hw", [(15, 15), (5, 5), (7, 3)])
@pytest.mark.parametrize("N", [1, 3])
def test_chain_boundary_against_float64(env, N, hw, nb, p16):
    hp, ps = env
    H, W = hw
    tol = 1e-2 if p16 else 1e-4
    outside = _outside(ps, N, H, W)
    for use_scale in (True, False):
        d, (a_ref, c_ref, o_ref, dz1_ref, dz2_ref, dx_ref) = _setup(hp, ps, N, H, W, nb, use_scale, p16, N * 1000 + H * 10 + W + nb)
        tag = f"N{N} {H}x{W} nb{nb} scale{int(use_scale)} {'p16' if p16 else 'x3'}"
        # training flavour: a, the hi plane of c, the block outputs, the chain output
        a_p, c_p, o_p, last = _run_fwd(ps, d, N, H, W, nb, p16)
        close(last, o_ref[-1], tol, f"{tag} out")
        for k in range(nb):
            close(a_p[k].to_f32(), a_ref[k], tol, f"{tag} a[{k}]")
            chi = c_p[k].to_f32().cpu().double()
            cscale = max(1.0, float(c_ref[k].abs().max()))
            assert bool(((chi - c_ref[k]).abs() <= c_ref[k].abs() * 2.0 ** -8 + tol * cscale).all()), f"{tag} c[{k}] hi plane"
            firm = c_ref[k].abs() > 10 * tol * cscale
            assert torch.equal((chi > 0)[firm], (c_ref[k] > 0)[firm]), f"{tag} c[{k}] signs"
            assert torch.equal(chi.float(), bf(chi.float())), f"{tag} c[{k}]: lo plane written"
            if k + 1 < nb:
                close(o_p[k].to_f32(), o_ref[k], tol, f"{tag} out[{k}]")
            if p16:
                for t in [a_p[k]] + ([o_p[k]] if k + 1 < nb else []):
                    v = t.to_f32().cpu()
                    assert torch.equal(v, bf(v)), f"{tag}: precision16 wrote a lo plane"
        for t in a_p + c_p + o_p:
            assert int((t.buf.view(torch.int16)[outside] != 0).sum()) == 0, f"{tag}: write outside the real elements"
        # eval flavour: nothing kept, the same chain output
        last_e = _nan(N, H, W)
        ps.block_chain_fwd_ps(d["x_ps"], d["wf1"], d["b1"], d["wf2"], d["b2"], d["sc"], None, None, None, last_e, slope=SLOPE, p16=p16)
        assert torch.equal(last_e, last), f"{tag}: eval flavour differs"
        # backward on the reference's activations (a device a / c within rounding of zero may carry the other sign)
        rnd = bf if p16 else (lambda t: t)
        a_t = [ps.PsTensor.from_f32(rnd(t.float()).cuda()) for t in a_ref]
        c_t = [ps.PsTensor.from_f32(rnd(t.float()).cuda()) for t in c_ref]
        z1, z2, dx = _run_bwd(ps, d, a_t, c_t, N, H, W, nb, p16)
        close(dx, dx_ref, tol, f"{tag} dx")
        for k in range(nb):
            close(z1[k].to_f32(), dz1_ref[k], tol, f"{tag} dz1[{k}]")
            close(z2[k].to_f32(), dz2_ref[k], tol, f"{tag} dz2[{k}]")
        for t in z1 + z2:
            assert int((t.buf.view(torch.int16)[outside] != 0).sum()) == 0, f"{tag}: write outside the real elements"


def _bits(ts):
    return [t.buf.view(torch.int32).clone() for t in ts]


@pytest.mark.parametrize("p16", [False, True], ids=["bf16x3", "p16"])
def test_chain_boundary_no_job_left_pending(env, p16):
    """A deferred job belongs to one layer of one launch: the chain twice on recycled buffers, then one block directly after
    three on the same buffers, must give what fresh buffers give, bit for bit."""
    hp, ps = env
    N, H, W = 3, 15, 15
    d3, ref3 = _setup(hp, ps, N, H, W, 3, True, p16, 31)
    d1, ref1 = _setup(hp, ps, N, H, W, 1, True, p16, 32)
    rnd = bf if p16 else (lambda t: t)
    acts = lambda ref: ([ps.PsTensor.from_f32(rnd(t.float()).cuda()) for t in ref[0]], [ps.PsTensor.from_f32(rnd(t.float()).cuda()) for t in ref[1]])
    # fresh buffers
    f3 = _run_fwd(ps, d3, N, H, W, 3, p16); b3 = _run_bwd(ps, d3, *acts(ref3), N, H, W, 3, p16)
    f1 = _run_fwd(ps, d1, N, H, W, 1, p16); b1 = _run_bwd(ps, d1, *acts(ref1), N, H, W, 1, p16)
    want3 = _bits(f3[0] + f3[1] + f3[2]) + [f3[3].clone()] + _bits(b3[0] + b3[1]) + [b3[2].clone()]
    want1 = _bits(f1[0] + f1[1]) + [f1[3].clone()] + _bits(b1[0] + b1[1]) + [b1[2].clone()]
    # the three-block chain again into the buffers it has just filled
    g3 = _run_fwd(ps, d3, N, H, W, 3, p16, bufs=f3[:3]); c3 = _run_bwd(ps, d3, *acts(ref3), N, H, W, 3, p16, bufs=b3[:2])
    got3 = _bits(g3[0] + g3[1] + g3[2]) + [g3[3]] + _bits(c3[0] + c3[1]) + [c3[2]]
    assert all(torch.equal(u, v) for u, v in zip(got3, want3)), "second run on recycled buffers differs"
    # one block directly after three, into the first block's buffers of that run
    g1 = _run_fwd(ps, d1, N, H, W, 1, p16, bufs=f3[:3]); c1 = _run_bwd(ps, d1, *acts(ref1), N, H, W, 1, p16, bufs=b3[:2])
    got1 = _bits(g1[0][:1] + g1[1][:1]) + [g1[3]] + _bits(c1[0][:1] + c1[1][:1]) + [c1[2]]
    assert all(torch.equal(u, v) for u, v in zip(got1, want1)), "one block after three differs from one block alone"
    # ... and the buffers of blocks 1, 2 were left alone by the one-block launch
    # (want3 holds a[3], c[3], out[2], last, dz1[3], dz2[3], dx)
    kept = want3[1:3] + want3[4:6] + want3[10:12] + want3[13:15]
    assert all(torch.equal(u, v) for u, v in zip(_bits(g1[0][1:] + g1[1][1:] + c1[0][1:] + c1[1][1:]), kept)), "a later block's buffer was touched"
