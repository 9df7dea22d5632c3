"""Child process of tests/test_gpu_ps_pool_wg2.py: the launcher reads FDET_PS_POOL_WG2 once per process, so each form of the
pooled forward (0 = one workgroup per CU with two chunk buffers, 1 = two workgroups per CU with one) runs in a process
of its own.  Runs every case twice on the same buffers and saves what the parent compares.

    FDET_PS_POOL_WG2=<0|1> python tests/ps_pool_wg2_worker.py <out.pt>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch

# (N, C, H, W).  60x60 / 30x30: the two levels of the headline model (64- and 32-slot rows); the short maps of the
# existing pooled-block test (bands that run across images; nine images); one image of two tiles (fewer tiles than any
# grid); 15 tiles (odd, not a multiple of 8: the plain walk and an uneven last round); 80 columns = two column strips.
SHAPES = [(3, 64, 60, 60), (5, 64, 30, 30), (2, 64, 12, 56), (9, 64, 16, 30), (1, 64, 30, 30), (5, 64, 22, 40), (2, 64, 12, 80)]
SENTINEL = 0xA5


def case_inputs(shape, train):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(N * 31 + H + W + int(train))
    x = torch.randn(N, C, H, W, generator=g)
    skip = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * 0.1
    b = torch.randn(C, generator=g)
    scale = (torch.rand(N, C, generator=g) > 0.25).float() / 0.75 if train else None
    return x, skip, w, b, scale


def run_case(shape, train):
    from fdet_amd import hotpath as hp, ps
    N, C, H, W = shape
    x, skip, w, b, scale = case_inputs(shape, train)
    nf, nb = hp.packed_sizes(C, C)
    wf = torch.empty(nf, device="cuda"); wb = torch.empty(nb, device="cuda")
    hp.pack_conv3x3_weights(w.cuda(), wf, wb, x3=True)
    xp = ps.PsTensor.from_f32(x.cuda()); sp = ps.PsTensor.from_f32(skip.cuda())
    strips = xp.strips > 1
    pool_ps = None if strips else ps.PsTensor(N, C, H // 2, W // 2, "cuda")          # zeroed: its halo slots must stay zero
    pool_f = torch.full((N, C, H // 2, W // 2), float("nan"), device="cuda")
    route = ps.route8_like(N, C, H, W, "cuda").fill_(SENTINEL) if train else None
    sc = scale.cuda() if train else None
    bc = b.cuda()

    def snap():
        torch.cuda.synchronize()
        return {"pool_f": pool_f.cpu().clone(), "pool_ps_buf": None if strips else pool_ps.buf.cpu().clone(),
                "pool_ps": None if strips else pool_ps.to_f32().cpu(), "route": route.cpu().clone() if train else None}

    ps.conv3x3_ps_fwd_pool(xp, wf, bc, sp, sc, pool_ps, pool_f, route)
    first = snap()
    ps.conv3x3_ps_fwd_pool(xp, wf, bc, sp, sc, pool_ps, pool_f, route)                 # the same, recycled buffers
    second = snap()
    first["repeat_equal"] = all(
        (first[k] is None and second[k] is None) or torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8))
        for k in ("pool_f", "pool_ps_buf", "route"))
    first["xr"] = xp.to_f32().cpu(); first["sr"] = sp.to_f32().cpu()
    # one output kind at a time (the store count behind the DMA differs: pool_cnt in the kernel)
    only_f = torch.full_like(pool_f, float("nan"))
    ps.conv3x3_ps_fwd_pool(xp, wf, bc, sp, sc, None, only_f, route)
    first["only_f"] = only_f.cpu()
    if not strips:
        # the 16-bit words of the pooled PS buffer that belong to real elements: 1 + 2^-10 has a non-zero hi AND lo part
        full = ps.PsTensor.from_f32(torch.full((N, C, H // 2, W // 2), 1.0 + 2.0 ** -10, device="cuda"))
        first["real_words"] = (full.buf.view(torch.int16) != 0).cpu()
        only_ps = ps.PsTensor(N, C, H // 2, W // 2, "cuda")
        ps.conv3x3_ps_fwd_pool(xp, wf, bc, sp, sc, only_ps, None, None)
        first["only_ps_buf"] = only_ps.buf.cpu()
    return first


def train_two_steps():
    """Two fused training steps of the headline model at batch 3 (as __graft_entry__.smoke builds it) -> every parameter."""
    import oracle as O
    from fdet_amd.models import ModelMeta
    from fdet_amd.models.PoolResnet import PoolResnet
    F_, S, size, B = 64, 10, 480, 3
    spec = O.poolresnet_spec(F_, (3, size, size), S)
    P = O.init_params(spec, seed=0)
    model = PoolResnet(F_, (3, size, size), S)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    model = model.cuda().train()
    mm = ModelMeta(model=model, lr=1e-4)
    mm.configure_optimizers()
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(0)).cuda()
    y = torch.stack([O.encode_targets(b, (size, size), S) for b in O.synthetic_boxes(B, size, seed=1)]).cuda()
    model.set_dropout_masks(O.make_dropout_masks(spec, B, seed=2))
    losses = []
    for _ in range(2):
        lsum, _, _ = mm.fused_train_step(x, y)
        losses.append(float(lsum))
    torch.cuda.synchronize()
    return {"losses": losses, "params": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}}


def main(out_path):
    torch.cuda.set_device(0)
    res = {"wg2": os.environ.get("FDET_PS_POOL_WG2"), "cases": {}}
    for shape in SHAPES:
        for train in (True, False):
            res["cases"][(shape, train)] = run_case(shape, train)
    res["train"] = train_two_steps()
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
