"""Test-time augmentation of tiled detection on the GPU (csrc/fdet_tiles.hip): fdet_tile_gather_flags against
fdet_tile_gather and its flip, fdet_tile_merge_vote against tests/tta_cpu_ref.py and against fdet_tile_merge, the limits, and
TiledDetector(flip=True, vote=True) end to end with the stored trained weights."""
import functools

import numpy as np
import pytest
import torch

import tta_cpu_ref as V

pytestmark = pytest.mark.gpu

HO = WO = 480
f32 = np.float32


def _mods():
    import fdet_amd  # noqa: F401
    from fdet_amd import hotpath, tiling
    from fdet_amd.datasets import augment
    return augment, hotpath, tiling


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ------------------------------------------------------------------------------------------------------------ gather
BANK_SIZES = [(1, 1), (479, 1), (97, 131), (300, 211), (1200, 1600)]        # (h, w); the last image ends the bank


def _images():
    g = np.random.default_rng(7)
    return [g.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in BANK_SIZES]


def _bank():
    A, _, _ = _mods()
    return A.DeviceImageBank.from_arrays(_images(), "cuda")


def _windows(Ho, Wo):
    """Per image: the whole image, a window of the frame's size (a copy) inside and flush with the far corner, one magnified
    1.5x, one reduced 3x, the last pixel, and a small window flush with the right and bottom edge - whichever fit."""
    wins = []
    for i, (h, w) in enumerate(BANK_SIZES):
        mine = [(i, 0, 0, w, h), (i, w - 1, h - 1, 1, 1), (i, w - min(w, 37), h - min(h, 29), min(w, 37), min(h, 29))]
        if w >= Wo and h >= Ho:
            mine += [(i, (w - Wo) // 3, (h - Ho) // 2, Wo, Ho), (i, w - Wo, h - Ho, Wo, Ho)]
        uw, uh = max(1, int(Wo / 1.5)), max(1, int(Ho / 1.5))
        if w >= uw and h >= uh:
            mine += [(i, (w - uw) // 2, (h - uh) // 3, uw, uh), (i, w - uw, h - uh, uw, uh)]
        if w >= 3 * Wo and h >= 3 * Ho:
            mine += [(i, 0, 0, 3 * Wo, 3 * Ho), (i, w - 3 * Wo, h - 3 * Ho, 3 * Wo, 3 * Ho)]
        wins += mine
    return wins


@pytest.mark.parametrize("hw", [(480, 480), (33, 50), (7, 5)])
def test_flagged_gather_is_the_plain_gather_and_its_flip(hw):
    """Every window twice, unflagged and flagged.  At (33, 50) and (7, 5) one block covers the frame's whole width, so the
    whole-image window of the 1200x1600 image taps far more than 32 KB of source and takes the direct global path; at
    (480, 480) every window is staged, and the windows flush with the corner of the last image make the 16-byte loads
    straddle the end of the bank."""
    _, hp, T = _mods()
    Ho, Wo = hw
    bank = _bank()
    wins = _windows(Ho, Wo)
    n = len(wins)
    assert n >= 3 * len(BANK_SIZES) + 2
    tiles = np.array(wins + wins, dtype=T.TILE_DTYPE)
    g = np.random.default_rng(1)
    first = g.integers(0, 2, n).astype(np.uint8)                             # which of the two copies is the flagged one
    flags = np.concatenate([first, 1 - first]).astype(np.uint8)
    plain = hp.tile_gather(bank.data, bank.d_table, bank.table, _dev(tiles[:n]), tiles[:n], (Ho, Wo))
    got = hp.tile_gather_flags(bank.data, bank.d_table, bank.table, _dev(tiles), tiles, _dev(flags), flags, (Ho, Wo))
    torch.cuda.synchronize()
    plain2 = torch.cat([plain, plain])
    un = torch.from_numpy(flags == 0).cuda()
    assert torch.equal(got[un], plain2[un])
    assert torch.equal(got[~un], plain2[~un].flip(-1))
    assert not torch.equal(got[~un], plain2[~un])                           # random pixels: the mirror is visible
    zeros = np.zeros(2 * n, np.uint8)                                       # all unflagged: fdet_tile_gather's bytes
    assert torch.equal(hp.tile_gather_flags(bank.data, bank.d_table, bank.table, _dev(tiles), tiles, _dev(zeros), zeros, (Ho, Wo)),
                       plain2)
    # the numpy restatement's mirrored gather on the windows of the two mid-sized images, within the bound
    # tests/test_gpu_tiles.py holds the plain gather to against the same restatement: one step, 99.9 % of the bytes equal
    imgs, host = _images(), got.cpu().numpy()
    checked = 0
    for k, w in enumerate(wins + wins):
        if w[0] in (2, 3) and flags[k]:
            d = np.abs(host[k].astype(np.int32) - V.gather(imgs[w[0]], w[1:], Ho, Wo, 1).astype(np.int32))
            assert d.max() <= 1 and (d == 0).mean() >= 0.999, (w, d.max(), (d == 0).mean())
            checked += 1
    assert checked >= 6


def test_flagged_gather_refuses_an_undefined_flag_bit_and_writes_nothing():
    _, hp, T = _mods()
    from fdet_amd import FdetError
    bank = _bank()
    tiles = np.array([(4, 0, 0, 1600, 1200), (3, 1, 2, 100, 100)], dtype=T.TILE_DTYPE)
    for bad in ([0, 2], [3, 0], [128, 1]):
        flags = np.array(bad, np.uint8)
        out = torch.full((2, 3, 33, 50), 171, dtype=torch.uint8, device="cuda")
        with pytest.raises(FdetError, match="tile_gather_flags"):
            hp.tile_gather_flags(bank.data, bank.d_table, bank.table, _dev(tiles), tiles, _dev(flags), flags, (33, 50), out)
        torch.cuda.synchronize()
        assert bool((out == 171).all()), bad


# ------------------------------------------------------------------------------------------------------------- merge
MERGE_SIZES = [(720, 960), (840, 840), (1200, 1200)]                        # (h, w): 1, 4 and 9 windows


def _merge_plan():
    _, _, T = _mods()
    tiles = [(0, 0, 0, 960, 720)]                                            # the whole image: kx = 2, ky = 1.5
    for i, L in ((1, 840), (2, 1200)):
        o = T.axis_origins(L, 480, 360)
        tiles += [(i, x0, y0, 480, 480) for y0 in o for x0 in o]
    offs = [0, 1, 5, 14]
    assert len(tiles) == 14
    return np.array(tiles, dtype=T.TILE_DTYPE), np.array(offs, np.int32)


def _cluster_rows(g, K, c):
    """c integer-valued rows in frame pixels, in clusters of 1 to 6 around random centres; members of a cluster are shifted
    along a line, so that neighbours overlap and the ends of a long cluster do not (A over B, B over C, A not over C)."""
    out = []
    while len(out) < c:
        m = int(g.integers(1, 7))
        w, h = int(g.integers(20, 80)), int(g.integers(20, 80))
        x, y = int(g.integers(-5, 440)), int(g.integers(-5, 440))
        step = int(g.integers(0, max(2, w // 3)))
        for k in range(m):
            out.append([np.round(g.uniform(0.05, 1.0) * 16) / 16, x + k * step + int(g.integers(-3, 4)), y + int(g.integers(-3, 4)),
                        w + int(g.integers(-2, 3)), h + int(g.integers(-2, 3))])
    idx = g.permutation(len(out))[:c]
    return np.array(out, f32).reshape(-1, 5)[idx]


@functools.lru_cache(maxsize=None)
def _merge_case(K):
    tiles, offs = _merge_plan()
    g = np.random.default_rng(100 + K)
    Tn = len(tiles)
    flags = g.integers(0, 2, Tn).astype(np.uint8)
    flags[[0, 1, 2]] = [1, 0, 1]                                             # both kinds in every image with several tiles
    rows = np.full((Tn, K, 5), -7.0, f32)                                    # garbage past the counts is never read
    counts = g.integers(K // 2, K + 1, Tn).astype(np.int32)
    counts[7] = 0                                                            # an empty tile
    for t in range(Tn):
        c = int(counts[t])
        rows[t, :c] = _cluster_rows(g, K, c)
    rows[3, 0, 0] = np.nan
    rows[5, 1, 0] = 0.0
    rows[9, 2, 0] = 1.5
    rows[2, 0, 0] = rows[4, 0, 0] = rows[12, 0, 0] = 0.8125                  # exact ties across tiles
    for a in (rows, counts, flags, tiles, offs):
        a.setflags(write=False)
    return rows, counts, flags, tiles, offs


@functools.lru_cache(maxsize=None)
def _merge_ref(K, margin, vote, min_votes):
    rows, counts, flags, tiles, offs = _merge_case(K)
    return V.merge_vote(rows, counts, tiles, flags, offs, MERGE_SIZES, HO, WO, margin, 0.5, 4864, vote, min_votes)


def _table(sizes):
    A, _, _ = _mods()
    table = np.zeros(len(sizes), A.IMAGE_DTYPE)
    table["h"], table["w"] = [s[0] for s in sizes], [s[1] for s in sizes]
    return _dev(table)


def _vote_gpu(rows, counts, flags, tiles, offs, sizes, margin, thr, Kout, vote, min_votes):
    _, hp, _ = _mods()
    out, votes, cnt, rej = hp.tile_merge_vote(torch.from_numpy(np.array(rows)).cuda(), torch.from_numpy(np.array(counts, np.int32)).cuda(),
                                              _dev(tiles), None if flags is None else _dev(flags),
                                              torch.from_numpy(np.array(offs, np.int32)).cuda(), _table(sizes), (HO, WO), margin, thr,
                                              Kout, vote, min_votes)
    torch.cuda.synchronize()
    return out.cpu().numpy(), votes.cpu().numpy(), cnt.cpu().numpy(), int(rej.item())


def _plain_gpu(rows, counts, tiles, offs, sizes, margin, thr, Kout):
    _, hp, _ = _mods()
    out, cnt, rej = hp.tile_merge(torch.from_numpy(np.array(rows)).cuda(), torch.from_numpy(np.array(counts, np.int32)).cuda(), _dev(tiles),
                                  torch.from_numpy(np.array(offs, np.int32)).cuda(), _table(sizes), (HO, WO), margin, thr, Kout)
    torch.cuda.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy(), int(rej.item())


def _same(got, want):
    assert got[3] == want[3] == 0
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0], want[0], equal_nan=True)


@pytest.mark.parametrize("margin", [0.0, 8.0])
@pytest.mark.parametrize("K", [8, 225])
def test_merge_vote_equals_the_restatement_and_the_plain_merge(K, margin):
    rows, counts, flags, tiles, offs = _merge_case(K)
    args = (rows, counts, flags, tiles, offs, MERGE_SIZES, margin, 0.5, 4864)
    voted = _vote_gpu(*args, True, 1)
    _same(voted, _merge_ref(K, margin, 1, 1))
    out, votes, cnt, _ = voted
    assert cnt.min() >= 1 and votes.max() >= 3                               # most keepers own several members
    assert np.mean(votes[votes > 0] >= 2) > 0.3
    for i in range(3):                                                       # rows and votes past the count are zero
        assert not out[i, cnt[i]:].any() and not votes[i, cnt[i]:].any() and (votes[i, :cnt[i]] >= 1).all()
    # vote = 0: the plain merge of the un-mirrored rows, byte for byte
    own = _vote_gpu(*args, False, 1)
    _same(own, _merge_ref(K, margin, 0, 1))
    plain = _plain_gpu(V.unmirror_rows(rows, flags, WO), counts, tiles, offs, MERGE_SIZES, margin, 0.5, 4864)
    assert plain[2] == 0 and np.array_equal(own[2], plain[1])
    assert own[0].tobytes() == plain[0].tobytes()
    # vote = 1 moves boxes only: scores, counts, member counts and the visiting order are the plain merge's
    assert np.array_equal(cnt, plain[1]) and np.array_equal(votes, own[1])
    assert out[:, :, 0].tobytes() == plain[0][:, :, 0].tobytes()
    assert not np.array_equal(out[:, :, 1:], own[0][:, :, 1:])               # and it does move some
    # min_votes = 2: the survivors with at least two members, in order
    two = _vote_gpu(*args, True, 2)
    _same(two, _merge_ref(K, margin, 1, 2))
    assert 0 < two[2].sum() < cnt.sum()
    for i in range(3):
        sel = votes[i, :cnt[i]] >= 2
        k = int(sel.sum())
        assert two[2][i] == k
        assert np.array_equal(two[0][i, :k], out[i, :cnt[i]][sel], equal_nan=True) and np.array_equal(two[1][i, :k], votes[i, :cnt[i]][sel])
        assert not two[0][i, k:].any() and not two[1][i, k:].any()


def test_merge_vote_without_flags_is_the_plain_merge():
    rows, counts, _, tiles, offs = _merge_case(8)
    own = _vote_gpu(rows, counts, None, tiles, offs, MERGE_SIZES, 8.0, 0.5, 4864, False, 1)
    plain = _plain_gpu(rows, counts, tiles, offs, MERGE_SIZES, 8.0, 0.5, 4864)
    assert own[3] == plain[2] == 0 and np.array_equal(own[2], plain[1]) and own[0].tobytes() == plain[0].tobytes()


# ------------------------------------------------------------------------------------------------------------ limits
@functools.lru_cache(maxsize=None)
def _limit_case():
    """Image 1 owns 20 windows of K = 256 rows: 19 full ones are exactly 4864 candidates, the 20th holds the one too many."""
    _, _, T = _mods()
    K = 256
    o = T.axis_origins(1200, 480, 360)
    nine = [(1, x0, y0, 480, 480) for y0 in o for x0 in o]
    tiles = np.array([(0, 0, 0, 480, 480)] + nine + nine + [(1, 0, 0, 480, 480), (1, 720, 720, 480, 480)] + [(2, 0, 0, 480, 480)],
                     dtype=T.TILE_DTYPE)
    offs = np.array([0, 1, 21, 22], np.int32)
    flags = np.array([0] + [0] * 9 + [1] * 9 + [1, 0] + [1], np.uint8)
    g = np.random.default_rng(11)
    rows = np.zeros((22, K, 5), f32)
    rows[:, :, 0] = np.round(g.uniform(0.05, 1.0, (22, K)) * 64) / 64
    rows[:, :, 1:3] = g.integers(0, 450, (22, K, 2))
    rows[:, :, 3:] = g.integers(8, 40, (22, K, 2))
    counts = np.array([40] + [K] * 19 + [0] + [60], np.int32)
    return rows, counts, flags, tiles, offs, [(480, 480), (1200, 1200), (480, 480)]


def test_merge_vote_limits_reject_whole_images():
    rows, counts, flags, tiles, offs, sizes = _limit_case()
    assert int(counts[1:21].sum()) == 4864 == V.MAX_CANDIDATES
    want = V.merge_vote(rows, counts, tiles, flags, offs, sizes, HO, WO, 0.0, 0.5, 4864, 1, 1)
    got = _vote_gpu(rows, counts, flags, tiles, offs, sizes, 0.0, 0.5, 4864, True, 1)
    _same(got, want)                                                         # exactly at the limit: accepted
    assert got[2].min() >= 2 and int(got[1][1].sum()) == 4864                # every candidate is owned exactly once
    # one candidate more: image 1 is rejected as a whole, the others are intact
    more = counts.copy()
    more[20] = 1
    over = _vote_gpu(rows, more, flags, tiles, offs, sizes, 0.0, 0.5, 4864, True, 1)
    assert over[3] == 1 and over[2].tolist() == [got[2][0], 0, got[2][2]]
    assert not over[0][1].any() and not over[1][1].any()
    for i in (0, 2):
        assert np.array_equal(over[0][i], got[0][i]) and np.array_equal(over[1][i], got[1][i])
    assert V.merge_vote(rows, more, tiles, flags, offs, sizes, HO, WO, 0.0, 0.5, 4864, 1, 1)[3] == 1
    # room for one survivor fewer than image 1 has: rejected as a whole, nothing truncated
    k1 = int(got[2][1])
    assert k1 > max(int(got[2][0]), int(got[2][2]))
    small = _vote_gpu(rows, counts, flags, tiles, offs, sizes, 0.0, 0.5, k1 - 1, True, 1)
    assert small[3] == 1 and small[2].tolist() == [got[2][0], 0, got[2][2]]
    assert not small[0][1].any() and not small[1][1].any()
    for i in (0, 2):
        assert np.array_equal(small[0][i], got[0][i, :k1 - 1]) and np.array_equal(small[1][i], got[1][i, :k1 - 1])
    exact = _vote_gpu(rows, counts, flags, tiles, offs, sizes, 0.0, 0.5, k1, True, 1)
    assert exact[3] == 0 and exact[2].tolist() == got[2].tolist()


# ------------------------------------------------------------------------------------------------------- end to end
QUADS = [0, 1, 2, 0]                                                        # as tests/test_gpu_tiles.py: a 960x960 mosaic
ORIGINS = [(0, 0), (480, 0), (0, 480), (480, 480)]


def _trained(golden):
    from fdet_amd.models.PoolResnet import PoolResnet
    g = golden("g6_trained_small")
    P = {k[len("param/"):]: v for k, v in g.items() if k.startswith("param/")}
    model = PoolResnet(filters=32, input_shape=(3, 480, 480), num_of_patches=10, probability_threshold=0.7, iou_threshold=0.01)
    model.load_state_dict({k: v.clone() for k, v in P.items()})
    return model.cuda().eval()


def _mosaic(golden):
    A, _, _ = _mods()
    images = golden("g6_trained_small")["images"].numpy()
    src = np.zeros((960, 960, 3), np.uint8)
    for q, (x0, y0) in zip(QUADS, ORIGINS):
        src[y0:y0 + 480, x0:x0 + 480] = images[q].transpose(1, 2, 0)
    return A.DeviceImageBank.from_arrays([src], "cuda")


def test_detect_with_flip_and_vote_equals_the_restatement_on_independent_rows(golden, monkeypatch):
    _, hp, T = _mods()
    from fdet_amd.evaluation import DetectionEvaluator
    model = _trained(golden)
    bank = _mosaic(golden)
    kw = dict(tile_sizes=(480,), overlap=0.0, include_whole=False)
    plan = T.plan_tiles(bank.sizes, **kw)
    assert [tuple(t)[1:3] for t in plan.tiles] == ORIGINS
    red = model.reduce_bounding_boxes
    # the rows, independently: the plain gather, torch.flip for the second half, the network, the reducer
    with torch.no_grad():
        frames = hp.tile_gather(bank.data, bank.d_table, bank.table, _dev(plan.tiles), plan.tiles, (HO, WO))
        r, c = red.forward_batch(model.forward_frames(torch.cat([frames, torch.flip(frames, dims=(-1,))])))
    rows, counts = r.cpu().numpy(), c.cpu().numpy()
    assert counts[:4].sum() >= 2 and counts[4:].sum() >= 1                  # both passes detect something
    tiles2 = [tuple(int(v) for v in t) for t in plan.tiles] * 2
    flags = [0] * 4 + [1] * 4
    gathers = []
    for name in ("tile_gather", "tile_gather_flags"):
        orig = getattr(hp, name)
        monkeypatch.setattr(hp, name, lambda *a, _o=orig, _n=name, **k: (gathers.append(_n), _o(*a, **k))[1])
    # both ways tiling has of making the mirrored frames: the flagged gather, or the plain gather and a flip of the flagged frames
    both = torch.cat([frames, torch.flip(frames, dims=(-1,))])
    for flagged_gather in (True, False):                 # network calls of 3 frames cut through the run of flagged frames
        monkeypatch.setattr(T, "FLAGGED_GATHER_MEASURED_FASTER", flagged_gather)
        det = T.TiledDetector(model, flip=True, vote=True, max_frames=3, **kw)
        fed = []
        monkeypatch.setattr(det, "_maps", lambda fr, _m=det._maps: (fed.append(fr.clone()), _m(fr))[1])
        del gathers[:]
        det.detect(bank, [0])
        assert gathers == ["tile_gather_flags" if flagged_gather else "tile_gather"] * 3
        assert [int(f.shape[0]) for f in fed] == [3, 3, 2] and torch.equal(torch.cat(fed), both)
    for vote, min_votes, flagged_gather in ((True, 1, True), (True, 1, False), (False, 1, True), (False, 1, False), (True, 2, True)):
        want = V.merge_vote(rows, counts, tiles2, flags, [0, 8], [(960, 960)], HO, WO, 0.0, 0.01, 4864, int(vote), min_votes)
        monkeypatch.setattr(T, "FLAGGED_GATHER_MEASURED_FASTER", flagged_gather)
        det = T.TiledDetector(model, flip=True, vote=vote, min_votes=min_votes, **kw)
        del gathers[:]
        out, cnt = det.detect(bank, [0])
        assert gathers == ["tile_gather_flags" if flagged_gather else "tile_gather"]
        assert want[3] == 0 and tuple(out.shape) == (1, 4864, 5) and tuple(det.last_votes.shape) == (1, 4864)
        assert det.last_votes.dtype == torch.int32 and cnt.dtype == torch.int32
        assert np.array_equal(cnt.cpu().numpy(), want[2]) and np.array_equal(det.last_votes.cpu().numpy(), want[1])
        assert np.array_equal(out.cpu().numpy(), want[0])
        if (vote, min_votes) == (True, 1):
            k = int(cnt[0])
            assert k >= 2
            ev = DetectionEvaluator()                                        # the voted rows are rows like any other
            gt = out[0, :k].clone()
            gt[:, 0] = 1.0
            ev.update(out, cnt, [gt])
            res = ev.compute()
            assert res.ap == 1.0 and (res.n_gt, res.n_images, res.n_det) == (k, 1, k)
    monkeypatch.undo()
    # vote without flip: the plain plan through the vote entry
    det = T.TiledDetector(model, vote=True, **kw)
    out, cnt = det.detect(bank, [0])
    want = V.merge_vote(rows[:4], counts[:4], tiles2[:4], None, [0, 4], [(960, 960)], HO, WO, 0.0, 0.01, 4864, 1, 1)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(det.last_votes.cpu().numpy(), want[1])
    # the flagged gather gives the frames the independent rows came from
    tiles8 = np.concatenate([plan.tiles, plan.tiles])
    f8 = np.array(flags, np.uint8)
    got = hp.tile_gather_flags(bank.data, bank.d_table, bank.table, _dev(tiles8), tiles8, _dev(f8), f8, (HO, WO))
    assert torch.equal(got, torch.cat([frames, torch.flip(frames, dims=(-1,))]))


def test_default_detect_calls_the_old_entries_and_returns_their_bytes(golden, monkeypatch):
    _, hp, T = _mods()
    model = _trained(golden)
    bank = _mosaic(golden)
    kw = dict(tile_sizes=(480,), overlap=0.25, include_whole=True, edge_margin=4.0)
    plan = T.plan_tiles(bank.sizes, (480,), 0.25, True)
    red = model.reduce_bounding_boxes
    with torch.no_grad():
        frames = hp.tile_gather(bank.data, bank.d_table, bank.table, _dev(plan.tiles), plan.tiles, (HO, WO))
        r, c = red.forward_batch(model.forward_frames(frames))
        want = hp.tile_merge(r, c, _dev(plan.tiles), torch.from_numpy(plan.tile_offset).cuda(), bank.d_table, (HO, WO), 4.0, 0.01, 4864)
    called = []
    for name in ("tile_gather", "tile_merge", "tile_gather_flags", "tile_merge_vote"):
        orig = getattr(hp, name)
        monkeypatch.setattr(hp, name, lambda *a, _o=orig, _n=name, **k: (called.append(_n), _o(*a, **k))[1])
    det = T.TiledDetector(model, **kw)
    out, cnt = det.detect(bank, [0])
    assert sorted(set(called)) == ["tile_gather", "tile_merge"] and det.last_votes is None
    assert int(cnt[0]) >= 2 and torch.equal(cnt, want[1]) and torch.equal(out, want[0])
