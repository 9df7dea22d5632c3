"""The shape list of tests/test_gpu_stem_paths.py against the routes the library builds (no GPU): every
(family, pass, precision16, uint8, PS) combination has a case -- switch groups included --, every family has a case
with a bottom pad, a right pad and H != W wherever its predicate admits one, every loop case loops, and the cases the
list promises as refusals are refused."""
import pytest

import test_gpu_stem_paths as T

# every kernel route the stem launchers can record (csrc/fdet_stem*.hip): (family, pass, p16, u8, PS output)
ALL_ROUTES = {
    ("valu_k10", "fwd", 0, 0, 0), ("valu_k10", "wgrad", 0, 0, 0),
    ("valu_k3_generic", "fwd", 0, 0, 0), ("valu_k3_generic", "wgrad", 0, 0, 0),
    ("valu_k3_scalar", "wgrad", 0, 0, 0),
    ("mfma", "fwd", 0, 0, 0), ("mfma", "wgrad", 0, 0, 0),
    ("x3_single", "fwd", 0, 0, 0), ("x3_single", "wgrad", 0, 0, 0),
    ("x3_pipe", "fwd", 0, 0, 0),
    ("x3_pipe", "fwd", 0, 0, 1), ("x3_pipe", "fwd", 1, 0, 1), ("x3_pipe", "fwd", 0, 1, 1), ("x3_pipe", "fwd", 1, 1, 1),
    ("x3_pipe", "wgrad", 0, 0, 0), ("x3_pipe", "wgrad", 1, 0, 0),
    ("k3_matrix", "wgrad", 0, 0, 0), ("k3_matrix", "wgrad", 1, 0, 0),
    ("k3_ps_fwd", "fwd", 0, 0, 1), ("k3_ps_fwd", "fwd", 1, 0, 1),
}


def _ksp(case):
    return T.K10 if case[0] == 10 else T.K3


def _routes(case, env, entries=T.ENTRIES):
    k, N, F_, H, W, _ = case
    out = []
    for entry, p16, u8 in entries:
        r = T.expected_stem_route(entry, N, F_, H, W, *_ksp(case), p16, u8, env=env)
        if r is not None:
            out.append(tuple(r[f] for f in T.ROUTE_KEYS))
    return out


def _reached():
    seen = {}
    for c in T.CASES:
        for r in _routes(c, {}):
            seen.setdefault(r, []).append(c)
    for extra, cases, loops in T.SWITCH_GROUPS:
        assert cases and all(c in T.CASES for c in cases), f"switch group {extra} selects no case of the table"
        assert all(i in T.LOOP_IDS for i in loops), f"switch group {extra}: unknown loop case"
        for c in cases:
            for r in _routes(c, extra):
                seen.setdefault(r, []).append(c)
    return seen


def test_every_route_has_a_case():
    seen = _reached()
    assert set(seen) == ALL_ROUTES, f"no case for {sorted(ALL_ROUTES - set(seen))}; unknown routes {sorted(set(seen) - ALL_ROUTES)}"


def test_loop_ids_name_the_loop_cases():
    assert len(T.LOOP_IDS) == len(set(T.LOOP_IDS)) == len(T.loop_cases())


def test_every_switch_changes_a_route_of_its_subset():
    for extra, cases, _ in T.SWITCH_GROUPS:
        changed = [c for c in cases if _routes(c, extra) != _routes(c, {})]
        assert changed, f"{extra}: no selected case takes another route under the switch"


def _bottom_pad(case):
    k, _, _, H, W, _ = case
    k, s, p = _ksp(case)
    Ho, _ = T.out_hw(H, W, k, s, p)
    return (Ho - 1) * s - p + k - 1 >= H                   # the last window reads a row past the image


def _right_pad(case):
    k, _, _, H, W, _ = case
    k, s, p = _ksp(case)
    _, Wo = T.out_hw(H, W, k, s, p)
    return (Wo - 1) * s - p + k - 1 >= W


# families whose predicate admits no such shape.  The k10 matrix-core kernels need W % 4 == 0: with W = 8 q or 8 q + 4 the
# last window ends on column 8 q - 1 < W, so no right pad exists (checked by enumeration below).  The even-only k3
# kernels have H = 2 Ho, W = 2 Wo: the last window ends on the last row / column exactly.
NO_RIGHT_PAD = {"mfma", "x3_single", "x3_pipe", "valu_k3_scalar", "k3_matrix", "k3_ps_fwd"}
NO_BOTTOM_PAD = {"valu_k3_scalar", "k3_matrix", "k3_ps_fwd"}


def test_every_family_has_pad_and_nonsquare_cases():
    seen = _reached()
    assert not [W for W in range(4, 1025, 4) if T.stem_mfma_ok(64, 64, W, *T.K10) and _right_pad((10, 1, 64, 64, W, 0))]
    no_right = NO_RIGHT_PAD
    for family in sorted({r[0] for r in ALL_ROUTES}):
        cases = [c for r, cs in seen.items() if r[0] == family for c in cs]
        assert any(c[3] != c[4] for c in cases), f"{family}: no case with H != W"
        if family not in NO_BOTTOM_PAD:
            assert any(_bottom_pad(c) for c in cases), f"{family}: no case reads a bottom padding row"
        if family not in no_right:
            assert any(_right_pad(c) for c in cases), f"{family}: no case reads a right padding column"
    # the even-only k3 kernels: H = 2 Ho, W = 2 Wo, the last window ends on the last row / column exactly
    for c in T.K3_CASES:
        if c[3] % 2 == 0 and c[4] % 2 == 0:
            assert not _bottom_pad(c) and not _right_pad(c)


def test_promised_refusals_are_refusals():
    E = T.expected_stem_route
    assert E("wgrad_x3", 2, 128, 94, 352, *T.K10, p16=True, env={}) is None          # precision16 k10 wgrad at Wo = 44
    assert E("wgrad_x3", 2, 128, 94, 352, *T.K10, p16=False, env={})["family"] == "x3_single"
    assert E("fwd_ps", 2, 32, 22, 32, *T.K10, env={}) is None                         # PS forward with F = 32
    assert E("fwd_ps", 2, 64, 478, 478, *T.K10, u8=True, env={}) is None              # uint8 frames with W % 4 != 0
    assert E("fwd_ps", 2, 64, 70, 512, *T.K10, env={}) is None                        # Wo = 64: no 64-slot PS row
    assert E("wgrad_x3", 2, 64, 478, 484, *T.K10, env={}) is None                     # W % 16 != 0
    assert E("wgrad_x3", 2, 8, 6, 1280, *T.K3, env={}) is None                        # Wo = 640 > 320
    assert E("wgrad_x3", 2, 64, 96, 480, *T.K10, p16=True, env={"FDET_STEM_PIPE": "0"}) is None
    refused = sum(E(e, c[1], c[2], c[3], c[4], *_ksp(c), p16, u8, env={}) is None for c in T.CASES for e, p16, u8 in T.ENTRIES)
    assert refused >= len(T.CASES)                                                    # the table keeps testing refusals


@pytest.mark.parametrize("ncu", [256, 304, 80])
def test_loop_cases_loop(ncu):
    for entries, c in T.loop_cases(ncu):
        for entry, p16, u8 in entries:
            r = T.expected_stem_route(entry, c[1], c[2], c[3], c[4], *_ksp(c), p16, u8, env={}, ncu=ncu)
            assert r is not None and r["items"] > r["grid"] and r["items"] % r["grid"] != 0, (ncu, entry, c, r)
    r = T.expected_stem_route("wgrad", *T.loop_cases(ncu)[4][1][1:5], *T.K3, env={}, ncu=ncu)
    ipw = -(-r["items"] // r["grid"])
    assert ipw >= 2 and ipw * (r["grid"] - 1) >= r["items"], "the scalar-fed loop case has no idle tail workgroup"


def test_table_reaches_the_edges_it_names():
    ids = {T.case_id(c) for c in T.CASES}
    assert len(ids) == len(T.CASES)
    k3 = {(c[3], c[4]): c for c in T.K3_CASES}
    for hw, wo, rem in (((64, 40), 20, 4), ((8, 24), 12, 4), ((30, 136), 68, 4), ((32, 488), 244, 4)):
        assert hw[1] // 2 == wo and wo % 8 == rem and hw[1] % 16 != 0                 # !w16 and a partial last chunk
    assert k3[(64, 32)][5] == 4 and 32 % 16 == 0                                      # w16 by width, misaligned by base
    assert T.ps_strips(244) == (4, 62, 58) and T.ps_strips(640)[0] == 11 and T.ps_strips(320)[0] == 6 and T.ps_strips(68)[0] == 2
    assert [c[4] // 2 // 16 for c in T.K3_CASES if c[3:5] in ((50, 64), (48, 96), (20, 640))] == [2, 3, 20]
    assert T.stem_plan(2, 8, 6, 1280, *T.K3) is None                                  # the LDS bound of the fp32 plan
    k10 = {(c[3], c[4]): c for c in T.K10_CASES}
    assert T.stem_plan(2, 128, 100, 640, *T.K10)["lds_fwd"] > 64 * 1024
    assert [T.ps_wp(T.out_hw(h, w, *T.K10)[1]) for h, w in ((10, 36), (102, 224), (62, 416), (478, 484))] == [16, 32, 64, 64]
    assert T.out_hw(486, 96, *T.K10) == (61, 12) and T.out_hw(62, 416, *T.K10) == (8, 52) and T.out_hw(13, 12, *T.K10) == (1, 1)
    assert {c[2] for c in T.K10_CASES} == {64, 8, 100, 128, 32} and {c[2] for c in T.K3_CASES} == {16, 64, 8, 72}
    assert any(c[1] == 1 for c in T.K10_CASES) and any(c[1] == 1 for c in T.K3_CASES)
    assert (478, 484) in k10 and _bottom_pad(k10[(478, 484)]) and not _right_pad(k10[(478, 484)])
    assert _bottom_pad(k10[(478, 478)]) and _right_pad(k10[(478, 478)])
