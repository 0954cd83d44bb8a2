"""CPU tests: every (tile, splits) plan the f16x3 planes path can pick -- the shipped `tuned_plans_x3.json`,
`planes.heuristic_plan`, `planes.halo_fallback_plan` -- falls into a slab class (`tests/x3p_slab_classes.py`) that one of the
cases of `tests/test_gpu_x3p_splitk.py` runs on the GPU against fp64.  A retune that introduces a new class (a tile under a
variant it never ran, slabs that stop being tap-aligned, a first empty or short slab) fails here until a case is added there."""
import json
import os

import pytest

from ief_amd import planes  # noqa: E402

import test_gpu_x3p_splitk as gpu_cases  # noqa: E402
import x3p_slab_classes as sc  # noqa: E402


def _covered(cases=None):
    return {gpu_cases.case_class(c) for c in (gpu_cases.CASES if cases is None else cases)}


def _table():
    with open(os.path.join(os.path.dirname(os.path.abspath(planes.__file__)), "tuned_plans_x3.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def _missing(plans, covered):
    """{class: [keys]} of the plans {key: (tile, splits)} whose class no case runs"""
    out = {}
    for key, (tile, splits) in plans.items():
        kind, variant, M, N, K = sc.parse_key(key)
        if variant == "g":
            splits = 1                                    # `planes.gemm` never splits the GEGLU epilogue
        cls = sc.plan_class(kind, variant, M, N, K, tile, splits)
        if cls not in covered:
            out.setdefault(cls, []).append(key)
    return out


def sd15_layers(B):
    """(convs, gemms) of one SD1.5 UNet forward at batch B, 64 x 64 latents, as the planes path launches them:
    convs (variant, M, Cout, K), gemms (variant, M, N, K).  conv_in (K = 36) and conv_out (N = 4) are not planes shapes."""
    convs, gemms = [], []

    def resnet(hw, cin, cout):
        convs.append(("", B * hw, cout, 9 * cin))                                  # conv1 (after GroupNorm over the concat)
        convs.append(("", B * hw, cout, 9 * cout) if cin == cout else ("e", B * hw, cout, 9 * cout + cin))        # conv2 (+ fused 1x1 shortcut)

    def transformer(hw, C):
        M = B * hw
        gemms.extend([("", M, C, C)] * 5)                 # proj_in, cross to_q, to_out x 2, proj_out
        gemms.extend([("", M, 3 * C, C), ("g", M, 8 * C, C), ("", M, C, 4 * C)])      # self q|k|v, FeedForward GEGLU, FeedForward out

    # down blocks, mid block
    for hw, cin, cout in [(4096, 320, 320), (4096, 320, 320), (1024, 320, 640), (1024, 640, 640), (256, 640, 1280), (256, 1280, 1280),
                          (64, 1280, 1280), (64, 1280, 1280), (64, 1280, 1280), (64, 1280, 1280)]:
        resnet(hw, cin, cout)
    convs.extend([("s2", B * 1024, 320, 2880), ("s2", B * 256, 640, 5760), ("s2", B * 64, 1280, 11520)])
    # up blocks: the skip concatenated to the input
    for hw, cin, cout in [(64, 2560, 1280)] * 3 + [(256, 2560, 1280), (256, 2560, 1280), (256, 1920, 1280),
                                                    (1024, 1920, 640), (1024, 1280, 640), (1024, 960, 640),
                                                    (4096, 960, 320), (4096, 640, 320), (4096, 640, 320)]:
        resnet(hw, cin, cout)
    convs.extend([("u", B * 256, 1280, 11520), ("u", B * 1024, 1280, 11520), ("u", B * 4096, 640, 5760)])
    for hw, C in [(4096, 320), (1024, 640), (256, 1280)]:
        transformer(hw, C)
    return convs, gemms


def _key(kind, variant, M, N, K):
    return f"{kind}|{M}|{N}|{K}" + (f"|{variant}" if variant else "")


def test_slabs_agree_with_a_brute_force_count():
    for n in range(1, 65):
        for splits in range(1, 65):
            per = next(p for p in range(1, n + 1) if p * splits >= n)          # ceil(n / splits) without a division
            owner = [min(t // per, splits) for t in range(n)]                  # K tile t belongs to slab t / per
            sl = sc.slabs(n, splits)
            assert len(sl) == splits and max(owner) < splits
            for y, (lo, hi) in enumerate(sl):
                assert 0 <= lo <= hi <= n and hi - lo == owner.count(y), (n, splits, y)
                assert all(owner[t] == y for t in range(lo, hi))
            assert sum(hi - lo for lo, hi in sl) == n


def test_every_shipped_plan_has_a_gpu_case_of_its_class():
    table = _table()
    assert len(table) > 300
    missing = _missing(table, _covered())
    assert not missing, f"plans of a slab class no case of test_gpu_x3p_splitk.py runs: {missing}"


def test_every_heuristic_and_halo_fallback_plan_has_a_gpu_case_of_its_class():
    heuristic, halo = {}, {}
    for B in (1, 2, 4):
        convs, gemms = sd15_layers(B)
        for variant, M, N, K in convs:
            heuristic[_key("conv", variant, M, N, K)] = planes.heuristic_plan(M, N, K, conv=True)
            if variant in ("", "u"):                      # every SD1.5 resolution has the halo form's geometry
                halo[_key("conv", variant, M, N, K)] = planes.halo_fallback_plan(M, N, K // 9 // 32)
        for variant, M, N, K in gemms:
            heuristic[_key("gemm", variant, M, N, K)] = planes.heuristic_plan(M, N, K)
    assert any(sp > 1 for _, sp in heuristic.values()) and any(t == 11 and sp > 1 for t, sp in halo.values())
    missing = _missing(heuristic, _covered())
    missing.update(_missing(halo, _covered()))
    assert not missing, f"fallback plans of a slab class no case of test_gpu_x3p_splitk.py runs: {missing}"


def test_the_sd15_shape_list_is_the_one_the_table_was_tuned_on():
    """the restated layer list names only shapes the shipped table holds (batch 1, 2 and 4)"""
    table = _table()
    for B in (1, 2, 4):
        convs, gemms = sd15_layers(B)
        for kind, layers in (("conv", convs), ("gemm", gemms)):
            for variant, M, N, K in layers:
                assert _key(kind, variant, M, N, K) in table, _key(kind, variant, M, N, K)


def test_removing_a_case_class_is_noticed():
    """without the fused-shortcut cases of tile 4 under split-K (31 shipped plans) the table is no longer covered"""
    fewer = [c for c in gpu_cases.CASES if not (c.family == "extra" and c.tile == 4 and c.splits > 1)]
    missing = _missing(_table(), _covered(fewer))
    assert missing and all(cls[:4] == ("conv", "e", 4, True) for cls in missing)
    for family in sorted({c.family for c in gpu_cases.CASES}):
        rest = [c for c in gpu_cases.CASES if c.family != family]
        assert _covered(rest) != _covered(), family


def test_the_issue_s_slab_pictures_and_start_sites():
    # plain / concat conv: C1 = 96, C2 = 64, 5 K tiles per tap, nk = 45
    assert [hi - lo for lo, hi in sc.slabs(45, 4)] == [12, 12, 12, 9]
    assert sc.start_sites(4, 96, 64) == [(0, 0, "tap"), (12, 2, "in_x"), (24, 4, "in_x2"), (36, 7, "in_x")]
    assert [hi - lo for lo, hi in sc.slabs(45, 16)] == [3] * 15 + [0]
    assert [hi - lo for lo, hi in sc.slabs(45, 32)] == [2] * 22 + [1] + [0] * 9
    # fused shortcut: h of 64 channels (18 K tiles), CE1 = 96, CE2 = 64: nk = 23
    assert sc.start_sites(5, 64, 0, 96, 64)[-1] == (20, 9, "in_e1") and sc.slabs(23, 5)[-1] == (20, 23)
    s8 = sc.start_sites(8, 64, 0, 96, 64)
    assert (18, 9, "extras_boundary") in s8 and (21, 9, "e2_start") in s8 and len(s8) == 8
    s12 = sc.start_sites(12, 64, 0, 96, 64)
    assert s12[-1] == (22, 9, "in_e2") and [hi - lo for lo, hi in sc.slabs(23, 12)] == [2] * 11 + [1]
    assert sc.start_sites(16, 64, 0, 96, 64) == s12 and [hi - lo for lo, hi in sc.slabs(23, 16)][12:] == [0] * 4
    assert sc.start_sites(4, 64, 0, 96, 0)[-1] == (18, 9, "extras_boundary") and sc.slabs(21, 4)[-1] == (18, 21)
    # every split-K `|e` slab after the first starts mid-tap; the site names at the edges
    assert sc.start_site(0, 64, 0, 96, 64) == (0, "tap") and sc.start_site(23, 64, 0, 96, 64) == (9, "end")
    assert sc.start_site(3, 96, 64) == (0, "in_x2") and sc.start_site(5, 96, 64) == (1, "tap") and sc.start_site(45, 96, 64) == (8, "end")
    # halo forms: five channel blocks; linear GEMM: nine K tiles
    assert [[hi - lo for lo, hi in sc.slabs(5, s)] for s in (2, 3, 4, 5)] == [[3, 2], [2, 2, 1], [2, 2, 1, 0], [1] * 5]
    assert [hi - lo for lo, hi in sc.slabs(9, 4)] == [3, 3, 3, 0] and [hi - lo for lo, hi in sc.slabs(9, 8)] == [2, 2, 2, 2, 1, 0, 0, 0]
    # ... and the GPU file's tables are these
    assert gpu_cases.CONV_SLABS[4] == [12, 12, 12, 9] and gpu_cases.CONV_SITES[4] == sc.start_sites(4, 96, 64)
    assert gpu_cases.EXTRA_SLABS[(96, 64)][8] == [3] * 7 + [2] and gpu_cases.HALO_SLABS[4] == [2, 2, 1, 0]
    assert gpu_cases.GEMM_SLABS[8] == [2, 2, 2, 2, 1, 0, 0, 0]


@pytest.mark.parametrize("bad", [("conv", "e", 64, 160, 736, 11, 2), ("gemm", "", 64, 160, 288, 9, 2)])
def test_plan_class_refuses_what_no_kernel_runs(bad):
    with pytest.raises(ValueError):
        sc.plan_class(*bad)
