"""CPU tests of the key-split policy of the planes attention (`planes.attn_key_splits`): a pure host
function of the launch's shape, called here with the MI355X's 256 compute units, and the workspace query of the C-ABI
(`ief_attn_flash_ws_floats`), which clamps a split count the same way."""
import itertools

import pytest

from ief_amd import hip, planes  # noqa: E402

CUS = 256


def _tiles(L, d):
    return -(-L // (64 if d == 40 else 32))


def _grid(B, heads, N, d):
    return -(-N // (256 if d == 40 else 128)) * B * heads


def _no_empty_split(S, L, d):
    nt = _tiles(L, d)
    T = -(-nt // S)
    return (S - 1) * T < nt


def test_auto_keeps_the_batch4_step_and_short_key_sets_on_the_single_launch():
    assert planes.attn_key_splits(4, 8, 4096, 4096, 40, cus=CUS) == 1
    assert planes.attn_key_splits(2, 8, 4096, 4096, 40, cus=CUS) == 1      # one workgroup per CU already: measured no faster split
    for L, d in itertools.product((1, 64, 77, 96, 127), (40, 64, 80)):
        assert planes.attn_key_splits(1, 8, 4096, L, d, cus=CUS) == 1, (L, d)
        assert planes.attn_key_splits(1, 1, 64, L, d, cus=CUS) == 1, (L, d)


def test_auto_splits_the_batch1_step():
    S = planes.attn_key_splits(1, 8, 4096, 4096, 40, cus=CUS)
    assert S > 1 and S in (2, 4, 8)
    assert _grid(1, 8, 4096, 40) * S <= 2 * CUS


def test_auto_never_overfills_the_chip_or_leaves_a_split_without_a_tile():
    for N, L, d, B, heads in itertools.product((77, 256, 1000, 1024, 4096, 16384), (128, 144, 257, 333, 1024, 4096, 16384),
                                               (40, 64, 80), (1, 2, 4), (5, 8, 10)):
        S = planes.attn_key_splits(B, heads, N, L, d, cus=CUS)
        assert 1 <= S <= planes.KEY_SPLIT_MAX, (B, heads, N, L, d, S)
        if S > 1:
            assert _grid(B, heads, N, d) * S <= 2 * CUS and 2 * _grid(B, heads, N, d) <= CUS, (B, heads, N, L, d, S)
            assert _tiles(L, d) // S >= planes.KEY_SPLIT_MIN_TILES, (B, heads, N, L, d, S)
            assert _no_empty_split(S, L, d), (B, heads, N, L, d, S)


@pytest.mark.parametrize("L,d,asked,want", [(1024, 40, 4, 4), (333, 40, 3, 3), (144, 64, 2, 2), (64, 80, 8, 2), (256, 80, 3, 3),
                                             (160, 64, 4, 3), (64, 40, 8, 1), (4096, 40, 1, 1), (4096, 40, "4", 4)])
def test_an_int_setting_passes_through_clamped(L, d, asked, want):
    """5 tiles over 4 splits are 2 + 2 + 1: three splits, as the library launches them"""
    S = planes.attn_key_splits(1, 8, 512, L, d, cus=CUS, setting=asked)
    assert S == want and _no_empty_split(S, L, d)
    # an int does not look at the grid: the caller asked for it
    assert planes.attn_key_splits(4, 8, 4096, L, d, cus=1, setting=asked) == want


def test_bad_settings_are_refused():
    for bad in (0, -2, "many"):
        with pytest.raises(ValueError):
            planes.attn_key_splits(1, 8, 512, 512, 40, cus=CUS, setting=bad)


def test_workspace_query_agrees_with_the_policys_clamp():
    """`ief_attn_flash_ws_floats`: S (d + 2) floats per (b, head, query) after the clamp, 0 where the launch would not split"""
    lib = hip.load()
    for (B, heads, N, L, d), asked in itertools.product([(1, 8, 512, 1024, 40), (1, 3, 77, 333, 40), (2, 2, 200, 144, 64),
                                                         (1, 1, 130, 64, 80), (1, 4, 256, 256, 80), (1, 2, 64, 32, 64)],
                                                        (1, 2, 3, 4, 8)):
        S = planes.attn_key_splits(B, heads, N, L, d, cus=CUS, setting=asked)
        want = S * B * heads * N * (d + 2) if S > 1 else 0
        assert lib.ief_attn_flash_ws_floats(B, heads, N, L, d, asked) == want, (B, heads, N, L, d, asked)
    assert lib.ief_attn_flash_ws_floats(1, 8, 512, 1024, 32, 4) == 0      # no planes instantiation for d = 32
    assert hip.ctypes.sizeof(hip.IefAttnF32Params) == lib.ief_struct_size(6)
