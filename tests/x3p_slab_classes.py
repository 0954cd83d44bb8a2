"""How the f16x3 planes kernels cut K into split-K slabs, restated in plain Python (no torch, no GPU): shared by the CPU test
that classifies every plan the library can pick (`test_x3p_plan_classes.py`) and by the GPU test that runs one case per class
(`test_gpu_x3p_splitk.py`).

`igemm_x3p_kernel` cuts the K / 32 K tiles of a launch, the halo kernels (`conv3x3_halo_x3p_kernel`, `..._phase`) the
(C1 + C2) / 32 channel blocks, both as

    per = ceil(n / splits);  lo = min(n, y * per);  hi = min(n, lo + per)          (y = blockIdx.y)

so a slab may start in the middle of a tap, may be shorter than the staging ring, and trailing slabs may be empty (their
workgroups still write zeros into the workspace the reducer sums).
"""
BK = 32                      # XP_BK: channels per K tile / channel block
IGEMM_TILES = (1, 2, 3, 4, 5, 6, 7, 8)
HALO_TILES = (11, 12, 13)    # 11 plain, 12 nearest-2x fused (nine taps), 13 nearest-2x in phase form


def slabs(n, splits):
    """the [lo, hi) ranges of `splits` slabs over n K tiles (or channel blocks), exactly as the kernels compute them"""
    splits = max(1, int(splits))
    per = -(-n // splits)
    out = []
    for y in range(splits):
        lo = min(n, y * per)
        out.append((lo, min(n, lo + per)))
    return out


def parse_key(key):
    """'conv|256|640|5760|s2' -> ('conv', 's2', 256, 640, 5760)"""
    parts = key.split("|")
    return parts[0], "|".join(parts[4:]), int(parts[1]), int(parts[2]), int(parts[3])


def plan_class(kind, variant, M, N, K, tile, splits):
    """the coarse class of one (tile, splits) plan of a plan-table key `kind|M|N|K|variant` (variant: '', 's2', 'u', 'e', 'g').

    tiles 1-8:   (kind, variant, tile, split?, empty?, short?, tap_aligned?)   over n = K / 32 K tiles; `short`: some non-empty
                 slab has at most 2 K tiles (below every ring depth); `tap_aligned` (conv without the fused 1x1 only, else None):
                 every slab starts on a tap boundary, i.e. at a multiple of K / 9 / 32
    tiles 11-13: (tile, variant, split?, 'even' | 'ragged' | 'empty')   over ncb = K / 9 / 32 channel blocks after
                 splits = min(splits, ncb), as `planes.conv3x3` clamps them; a table entry of tile 11 under `u` runs as tile 12
    """
    splits = max(1, int(splits))
    if tile in HALO_TILES:
        if kind != "conv" or variant not in ("", "u") or K % (9 * BK):
            raise ValueError(f"no halo form for {kind}|{M}|{N}|{K}|{variant}")
        if tile in (11, 12):
            tile = 12 if variant == "u" else 11
        ncb = K // 9 // BK
        splits = min(splits, ncb)
        sizes = [hi - lo for lo, hi in slabs(ncb, splits)]
        picture = "empty" if 0 in sizes else "even" if len(set(sizes)) == 1 else "ragged"
        return (tile, variant, splits > 1, picture)
    if tile not in IGEMM_TILES or K % BK:
        raise ValueError(f"unknown tile {tile} / K {K}")
    sl = slabs(K // BK, splits)
    sizes = [hi - lo for lo, hi in sl]
    aligned = None
    if kind == "conv" and variant != "e":
        per_tap = K // 9 // BK
        aligned = all(lo % per_tap == 0 for lo, _ in sl)
    return (kind, variant, tile, splits > 1, 0 in sizes, any(0 < s <= 2 for s in sizes), aligned)


def start_site(kt, C1, C2=0, CE1=0, CE2=0):
    """where K tile `kt` of a convolution [9 taps x (x | x2)] [e1 | e2] lies: (tap, site) with tap 9 = the fused 1x1 range and
    site one of 'tap' (first tile of a tap), 'in_x', 'in_x2', 'extras_boundary' (first tile after the ninth tap), 'in_e1',
    'e2_start', 'in_e2'; 'end' for kt = the number of K tiles (where an empty slab starts)"""
    Ctot, k0 = C1 + C2, kt * BK
    K = 9 * Ctot + CE1 + CE2
    if not 0 <= k0 <= K:
        raise ValueError("K tile out of range")
    if k0 == K:
        return (9 if CE1 else 8, "end")
    if k0 < 9 * Ctot:
        tap = k0 // Ctot
        c = k0 - tap * Ctot
        return (tap, "tap" if c == 0 else "in_x" if c < C1 else "in_x2")
    c = k0 - 9 * Ctot
    return (9, "extras_boundary" if c == 0 else "in_e1" if c < CE1 else "e2_start" if c == CE1 else "in_e2")


def start_sites(splits, C1, C2=0, CE1=0, CE2=0):
    """[(first K tile, tap, site)] of the non-empty slabs of a convolution cut into `splits`"""
    n = (9 * (C1 + C2) + CE1 + CE2) // BK
    return [(lo,) + start_site(lo, C1, C2, CE1, CE2) for lo, hi in slabs(n, splits) if hi > lo]
