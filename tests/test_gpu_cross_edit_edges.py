"""The Prompt-to-Prompt map edit inside cross-attention (P' = c1 (P_src M) + c2 P_tgt, then P' V) on a real MI355X, on its four routes,
at the key, row and slot edges where a restaged kernel goes wrong:
    x3      `attn_cross_p2p_x3_kernel<D, QS>` (csrc/cross_p2p_x3.hip), the f16x3 headline, with and without q_src
    x3mat   scores -> softmax -> `p2p_cross_edit_f32_kernel` -> apply with `hip.X3_FUSE_CROSS = False` (the f16x3 A/B route)
    f32     the same four launches under `hip.f32_contraction("f32")`
    f16     `attn_cross_p2p_kernel<D>` (csrc/attention.hip), fp16 storage
Every launch that `hip.profile_begin()` times has its kernel names asserted, so no case can silently take another route.

Key counts 1, 2, 31, 32, 33, 63, 64, 65, 77, 95, 96 (one key tile, both sides of every tile edge, the edges themselves: no tile is
masked there and the tiles past the last hold what the previous phase left in the one LDS region); 1, 31, 129 and 163 queries (one
partial wave, a whole block + 1 row); B = 4, 2 heads.  Every key count meets d = 40 (padded K columns) and d = 160 (one workgroup per
CU, the widest staging), every head dim meets 33, 77 and 96 keys; d = 32 exists on the fp16 and the materialised routes only.

Every reference is torch fp64 on the CPU (or a closed form in exact arithmetic), computed here from the inputs; no kernel of this
library serves as a reference.  Stated tolerances (every test prints what it measured):
  1. pointer probe: K rows carry the +-1 code of a key index, V rows its 0/1 code (+ index / 128), Q = 8 x the code a per-row
     pointer names, scale 1: every softmax row is one-hot to 1e-6 (asserted), so an output row DECODES to the key it reached, and
     with permutation tables and gates in {0, 1/4, 3/4, 1} to  c1[n1] V[n1] + c2[t] V[t].  The key order differs per (batch row,
     head).  fp64 restatement vs that closed form <= 2 x 7 exp(-16) = 1.58e-6 (asserted: a one-hot row misses at most the mass of its
     7 keys at Hamming distance 1, an edited row carries two such rows weighted c1[n1] + c2[t] <= 2; the draws used here reach
     1.32e-6, so the 1.2e-6 of one instance is not a bound of the construction); a kernel vs the closed form, absolute:
         x3, x3mat  1e-5     >= 1.58e-6 + XTOL max |ref|, max |ref| <= 1
         f32        2.5e-5   = the same with KTOL
         f16        2^-10    = one fp16 rounding of P' <= 1 and one of the output <= 1
     and a kernel vs the fp64 restatement within the route's bound of 2.  Rows with edit_src < 0 equal the launch without edit
     pointers bit for bit.  Source / slot patterns: two slots in one launch, sources after their targets, three targets on one
     source, a row edited from itself, a source that is itself edited (its UNEDITED maps count), slots up to 2.
  2. gaussian inputs (k at scale 1.5, refine-style tables with one (1/3, 2/3) entry, gates 0.25 .. 1) vs fp64 at the same edges:
         x3, x3mat  <= 4e-6 of max |ref|            (XTOL, tests/test_gpu_x3.py)
         f32        <= 2e-5 of max |ref|            (KTOL, tests/test_gpu_glue_f32.py)
         f16        <= 4e-3 max |ref| + 1e-3        (tests/test_gpu_ops.py::test_attn_cross_p2p; M rounded to fp16 in the reference)
     and AttentionReweight (identity table, c1[7] in {5, 40}, a source row with P > 0.8 so that P' reaches the equalizer) on all
     four routes: finite, same bounds.
  3. views, poison, untouched memory (x3 and f16): q / k / v as column slices between NaN columns, k | v as the halves of one
     buffer, operands followed by NaN rows behind the last (edited) batch row, B = 1; destinations with a sentinel tail, and on
     x3 o[1::2] of a [2 B, N, C] buffer and a column slice: finite, bit-equal to the contiguous call, every sentinel intact (N = 31
     and 129 pin the `qi < N` store guard).  `out_planes=True` is the split of the fp32 result bit for bit, and so are the planes
     of a launch that writes Out and OutP together (`out=` + a `planes.Planes` destination).  q_src = [0, 1, 0, 1] over a 2-row Q at
     L = 33 / 64, N = 129, edit on: bit-equal to the repeated-Q launch.
     A rewrite that loads the rows it then masks turns (a) - (c) red through the V rows: 0 x NaN is NaN in the MFMA.
  4. host checks: short / long edit_src or edit_slot, edit_slot=None with an edit, a table with fewer slots than coef, coef
     [slots, 96], 97 keys: ValueError / TypeError on every route before anything is launched, the destination's sentinel intact.

Defects found while writing it (fixed with it):
  * by reading, not by a red case: `p2p_cross_edit_f32_kernel` edits the maps in place, so a source row that the same launch edits
    too ([-1, 0, 1, -1]) is read by the other row's workgroups while its own overwrite it.  Nothing orders the two; at these sizes
    every workgroup is resident at once and reads before any of them stores, so the parent's kernel passes the case as well.
    `ief_p2p_cross_edit_keep_f32` now sets such rows aside first (nothing is copied where the lists hold none, as in every plan of
    this project), which makes the expected value of that case a property of the code and not of the dispatch order.
  * `hip._attn_cross_p2p_x3` refused a destination whose batch stride is not N * ld (o[1::2]), which its kernel carries and
    `_fill_attn` documents (`hip._attn_dest` now).
  * the edit lists were unchecked on the fp16 and the materialised routes, the tables' slot counts on all, and 97 keys with an edit
    ended as a library error code after the scores launch of the materialised routes (`hip._edit_lists`, `hip._edit_tables`).
No fused kernel had to change: both zero-fill key rows >= L and query rows >= N and were right at every edge above.

Measured on the MI355X (largest of each group):
    probe, kernel vs closed form     x3 1.43e-6, x3mat 1.43e-6, f32 1.55e-6, f16 1.01e-6 absolute (fp64 vs closed form: 1.32e-6);
                                     unedited rows bit-equal to the launch without edit pointers in every case
    gaussian vs fp64                 x3 6.5e-7, x3mat 8.6e-7, f32 1.5e-6 of max |ref|; f16 2.2e-3 absolute
    reweight, equalizer 5 / 40       x3 9.8e-8, x3mat 9.8e-8, f32 1.0e-7 of max |ref|; f16 3.1e-2 absolute at max |ref| = 98 (bound 0.39)
    views / planes / q_src           bit-equal throughout, every sentinel intact, nothing not finite
    the whole file                   1.4 s (379 tests), library load excluded
"""
import contextlib
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import ief_amd  # noqa: E402,F401
from ief_amd import hip, planes  # noqa: E402

XTOL, KTOL = 4e-6, 2e-5
DEV = torch.device("cuda:0")
B, HEADS = 4, 2
SENTINEL = -7.0
ROUTES = ("x3", "x3mat", "f32", "f16")
L_ALL = (1, 2, 31, 32, 33, 63, 64, 65, 77, 95, 96)
DECODE = {"x3": 1e-5, "x3mat": 1e-5, "f32": 2.5e-5, "f16": 2.0 ** -10}
# fp64 restatement vs closed form: a one-hot row misses the mass of its keys at Hamming distance 1, at most 7 exp(-16) (+ 21 exp(-32)
# at distance 2), and an edited row carries two such rows weighted c1[n1] + c2[t] <= 2
GAP = 2 * (7 * math.exp(-16) + 21 * math.exp(-32))
DEFAULT = ((-1, 0, -1, 2), (0, 1, 0, 2))                                  # two slots in one launch, slot 2
PATTERNS = [DEFAULT,
            ((1, -1, 3, -1), (2, 0, 1, 0)),                               # sources after their targets
            ((-1, 0, 0, 0), (0, 0, 1, 2)),                                # three targets on one source, three slots
            ((-1, 1, -1, -1), (0, 2, 0, 0)),                              # a row edited from itself
            ((-1, 0, 1, -1), (0, 1, 2, 0))]                               # row 2's source is row 1, itself edited


def _dims(route):
    return (40, 64, 80, 160) if route == "x3" else (32, 40, 64, 80, 160)


def _grid(route):
    """(L, d, N): every L at d = 40 and d = 160, every other d at 33 / 77 / 96 keys, the row counts 1, 31, 129 at two or three shapes"""
    g = [(L, d, 163) for L in L_ALL for d in (40, 160)]
    g += [(L, d, 163) for d in _dims(route) if d not in (40, 160) for L in (33, 77, 96)]
    g += [(33, 40, 1), (96, 160, 1), (2, 40, 31), (77, 160, 31), (64, 40, 129), (65, 160, 129), (32, 64, 129)]
    return g


GRID = [(r,) + c for r in ROUTES for c in _grid(r)]
_worst = {}
_t0 = None


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    global _t0
    hip.load()
    torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    _t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\ncross edit edges: file wall time {time.time() - _t0:.1f} s (library load excluded); largest errors: "
          + ", ".join(f"{k} {v:.2e}" for k, v in sorted(_worst.items())))


def _note(group, e):
    _worst[group] = max(_worst.get(group, 0.0), e)


@contextlib.contextmanager
def _mode(route):
    if route == "f16":
        yield
        return
    saved, hip.X3_FUSE_CROSS = hip.X3_FUSE_CROSS, route == "x3"
    try:
        with hip.f32_contraction("f32" if route == "f32" else "x3"):
            yield
    finally:
        hip.X3_FUSE_CROSS = saved


def _names(route, d):
    if route == "x3":
        return [f"attn_cross_p2p_x3_kernel<{d}>"]
    if route == "f16":
        return [f"attn_cross_p2p_kernel<{d}>"]
    g = "igemm_x3_kernel" if route == "x3mat" else "igemm_f32_kernel"
    return [f"{g}<scores {d}>", "softmax_rows_f32_kernel", f"{g}<apply {d}>"]       # the edit kernel between them is not timed


def _dt(route):
    return torch.float16 if route == "f16" else torch.float32


def _put(route, *ts):
    return tuple(t.to(DEV, _dt(route)) for t in ts)


def _lists(es, sl):
    return torch.tensor(es, dtype=torch.int32, device=DEV), torch.tensor(sl, dtype=torch.int32, device=DEV)


def _edited(route, q, k, v, d, scale, es, sl, mt, coef, bound=1.0, out=None):
    """the edited layer on `route` through the public entry; asserts the kernels it took"""
    with _mode(route):
        hip.profile_begin()
        o = hip.attn_cross_p2p(q, k, v, q.shape[2] // d, scale, es, sl, mt.to(_dt(route)), coef, out=out, coef_bound=bound)
        names = [n for n, _, _ in hip.profile_end()]
    assert names == _names(route, d), names
    return o


def _plain(route, q, k, v, d, scale, bound=1.0):
    """the same launches WITHOUT edit pointers (the public entry would hand the unedited fp32 layer to the flash kernel)"""
    heads = q.shape[2] // d
    with _mode(route):
        hip.profile_begin()
        if route == "x3":
            o = hip._attn_cross_p2p_x3(q, k, v, heads, scale, None, None, None, None, coef_bound=bound)
        elif route == "f16":
            o = hip.attn_cross_p2p(q, k, v, heads, scale)
        else:
            o = hip._attn_apply_f32(hip._attn_scores_f32(q, k, heads, scale), v, heads, map_scale=hip.map_split_scale(bound))
        names = [n for n, _, _ in hip.profile_end()]
    assert names == _names(route, d), names
    return o


def _heads(x, d):
    b, r, c = x.shape
    return x.double().reshape(b, r, c // d, d).permute(0, 2, 1, 3)


def _maps64(q, k, d, scale):
    return torch.softmax(_heads(q, d) @ _heads(k, d).transpose(-1, -2) * scale, -1)


def _edit64(P, v, d, es, sl, mt, coef):
    """fp64: P' = c1 (P_src M) + c2 P_tgt on the rows es marks -- always from the UNEDITED maps P -- then P' V"""
    L = P.shape[-1]
    Pe = P.clone()
    for b, s in enumerate(es):
        if s >= 0:
            M = mt[sl[b], :L, :L].double().t()
            Pe[b] = coef[sl[b], 0, :L].double() * (P[s] @ M) + coef[sl[b], 1, :L].double() * P[b]
    o = (Pe @ _heads(v, d)).permute(0, 2, 1, 3)
    return o.reshape(o.shape[0], o.shape[1], -1), Pe


def _abs_err(got, ref):
    got = got.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return (got - ref).abs().max().item()


def _within(route, got, ref):
    """error of `got` in the units of the route's bound (<= 1 passes) and the plain figure that is printed"""
    e, m = _abs_err(got, ref), ref.abs().max().item()
    if route == "f16":
        return e / (4e-3 * m + 1e-3), e
    return (e / m if m else e) / (KTOL if route == "f32" else XTOL), (e / m if m else e)


# ------------------------------------------------------------------------------------------------ 1. pointer probe
def _bits(idx):
    return ((idx[..., None] >> torch.arange(7)) & 1).float()


def _probe_case(L, d, N):
    C = HEADS * d
    g = torch.Generator().manual_seed(7919 * L + d)
    perm = torch.arange(L).repeat(B, HEADS, 1)               # key row l of (b, h) carries the code perm[b, h, l]; rows 0 and L - 1 stay
    for b in range(B):
        for h in range(HEADS):
            if L > 3:
                perm[b, h, 1:L - 1] = 1 + torch.randperm(L - 2, generator=g)
    kb = _bits(perm)                                         # [B, H, L, 7]
    k, v = torch.zeros(B, L, HEADS, d), torch.zeros(B, L, HEADS, d)
    k[..., :7] = (2 * kb - 1).permute(0, 2, 1, 3)
    v[..., :7] = kb.permute(0, 2, 1, 3)
    v[..., 7] = (perm.float() / 128).permute(0, 2, 1)
    a = [i for i in range(1, 4 * L + 8) if math.gcd(i, L) == 1][:B]
    t = (torch.tensor(a)[:, None] * torch.arange(N)[None] + L - 1) % L      # pointer of (b, q): query 0 names code L - 1
    q = torch.zeros(B, N, HEADS, d)
    q[..., :7] = 8 * (2 * _bits(t) - 1)[:, :, None, :]
    mt, coef = torch.zeros(3, 96, 96), torch.zeros(3, 2, 96)
    inv_map = []
    for s in range(3):
        mapper = torch.randperm(L, generator=g)              # M[mapper[n], n] = 1
        mt[s, torch.arange(L), mapper] = 1.0
        inv_map.append(torch.argsort(mapper))
        c1 = torch.tensor([0.0, 0.25, 0.75, 1.0])[torch.randint(0, 4, (L,), generator=g)]
        coef[s, 0, :L], coef[s, 1, :L] = c1, 1 - c1
    col = torch.gather(torch.argsort(perm, -1), 2, t[:, None, :].expand(B, HEADS, N))    # the key row each pointer reaches
    q, k, v = q.reshape(B, N, C), k.reshape(B, L, C), v.reshape(B, L, C)
    P = _maps64(q, k, d, 1.0)
    assert bool((P.max(-1).values >= 1 - 1e-6).all()), "every softmax row of the probe is one-hot to 1e-6"
    assert torch.equal(P.argmax(-1), col)
    return dict(L=L, d=d, N=N, q=q, k=k, v=v, mt=mt, coef=coef, inv_map=inv_map, col=col, P=P, vrow=_heads(v, d))


def _closed(c, es, sl):
    """unedited rows: V[t]; edited rows: c1[n1] V[n1] + c2[t] V[t], n1 = the column the source row's pointer lands in"""
    out = torch.zeros(B, HEADS, c["N"], c["d"], dtype=torch.float64)
    for b in range(B):
        for h in range(HEADS):
            V, lt = c["vrow"][b, h], c["col"][b, h]
            if es[b] < 0:
                out[b, h] = V[lt]
            else:
                n1 = c["inv_map"][sl[b]][c["col"][es[b], h]]
                c1, c2 = c["coef"][sl[b], 0].double(), c["coef"][sl[b], 1].double()
                out[b, h] = c1[n1, None] * V[n1] + c2[lt, None] * V[lt]
    return out.permute(0, 2, 1, 3).reshape(B, c["N"], -1)


_probe = {}


def _run_probe(route, L, d, N, es, sl):
    c = _probe.get((L, d, N)) or _probe.setdefault((L, d, N), _probe_case(L, d, N))
    closed = _closed(c, es, sl)
    ref, _ = _edit64(c["P"], c["v"], d, es, sl, c["mt"], c["coef"])
    e64 = (ref - closed).abs().max().item()
    assert e64 <= GAP, f"fp64 restatement vs closed form {e64:.2e}"
    q, k, v = _put(route, c["q"], c["k"], c["v"])
    mt, coef = c["mt"].to(DEV), c["coef"].to(DEV)
    got = _edited(route, q, k, v, d, 1.0, *_lists(es, sl), mt, coef)
    off = _plain(route, q, k, v, d, 1.0)
    dec, dec_off = _abs_err(got, closed), _abs_err(off, _closed(c, (-1,) * B, sl))
    u, e = _within(route, got, ref)
    keep = [b for b in range(B) if es[b] < 0]
    same = torch.equal(got[keep], off[keep])
    print(f"probe {route} L={L} d={d} N={N} src={list(es)} slot={list(sl)}: decode {dec:.2e} (no edit {dec_off:.2e}), vs fp64 {e:.2e}, "
          f"fp64 vs closed form {e64:.2e}, unedited rows bit-equal: {same}")
    _note(f"probe decode {route}", max(dec, dec_off))
    assert dec <= DECODE[route] and dec_off <= DECODE[route] and u <= 1
    assert same, "rows with edit_src < 0 must equal the launch without edit pointers bit for bit"


@pytest.mark.parametrize("route,L,d,N", GRID)
def test_pointer_probe(route, L, d, N):
    _run_probe(route, L, d, N, *DEFAULT)


@pytest.mark.parametrize("es,sl", PATTERNS[1:])
@pytest.mark.parametrize("L,d", [(77, 40), (31, 40), (77, 160)])
@pytest.mark.parametrize("route", ROUTES)
def test_pointer_probe_sources_and_slots(route, L, d, es, sl):
    _run_probe(route, L, d, 163, es, sl)


# ------------------------------------------------------------------------------------------------ 2. gaussian inputs
def f32(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _tables(L, slots=2):
    """the refine-style tables of tests/test_gpu_x3.py::test_cross_attention_p2p_edit_fused_x3"""
    g = torch.Generator().manual_seed(0)
    mt, coef = torch.zeros(slots, 96, 96), torch.zeros(slots, 2, 96)
    for s in range(slots):
        mapper = torch.randint(-1, L, (L,), generator=g)
        a = (mapper != -1).float()
        M = torch.zeros(L, L)
        M[mapper % L, torch.arange(L)] = 1.0
        if L > 6:
            M[5, 5], M[5, 6] = 1.0 / 3.0, 2.0 / 3.0
        gate = (torch.rand(L, generator=g) > 0.3).float() * (0.25 + 0.75 * torch.rand(L, generator=g))
        mt[s, :L, :L] = M.t()
        coef[s, 0, :L], coef[s, 1, :L] = gate * a, 1 - gate * a
    return mt, coef


def _gauss_case(L, d, N, half, nb=B):
    """inputs (rounded to fp16 numbers for the fp16 route, M too), the unedited fp64 maps and result -- once per shape and storage"""
    C = HEADS * d
    q, k, v = f32(nb, N, C, seed=1), f32(nb, L, C, seed=2, scale=1.5), f32(nb, L, C, seed=3)
    mt, coef = _tables(L)
    if half:
        q, k, v, mt = (t.half().float() for t in (q, k, v, mt))
    P = _maps64(q, k, d, d ** -0.5)
    es, sl = ((-1, 0, -1, 2), (0, 1, 0, 0)) if nb == B else ((0,), (1,))
    ref_on, _ = _edit64(P, v, d, es, sl, mt, coef)
    ref_off, _ = _edit64(P, v, d, (-1,) * nb, sl, mt, coef)
    return dict(q=q, k=k, v=v, mt=mt, coef=coef, es=es, sl=sl, ref_on=ref_on, ref_off=ref_off)


_gauss = {}


def _gcase(L, d, N, route, nb=B):
    key = (L, d, N, route == "f16", nb)
    return _gauss.get(key) or _gauss.setdefault(key, _gauss_case(*key))


@pytest.mark.parametrize("route,L,d,N", GRID)
def test_gaussian_vs_fp64(route, L, d, N):
    c = _gcase(L, d, N, route)
    q, k, v = _put(route, c["q"], c["k"], c["v"])
    got = _edited(route, q, k, v, d, d ** -0.5, *_lists(c["es"], c["sl"]), c["mt"].to(DEV), c["coef"].to(DEV))
    off = _plain(route, q, k, v, d, d ** -0.5)
    (u, e), (uo, eo) = _within(route, got, c["ref_on"]), _within(route, off, c["ref_off"])
    print(f"gaussian {route} L={L} d={d} N={N}: edited {e:.2e}, no edit {eo:.2e} ({'absolute' if route == 'f16' else 'of max |ref|'})")
    _note(f"gaussian {route}", max(e, eo))
    assert got.dtype == _dt(route) and u <= 1 and uo <= 1


@pytest.mark.parametrize("equalizer", [5.0, 40.0])
@pytest.mark.parametrize("route", ROUTES)
def test_reweight_reaches_the_equalizer(route, equalizer):
    L, d, N = 77, 40, 163
    C = HEADS * d
    q, k, v = f32(B, N, C, seed=1), f32(B, L, C, seed=2, scale=1.5), f32(B, L, C, seed=3)
    k[0, 7] = 3.0 * torch.sign(f32(C, seed=9))                # a key that dominates many source rows: maps near 1
    q[0] = q[0] + 2.0 * torch.sign(f32(C, seed=9))
    if route == "f16":
        q, k, v = (t.half().float() for t in (q, k, v))
    mt, coef = torch.zeros(1, 96, 96), torch.zeros(1, 2, 96)
    mt[0, :L, :L] = torch.eye(L)
    coef[0, 0, :L] = 1.0
    coef[0, 0, 7] = equalizer
    es, sl = (-1, 0, -1, 0), (0, 0, 0, 0)
    P = _maps64(q, k, d, d ** -0.5)
    assert P[0, :, :, 7].max() > 0.8, "the source map must be peaky for the test to mean anything"
    ref, Pe = _edit64(P, v, d, es, sl, mt, coef)
    bound = float((coef[:, 0].abs() + coef[:, 1].abs()).max())
    got = _edited(route, *_put(route, q, k, v), d, d ** -0.5, *_lists(es, sl), mt.to(DEV), coef.to(DEV), bound=bound)
    u, e = _within(route, got, ref)
    print(f"reweight {route} equalizer {equalizer}: max P' {Pe.max():.2f}, max |ref| {ref.abs().max():.2f}: {e:.2e}")
    _note(f"reweight {route}", e)
    assert u <= 1


# ------------------------------------------------------------------------------------------------ 3. views, poison, untouched memory
def _colslice(x, fill):
    """x as the columns 8 : 8 + C of a buffer whose 8 + 8 neighbouring columns hold `fill` (16-byte aligned in both dtypes)"""
    buf = torch.full((x.shape[0], x.shape[1], x.shape[2] + 16), fill, dtype=x.dtype, device=x.device)
    buf[..., 8:-8] = x
    return buf, buf[..., 8:-8]


def _tailed(x, fill):
    """x as the first rows of a flat buffer with three more rows of `fill` behind the last batch row"""
    flat = torch.full(((x.shape[0] * x.shape[1] + 3) * x.shape[2],), fill, dtype=x.dtype, device=x.device)
    flat[:x.numel()] = x.reshape(-1)
    return flat, flat[:x.numel()].view(x.shape)


@pytest.mark.parametrize("nb", [B, 1])
@pytest.mark.parametrize("L,d,N", [(33, 40, 31), (64, 160, 129), (77, 64, 163)])
@pytest.mark.parametrize("route", ["x3", "f16"])
def test_views_poison_and_untouched_memory(route, L, d, N, nb):
    """the last batch row is an edited one (B = 1: edited from itself), so the source AND the target loads run up to the poison"""
    c = _gcase(L, d, N, route, nb)
    C, nan = HEADS * d, float("nan")
    q, k, v = _put(route, c["q"], c["k"], c["v"])
    edit = (*_lists(c["es"], c["sl"]), c["mt"].to(DEV), c["coef"].to(DEV))
    run = lambda q_, k_, v_, out=None: _edited(route, q_, k_, v_, d, d ** -0.5, *edit, out=out)
    base = run(q, k, v)
    u, e = _within(route, base, c["ref_on"])
    assert u <= 1
    blank = lambda *shape: torch.full(shape, SENTINEL, dtype=_dt(route), device=DEV)
    # (a) column slices between NaN columns; the destination a flat buffer with a sentinel tail
    flat, dst = _tailed(blank(nb, N, C), SENTINEL)
    run(_colslice(q, nan)[1], _colslice(k, nan)[1], _colslice(v, nan)[1], out=dst)
    assert torch.isfinite(dst).all() and torch.equal(dst, base), "column slices of wider projections"
    assert bool((flat[nb * N * C:] == SENTINEL).all()), "the tail behind the destination"
    # (b) k | v as the halves of one buffer; on x3 the destination o[1::2] of a [2 B, N, C] buffer
    kv = torch.cat([k, v], -1)
    if route == "x3":
        o2 = blank(2 * nb, N, C)
        got = run(q, kv[..., :C], kv[..., C:], out=o2[1::2])
        assert got.data_ptr() == o2[1::2].data_ptr() and bool((o2[0::2] == SENTINEL).all()), "the skipped batch rows"
        got = o2[1::2]
    else:
        got = run(q, kv[..., :C], kv[..., C:])
    assert torch.isfinite(got).all() and torch.equal(got, base), "k | v halves of one buffer"
    # (c) NaN rows behind the last batch row of every operand; on x3 the destination a column slice
    ops = [_tailed(t, nan)[1] for t in (q, k, v)]
    if route == "x3":
        wide, dst = _colslice(blank(nb, N, C), SENTINEL)
        run(*ops, out=dst)
        assert bool((wide[..., :8] == SENTINEL).all()) and bool((wide[..., -8:] == SENTINEL).all()), "the neighbouring columns"
    else:
        dst = run(*ops)
    assert torch.isfinite(dst).all() and torch.equal(dst, base), "operands followed by NaN rows"
    print(f"views {route} L={L} d={d} N={N} B={nb}: three view forms bit-equal to the contiguous call, sentinels intact; vs fp64 {e:.2e}")


@pytest.mark.parametrize("L,d,N", [(33, 40, 31), (64, 160, 129), (77, 64, 163)])
def test_planes_out_is_the_split_of_the_fp32_result(L, d, N):
    c = _gcase(L, d, N, "x3")
    q, k, v = _put("x3", c["q"], c["k"], c["v"])
    args = (q, k, v, HEADS, d ** -0.5, *_lists(c["es"], c["sl"]), c["mt"].to(DEV), c["coef"].to(DEV))
    with _mode("x3"):
        o = hip._attn_cross_p2p_x3(*args)
        gp = hip._attn_cross_p2p_x3(*args, out_planes=True)
        # Out and OutP of ONE launch: the caller's fp32 destination and the caller's planes, both between sentinels
        o2, p2 = torch.full((2 * B, N, HEADS * d), SENTINEL, device=DEV), planes.Planes(torch.full((2, 2 * B, N, HEADS * d), SENTINEL, dtype=torch.float16, device=DEV))
        hip._attn_cross_p2p_x3(*args, out=o2[1::2], out_planes=p2[1::2])
    hi, lo = o.half(), (o - o.half().float()).half()
    assert torch.equal(gp.hi, hi) and torch.equal(gp.lo, lo), "out_planes=True: the split of the same fp32 numbers"
    assert torch.equal(o2[1::2], o) and torch.equal(p2.hi[1::2], hi) and torch.equal(p2.lo[1::2], lo), "Out + OutP in one launch"
    assert bool((o2[0::2] == SENTINEL).all()) and bool((p2.t[:, 0::2] == SENTINEL).all())
    print(f"planes out L={L} d={d} N={N}: hi / lo bit-equal to the split of the fp32 result, alone and beside it")


@pytest.mark.parametrize("L,d", [(33, 40), (64, 40), (33, 160), (64, 160)])
def test_q_src_at_the_tile_edges(L, d):
    N = 129
    c = _gcase(L, d, N, "x3")
    q2 = c["q"][:2]
    q4 = torch.cat([q2, q2])
    ref, _ = _edit64(_maps64(q4, c["k"], d, d ** -0.5), c["v"], d, c["es"], c["sl"], c["mt"], c["coef"])
    q2, q4, k, v = _put("x3", q2, q4, c["k"], c["v"])
    edit = (*_lists(c["es"], c["sl"]), c["mt"].to(DEV), c["coef"].to(DEV))
    with _mode("x3"):
        hip.profile_begin()
        got = hip._attn_cross_p2p_x3(q2, k, v, HEADS, d ** -0.5, *edit, q_src=hip.BatchRows([0, 1, 0, 1], 2, DEV))
        rep = hip._attn_cross_p2p_x3(q4, k, v, HEADS, d ** -0.5, *edit)
        names = [n for n, _, _ in hip.profile_end()]
    assert names == _names("x3", d) * 2, names
    u, e = _within("x3", got, ref)
    print(f"q_src L={L} d={d} N={N} edit on: {e:.2e} vs fp64; bit-equal to the repeated Q: {torch.equal(got, rep)}")
    assert torch.equal(got, rep) and u <= 1


# ------------------------------------------------------------------------------------------------ 4. host checks
def _refused(call, *bufs):
    with pytest.raises((ValueError, TypeError)):
        call()
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == SENTINEL).all()), "a refused call wrote its output"


@pytest.mark.parametrize("route", ROUTES + ("x3 kernel entry",))
def test_bad_edit_lists_and_tables_are_refused_on_the_host(route):
    L, d, N = 33, 40, 31
    direct = route == "x3 kernel entry"
    r = "x3" if direct else route
    c = _gcase(L, d, N, r)
    q, k, v = _put(r, c["q"], c["k"], c["v"])
    es, sl = _lists(c["es"], c["sl"])
    mt, coef = c["mt"].to(DEV, _dt(r)), c["coef"].to(DEV)
    out = torch.full((B, N, HEADS * d), SENTINEL, dtype=_dt(r), device=DEV)

    def call(q=q, k=k, v=v, es=es, sl=sl, mt=mt, coef=coef):
        with _mode(r):
            if direct:
                return hip._attn_cross_p2p_x3(q, k, v, HEADS, d ** -0.5, es, sl, mt, coef, out=out)
            return hip.attn_cross_p2p(q, k, v, HEADS, d ** -0.5, es, sl, mt, coef, out=out)
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    _refused(lambda: call(es=es[:-1]), out)                                           # short lists: read past their end on the device
    _refused(lambda: call(sl=sl[:-1]), out)
    _refused(lambda: call(es=torch.cat([es, one])), out)                              # long lists
    _refused(lambda: call(sl=torch.cat([sl, one])), out)
    _refused(lambda: call(sl=None), out)
    _refused(lambda: call(mt=mt[:1]), out)                                            # a table with fewer slots than coef
    _refused(lambda: call(coef=coef[:, 0].contiguous()), out)                         # coef [slots, 96]
    _refused(lambda: call(coef=torch.cat([coef, coef], 1)[:, ::2]), out)              # [slots, 2, 96], not contiguous
    k97 = torch.zeros(B, 97, HEADS * d, dtype=_dt(r), device=DEV)
    _refused(lambda: call(k=k97, v=k97), out)                                         # 97 keys: the tables hold 96
    good = call()                                                                     # and the same call with nothing wrong goes through
    assert good.data_ptr() == out.data_ptr() and _within(r, out, c["ref_on"])[0] <= 1


def test_bad_edit_lists_and_tables_are_refused_by_the_map_edit():
    heads, N, L = 2, 31, 33
    maps = torch.full((B * heads, N, L), SENTINEL, device=DEV)
    mt, coef = _tables(L)
    mt, coef = mt.to(DEV), coef.to(DEV)
    es, sl = _lists((-1, 0, -1, 2), (0, 1, 0, 0))
    call = lambda es=es, sl=sl, mt=mt, coef=coef, maps=maps: hip.p2p_cross_edit_(maps, B, heads, es, sl, mt, coef)
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    for kw in (dict(es=es[:-1]), dict(sl=sl[:-1]), dict(es=torch.cat([es, one])), dict(sl=torch.cat([sl, one])), dict(sl=None),
               dict(mt=mt[:1]), dict(coef=coef[:, 0].contiguous()), dict(es=es.long())):
        _refused(lambda: call(**kw), maps)
    maps97 = torch.full((B * heads, N, 97), SENTINEL, device=DEV)
    _refused(lambda: call(maps=maps97), maps97)
    _refused(lambda: call(maps=maps[:-1]), maps)                                      # not B * heads maps
