"""Negative-prompt inversion and proximal guidance, the host side (no GPU): the rule's fp32 restatement against an fp64 one, the
rank arithmetic against `torch.quantile`, every argparse error and every `ValueError` pair, the NPI context, the plan's tables and
the ABI pins (flat arguments: no struct joins, the version stays).

The bound of the fp32-vs-fp64 restatement: an element of x_out is formed by at most 12 correctly rounded fp32 operations (sub, mul,
add, mul, sub, div, sub, mul, sub, mul, mul, add) on coefficients that carry 4 more roundings (two 1 - a and two sqrt each way),
16 in all, each at most 2^-24 of an intermediate.  The intermediates (eps, x0) are larger than the result: with a_from = 0.55,
a_to = 0.71, x' = sa_t x0 + sb_t eps cancels to about -0.22 eps while x0 is about -0.9 eps, so they stay below 8 max |ref|.
16 x 8 x 2^-24 = 2^-17 of max |ref|.
"""
import ctypes
import importlib.util
import inspect
import os
import sys

import pytest
import torch

import ief_amd  # noqa: F401
from ief_amd import cabi, denoise, hip
import prox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
P2P, MASA = os.path.join(PKG, "p2p"), os.path.join(PKG, "masactrl")


def inputs(Bp, C, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return r(Bp, C, h, w), r(Bp, C, h, w), r(Bp, C, h, w), r(C, h, w)


# ------------------------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("mode", ["l0", "l1"])
@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("shape", [(3, 4, 8, 8), (2, 4, 7, 9), (1, 1, 1, 1), (2, 4, 64, 64)])
def test_fp32_restatement_against_fp64(mode, radius, shape):
    eu, ec, x, z0 = inputs(*shape, seed=11 + radius)
    lam = prox_ref.thresholds(eu, ec, 0.7)
    for on, eta in ((1.0, 0.0), (1.0, 0.7), (0.0, 1.0), (0.0, 0.0), (1.0, 1.0)):
        coef = [0.55, 0.71, 7.5, on, eta]
        x32, x0_32 = prox_ref.step(eu, ec, x, coef, lam, z0, mode, radius, torch.float32)
        x64, x0_64 = prox_ref.step(eu, ec, x, coef, lam, z0, mode, radius, torch.float64)
        assert x32.dtype == torch.float32 and x64.dtype == torch.float64
        fig = ((x32.double() - x64).abs().max() / x64.abs().max()).item()
        fig0 = ((x0_32.double() - x0_64).abs().max() / x0_64.abs().max()).item()
        print(f"{mode} r={radius} {shape} prox_on={on} eta={eta}: fp32 vs fp64 restatement {fig:.3e} (x_out), {fig0:.3e} (x0); bound {2.0 ** -17:.3e}")
        assert fig <= 2.0 ** -17 and fig0 <= 2.0 ** -17


def test_restatement_properties():
    eu, ec, x, z0 = inputs(3, 4, 8, 8, seed=5)
    lam = prox_ref.thresholds(eu, ec, 0.7)
    plain, plain0 = prox_ref.step(eu, ec, x, [0.55, 0.71, 7.5, 0.0, 0.0], lam, z0, "l0", 1, torch.float32)
    # prox_on == 0 and eta == 0: the CFG + DDIM step written out
    e = eu + 7.5 * (ec - eu)
    a_f, a_t = torch.tensor(0.55), torch.tensor(0.71)
    root = prox_ref.sqrt_of
    x0 = (x - root(1 - a_f) * e) / root(a_f)
    assert torch.equal(plain0, x0) and torch.equal(plain, root(a_t) * x0 + root(1 - a_t) * e)
    import numpy as np
    assert root(1 - a_f).item() == float(np.sqrt(np.float32(1) - np.float32(0.55))) and root(a_f.double()).dtype == torch.float64
    keep, m = prox_ref.decisions(eu, ec, lam, 1)
    assert abs(keep[1:].float().mean().item() - 0.3) < 0.02, "the 0.7-quantile keeps 30 % of a row"
    assert (m | ~keep).all() and m.sum() > keep.sum(), "the dilated mask contains the edit"
    for mode in ("l0", "l1"):
        out, out0 = prox_ref.step(eu, ec, x, [0.55, 0.71, 7.5, 1.0, 1.0], lam, z0, mode, 1, torch.float32)
        assert torch.equal(out[0], plain[0]) and torch.equal(out0[0], plain0[0]), "row 0 is the plain step"
        _, thr0 = prox_ref.step(eu, ec, x, [0.55, 0.71, 7.5, 1.0, 0.0], lam, z0, mode, 1, torch.float32)
        off = ~m[1:]
        # eta = 1: x0 - (x0 - z0), two correctly rounded operations: within 2^-23 (|z0| + |x0|) of z0 (tests/test_gpu_direct_inversion.py)
        bound = 2.0 ** -23 * (z0.abs()[None] + thr0[1:].abs())
        assert ((out0[1:] - z0[None]).abs()[off] <= bound[off]).all(), "eta = 1: unedited elements land on z0 to rounding"
        assert torch.equal(out0[1:][m[1:]], thr0[1:][m[1:]]), "inside the dilated mask x0 is not pulled"
        if mode == "l0":
            assert torch.equal(out[1:][keep[1:]], plain[1:][keep[1:]]), "l0 keeps d where it is above the threshold"
    # eta without thresholding: m = 1 everywhere, nothing is pulled
    out, _ = prox_ref.step(eu, ec, x, [0.55, 0.71, 7.5, 0.0, 1.0], lam, z0, "l0", 1, torch.float32)
    assert torch.equal(out, plain)


# ------------------------------------------------------------------------------------------------------------- the rank
@pytest.mark.parametrize("q", [0.0, 0.3, 0.7, 1.0])
@pytest.mark.parametrize("n", [1, 2, 257, 16384])
def test_rank_arithmetic_against_torch_quantile(q, n):
    from ief_amd.control import ledits_rank
    lo, frac = ledits_rank(q, n)
    pos = q * (n - 1)
    assert 0 <= lo <= n - 1 and 0.0 <= frac < 1.0
    assert abs((lo + frac) - pos) <= 2.0 ** -24 * max(1.0, pos), "lo + frac is q (n - 1), the remainder rounded to fp32"
    assert lo == min(int(pos // 1), n - 1) or (lo == int(pos // 1) + 1 and frac == 0.0)
    plan = denoise.ProxGuidance("l0", q, 1, [1], [0.0])
    r = plan.rank(n)
    assert r.dtype == torch.float32 and r.tolist() == [float(lo), frac] and float(lo) == lo
    v = torch.randn(3, n, generator=torch.Generator().manual_seed(n)).abs()
    got = prox_ref.quantile_f32(v, q)
    want = torch.quantile(v.double(), q, dim=1)
    assert got.dtype == torch.float32
    # one subtraction, one product, one sum, each rounded: 3 x 2^-24 of the larger order statistic (and frac's own rounding)
    assert ((got.double() - want).abs() <= 2.0 ** -22 * v.max(dim=1).values.double()).all(), (got, want)
    assert torch.allclose(got, torch.quantile(v, q, dim=1), rtol=2.0 ** -21, atol=0)


def test_plan_tables_and_refusals():
    ts = [981, 741, 501, 261, 21]
    p = denoise.ProxGuidance.from_schedule(ts, "l1", 0.7, 2, prox_steps=(1, 4), recon_lr=0.5, recon_t=400)
    assert (p.mode, p.quantile, p.radius) == ("l1", 0.7, 2)
    assert p.prox_on == [0.0, 1.0, 1.0, 1.0, 0.0] and p.eta == [0.0, 0.0, 0.0, 0.5, 0.5]
    assert denoise.ProxGuidance.from_schedule(ts).prox_on == [1.0] * 5
    for bad in (dict(mode="l2"), dict(quantile=1.5), dict(quantile=-0.1), dict(radius=4), dict(radius=-1), dict(radius=1.0),
                dict(prox_steps=(3, 2)), dict(prox_steps=(0, 6))):
        with pytest.raises(ValueError, match="prox"):
            denoise.ProxGuidance.from_schedule(ts, **bad)
    with pytest.raises(ValueError, match="prox"):
        denoise.ProxGuidance("l0", 0.7, 1, [1, 1], [0.0])
    assert hip.PROX_MODES == {"l0": 0, "l1": 1} and hip.PROX_MAX_ROW == 65536


# ------------------------------------------------------------------------------------------------------------- ValueError pairs
def _check(**kw):
    plan = denoise.ProxGuidance("l0", 0.7, 1, [1] * 4, [0.0] * 4)
    good = dict(mode="denoise", cfg=True, uncond_list=None, source_trajectory=None, noise_maps=None, edit_mask=None, ledits=None,
                added_cond_kwargs=None, local_blend=None, source_latent=torch.zeros(4, 8, 8), row_shape=(4, 8, 8), num_steps=4)
    good.update(kw)
    return denoise.check_prox(good.pop("plan", plan), **good)


def test_check_prox_names_every_pair():
    assert _check() is None
    t = torch.zeros(4, 4, 8, 8)
    for name, value in (("uncond_list", [t]), ("source_trajectory", t), ("noise_maps", t), ("edit_mask", t[0, 0]),
                        ("ledits", object()), ("added_cond_kwargs", {"text_embeds": t}), ("local_blend", t)):
        shown = "LocalBlend" if name == "local_blend" else name
        with pytest.raises(ValueError, match=f"prox together with {shown}"):
            _check(**{name: value})
    with pytest.raises(ValueError, match="prox together with a loop without guidance"):
        _check(cfg=False)
    with pytest.raises(ValueError, match="prox together with a loop without guidance"):
        _check(mode="invert")
    for kw in (dict(source_latent=None), dict(source_latent=torch.zeros(4, 8, 8).double()), dict(source_latent=torch.zeros(4, 8, 9)),
               dict(num_steps=5), dict(plan=dict(mode="l0")), dict(row_shape=(4, 160, 160), source_latent=torch.zeros(4, 160, 160))):
        with pytest.raises(ValueError, match="prox"):
            _check(**kw)
    assert _check(source_latent=torch.zeros(1, 4, 8, 8)) is None


def test_sampler_checks_and_the_loop_key():
    from ief_amd.p2p.model.sd_utils import check_npi
    plan = denoise.ProxGuidance("l0", 0.7, 1, [1] * 4, [0.0] * 4)
    neg = torch.zeros(1, 77, 8)
    ok = dict(uncond_list=None, cfg_split=False, low_resource=False)
    assert check_npi(neg, plan, **ok) is None and check_npi(None, None, **ok) is None and check_npi(neg, None, **ok) is None
    with pytest.raises(ValueError, match="negative_prompt_embeds together with uncond_embeddings_list"):
        check_npi(neg, None, **dict(ok, uncond_list=[neg]))
    with pytest.raises(ValueError, match="prox without negative_prompt_embeds"):
        check_npi(None, plan, **ok)
    with pytest.raises(ValueError, match="prox together with the CFG split"):
        check_npi(neg, plan, **dict(ok, cfg_split=True))
    with pytest.raises(ValueError, match="prox together with low_resource"):
        check_npi(neg, plan, **dict(ok, low_resource=True))
    for fn, names in ((denoise.acquire, ("prox", "source_latent")), (denoise.FusedDenoiser.__init__, ("prox", "source_latent")),
                      (denoise.FusedDenoiser.rebind, ("prox", "source_latent")), (hip.cfg_ddim_step, ("prox",))):
        for n in names:
            assert inspect.signature(fn).parameters[n].default is None
    from ief_amd.masactrl.model.sd_utils import MasaCtrl
    from ief_amd.p2p.model.sd_utils import P2P
    for fn in (P2P.text2image_ldm_stable, MasaCtrl.__call__):
        for n in ("negative_prompt_embeds", "prox", "source_latent"):
            assert inspect.signature(fn).parameters[n].default is None
    # mode and radius are part of the key, the quantile and the rows are not
    probe = denoise.FusedDenoiser.__new__(denoise.FusedDenoiser)

    class _U:
        _plan = None

    class _S:
        timesteps = [3, 2, 1, 0]

    probe.unet, probe.sched, probe.mode, probe.cfg, probe.Bp, probe.ledits = _U(), _S(), "denoise", True, 2, None
    probe.lat = torch.empty(0, 0, 8, 8)
    ctx = torch.zeros(4, 77, 8)
    key = lambda p: probe._key(ctx, None, prox=p)
    other_rows = denoise.ProxGuidance("l0", 0.5, 1, [0, 1, 1, 0], [0.0, 0.0, 1.0, 1.0])
    assert key(plan) == key(other_rows) and key(plan) != key(None) and key(None) == probe._key(ctx, None)
    assert key(plan) != key(denoise.ProxGuidance("l1", 0.7, 1, [1] * 4, [0.0] * 4))
    assert key(plan) != key(denoise.ProxGuidance("l0", 0.7, 2, [1] * 4, [0.0] * 4))


# ------------------------------------------------------------------------------------------------------------- the NPI context
def test_npi_context_has_the_source_embedding_in_every_unconditional_row():
    from ief_amd.masactrl.inversion.npi import NPI as MasaNPI
    from ief_amd.p2p.inversion.ddim import ddim_inversion
    from ief_amd.p2p.inversion.npi import NPI
    from ief_amd.p2p.model.sd_utils import npi_context
    assert MasaNPI is NPI and issubclass(NPI, ddim_inversion) and "ddim_inversion_loop" not in NPI.__dict__
    g = torch.Generator().manual_seed(3)
    context = torch.randn(2, 77, 8, generator=g)                    # the inversion's (uncond, cond) of the SOURCE prompt
    text = torch.randn(3, 77, 8, generator=g)                       # the edit's conditional rows: source + two targets
    inv = NPI()
    neg = inv.negative_prompt_embeds(context)
    assert neg.shape == (1, 77, 8) and torch.equal(neg[0], context[1]) and neg.data_ptr() != context.data_ptr()
    unc = npi_context(neg, text)
    assert unc.shape == text.shape and all(torch.equal(unc[b], context[1]) for b in range(3))
    assert torch.equal(npi_context(neg[0], text), unc)
    for bad in (torch.zeros(2, 77, 8), torch.zeros(1, 76, 8), torch.zeros(77), None):
        with pytest.raises(ValueError, match="negative_prompt_embeds"):
            npi_context(bad, text)
    with pytest.raises(ValueError):
        inv.negative_prompt_embeds(context[:1])
    latents = [torch.full((1, 4, 3, 2), float(k)) for k in range(5)]
    z0 = inv.source_latent(latents)
    assert z0.shape == (4, 3, 2) and z0.dtype == torch.float32 and torch.equal(z0, latents[0][0])

    class _Sched:
        timesteps = torch.tensor([981, 741, 501, 261, 21])

    class _Pipe:
        scheduler = _Sched()

    assert inv.prox_plan(_Pipe(), mode="none") is None
    plan = inv.prox_plan(_Pipe(), mode="l0", quantile=0.6, radius=2, prox_steps=None, recon_lr=1.0, recon_t=400)
    assert isinstance(plan, denoise.ProxGuidance) and plan.eta == [0.0, 0.0, 0.0, 1.0, 1.0] and plan.radius == 2


# ------------------------------------------------------------------------------------------------------------- argparse
def _load(folder, script, name):
    """a script loaded the way `python <script>` finds its neighbours, under a private module name"""
    bare = ("_bootstrap", "edit_real", "test")
    saved_path = list(sys.path)
    saved_mods = {k: sys.modules.pop(k) for k in bare if k in sys.modules}
    try:
        sys.path[:0] = [folder, P2P]
        spec = importlib.util.spec_from_file_location(name, os.path.join(folder, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved_path
        for k in bare:
            sys.modules.pop(k, None)
        sys.modules.update(saved_mods)
    return mod


def _errors(parse, argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and word in err, (argv, err)


BAD_VALUES = (["--prox_quantile", "1.2"], ["--prox_quantile", "-0.1"], ["--dilate_mask", "4"], ["--dilate_mask", "-1"],
              ["--prox", "l2"], ["--prox_steps", "30", "20"], ["--prox_steps", "0", "51"])


def test_p2p_argparse(capsys):
    drv = _load(P2P, "test.py", "_host_prox_p2p_test")
    npi = ["--inversion_type", "npi"]
    a = drv.parse_args(npi + ["--invert_batch", "4", "--in_flight", "2"])
    assert (a.inversion_type, a.prox, a.prox_plan, a.invert_batch, a.in_flight) == ("npi", "none", None, 4, 2), "plain npi is only a context"
    a = drv.parse_args(npi + ["--prox", "l0", "--invert_batch", "4"])
    assert a.prox_plan == dict(mode="l0", quantile=0.7, radius=1, prox_steps=None, recon_lr=1.0, recon_t=400)
    a = drv.parse_args(npi + ["--prox", "l1", "--prox_quantile", "0.6", "--prox_steps", "5", "40", "--recon_lr", "0.5", "--recon_t", "300",
                              "--dilate_mask", "3"])
    assert a.prox_plan == dict(mode="l1", quantile=0.6, radius=3, prox_steps=[5, 40], recon_lr=0.5, recon_t=300)
    assert drv.parse_args([]).prox_plan is None and drv.parse_args(["--inversion_type", "direct"]).prox == "none"
    for argv, word in ((["--prox", "l0"], "--inversion_type npi"), (["--inversion_type", "ddim", "--prox", "l1"], "--inversion_type npi"),
                       (npi + ["--prox", "l0", "--in_flight", "2"], "--in_flight"), (npi + ["--prox", "l0", "--nti_batch", "2"], "--nti_batch"),
                       (npi + ["--nti_batch", "2"], "--nti_batch"), (npi + ["--prox", "l0", "--sd_version", "smallxl"], "--sd_version"),
                       (npi + ["--prox", "l1", "--sd_version", "xl-base"], "--sd_version")):
        _errors(drv.parse_args, argv, word, capsys)
    for bad in BAD_VALUES:
        _errors(drv.parse_args, npi + (bad if bad[0] == "--prox" else ["--prox", "l0"] + bad), bad[0], capsys)
    from ief_amd.p2p.inversion.npi import NPI
    assert drv.NPI is NPI
    real = _load(P2P, "edit_real.py", "_host_prox_p2p_edit_real")
    check = lambda argv: real.check_prox_arguments(real.parser, real.parser.parse_args(argv),
                                                   blend="--blend_source_words" in argv or "--blend_target_words" in argv)
    assert check(npi) is None and check([]) is None
    assert check(npi + ["--prox", "l0"])["mode"] == "l0"
    blend = ["--blend_source_words", "house", "--blend_target_words", "fall"]
    assert check(npi + blend) is None, "plain npi is only a context: a LocalBlend goes with it"
    for argv, word in ((["--prox", "l0"], "--inversion_type npi"), (npi + ["--prox", "l0"] + blend, "--blend_source_words"),
                       (npi + ["--prox", "l1", "--sd_version", "smallxl"], "--sd_version")):
        _errors(check, argv, word, capsys)
    for bad in BAD_VALUES:
        _errors(check, npi + (bad if bad[0] == "--prox" else ["--prox", "l0"] + bad), bad[0], capsys)


def test_masactrl_argparse_and_pick(capsys):
    from ief_amd.masactrl.model.sd_utils import MasaCtrl
    from ief_amd.p2p.inversion.npi import NPI
    real = _load(MASA, "edit_real.py", "_host_prox_masa_edit_real")
    drv = _load(MASA, "test.py", "_host_prox_masa_test")
    npi = ["--inversion_type", "npi"]
    check = lambda argv: real.check_prox_arguments(real.parser, real.parser.parse_args(argv))
    for parse in (check, lambda argv: drv.parse_args(argv).prox_plan):
        assert parse(npi) == dict(mode="l0", quantile=0.7, radius=1, prox_steps=None, recon_lr=1.0, recon_t=400), "l0 is this folder's default"
        assert parse(npi + ["--prox", "none"]) is None and parse([]) is None and parse(["--inversion_type", "direct"]) is None
        assert parse(npi + ["--prox", "l1", "--dilate_mask", "0"])["radius"] == 0
        for argv, word in ((["--prox", "l0"], "--inversion_type npi"), (npi + ["--sd_version", "smallxl"], "--sd_version")):
            _errors(parse, argv, word, capsys)
        for bad in BAD_VALUES:
            _errors(parse, npi + bad, bad[0], capsys)

    class _Sched:
        timesteps = torch.tensor([3, 2, 1, 0])

        def set_timesteps(self, n):
            self.n = n

    class _Pipe:
        scheduler = _Sched()

    class StableDiffusionXLPipeline(_Pipe):
        pass

    inv, ed = real.pick(_Pipe(), "npi", 4)
    assert type(inv) is NPI and type(ed) is MasaCtrl
    with pytest.raises(ValueError, match="Please choose right inversion type"):
        real.pick(StableDiffusionXLPipeline(), "npi", 4)


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_pins_and_both_prototypes_parsed_from_the_header():
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert len(cabi.structs) == 10 and cabi.defines["IEF_ABI_VERSION"] == 4, "flat arguments: no struct joins the ABI"
    assert cabi.functions["ief_prox_threshold_f32"] == (I, [P, P, P, P, I, LL, P])
    assert cabi.functions["ief_cfg_ddim_step_prox_f32"] == (I, [P, P, P, P, P, P, P, P, LL, LL, I, I, I, I, P])
    assert cabi.functions["ief_cfg_ddim_step_prox_f32"][1][:6] == cabi.functions["ief_cfg_ddim_step_f32"][1][:6]
    lib = hip.load()
    assert lib.ief_abi_version() == 4 and hip.ABI_VERSION == 4
    for name in ("ief_prox_threshold_f32", "ief_cfg_ddim_step_prox_f32"):
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == cabi.functions[name][1]
    z = torch.zeros(2, 4, 8, 8)
    with pytest.raises(TypeError):
        hip.prox_threshold(z, z, torch.zeros(2))
    with pytest.raises(TypeError):
        hip.cfg_ddim_step(z, z, z, torch.zeros(5), prox=(torch.zeros(2), torch.zeros(4, 8, 8), "l0", 1))
