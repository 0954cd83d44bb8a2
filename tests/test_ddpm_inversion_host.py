"""CPU: edit-friendly DDPM inversion's host side -- `DDIMScheduler.ddpm_coeffs`, the rule restated in torch fp64 (extraction and step
undo each other on the source row), `DDPMInversion.sample_xts`, every `ValueError` / `argparse` error of the new arguments, and the
two entry points in the binding derived from the header."""
import ctypes
import importlib.util
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

from ief_amd import cabi, hip
from ief_amd.denoise import CfgSplitDenoiser, FusedDenoiser, acquire, check_noise_maps
from ief_amd.scheduler import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2P_DIR = os.path.join(ROOT, "image-editing-framework_amd", "p2p")


# ------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("S", [4, 50])
def test_ddpm_coeffs_against_the_fp64_formulas(S):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    ts = sched.timesteps.tolist()
    assert all(a > b for a, b in zip(ts, ts[1:])), "edit order: t_0 > ... > t_{S-1}"
    for t in ts:
        a, p = sched.step_coeffs(t)
        got = sched.ddpm_coeffs(t)
        assert got[:2] == (a, p), "a_t / a_prev are step_coeffs' fp32 table values"
        a64, p64 = np.float64(a), np.float64(p)
        v = (1 - p64) / (1 - a64) * (1 - a64 / p64)
        sigma, dirc = np.sqrt(v), np.sqrt(1 - p64 - v)
        assert got[2] == float(np.float32(sigma)) and got[3] == float(np.float32(dirc)), "fp64 on the host, rounded to fp32 once"
        assert got[2] > 0, "sigma > 0 on every step of the project's schedule"
        assert abs(got[3] ** 2 + got[2] ** 2 - (1 - p64)) <= 1e-6 * (1 - p64), "dir^2 + sigma^2 = 1 - p"


# ------------------------------------------------------------------------------------------------------------- the rule, in fp64
def _rule_fp64(S, skip, eps_target=None):
    """extraction and edit written out in torch fp64 with a toy eps function -> (x0, xts, per-step rows [S - skip][2, ...])"""
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    ts = sched.timesteps.tolist()
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(4, 5, 3, generator=g, dtype=torch.float64)
    w = torch.randn(4, 5, 3, generator=g, dtype=torch.float64)
    eps_src = lambda y, t: torch.tanh(y * 0.7 + w) * (1 + t / 1000)
    eps_tgt = eps_target or eps_src
    coef = [tuple(np.float64(c) for c in sched.ddpm_coeffs(t)) for t in ts]
    xts = [np.sqrt(a) * x0 + np.sqrt(1 - a) * torch.randn(4, 5, 3, generator=g, dtype=torch.float64) for a, _, _, _ in coef] + [x0]

    def mu(y, e, c):
        a, p, _, d = c
        return np.sqrt(p) * (y - np.sqrt(1 - a) * e) / np.sqrt(a) + d * e

    z = {i: (xts[i + 1] - mu(xts[i], eps_src(xts[i], ts[i]), coef[i])) / coef[i][2] for i in range(skip, S)}
    x = torch.stack([xts[skip], xts[skip]])
    rows = []
    for i in range(skip, S):
        e = torch.stack([eps_src(x[0], ts[i]), eps_tgt(x[1], ts[i])])
        x = mu(x, e, coef[i]) + coef[i][2] * z[i]
        rows.append(x)
    return x0, xts, rows


@pytest.mark.parametrize("S,skip", [(4, 0), (4, 1), (50, 0), (50, 18)])
def test_rule_source_row_reproduces_every_stored_latent_and_x0(S, skip):
    x0, xts, rows = _rule_fp64(S, skip)
    for k, x in enumerate(rows):
        want = xts[skip + k + 1]
        assert (x[0] - want).abs().max() <= 1e-12 * max(1.0, want.abs().max()), f"source row after step {skip + k} is y_{skip + k + 1}"
    assert (rows[-1][0] - x0).abs().max() <= 1e-12 * x0.abs().max(), "... and x0 at the end"
    assert torch.equal(rows[-1][0], rows[-1][1]), "the same eps on both rows: the same result"
    _, _, other = _rule_fp64(S, skip, eps_target=lambda y, t: torch.sin(y) * 0.5)
    assert (other[-1][0] - x0).abs().max() <= 1e-12 * x0.abs().max()
    assert (other[-1][1] - other[-1][0]).abs().max() > 1e-3, "another eps on the target row: the rows differ"


# ------------------------------------------------------------------------------------------------------------- sample_xts
class _Sched(DDIMScheduler):
    pass


def _model(S=4, device="cpu"):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    unet = types.SimpleNamespace(device=torch.device(device), config=types.SimpleNamespace(in_channels=4), _plan=None)
    return types.SimpleNamespace(unet=unet, scheduler=sched)


def test_sample_xts_shape_seed_and_last_row():
    from ief_amd.p2p.inversion.ddim import ddim_inversion
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    inv = DDPMInversion()
    assert isinstance(inv, ddim_inversion) and "ddim_inversion_loop" not in DDPMInversion.__dict__
    model = _model(S=5)
    x0 = torch.randn(1, 4, 6, 3, generator=torch.Generator().manual_seed(1))
    a = inv.sample_xts(model, x0, torch.Generator().manual_seed(7))
    b = inv.sample_xts(model, x0, torch.Generator().manual_seed(7))
    c = inv.sample_xts(model, x0, torch.Generator().manual_seed(8))
    assert a.shape == (6, 4, 6, 3) and a.dtype == torch.float32 and a.is_contiguous()
    assert torch.equal(a, b), "same seed, same bits"
    assert not torch.equal(a[:-1], c[:-1])
    assert torch.equal(a[-1], x0[0]) and torch.equal(c[-1], x0[0]), "row S is x0"
    # row i is sqrt(a_i) x0 + sqrt(1 - a_i) n_i with independent unit normals: its residual has the variance 1 - a_i
    for i, t in enumerate(model.scheduler.timesteps.tolist()):
        a_i = model.scheduler.step_coeffs(t)[0]
        n = (a[i] - a_i ** 0.5 * x0[0]) / (1 - a_i) ** 0.5
        assert abs(float(n.std()) - 1) < 0.35 and abs(float(n.mean())) < 0.4
    sig = inspect.signature(DDPMInversion.noise_maps).parameters
    assert sig["guidance_scale"].default == 3.5 and sig["skip"].default == 0 and "rows_per_launch" in sig and sig["generator"].default is None


def test_noise_maps_refuses_a_hooked_unet_with_the_xl_inversions_message():
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    model = _model()
    model.unet.attention_modules = lambda: [types.SimpleNamespace(is_native=lambda: False)]
    with pytest.raises(RuntimeError, match="an attention hook is installed; invert before registering controllers"):
        DDPMInversion().noise_maps(model, torch.zeros(1, 4, 8, 8), ["a"])
    model.unet.attention_modules = lambda: []
    model.unet._plan = object()
    with pytest.raises(RuntimeError, match="an attention hook is installed; invert before registering controllers"):
        DDPMInversion().noise_maps(model, torch.zeros(1, 4, 8, 8), ["a"])
    model.unet._plan = None
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="skip"):
            DDPMInversion().noise_maps(model, torch.zeros(1, 4, 8, 8), ["a"], skip=bad)


# ------------------------------------------------------------------------------------------------------------- ValueErrors
def test_check_noise_maps_and_the_loops_refuse_bad_combinations_before_touching_the_device():
    model, ctx2, ctx1 = _model(), torch.zeros(4, 77, 8), torch.zeros(2, 77, 8)
    good = torch.zeros(4, 4, 8, 8)
    cases = [
        (dict(context=ctx1, guidance_scale=None, mode="invert", noise_maps=good), "denoising loop"),
        (dict(context=ctx1, guidance_scale=None, noise_maps=good), "guidance"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=good, uncond_list=[torch.zeros(1, 77, 8)] * 4), "null-text"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=good, source_trajectory=good), "Direct Inversion"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=torch.zeros(4, 4, 8, 4)), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=torch.zeros(4, 1, 4, 8, 8)), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=torch.zeros(5, 4, 8, 8)), "5 rows for a schedule of 4 steps with skip 0"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=good, skip=1), "4 rows for a schedule of 4 steps with skip 1"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=good, skip=4), "skip"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=good, skip=-1), "skip"),
        (dict(context=ctx2, guidance_scale=7.5, noise_maps=good.double()), "fp32"),
        (dict(context=ctx2, guidance_scale=(3.5, 15.0, 7.5), noise_maps=good), "3 guidance scales for 2 batch rows"),
        (dict(context=ctx2, guidance_scale=(3.5,), noise_maps=good), "1 guidance scales for 2 batch rows"),
        (dict(context=ctx2, guidance_scale=7.5, skip=1), "skip"),
    ]
    for kw, words in cases:
        with pytest.raises(ValueError, match=words):
            FusedDenoiser(model, kw.pop("context"), 2, (8, 8), kw.pop("guidance_scale"), **kw)
    ok = dict(mode="denoise", cfg=True, uncond_list=None, source_trajectory=None, row_shape=(4, 8, 8), num_steps=4)
    check_noise_maps(good, skip=0, guidance_scale=(3.5, 15.0), num_latents=2, **ok)                # the good ones pass
    check_noise_maps(good[1:], skip=1, guidance_scale=7.5, num_latents=2, **ok)
    with pytest.raises(ValueError, match="CFG split.*DDPM inversion"):
        CfgSplitDenoiser(model, ctx2, 2, (8, 8), 7.5, noise_maps=good)
    for fn in (FusedDenoiser.__init__, acquire):
        p = inspect.signature(fn).parameters
        assert p["noise_maps"].default is None and p["skip"].default == 0


def test_presence_of_maps_and_skip_join_the_pool_key_and_nothing_else_moves():
    probe = FusedDenoiser.__new__(FusedDenoiser)
    model = _model()
    probe.unet, probe.sched, probe.mode, probe.cfg, probe.Bp = model.unet, model.scheduler, "denoise", True, 2
    probe.lat = torch.empty(0, 0, 8, 8)
    ctx = torch.zeros(4, 77, 8)
    maps = torch.zeros(4, 4, 8, 8)
    plain, with_maps = probe._key(ctx, None), probe._key(ctx, None, None, maps)
    assert plain != with_maps and with_maps == probe._key(ctx, None, None, torch.ones(4, 4, 8, 8), 0)
    assert probe._key(ctx, None, None, maps[1:], 1) != with_maps, "skip is part of the key"
    assert plain == probe._key(ctx, None, None, None, 0)
    traj = probe._key(ctx, None, maps)
    assert traj != plain and traj != with_maps
    # without maps the new fields are constants, in front of the key-split setting (which stays last)
    assert plain[-3:-1] == (False, 0) and traj[-3:-1] == (False, 0) and with_maps[-3:-1] == (True, 0)
    assert with_maps[:-3] == plain[:-3] and with_maps[-1] == plain[-1] == 1


def test_samplers_take_noise_maps_and_refuse_the_mutual_exclusions():
    from ief_amd.p2p.model.sd_utils import P2P, P2P_XL
    for fn in (P2P.text2image_ldm_stable, P2P_XL.text2image_ldm_stable):
        p = inspect.signature(fn).parameters
        assert p["noise_maps"].default is None and p["skip"].default == 0
    assert "ddpm" in inspect.signature(P2P.diffusion_step).parameters
    model = _model()
    editor = P2P(model, 4)
    maps = torch.zeros(4, 4, 8, 8)
    with pytest.raises(ValueError, match="ONE of"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, uncond_embeddings_list=[torch.zeros(1, 77, 8)] * 4, noise_maps=maps)
    with pytest.raises(ValueError, match="ONE of"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, source_trajectory=maps, noise_maps=maps)
    with pytest.raises(ValueError, match="low_resource"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, noise_maps=maps, low_resource=True)
    with pytest.raises(ValueError, match="CFG split"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, noise_maps=maps, cfg_split_group=object())
    with pytest.raises(ValueError, match="skip"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, skip=2)
    with pytest.raises(ValueError, match="one scale per prompt needs noise_maps"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, guidance_scale=(3.5, 15.0))


# ------------------------------------------------------------------------------------------------------------- the scripts
def _load(folder, script, name):
    """a script loaded the way `python <script>` finds its neighbours, under a private module name"""
    bare = ("_bootstrap", "edit_real", "test")
    saved_path = list(sys.path)
    saved_mods = {k: sys.modules.pop(k) for k in bare if k in sys.modules}
    try:
        sys.path[:0] = [folder]
        spec = importlib.util.spec_from_file_location(name, os.path.join(folder, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved_path
        for k in bare:
            sys.modules.pop(k, None)
        sys.modules.update(saved_mods)
    return mod


def test_pie_driver_parser_ddpm_flags_defaults_and_errors(capsys):
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    drv = _load(P2P_DIR, "test.py", "_host_ddpm_p2p_test")
    assert drv.DDPMInversion is DDPMInversion
    args = drv.parse_args(["--inversion_type", "ddpm", "--invert_batch", "4", "--in_flight", "2"])
    assert (args.inversion_type, args.invert_batch, args.in_flight) == ("ddpm", 4, 2)
    assert (args.ddpm_guidance_src, args.ddpm_guidance_tar, args.skip, args.seed) == (3.5, 15.0, 18, 42)
    assert args.skip / 50 == 0.36, "--skip 18 is 36 % of the 50 steps"
    assert args.ddpm == dict(guidance_src=3.5, guidance_tar=15.0, skip=18, rows_per_launch=4, seed=42)
    assert drv.parse_args(["--inversion_type", "ddpm", "--skip", "0", "--seed", "7"]).ddpm["seed"] == 7
    assert drv.parse_args(["--inversion_type", "ddim"]).ddpm is None and drv.parse_args([]).seed == 42
    for argv, word in ((["--nti_batch", "2"], "--nti_batch"), (["--sd_version", "smallxl"], "smallxl"),
                       (["--sd_version", "xl-base"], "xl-base"), (["--skip", "50"], "--skip"), (["--skip", "-1"], "--skip")):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(["--inversion_type", "ddpm"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    assert drv.parse_args(["--inversion_type", "ddpm", "--skip", "49"]).skip == 49
    assert drv.parse_args(["--inversion_type", "null-text", "--nti_batch", "2"]).nti_batch == 2      # as before
    assert drv.parse_args(["--inversion_type", "ddim", "--skip", "77"]).skip == 77, "the flags bind only with ddpm"


def test_edit_real_parser_ddpm_flags_and_errors(capsys):
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    real = _load(P2P_DIR, "edit_real.py", "_host_ddpm_p2p_edit_real")
    assert real.DDPMInversion is DDPMInversion
    args = real.parser.parse_args(["--inversion_type", "ddpm"])
    assert (args.ddpm_guidance_src, args.ddpm_guidance_tar, args.skip, args.seed, args.invert_batch) == (3.5, 15.0, 18, 42, 4)
    assert real.check_ddpm_arguments(real.parser, args) == dict(guidance_src=3.5, guidance_tar=15.0, skip=18, rows_per_launch=4, seed=42)
    assert real.check_ddpm_arguments(real.parser, real.parser.parse_args([])) is None
    for argv in (["--skip", "50"], ["--skip", "-3"], ["--sd_version", "smallxl"]):
        with pytest.raises(SystemExit) as e:
            real.check_ddpm_arguments(real.parser, real.parser.parse_args(["--inversion_type", "ddpm"] + argv))
        assert e.value.code == 2 and argv[0] in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------------------- the binding
def test_entry_points_are_in_the_binding_derived_from_the_header():
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    want = {"ief_cfg_ddpm_step_f32": (I, [P, P, P, P, P, P, P, LL, LL, P, I, P, P]),
            "ief_ddpm_noise_maps_f32": (I, [P, P, P, P, P, P, I, LL, P])}
    lib = hip.load()
    for name, (res, args) in want.items():
        assert cabi.functions[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the step is the rectifying sibling's prototype with g_rows in front of n
    sib = cabi.functions["ief_cfg_ddim_step_rect_f32"][1]
    assert want["ief_cfg_ddpm_step_f32"][1] == sib[:6] + [P] + sib[6:]
    assert len(cabi.structs) == 10 and lib.ief_abi_version() == 4 and cabi.defines["IEF_ABI_VERSION"] == 4
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(name in text for name in want)


def test_bindings_refuse_host_tensors():
    z = torch.zeros(2, 4, 8, 8)
    step = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError):
        hip.cfg_ddpm_step(z, z, z, torch.zeros(4), torch.zeros(2), torch.zeros(3, 4, 8, 8), step)
    with pytest.raises(TypeError):
        hip.ddpm_noise_maps(z, z, z, z, torch.zeros(2, 5))
    p = inspect.signature(hip.cfg_ddpm_step).parameters
    assert list(p) == ["eps_u", "eps_c", "x", "coef", "g_rows", "noise", "step", "out", "x0_out"]
    assert list(inspect.signature(hip.ddpm_noise_maps).parameters) == ["eps_u", "eps_c", "x_t", "x_prev", "coef_rows", "out"]
