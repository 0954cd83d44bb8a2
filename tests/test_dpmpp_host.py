"""CPU: the host side of the second-order multistep SDE-DPM-Solver++ on the edit-friendly DDPM noise space -- `DDIMScheduler.dpmpp_coeffs`
against its fp64 closed form and the identity with the eta = 1 DDPM coefficients, the order rule as a function of (S, skip), the rule
restated in fp64 (an order-2 step undoes an order-2 extraction), every `ValueError` / `argparse` error of the new keywords and flags,
the pool key, the CLI defaults, and the three entry points in the binding derived from the header.

The rule: with lambda(a) = 1/2 log(a / (1 - a)), h_i = lambda(p_i) - lambda(a_i) and v_i = `ddpm_coeffs`' v = (1 - p_i) (1 - e^{-2 h_i}),
    mu_i = sqrt(p_i) x0_i + dir_i e_i + c2_i (x0_i - x0_{i-1}),    c2_i = 1/2 sqrt(p_i) (v_i / (1 - p_i)) (h_i / h_{i-1})
and c2_i = 0 on the first step run (i = skip), on the last step (i = S - 1) and everywhere at solver order 1."""
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
from ief_amd.denoise import CfgSplitDenoiser, FusedDenoiser, acquire, check_solver_order
from ief_amd.scheduler import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2P_DIR = os.path.join(ROOT, "image-editing-framework_amd", "p2p")
LEDITS_DIR = os.path.join(ROOT, "image-editing-framework_amd", "ledits")


def lam(a):
    a = np.float64(a)
    return 0.5 * np.log(a / (1 - a))


# ------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("S", [4, 5, 20, 50])
def test_dpmpp_coeffs_are_the_ddpm_coefficients_plus_the_closed_form_c2(S):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    ts = sched.timesteps.tolist()
    T = sched.config.num_train_timesteps
    for i, t in enumerate(ts):
        a, p, sigma, dirc = sched.ddpm_coeffs(t)
        one = sched.dpmpp_coeffs(t, False)
        assert one == (a, p, sigma, dirc, 0.0), "order 1: the eta = 1 DDPM coefficients and c2 = 0"
        if i > 0:
            assert sched.step_coeffs(ts[i - 1])[1] == a, "on this scheduler p_{i-1} = a_i"
        # the first-order SDE-DPM-Solver++ coefficients in fp64: sigma_to^2 (1 - e^{-2h}) and sigma_to e^{-h}, sigma_to^2 = 1 - p
        a64, p64 = np.float64(a), np.float64(p)
        h = lam(p64) - lam(a64)
        s2, d2 = (1 - p64) * (1 - np.exp(-2 * h)), (1 - p64) * np.exp(-2 * h)
        # sigma and dir hold fp32 roundings of the square roots: their squares sit within 2 ulp (fp32) of the fp64 values
        assert abs(sigma ** 2 - s2) <= 2 * 2.0 ** -23 * s2 and abs(dirc ** 2 - d2) <= 2 * 2.0 ** -23 * d2
        if i == 0:
            with pytest.raises(ValueError, match="order 1"):
                sched.dpmpp_coeffs(t, True)
            continue
        if i == S - 1 and p64 >= 1.0:
            continue
        two = sched.dpmpp_coeffs(t, True)
        assert two[:4] == (a, p, sigma, dirc), "the first four values are ddpm_coeffs' exactly"
        a_before = np.float64(sched.step_coeffs(ts[i - 1])[0])
        assert ts[i - 1] == t + T // S
        h_before = lam(a64) - lam(a_before)
        v = (1 - p64) / (1 - a64) * (1 - a64 / p64)
        want = 0.5 * np.sqrt(p64) * (v / (1 - p64)) * (h / h_before)
        assert two[4] == float(np.float32(want)), f"S={S} t={t}: c2 is the fp64 closed form rounded to fp32 once"
        assert two[4] > 0
        assert abs(v / (1 - p64) - (1 - np.exp(-2 * h))) <= 1e-12, "ddpm_coeffs' v over 1 - p is 1 - e^{-2h}"


@pytest.mark.parametrize("S,skip", [(4, 0), (5, 0), (5, 1), (20, 0), (20, 7), (50, 18), (50, 7)])
def test_c2_is_zero_on_the_first_step_run_on_the_last_step_and_at_order_1(S, skip):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    two, one = sched.dpmpp_table(skip, 2), sched.dpmpp_table(skip, 1)
    assert len(two) == len(one) == S - skip
    assert all(r[4] == 0.0 for r in one), "order 1: c2 = 0 everywhere"
    assert [r[:4] for r in two] == [r[:4] for r in one] == [sched.ddpm_coeffs(t) for t in sched.timesteps.tolist()[skip:]]
    assert two[0][4] == 0.0 and two[-1][4] == 0.0
    assert all(r[4] > 0 for r in two[1:-1])


def test_the_c2_values_of_the_20_and_50_step_schedules():
    sched = DDIMScheduler()
    sched.set_timesteps(20)
    c2 = {t: r[4] for t, r in zip(sched.timesteps.tolist(), sched.dpmpp_table(0, 2))}
    assert abs(c2[901] - 0.028) < 5e-4 and abs(c2[851] - 0.034) < 5e-4 and abs(c2[101] - 0.41) < 5e-3 and abs(c2[51] - 1.98) < 5e-3
    sched.set_timesteps(50)
    c2 = {t: r[4] for t, r in zip(sched.timesteps.tolist(), sched.dpmpp_table(0, 2))}
    assert abs(c2[961] - 0.0094) < 5e-5 and abs(c2[21] - 1.58) < 5e-3


def test_equal_log_snr_steps_give_half_sqrt_p_v_over_one_minus_p():
    sig = lambda l: 1.0 / (1.0 + np.exp(-2.0 * l))          # a with lambda(a) = l
    for l0, h in ((-2.0, 0.3), (0.1, 0.05), (1.5, 0.7)):
        a_before, a, p = sig(l0), sig(l0 + h), sig(l0 + 2 * h)
        v = (1 - p) / (1 - a) * (1 - a / p)
        want = 0.5 * np.sqrt(p) * v / (1 - p)
        got = DDIMScheduler.dpmpp_c2(a_before, a, p)
        assert abs(got - want) <= 4 * 2.0 ** -24 * want, "h_i = h_{i-1}: c2 = 1/2 sqrt(p) v / (1 - p)"
    for bad in ((0.5, 0.4, 0.6), (0.3, 0.5, 1.0), (0.0, 0.5, 0.6)):
        with pytest.raises(ValueError, match="dpmpp_c2"):
            DDIMScheduler.dpmpp_c2(*bad)


@pytest.mark.parametrize("S,skip", [(2, 0), (3, 0), (4, 0), (4, 1), (4, 3), (5, 1), (20, 7), (50, 18)])
def test_order_rule(S, skip):
    orders = DDIMScheduler.dpmpp_orders(S, skip, 2)
    assert len(orders) == S
    for i, o in enumerate(orders):
        assert o == (2 if skip < i < S - 1 else 1), f"S={S} skip={skip} step {i}"
    assert DDIMScheduler.dpmpp_orders(S, skip, 1) == [1] * S
    for bad in (0, 3, "2"):
        with pytest.raises(ValueError, match="solver_order"):
            DDIMScheduler.dpmpp_orders(S, skip, bad)
    for bad in (-1, S, 1.0):
        with pytest.raises(ValueError, match="skip"):
            DDIMScheduler.dpmpp_orders(S, bad, 2)


# ------------------------------------------------------------------------------------------------------------- the rule, in fp64
@pytest.mark.parametrize("S,skip", [(5, 0), (5, 1), (20, 7)])
def test_rule_in_fp64_the_source_row_reproduces_every_stored_latent(S, skip):
    """extraction (chain-free: x0_{i-1} from row i - 1's own eps) and edit (x0_prev carried from step to step) written out in fp64
    with a toy eps function: the source row walks y_{skip+1} .. y_S = x0, and the order-2 maps differ from the order-1 maps"""
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    ts = sched.timesteps.tolist()
    g = torch.Generator().manual_seed(S + skip)
    x0 = torch.randn(4, 6, generator=g, dtype=torch.float64)
    a = [sched.step_coeffs(t)[0] for t in ts]
    xts = [a_i ** 0.5 * x0 + (1 - a_i) ** 0.5 * torch.randn(4, 6, generator=g, dtype=torch.float64) for a_i in a] + [x0]
    eps = lambda y, t: torch.cos(y + t / 1000.0) * 0.7

    def maps(order):
        coef = [None] * skip + sched.dpmpp_table(skip, order)
        z, x0_prev = {}, None
        for i in range(skip, S):
            a_i, p_i, sigma, dirc, c2 = coef[i]
            e = eps(xts[i], ts[i])
            x0_i = (xts[i] - (1 - a_i) ** 0.5 * e) / a_i ** 0.5
            mu = p_i ** 0.5 * x0_i + dirc * e
            if c2 != 0.0:
                mu = mu + c2 * (x0_i - x0_prev)
            z[i] = (xts[i + 1] - mu) / sigma
            x0_prev = x0_i
        return coef, z

    coef, z = maps(2)
    x, x0_prev = xts[skip], torch.full_like(x0, float("nan"))
    for i in range(skip, S):
        a_i, p_i, sigma, dirc, c2 = coef[i]
        e = eps(x, ts[i])
        x0_i = (x - (1 - a_i) ** 0.5 * e) / a_i ** 0.5
        mu = p_i ** 0.5 * x0_i + dirc * e
        if c2 != 0.0:
            mu = mu + c2 * (x0_i - x0_prev)
        x, x0_prev = mu + sigma * z[i], x0_i
        assert (x - xts[i + 1]).abs().max() <= 1e-11 * max(1.0, xts[i + 1].abs().max()), f"after step {i} the source row is y_{i + 1}"
    _, z1 = maps(1)
    assert torch.equal(z[skip], z1[skip]) and torch.equal(z[S - 1], z1[S - 1]), "rows skip and S - 1 are order 1"
    if S - skip > 2:
        assert all(not torch.equal(z[i], z1[i]) for i in range(skip + 1, S - 1)), "the correction acts on the rows between"


# ------------------------------------------------------------------------------------------------------------- ValueErrors
def _model(S=4, device="cpu"):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    unet = types.SimpleNamespace(device=torch.device(device), config=types.SimpleNamespace(in_channels=4), _plan=None)
    return types.SimpleNamespace(unet=unet, scheduler=sched)


def test_solver_order_is_valid_only_with_noise_maps():
    model, ctx2 = _model(), torch.zeros(4, 77, 8)
    maps = torch.zeros(4, 4, 8, 8)
    check_solver_order(1, None), check_solver_order(1, maps), check_solver_order(2, maps)
    with pytest.raises(ValueError, match="noise maps"):
        check_solver_order(2, None)
    for bad in (0, 3, True, "2", None, 2.5):
        with pytest.raises(ValueError, match="solver_order must be 1 or 2"):
            check_solver_order(bad, maps)
    with pytest.raises(ValueError, match="solver_order=2.*noise maps"):
        FusedDenoiser(model, ctx2, 2, (8, 8), 7.5, solver_order=2)
    with pytest.raises(ValueError, match="solver_order=2.*noise maps"):
        FusedDenoiser(model, ctx2, 2, (8, 8), 7.5, source_trajectory=maps, solver_order=2)
    with pytest.raises(ValueError, match="solver_order=2.*noise maps"):
        acquire(model, ctx2, 2, (8, 8), 7.5, solver_order=2)
    with pytest.raises(ValueError, match="solver_order must be 1 or 2"):
        FusedDenoiser(model, ctx2, 2, (8, 8), 7.5, noise_maps=maps, solver_order=3)
    with pytest.raises(ValueError, match="CFG split.*second-order"):
        CfgSplitDenoiser(model, ctx2, 2, (8, 8), 7.5, solver_order=2)
    with pytest.raises(ValueError, match="CFG split.*second-order"):
        CfgSplitDenoiser(model, ctx2, 2, (8, 8), 7.5, noise_maps=maps, solver_order=2)
    for fn in (FusedDenoiser.__init__, acquire, FusedDenoiser.rebind, CfgSplitDenoiser.__init__):
        assert inspect.signature(fn).parameters["solver_order"].default == 1


def test_samplers_and_the_inversion_take_solver_order_and_refuse_it_without_maps():
    from ief_amd.ledits.model.sd_utils import LEDITS
    from ief_amd.p2p.inversion.ddpm import DDPMInversion
    from ief_amd.p2p.model.sd_utils import P2P
    assert inspect.signature(P2P.text2image_ldm_stable).parameters["solver_order"].default == 1
    assert inspect.signature(DDPMInversion.noise_maps).parameters["solver_order"].default == 1
    assert inspect.signature(LEDITS.__init__).parameters["solver_order"].default == 1
    model = _model()
    editor = P2P(model, 4)
    with pytest.raises(ValueError, match="solver_order=2.*noise maps"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, solver_order=2)
    with pytest.raises(ValueError, match="solver_order must be 1 or 2"):
        editor.text2image_ldm_stable(model, ["a", "b"], None, noise_maps=torch.zeros(4, 4, 8, 8), solver_order=0)
    with pytest.raises(ValueError, match="solver_order must be 1 or 2"):
        LEDITS(model, 4, solver_order=3)
    assert LEDITS(model, 5, solver_order=2).solver_order == 2 and len(model.scheduler.timesteps) == 5
    assert LEDITS(model, 4).solver_order == 1


def test_the_pool_key_separates_the_orders_and_leaves_order_1_keys_as_they_were():
    probe = FusedDenoiser.__new__(FusedDenoiser)
    model = _model()
    probe.unet, probe.sched, probe.mode, probe.cfg, probe.Bp = model.unet, model.scheduler, "denoise", True, 2
    probe.lat = torch.empty(0, 0, 8, 8)
    ctx, maps = torch.zeros(4, 77, 8), torch.zeros(3, 4, 8, 8)
    before = probe._key(ctx, None, None, maps, 1)                       # the call, and the key, every order-1 caller has
    one = probe._key(ctx, None, None, maps, 1, None, None, 1)
    two = probe._key(ctx, None, None, maps, 1, None, None, 2)
    assert one == before and len(before) == 15 and before[-3:] == (True, 1, 1), "order 1: not one field more"
    assert two != one and two[:len(one)] == one, "order 2: the order-1 key and the solver's own field"
    led1 = probe._key(ctx, None, None, maps, 1, None, object())
    led2 = probe._key(ctx, None, None, maps, 1, None, object(), 2)
    assert led1 == before + ("ledits",) and led2 != led1 and led2 != two and led2[:len(led1)] == led1


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


def _exits(fn, argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_p2p_clis_num_steps_solver_order_and_the_skip_default(capsys):
    drv = _load(P2P_DIR, "test.py", "_host_dpmpp_p2p_test")
    real = _load(P2P_DIR, "edit_real.py", "_host_dpmpp_p2p_edit_real")
    assert real.NUM_STEPS == 50
    parse_real = lambda argv: (lambda a: (a, real.check_ddpm_arguments(real.parser, a)))(real.parser.parse_args(argv))
    for parse in (lambda argv: (lambda a: (a, a.ddpm))(drv.parse_args(argv)), parse_real):
        args, ddpm = parse(["--inversion_type", "ddpm"])
        assert (args.num_steps, args.solver_order, args.skip) == (50, 1, 18) and ddpm["skip"] == 18
        assert "num_steps" not in ddpm and "solver_order" not in ddpm, "a default run hands on what it always did"
        args, ddpm = parse(["--inversion_type", "ddpm", "--num_steps", "20", "--solver_order", "2"])
        assert (args.num_steps, args.solver_order, args.skip) == (20, 2, 7) and ddpm["skip"] == 7, "int(0.36 * 20) = 7"
        assert ddpm["num_steps"] == 20 and ddpm["solver_order"] == 2
        assert parse(["--inversion_type", "ddpm", "--num_steps", "20"])[1]["skip"] == 7, "the default follows N at order 1 too"
        assert parse(["--inversion_type", "ddpm", "--num_steps", "20", "--skip", "18"])[1]["skip"] == 18, "a given --skip stays"
        assert parse(["--inversion_type", "ddpm", "--num_steps", "100"])[1]["skip"] == 36
        assert parse(["--inversion_type", "ddpm", "--solver_order", "2"])[1] == dict(
            guidance_src=3.5, guidance_tar=15.0, skip=18, rows_per_launch=args.invert_batch if parse is parse_real else 1, seed=42,
            solver_order=2)
        assert parse(["--inversion_type", "ddpm", "--num_steps", "2"])[1]["skip"] == 0
        assert parse(["--inversion_type", "ddpm", "--num_steps", "1000"])[1]["skip"] == 360
    for fn in (drv.parse_args, lambda argv: real.check_ddpm_arguments(real.parser, real.parser.parse_args(argv))):
        _exits(fn, ["--inversion_type", "ddpm", "--num_steps", "1"], "--num_steps", capsys)
        _exits(fn, ["--inversion_type", "ddpm", "--num_steps", "1001"], "--num_steps", capsys)
        _exits(fn, ["--inversion_type", "ddpm", "--solver_order", "3"], "--solver_order", capsys)
        _exits(fn, ["--inversion_type", "ddpm", "--num_steps", "20", "--skip", "20"], "[0, 20)", capsys)
        _exits(fn, ["--inversion_type", "ddpm", "--num_steps", "20", "--skip", "-1"], "--skip", capsys)
        for other in ("ddim", "null-text", "direct"):
            _exits(fn, ["--inversion_type", other, "--num_steps", "20"], "--inversion_type ddpm", capsys)
            _exits(fn, ["--inversion_type", other, "--solver_order", "2"], "--inversion_type ddpm", capsys)
    assert drv.parse_args(["--inversion_type", "ddim"]).ddpm is None


def test_ledits_clis_num_steps_solver_order_and_the_skip_default(capsys):
    real = _load(LEDITS_DIR, "edit_real.py", "_host_dpmpp_ledits_edit_real")
    drv = _load(LEDITS_DIR, "test.py", "_host_dpmpp_ledits_test")
    assert real.NUM_STEPS == 50 and drv.NUM_STEPS == 50
    check = lambda argv: (lambda a: (a, real.check_ledits_arguments(real.parser, a, 1)))(real.parser.parse_args(argv))
    args, kw = check([])
    assert (args.num_steps, args.solver_order, kw["skip"]) == (50, 1, 7)
    assert set(kw) <= set(inspect.signature(real.LEDITS.__call__).parameters), "steps and order go to the constructor"
    args, kw = check(["--num_steps", "20", "--solver_order", "2"])
    assert (args.num_steps, args.solver_order, kw["skip"]) == (20, 2, 3), "int(0.15 * 20) = 3"
    assert check(["--num_steps", "20", "--skip", "7"])[1]["skip"] == 7, "a given --skip stays"
    assert check(["--solver_order", "2"])[1]["skip"] == 7
    for fn in (lambda argv: check(argv), drv.main):
        _exits(fn, ["--num_steps", "1"], "--num_steps", capsys)
        _exits(fn, ["--num_steps", "1001"], "--num_steps", capsys)
        _exits(fn, ["--solver_order", "0"], "--solver_order", capsys)
        _exits(fn, ["--num_steps", "20", "--skip", "20"], "[0, 20)", capsys)


# ------------------------------------------------------------------------------------------------------------- the binding
def test_entry_points_are_in_the_binding_derived_from_the_header():
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    want = {"ief_cfg_dpmpp_step_f32": (I, [P, P, P, P, P, P, P, P, LL, LL, P, I, P, P]),
            "ief_dpmpp_noise_maps_f32": (I, [P, P, P, P, P, P, P, I, LL, P]),
            "ief_ledits_dpmpp_step_f32": (I, [P, P, P, P, P, P, P, P, LL, LL, P, I, P, I, P])}
    lib = hip.load()
    for name, (res, args) in want.items():
        assert cabi.functions[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # each is its sibling's prototype with x0_prev / x0_carry in front of the coefficients / the row count
    for new, old, at in (("ief_cfg_dpmpp_step_f32", "ief_cfg_ddpm_step_f32", 5), ("ief_dpmpp_noise_maps_f32", "ief_ddpm_noise_maps_f32", 6),
                         ("ief_ledits_dpmpp_step_f32", "ief_ledits_ddpm_step_f32", 6)):
        sib = cabi.functions[old][1]
        assert want[new][1] == sib[:at] + [P] + sib[at:]
    assert lib.ief_abi_version() == 4 and cabi.defines["IEF_ABI_VERSION"] == 4, "the ABI number stays"
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(name in text for name in want) and "solver_order" in text


def test_bindings_refuse_host_tensors_and_wrong_coefficient_widths():
    z = torch.zeros(2, 4, 8, 8)
    step = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError):
        hip.cfg_dpmpp_step(z, z, z, torch.zeros(5), torch.zeros(2), torch.zeros(3, 4, 8, 8), step, z.clone())
    with pytest.raises(TypeError):
        hip.dpmpp_noise_maps(z, z, z, z, torch.zeros(2, 6), torch.zeros(4, 8, 8))
    with pytest.raises(TypeError):
        hip.ledits_dpmpp_step(torch.zeros(3, 4, 8, 8), None, torch.zeros(2), z[:1], torch.zeros(5), torch.zeros(3, 4, 8, 8), step, z[0].clone())
