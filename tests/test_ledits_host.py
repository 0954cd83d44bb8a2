"""CPU: the host side of LEDITS++ -- the rank table of the pinned quantile, the smoothing taps, the token windows, the per-step scale
table, every argparse / `ValueError` refusal, the entry points in the binding derived from the header, the plan's signature and pool
key, and the torch fp32 restatement of the three rules (`tests/ledits_ref.py`) that `tests/test_gpu_ledits.py` compares the kernels
with bit for bit.

The restatement's threshold against `torch.quantile` in fp64: |t - t64| <= 4 * 2^-24 * v_(hi) -- the fraction, the difference, the
product and the sum are rounded operations on non-negative values with v_(lo) <= t <= v_(hi), each within 2^-24 v_(hi)."""
import ctypes
import importlib.util
import inspect
import os
import sys
import types

import pytest
import torch

import ledits_ref as ref
from ief_amd import cabi, control, hip
from ief_amd.control import (ControlPlan, StepCounter, check_ledits, ledits_rank, ledits_rank_table, ledits_scale_table, ledits_taps,
                             ledits_token_weights)
from ief_amd.denoise import CfgSplitDenoiser, FusedDenoiser, acquire, cfg_shared_prefix_reason, check_ledits_loop
from ief_amd.scheduler import DDIMScheduler
from ief_amd.tokenizer import WordPieceTokenizer as CLIPTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDITS_DIR = os.path.join(ROOT, "image-editing-framework_amd", "ledits")
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------- host tables
@pytest.mark.parametrize("n", [256, 1024, 4096])
@pytest.mark.parametrize("q", [0.0, 0.5, 0.9, 1.0])
def test_rank_table_is_q_times_n_minus_1(q, n):
    lo, frac = ledits_rank(q, n)
    pos = q * (n - 1)
    assert isinstance(lo, int) and 0 <= lo <= n - 1 and 0.0 <= frac < 1.0
    assert abs((lo + frac) - pos) <= 2.0 ** -24, (lo, frac, pos)
    assert lo == int(pos) and frac == float(torch.tensor(pos - int(pos), dtype=torch.float64).float())
    if q == 1.0:
        assert (lo, frac) == (n - 1, 0.0)
    if q == 0.0:
        assert (lo, frac) == (0, 0.0)
    tab = ledits_rank_table([q, q], n)
    assert tab.dtype == torch.float32 and tab.shape == (2, 2) and tab[0].tolist() == [float(lo), frac]


def test_rank_refuses_thresholds_outside_0_1():
    for q in (-0.01, 1.01, 2):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            ledits_rank(q, 256)


def test_taps_sum_to_one_and_are_the_gaussian():
    t = ledits_taps()
    assert t.dtype == torch.float32 and t.shape == (9,)
    assert abs(t.double().sum().item() - 1.0) <= 2.0 ** -23
    k = t.reshape(3, 3)
    assert torch.equal(k, k.t()) and torch.equal(k, k.flip(0)) and k[1, 1] == k.max()
    assert abs(k[1, 0].item() / k[1, 1].item() - torch.exp(torch.tensor(-2.0, dtype=torch.float64)).item()) < 1e-6     # sigma 0.5


def test_token_windows_of_one_word_and_three_word_concepts():
    from ief_amd.ledits.model.sd_utils import concept_token_counts
    tok = CLIPTokenizer()
    counts = concept_token_counts(tok, ["hat", "a red hat"])
    assert counts == [1, 3]
    w = ledits_token_weights(counts)
    assert w.shape == (2, 2, control.XL) and w.dtype == torch.float32
    assert (w[:, 0] == 0).all(), "u = 0: there is no source row"
    assert w[0, 1].nonzero().flatten().tolist() == [1] and w[1, 1].nonzero().flatten().tolist() == [1, 2, 3]
    assert (w[:, 1, 0] == 0).all(), "BOS is outside the window"
    with pytest.raises(ValueError, match="no tokens"):
        concept_token_counts(tok, ["hat", ""])
    with pytest.raises(ValueError):
        ledits_token_weights([0])
    with pytest.raises(ValueError):
        ledits_token_weights([76])


def test_scale_table_warmup_cooldown_and_a_reversed_concept():
    tab = ledits_scale_table(6, [5.0, 7.0, 2.0], reverse=[1], warmup=[2, 0, 0], cooldown=[None, 3, None])
    assert tab.dtype == torch.float32 and tab.shape == (7, 3)
    assert tab[:, 0].tolist() == [0, 0, 5, 5, 5, 5, 0], "warm-up 2: off in steps 0 and 1; the row past the schedule is 0"
    assert tab[:, 1].tolist() == [-7, -7, -7, 0, 0, 0, 0], "reversed, cool-down 3: off from step 3 on"
    assert tab[:, 2].tolist() == [2, 2, 2, 2, 2, 2, 0]
    both = ledits_scale_table(6, [5.0], warmup=2, cooldown=3)
    assert both[:, 0].tolist() == [0, 0, 5, 0, 0, 0, 0]
    assert ledits_scale_table(4, [5.0, 6.0], warmup=1)[:, 1].tolist() == [0, 6, 6, 6, 0], "one value serves every concept"
    for bad in (dict(reverse=[2]), dict(warmup=[1, 2, 3]), dict(warmup=-1), dict(cooldown=[-1, 0])):
        with pytest.raises(ValueError):
            ledits_scale_table(4, [5.0, 6.0], **bad)


# ------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n", [256, 1024, 1536])
@pytest.mark.parametrize("q", [0.0, 0.5, 0.9, 0.123, 1.0])
def test_restated_threshold_against_torch_quantile_in_fp64(q, n):
    v = torch.rand(n, generator=torch.Generator().manual_seed(n + int(1000 * q))) * 3.0
    lo, frac = ledits_rank(q, n)
    t, vlo, vhi = ref.quantile_threshold(v, lo, frac)
    t64 = torch.quantile(v.double(), q).item()
    assert t.dtype == torch.float32 and vlo <= t <= vhi
    err, bound = abs(t.item() - t64), 4 * U * vhi.item()
    print(f"q = {q}, n = {n}: |t - t64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    bits = v >= t
    assert int(bits.sum()) == n - lo - (1 if frac != 0 else 0), "distinct values: the count of set elements"


def test_restated_attention_mask_reflects_at_the_border():
    acc = torch.rand(2, 256, generator=torch.Generator().manual_seed(0)) + 0.5
    acc[0, 0], acc[1, 255] = 50.0, 50.0                # peaks at the cells (0, 0) and (15, 15)
    taps = ledits_taps()
    m1, sm, ts = ref.attn_mask(acc, taps, ledits_rank_table([0.9, 0.9], 256))
    img = sm.reshape(2, 16, 16)
    k = taps.reshape(3, 3)
    a = acc.reshape(2, 16, 16)
    # cell (0, 0) of a reflected image sees (1, 1) at its four corners, (0, 1) and (1, 0) twice each
    want = ((k[0, 0] * a[0, 1, 1] + k[0, 1] * a[0, 1, 0]) + k[0, 2] * a[0, 1, 1])
    want = ((want + k[1, 0] * a[0, 0, 1]) + k[1, 1] * a[0, 0, 0]) + k[1, 2] * a[0, 0, 1]
    want = ((want + k[2, 0] * a[0, 1, 1]) + k[2, 1] * a[0, 1, 0]) + k[2, 2] * a[0, 1, 1]
    assert img[0, 0, 0] == want
    assert m1[0, 0] == 1 and m1[1, 255] == 1 and set(m1.unique().tolist()) == {0.0, 1.0}
    assert int(m1[0].sum()) == 256 - 229 - 1                       # 0.9 * 255 = 229.5
    all_set, _, _ = ref.attn_mask(acc, taps, ledits_rank_table([0.0, 0.0], 256))
    assert (all_set == 1).all()
    maxima, sm, _ = ref.attn_mask(acc, taps, ledits_rank_table([1.0, 1.0], 256))
    assert torch.equal(maxima, (sm == sm.max(1, keepdim=True).values).float())


def test_restated_guidance_mask_and_step_rules():
    g = torch.Generator().manual_seed(3)
    eps = torch.randn(3, 4, 32, 48, generator=g)
    m1 = (torch.rand(2, 256, generator=g) > 0.5).float()
    n = 32 * 48
    full, ts, s = ref.guidance_mask(eps, None, ledits_rank_table([0.9, 0.5], n))
    assert [int(full[e].sum()) for e in range(2)] == [n - ledits_rank(0.9, n)[0] - 1, n - ledits_rank(0.5, n)[0] - 1]
    both, ts2, s2 = ref.guidance_mask(eps, m1, ledits_rank_table([0.9, 0.2], n))
    sp = ref.spread(m1, 32, 48)
    assert sp.shape == (2, 32, 48) and sp[0, 3, 5] == m1[0, 1 * 16 + 1] and sp[1, 31, 47] == m1[1, 255]
    assert ((both == 1) <= (sp == 1)).all(), "the mask lies inside the cell mask"
    assert ts2[1] == 0 and torch.equal(both[1], sp[1]), "a rank inside the zeros: t = 0 and every pixel under m1 is set"
    only_m1, none, _ = ref.guidance_mask(eps, m1, None)
    assert none is None and torch.equal(only_m1, sp)
    # the step: E = 1 without a mask is CFG; zero scales leave eps_u; outside the masks nothing moves
    coef = torch.tensor([0.55, 0.71, 0.3, 0.4])
    x, z = torch.randn(4, 32, 48, generator=g), torch.randn(4, 32, 48, generator=g)
    out1, _ = ref.ddpm_step(eps[:2], None, torch.tensor([7.5]), x, coef, z)
    e = eps[0] + torch.tensor(7.5) * (eps[1] - eps[0])
    sb, sa, st = torch.sqrt(torch.tensor(1.0) - coef[0]), torch.sqrt(coef[0]), torch.sqrt(coef[1])
    assert torch.equal(out1, (st * ((x - sb * e) / sa) + coef[3] * e) + coef[2] * z)
    zero, _ = ref.ddpm_step(eps, both, torch.zeros(2), x, coef, z)
    out, _ = ref.ddpm_step(eps, both, torch.tensor([5.0, -3.0]), x, coef, z)
    outside = (both.sum(0) == 0)[None].expand_as(out)
    assert torch.equal(out[outside], zero[outside]) and not torch.equal(out, zero)
    gated, _ = ref.ddpm_step(eps, both, torch.tensor([5.0, 0.0]), x, coef, z)
    nan_eps = eps.clone()
    nan_eps[2] = float("nan")
    assert torch.equal(ref.ddpm_step(nan_eps, both, torch.tensor([5.0, 0.0]), x, coef, z)[0], gated), "a gated concept is skipped"


# ------------------------------------------------------------------------------------------------------------- the binding
def test_entry_points_are_in_the_binding_derived_from_the_header():
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    want = {"ief_ledits_attn_mask_f32": (I, [P, P, P, P, I, P]),
            "ief_ledits_guidance_mask_f32": (I, [P, P, P, P, P, I, I, I, I, P]),
            "ief_ledits_ddpm_step_f32": (I, [P, P, P, P, P, P, P, LL, LL, P, I, P, I, P])}
    lib = hip.load()
    for name, (res, args) in want.items():
        assert cabi.functions[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert len(cabi.structs) == 10 and lib.ief_abi_version() == 4, "flat arguments: no struct joins the ABI"
    for fn in (hip.ledits_attn_mask, hip.ledits_guidance_mask, hip.ledits_ddpm_step):
        assert callable(fn) and "ief_ledits_" in fn.__doc__
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert all(name in text for name in want), doc


# ------------------------------------------------------------------------------------------------------------- ValueErrors
def _model(S=4):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    unet = types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(in_channels=4), _plan=None,
                                 cfg=types.SimpleNamespace(addition_embed=False, sample_size=16), attention_modules=lambda: [])
    return types.SimpleNamespace(unet=unet, scheduler=sched)


def _plan(E=2, steps=4, cross=False, intersect=True, hw=(16, 16), modules=(3, 5, 7, 9, 11), thresholds=None):
    return ControlPlan(StepCounter(), "ledits", "cpu", num_steps=steps,
                       ledits=dict(scale=ledits_scale_table(steps, [5.0] * E), thresholds=thresholds or [0.9] * E, token_counts=[1] * E,
                                   cross_mask=cross, intersect_mask=intersect, modules=modules, latent_hw=hw, channels=4))


def test_check_ledits_names_every_refusal():
    check_ledits(1, [0.0, 1.0])
    check_ledits(8, [0.9])
    for kw, words in ((dict(sdxl=True), "SDXL"), (dict(cfg_split=True), "two-GPU CFG split"), (dict(uncond_list=[1]), "null-text"),
                      (dict(source_trajectory=torch.zeros(1)), "source_trajectory"), (dict(edit_mask=torch.zeros(1)), "edit_mask"),
                      (dict(controller=True), "controller")):
        with pytest.raises(ValueError, match=words):
            check_ledits(2, [0.9, 0.9], **kw)
    for E in (0, 9, -1, 2.0):
        with pytest.raises(ValueError, match="1 .. 8"):
            check_ledits(E)
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            check_ledits(2, [0.5, q])
    with pytest.raises(ValueError, match="1 .. 8"):
        _plan(E=9)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        _plan(thresholds=[0.9, 1.2])
    with pytest.raises(ValueError, match="16384"):
        _plan(hw=(144, 128))


def test_the_loop_refuses_bad_combinations_before_touching_the_device():
    model = _model()
    plan = _plan()
    model.unet._plan = plan
    ctx, maps = torch.zeros(3, 77, 8), torch.zeros(4, 4, 16, 16)
    ok = dict(context=ctx, guidance_scale=None, noise_maps=maps, ledits=plan)
    cases = [
        (dict(ok, guidance_scale=7.5), "guidance_scale stays None"),
        (dict(ok, noise_maps=None), "noise maps"),
        (dict(ok, uncond_list=[torch.zeros(1, 77, 8)] * 4), "null-text"),
        (dict(ok, source_trajectory=maps), "source_trajectory"),
        (dict(ok, edit_mask=torch.ones(16, 16)), "edit_mask"),
        (dict(ok, added_cond_kwargs={"text_embeds": torch.zeros(3, 8), "time_ids": torch.zeros(3, 6)}), "SDXL"),
        (dict(ok, context=torch.zeros(2, 77, 8)), "3 rows"),
        (dict(ok, noise_maps=maps[1:]), "3 rows for a schedule of 4 steps"),
        (dict(ok, noise_maps=maps[1:], skip=1), "covers 4 edit steps"),
        (dict(ok, mode="invert"), "denoising loop"),
        (dict(ok, ledits=object()), "ControlPlan"),
        (dict(ok, ledits=_plan()), "controller"),                                 # a plan that is not the registered one
    ]
    for kw, words in cases:
        kw = dict(kw)
        with pytest.raises(ValueError, match=words):
            FusedDenoiser(model, kw.pop("context"), 1, (16, 16), kw.pop("guidance_scale"), **kw)
    with pytest.raises(ValueError, match="ONE latent"):
        FusedDenoiser(model, ctx, 2, (16, 16), None, noise_maps=maps, ledits=plan)
    with pytest.raises(ValueError, match="lowered for latents"):
        FusedDenoiser(model, ctx, 1, (8, 8), None, noise_maps=torch.zeros(4, 4, 8, 8), ledits=plan)
    with pytest.raises(ValueError, match="ledits=plan"):
        FusedDenoiser(model, torch.zeros(2, 77, 8), 1, (16, 16), 7.5)                 # the plan is registered, the loop does not say so
    check_ledits_loop(plan, unet_plan=plan, mode="denoise", guidance_scale=None, uncond_list=None, source_trajectory=None, edit_mask=None,
                      noise_maps=maps, skip=0, row_shape=(4, 16, 16), num_steps=4, num_latents=1, context_rows=3)
    with pytest.raises(ValueError, match="CFG split"):
        CfgSplitDenoiser(model, torch.zeros(2, 77, 8), 1, (16, 16), 7.5, group=types.SimpleNamespace())
    for fn in (FusedDenoiser.__init__, acquire, FusedDenoiser.rebind, FusedDenoiser._key):
        assert inspect.signature(fn).parameters["ledits"].default is None


def test_signature_pool_key_and_shared_prefix_reason():
    model = _model()
    a, b = _plan(cross=False), _plan(cross=False)
    assert a.signature(model.unet) == b.signature(model.unet) == ("ledits", 2, 4, False, True, (), (16, 16))
    sigs = {p.signature(model.unet) for p in (a, _plan(E=3), _plan(intersect=False), _plan(cross=True), _plan(cross=True, modules=(1, 2, 3, 4, 5)),
                                              _plan(steps=3), _plan(hw=(32, 32)))}
    assert len(sigs) == 7, "E, the mask mode, the module indices, the steps and the size are baked into a captured graph"
    assert a.batch == 3 and a.num_prompts == 2
    probe = FusedDenoiser.__new__(FusedDenoiser)
    probe.unet, probe.sched, probe.mode, probe.cfg, probe.Bp = model.unet, model.scheduler, "denoise", False, 1
    probe.lat = torch.empty(0, 0, 16, 16)
    ctx, maps = torch.zeros(3, 77, 8), torch.zeros(4, 4, 16, 16)
    model.unet._plan = a
    probe.ledits = a
    key = probe._key(ctx, None, None, maps, 0, None, a)
    assert key[-1] == "ledits" and a.signature(model.unet) in key
    model.unet._plan = _plan(intersect=False)
    assert probe._key(ctx, None, None, maps, 0, None, model.unet._plan) != key
    facts = dict(mode="denoise", cfg=True, x3p=True, aug=False, first_block_cross=True, native=True, fused_cross=True, ln_folded=False,
                 plan_on_first_self=False)
    assert cfg_shared_prefix_reason(**facts) is None
    assert "LEDITS++" in cfg_shared_prefix_reason(ledits=True, **facts)
    # load_from: a pooled plan takes the next job's tables
    c = _plan(thresholds=[0.5, 0.25])
    a.load_from(c, 3)
    assert torch.equal(a.led["rank_pix"], c.led["rank_pix"]) and torch.equal(a.led["scale"], c.led["scale"])


def test_sampler_refuses_by_name_and_the_cross_mask_outside_its_path():
    from ief_amd.ledits.model import sd_utils
    from ief_amd.ledits.model.sd_utils import LEDITS, lower_ledits
    model = _model()
    model.tokenizer = CLIPTokenizer()
    editor = LEDITS(model, 4)
    x0 = torch.zeros(1, 4, 16, 16)
    for kw, words in ((dict(cfg_split_group=object()), "two-GPU CFG split"), (dict(uncond_embeddings_list=[1]), "null-text"),
                      (dict(source_trajectory=x0), "source_trajectory"), (dict(edit_mask=x0[0, 0]), "edit_mask"),
                      (dict(controller=object()), "controller"), (dict(edit_threshold=1.5), r"\[0, 1\]"),
                      (dict(edit_threshold=[0.5, -0.5]), r"\[0, 1\]")):
        with pytest.raises(ValueError, match=words):
            editor(model, x0, ["hat", "glasses"], **kw)
    with pytest.raises(ValueError, match="1 .. 8"):
        editor(model, x0, [])
    with pytest.raises(ValueError, match="1 .. 8"):
        editor(model, x0, ["a"] * 9)
    model.unet._plan = object()
    with pytest.raises(ValueError, match="controller"):
        editor(model, x0, ["hat"])
    model.unet._plan = None
    model.unet.cfg.addition_embed = True
    with pytest.raises(ValueError, match="SDXL"):
        editor(model, x0, ["hat"])
    model.unet.cfg.addition_embed = False
    # the cross-attention mask stands where LocalBlend's fused form stands
    five = [(8, 40, 256)] * 5
    assert control.ledits_cross_mask_refusal("f16x3", True, five, (64, 64)) is None
    assert "f16x3" in control.ledits_cross_mask_refusal("f16", False, five, (64, 64))
    assert "f16x3" in control.ledits_cross_mask_refusal("f32", False, five, (64, 64))
    assert "queries" in control.ledits_cross_mask_refusal("f16x3", True, five[:4], (64, 64))
    assert "queries" in control.ledits_cross_mask_refusal("f16x3", True, [(8, 40, 64)] * 5, (64, 64))
    assert "heads" in control.ledits_cross_mask_refusal("f16x3", True, [(8, 36, 256)] * 5, (64, 64))
    assert "multiple" in control.ledits_cross_mask_refusal("f16x3", True, five, (24, 24))
    model.unet.precision, model.unet.x3p = "f16", False
    real = sd_utils.blend_modules
    sd_utils.blend_modules = lambda unet: []
    try:
        with pytest.raises(ValueError, match="f16x3 mode only"):
            lower_ledits(model.unet, 4, [1], 5.0, cross_attn_mask=True)
    finally:
        sd_utils.blend_modules = real
    plan = lower_ledits(model.unet, 4, [1, 3], [5.0, 7.0], reverse=[1], thresholds=0.9, warmup=[1, 0], cross_attn_mask=False)
    assert plan.kind == "ledits" and plan.led["E"] == 2 and not plan.led["cross"] and plan.led["intersect"]
    assert plan.led["scale"][:, 1].tolist() == [-7, -7, -7, -7, 0] and plan.led["scale"][:, 0].tolist() == [0, 5, 5, 5, 0]
    assert plan.led["rank_pix"].tolist() == [[229.0, 0.5]] * 2 and plan.led["w"][1, 1, 1:4].tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------------------------------------- the scripts
def _load(script, name):
    """a script loaded the way `python <script>` finds its neighbours, under a private module name"""
    bare = ("_bootstrap", "edit_real", "test")
    saved_path = list(sys.path)
    saved_mods = {k: sys.modules.pop(k) for k in bare if k in sys.modules}
    try:
        sys.path[:0] = [LEDITS_DIR]
        spec = importlib.util.spec_from_file_location(name, os.path.join(LEDITS_DIR, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved_path
        for k in bare:
            sys.modules.pop(k, None)
        sys.modules.update(saved_mods)
    return mod


BAD_ARGV = [(["--sd_version", "smallxl"], "smallxl"), (["--sd_version", "xl-base"], "xl-base"),
            (["--edit_prompt"] + ["a"] * 9, "1 .. 8"), (["--edit_threshold", "1.5"], "--edit_threshold"),
            (["--edit_threshold", "-0.1"], "--edit_threshold"), (["--edit_prompt", "a", "b", "--edit_threshold", "0.5", "0.6", "0.7"], "--edit_threshold"),
            (["--edit_prompt", "a", "b", "--edit_guidance_scale", "1", "2", "3"], "--edit_guidance_scale"),
            (["--edit_warmup_steps", "-1"], "--edit_warmup_steps"), (["--edit_cooldown_steps", "-2"], "--edit_cooldown_steps"),
            (["--remove", "1"], "--remove"), (["--skip", "50"], "--skip"), (["--skip", "-1"], "--skip"), (["--invert_batch", "0"], "--invert_batch"),
            (["--cfg_split"], "unrecognized"), (["--in_flight", "2"], "unrecognized"), (["--inversion_type", "nti"], "unrecognized")]


def test_edit_real_parser_flags_defaults_and_errors(capsys):
    real = _load("edit_real.py", "_host_ledits_edit_real")
    args = real.parser.parse_args([])
    assert (args.edit_guidance_scale, args.remove, args.edit_threshold, args.edit_warmup_steps, args.edit_cooldown_steps) == (
        [5.0], [], [0.9], [0], None)
    assert (args.source_prompt, args.source_guidance_scale, args.skip, args.invert_batch, args.seed, args.mask_save_dir) == (
        "", 3.5, 7, 4, 42, None)
    assert not args.no_cross_attn_mask and not args.no_intersect_mask
    kw = real.check_ledits_arguments(real.parser, args, 1)
    assert kw == dict(edit_guidance_scale=[5.0], reverse=[], edit_threshold=[0.9], edit_warmup_steps=[0], edit_cooldown_steps=None,
                      source_guidance_scale=3.5, skip=7, cross_attn_mask=True, intersect_mask=True, rows_per_launch=4)
    assert set(kw) <= set(inspect.signature(real.LEDITS.__call__).parameters)
    args = real.parser.parse_args(["--edit_prompt", "glasses", "a hat", "--remove", "1", "--edit_guidance_scale", "5", "7",
                                   "--no_cross_attn_mask", "--no_intersect_mask", "--edit_cooldown_steps", "30"])
    kw = real.check_ledits_arguments(real.parser, args, 2)
    assert kw["reverse"] == [1] and kw["edit_guidance_scale"] == [5.0, 7.0] and kw["edit_cooldown_steps"] == [30]
    assert not kw["cross_attn_mask"] and not kw["intersect_mask"]
    for argv, word in BAD_ARGV:
        with pytest.raises(SystemExit) as e:
            real.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_pie_driver_parser_errors(capsys):
    drv = _load("test.py", "_host_ledits_test")
    for argv, word in BAD_ARGV:
        with pytest.raises(SystemExit) as e:
            drv.main(["--synthetic", "2"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    capsys.readouterr()
