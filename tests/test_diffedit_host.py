"""CPU: DiffEdit's host side -- the three entry points in the binding derived from the header, every `ValueError` of
`check_edit_mask`, the pool key, the index rules of the two strengths, the order of the partial trajectory, the argparse errors of both
CLIs, and rule 1 (the mask) restated in torch fp64, which tests/test_gpu_diffedit.py compares the kernels with.

The restatement (`mask_rule`): for eps_t, eps_s [n, C, h, w]
    d[p] = 1 / (n C) sum_j sum_c |eps_t - eps_s|;   clamp = ratio mean_p d;   v = min(max(d, 0), clamp) / clamp;   M = v > thres
with 0 / 0 = NaN comparing false.  `mask_case` builds the inputs the GPU file uses: d = g s with g unit Gaussian, s = 1 inside the
centred rectangle [int(0.3125 h), int(0.6875 h)) x [int(0.3125 w), int(0.6875 w)) (0.375 of each side) and 0.25 outside; a unit
Gaussian, b = a + d in fp32."""
import ctypes
import importlib.util
import inspect
import os
import sys
import types

import pytest
import torch

from ief_amd import cabi, hip
from ief_amd.denoise import CfgSplitDenoiser, FusedDenoiser, acquire, check_edit_mask
from ief_amd.scheduler import DDIMScheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIFFEDIT_DIR = os.path.join(ROOT, "image-editing-framework_amd", "diffedit")
MASK_SIZES = [(8, 8), (7, 9), (64, 64), (96, 96)]
FOREGROUND = {(8, 8): 9, (7, 9): 8, (64, 64): 576, (96, 96): 1296}


# ------------------------------------------------------------------------------------------------------------- rule 1, in fp64
def mask_rule(eps_t, eps_s, ratio=3.0, thres=0.5, dtype=torch.float64):
    """-> (mask bool [h, w], v [h, w], d [h, w]) in `dtype`"""
    n, C = eps_t.shape[:2]
    d = (eps_t.to(dtype) - eps_s.to(dtype)).abs().sum((0, 1)) / (n * C)
    return mask_from_map(d, ratio, thres)


def mask_from_map(d, ratio=3.0, thres=0.5):
    clamp = ratio * d.mean()
    v = torch.minimum(d.clamp(min=0), clamp) / clamp
    return v > thres, v, d


def mask_case(h, w, seed, R=10, C=4):
    """-> (a, b) fp32 [R, C, h, w] and the rectangle bool [h, w]"""
    g = torch.Generator().manual_seed(seed)
    rect = torch.zeros(h, w, dtype=torch.bool)
    rect[int(0.3125 * h):int(0.6875 * h), int(0.3125 * w):int(0.6875 * w)] = True
    s = torch.where(rect, torch.tensor(1.0), torch.tensor(0.25))
    d = torch.randn(R, C, h, w, generator=g) * s
    a = torch.randn(R, C, h, w, generator=g)
    return a, a + d, rect


@pytest.mark.parametrize("hw", MASK_SIZES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mask_rule_on_the_cases_the_gpu_file_uses(hw, seed):
    a, b, rect = mask_case(*hw, seed)
    mask, v, _ = mask_rule(b, a)
    gap = (v - 0.5).abs().min().item()
    print(f"{hw[0]} x {hw[1]} seed {seed}: {int(mask.sum())} foreground pixels, smallest |v - 0.5| = {gap:.3e}")
    assert int(rect.sum()) == FOREGROUND[hw] and torch.equal(mask, rect), "the mask is the rectangle"
    assert gap >= 1e-4
    assert mask.any() and not mask.all()


def test_mask_rule_zero_difference_is_a_zero_mask():
    a, _, _ = mask_case(8, 8, 0)
    mask, v, d = mask_rule(a, a)
    assert (d == 0).all() and torch.isnan(v).all() and not mask.any()


# ------------------------------------------------------------------------------------------------------------- the binding
def test_entry_points_are_in_the_binding_derived_from_the_header():
    P, LL, I, F = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_float
    want = {"ief_cfg_ddim_step_masked_f32": (I, [P, P, P, P, P, P, LL, LL, LL, P, I, P, P, P]),
            "ief_diffedit_map_accum_f32": (I, [P, P, P, I, I, I, P]),
            "ief_diffedit_mask_f32": (I, [P, P, I, I, F, F, P])}
    lib = hip.load()
    for name, (res, args) in want.items():
        assert cabi.functions[name] == (res, args)
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # the masked step is the rectifying sibling's prototype with hw behind row_elems and the mask in front of the stream
    sib = cabi.functions["ief_cfg_ddim_step_rect_f32"][1]
    assert want["ief_cfg_ddim_step_masked_f32"][1] == sib[:8] + [LL] + sib[8:-1] + [P] + sib[-1:]
    assert len(cabi.structs) == 10 and lib.ief_abi_version() == 4 and cabi.defines["IEF_ABI_VERSION"] == 4
    for fn in (hip.diffedit_map_accum, hip.diffedit_mask):
        assert callable(fn)
    assert inspect.signature(hip.cfg_ddim_step).parameters["masked"].default is None
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert all(name in text for name in want)


# ------------------------------------------------------------------------------------------------------------- ValueErrors
def _model(S=4):
    sched = DDIMScheduler()
    sched.set_timesteps(S)
    unet = types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(in_channels=4), _plan=None)
    return types.SimpleNamespace(unet=unet, scheduler=sched)


def test_check_edit_mask_and_the_loops_refuse_bad_arguments_before_touching_the_device():
    model, ctx2, ctx1 = _model(), torch.zeros(4, 77, 8), torch.zeros(2, 77, 8)
    mask, traj3, traj4 = torch.ones(2, 8, 8), torch.zeros(3, 4, 8, 8), torch.zeros(4, 4, 8, 8)
    cases = [
        (dict(context=ctx1, guidance_scale=None, mode="invert", edit_mask=mask, source_trajectory=traj4), "denoising loop"),
        (dict(context=ctx1, guidance_scale=None, edit_mask=mask, source_trajectory=traj4), "guidance"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4, uncond_list=[torch.zeros(1, 77, 8)] * 4),
         "null-text"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4, noise_maps=traj4), "DDPM inversion"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask.double(), source_trajectory=traj4), "fp32 or bool"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask.to(torch.int32), source_trajectory=traj4), "fp32 or bool"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=[[1.0]], source_trajectory=traj4), "fp32 or bool"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=torch.ones(3, 8, 8), source_trajectory=traj4), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=torch.ones(2, 8, 4), source_trajectory=traj4), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=torch.ones(2, 1, 8, 8), source_trajectory=traj4), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask), "needs the source_trajectory"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4.double()), "fp32"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=torch.zeros(4, 4, 8, 4)), "trajectory rows of shape"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4, skip=1),
         "4 trajectory rows for a schedule of 4 steps with skip 1"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj3), "3 trajectory rows for a schedule of 4 steps with skip 0"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4, skip=4), "skip"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4, skip=-1), "skip"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4, skip=True), "skip"),
        (dict(context=ctx2, guidance_scale=7.5, edit_mask=mask, source_trajectory=traj4,
              added_cond_kwargs={"text_embeds": torch.zeros(4, 8), "time_ids": torch.zeros(4, 6)}), "SD1.x"),
        # without a mask the older messages stand
        (dict(context=ctx2, guidance_scale=7.5, skip=1), "skip: only a loop with noise maps"),
        (dict(context=ctx2, guidance_scale=7.5, source_trajectory=traj3), "3 rows for a schedule of 4 steps"),
    ]
    for kw, words in cases:
        with pytest.raises(ValueError, match=words):
            FusedDenoiser(model, kw.pop("context"), 2, (8, 8), kw.pop("guidance_scale"), **kw)
    ok = dict(mode="denoise", cfg=True, uncond_list=None, noise_maps=None, row_shape=(4, 8, 8), num_steps=4, num_latents=2)
    check_edit_mask(mask, source_trajectory=traj4, skip=0, **ok)                         # the good ones pass
    check_edit_mask(mask[0] > 0, source_trajectory=traj3, skip=1, **ok)                  # bool, [h, w] for every row
    check_edit_mask(mask, source_trajectory=traj4[:1], skip=3, **ok)
    with pytest.raises(ValueError, match="CFG split.*DiffEdit"):
        CfgSplitDenoiser(model, ctx2, 2, (8, 8), 7.5, edit_mask=mask, source_trajectory=traj4)
    for fn in (FusedDenoiser.__init__, acquire, CfgSplitDenoiser.__init__, FusedDenoiser.rebind, FusedDenoiser._key):
        assert inspect.signature(fn).parameters["edit_mask"].default is None


def test_presence_of_a_mask_and_its_skip_join_the_pool_key():
    probe = FusedDenoiser.__new__(FusedDenoiser)
    model = _model()
    probe.unet, probe.sched, probe.mode, probe.cfg, probe.Bp = model.unet, model.scheduler, "denoise", True, 2
    probe.lat = torch.empty(0, 0, 8, 8)
    ctx, traj, mask = torch.zeros(4, 77, 8), torch.zeros(4, 4, 8, 8), torch.ones(2, 8, 8)
    plain, direct = probe._key(ctx, None), probe._key(ctx, None, traj)
    masked = probe._key(ctx, None, traj, None, 0, mask)
    assert len({plain, direct, masked}) == 3, "loops with and without a mask never share a pool entry"
    assert masked == probe._key(ctx, None, traj, None, 0, torch.zeros(8, 8)), "the mask's values and form are not part of the key"
    assert masked != probe._key(ctx, None, traj[1:], None, 1, mask), "its skip is"
    assert plain == probe._key(ctx, None, None, None, 0, None)


# ------------------------------------------------------------------------------------------------------------- index rules, trajectory
def test_strength_index_rules():
    from ief_amd.diffedit.model.sd_utils import strength_index
    want = {(50, 0.5): 25, (50, 0.8): 10, (50, 1.0): 0, (4, 0.5): 2, (4, 0.8): 1, (4, 1.0): 0, (1, 1.0): 0}
    for (S, s), i in want.items():
        assert strength_index(S, s) == i == S - int(S * s), (S, s)
    for S, s in ((1, 0.5), (1, 0.8), (4, 0.2)):          # S - int(S s) == S: no timestep at that index, no step to run
        with pytest.raises(ValueError, match="leaves no step"):
            strength_index(S, s)
    for s in (0.0, -0.1, 1.01):
        with pytest.raises(ValueError, match=r"\(0, 1\]"):
            strength_index(50, s)


def test_trajectory_order_on_fake_latents():
    from ief_amd.diffedit.model import sd_utils
    from ief_amd.p2p.inversion import direct
    assert sd_utils._trajectory is direct._trajectory, "the convention of Direct Inversion, not a fork of it"
    S, skip = 5, 1
    latents = [torch.full((1, 4, 2, 3), float(k)) for k in range(S - skip + 1)]          # z*_0 ... z*_{S-skip}
    rows = sd_utils.trajectory(latents)
    assert rows.shape == (S - skip, 4, 2, 3) and rows.dtype == torch.float32 and rows.is_contiguous()
    assert [float(r[0, 0, 0]) for r in rows] == [3.0, 2.0, 1.0, 0.0], "row i = z*_{S-skip-1-i}; the last row is x0, the start is no row"
    with pytest.raises(ValueError):
        sd_utils.trajectory([torch.zeros(2, 4, 2, 3)] * 3)
    check_edit_mask(torch.ones(2, 3), mode="denoise", cfg=True, uncond_list=None, noise_maps=None, source_trajectory=rows,
                    row_shape=(4, 2, 3), num_steps=S, skip=skip, num_latents=1)


def test_mask_from_image_nearest_and_threshold(tmp_path):
    import numpy as np
    from PIL import Image
    from ief_amd.diffedit.model.sd_utils import mask_from_image
    arr = np.zeros((16, 16), dtype=np.uint8)
    arr[:8, :8], arr[8:, 8:] = 255, 127          # 127 / 255 < 0.5
    arr[8:, :8] = 128                            # 128 / 255 >= 0.5
    Image.fromarray(arr).save(tmp_path / "m.png")
    for src in (str(tmp_path / "m.png"), tmp_path / "m.png", Image.fromarray(arr)):
        m = mask_from_image(src, (4, 4))
        assert m.dtype == torch.float32 and m.shape == (4, 4)
        assert m[:2, :2].eq(1).all() and m[2:, :2].eq(1).all() and m[:2, 2:].eq(0).all() and m[2:, 2:].eq(0).all()


def test_diffedit_refuses_hooks_plans_and_sdxl():
    from ief_amd.diffedit.model.sd_utils import DiffEdit
    model = _model()
    model.unet.attention_modules = lambda: [types.SimpleNamespace(is_native=lambda: False)]
    editor = DiffEdit(model, 4)
    x0 = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="attention hook or control plan"):
        editor.infer_mask(model, x0, "a", ["b"])
    model.unet.attention_modules = lambda: []
    model.unet._plan = object()
    with pytest.raises(RuntimeError, match="attention hook or control plan"):
        editor(model, x0, "a", ["b"])
    model.unet._plan = None
    model.unet.cfg = types.SimpleNamespace(addition_embed=True)
    with pytest.raises(ValueError, match="SDXL"):
        editor.infer_mask(model, x0, "a", ["b"])
    sig = inspect.signature(DiffEdit.infer_mask).parameters
    assert (sig["num_maps"].default, sig["strength_mask"].default, sig["ratio"].default, sig["threshold"].default) == (10, 0.5, 3.0, 0.5)
    assert inspect.signature(DiffEdit.__call__).parameters["strength"].default == 0.8


# ------------------------------------------------------------------------------------------------------------- the scripts
def _load(script, name):
    """a script loaded the way `python <script>` finds its neighbours, under a private module name"""
    bare = ("_bootstrap", "edit_real", "test")
    saved_path = list(sys.path)
    saved_mods = {k: sys.modules.pop(k) for k in bare if k in sys.modules}
    try:
        sys.path[:0] = [DIFFEDIT_DIR]
        spec = importlib.util.spec_from_file_location(name, os.path.join(DIFFEDIT_DIR, script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path[:] = saved_path
        for k in bare:
            sys.modules.pop(k, None)
        sys.modules.update(saved_mods)
    return mod


BAD_ARGV = [(["--sd_version", "smallxl"], "smallxl"), (["--sd_version", "xl-base"], "xl-base"), (["--strength", "0"], "--strength"),
            (["--strength", "1.2"], "--strength"), (["--strength_mask", "0"], "--strength_mask"),
            (["--strength_mask", "-0.5"], "--strength_mask"), (["--num_maps", "0"], "--num_maps"), (["--mask_batch", "0"], "--mask_batch")]


def test_edit_real_parser_flags_defaults_and_errors(capsys):
    real = _load("edit_real.py", "_host_diffedit_edit_real")
    args = real.parser.parse_args([])
    assert (args.num_maps, args.mask_batch, args.strength, args.strength_mask, args.mask_ratio, args.seed, args.mask) == (
        10, 10, 0.8, 0.5, 3.0, 42, None)
    assert real.check_diffedit_arguments(real.parser, args) == dict(strength=0.8, guidance_scale=7.5, num_maps=10, rows_per_launch=10,
                                                                     strength_mask=0.5, ratio=3.0)
    assert real.parser.parse_args(["--mask", "m.png", "--strength", "1.0"]).mask == "m.png"
    for argv, word in BAD_ARGV:
        with pytest.raises(SystemExit) as e:
            real.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_pie_driver_parser_errors(capsys):
    drv = _load("test.py", "_host_diffedit_test")
    for argv, word in BAD_ARGV:
        with pytest.raises(SystemExit) as e:
            drv.main(["--synthetic", "2"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
    with pytest.raises(SystemExit):
        drv.main(["--invert_batch", "2"])          # out of scope for this folder: not a flag
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------------------- plans per row
def test_plans_per_row_plans_a_launch_as_one_of_its_rows():
    """what makes `rows_per_launch` a schedule in f16: inside the context the fp16-storage front-end plans M = rows x tokens as
    tokens, so tile and split-K count do not follow the batch (`small`'s shapes: they do otherwise)"""
    shapes = [(256, 640, 5760, True), (256, 640, 2560, False), (1024, 320, 8640, True)]
    assert hip._plan_m(2560) == 2560
    by_batch = {b: [hip.pick_plan(hip._plan_m(b * t), N, K, conv=c)[:2] for t, N, K, c in shapes] for b in (2, 4, 10)}
    assert len({tuple(v) for v in by_batch.values()}) > 1, "planned by the batch, the split-K counts differ"
    for b in (2, 4, 10):
        with hip.plans_per_row(b):
            assert [hip.pick_plan(hip._plan_m(b * t), N, K, conv=c) for t, N, K, c in shapes] == [
                hip.pick_plan(t, N, K, conv=c) for t, N, K, c in shapes]
            assert hip._plan_m(b * 77) == 77 and hip._plan_m(b * 77 + 1) == b * 77 + 1, "only whole rows"
            with hip.plans_per_row(1):
                assert hip._plan_m(b * 256) == b * 256
            assert hip._plan_m(b * 256) == 256, "nested contexts restore"
    assert hip._plan_m(2560) == 2560
    with pytest.raises(RuntimeError):
        with hip.plans_per_row(4):
            raise RuntimeError("inside")
    assert hip._plan_m(1024) == 1024, "restored when the body raises"
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            hip.plans_per_row(bad)
