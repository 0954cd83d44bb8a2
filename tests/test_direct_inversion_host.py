"""CPU: Direct Inversion's host side -- the entry point in the header and the library, the order of `trajectory()`, the
`--inversion_type direct` value of the p2p / masactrl scripts, and the argument checks of `FusedDenoiser` that need no device."""
import ctypes
import importlib.util
import os
import sys
import types

import pytest
import torch

from ief_amd import cabi, hip
from ief_amd.denoise import CfgSplitDenoiser, FusedDenoiser, check_source_trajectory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-editing-framework_amd")
P2P, MASA = os.path.join(PKG, "p2p"), os.path.join(PKG, "masactrl")
NAME = "ief_cfg_ddim_step_rect_f32"


def test_header_declares_the_entry_point_and_the_library_exports_it():
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    want = (ctypes.c_int, [P, P, P, P, P, P, LL, LL, P, I, P, P])
    assert cabi.functions[NAME] == want
    # the sibling's prototype is the same up to the four new arguments
    sib = cabi.functions["ief_cfg_ddim_step_f32"]
    assert sib[1][:7] == want[1][:7] and len(sib[1]) == 8
    lib = hip.load()
    fn = getattr(lib, NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[1]
    assert lib.ief_abi_version() == 4 and cabi.defines["IEF_ABI_VERSION"] == 4


def test_binding_takes_rect_and_refuses_host_tensors():
    import inspect
    assert inspect.signature(hip.cfg_ddim_step).parameters["rect"].default is None
    z = torch.zeros(2, 4, 8, 8)
    with pytest.raises(TypeError):
        hip.cfg_ddim_step(z, z, z, torch.zeros(3), rect=(torch.zeros(3, 4, 8, 8), torch.zeros(1, dtype=torch.int32)))


@pytest.mark.parametrize("xl", [False, True])
def test_trajectory_row_i_is_latent_S_minus_1_minus_i(xl):
    from ief_amd.p2p.inversion.ddim import ddim_inversion, ddim_inversion_xl
    from ief_amd.p2p.inversion.direct import DirectInversion, DirectInversion_XL
    inv = (DirectInversion_XL if xl else DirectInversion)()
    assert isinstance(inv, ddim_inversion_xl if xl else ddim_inversion)
    assert "ddim_inversion_loop" not in type(inv).__dict__, "the inherited loop stays untouched"
    S = 5
    latents = [torch.full((1, 4, 3, 2), float(k)) + torch.arange(24.0).reshape(1, 4, 3, 2) / 100 for k in range(S + 1)]
    rows = inv.trajectory(latents)
    assert rows.shape == (S, 4, 3, 2) and rows.dtype == torch.float32 and rows.is_contiguous()
    for i in range(S):
        assert torch.equal(rows[i], latents[S - 1 - i][0])
    assert torch.equal(rows[-1], latents[0][0]) and not any(torch.equal(r, latents[S][0]) for r in rows)   # z*_0 last, x_T never
    # a batched inversion: the first dimension is per image
    batched = [torch.cat([t, t + 100]) for t in latents]
    rows2 = inv.trajectory(batched)
    assert rows2.shape == (2, S, 4, 3, 2)
    assert torch.equal(rows2[0], rows) and torch.equal(rows2[1], rows + 100)
    with pytest.raises(ValueError):
        inv.trajectory(latents[:1])


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


class _FakeSched:
    timesteps = torch.tensor([3, 2, 1, 0])

    def set_timesteps(self, n):
        self.n = n


class _FakePipe:
    scheduler = _FakeSched()


class StableDiffusionXLPipeline(_FakePipe):       # the scripts dispatch on the class name
    pass


def test_p2p_parsers_accept_direct_and_nti_batch_with_it_errors(capsys):
    drv = _load(P2P, "test.py", "_host_direct_p2p_test")
    args = drv.parse_args(["--inversion_type", "direct", "--invert_batch", "2", "--in_flight", "2"])
    assert (args.inversion_type, args.invert_batch, args.in_flight, args.nti_batch) == ("direct", 2, 2, 1)
    with pytest.raises(SystemExit) as e:
        drv.parse_args(["--inversion_type", "direct", "--nti_batch", "2"])
    assert e.value.code == 2 and "--nti_batch" in capsys.readouterr().err
    assert drv.parse_args(["--inversion_type", "null-text", "--nti_batch", "2"]).nti_batch == 2      # as before
    from ief_amd.p2p.inversion.direct import DirectInversion, DirectInversion_XL
    assert drv.DirectInversion is DirectInversion and drv.DirectInversion_XL is DirectInversion_XL
    real = _load(P2P, "edit_real.py", "_host_direct_p2p_edit_real")
    assert real.parser.parse_args(["--inversion_type", "direct"]).inversion_type == "direct"
    assert real.DirectInversion is DirectInversion


def test_masactrl_parsers_accept_direct_and_pick_dispatches():
    from ief_amd.masactrl.model.sd_utils import MasaCtrl, MasaCtrl_NTI, MasaCtrl_XL, MasaCtrl_XL_NTI
    from ief_amd.p2p.inversion.direct import DirectInversion, DirectInversion_XL
    real = _load(MASA, "edit_real.py", "_host_direct_masa_edit_real")
    assert real.parser.parse_args(["--inversion_type", "direct"]).inversion_type == "direct"
    inv, ed = real.pick(_FakePipe(), "direct", 4)
    assert type(inv) is DirectInversion and type(ed) is MasaCtrl
    inv, ed = real.pick(StableDiffusionXLPipeline(), "direct", 4)
    assert type(inv) is DirectInversion_XL and type(ed) is MasaCtrl_XL
    assert type(real.pick(_FakePipe(), "null-text", 4)[1]) is MasaCtrl_NTI                            # as before
    assert type(real.pick(StableDiffusionXLPipeline(), "null-text", 4)[1]) is MasaCtrl_XL_NTI
    with pytest.raises(ValueError, match="Please choose right inversion type"):
        real.pick(_FakePipe(), "directly", 4)
    drv = _load(MASA, "test.py", "_host_direct_masa_test")
    assert drv.parse_args(["--inversion_type", "direct", "--synthetic", "2"]).inversion_type == "direct"
    assert drv.parse_args([]).inversion_type == "ddim"


def _fake_model():
    unet = types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(in_channels=4), _plan=None)
    return types.SimpleNamespace(unet=unet, scheduler=_FakeSched())


def test_fused_denoiser_rejects_a_bad_trajectory_before_touching_the_device():
    model, ctx2, ctx1 = _fake_model(), torch.zeros(4, 77, 8), torch.zeros(2, 77, 8)
    good = torch.zeros(4, 4, 8, 8)
    cases = [
        (dict(context=ctx1, guidance_scale=None, mode="invert", source_trajectory=good), "denoising loop"),
        (dict(context=ctx1, guidance_scale=None, source_trajectory=good), "guidance"),
        (dict(context=ctx2, guidance_scale=7.5, source_trajectory=torch.zeros(4, 4, 8, 4)), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, source_trajectory=torch.zeros(4, 1, 4, 8, 8)), "shape"),
        (dict(context=ctx2, guidance_scale=7.5, source_trajectory=torch.zeros(5, 4, 8, 8)), "5 rows for a schedule of 4 steps"),
        (dict(context=ctx2, guidance_scale=7.5, source_trajectory=good.double()), "fp32"),
        (dict(context=ctx2, guidance_scale=7.5, source_trajectory=good, uncond_list=[torch.zeros(1, 77, 8)] * 4), "null-text"),
    ]
    for kw, words in cases:
        with pytest.raises(ValueError, match=words):
            FusedDenoiser(model, kw.pop("context"), 2, (8, 8), kw.pop("guidance_scale"), **kw)
    check_source_trajectory(good, mode="denoise", cfg=True, uncond_list=None, row_shape=(4, 8, 8), num_steps=4)    # the good one passes
    with pytest.raises(ValueError, match="CFG split.*Direct Inversion"):
        CfgSplitDenoiser(model, ctx2, 2, (8, 8), 7.5, source_trajectory=good)


def test_presence_of_a_trajectory_joins_the_pool_key():
    probe = FusedDenoiser.__new__(FusedDenoiser)
    model = _fake_model()
    probe.unet, probe.sched, probe.mode, probe.cfg, probe.Bp = model.unet, model.scheduler, "denoise", True, 2
    probe.lat = torch.empty(0, 0, 8, 8)
    ctx = torch.zeros(4, 77, 8)
    a, b = probe._key(ctx, None), probe._key(ctx, None, torch.zeros(4, 4, 8, 8))
    assert a != b and a == probe._key(ctx, None, None) and b == probe._key(ctx, None, torch.ones(4, 4, 8, 8))


def test_samplers_take_source_trajectory_and_refuse_it_with_null_text_embeddings():
    import inspect
    from ief_amd.denoise import acquire
    from ief_amd.masactrl.model.sd_utils import MasaCtrl
    from ief_amd.p2p.model.sd_utils import P2P, P2P_XL
    for fn in (P2P.text2image_ldm_stable, P2P_XL.text2image_ldm_stable, MasaCtrl.__call__, acquire, FusedDenoiser.__init__):
        assert inspect.signature(fn).parameters["source_trajectory"].default is None
    model = _fake_model()
    with pytest.raises(ValueError, match="not both"):
        P2P(model, 4).text2image_ldm_stable(model, ["a", "b"], None, uncond_embeddings_list=[torch.zeros(1, 77, 8)] * 4,
                                            source_trajectory=torch.zeros(4, 4, 8, 8))
