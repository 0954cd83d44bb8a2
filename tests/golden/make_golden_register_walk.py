"""Golden record of the reference's registration walks over OUR module tree, made by IMPORTING the reference's own
`p2p/model/register.py` and `masactrl/model/register.py` and running them on the repo's TINY UNet (CPU, synthetic weights):
which modules each walk patched (qualified name, in the order it counted them), the place (`down` / `mid` / `up`) it handed
to the hooked forward, the layer count it stored on the controller, and that its unregister left every module native again.
The reference checkout is an argument (it is not part of this repository):

    python tests/golden/make_golden_register_walk.py <reference checkout>   ->  tests/golden/register_walk.json   (G16)
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import ief_amd  # noqa: E402,F401
from ief_amd import config, weights  # noqa: E402
from ief_amd.unet import UNet2DConditionModel  # noqa: E402

PLACES = ("down", "mid", "up")


def _place(m):
    """the place string the hooked forward closes over"""
    cells = [c.cell_contents for c in (m.__dict__["forward"].__closure__ or ())]
    found = [c for c in cells if isinstance(c, str) and c in PLACES]
    assert len(found) == 1, found
    return found[0]


def _record(unet, register, unregister, controller):
    from types import SimpleNamespace
    model = SimpleNamespace(unet=unet)
    register(model, controller)
    patched = [{"name": n, "place": _place(m)} for n, m in unet.named_modules() if "forward" in m.__dict__]
    count = controller.num_att_layers
    unregister(model, controller)
    native = all(m.is_native() for m in unet.attention_modules())
    count_after = controller.num_att_layers
    for m in unet.modules():                       # leave the tree as it was for the next walk
        m.__dict__.pop("forward", None)
        m.__dict__.pop("_original_forward", None)
    return {"patched": patched, "num_att_layers": count, "native_after_unregister": native,
            "num_att_layers_after_unregister": count_after}


def main(ref):
    unet = UNet2DConditionModel(config.TINY, weights.synthetic_state_dict(config.TINY, 0), device="cpu")
    out = {"config": "tiny", "weights_seed": 0}

    spec = importlib.util.spec_from_file_location("ref_p2p_register", os.path.join(ref, "p2p", "model", "register.py"))
    p2p = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(p2p)

    class Ctl:
        num_att_layers = -1

        def __call__(self, attn, is_cross, place):
            return attn
    out["p2p"] = _record(unet, p2p.register_attention_control, p2p.unregister_attention_control, Ctl())

    sys.path.insert(0, os.path.join(ref, "masactrl"))       # its register.py imports `model.attention_base`
    spec = importlib.util.spec_from_file_location("ref_masa_register", os.path.join(ref, "masactrl", "model", "register.py"))
    masa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(masa)
    out["masactrl"] = _record(unet, masa.regiter_attention_editor_diffusers, masa.unregister_attention_control,
                              masa.AttentionBase())

    path = os.path.join(HERE, "register_walk.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {k: v["num_att_layers"] for k, v in out.items() if isinstance(v, dict)})


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
