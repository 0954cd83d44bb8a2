"""`register_attention_control(model, controller)` / `unregister_attention_control(model, controller)`.

Same entry points and side effects as `/root/reference/p2p/model/register.py:3-117`:
  - every module named 'Attention' under the UNet children whose names contain "down" / "up" /
    "mid" is attached to the controller, counted, and `controller.num_att_layers` is set (:78-98);
  - `controller is None` installs a pass-through controller (:67-76);
  - unregister restores the modules and zeroes `num_att_layers` (:100-117).

Two ways a controller is attached:

  lowered (fused)   for the controller classes whose arithmetic is known — `EmptyControl`,
      `AttentionReplace`, `AttentionRefine`, `AttentionReweight` from this package OR the reference's
      own classes of the same names (duck-typed on their attributes) — `lower_controller` turns
      the controller into a `control.ControlPlan` (device tables); `Attention.forward` stays the
      native fused kernel path and reads the plan.  No attention map is materialised.
  generic           anything else (user subclasses, `AttentionStore`, a `LocalBlend` where `blend_refusal` names a reason):
      `Attention.forward` is replaced by a closure with the reference's dataflow
      (register.py:11-64): Q/K/V projections -> materialised maps -> `controller(maps, is_cross,
      place)` in Python (in place on the cond half) -> maps x V -> out-projection.

An edit controller with a `LocalBlend` is lowered too (f16x3 on the operand-planes path): the blend reads the EDITED maps of five
16 x 16 cross-attention modules summed over the blend words, which is linear in the two softmax rows the edit mixes, so the plan
carries per-step weight vectors instead of maps (`blend_weights`) and two small kernels do the rest (csrc/local_blend.hip).

`fused=False` forces the generic path for a lowerable controller (used by the parity tests
that hold both paths to identical results).
"""
from typing import Optional

import torch

from ... import control
from ...control import ControlPlan, XL

_LOWERABLE = {"EmptyControl", "DummyController", "AttentionReplace", "AttentionRefine", "AttentionReweight"}


class DummyController:
    def __call__(self, *args):
        return args[0]

    def __init__(self):
        self.num_att_layers = 0
        self.cur_step = 0
        self.cur_att_layer = 0

    def between_steps(self):
        return None


def _attention_modules(unet):
    """(place, module) in the reference's registration order."""
    out = []
    for name, child in unet.named_children():
        place = "down" if "down" in name else "up" if "up" in name else "mid" if "mid" in name else None
        if place is None:
            continue
        out += [(place, m) for m in child.modules() if m.__class__.__name__ == "Attention"]
    return out


# --------------------------------------------------------------------------------------- lowering
def _edit_tables(c):
    """(M [slots,77,77] fp32, scale1 [slots,77], keep_tgt [slots,77]) such that
    replace_cross_attention(P_src, P_tgt) == (P_src @ M) * scale1 + P_tgt * keep_tgt."""
    name = type(c).__name__
    if name == "AttentionReplace":
        M = c.mapper.detach().float().cpu()
        slots = M.shape[0]
        return M, torch.ones(slots, 77), torch.zeros(slots, 77)
    if name == "AttentionRefine":
        mapper = c.mapper.detach().cpu().long()
        a = c.alphas.detach().float().cpu().reshape(mapper.shape[0], 77)
        slots = mapper.shape[0]
        M = torch.zeros(slots, 77, 77)
        cols = torch.arange(77)
        for s in range(slots):
            M[s, mapper[s] % 77, cols] = 1.0  # column n gathers source word mapper[n]; -1 wraps like torch indexing
        return M, a, 1.0 - a
    if name == "AttentionReweight":
        eq = c.equalizer.detach().float().cpu()
        prev = getattr(c, "prev_controller", None)
        if prev is None:
            slots = eq.shape[0]
            return torch.eye(77).repeat(slots, 1, 1), eq.clone(), torch.zeros(slots, 77)
        M, s1, keep = _edit_tables(prev)
        return M, s1 * eq, keep * eq
    raise TypeError(name)


def _cross_queries(unet):
    """{id(module): queries} of every cross-attention module at the UNet's configured sample size"""
    out, res = {}, int(unet.cfg.sample_size)

    def visit(block):
        out.update((id(m), res * res) for m in block.modules() if m.__class__.__name__ == "Attention" and m.is_cross)

    for blk in unet.down_blocks:
        visit(blk)
        if blk.downsamplers is not None:
            res //= 2
    visit(unet.mid_block)
    for blk in unet.up_blocks:
        visit(blk)
        if blk.upsamplers is not None:
            res *= 2
    return out


def blend_modules(unet):
    """the cross-attention modules whose maps `LocalBlend.__call__` reads, `down_cross[2:4] + up_cross[:3]` of the store: per
    place the modules with <= 32^2 queries (at the configured sample size) in registration order -> [(module, queries)]"""
    queries = _cross_queries(unet)
    stored = {"down": [], "mid": [], "up": []}
    for place, m in _attention_modules(unet):
        if m.is_cross and id(m) in queries and queries[id(m)] <= 32 ** 2:
            stored[place].append((m, queries[id(m)]))
    return stored["down"][2:4] + stored["up"][:3]


def blend_refusal(controller, rows, precision, x3p, modules):
    """the host part of the decision to lower a controller's `LocalBlend`: None, or the reason it takes the generic path.
    modules: (heads, head dim, queries) of the modules `blend_modules` names"""
    lb = controller.local_blend
    if precision != "f16x3" or not x3p:
        return "the fused blend runs on the operand-planes path of the f16x3 mode only"
    if rows != "all":
        return f'rows = "{rows}": the blend needs the whole CFG batch on one device'
    if getattr(controller, "LOW_RESOURCE", False):
        return "LOW_RESOURCE runs two half-batch forwards per step, which keep the Python protocol"
    layers = getattr(lb, "alpha_layers", None)
    if not isinstance(layers, torch.Tensor) or layers.shape[0] != controller.batch_size or layers.numel() != controller.batch_size * 77:
        got = None if not isinstance(layers, torch.Tensor) else tuple(layers.shape)
        return f"alpha_layers {got} does not hold one row of 77 words for each of the {controller.batch_size} prompts"
    if len(modules) != 5 or any(N != ControlPlan.MAP_TOKENS for _, _, N in modules):
        return (f"the modules LocalBlend reads have {[N for _, _, N in modules]} queries at the UNet's configured sample size, not "
                f"five times {ControlPlan.MAP_TOKENS}")
    for heads, d, _ in modules:
        if heads > 64 or d % 8:
            return f"a module LocalBlend reads has {heads} heads of dim {d} (at most 64 heads, head dim a multiple of 8)"
    th = lb.threshold
    if not (isinstance(th, (int, float)) and 0 < th < 1):
        return f"threshold = {th!r} is outside (0, 1)"
    return None


def blend_weights(coef, M, alpha_layers):
    """fp32 [steps+1, Bp, 2, XL] = (u_i, v_i) per step: with the edited map P'_i[n] = c1[n] sum_w P_src[w] M[w][n] + c2[n] P_i[n]
    and a_i the blend words of prompt row i,  sum_n a_i[n] P'_i[n] = P_src . u_i + P_i . v_i  where
    u_i[w] = sum_n a_i[n] c1[n] M[w][n] and v_i[n] = a_i[n] c2[n]; the source row has u_0 = 0, v_0 = a_0.
    coef fp32 [steps+1, slots, 2, XL] (the plan's coef_table), M fp32 [slots, 77, 77], alpha_layers [Bp, ..., 77]"""
    steps1, slots = coef.shape[0], coef.shape[1]
    a = alpha_layers.detach().float().cpu().reshape(slots + 1, 77)
    w = torch.zeros(steps1, slots + 1, 2, XL)
    w[:, 0, 1, :77] = a[0]
    for s in range(slots):
        c1, c2 = coef[:, s, 0, :77], coef[:, s, 1, :77]
        w[:, s + 1, 0, :77] = (a[s + 1] * c1) @ M[s].t()
        w[:, s + 1, 1, :77] = a[s + 1] * c2
    return w


def lower_controller(controller, device, rows: str = "all", unet=None) -> Optional[ControlPlan]:
    """ControlPlan for a known controller class, else None (generic path).
    unet: needed only to lower a controller's `LocalBlend` (which modules it reads, the arithmetic mode).
    rows: which rows of the CFG batch this UNet runs — "all" ([uncond..., cond...], the reference's batch), "cond" (only
    the conditional rows: the half every controller acts on) or "uncond" (only the unconditional rows: nothing to edit,
    the plan just keeps the controller's counters moving).  "cond" / "uncond" are the two ranks of a 2-GPU CFG split."""
    if rows not in ("all", "cond", "uncond"):
        raise ValueError('rows must be "all", "cond" or "uncond"')
    name = type(controller).__name__
    if name not in _LOWERABLE:
        return None
    blend = None
    if name not in ("EmptyControl", "DummyController") and getattr(controller, "local_blend", None) is not None:
        mods = blend_modules(unet) if unet is not None else []
        why = blend_refusal(controller, rows, getattr(unet, "precision", None), getattr(unet, "x3p", False),
                            [(m.heads, m.dim_head, N) for m, N in mods])
        if why is not None:
            print(f"LocalBlend takes the generic path: {why}")
            return None
        blend = tuple(m._exec_index for m, _ in mods)
    if getattr(controller, "LOW_RESOURCE", False):
        return None  # two half-batch forwards per step: keep the Python protocol
    if name in ("EmptyControl", "DummyController") or rows == "uncond":
        return ControlPlan(controller, "empty", device)
    try:
        M, s1, keep = _edit_tables(controller)
    except (TypeError, AttributeError):
        return None
    alpha = controller.cross_replace_alpha.detach().float().cpu()  # [steps+1, slots, 1, 1, 77]
    steps1, slots = alpha.shape[0], alpha.shape[1]
    alpha = alpha.reshape(steps1, slots, 77)
    if M.shape[0] != slots or controller.batch_size != slots + 1:
        return None
    # P' = alpha * ((P_src M) s1 + P_tgt keep) + (1 - alpha) P_tgt
    c1 = alpha * s1[None]
    c2 = alpha * keep[None] + (1.0 - alpha)
    coef = torch.zeros(steps1, slots, 2, XL)
    coef[:, :, 0, :77], coef[:, :, 1, :77] = c1, c2
    mt = torch.zeros(slots, XL, XL)
    mt[:, :77, :77] = M.transpose(1, 2)
    lo, hi = controller.num_self_replace
    if blend is not None:
        blend = (blend, blend_weights(coef, M, controller.local_blend.alpha_layers), controller.local_blend.threshold)
    return ControlPlan(controller, "p2p", device, num_prompts=slots + 1, num_steps=steps1 - 1, mt=mt, coef_table=coef,
                       self_window=(int(lo), int(hi)), cond_only=(rows == "cond"), blend=blend)


# --------------------------------------------------------------------------------------- generic hook
def _generic_forward(attn, controller, place_in_unet):
    """Closure with the dataflow of `/root/reference/p2p/model/register.py:11-64` on our kernels."""
    to_out = attn.to_out[0] if isinstance(attn.to_out, torch.nn.ModuleList) else attn.to_out

    def forward(hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None):
        is_cross = encoder_hidden_states is not None
        query = attn.to_q(hidden_states)
        context = encoder_hidden_states if is_cross else hidden_states
        key, value = attn.to_k(context), attn.to_v(context)
        probs = attn.get_attention_scores(attn.head_to_batch_dim(query), attn.head_to_batch_dim(key), None)
        probs = controller(probs, is_cross, place_in_unet)
        out = attn.apply_probs(probs, attn.head_to_batch_dim(value))
        return to_out(out)

    return forward


def register_attention_control(model, controller, fused: Optional[bool] = None, rows: str = "all"):
    """`rows` (not a reference argument): see `lower_controller`; anything but "all" needs a lowerable controller"""
    if controller is None:
        controller = DummyController()
    unet = model.unet
    mods = _attention_modules(unet)
    plan = None
    if fused is not False and all(getattr(m, "is_native", None) is not None for _, m in mods):
        plan = lower_controller(controller, unet.device, rows, unet)
    if rows != "all" and plan is None:
        raise ValueError(f"{type(controller).__name__} cannot be lowered: a CFG-split forward needs a device plan")
    if fused is True and plan is None:
        raise ValueError(f"{type(controller).__name__} cannot be lowered to the fused path")
    for place, m in mods:
        if plan is not None:
            m.__dict__.pop("forward", None)      # back to the native fused forward
            m._plan = plan
        else:
            m._plan = None
            if "forward" not in m.__dict__:
                m._original_forward = m.forward
            m.forward = _generic_forward(m, controller, place)
    unet._plan = plan
    if getattr(controller, "local_blend", None) is not None:
        # where the blend was lowered, `step_callback` blends on the device from this plan's accumulator
        controller._device_blend = plan if plan is not None and plan.blend_w is not None else None
    controller.num_att_layers = len(mods)
    return controller


def unregister_attention_control(model, controller):
    unet = model.unet
    for _, m in _attention_modules(unet):
        m.__dict__.pop("forward", None)
        m.__dict__.pop("_original_forward", None)
        m._plan = None
    unet._plan = None
    if controller is not None:
        controller.num_att_layers = 0
        if getattr(controller, "_device_blend", None) is not None:
            controller._device_blend = None
