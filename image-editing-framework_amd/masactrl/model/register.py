"""`regiter_attention_editor_diffusers(model, editor)` (sic) / `unregister_attention_control(model, editor)` —
the hook API of `/root/reference/masactrl/model/register.py:6-89`.

The reference patches every `Attention.forward` with a closure that materialises `sim` and `attn`
([B*heads, N, N]: 2 GiB each in fp32 at 64x64) and hands them to the editor (:35-48).  Here the two editor classes
the reference CLIs use — `AttentionBase` (plain attention) and `MutualSelfAttentionControl` — are lowered to a
device plan: the fused flash-attention kernel takes per-batch K/V source rows, which IS mutual self-attention
(`ief_attn_flash_f16`, k_src / v_src).  `MutualSelfAttentionControlMask` with two binary masks is lowered too where
the planes attention runs (f16x3): the mutual launch plus two launches over gathered row lists (`control.py`,
kind 'masactrl_mask'), and so is `MutualSelfAttentionControlMaskAuto`, whose masks come from the step's own 16 x 16
cross-attention maps: two small kernels make packed class bits on the device and ONE class-masked launch per controlled layer
reads them (kind 'masactrl_mask_auto'), and `MutualSelfAttentionControlUnion`, whose target rows attend over their half's
source keys followed by their own: ONE launch of the planes attention's two-segment form per controlled layer (kind
'masactrl_union').  `lower_editor` prints why when it cannot.  Any OTHER editor (a user subclass of
`AttentionBase` or of the classes above) takes the GENERIC path: a closure with the reference's dataflow
(:10-48) on our kernels materialises `sim` and `attn` ([B*heads, N, L]) and calls the editor's Python, exactly as
`p2p/model/register.py` does for controllers.
"""
import torch

from ... import hip, planes
from ...control import ControlPlan


def _attention_modules(unet):
    out = []
    for name, child in unet.named_children():
        if "down" in name or "mid" in name or "up" in name:
            out += [m for m in child.modules() if m.__class__.__name__ == "Attention"]
    return out


def _controlled_self_layers(unet, layers):
    """(head dim, tokens) of the self-attention of every transformer layer in `layers` (layer = execution index // 2), at
    the UNet's configured sample size"""
    out, res = [], int(unet.cfg.sample_size)

    def visit(block):
        for m in block.modules():
            if m.__class__.__name__ == "Attention" and not m.is_cross and (m._exec_index // 2) in layers:
                out.append((m.dim_head, res * res))

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


def _attention_order(unet):
    """(module, tokens) of every attention module in execution order, at the UNet's configured sample size"""
    out, res = [], int(unet.cfg.sample_size)

    def visit(block):
        out.extend((m, res * res) for m in block.modules() if m.__class__.__name__ == "Attention")

    for blk in unet.down_blocks:
        visit(blk)
        if blk.downsamplers is not None:
            res //= 2
    visit(unet.mid_block)
    for blk in unet.up_blocks:
        visit(blk)
        if blk.upsamplers is not None:
            res *= 2
    return sorted(out, key=lambda e: e[0]._exec_index)


def auto_mask_refusal(editor, precision, x3p, flash_planes, layer_shapes, batch=4):
    """the host part of the decision to lower `MutualSelfAttentionControlMaskAuto`: None, or the reason it takes the generic
    path.  layer_shapes: (head dim, tokens) of the controlled self-attention layers; batch: the UNet batch it will see"""
    if precision != "f16x3" or not x3p or not flash_planes:
        return "the fused rule runs on the planes attention of the f16x3 mode only"
    if editor.mask_save_dir is not None:
        return "mask_save_dir writes every layer's masks to disk, which the fused plan never brings to the host"
    if not (isinstance(editor.thres, (int, float)) and 0 < editor.thres <= 1):
        return f"thres = {editor.thres!r} is outside (0, 1]: a key class could be empty"
    for idx, nm in ((editor.ref_token_idx, "ref_token_idx"), (editor.cur_token_idx, "cur_token_idx")):
        if not isinstance(idx, (list, tuple)) or not idx or not all(isinstance(i, int) and 0 <= i < ControlPlan.CTX_TOKENS for i in idx):
            return f"{nm} = {idx!r} is not a non-empty list of token indices in [0, {ControlPlan.CTX_TOKENS})"
    if batch != 4:
        return f"the rule is stated for the UNet batch [u_src, u_tgt, c_src, c_tgt]; got batch {batch}"
    for d, N in layer_shapes:
        if d not in planes.FLASH_PLANES_DIMS:
            return f"a controlled layer has head dim {d}, outside the planes attention's {planes.FLASH_PLANES_DIMS}"
        if N < ControlPlan.MAP_TOKENS:
            return f"a controlled layer has {N} tokens, fewer than the {ControlPlan.MAP_TOKENS} of the maps the masks come from"
        if N % 32:
            return f"a controlled layer has {N} tokens, no multiple of the 32 a class word covers"
    return None


def _lower_auto_editor(editor, device, unet):
    """the fused plan of `MutualSelfAttentionControlMaskAuto`, or None with one printed line saying why not.  Which modules have
    256 queries, and how many of them precede each controlled layer, is counted at the UNet's configured sample size"""
    layers = set(int(l) for l in editor.layer_idx)
    why = auto_mask_refusal(editor, getattr(unet, "precision", None), getattr(unet, "x3p", False), planes.FLASH_PLANES,
                            _controlled_self_layers(unet, layers) if unet is not None else ())
    if why is not None:
        print(f"auto-mask MasaCtrl takes the generic path: {why}")
        return None
    slots, counts = {}, {}
    for m, N in _attention_order(unet):
        if m.is_cross and N == ControlPlan.MAP_TOKENS:
            slots[m._exec_index] = len(slots)
        elif not m.is_cross and (m._exec_index // 2) in layers:
            counts[m._exec_index] = (len(slots), N)
    return ControlPlan(editor, "masactrl_mask_auto", device, masa_steps=editor.step_idx, masa_layers=layers, auto_slots=slots,
                       auto_layers=counts, auto_thres=editor.thres, auto_ref=editor.ref_token_idx, auto_cur=editor.cur_token_idx)


def _lower_mask_editor(editor, device, unet):
    """the fused plan of `MutualSelfAttentionControlMask`, or None with one printed line saying why not.  The resolutions are
    those of the UNet's configured sample size (the latent size is not known at registration); latents of another size get
    their lists at the first forward, where an empty key class is an error instead of a fall-back"""
    def no(why):
        print(f"mask-guided MasaCtrl takes the generic path: {why}")
        return None

    if unet is None or getattr(unet, "precision", None) != "f16x3" or not getattr(unet, "x3p", False) or not planes.FLASH_PLANES:
        return no("the fused rule runs on the planes attention of the f16x3 mode only")
    ms, mt = editor.mask_s, editor.mask_t
    if ms is None or mt is None:
        return no("it needs both mask_s and mask_t")
    for m, nm in ((ms, "mask_s"), (mt, "mask_t")):
        if not (isinstance(m, torch.Tensor) and m.dim() == 2 and m.shape[0] == m.shape[1]):
            return no(f"{nm} is not a square [h, w] tensor")
        if not bool(((m == 0) | (m == 1)).all()):
            return no(f"{nm} is not binary (values other than 0 and 1)")
    layers = set(int(l) for l in editor.layer_idx)
    shapes = _controlled_self_layers(unet, layers)
    for d, N in shapes:
        if d not in planes.FLASH_PLANES_DIMS:
            return no(f"a controlled layer has head dim {d}, outside the planes attention's {planes.FLASH_PLANES_DIMS}")
    tokens = sorted(set(N for _, N in shapes))
    for N in tokens:
        r = ControlPlan.resized_mask(ms.detach().float().cpu(), N)
        if not bool((r == 1).any()) or not bool((r == 0).any()):
            return no(f"mask_s has an empty key class at {N} tokens")
    return ControlPlan(editor, "masactrl_mask", device, masa_steps=editor.step_idx, masa_layers=layers,
                       mask_s=ms, mask_t=mt, mask_tokens=tokens)


def _lower_union_editor(editor, device, unet):
    """the fused plan of `MutualSelfAttentionControlUnion`, or None with one printed line saying why not.  The head dims of the
    controlled layers are counted at the UNet's configured sample size"""
    def no(why):
        print(f"MasaCtrl Union takes the generic path: {why}")
        return None

    if unet is None or getattr(unet, "precision", None) != "f16x3" or not getattr(unet, "x3p", False) or not planes.FLASH_PLANES:
        return no("the fused rule runs on the planes attention of the f16x3 mode only")
    layers = set(int(l) for l in editor.layer_idx)
    for d, _ in _controlled_self_layers(unet, layers):
        if d not in planes.FLASH_PLANES_DIMS:
            return no(f"a controlled layer has head dim {d}, outside the planes attention's {planes.FLASH_PLANES_DIMS}")
    return ControlPlan(editor, "masactrl_union", device, masa_steps=editor.step_idx, masa_layers=layers)


def lower_editor(editor, device, unet=None):
    name = type(editor).__name__
    if name == "AttentionBase":
        return ControlPlan(editor, "empty", device)
    if name == "MutualSelfAttentionControl":
        return ControlPlan(editor, "masactrl", device, masa_steps=editor.step_idx, masa_layers=editor.layer_idx)
    if name == "MutualSelfAttentionControlMask":
        return _lower_mask_editor(editor, device, unet)
    if name == "MutualSelfAttentionControlMaskAuto":
        return _lower_auto_editor(editor, device, unet)
    if name == "MutualSelfAttentionControlUnion":
        return _lower_union_editor(editor, device, unet)
    return None


def _generic_forward(attn, editor, place_in_unet):
    """`ca_forward` of `/root/reference/masactrl/model/register.py:10-48` on our kernels: q, k, v as [(B*heads), N, d],
    `sim` = scaled scores, `attn` = their row softmax, all materialised; the editor returns [B, N, heads*d]"""
    to_out = attn.to_out[0] if isinstance(attn.to_out, torch.nn.ModuleList) else attn.to_out

    def forward(x, encoder_hidden_states=None, attention_mask=None, context=None, mask=None, **unused):
        if encoder_hidden_states is not None:
            context = encoder_hidden_states
        if attention_mask is not None or mask is not None:
            raise NotImplementedError("attention masks are not on the reference path (always None)")
        is_cross = context is not None
        context = context if is_cross else x
        q, k, v = attn.to_q(x), attn.to_k(context), attn.to_v(context)
        sim, probs = hip.attn_scores(q.contiguous(), k.contiguous(), attn.heads, attn.scale)
        out = editor(attn.head_to_batch_dim(q), attn.head_to_batch_dim(k), attn.head_to_batch_dim(v), sim, probs, is_cross,
                     place_in_unet, attn.heads, scale=attn.scale)
        return to_out(out.to(x.dtype).contiguous())

    return forward


def _places(unet):
    """(place, module) in the reference's registration order (:64-72: "down" / "mid" / "up" by child name)"""
    out = []
    for name, child in unet.named_children():
        for key in ("down", "mid", "up"):
            if key in name:
                out += [(key, m) for m in child.modules() if m.__class__.__name__ == "Attention"]
                break
    return out


def regiter_attention_editor_diffusers(model, editor):
    unet = model.unet
    plan = lower_editor(editor, unet.device, unet)
    mods = _places(unet)
    for place, m in mods:
        m.__dict__.pop("forward", None)
        m._plan = plan
        if plan is None:                       # generic path: the editor's own Python on materialised tensors
            m._original_forward = m.forward
            m.forward = _generic_forward(m, editor, place)
    unet._plan = plan
    editor.num_att_layers = len(mods)
    return editor


def unregister_attention_control(model, editor):
    unet = model.unet
    for m in _attention_modules(unet):
        m.__dict__.pop("forward", None)
        m.__dict__.pop("_original_forward", None)
        m._plan = None
    unet._plan = None
    if editor is not None:
        editor.num_att_layers = 0
