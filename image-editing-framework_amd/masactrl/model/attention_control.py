"""Mutual self-attention control (`/root/reference/masactrl/model/attention_control.py:10-68`).

From `start_step` on, in transformer layers >= `start_layer` (layer = cur_att_layer // 2, counted in execution order:
6 down, 1 mid, 9 up for SD), every SELF-attention of the uncond half uses the K and V of that half's first sample
(the source image), and likewise for the cond half (:59-66).  Only this class is reachable from the reference CLIs
(`masactrl/edit_syn.py:108`, `edit_real.py:136`).

`MutualSelfAttentionControlMask` (:110-189) is the mask-guided variant for the batch [u_src, u_tgt, c_src, c_tgt]: the
source rows attend to themselves; each target row attends to its half's source keys twice -- "fg" with every key outside
`mask_s` pushed to `finfo.min`, "bg" with every key inside it -- and the two outputs are blended per query by `mask_t`.
Here the CLIs reach it through `--mask_s / --mask_t`.  With binary masks in the f16x3 mode `register.py` lowers it to
gathered flash-attention launches; everywhere else the bodies below run on the generic path.

`MutualSelfAttentionControlMaskAuto` (:192-330) needs no masks from the user: per controlled layer it makes them from the
16 x 16 cross-attention maps the step has computed so far (`--mask_auto`).  In the f16x3 mode `register.py` lowers it to one
class-masked flash-attention launch per controlled layer (`control.py`, kind 'masactrl_mask_auto').

`MutualSelfAttentionControlUnion` (:71-107) is the variant with united keys for the same batch: a target row attends with its
own queries over its half's source keys FOLLOWED by its own (one softmax over 2 N keys), the source rows attend to themselves
(`--union`).  In the f16x3 mode `register.py` lowers it to one two-segment flash-attention launch per controlled layer
(`control.py`, kind 'masactrl_union').
"""
import os

import torch
import torch.nn.functional as F

from .attention_base import AttentionBase


class MutualSelfAttentionControl(AttentionBase):
    MODEL_TYPE = {"SD": 16, "SDXL": 70}

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, model_type="SD"):
        super().__init__()
        self.total_steps = total_steps
        self.total_layers = self.MODEL_TYPE.get(model_type, 16)
        self.start_step = start_step
        self.start_layer = start_layer
        self.layer_idx = layer_idx if layer_idx is not None else list(range(start_layer, self.total_layers))
        self.step_idx = step_idx if step_idx is not None else list(range(start_step, total_steps))
        print("MasaCtrl at denoising steps: ", self.step_idx)
        print("MasaCtrl at U-Net layers: ", self.layer_idx)

    def attn_batch(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        """all samples of q attend to the keys of k's samples, concatenated per head in sample order:
        [(b h), n, d] x [(bk h), n, d] -> [b, n, h*d]; bk == 1 (ONE sample's k, v, all the mutual editor passes) leaves k and v
        as they are"""
        bh, n, d = q.shape
        b = bh // num_heads
        qh = q.reshape(b, num_heads, n, d).permute(1, 0, 2, 3).reshape(num_heads, b * n, d)
        bk = k.shape[0] // num_heads
        if bk > 1:
            k = k.reshape(bk, num_heads, -1, d).permute(1, 0, 2, 3).reshape(num_heads, -1, d)
            v = v.reshape(bk, num_heads, -1, d).permute(1, 0, 2, 3).reshape(num_heads, -1, d)
        s = torch.bmm(qh, k.transpose(1, 2)) * kwargs.get("scale")
        out = torch.bmm(s.softmax(-1), v)                           # h (b n) d
        return out.reshape(num_heads, b, n, d).permute(1, 2, 0, 3).reshape(b, n, num_heads * d)

    def forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        if is_cross or self.cur_step not in self.step_idx or self.cur_att_layer // 2 not in self.layer_idx:
            return super().forward(q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs)
        qu, qc = q.chunk(2)
        ku, kc = k.chunk(2)
        vu, vc = v.chunk(2)
        out_u = self.attn_batch(qu, ku[:num_heads], vu[:num_heads], None, None, is_cross, place_in_unet, num_heads, **kwargs)
        out_c = self.attn_batch(qc, kc[:num_heads], vc[:num_heads], None, None, is_cross, place_in_unet, num_heads, **kwargs)
        return torch.cat([out_u, out_c], dim=0)


class MutualSelfAttentionControlUnion(MutualSelfAttentionControl):
    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, model_type="SD"):
        """mutual self-attention with UNITED source and target keys, for the UNet batch [u_src, u_tgt, c_src, c_tgt].  At a
        controlled (step, layer) row u_tgt attends with its own queries over [K_u_src ; K_u_tgt] with values
        [V_u_src ; V_u_tgt] -- one softmax over 2 N keys, source keys first -- and row c_tgt likewise over its half; rows u_src
        and c_src are plain self-attention on their own K, V.

        The source rows are where this class leaves the reference's text: there the source branch calls the parent's
        `forward` on ONE batch row, which at a controlled step halves the HEADS with `q.chunk(2)` and then asks einops for a
        batch of (h / 2) // h = 0, so the reference raises at its first controlled layer and no run of it exists to compare
        with.  Its comment ("source image branch") and the Mask / MaskAuto variants, whose source rows attend to themselves,
        state the intent, and that is what is built here.  Any UNet batch other than 4 raises, where `chunk(4)` would split
        it silently into something else."""
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps, model_type)
        print("Using MutualSelfAttentionControlUnion")

    def forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        if is_cross or self.cur_step not in self.step_idx or self.cur_att_layer // 2 not in self.layer_idx:
            return AttentionBase.forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs)
        h = num_heads
        if q.shape[0] != 4 * h:
            raise RuntimeError(f"Union acts on the UNet batch [u_src, u_tgt, c_src, c_tgt]; got batch {q.shape[0] // h}")
        outs = []
        for half in (0, 2):        # rows (src, tgt) of the uncond, then of the cond half
            src, tgt, both = slice(half * h, (half + 1) * h), slice((half + 1) * h, (half + 2) * h), slice(half * h, (half + 2) * h)
            outs.append(AttentionBase.forward(self, q[src], k[src], v[src], None, attn[src], is_cross, place_in_unet, h, **kwargs))
            outs.append(self.attn_batch(q[tgt], k[both], v[both], None, None, is_cross, place_in_unet, h, **kwargs))
        return torch.cat(outs, dim=0)


def _save_mask_png(mask, path):
    """what `torchvision.utils.save_image(mask[None, None], path)` writes for one [h, w] map: x 255, + 0.5, clamp, 8 bit, RGB"""
    from PIL import Image
    g = mask.detach().float().cpu().mul(255).add(0.5).clamp(0, 255).to(torch.uint8)
    Image.fromarray(g[..., None].expand(-1, -1, 3).contiguous().numpy()).save(path)


class MutualSelfAttentionControlMask(MutualSelfAttentionControl):
    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, mask_s=None, mask_t=None,
                 mask_save_dir=None, model_type="SD"):
        """mask_s / mask_t: source / target masks [h, w] (same shape), resized per layer by `F.interpolate` (nearest)"""
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps, model_type)
        self.mask_s = mask_s
        self.mask_t = mask_t
        print("Using mask-guided MasaCtrl")
        if mask_save_dir is not None:
            os.makedirs(mask_save_dir, exist_ok=True)
            _save_mask_png(self.mask_s, os.path.join(mask_save_dir, "mask_s.png"))
            _save_mask_png(self.mask_t, os.path.join(mask_save_dir, "mask_t.png"))

    def attn_batch(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        """as the parent's; with is_mask_attn and a source mask the scores are taken twice, fg (keys outside the mask at
        finfo.min, the others + 1) and bg (keys inside at finfo.min), and the outputs come back as [fg rows | bg rows]"""
        bh, n, d = q.shape
        b = bh // num_heads
        H = W = int(n ** 0.5)
        # only q is regrouped to h (b n) d: k / v are ONE sample's [h, n, d], which is all `forward` ever passes
        assert k.shape[0] == num_heads and v.shape[0] == num_heads, "attn_batch: k / v must be one sample's [heads, n, d]"
        qh = q.reshape(b, num_heads, n, d).permute(1, 0, 2, 3).reshape(num_heads, b * n, d)
        s = torch.bmm(qh, k.transpose(1, 2)) * kwargs.get("scale")
        if kwargs.get("is_mask_attn") and self.mask_s is not None:
            print("masked attention")
            mask = F.interpolate(self.mask_s[None, None].to(device=s.device, dtype=s.dtype), (H, W)).flatten()
            lowest = torch.finfo(s.dtype).min
            s_bg = s + mask.masked_fill(mask == 1, lowest)
            s_fg = s + mask.masked_fill(mask == 0, lowest)
            s = torch.cat([s_fg, s_bg], dim=0)
        p = s.softmax(-1)
        if len(p) == 2 * len(v):
            v = torch.cat([v] * 2)
        out = torch.bmm(p, v)                                       # (h1 h) (b n) d
        h1 = out.shape[0] // num_heads
        return out.reshape(h1, num_heads, b, n, d).permute(0, 2, 3, 1, 4).reshape(h1 * b, n, num_heads * d)

    def forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        if is_cross or self.cur_step not in self.step_idx or self.cur_att_layer // 2 not in self.layer_idx:
            return AttentionBase.forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs)
        n = q.shape[1]
        H = W = int(n ** 0.5)
        qu, qc = q.chunk(2)
        ku, kc = k.chunk(2)
        vu, vc = v.chunk(2)
        args = (None, None, is_cross, place_in_unet, num_heads)
        out_u_source = self.attn_batch(qu[:num_heads], ku[:num_heads], vu[:num_heads], *args, **kwargs)
        out_c_source = self.attn_batch(qc[:num_heads], kc[:num_heads], vc[:num_heads], *args, **kwargs)
        out_u_target = self.attn_batch(qu[-num_heads:], ku[:num_heads], vu[:num_heads], *args, is_mask_attn=True, **kwargs)
        out_c_target = self.attn_batch(qc[-num_heads:], kc[:num_heads], vc[:num_heads], *args, is_mask_attn=True, **kwargs)
        if self.mask_s is not None and self.mask_t is not None:
            out_u_fg, out_u_bg = out_u_target.chunk(2, 0)
            out_c_fg, out_c_bg = out_c_target.chunk(2, 0)
            mask = F.interpolate(self.mask_t[None, None].to(device=q.device, dtype=out_u_fg.dtype), (H, W)).reshape(-1, 1)
            out_u_target = out_u_fg * mask + out_u_bg * (1 - mask)
            out_c_target = out_c_fg * mask + out_c_bg * (1 - mask)
        return torch.cat([out_u_source, out_u_target, out_c_source, out_c_target], dim=0)


class MutualSelfAttentionControlMaskAuto(MutualSelfAttentionControl):
    MAP_TOKENS = 16 * 16       # the cross-attention level whose maps make the masks

    def __init__(self, start_step=4, start_layer=10, layer_idx=None, step_idx=None, total_steps=50, thres=0.1, ref_token_idx=[1],
                 cur_token_idx=[1], mask_save_dir=None, model_type="SD"):
        """the masks of `MutualSelfAttentionControlMask` made from the prompt instead of two images: the head-mean of every
        16 x 16 cross-attention map of the CURRENT step so far, summed over the prompt tokens `ref_token_idx` (source, keys) /
        `cur_token_idx` (target, queries; a token listed twice counts twice), normalised to [0, 1] per batch row and
        thresholded at `thres`.  A map that is constant over the image (max == min) gives NaN and with it an all-background
        mask here; the fused plan (`control.py`, kind 'masactrl_mask_auto') makes every token background in that case, which
        is plain mutual attention"""
        super().__init__(start_step, start_layer, layer_idx, step_idx, total_steps, model_type)
        print("Using MutualSelfAttentionControlMaskAuto")
        self.thres = thres
        self.ref_token_idx = ref_token_idx
        self.cur_token_idx = cur_token_idx
        self.cross_attns = []          # head-mean maps [B, 256, L] of this step, in execution order
        self.mask_s = None             # binary masks [res, res] of the last controlled call that had maps (None before)
        self.mask_t = None
        self.mask_save_dir = mask_save_dir
        if mask_save_dir is not None:
            os.makedirs(mask_save_dir, exist_ok=True)

    def after_step(self):
        self.cross_attns = []

    def token_image(self, idx):
        """[B, 16, 16]: mean of the collected maps, summed over the tokens `idx`, each batch row scaled to min 0 / max 1"""
        a = torch.stack(self.cross_attns).mean(0)
        res = int(a.shape[1] ** 0.5)
        img = a.reshape(a.shape[0], res, res, a.shape[-1])[..., list(idx) if isinstance(idx, (list, tuple)) else [idx]].sum(-1)
        lo, hi = img.amin(dim=(1, 2), keepdim=True), img.amax(dim=(1, 2), keepdim=True)
        return (img - lo) / (hi - lo)

    def _layer_mask(self, img, res, name):
        soft = F.interpolate(img[None, None], (res, res))[0, 0]
        if self.mask_save_dir is not None:
            _save_mask_png(soft, os.path.join(self.mask_save_dir, f"{name}_{self.cur_step}_{self.cur_att_layer}.png"))
        return (soft >= self.thres).to(img.dtype)

    def masked_target(self, q, k, v, key_mask, query_mask, num_heads, scale):
        """one target row over its half's source keys: q, k, v [h, n, d]; queries inside `query_mask` take the softmax over
        the keys inside `key_mask`, the others over the keys outside it -> [1, n, h*d]"""
        s = torch.bmm(q, k.transpose(1, 2)) * scale
        lowest = torch.finfo(s.dtype).min
        km = key_mask.flatten()
        fg = torch.bmm((s + km.masked_fill(km == 0, lowest)).softmax(-1), v)
        bg = torch.bmm((s + km.masked_fill(km == 1, lowest)).softmax(-1), v)
        qm = query_mask.reshape(-1, 1)
        out = fg * qm + bg * (1 - qm)
        return out.permute(1, 0, 2).reshape(1, q.shape[1], -1)

    def forward(self, q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs):
        if is_cross and attn.shape[1] == self.MAP_TOKENS:
            self.cross_attns.append(attn.reshape(-1, num_heads, *attn.shape[-2:]).mean(1))
        if is_cross or self.cur_step not in self.step_idx or self.cur_att_layer // 2 not in self.layer_idx or not self.cross_attns:
            return super().forward(q, k, v, sim, attn, is_cross, place_in_unet, num_heads, **kwargs)
        h, n = num_heads, q.shape[1]
        if q.shape[0] != 4 * h:
            raise RuntimeError(f"MaskAuto acts on the UNet batch [u_src, u_tgt, c_src, c_tgt]; got batch {q.shape[0] // h}")
        res = int(n ** 0.5)
        self.mask_s = self._layer_mask(self.token_image(self.ref_token_idx)[-2].to(q.dtype), res, "mask_s")
        self.mask_t = self._layer_mask(self.token_image(self.cur_token_idx)[-1].to(q.dtype), res, "mask_t")
        outs = []
        for half in (0, 2):        # rows (src, tgt) of the uncond, then of the cond half
            src, tgt = slice(half * h, (half + 1) * h), slice((half + 1) * h, (half + 2) * h)
            outs.append(MutualSelfAttentionControl.attn_batch(self, q[src], k[src], v[src], None, None, is_cross, place_in_unet, h,
                                                              **kwargs))
            outs.append(self.masked_target(q[tgt], k[src], v[src], self.mask_s, self.mask_t, h, kwargs.get("scale")))
        return torch.cat(outs, dim=0)


def load_mask_png(path, device="cpu"):
    """a mask image -> fp32 [h, w] in {0, 1}: grey levels / 255 thresholded at 0.5 (the CLIs' --mask_s / --mask_t)"""
    import numpy as np
    from PIL import Image
    g = torch.from_numpy(np.asarray(Image.open(path).convert("L"), dtype=np.float32) / 255.0)
    return (g > 0.5).float().to(device)
