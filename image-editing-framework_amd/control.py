"""Device-side control plan: a known controller lowered to data the fused attention kernels read.

The reference hands every materialised attention map to Python
(`/root/reference/p2p/model/register.py:47-48`).  For the controller classes whose arithmetic is
known (`EmptyControl`, `AttentionReplace / Refine / Reweight`; MasaCtrl's mutual self-attention)
the same effect is expressed as small device tables, so no map is ever written to HBM:

  cross-attention edit (attention_base.py:118-121, attention_control.py:15-46)
      P' = c1[step][w] * (P_src @ M)[w] + c2[step][w] * P_tgt[w]
      M^T fp16 [slots,96,96], coef table fp32 [steps+1, slots, 2, 96]
  self-attention replace (attention_base.py:123,132-136), only for maps with N <= 16*16 and
      num_self_replace[0] <= step < num_self_replace[1]:
      target rows take the source row's Q and K (=> identical map), keep their own V
      source-row table int32 [steps+1, 2B]  (identity rows outside the window)
  LocalBlend of an edit controller (p2p/model/ptp_utils.py, LocalBlend.__call__; the 'p2p' plan with a blend part): the masks
      come from the EDITED maps of the five 16 x 16 cross-attention modules, summed over the blend words, over heads, modules
      and all steps so far.  The edit is linear in the two softmax rows it mixes, so that sum is  P_src . u_i + P_i . v_i  with
      per-step vectors fp32 [steps+1, Bp, 2, 96] the lowering folds from the tables above and the blend words; each of the five
      modules adds it into one accumulator fp32 [Bp, 256] (`ief_cross_blend_mass_f32`), and after the step's latent update one
      launch makes the masks and blends the latents in place (`ief_local_blend_f32`)
  MasaCtrl mutual self-attention (/root/reference/masactrl/model/attention_control.py:37-68):
      K,V source rows per (step, layer)
  MasaCtrl mask-guided mutual self-attention (/root/reference/masactrl/model/attention_control.py:134-189), binary masks,
      batch [u_src, u_tgt, c_src, c_tgt]: a target query inside mask_t attends to the source keys inside mask_s, one
      outside to the keys outside (the fg / bg blend picks one of two softmaxes per query, and the +1 the fg branch adds
      to its surviving keys is softmax-invariant): the mutual launch as above, then two launches over gathered row lists
      that overwrite the target rows -- int32 lists fg_keys / bg_keys / fg_queries / bg_queries per token count and a
      per-step gate table (1 in the controlled steps) that switches those launches inside a captured graph
  MasaCtrl with masks from cross-attention (/root/reference/masactrl/model/attention_control.py:192-330), same batch: the masks
      of a controlled layer are the mean of the head-mean 16 x 16 cross-attention maps the step has computed SO FAR, summed over
      prompt tokens, normalised per row, resized and thresholded -- data made on the device per step and layer, so no list
      length can be a launch argument.  Every 256-token cross-attention module writes its two token-mass rows into its slot
      of a [K, 2, 256] buffer (`ief_cross_token_mass_f32`: rows c_src / c_tgt, token multiplicity vectors), a controlled layer
      with c >= 1 earlier slots turns the first c slots into packed class bits (`ief_masa_auto_classes`) and ONE class-masked
      launch over all source keys overwrites the two target rows; the per-step gate switches both off in uncontrolled steps.
      c is a property of the layer's place in the execution order (static); thres, the multiplicities and the gate are data
  MasaCtrl with united source and target keys (/root/reference/masactrl/model/attention_control.py:71-107), same batch: a
      target row attends with its own queries over [K_src ; K_tgt] of its half, ONE softmax over 2 N keys, source keys first;
      the source rows are plain self-attention (what the reference intends; its own call for them raises, see the class).  The
      planes attention walks two key / value segments from two batch rows (`k2_src / v2_src`): the mutual table
      [0, 0, 2, 2] as the first segment's rows and a second table [-1, 1, -1, 3] -- ONE launch per controlled layer for all
      four rows, identity / -1 rows in the uncontrolled steps, so a captured graph needs no gate
  Plug-and-Play injection (/root/reference/pnp/model/register.py:27-90,100-182), batch = 4 blocks of s rows
      [uncond_src, uncond_tgt, cond_src, cond_tgt]: during the first qk_steps timesteps the self-attention of the chosen
      decoder layers computes rows of blocks 1 and 3 with the Q and K of block 2 (:45-52), and during the first
      conv_steps timesteps `up_blocks[1].resnets[1]` replaces their conv2 output by block 2's (:161-166):
      a Q/K source-row table and a feature source-row table, int32 [steps+1, B]

The step index lives in device memory (`step`), the per-step rows are copied into fixed
"current" buffers by `ief_select_step` at the start of every UNet forward, and the counter is
bumped by `ief_advance_step` at its end — all stream-ordered kernels, so ONE captured hipGraph
replays correctly for all 50 steps.  The Python controller's own counters (`cur_step`,
`cur_att_layer`, `between_steps()`) are advanced exactly as `AttentionControl.__call__` does
(attention_base.py:23-27) so user code observing them sees reference behaviour.
"""
from typing import Optional

import torch

from . import hip

XL = 96  # padded key count of the cross-attention kernel


def _step_hook(c):
    # P2P controllers call it between_steps (p2p/model/attention_base.py:27), MasaCtrl editors after_step
    # (masactrl/model/attention_base.py:21)
    fn = getattr(c, "between_steps", None) or getattr(c, "after_step", None)
    if fn is not None:
        fn()


def advance_controller(c):
    """`attention_base.py:23-27` for any object following the controller protocol."""
    c.cur_att_layer += 1
    uncond = c.num_att_layers if getattr(c, "LOW_RESOURCE", False) else 0
    if c.cur_att_layer == c.num_att_layers + uncond:
        c.cur_att_layer = 0
        c.cur_step += 1
        _step_hook(c)


class StepCounter:
    """the counters of `AttentionControl` (attention_base.py:10-27) for plans that have no controller object (PnP)"""

    def __init__(self, num_att_layers: int = 0):
        self.cur_step, self.cur_att_layer, self.num_att_layers = 0, 0, num_att_layers

    def between_steps(self):
        pass

    def reset(self):
        self.cur_step, self.cur_att_layer = 0, 0


# ------------------------------------------------------------------------------------------ LEDITS++: host tables
LEDITS_MAX_CONCEPTS = 8


def ledits_rank(q: float, n: int):
    """(lo, frac) of torch.quantile's linear rule over n values with the arithmetic pinned: q (n - 1) in double, its floor, and
    the remainder rounded to fp32 -- t = v_(lo) + frac (v_(lo + 1) - v_(lo)).  frac lies in [0, 1): a remainder that rounds to 1.0f
    moves to the next rank."""
    import numpy as np
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"LEDITS++: a threshold is a quantile in [0, 1], got {q!r}")
    if n < 1:
        raise ValueError("ledits_rank: n must be >= 1")
    pos = q * (n - 1)
    lo = int(pos // 1)
    frac = float(np.float32(pos - lo))
    if frac >= 1.0:
        lo, frac = lo + 1, 0.0
    if lo >= n - 1:
        lo, frac = n - 1, 0.0
    return lo, frac


def ledits_rank_table(qs, n: int):
    """fp32 [E, 2] = [lo, frac] per concept (`ief_ledits_attn_mask_f32` / `ief_ledits_guidance_mask_f32`); lo < 2^24 is exact"""
    return torch.tensor([list(ledits_rank(q, n)) for q in qs], dtype=torch.float32).reshape(-1, 2)


def ledits_taps(sigma: float = 0.5):
    """the nine fp32 taps of the 3 x 3 smoothing, row-major: the normalised 2-D Gaussian, formed in double"""
    g = torch.exp(-(torch.arange(3, dtype=torch.float64) - 1.0) ** 2 / (2.0 * float(sigma) ** 2))
    k = torch.outer(g, g)
    return (k / k.sum()).to(torch.float32).flatten()


def ledits_token_weights(token_counts):
    """fp32 [E, 2, XL] = (u_e, v_e) for `ief_cross_blend_mass_f32`: u_e = 0 (no source row), v_e = 1 on tokens 1 .. n_e of concept
    e's tokenisation (between BOS and EOS), 0 elsewhere"""
    w = torch.zeros(len(token_counts), 2, XL)
    for e, n in enumerate(token_counts):
        n = int(n)
        if not 1 <= n <= ControlPlan.CTX_TOKENS - 2:
            raise ValueError(f"LEDITS++: concept {e} has {n} tokens between BOS and EOS (1 .. {ControlPlan.CTX_TOKENS - 2})")
        w[e, 1, 1:1 + n] = 1.0
    return w


def _per_concept(value, E, name, kind=float, none_ok=False):
    vals = list(value) if isinstance(value, (list, tuple)) else [value]
    if len(vals) == 1:
        vals = vals * E
    if len(vals) != E:
        raise ValueError(f"LEDITS++: {len(vals)} values of {name} for {E} concepts (one value, or one per concept)")
    return [None if (v is None and none_ok) else kind(v) for v in vals]


def ledits_scale_table(num_steps: int, scales, reverse=(), warmup=0, cooldown=None):
    """fp32 [num_steps + 1, E]: the guidance scale of concept e in edit step i (counted from 0 at the first step the edit runs),
    sign and gate folded in: -scale for a concept in `reverse` (its direction is removed), 0 while i < warmup_e and from
    i >= cooldown_e on (None: no cool-down), 0 in the row past the schedule.  A zero switches the concept off in that step."""
    scales = list(scales) if isinstance(scales, (list, tuple)) else [scales]
    E = len(scales)
    warm = _per_concept(warmup, E, "warm-up steps", int)
    cool = _per_concept(cooldown, E, "cool-down steps", int, none_ok=True)
    rev = set(int(r) for r in reverse)
    if any(not 0 <= r < E for r in rev):
        raise ValueError(f"LEDITS++: a reversed concept index outside [0, {E})")
    if any(w < 0 for w in warm) or any(c is not None and c < 0 for c in cool):
        raise ValueError("LEDITS++: warm-up and cool-down steps are >= 0")
    tab = torch.zeros(num_steps + 1, E, dtype=torch.float32)
    for e in range(E):
        s = -float(scales[e]) if e in rev else float(scales[e])
        for i in range(num_steps):
            if i >= warm[e] and (cool[e] is None or i < cool[e]):
                tab[i, e] = s
    return tab


def check_ledits(E, thresholds=(), *, sdxl=False, cfg_split=False, uncond_list=None, source_trajectory=None, edit_mask=None,
                 controller=False):
    """what a LEDITS++ edit refuses (host-side facts only; raises ValueError)"""
    if sdxl:
        raise ValueError("LEDITS++: built for the SD1.x / SD2.x pipelines, not for an SDXL UNet")
    if cfg_split:
        raise ValueError("LEDITS++: the batch is [uncond | concepts], not two halves: not built for the two-GPU CFG split")
    if uncond_list is not None:
        raise ValueError("LEDITS++ together with uncond_list: the edit has no null-text embeddings")
    if source_trajectory is not None:
        raise ValueError("LEDITS++ together with source_trajectory: the edit has no source branch to rectify")
    if edit_mask is not None:
        raise ValueError("LEDITS++ together with edit_mask: the method makes its own masks")
    if controller:
        raise ValueError("LEDITS++: an attention controller, hook or control plan is installed; the masks on top of the "
                         "controllers are out of scope")
    if not isinstance(E, int) or not 1 <= E <= LEDITS_MAX_CONCEPTS:
        raise ValueError(f"LEDITS++: 1 .. {LEDITS_MAX_CONCEPTS} edit concepts, got {E!r}")
    for q in thresholds:
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError(f"LEDITS++: a threshold is a quantile in [0, 1], got {q!r}")


def ledits_cross_mask_refusal(precision, x3p, modules, latent_hw):
    """None, or why the cross-attention mask cannot be served: it stands where LocalBlend's fused form stands.
    modules: (heads, head dim, queries) of the five modules `p2p.model.register.blend_modules` names"""
    if precision != "f16x3" or not x3p:
        return "the cross-attention mask runs on the operand-planes path of the f16x3 mode only (pass cross_attn_mask=False)"
    if len(modules) != 5 or any(N != ControlPlan.MAP_TOKENS for _, _, N in modules):
        return (f"the 16 x 16 cross-attention modules have {[N for _, _, N in modules]} queries at the UNet's configured sample "
                f"size, not five times {ControlPlan.MAP_TOKENS}")
    for heads, d, _ in modules:
        if heads > 64 or d % 8:
            return f"a 16 x 16 cross-attention module has {heads} heads of dim {d} (at most 64 heads, head dim a multiple of 8)"
    if latent_hw[0] % 16 or latent_hw[1] % 16:
        return f"latents of {latent_hw[0]} x {latent_hw[1]} are no multiple of the 16 x 16 map"
    return None


class ControlPlan:
    """kind: 'empty' | 'p2p' | 'masactrl' | 'masactrl_mask' | 'masactrl_mask_auto' | 'masactrl_union' | 'pnp' | 'ledits'"""
    MASA_KINDS = ("masactrl", "masactrl_mask", "masactrl_mask_auto", "masactrl_union")
    GATED_KINDS = ("masactrl_mask", "masactrl_mask_auto")
    MAP_TOKENS, CTX_TOKENS = 256, 77

    def __init__(self, controller, kind: str, device, num_prompts: int = 1, num_steps: int = 0,
                 mt: Optional[torch.Tensor] = None, coef_table: Optional[torch.Tensor] = None,
                 self_window=(0, 0), self_max_tokens: int = 256, masa_steps=(), masa_layers=(),
                 pnp_layers=(), pnp_qk_steps: int = 0, pnp_conv_steps: int = 0, cond_only: bool = False,
                 mask_s: Optional[torch.Tensor] = None, mask_t: Optional[torch.Tensor] = None, mask_tokens=(),
                 auto_slots=None, auto_layers=None, auto_thres: float = 0.1, auto_ref=(), auto_cur=(), blend=None, ledits=None):
        """cond_only: the UNet batch holds ONLY the conditional rows [cond_src, cond_tgt...] — the half a controller acts
        on (`attention_base.py:20-22`) — as on the conditional rank of a 2-GPU CFG split (`denoise.CfgSplitDenoiser`) and
        in the reference's LOW_RESOURCE protocol (:18-19)
        blend ('p2p' only): None, or (execution indices of the five modules LocalBlend reads, per-step weights fp32
        [steps+1, Bp, 2, XL] = (u_i, v_i), threshold)
        ledits ('ledits' only): dict(scale fp32 [steps+1, E], thresholds [E], token_counts [E], cross_mask, intersect_mask, modules
        (execution indices of the five 16 x 16 cross-attention modules; used with cross_mask), latent_hw, channels)"""
        self.controller = controller
        self.kind = kind
        self.device = torch.device(device)
        self.num_prompts = num_prompts
        self.cond_only = bool(cond_only)
        self.batch = num_prompts if cond_only else 2 * num_prompts
        self.num_steps = num_steps
        self.self_window = self_window
        self.self_max_tokens = self_max_tokens
        self.captured = False   # True while a hipGraph replays the forward (Python bookkeeping moves to the replay wrapper)
        self.muted = False      # True during a warm-up forward that must not move any counter
        dev = self.device
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        B, Bp = self.batch, num_prompts
        self.blend_modules = ()
        self.blend_w = self.blend_w_cur = self.blend_acc = self.blend_thres = None
        if blend is not None:
            mods, bw, thres = blend
            assert kind == "p2p" and not cond_only and tuple(bw.shape) == (num_steps + 1, Bp, 2, XL)
            self.blend_modules = tuple(int(i) for i in mods)
            self.blend_w = bw.to(device=dev, dtype=torch.float32).contiguous()
            self.blend_w_cur = torch.zeros(Bp, 2, XL, dtype=torch.float32, device=dev)
            self.blend_acc = torch.zeros(Bp, self.MAP_TOKENS, dtype=torch.float32, device=dev)
            self.blend_thres = torch.tensor([float(thres)], dtype=torch.float32, device=dev)
        if kind == "p2p":
            slots = Bp - 1
            assert mt.shape == (slots, XL, XL) and coef_table.shape == (num_steps + 1, slots, 2, XL)
            self.mt = mt.to(device=dev, dtype=torch.float16).contiguous()
            self.mt32 = mt.to(device=dev, dtype=torch.float32).contiguous()      # the reference-precision kernels' copy
            self.coef_table = coef_table.to(device=dev, dtype=torch.float32).contiguous()
            self.coef_cur = torch.zeros(slots, 2, XL, dtype=torch.float32, device=dev)
            # the edited maps P' = c1 T + c2 P reach max (|c1| + |c2|) (AttentionReweight: c1 = alpha * equalizer): the
            # split-operand kernels size the hi / lo split of P' from it (hip.map_split_scale); the scale is a launch
            # argument, hence part of the signature a pooled step graph is matched on
            ct = coef_table.detach().float()
            self.coef_bound = float((ct[:, :, 0].abs() + ct[:, :, 1].abs()).max()) if ct.numel() else 1.0
            off = 0 if cond_only else Bp          # first conditional row (= the source prompt's) of this UNet batch
            es = torch.full((B,), -1, dtype=torch.int32)
            sl = torch.zeros(B, dtype=torch.int32)
            for k in range(slots):
                es[off + 1 + k] = off
                sl[off + 1 + k] = k
            self.edit_src, self.edit_slot = es.to(dev), sl.to(dev)
            ident = torch.arange(B, dtype=torch.int32)
            repl = ident.clone()
            repl[off + 1:] = off
            tab = ident.repeat(num_steps + 1, 1)
            lo, hi = self_window
            tab[lo:hi] = repl
            self.self_table = tab.contiguous().to(dev)
            self.self_cur = ident.clone().to(dev)
        # MasaCtrl mutual self-attention (/root/reference/masactrl/model/attention_control.py:52-66): in the chosen
        # transformer layers and steps every row of the uncond half attends to K,V of that half's FIRST row (the
        # source image), likewise for the cond half.  The batch size is not known at registration: tables per B.
        self.masa_steps = set(int(s) for s in masa_steps)
        self.masa_layers = set(int(l) for l in masa_layers)
        self._masa = {}
        self._union = {}                           # masactrl_union: B -> (second-segment table int32 [steps, B], its current row)
        self._step_synced = -1
        # masactrl_mask: the two binary masks (host fp32 [h, w]), the token counts of the controlled layers (their lists are
        # built by prepare), per N the four device lists, and the per-step gate of the gathered launches
        self.mask_s = None if mask_s is None else mask_s.detach().float().cpu()
        self.mask_t = None if mask_t is None else mask_t.detach().float().cpu()
        self.mask_tokens = tuple(sorted(set(int(n) for n in mask_tokens)))
        self._mask_lists = {}                      # N -> (fg_keys, bg_keys, fg_queries, bg_queries)
        self._gate = None                          # (table int32 [steps, 1], cur int32 [1])
        self._mask_rows = {}                       # B -> (target rows, their halves' source rows)
        # masactrl_mask_auto: {exec index of a 256-token cross-attention module: its slot}, {exec index of a controlled
        # self-attention module: (c = slots written before it in a forward, its token count at the configured sample size)}
        self.auto_slots = dict(auto_slots or {})
        self.auto_layers = dict(auto_layers or {})
        self.auto_thres = float(auto_thres)
        self.auto_ref, self.auto_cur = [int(i) for i in auto_ref], [int(i) for i in auto_cur]
        self._auto = None                          # (slots fp32 [K, 2, 256], weights fp32 [2, 77], thres fp32 [1])
        self._auto_cls = {}                        # (exec index, N) -> (k_cls, q_cls) int32 [N / 32]
        self.led = None
        if kind == "ledits":
            self._init_ledits(**ledits)
        self.pnp_layers = set(pnp_layers)          # id() of the Attention modules whose Q/K are injected
        self.pnp_qk_steps, self.pnp_conv_steps = int(pnp_qk_steps), int(pnp_conv_steps)
        self._pnp = {}                             # B -> (qk_table, qk_cur, conv_table, conv_cur)

    @staticmethod
    def masa_table(masa_steps, B: int):
        """host int32 [steps, B]: the K / V source rows of mutual self-attention per step -- every row of a half reads that half's
        first row in the controlled steps, itself otherwise; one identity row past the last controlled step"""
        n = (max(masa_steps) + 2) if masa_steps else 1
        ident = torch.arange(B, dtype=torch.int32)
        src = ident.clone()
        half = B // 2
        if half > 0:
            src[:half] = 0
            src[half:] = half
        tab = ident.repeat(n, 1)
        for st in masa_steps:
            tab[int(st)] = src
        return tab.contiguous()

    @classmethod
    def union_tables(cls, masa_steps):
        """host int32 tables of 'masactrl_union' for the batch [u_src, u_tgt, c_src, c_tgt], both [steps, 4] with one
        uncontrolled row past the last controlled step: (first-segment rows = `masa_table`: [0, 0, 2, 2] in the controlled
        steps, identity otherwise; second-segment rows: [-1, 1, -1, 3] in the controlled steps -- a target row appends its
        own keys behind its half's source keys -- and -1 everywhere otherwise: no second segment)"""
        tab = cls.masa_table(masa_steps, 4)
        k2 = torch.full_like(tab, -1)
        for st in masa_steps:
            k2[int(st)] = torch.tensor([-1, 1, -1, 3], dtype=torch.int32)
        return tab, k2.contiguous()

    def prepare(self, B: int):
        """allocate per-batch device tables OUTSIDE any graph capture"""
        if self.kind == "masactrl_union":
            if B != 4:
                raise RuntimeError(f"MasaCtrl Union acts on the UNet batch [u_src, u_tgt, c_src, c_tgt]; got batch {B}")
            if B not in self._union:
                k2 = self.union_tables(self.masa_steps)[1]
                self._union[B] = (k2.to(self.device), torch.full((B,), -1, dtype=torch.int32, device=self.device))
        if self.kind in self.GATED_KINDS:
            if B != 4:
                raise RuntimeError(f"mask-guided MasaCtrl acts on the UNet batch [u_src, u_tgt, c_src, c_tgt]; got batch {B}")
            n = (max(self.masa_steps) + 2) if self.masa_steps else 1
            if self._gate is None:
                g = torch.zeros(n, 1, dtype=torch.int32)
                for st in self.masa_steps:
                    g[st] = 1
                self._gate = (g.to(self.device), torch.zeros(1, dtype=torch.int32, device=self.device))
            if B not in self._mask_rows:
                half = B // 2
                self._mask_rows[B] = (torch.tensor([half - 1, B - 1], dtype=torch.int32, device=self.device),
                                      torch.tensor([0, half], dtype=torch.int32, device=self.device))
            for N in self.mask_tokens:
                self.mask_lists(N)
            if self.kind == "masactrl_mask_auto":
                if self._auto is None:
                    K = max(len(self.auto_slots), 1)
                    self._auto = (torch.zeros(K, 2, self.MAP_TOKENS, dtype=torch.float32, device=self.device),
                                  self.auto_weights().to(self.device),
                                  torch.tensor([self.auto_thres], dtype=torch.float32, device=self.device))
                for ei, (c, N) in self.auto_layers.items():
                    if c >= 1:
                        self._class_words(ei, N)
        if self.kind in self.MASA_KINDS and B not in self._masa:
            tab = self.masa_table(self.masa_steps, B)
            self.num_steps = max(self.num_steps, tab.shape[0] - 1)
            self._masa[B] = (tab.to(self.device), torch.arange(B, dtype=torch.int32, device=self.device))
        if self.kind == "pnp" and B not in self._pnp:
            ident = torch.arange(B, dtype=torch.int32)
            inj = ident.clone()
            s = B // 4
            if s > 0 and B == 4 * s:
                inj[s:2 * s] = ident[2 * s:3 * s]
                inj[3 * s:4 * s] = ident[2 * s:3 * s]
            n = self.num_steps + 1
            qk, cv = ident.repeat(n, 1), ident.repeat(n, 1)
            qk[: self.pnp_qk_steps] = inj
            cv[: self.pnp_conv_steps] = inj
            dev = self.device
            self._pnp[B] = (qk.contiguous().to(dev), ident.clone().to(dev), cv.contiguous().to(dev), ident.clone().to(dev))

    @staticmethod
    def resized_mask(mask, N: int):
        """the mask at a layer of N = H x W tokens, flattened: torch's own nearest resize, as the reference's attn_batch runs it"""
        H = W = int(N ** 0.5)
        if H * W != N:
            raise ValueError(f"mask-guided MasaCtrl needs square token grids, got {N} tokens")
        return torch.nn.functional.interpolate(mask[None, None], (H, W)).flatten()

    def mask_lengths(self, N: int):
        """the lengths of mask_lists(N), from the masks alone (host; builds nothing)"""
        ms, mt = self.resized_mask(self.mask_s, N), self.resized_mask(self.mask_t, N)
        return tuple(int((m == v).sum()) for m, v in ((ms, 1), (ms, 0), (mt, 1), (mt, 0)))

    def mask_lists(self, N: int):
        """(fg_keys, bg_keys, fg_queries, bg_queries) int32 device lists for layers of N tokens; built on first use, which must
        lie outside any graph capture (prepare builds those of `mask_tokens`: the lowering passes the token counts of the
        UNet's CONFIGURED sample size and has checked both key classes there; another latent size adds its counts at the
        first eager or warm-up forward, and raises if a key class is empty at one of them)"""
        if N not in self._mask_lists:
            if self.captured:
                raise RuntimeError(f"ControlPlan.prepare(B) must build the mask lists of {N} tokens before graph capture")
            ms, mt = self.resized_mask(self.mask_s, N), self.resized_mask(self.mask_t, N)
            ls = [torch.nonzero(m == v).flatten().to(torch.int32) for m, v in ((ms, 1), (ms, 0), (mt, 1), (mt, 0))]
            if ls[0].numel() == 0 or ls[1].numel() == 0:
                raise RuntimeError(f"mask_s has an empty key class at {N} tokens: no fused rule there.  The lowering checked the "
                                   f"token counts of the UNet's configured sample size {self.mask_tokens}; run at that size, "
                                   "or register a subclass of the editor to take the generic path")
            self._mask_lists[N] = tuple(t.to(self.device) for t in ls)
            # a token count first met at run time (latents of another size than the configured one): from here on part of
            # what prepare builds, signature() states and load_from() copies
            self.mask_tokens = tuple(sorted(set(self.mask_tokens) | {N}))
        return self._mask_lists[N]

    def mask_launches(self, B: int, N: int, attn):
        """the gathered launches of a controlled self-attention layer under 'masactrl_mask', after the mutual launch:
        None, or (q_src, kv_src, gate, [(q_idx, k_idx), ...]) -- a class without target queries launches nothing"""
        if self.kind != "masactrl_mask" or (attn._exec_index // 2) not in self.masa_layers:
            return None
        fk, bk, fq, bq = self.mask_lists(N)        # also in a muted warm-up forward: the lists exist before capture
        if self.muted:
            return None
        tgt, src = self._mask_rows[B]
        return tgt, src, self._gate[1], [(q, k) for q, k in ((fq, fk), (bq, bk)) if q.numel() > 0]

    # ------------------------------------------------------------------ masks from cross-attention ('masactrl_mask_auto')
    def auto_weights(self):
        """fp32 [2, 77]: how often each prompt token is listed in ref_token_idx (row 0) / cur_token_idx (row 1)"""
        w = torch.zeros(2, self.CTX_TOKENS, dtype=torch.float32)
        for r, idx in enumerate((self.auto_ref, self.auto_cur)):
            for i in idx:
                w[r, i] += 1
        return w

    def _class_words(self, ei: int, N: int):
        """(k_cls, q_cls) of the controlled layer with execution index ei at N tokens; allocated on first use, which must lie
        outside any graph capture (prepare allocates those of the configured sample size, a muted warm-up forward the rest)"""
        key = (ei, N)
        if key not in self._auto_cls:
            if self.captured:
                raise RuntimeError(f"ControlPlan.prepare(B) must allocate the class words of layer {ei // 2} before graph capture")
            if N % 32 or int(N ** 0.5) ** 2 != N:
                raise RuntimeError(f"masactrl_mask_auto: a controlled layer of {N} tokens (square grids of a multiple of 32 only)")
            self._auto_cls[key] = (torch.zeros(N // 32, dtype=torch.int32, device=self.device),
                                   torch.zeros(N // 32, dtype=torch.int32, device=self.device))
        return self._auto_cls[key]

    def cross_mass(self, B: int, N: int, attn, q, k):
        """under 'masactrl_mask_auto' a cross-attention module with 256 queries writes its slot: the head-mean map of row c_src
        summed over the reference tokens, that of row c_tgt over the current tokens (q fp32 [B, N, C], k fp32 [B, 77, C])"""
        if self.blend_w is not None:
            return self._blend_mass(B, N, attn, q, k)
        if self.kind == "ledits":
            return self._ledits_mass(B, N, attn, q, k)
        if self.kind != "masactrl_mask_auto":
            return
        slot = self.auto_slots.get(attn._exec_index)
        if (slot is not None) != (N == self.MAP_TOKENS):
            raise RuntimeError(f"{attn.layer_name}: the auto-mask plan was lowered for the UNet's configured sample size, where "
                               f"this module has {'256' if slot is not None else 'not 256'} queries; it runs at {N}.  Run at "
                               "that size, or register a subclass of the editor to take the generic path")
        if slot is None or self.muted:
            return
        if B != 4 or q.shape[0] != B or k.shape[0] != B or k.shape[1] != self.CTX_TOKENS:
            raise RuntimeError(f"masactrl_mask_auto: cross-attention of batch {tuple(q.shape)} x {tuple(k.shape)}; the rule is "
                               f"stated for the batch [u_src, u_tgt, c_src, c_tgt] and {self.CTX_TOKENS} prompt tokens")
        slots, w, _ = self._auto
        hip.cross_token_mass(q, k, attn.heads, attn.scale, (B // 2, B - 1), w, slots[slot])

    # ------------------------------------------------------------------ LocalBlend ('p2p' with a blend part)
    def _blend_mass(self, B: int, N: int, attn, q, k):
        """one of the five modules LocalBlend reads adds the word-masked, head-mean sum of its edited maps into the accumulator"""
        if attn._exec_index not in self.blend_modules:
            return
        if N != self.MAP_TOKENS:
            raise RuntimeError(f"{attn.layer_name}: the blend was lowered for the UNet's configured sample size, where this module has "
                               f"{self.MAP_TOKENS} queries; it runs at {N}, where LocalBlend's 16 x 16 reshape does not hold")
        if self.muted or not self.applies(B):
            return
        if q.shape[0] != B or k.shape[0] != B or k.shape[1] != self.CTX_TOKENS:
            raise RuntimeError(f"LocalBlend: cross-attention of batch {tuple(q.shape)} x {tuple(k.shape)}; the rule is stated for the "
                               f"full CFG batch of {B} rows and {self.CTX_TOKENS} prompt tokens")
        hip.cross_blend_mass(q, k, attn.heads, attn.scale, self.num_prompts, self.blend_w_cur, self.blend_acc)

    def blend_latents(self, x):
        """LocalBlend on the latents x fp32 [Bp, C, H, W], in place, from what the steps so far accumulated; nothing without a
        blend part or in a muted warm-up step"""
        if self.blend_w is not None and not self.muted:
            hip.local_blend(self.blend_acc, self.blend_thres, x)
        return x

    # ------------------------------------------------------------------ LEDITS++ ('ledits')
    def _init_ledits(self, scale, thresholds, token_counts, cross_mask, intersect_mask, modules, latent_hw, channels):
        """the device tables of a LEDITS++ edit on the UNet batch [uncond | concept_1 .. concept_E] of ONE latent.  Everything a
        step varies with is a row of `scale`, selected by the LOOP's device step counter (`ledits_step`): this plan keeps no
        counter of its own moving, so a warm-up forward needs no muting."""
        dev = self.device
        E, (h, w) = int(scale.shape[1]), latent_hw
        check_ledits(E, thresholds)
        if len(thresholds) != E or len(token_counts) != E or tuple(scale.shape) != (self.num_steps + 1, E):
            raise ValueError(f"LEDITS++: {E} concepts need {E} thresholds, {E} token counts and a scale table "
                             f"[{self.num_steps + 1}, {E}]")
        if h * w > 16384 or not 1 <= channels <= 16:
            raise ValueError(f"LEDITS++: latents of {channels} x {h} x {w}; the mask kernels hold h w <= 16384 pixels and <= 16 channels")
        self.num_prompts, self.batch = E, 1 + E
        led = self.led = {"E": E, "cross": bool(cross_mask), "intersect": bool(intersect_mask), "hw": (int(h), int(w)),
                          "modules": tuple(int(i) for i in modules) if cross_mask else ()}
        f32 = dict(dtype=torch.float32, device=dev)
        led["scale"] = scale.to(**f32).contiguous()
        led["scale_cur"] = torch.zeros(E, **f32)
        led["w"] = ledits_token_weights(token_counts).to(dev)
        led["taps"] = ledits_taps().to(dev)
        led["rank_attn"] = ledits_rank_table(thresholds, self.MAP_TOKENS).to(dev)
        led["rank_pix"] = ledits_rank_table(thresholds, h * w).to(dev)
        led["acc"] = torch.zeros(E, self.MAP_TOKENS, **f32)
        led["m1"] = torch.zeros(E, self.MAP_TOKENS, **f32)
        led["mask"] = torch.zeros(E, h, w, **f32)
        led["thres"] = torch.zeros(E, **f32)

    def _ledits_mass(self, B: int, N: int, attn, q, k):
        """one of the five 16 x 16 modules adds the head-mean map of every concept row, summed over the concept's own tokens"""
        led = self.led
        if attn._exec_index not in led["modules"]:
            return
        if N != self.MAP_TOKENS:
            raise RuntimeError(f"{attn.layer_name}: the cross-attention mask was lowered for the UNet's configured sample size, where "
                               f"this module has {self.MAP_TOKENS} queries; it runs at {N}")
        if B != self.batch or q.shape[0] != B or k.shape[0] != B or k.shape[1] != self.CTX_TOKENS:
            raise RuntimeError(f"LEDITS++: cross-attention of batch {tuple(q.shape)} x {tuple(k.shape)}; the rule is stated for the "
                               f"batch [uncond | {led['E']} concepts] and {self.CTX_TOKENS} prompt tokens")
        hip.cross_blend_mass(q, k, attn.heads, attn.scale, 1, led["w"], led["acc"])

    def ledits_step(self, eps, lat, coef_cur, maps, step, x0_prev=None):
        """after the UNet of a step: the implicit masks and the guided eta = 1 update of the ONE latent `lat`, in place.  eps fp32
        [1 + E, C, h, w]; step: the loop's device counter, which picks the scale row and the noise map.  x0_prev (an order-2 loop's
        buffer, with its five-column coef_cur): the second-order SDE-DPM-Solver++ update instead (`hip.ledits_dpmpp_step`)"""
        led = self.led
        hip.select_step(led["scale"], led["scale_cur"], step)
        m1 = hip.ledits_attn_mask(led["acc"], led["taps"], led["rank_attn"], out=led["m1"]) if led["cross"] else None
        mask = None
        if led["cross"] or led["intersect"]:
            mask, _ = hip.ledits_guidance_mask(eps, m1, led["rank_pix"] if led["intersect"] else None, out=led["mask"],
                                               thres_out=led["thres"] if led["intersect"] else None)
        if x0_prev is not None:
            hip.ledits_dpmpp_step(eps, mask, led["scale_cur"], lat, coef_cur, maps, step, x0_prev, out=lat)
            return
        hip.ledits_ddpm_step(eps, mask, led["scale_cur"], lat, coef_cur, maps, step, out=lat)

    def _rewound(self, step: int):
        """the step counter was set from outside a forward: at step 0 a new run begins and the blend accumulator starts empty"""
        if self.blend_acc is not None and step == 0:
            self.blend_acc.zero_()

    def auto_launch(self, B: int, N: int, attn):
        """a controlled self-attention layer under 'masactrl_mask_auto', after the mutual launch: None (not controlled, or no
        slot written before it: plain mutual attention), or -- after launching the class kernel -- (target rows, their halves'
        source rows, gate, k_cls, q_cls) for the class-masked launch that overwrites the target rows"""
        if self.kind != "masactrl_mask_auto" or (attn._exec_index // 2) not in self.masa_layers:
            return None
        c = self.auto_layers.get(attn._exec_index, (0, N))[0]
        if c < 1:
            return None
        kc, qc = self._class_words(attn._exec_index, N)      # also in a muted warm-up forward: they exist before capture
        if self.muted:
            return None
        tgt, src = self._mask_rows[B]
        slots, _, thres = self._auto
        hip.masa_auto_classes(slots, c, thres, int(N ** 0.5), kc, qc, gate=self._gate[1])
        return tgt, src, self._gate[1], kc, qc

    def class_bits(self, layer: int, N: int = None):
        """(key bits, query bits) bool [N] on the host: what the class kernel last wrote for transformer layer `layer` (tests)"""
        for (ei, n), (kc, qc) in self._auto_cls.items():
            if ei // 2 == layer and (N is None or n == N):
                return hip.unpack_class_bits(kc, n), hip.unpack_class_bits(qc, n)
        raise KeyError(f"no class words for layer {layer}")

    def controls_first_self(self, unet, tokens: int) -> bool:
        """does this plan act, in ANY step of its schedule, on the self-attention of the UNet's first transformer (`tokens`
        queries)?  Decided from what `signature` states -- which layers, which token limit -- never from a step window or a
        table's contents: those change under a captured graph, and a re-pointed loop (`load_from`) keeps its launches.  The
        shared prefix of a CFG step (`denoise.cfg_shared_prefix_reason`) runs that self-attention once for both halves of the
        batch, which is only right while no plan redirects its rows."""
        blk = unet.down_blocks[0]
        if not blk.attentions:
            return False
        first = blk.attentions[0].transformer_blocks[0].attn1
        if self.kind == "p2p":         # `/root/reference/p2p/model/attention_base.py:133`: self-attention replace at <= 16^2 keys
            # a blend module reads the q and k rows of the conditional half of the FULL batch
            return tokens <= self.self_max_tokens or (first._exec_index + 1) in self.blend_modules
        if self.kind == "masactrl_mask_auto" and (first._exec_index + 1) in self.auto_slots:
            return True                # the first transformer's cross-attention writes a slot from rows c_src / c_tgt of the FULL batch
        if self.kind in self.MASA_KINDS:
            return (first._exec_index // 2) in self.masa_layers
        if self.kind == "pnp":
            return id(first) in self.pnp_layers
        return False

    # ------------------------------------------------------------------ re-use of a captured loop (denoise.acquire)
    def signature(self, unet):
        """everything about this plan that is BAKED into a captured step graph (which kernels run, on which modules,
        with tables of which shape); two plans with equal signatures differ only in table contents"""
        if self.kind == "p2p":
            sig = ("p2p", self.num_prompts, self.num_steps, self.self_max_tokens, tuple(self.mt.shape), self.cond_only,
                   hip.map_split_scale(self.coef_bound))
            # the blend's launches (which modules accumulate, the blend after the latent update) are baked in; its words and
            # threshold are data
            return sig if self.blend_w is None else sig + ("blend", self.blend_modules)
        if self.kind == "masactrl":
            return ("masactrl", tuple(sorted(self.masa_layers)), (max(self.masa_steps) + 2) if self.masa_steps else 1)
        if self.kind == "masactrl_union":     # one two-segment launch per controlled layer in every step; both tables are data
            return ("masactrl_union", tuple(sorted(self.masa_layers)), (max(self.masa_steps) + 2) if self.masa_steps else 1)
        if self.kind == "masactrl_mask":      # the list LENGTHS are launch arguments (grid, N, L); their contents are data
            # Computed from the masks, so asking builds nothing.  NOTE: it covers `mask_tokens`, which states the UNet's
            # configured sample size until a forward at another latent size adds its counts (mask_lists) -- denoise keys a
            # pooled loop BEFORE its warm-up, so at such a size two plans can match here and still differ in a length:
            # load_from checks every length and refuses the reuse loudly.
            lens = tuple((N, self.mask_lengths(N)) for N in self.mask_tokens)
            return ("masactrl_mask", tuple(sorted(self.masa_layers)), (max(self.masa_steps) + 2) if self.masa_steps else 1, lens)
        if self.kind == "masactrl_mask_auto":  # which modules write a slot and which layers read how many: launches; the rest is data
            return ("masactrl_mask_auto", tuple(sorted(self.masa_layers)), (max(self.masa_steps) + 2) if self.masa_steps else 1,
                    tuple(sorted(self.auto_slots.items())), tuple(sorted(self.auto_layers.items())))
        if self.kind == "pnp":
            idx = {id(m): m._exec_index for m in unet.attention_modules()}
            # the injected resnet as `pnp/model/register.py:_conv_module` picks it: resnets[0] on the SDXL family, else [1]
            inj = (unet.up_blocks[1].resnets[0 if unet.cfg.addition_embed else 1]._inject is self
                   if len(unet.up_blocks) > 1 else False)
            return ("pnp", tuple(sorted(idx[i] for i in self.pnp_layers)), self.num_steps, bool(inj))
        if self.kind == "ledits":             # which launches run and on which modules; concepts, scales and thresholds are data
            led = self.led
            return ("ledits", led["E"], self.num_steps, led["cross"], led["intersect"], led["modules"], led["hw"])
        return (self.kind,)

    def load_from(self, other: "ControlPlan", B: int):
        """take over `other`'s controller and table CONTENTS (same signature): the captured graph keeps reading this
        plan's device tensors"""
        self.controller = other.controller
        if self.kind == "p2p":
            self.mt.copy_(other.mt)
            self.mt32.copy_(other.mt32)
            self.coef_table.copy_(other.coef_table)
            self.coef_bound = other.coef_bound       # same split scale (the signatures matched), possibly another bound below it
            self.self_table.copy_(other.self_table)
            self.self_window = other.self_window
            if self.blend_w is not None:         # equal signatures: `other` has a blend part on the same modules
                self.blend_w.copy_(other.blend_w)
                self.blend_thres.copy_(other.blend_thres)
                if hasattr(self.controller, "_device_blend"):
                    self.controller._device_blend = self       # its step_callback blends from THIS plan's accumulator
        elif self.kind == "masactrl":
            other.prepare(B)
            self.masa_steps = set(other.masa_steps)
            self._masa[B][0].copy_(other._masa[B][0])
        elif self.kind == "masactrl_union":
            other.prepare(B)
            self.prepare(B)
            self.masa_steps = set(other.masa_steps)
            self._masa[B][0].copy_(other._masa[B][0])
            self._union[B][0].copy_(other._union[B][0])
        elif self.kind == "masactrl_mask":
            other.prepare(B)
            self.prepare(B)
            self.masa_steps = set(other.masa_steps)
            self.mask_s, self.mask_t = other.mask_s, other.mask_t
            self._masa[B][0].copy_(other._masa[B][0])
            self._gate[0].copy_(other._gate[0])
            for N in self.mask_tokens:             # equal lengths where the signatures covered N; checked for the rest
                if tuple(int(t.numel()) for t in self.mask_lists(N)) != other.mask_lengths(N):
                    raise RuntimeError(f"masactrl_mask: the captured graph holds lists of other lengths at {N} tokens than "
                                       "these masks give; this loop cannot be reused for them")
                for mine, theirs in zip(self.mask_lists(N), other.mask_lists(N)):
                    mine.copy_(theirs)
        elif self.kind == "masactrl_mask_auto":
            other.prepare(B)
            self.prepare(B)
            self.masa_steps = set(other.masa_steps)
            self.auto_thres, self.auto_ref, self.auto_cur = other.auto_thres, list(other.auto_ref), list(other.auto_cur)
            self._masa[B][0].copy_(other._masa[B][0])
            self._gate[0].copy_(other._gate[0])
            self._auto[1].copy_(other._auto[1])
            self._auto[2].copy_(other._auto[2])
        elif self.kind == "pnp":
            other.prepare(B)
            self.pnp_qk_steps, self.pnp_conv_steps = other.pnp_qk_steps, other.pnp_conv_steps
            self._pnp[B][0].copy_(other._pnp[B][0])
            self._pnp[B][2].copy_(other._pnp[B][2])
        elif self.kind == "ledits":
            for name in ("scale", "w", "rank_attn", "rank_pix"):
                self.led[name].copy_(other.led[name])

    # ------------------------------------------------------------------ per-forward protocol
    def applies(self, B: int) -> bool:
        if self.kind == "empty" or self.muted:
            return False
        if self.kind in self.MASA_KINDS or self.kind == "pnp":
            return True
        if B != self.batch:
            raise RuntimeError(
                f"controller was built for {self.num_prompts} prompts (UNet batch {self.batch}) but the UNet was "
                f"called with batch {B}; the reference's AttentionControlEdit.forward would mis-reshape here")
        return True

    def begin_forward(self, B: int):
        if self.kind == "ledits":
            # the method reads the CURRENT step's maps (unlike LocalBlend's running sum): the accumulator is emptied every forward,
            # inside the captured graph; nothing else of this plan moves with a forward, so a muted warm-up runs it whole
            if B != self.batch:
                raise RuntimeError(f"LEDITS++ was lowered for {self.led['E']} concepts (UNet batch {self.batch}) but the UNet was "
                                   f"called with batch {B}")
            if self.led["cross"]:
                self.led["acc"].zero_()
            return
        if not self.applies(B):
            return
        if not self.captured:
            # keep the device counter equal to the controller's (covers reset() / manual edits)
            cs = int(self.controller.cur_step)
            if cs > self.num_steps and self.kind == "p2p":
                raise IndexError(f"cur_step {cs} exceeds the controller's {self.num_steps}-step tables")
            self.step.fill_(cs)
            self._rewound(cs)
        if self.kind == "p2p":
            hip.select_step(self.coef_table, self.coef_cur, self.step)
            hip.select_step(self.self_table, self.self_cur, self.step)
            if self.blend_w is not None:
                hip.select_step(self.blend_w, self.blend_w_cur, self.step)
        elif self.kind in self.MASA_KINDS:
            if B not in self._masa:
                if self.captured:
                    raise RuntimeError("ControlPlan.prepare(B) must run before graph capture")
                self.prepare(B)
            tab, cur = self._masa[B]
            if not self.captured and int(self.controller.cur_step) >= tab.shape[0]:
                self.step.fill_(tab.shape[0] - 1)   # past the last controlled step: identity row
            hip.select_step(tab, cur, self.step)
            if self.kind in self.GATED_KINDS:       # the gate table has the same rows: 0 in the identity row past the end
                hip.select_step(self._gate[0], self._gate[1], self.step)
            if self.kind == "masactrl_union":       # the second-segment table has the same rows: -1 in the row past the end
                hip.select_step(self._union[B][0], self._union[B][1], self.step)
        elif self.kind == "pnp":
            if B not in self._pnp:
                if self.captured:
                    raise RuntimeError("ControlPlan.prepare(B) must run before graph capture")
                self.prepare(B)
            qk, qk_cur, cv, cv_cur = self._pnp[B]
            if not self.captured and int(self.controller.cur_step) >= qk.shape[0]:
                self.step.fill_(qk.shape[0] - 1)    # past the schedule: identity rows
            hip.select_step(qk, qk_cur, self.step)
            hip.select_step(cv, cv_cur, self.step)

    def end_forward(self, B: int):
        if (self.kind in self.MASA_KINDS or self.kind == "pnp") and not self.muted:
            hip.advance_step(self.step)
        elif self.kind not in ("empty", "ledits") and not self.muted and B == self.batch:
            hip.advance_step(self.step)

    def layer_done(self, attn):
        if not self.captured and not self.muted and self.controller is not None:
            advance_controller(self.controller)

    def sync_step(self):
        """device step counter <- controller.cur_step (before the first replay of a captured loop)"""
        self.step.fill_(int(self.controller.cur_step))
        self._rewound(int(self.controller.cur_step))

    def replay_done(self):
        """one whole forward was replayed from a graph: num_att_layers controller calls happened"""
        c = self.controller
        if c is not None:
            c.cur_step += 1
            _step_hook(c)

    # ------------------------------------------------------------------ what the kernels read
    def self_sources(self, B: int, N: int, attn):
        if self.kind == "p2p" and self.applies(B) and N <= self.self_max_tokens:
            return self.self_cur, self.self_cur, None
        if self.kind in self.MASA_KINDS and not self.muted and (attn._exec_index // 2) in self.masa_layers:
            cur = self._masa[B][1]
            return None, cur, cur
        if self.kind == "pnp" and not self.muted and id(attn) in self.pnp_layers:
            cur = self._pnp[B][1]
            return cur, cur, None
        return None, None, None

    def second_sources(self, B: int, attn):
        """'masactrl_union', a controlled self-attention layer: the current second-segment rows (`k2_src = v2_src` of the planes
        attention, beside the `self_sources` rows of the first segment); None everywhere else"""
        if self.kind == "masactrl_union" and not self.muted and (attn._exec_index // 2) in self.masa_layers:
            return self._union[B][1]
        return None

    def feature_source(self, B: int):
        """source rows of the Plug-and-Play feature injection for the CURRENT step (identity outside its schedule)"""
        if self.kind == "pnp" and not self.muted and B in self._pnp:
            return self._pnp[B][3]
        return None

    def cross_edit(self, B: int, attn):
        if self.kind == "p2p" and self.applies(B):
            mt = self.mt32 if attn.to_q.weight.dtype == torch.float32 else self.mt
            args = dict(edit_src=self.edit_src, edit_slot=self.edit_slot, mt=mt, coef=self.coef_cur)
            if attn.to_q.weight.dtype == torch.float32:
                args["coef_bound"] = self.coef_bound
            return args
        return {}
