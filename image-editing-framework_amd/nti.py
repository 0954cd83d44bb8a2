"""Null-text optimisation engine: the loop of `/root/reference/p2p/inversion/nti.py:9-45` on the HIP kernels.

Per DDIM timestep i the reference
  1. computes eps_cond once (no grad),
  2. runs <= num_inner_steps of {UNet(uncond) -> CFG -> scheduler.step -> mse against the inversion latent ->
     backward -> Adam}, stopping early when the loss (of the PRE-update embedding) falls under eps + 2e-5 i,
  3. advances latent_cur with the optimised embedding.
Here each of the three is ONE captured hipGraph over static buffers (a fresh Adam per timestep = zeroed
moments and step counter, lr in a device scalar), so an inner iteration costs one graph replay plus the
host read of the loss that the early-stop rule needs — exactly the reference's `loss.item()`.

The gradient is not torch autograd: `grad.UNetAdjoint` chains activation-gradient kernels (weights are
frozen on this path).  Everything that varies with the timestep is a row of a device table.
"""
from typing import List, Optional

import torch

from . import hip
from .grad import UNetAdjoint


class _NullTextLoop:
    """What the per-image and the batched optimiser share: the static buffers with `rows` images in their leading dimension,
    the per-timestep tables, the cond-forward and tail bodies, graph capture and replay.  A subclass adds `_body_inner` and
    its own begin / outer_begin / inner_step / outer_end / run protocol."""

    def __init__(self, model, cond: torch.Tensor, guidance_scale: float, latent_hw, rows: int, grad_scale: float, use_graph: bool,
                 added_cond, added_uncond, lr: float, restart: bool, lr_decay: float):
        self._rows = int(rows)
        self.model, self.unet, self.sched = model, model.unet, model.scheduler
        dev = self.unet.device
        self.dev = dev
        self.adj = UNetAdjoint(self.unet, grad_scale)
        self.adj.prepack()
        h, w = latent_hw
        C, K = self.unet.config.in_channels, self._rows
        f32 = dict(dtype=torch.float32, device=dev)
        self.lat = torch.zeros(K, C, h, w, **f32)
        self.target = torch.zeros(K, C, h, w, **f32)
        self.eps_c = torch.zeros(K, C, h, w, **f32)
        self.d_eps = torch.zeros(K, C, h, w, **f32)
        self.hyper = torch.tensor([1e-2, 0.9, 0.999, 1e-8], **f32)     # torch.optim.Adam defaults (nti.py:17)
        self.adam_step = torch.zeros(1, dtype=torch.int32, device=dev)
        ts = self.sched.timesteps.tolist()
        self.num_steps = len(ts)
        g = float(guidance_scale)
        self.coef_table = torch.tensor([[*self.sched.step_coeffs(t), g, 0.0] for t in ts], **f32)
        self.coef = torch.zeros(4, **f32)
        tsd = torch.tensor(ts, **f32)
        self.temb_table = self.unet.time_rows(tsd, self.unet.aug_embedding(added_uncond)).contiguous()     # uncond calls
        self.temb = torch.zeros(1, self.temb_table.shape[1], **f32)
        if added_cond is not None:
            self.temb_table_c = self.unet.time_rows(tsd, self.unet.aug_embedding(added_cond)).contiguous()
            self.temb_c = torch.zeros_like(self.temb)
        else:
            self.temb_table_c, self.temb_c = self.temb_table, self.temb
        self.lr, self.restart, self.lr_decay = float(lr), bool(restart), float(lr_decay)      # lr_i = lr (1 - i / lr_decay)
        self.f32 = self.unet.dtype == torch.float32          # fp32-storage modes: the context the UNet reads IS the parameter
        self.cond16 = self.unet._act(cond.to(dev))
        L, Cc = self.cond16.shape[1:]
        self.param = torch.zeros(K, L, Cc, **f32)
        self.m = torch.zeros_like(self.param)
        self.v = torch.zeros_like(self.param)
        self.p16 = self.param if self.f32 else torch.zeros(K, L, Cc, dtype=torch.float16, device=dev)
        self.use_graph = use_graph
        self._graphs = None
        self.inner_steps_run: List[int] = []     # per timestep, how many Adam steps the early-stop rule allowed
        self.last_losses: List[float] = []

    # ------------------------------------------------------------------ the three stream-ordered bodies
    def _body_cond(self):
        eps = self.unet(self.lat, encoder_hidden_states=self.cond16, temb_row=self.temb_c)["sample"]
        self.eps_c.copy_(eps)

    def _body_tail(self):
        eps_u = self.unet(self.lat, encoder_hidden_states=self.p16, temb_row=self.temb)["sample"]
        hip.cfg_ddim_step(eps_u, self.eps_c, self.lat, self.coef, out=self.lat)

    def _sync_p16(self):
        if not self.f32:
            hip.to_f16(self.param, out=self.p16)

    def _capture(self):
        for m in self.unet.attention_modules():
            m.cache_kv = False          # the uncond context changes under the same buffer: never cache its K/V
        state = [self.lat, self.param, self.m, self.v, self.adam_step, self.eps_c] + ([] if self.f32 else [self.p16])
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        need = []
        with torch.cuda.stream(s):          # warm-up: allocator pools, packed adjoint weights
            for body in (self._body_cond, self._body_inner, self._body_tail):
                used0 = hip.counters_used()
                body()
                need.append(hip.counters_used() - used0)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graphs, self._arenas = [], []
        for body, n in zip((self._body_cond, self._body_inner, self._body_tail), need):
            arena = hip.counter_arena(n, self.dev)      # this graph's own split-K arrival counters
            g = torch.cuda.CUDAGraph()
            with arena, torch.cuda.graph(g):
                body()
            graphs.append(g)
            self._arenas.append(arena)
        for t, sv in zip(state, saved):
            t.copy_(sv)
        self._graphs = graphs

    def _run(self, which: int):
        if self._graphs is not None:
            self._graphs[which].replay()
        else:
            (self._body_cond, self._body_inner, self._body_tail)[which]()

    def _ready(self):
        """from `begin`: capture on first use; eager runs only switch the K/V cache off"""
        if self.use_graph and self._graphs is None:
            self._capture()
        elif not self.use_graph:
            for m in self.unet.attention_modules():
                m.cache_kv = False

    def release(self):
        self._graphs = None
        for m in self.unet.attention_modules():
            m.cache_kv = True
            m._kv_key, m._kv = None, None


class NullTextOptimizer(_NullTextLoop):
    def __init__(self, model, cond: torch.Tensor, guidance_scale: float, latent_hw, grad_scale: float = 1.0,
                 use_graph: bool = True, added_cond=None, added_uncond=None, lr: float = 1e-2, restart: bool = False,
                 lr_decay: float = 100.0):
        """added_cond / added_uncond, lr, restart: `NTI_XL` (`/root/reference/pix2pix-zero/inversion/nti.py:47-96`) — the
        conditional and unconditional UNet calls take their own SDXL `added_cond_kwargs` (folded into two tables of
        per-step time-embedding rows), lr = 5e-2, and the embedding restarts from its initial value every timestep."""
        super().__init__(model, cond, guidance_scale, latent_hw, 1, grad_scale, use_graph, added_cond, added_uncond, lr, restart,
                         lr_decay)
        self.stats = torch.zeros(2, dtype=torch.float32, device=self.dev)                 # (loss, factor)

    def _body_inner(self):
        eps_u = self.adj.forward(self.lat, self.temb, self.p16)
        hip.nti_loss_grad(eps_u, self.eps_c, self.lat, self.target, self.coef, self.d_eps, self.stats, self.adj.grad_scale)
        g16 = self.adj.backward(self.d_eps)
        hip.nti_adam(self.param, self.m, self.v, g16, self.stats, self.hyper, self.adam_step, self.p16)

    # ------------------------------------------------------------------ public: one image = begin, then per timestep
    # outer_begin -> inner_step / inner_loss ... -> outer_end  (so several images can be interleaved: `run_many`)
    def begin(self, latents: List[torch.Tensor], uncond: torch.Tensor):
        dev = self.dev
        self._latents = latents
        self.lat.copy_(latents[-1].to(dev).float())
        self.param.copy_(uncond.to(dev).float()[:1])
        self._param0 = self.param.clone()
        self._sync_p16()
        self._ready()
        self.out: List[torch.Tensor] = []
        self.inner_steps_run, self.last_losses = [], []

    def outer_begin(self, i: int):
        latents = self._latents
        self.temb.copy_(self.temb_table[i:i + 1])
        if self.temb_c is not self.temb:
            self.temb_c.copy_(self.temb_table_c[i:i + 1])
        if self.restart:
            self.param.copy_(self._param0)
            self._sync_p16()
        self.coef.copy_(self.coef_table[i])
        self.target.copy_(latents[len(latents) - i - 2].to(self.dev).float())
        self.m.zero_(), self.v.zero_(), self.adam_step.zero_()          # `Adam([uncond], lr=...)` anew (nti.py:17)
        self.hyper[0:1].fill_(self.lr * (1.0 - i / self.lr_decay))
        self._run(0)
        self._done, self._loss = 0, float("nan")

    def inner_step(self):
        self._run(1)
        self._done += 1

    def inner_loss(self) -> float:
        """loss of the embedding BEFORE the Adam step just taken (what the reference's `loss.item()` reads, :31)"""
        self._loss = float(self.stats[0].item())
        return self._loss

    def outer_end(self):
        self.inner_steps_run.append(self._done)
        self.last_losses.append(self._loss)
        self.out.append(self.param.clone())
        self._run(2)

    def run(self, latents: List[torch.Tensor], uncond: torch.Tensor, num_inner_steps: int, epsilon: float,
            num_outer: Optional[int] = None) -> List[torch.Tensor]:
        """latents: the 51 inversion latents (x_0 .. x_T); uncond [1,77,C].  Returns one [1,77,C] fp32 per timestep."""
        self.begin(latents, uncond)
        n = self.num_steps if num_outer is None else num_outer
        for i in range(n):
            self.outer_begin(i)
            for j in range(num_inner_steps):
                self.inner_step()
                if self.inner_loss() < epsilon + i * 2e-5:
                    break
            self.outer_end()
        return self.out


def run_many(opts: List[NullTextOptimizer], latents_list, uncond_list, num_inner_steps: int, epsilon: float,
             num_outer: Optional[int] = None) -> List[List[torch.Tensor]]:
    """Null-text optimisation of several independent images in flight, each on its own stream.

    An inner iteration is ~900 dependent launches at UNet batch 1 — almost pure dispatch latency — so E images
    stepped in turn fill each other's gaps.  Every image keeps its own early stop; per round the host reads one loss
    per still-active image (the reference's `loss.item()`, one image at a time there).  Same values as `run` per image."""
    cur = torch.cuda.current_stream()
    streams = [torch.cuda.Stream() for _ in opts]
    for o, lat, unc in zip(opts, latents_list, uncond_list):
        o.begin(lat, unc)                       # captures on first use (sequential: graphs share the UNet modules)
    for s in streams:
        s.wait_stream(cur)
    n = min(o.num_steps for o in opts) if num_outer is None else num_outer
    for i in range(n):
        for o, s in zip(opts, streams):
            with torch.cuda.stream(s):
                o.outer_begin(i)
        active = list(range(len(opts)))
        for j in range(num_inner_steps):
            for k in active:
                with torch.cuda.stream(streams[k]):
                    opts[k].inner_step()
            still = []
            for k in active:
                with torch.cuda.stream(streams[k]):
                    if opts[k].inner_loss() >= epsilon + i * 2e-5:
                        still.append(k)
            active = still
            if not active:
                break
        for o, s in zip(opts, streams):
            with torch.cuda.stream(s):
                o.outer_end()
    for s in streams:
        cur.wait_stream(s)
    torch.cuda.synchronize()
    return [o.out for o in opts]


def groups_of(n_items: int, batch: int) -> List[List[int]]:
    """indices 0 .. n_items-1 in consecutive groups of `batch`; only the last group may be smaller"""
    if batch < 1:
        raise ValueError("groups_of: batch must be >= 1")
    return [list(range(g0, min(g0 + batch, n_items))) for g0 in range(0, n_items, batch)]


def pad_group(items: list, batch: int) -> list:
    """a group of 1..batch items filled up to `batch` with copies of its last one"""
    if not 1 <= len(items) <= batch:
        raise ValueError(f"a group holds 1..{batch} images, got {len(items)}")
    return list(items) + [items[-1]] * (batch - len(items))


class BatchedNullTextOptimizer(_NullTextLoop):
    """Null-text optimisation of K images through ONE UNet batch: the three captured graphs of `NullTextOptimizer` (cond
    forward, inner iteration, tail) over static [K, ...] buffers.  All K images are at the same DDIM timestep, so the
    scheduler row, the time-embedding row, Adam's hyper-parameters and its step counter are shared; latents, targets, the
    embedding with its Adam moments, the objective's (loss, factor) pair and the early stop are per image
    (`hip.nti_loss_grad_batched`, `hip.nti_adam_batched`).

    Early stop: after every inner replay the host reads the K losses in one copy and applies the reference's rule
    (`/root/reference/p2p/inversion/nti.py:31-33`) to every image that is still active.  An image that satisfies it has
    taken that Adam step, as in `run`, and is switched off for the rest of the timestep: the graph keeps computing its
    row, the Adam kernel leaves its embedding and moments unwritten (`active[k] == 0`).  The flags are uploaded only when
    the set changes.  A group smaller than K is padded with copies of its last image; padded rows are never active and
    their results are dropped.  `begin(..., cond=)` loads a new group's conditional embeddings into the buffer the graphs
    read, so one optimiser serves every group of a run without capturing again.

    Serves what `NullTextOptimizer(restart=False)` serves, in all three precision modes.  The SDXL optimisers
    (`restart=True`, per-image `added_cond_kwargs`) are out of scope: they keep `run_many`."""

    def __init__(self, model, cond: torch.Tensor, guidance_scale: float, latent_hw, batch: int, grad_scale: float = 1.0,
                 use_graph: bool = True, lr: float = 1e-2, lr_decay: float = 100.0):
        """cond: [1,77,C] (every row) or [K,77,C]; `begin(cond=)` replaces it per group."""
        if batch < 1:
            raise ValueError("BatchedNullTextOptimizer: batch must be >= 1")
        K = int(batch)
        cond = cond.expand(K, -1, -1) if cond.shape[0] == 1 else cond
        if cond.shape[0] != K:
            raise ValueError(f"BatchedNullTextOptimizer: cond has {cond.shape[0]} rows, batch is {K}")
        super().__init__(model, cond, guidance_scale, latent_hw, K, grad_scale, use_graph, None, None, lr, False, lr_decay)
        self.cond16 = self.cond16.clone()           # a static buffer of this optimiser's own (`_act` may hand back its argument)
        self.stats = torch.zeros(K, 2, dtype=torch.float32, device=self.dev)              # (loss, factor) per image
        self.active = torch.zeros(K, dtype=torch.int32, device=self.dev)
        self._flags = [0] * K
        self.n_real = K

    def suspend(self):
        """between groups, while other work runs on the UNet: the attention modules cache K/V again; the graphs stay"""
        for m in self.unet.attention_modules():
            m.cache_kv = True
            m._kv_key, m._kv = None, None

    def _body_inner(self):
        eps_u = self.adj.forward(self.lat, self.temb, self.p16)
        hip.nti_loss_grad_batched(eps_u, self.eps_c, self.lat, self.target, self.coef, self.d_eps, self.stats,
                                  self.adj.grad_scale)
        g = self.adj.backward(self.d_eps)
        hip.nti_adam_batched(self.param, self.m, self.v, g, self.stats, self.active, self.hyper, self.adam_step, self.p16)

    def _set_active(self, flags):
        if flags != self._flags:
            self._flags = list(flags)
            self.active.copy_(torch.tensor(self._flags, dtype=torch.int32))

    def begin(self, latents_list, uncond_list, cond=None):
        """latents_list[k]: the inversion latents x_0 .. x_T of image k; uncond_list[k]: its [1,77,C]; cond: the group's
        conditional embeddings, a [n,77,C] tensor or a list of [1,77,C] (None keeps what the buffer holds)."""
        dev, K = self.dev, self._rows
        self.n_real = n = len(latents_list)
        if len(uncond_list) != n:
            raise ValueError("BatchedNullTextOptimizer.begin: one unconditional embedding per image")
        self._latents = pad_group(latents_list, K)
        if cond is not None:
            rows = [cond[k:k + 1] for k in range(cond.shape[0])] if isinstance(cond, torch.Tensor) else [c[:1] for c in cond]
            if len(rows) != n:
                raise ValueError("BatchedNullTextOptimizer.begin: one conditional embedding per image")
            self.cond16.copy_(self.unet._act(torch.cat([c.to(dev) for c in pad_group(rows, K)])))
        self.lat.copy_(torch.cat([l[-1].to(dev).float() for l in self._latents]))
        self.param.copy_(torch.cat([u.to(dev).float()[:1] for u in pad_group(uncond_list, K)]))
        self._sync_p16()
        self._flags = None                          # unknown on the device until `outer_begin` uploads them
        self._ready()
        self.out: List[List[torch.Tensor]] = [[] for _ in range(n)]
        self.inner_steps_run = [[] for _ in range(n)]       # [k][timestep]: Adam steps image k took
        self.last_losses = [[] for _ in range(n)]

    def outer_begin(self, i: int):
        lats = self._latents
        self.temb.copy_(self.temb_table[i:i + 1])
        self.coef.copy_(self.coef_table[i])
        self.target.copy_(torch.cat([l[len(l) - i - 2].to(self.dev).float() for l in lats]))
        self.m.zero_(), self.v.zero_(), self.adam_step.zero_()          # `Adam([uncond], lr=...)` anew (nti.py:17)
        self.hyper[0:1].fill_(self.lr * (1.0 - i / self.lr_decay))
        self._set_active([1] * self.n_real + [0] * (self._rows - self.n_real))
        self._run(0)
        self._done, self._loss = [0] * self.n_real, [float("nan")] * self.n_real

    def inner_step(self):
        self._run(1)
        for k in range(self.n_real):
            self._done[k] += self._flags[k]

    def inner_losses(self) -> List[float]:
        """the K losses of the embeddings BEFORE the Adam step just taken, in one device-to-host copy; recorded for the
        images that took the step"""
        losses = [row[0] for row in self.stats.tolist()]
        for k in range(self.n_real):
            if self._flags[k]:
                self._loss[k] = losses[k]
        return losses

    def stop(self, ks):
        """switch images `ks` off for the rest of the timestep"""
        flags = list(self._flags)
        for k in ks:
            flags[k] = 0
        self._set_active(flags)

    def any_active(self) -> bool:
        return any(self._flags)

    def outer_end(self):
        for k in range(self.n_real):
            self.inner_steps_run[k].append(self._done[k])
            self.last_losses[k].append(self._loss[k])
            self.out[k].append(self.param[k:k + 1].clone())
        self._run(2)

    def run(self, latents_list, uncond_list, num_inner_steps: int, epsilon: float, num_outer: Optional[int] = None,
            cond=None) -> List[List[torch.Tensor]]:
        """Returns, per image of the group, one [1,77,C] fp32 per timestep (what `NullTextOptimizer.run` returns for it)."""
        self.begin(latents_list, uncond_list, cond)
        n = self.num_steps if num_outer is None else num_outer
        for i in range(n):
            self.outer_begin(i)
            for j in range(num_inner_steps):
                self.inner_step()
                losses = self.inner_losses()
                self.stop([k for k in range(self.n_real) if self._flags[k] and losses[k] < epsilon + i * 2e-5])
                if not self.any_active():
                    break
            self.outer_end()
        return self.out
