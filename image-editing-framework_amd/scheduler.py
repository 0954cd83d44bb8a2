"""DDIM scheduler with the attribute surface the reference's loops touch.

The reference builds `diffusers.DDIMScheduler.from_config(cfg)` with the dict at
`/root/reference/p2p/edit_syn.py:46-57` and then reads (SURVEY.md §8b "Pipeline attrs"):
`set_timesteps`, `timesteps`, `init_noise_sigma`, `step(eps, t, x)["prev_sample"]` /
`.prev_sample` / `['pred_original_sample']`, `config.num_train_timesteps`,
`num_inference_steps`, `alphas_cumprod`, `final_alpha_cumprod`, `scale_model_input`, `order`.

Constants and the update rule restate diffusers' implementation [ext]:
    betas = linspace(sqrt(b0), sqrt(b1), T)^2 ; ac = cumprod(1 - betas)          (fp32)
    timesteps "leading": arange(n) * (T // n), reversed, + steps_offset
    step (eta = 0, epsilon prediction, no clipping):
        x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t);  x' = sqrt(a_p) x0 + sqrt(1 - a_p) eps
The elementwise update itself runs in the HIP kernel `ief_ddim_step` (csrc/elementwise.hip).
"""
from types import SimpleNamespace

import numpy as np
import torch

from .config import SCHEDULER_CONFIG


class SchedulerOutput(dict):
    """Supports both `out["prev_sample"]` and `out.prev_sample` (both forms occur:
    `/root/reference/p2p/model/sd_utils.py:76`, `/root/reference/p2p/inversion/nti.py:25`)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class DDIMScheduler:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, **config):
        cfg = dict(SCHEDULER_CONFIG)
        cfg.update(config)
        if cfg["beta_schedule"] != "scaled_linear" or cfg["trained_betas"] is not None:
            raise ValueError("only the reference's scaled_linear schedule is supported")
        self.config = SimpleNamespace(**cfg)
        T = cfg["num_train_timesteps"]
        betas = torch.linspace(cfg["beta_start"] ** 0.5, cfg["beta_end"] ** 0.5, T, dtype=torch.float32) ** 2
        self.betas = betas
        self.alphas = 1.0 - betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.final_alpha_cumprod = torch.tensor(1.0) if cfg["set_alpha_to_one"] else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, T)[::-1].copy().astype(np.int64))

    @classmethod
    def from_config(cls, config):
        return cls(**dict(config))

    def set_timesteps(self, num_inference_steps: int, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError("num_inference_steps exceeds num_train_timesteps")
        self.num_inference_steps = num_inference_steps
        ratio = T // num_inference_steps
        ts = (np.arange(0, num_inference_steps) * ratio).round()[::-1].copy().astype(np.int64)
        ts = ts + self.config.steps_offset
        self.timesteps = torch.from_numpy(ts)
        if device is not None:
            self.timesteps = self.timesteps.to(device)

    def scale_model_input(self, sample, timestep=None):
        return sample

    # ------------------------------------------------------------------ coefficients
    def step_coeffs(self, t: int):
        """(a_t, a_prev) as python floats taken from the fp32 table."""
        t = int(t)
        prev = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_p = float(self.alphas_cumprod[prev]) if prev >= 0 else float(self.final_alpha_cumprod)
        return a_t, a_p

    def reverse_coeffs(self, t: int):
        """(a_cur, a_next) of `ddim_reverse` (`/root/reference/p2p/inversion/ddim.py:9-18`)."""
        nxt = int(t)
        T = self.config.num_train_timesteps
        cur = min(T - 1, nxt - T // self.num_inference_steps)
        a_c = float(self.alphas_cumprod[cur]) if cur >= 0 else float(self.final_alpha_cumprod)
        return a_c, float(self.alphas_cumprod[nxt])

    def ddpm_coeffs(self, t: int):
        """(a_t, a_prev, sigma, dir) of the eta = 1 step at timestep t (edit-friendly DDPM inversion, `p2p.inversion.ddpm`):
            v = (1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev);  sigma = sqrt(v);  dir = sqrt(1 - a_prev - v)
        a_t / a_prev are `step_coeffs`' fp32 table values; sigma and dir are formed here in fp64 and rounded to fp32 (returned as
        python floats that hold fp32 values), so dir^2 + sigma^2 = 1 - a_prev to fp32 rounding.  v is clamped at 0 from below and
        1 - a_prev - v likewise: a step with sigma == 0 adds no noise."""
        a_t, a_p = self.step_coeffs(t)
        v = max(0.0, (1.0 - a_p) / (1.0 - a_t) * (1.0 - a_t / a_p))
        d = max(0.0, 1.0 - a_p - v)
        return a_t, a_p, float(np.float32(np.sqrt(v))), float(np.float32(np.sqrt(d)))

    @staticmethod
    def dpmpp_c2(a_before: float, a_t: float, a_prev: float) -> float:
        """the coefficient of the second-order correction of the multistep SDE-DPM-Solver++ step a_t -> a_prev that follows the
        step a_before -> a_t: with lambda(a) = 1/2 log(a / (1 - a)), h = lambda(a_prev) - lambda(a_t), h_before = lambda(a_t) -
        lambda(a_before) and v = (1 - a_prev) (1 - e^{-2h}) in `ddpm_coeffs`' form,
            c2 = 1/2 sqrt(a_prev) (v / (1 - a_prev)) (h / h_before)
        in fp64, rounded to fp32 once (a python float that holds an fp32 value)."""
        if not 0.0 < a_before < a_t < a_prev < 1.0:
            raise ValueError(f"dpmpp_c2: an order-2 step needs 0 < a_before < a_t < a_prev < 1, got {a_before}, {a_t}, {a_prev}")
        lam = lambda a: 0.5 * np.log(a / (1.0 - a))
        v = max(0.0, (1.0 - a_prev) / (1.0 - a_t) * (1.0 - a_t / a_prev))
        h, h_before = lam(a_prev) - lam(a_t), lam(a_t) - lam(a_before)
        return float(np.float32(0.5 * np.sqrt(a_prev) * (v / (1.0 - a_prev)) * (h / h_before)))

    def dpmpp_coeffs(self, t: int, order2: bool):
        """(a_t, a_prev, sigma, dir, c2) of the SDE-DPM-Solver++ step at timestep t.  The first four ARE `ddpm_coeffs(t)`: with
        lambda(a) = 1/2 log(a / (1 - a)) and h = lambda(a_prev) - lambda(a_t), sigma_prev^2 (1 - e^{-2h}) is its v and
        sigma_prev e^{-h} its dir, so the first-order solver is the eta = 1 update.  c2 (`dpmpp_c2`) weighs the correction
        x0 - x0_before of an order-2 step, 0.0 for an order-1 step; the step before this one ran t + T // S.  `dpmpp_orders` says
        which steps of a schedule are order 2 (never the first one run, never the last)."""
        coef = self.ddpm_coeffs(t)
        if not order2:
            return (*coef, 0.0)
        before = int(t) + self.config.num_train_timesteps // self.num_inference_steps
        if before >= self.config.num_train_timesteps:
            raise ValueError(f"dpmpp_coeffs: no step runs before timestep {int(t)} of this schedule; its step is order 1")
        return (*coef, self.dpmpp_c2(float(self.alphas_cumprod[before]), coef[0], coef[1]))

    @staticmethod
    def dpmpp_orders(num_steps: int, skip: int, solver_order: int):
        """the order of step i = 0 .. num_steps - 1 of a schedule whose run starts at step `skip` (steps before it are not run and
        count as order 1): order 1 on the first step run, on the last step (the published multistep solver's final step, where h
        jumps to the end of the schedule) and everywhere for solver_order 1; order 2 otherwise"""
        if solver_order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2, got {solver_order!r}")
        if not isinstance(skip, int) or isinstance(skip, bool) or not 0 <= skip < num_steps:
            raise ValueError(f"skip must be an integer in [0, {num_steps}), got {skip!r}")
        return [2 if (solver_order == 2 and skip < i < num_steps - 1) else 1 for i in range(num_steps)]

    def dpmpp_table(self, skip: int, solver_order: int):
        """[dpmpp_coeffs(t_i, order of step i)] for the steps i = skip .. S - 1 of the current schedule"""
        ts = self.timesteps.tolist()
        orders = self.dpmpp_orders(len(ts), skip, solver_order)
        return [self.dpmpp_coeffs(t, o == 2) for t, o in zip(ts[skip:], orders[skip:])]

    @staticmethod
    def linear_form(a_from: float, a_to: float):
        """x' = cx * x + ce * eps  for  x0=(x-sqrt(1-a_from)eps)/sqrt(a_from); x'=sqrt(a_to)x0+sqrt(1-a_to)eps.

        Used by the fused CFG+DDIM kernel, which evaluates x0 and x' in the same operation
        order as the formula above (not this folded form) to stay bit-close to the reference.
        """
        cx = (a_to / a_from) ** 0.5
        ce = (1 - a_to) ** 0.5 - cx * (1 - a_from) ** 0.5
        return cx, ce

    # ------------------------------------------------------------------ update
    def step(self, model_output, timestep, sample, eta: float = 0.0, return_dict: bool = True, **kw):
        if eta != 0.0:
            raise ValueError("only eta = 0 (deterministic DDIM) is on the reference path")
        a_t, a_p = self.step_coeffs(int(timestep))
        if model_output.requires_grad or sample.requires_grad:
            # differentiable form for null-text inversion (`inversion/nti.py:25-28`)
            x0 = (sample - (1 - a_t) ** 0.5 * model_output) / a_t ** 0.5
            prev = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * model_output
        else:
            from . import hip
            prev, x0 = hip.ddim_step(model_output, sample, a_t, a_p)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev, pred_original_sample=x0)
