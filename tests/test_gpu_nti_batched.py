"""Null-text optimisation of K images in one UNet batch (`ief_amd.nti.BatchedNullTextOptimizer`) on a real MI355X.

The reference optimises one image at a time (`/root/reference/p2p/inversion/nti.py:9-45`); the batched optimiser takes K
images that are at the same DDIM timestep through one UNet batch, every image with its own objective, Adam state and early
stop.  What is held here:
    the batched objective / Adam kernels          bit-equal to the single-image kernels on every slice; a gated image unwritten
    K = 1                                         bit-identical to `NullTextOptimizer.run` in all three precision modes
    the same image twice (K = 2)                  rows bit-equal after every timestep
    a real group vs the fp32 autograd oracle      every element with a resolvable gradient <= 1e-2 of the timestep's movement,
                                                  unresolved elements <= 5 % of all and <= 2.1 movements (the bounds and the
                                                  protocol of tests/test_gpu_grad_f32.py::test_nti_loop_fp32_modes_elementwise)
    ragged early stop                             per-image step counts; a stopped image's embedding frozen bit for bit
    graph == eager, reuse across groups, padding
All on the `synthetic:tiny` family, 4-step schedule, 3 timesteps x 3 inner steps.
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from ief_amd import hip  # noqa: E402
from ief_amd.nti import BatchedNullTextOptimizer, NullTextOptimizer  # noqa: E402
from ief_amd.pipeline import StableDiffusionPipeline  # noqa: E402
from oracle import p2p_ref  # noqa: E402

DEV = torch.device("cuda:0")
STEPS, INNER, OUTER, GS = 4, 3, 3, 7.5
NOISE = 1e-3            # a gradient below this share of the largest is not resolved by the fp32 pass (test_gpu_grad_f32.py)
NEVER = -1.0            # epsilon that disables the early stop: loss < -1 + i * 2e-5 never holds


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [4 * 16 * 16, 2304, 4 * 64 * 64])
def test_loss_grad_batched_bit_equal_to_single(n):
    K = 3
    g = torch.Generator().manual_seed(n)
    eu, ec, x, tgt = (torch.randn(K, n, generator=g) for _ in range(4))
    for t in (eu, ec, x, tgt):
        t[1] = 0.0          # image 1: e = 0 + g (0 - 0) = 0, rec = sa_t ((0 - 0) / sa_f) + 0 = 0, target 0: every residual is exactly 0
    eu, ec, x, tgt = (t.to(DEV) for t in (eu, ec, x, tgt))
    a_f, a_t, gs = 0.31, 0.42, 7.5
    coef = torch.tensor([a_f, a_t, gs, 0.0], device=DEV)
    d_eps, stats = torch.full((K, n), 7.0, device=DEV), torch.full((K, 2), 7.0, device=DEV)
    hip.nti_loss_grad_batched(eu, ec, x, tgt, coef, d_eps, stats, 4.0)
    for k in range(K):
        d1, s1 = torch.full((n,), 9.0, device=DEV), torch.full((2,), 9.0, device=DEV)
        hip.nti_loss_grad(eu[k], ec[k], x[k], tgt[k], coef, d1, s1, 4.0)
        assert torch.equal(d_eps[k], d1) and torch.equal(stats[k], s1), k
    assert stats[1].abs().max().item() == 0.0 and d_eps[1].abs().max().item() == 0.0      # max |d| == 0: inv = 0, factor 0
    eur = eu[0].double().requires_grad_(True)
    e = eur + gs * (ec[0].double() - eur)
    rec = math.sqrt(a_t) * (x[0].double() - math.sqrt(1 - a_f) * e) / math.sqrt(a_f) + math.sqrt(1 - a_t) * e
    loss = ((rec - tgt[0].double()) ** 2).mean()
    loss.backward()
    e_loss = abs(stats[0, 0].item() - loss.item()) / loss.item()
    e_grad = ((d_eps[0].double() * stats[0, 1].double() - eur.grad).abs().max() / eur.grad.abs().max()).item()
    print(f"nti_loss_grad_batched n={n}: image 0 vs fp64: loss {e_loss:.2e}, gradient {e_grad:.2e}")
    assert e_loss <= 1e-5 and abs(d_eps[0].abs().max().item() - 4.0) < 1e-5 and e_grad < 1e-5


@pytest.mark.parametrize("grad_dtype", [torch.float16, torch.float32])
def test_adam_batched_gate_and_bit_equality(grad_dtype):
    K, n, lr = 3, 77 * 64, 7e-3
    half = grad_dtype == torch.float16
    g = torch.Generator().manual_seed(1)
    p0 = torch.randn(K, n, generator=g)
    grads = [(torch.randn(K, n, generator=g) * 2.0).to(grad_dtype) for _ in range(5)]
    factors = [[3e-4 * (1 + it), 5e-4, 7e-4 / (1 + it)] for it in range(5)]          # stats[k][1]: per image, per step
    hyper = torch.tensor([lr, 0.9, 0.999, 1e-8], device=DEV)

    def run(active):
        param, m, v = p0.clone().to(DEV), torch.zeros(K, n, device=DEV), torch.zeros(K, n, device=DEV)
        p16 = torch.full((K, n), 3.0, dtype=torch.float16, device=DEV) if half else None
        for k, a in enumerate(active):
            if not a:                               # a gated image's state is arbitrary and must come back untouched
                m[k], v[k] = 0.25, 0.5
        init = [t.clone() for t in (param, m, v)] + ([p16.clone()] if half else [])
        step = torch.zeros(1, dtype=torch.int32, device=DEV)
        act = torch.tensor(active, dtype=torch.int32, device=DEV)
        for it in range(5):
            st = torch.tensor([[0.0, f] for f in factors[it]], device=DEV)
            hip.nti_adam_batched(param, m, v, grads[it].to(DEV), st, act, hyper, step, p16)
        return (param, m, v) + ((p16,) if half else ()), init, step

    got, init, step = run([1, 0, 1])
    assert step.item() == 5
    for t, t0 in zip(got, init):
        assert torch.equal(t[1], t0[1])             # gated: param, m, v (and param16) bit-equal to their initial values
    for k in (0, 2):
        p_ref = p0[k].clone().requires_grad_(True)
        opt = torch.optim.Adam([p_ref], lr=lr)
        for it in range(5):
            p_ref.grad = grads[it][k].float() * factors[it][k]
            opt.step()
        err = (got[0][k].cpu() - p_ref.detach()).abs().max().item()
        print(f"nti_adam_batched [{grad_dtype}] image {k} vs torch.optim.Adam: {err:.2e}")
        assert err < 1e-6
        if half:
            assert torch.equal(got[3][k], got[0][k].half())
    allon, _, step = run([1, 1, 1])
    assert step.item() == 5
    for k in range(K):
        param, m, v = p0[k].clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        p16 = torch.empty(n, dtype=torch.float16, device=DEV) if half else None
        st1 = torch.zeros(1, dtype=torch.int32, device=DEV)
        for it in range(5):
            hip.nti_adam(param, m, v, grads[it][k].to(DEV), torch.tensor([0.0, factors[it][k]], device=DEV), hyper, st1, p16)
        single = (param, m, v) + ((p16,) if half else ())
        for a, b in zip(allon, single):
            assert torch.equal(a[k], b), k


def test_batched_entry_points_refuse_bad_arguments():
    """IEF_EINVAL / IEF_ESHAPE / IEF_EALIGN before any launch, straight at the C ABI"""
    lib = hip.load()
    f = torch.zeros(64, device=DEV)
    h = torch.zeros(64, dtype=torch.float16, device=DEV)
    i = torch.zeros(4, dtype=torch.int32, device=DEV)
    p, ph, pi = f.data_ptr(), h.data_ptr(), i.data_ptr()
    assert lib.ief_nti_loss_grad_batched_f32(p, p, p, p, p, p, None, 8, 2, 1.0, None) == -1
    assert lib.ief_nti_loss_grad_batched_f32(p, p, p, p, p, p, p, 8, 0, 1.0, None) == -2
    assert lib.ief_nti_loss_grad_batched_f32(p, p, p, p, p, p, p, (1 << 20) + 1, 1, 1.0, None) == -2
    assert lib.ief_nti_loss_grad_batched_f32(p, p, p, p, p, p + 2, p, 8, 2, 1.0, None) == -3
    assert lib.ief_nti_adam_batched_f32(p, p, p, ph, p, None, p, pi, ph, 8, 2, None) == -1
    assert lib.ief_nti_adam_batched_f32(p, p, p, ph, p, pi, p, pi, ph, 8, 0, None) == -2
    assert lib.ief_nti_adam_batched_f32(p, p, p, ph + 1, p, pi, p, pi, ph, 8, 2, None) == -3
    assert lib.ief_nti_adam_batched_f32g(p, p, p, None, p, pi, p, pi, 8, 2, None) == -1
    assert lib.ief_nti_adam_batched_f32g(p, p, p, p, p, pi, p, pi, 0, 2, None) == -2
    assert lib.ief_nti_adam_batched_f32g(p, p, p, p, p, pi + 2, p, pi, 8, 2, None) == -3
    torch.cuda.synchronize()
    assert f.abs().max().item() == 0 and i.abs().max().item() == 0


# ------------------------------------------------------------------------------------------------ the loop
@functools.lru_cache(maxsize=None)
def pipe_of(mode):
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", keep_state_dict=True, precision=mode)
    pipe.scheduler.set_timesteps(STEPS)
    return pipe


@functools.lru_cache(maxsize=None)
def sched_ref():
    return p2p_ref.DDIMRef(num_inference_steps=STEPS)


@functools.lru_cache(maxsize=None)
def image(seed, cscale=0.1):
    """(context [2,77,C] = (uncond, cond), the inversion latents x_0 .. x_T of the oracle): computed once, never written"""
    pipe = pipe_of("f16x3")          # the oracle reads the state dict, which the modes share
    cfg = pipe.cfg
    g = torch.Generator().manual_seed(seed)
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * cscale
    x0 = torch.randn(1, 4, cfg.sample_size, cfg.sample_size, generator=g)
    lat = p2p_ref.ddim_inversion_loop(pipe._state_dict, cfg, ctx[1:], x0, sched_ref())
    return ctx, lat


def group(images):
    return dict(lats=[l for _, l in images], uncs=[c[:1] for c, _ in images], cond=[c[1:] for c, _ in images])


def batched(mode, images, K=None, use_graph=True):
    K = K or len(images)
    return BatchedNullTextOptimizer(pipe_of(mode), images[0][0][1:], GS, tuple(images[0][1][-1].shape[-2:]), K, use_graph=use_graph)


def drive(opt, images, epsilon, after_timestep=None):
    """`BatchedNullTextOptimizer.run` spelt out, keeping what the checks need: the state entering every timestep, every
    loss the stop rule looked at with its threshold, and the embeddings after every inner replay"""
    gr = group(images)
    opt.begin(gr["lats"], gr["uncs"], gr["cond"])
    entering, looked, params = [], [], []
    for i in range(OUTER):
        entering.append((opt.lat.clone().cpu(), opt.param.clone().cpu()))
        opt.outer_begin(i)
        params.append([])
        for j in range(INNER):
            opt.inner_step()
            losses = opt.inner_losses()
            on = [k for k in range(opt.n_real) if opt._flags[k]]
            looked += [(k, i, j, losses[k], epsilon + i * 2e-5) for k in on]
            opt.stop([k for k in on if losses[k] < epsilon + i * 2e-5])
            params[-1].append(opt.param.clone())
            if not opt.any_active():
                break
        opt.outer_end()
        if after_timestep is not None:
            after_timestep(i)
    return entering, looked, params


def drive_single(mode, img, epsilon):
    """`NullTextOptimizer.run` on one image, spelt out the same way"""
    ctx, lat = img
    opt = NullTextOptimizer(pipe_of(mode), ctx[1:], GS, tuple(lat[-1].shape[-2:]))
    opt.begin(lat, ctx[:1])
    looked = []
    for i in range(OUTER):
        opt.outer_begin(i)
        for j in range(INNER):
            opt.inner_step()
            loss = opt.inner_loss()
            looked.append((i, j, loss, epsilon + i * 2e-5))
            if loss < epsilon + i * 2e-5:
                break
        opt.outer_end()
    opt.release()
    return [o.cpu() for o in opt.out], list(opt.inner_steps_run), list(opt.last_losses), opt.lat.clone().cpu(), looked


def oracle_timestep(img, i, lat_i, u_i, epsilon):
    """the oracle's loop body at timestep i from the product's own state -> (embedding, movement, mask of the elements
    whose gradient the fp32 pass does not resolve at one of the timestep's Adam steps)"""
    ctx, lat = img
    pipe = pipe_of("f16x3")
    trace = []
    b = p2p_ref.null_optimization(pipe._state_dict, pipe.cfg, lat, torch.cat([u_i, ctx[1:]]), sched_ref(), num_inner_steps=INNER,
                                  epsilon=epsilon, guidance_scale=GS, num_outer=1, start=i, cur0=lat_i, grad_trace=trace)[0]
    unresolved = torch.zeros_like(u_i, dtype=torch.bool)
    for _, _, gr in trace:
        unresolved |= gr[:1].abs() < NOISE * gr.abs().max()
    return b, (b - u_i).abs().max().item(), unresolved


def check_group_vs_oracle(label, images, opt, entering, singles, epsilon, rows=None, other="per-image run"):
    """the protocol of test_nti_loop_fp32_modes_elementwise per image and per timestep, plus the batched row against
    `singles` (the per-image `run`) on the resolvable elements"""
    for k in (range(len(images)) if rows is None else rows):
        for i in range(OUTER):
            lat_i, u_i = entering[i][0][k:k + 1], entering[i][1][k:k + 1]
            b, moved, unresolved = oracle_timestep(images[k], i, lat_i, u_i, epsilon)
            a = opt.out[k][i].cpu()
            diff = (a - b).abs()
            worst, n_un = diff[~unresolved].max().item(), int(unresolved.sum())
            worst_un = diff[unresolved].max().item() if n_un else 0.0
            vs_run = (a - singles[k][i]).abs()[~unresolved].max().item()
            print(f"{label} image {k} timestep {i}: moved {moved:.3e}; resolvable elements within {worst / moved:.2e} of the movement; "
                  f"{n_un} of {diff.numel()} unresolved, worst {worst_un / moved:.2e}; vs {other} {vs_run / moved:.2e}")
            assert worst <= 1e-2 * moved
            assert n_un <= 0.05 * diff.numel() and worst_un <= 2.1 * moved
            assert vs_run <= 1e-2 * moved


@pytest.mark.parametrize("mode", ["f16x3", "f32", "f16"])
def test_k1_is_the_existing_optimiser(mode):
    img = image(0)
    out1, steps1, losses1, lat1, _ = drive_single(mode, img, 1e-5)
    ctx, lat = img
    ref = NullTextOptimizer(pipe_of(mode), ctx[1:], GS, tuple(lat[-1].shape[-2:]))
    out_run = [o.cpu() for o in ref.run(lat, ctx[:1], INNER, 1e-5, num_outer=OUTER)]
    ref.release()
    opt = batched(mode, [img])
    gr = group([img])
    out = opt.run(gr["lats"], gr["uncs"], INNER, 1e-5, num_outer=OUTER, cond=gr["cond"])
    opt.release()
    assert len(out) == 1 and len(out[0]) == OUTER
    for a, b, c in zip(out[0], out_run, out1):
        assert a.shape == b.shape and torch.equal(a.cpu(), b) and torch.equal(b, c)
    assert torch.equal(opt.lat.cpu(), ref.lat.cpu()) and torch.equal(opt.lat.cpu(), lat1)
    assert opt.inner_steps_run == [ref.inner_steps_run] and ref.inner_steps_run == steps1 == [INNER] * OUTER
    assert opt.last_losses == [ref.last_losses] and ref.last_losses == losses1


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_rows_do_not_leak(mode):
    img = image(0)
    opt = batched(mode, [img, img])

    def same_rows(i):
        assert torch.equal(opt.param[0], opt.param[1]), f"embedding rows differ after timestep {i}"
        assert torch.equal(opt.lat[0], opt.lat[1]), f"latent rows differ after timestep {i}"
        assert torch.equal(opt.stats[0], opt.stats[1])

    drive(opt, [img, img], NEVER, after_timestep=same_rows)
    opt.release()
    assert opt.inner_steps_run == [[INNER] * OUTER] * 2


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_real_group_vs_oracle(mode):
    images = [image(0), image(1)]
    singles = [drive_single(mode, img, NEVER)[0] for img in images]
    opt = batched(mode, images)
    entering, _, _ = drive(opt, images, NEVER)
    opt.release()
    assert opt.inner_steps_run == [[INNER] * OUTER] * 2
    check_group_vs_oracle(f"NTI batched K=2 [{mode}]", images, opt, entering, singles, NEVER)


def test_ragged_early_stop():
    """Image A (a weak prompt: the guided step almost reproduces the inversion) meets the stop rule at its first inner step of
    timestep 0 while image B (a strong prompt) runs every step.  Losses measured on the oracle while the inputs were chosen:
    A 0.398 at its first step, B 1.15 / 0.99 / 0.87; the threshold is put at their geometric mean."""
    mode = "f16x3"
    A, B = image(4, 0.03), image(3, 0.5)
    free = [drive_single(mode, img, NEVER)[4] for img in (A, B)]
    a0 = free[0][0][2]
    b_min = min(loss for i, j, loss, _ in free[1] if i == 0)
    epsilon = math.sqrt(a0 * b_min)
    print(f"ragged stop: A's first loss {a0:.4e}, B's smallest of timestep 0 {b_min:.4e}, epsilon {epsilon:.4e}")
    assert a0 < epsilon < b_min
    singles = [drive_single(mode, img, epsilon) for img in (A, B)]
    opt = batched(mode, [A, B])
    entering, looked, params = drive(opt, [A, B], epsilon)
    opt.release()
    for who, i, j, loss, thr in [("A",) + t for t in singles[0][4]] + [("B",) + t for t in singles[1][4]] + \
            [("batched %d" % k, i, j, loss, thr) for k, i, j, loss, thr in looked]:
        assert abs(loss - thr) > 0.05 * thr, f"{who}: loss {loss:.4e} of timestep {i} step {j} within 5 % of its threshold {thr:.4e}"
    print(f"ragged stop: steps per timestep, batched {opt.inner_steps_run}, per image {[s[1] for s in singles]}")
    assert opt.inner_steps_run == [singles[0][1], singles[1][1]]
    assert opt.inner_steps_run[0][0] == 1 and opt.inner_steps_run[1][0] == INNER
    assert opt.last_losses[0][0] == [l for k, i, j, l, _ in looked if k == 0 and i == 0][-1]
    for k in range(2):
        for i in range(OUTER):
            done = opt.inner_steps_run[k][i]
            for later in params[i][done:]:          # replays after image k's stop: its embedding must not move at all
                assert torch.equal(later[k], params[i][done - 1][k]), (k, i)
            assert torch.equal(opt.out[k][i][0], params[i][-1][k])
    assert len(params[0]) == INNER and not torch.equal(params[0][0][1], params[0][-1][1])      # B kept moving meanwhile
    check_group_vs_oracle("NTI ragged stop", [A, B], opt, entering, [s[0] for s in singles], epsilon, rows=[0])


def test_graph_equals_eager_and_reuse_across_groups():
    mode = "f16x3"
    first, second = [image(0), image(1)], [image(2), image(3, 0.5)]
    opt = batched(mode, first)
    eager = batched(mode, first, use_graph=False)
    g1, g2 = group(first), group(second)
    out_g = opt.run(g1["lats"], g1["uncs"], INNER, NEVER, num_outer=OUTER, cond=g1["cond"])
    out_e = eager.run(g1["lats"], g1["uncs"], INNER, NEVER, num_outer=OUTER, cond=g1["cond"])
    eager.release()
    for a, b in zip(sum(out_g, []), sum(out_e, [])):
        assert torch.equal(a, b)                    # graph replay == eager launches, bit for bit
    # a second group through the same optimiser (same graphs, new conditional embeddings) == a fresh optimiser
    graphs = opt._graphs
    out_2 = opt.run(g2["lats"], g2["uncs"], INNER, NEVER, num_outer=OUTER, cond=g2["cond"])
    assert graphs is not None and opt._graphs is graphs
    lat_2 = opt.lat.clone()
    opt.release()
    fresh = batched(mode, second)
    out_f = fresh.run(g2["lats"], g2["uncs"], INNER, NEVER, num_outer=OUTER, cond=g2["cond"])
    fresh.release()
    for a, b in zip(sum(out_2, []), sum(out_f, [])):
        assert torch.equal(a, b)
    assert torch.equal(lat_2, fresh.lat)
    assert not torch.equal(out_g[0][0], out_2[0][0])


def test_padded_group():
    """3 images through a K = 4 optimiser (one padded row) against the same 3 at K = 3: other split-K shapes, so the oracle's
    bound on resolvable elements and not bit equality"""
    mode = "f16x3"
    three = [image(0), image(1), image(2)]
    k3 = batched(mode, three)
    entering, _, _ = drive(k3, three, NEVER)
    k3.release()
    k4 = batched(mode, three, K=4)
    g3 = group(three)
    out_4 = k4.run(g3["lats"], g3["uncs"], INNER, NEVER, num_outer=OUTER, cond=g3["cond"])
    k4.release()
    assert len(out_4) == 3 and k4.inner_steps_run == [[INNER] * OUTER] * 3 and k4._flags == [1, 1, 1, 0]
    check_group_vs_oracle("NTI K=3", three, k3, entering, [[o.cpu() for o in img] for img in out_4], NEVER,
                          other="the 3 images padded to K=4")


def test_public_surface_keeps_one_optimiser_across_calls():
    """`NTI.null_optimization_batched` the way the PIE driver uses it: two calls with batch = 2 on one invertor, plain UNet
    forwards (the edits' place) in between; the second call brings new contexts and a padded last group (3 images) and must
    run on the optimiser and graphs the first call left.  Outputs against `null_optimization_many` to the bound of
    `test_real_group_vs_oracle` (unresolved elements from the oracle's own run of the image), step counts equal."""
    from ief_amd.p2p.inversion.nti import NTI
    steps = 2
    pipe = StableDiffusionPipeline.from_pretrained("synthetic:tiny", keep_state_dict=True, precision="f16x3")
    pipe.scheduler.set_timesteps(steps)
    sched, cfg = p2p_ref.DDIMRef(num_inference_steps=steps), pipe.cfg
    ctxs, lats, masks = [], [], []
    for seed in range(3):
        g = torch.Generator().manual_seed(seed)
        ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g) * 0.1
        lat = p2p_ref.ddim_inversion_loop(pipe._state_dict, cfg, ctx[1:], torch.randn(1, 4, cfg.sample_size, cfg.sample_size, generator=g), sched)
        trace = []
        p2p_ref.null_optimization(pipe._state_dict, cfg, lat, ctx, sched, num_inner_steps=INNER, epsilon=1e-5, guidance_scale=GS,
                                  grad_trace=trace)
        per_step = [torch.zeros(1, 77, cfg.cross_attention_dim, dtype=torch.bool) for _ in range(steps)]
        for i, _, gr in trace:
            per_step[i] |= gr[:1].abs() < NOISE * gr.abs().max()
        ctxs.append(ctx.to(DEV)), lats.append([l.to(DEV) for l in lat]), masks.append(per_step)

    x = torch.randn(2, 4, cfg.sample_size, cfg.sample_size, generator=torch.Generator().manual_seed(9)).to(DEV)
    forward = lambda: pipe.unet(x, 601, encoder_hidden_states=torch.cat([ctxs[0][1:], ctxs[1][1:]]))["sample"].clone()
    eps_before = forward()

    def check(order, outs, steps_run):
        ref_nti = NTI()
        many = ref_nti.null_optimization_many(pipe, [lats[k] for k in order], [ctxs[k] for k in order], INNER, 1e-5, GS)
        assert steps_run == ref_nti.inner_steps_run and len(outs) == len(order)
        for k, a, b in zip(order, outs, many):
            assert len(a) == len(b) == steps
            for i in range(steps):
                start = ctxs[k][:1] if i == 0 else b[i - 1]
                moved = (b[i] - start).abs().max().item()
                un = masks[k][i].to(DEV)
                diff = (a[i] - b[i]).abs()
                print(f"null_optimization_batched image {k} timestep {i}: vs null_optimization_many {diff[~un].max().item() / moved:.2e} "
                      f"of the movement on resolvable elements, {int(un.sum())} unresolved: {diff[un].max().item() / moved:.2e}")
                assert diff[~un].max().item() <= 1e-2 * moved
                assert int(un.sum()) <= 0.05 * un.numel() and diff[un].max().item() <= 2.1 * moved

    nti = NTI()
    try:
        out1 = nti.null_optimization_batched(pipe, lats[:2], ctxs[:2], INNER, 1e-5, GS, batch=2)
        kept, graphs = nti._batched, nti._batched._graphs
        assert graphs is not None and all(m.cache_kv for m in pipe.unet.attention_modules())
        check([0, 1], out1, nti.inner_steps_run)
        assert torch.equal(forward(), eps_before) and torch.equal(forward(), eps_before)     # the UNet between two calls is as it was
        order = [1, 2, 0]                                                                   # groups [1, 2] and [0, padded]
        out2 = nti.null_optimization_batched(pipe, [lats[k] for k in order], [ctxs[k] for k in order], INNER, 1e-5, GS, batch=2)
        assert nti._batched is kept and kept._graphs is graphs and kept.n_real == 1
        check(order, out2, nti.inner_steps_run)
        assert torch.equal(forward(), eps_before)
    finally:
        nti.release_batched()
    assert nti._batched is None and all(m.cache_kv for m in pipe.unet.attention_modules())
