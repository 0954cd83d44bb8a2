// LEDITS++ (Brack, Friedrich, Kornmeier, Tsaban, Schramowski, Kersting, Passos, "LEDITS++: Limitless Image Editing using
// Text-to-Image Models", CVPR 2024): the per-step rule of the masked multi-concept guidance, on the edit-friendly DDPM noise space.
//   ledits_attn_mask       3 x 3 smoothing of a concept's 16 x 16 cross-attention mass, then a quantile threshold      -> M1
//   ledits_guidance_mask   s[p] = sum_c |eps_e - eps_u| M1, a quantile threshold over the pixels, AND M1                -> M
//   ledits_ddpm_step       eps' = eps_u + sum_e scale_e M_e (eps_e - eps_u), then the eta = 1 update of ddpm_step.h
//   ledits_dpmpp_step      the same guidance, then the second-order SDE-DPM-Solver++ update of ddpm_step.h (the paper's solver)
// The two mask kernels run ONE workgroup per concept: they are latency, not throughput (256 and at most 16384 values).  Their
// quantile is torch.quantile's linear rule with the arithmetic pinned, and its two order statistics are EXACT: the values are
// non-negative, so their bit patterns order as unsigned integers, and a radix select walks those bits a byte at a time over a
// 256-bin histogram in LDS.  The histogram's LDS atomics add integers, so their order changes nothing.  Plain fp32 on the vector ALU,
// one writer per output element, no atomics on global memory; built without fma contraction (the generic rule of the Makefile).
#include "ief_common.h"
#include "ief_params.h"
#include "ddpm_step.h"

#define LEDITS_MAX_E 8
#define LEDITS_MAX_C 16
#define LEDITS_MAX_HW 16384

// LDS scratch of one select: the byte histogram and a few words every thread reads back after a barrier
struct LeditsSelect {
    unsigned hist[256];
    unsigned wtot[4];
    unsigned prefix, k, cnt, above;
};

// t = v_(lo) + frac (v_(hi) - v_(lo)), hi = min(lo + 1, n - 1), over the n non-negative floats vals[] (LDS).  Called by every thread
// of a workgroup of 256 .. 1024 threads (a multiple of 64) after a barrier that made vals[] visible; every thread gets the same t.
// Four passes, most significant byte first.  A pass counts, among the values that agree with the bytes chosen so far, the next byte;
// threads 0 .. 255 scan the 256 counts (a shuffle scan inside each of their four waves, then the wave totals) and the one whose bin
// holds rank k keeps its byte, the rank inside the bin and the bin's count.  After the last pass the chosen bytes ARE v_(lo), cnt is
// the number of values equal to it and k its rank among them, so lo - k + cnt values are <= v_(lo).  If that covers rank hi, v_(hi)
// is v_(lo); otherwise it is the smallest value above v_(lo): an integer minimum, order-free.
__device__ __forceinline__ float ledits_quantile(const float* vals, int n, int lo, float frac, LeditsSelect& s) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    unsigned prefix = 0, k = (unsigned)lo, cnt = (unsigned)n;
    if (tid == 0) s.above = 0xffffffffu;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s.hist[tid] = 0;
        __syncthreads();
        const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        for (int p = tid; p < n; p += nt) {
            const unsigned b = __float_as_uint(vals[p]);
            if ((b & himask) == prefix) atomicAdd(&s.hist[(b >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned c = 0, inc = 0;
        if (tid < 256) {
            c = s.hist[tid];
            inc = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_up(inc, off);
                if (lane >= off) inc += o;
            }
            if (lane == 63) s.wtot[tid >> 6] = inc;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < (tid >> 6); ++w) inc += s.wtot[w];
            const unsigned exc = inc - c;
            if (c != 0 && exc <= k && k < inc) {         // exactly one bin: k < the number of values still in play
                s.prefix = prefix | ((unsigned)tid << shift);
                s.k = k - exc;
                s.cnt = c;
            }
        }
        __syncthreads();
        prefix = s.prefix;
        k = s.k;
        cnt = s.cnt;
    }
    const int hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    unsigned hib = prefix;
    if ((unsigned)hi >= (unsigned)lo - k + cnt) {        // uniform: every operand came out of LDS after a barrier
        for (int p = tid; p < n; p += nt) {
            const unsigned b = __float_as_uint(vals[p]);
            if (b > prefix) atomicMin(&s.above, b);
        }
        __syncthreads();
        hib = s.above;
    }
    const float vlo = __uint_as_float(prefix), vhi = __uint_as_float(hib);
    return vlo + frac * (vhi - vlo);
}

// One workgroup of 256 threads per concept, thread t = cell (t / 16, t % 16).  The nine taps are added in row-major tap order,
// (..((0 + w_00 a) + w_01 a) ..) + w_22 a, each product and each sum rounded; REFLECT padding (index -1 reads 1, index 16 reads 14).
__global__ __launch_bounds__(256) void ledits_attn_mask_kernel(const float* __restrict__ acc, const float* __restrict__ taps,
                                                              const float* __restrict__ rank, float* __restrict__ m1) {
    __shared__ float img[256];
    __shared__ float sm[256];
    __shared__ LeditsSelect sel;
    const int e = blockIdx.x, tid = threadIdx.x;
    img[tid] = acc[e * 256 + tid];
    __syncthreads();
    const int py = tid >> 4, px = tid & 15;
    float v = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            int yy = py + dy, xx = px + dx;
            yy = yy < 0 ? 1 : (yy > 15 ? 14 : yy);
            xx = xx < 0 ? 1 : (xx > 15 ? 14 : xx);
            v = v + taps[(dy + 1) * 3 + dx + 1] * img[yy * 16 + xx];
        }
    sm[tid] = v;
    __syncthreads();
    const float t = ledits_quantile(sm, 256, (int)rank[2 * e], rank[2 * e + 1], sel);
    m1[e * 256 + tid] = v >= t ? 1.0f : 0.0f;
}

extern "C" int ief_ledits_attn_mask_f32(const float* acc, const float* taps, const float* rank, float* m1_out, int E, void* stream) {
    if (!acc || !taps || !rank || !m1_out) return IEF_EINVAL;
    if (E < 1 || E > LEDITS_MAX_E) return IEF_ESHAPE;
    if (((uintptr_t)acc | (uintptr_t)taps | (uintptr_t)rank | (uintptr_t)m1_out) & 3) return IEF_EALIGN;
    hipLaunchKernelGGL(ledits_attn_mask_kernel, dim3(E), dim3(256), 0, (hipStream_t)stream, acc, taps, rank, m1_out);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// One workgroup of 1024 threads (16 waves) per concept.  s[] of the whole image stays in LDS (at most 16384 floats = 64 KiB; with the
// 1 KiB cell mask and the select's scratch 66.0 KiB of the CU's 160 KiB, so two concepts can share a CU), is read by the four
// histogram passes from there, and once more for the bits.  Thread t takes pixels t, t + 1024, ...: coalesced over p in every channel.
__global__ __launch_bounds__(1024) void ledits_guidance_mask_kernel(const float* __restrict__ eps, const float* __restrict__ m1,
                                                                   const float* __restrict__ rank, float* __restrict__ mask,
                                                                   float* __restrict__ thres, int C, int H, int W) {
    __shared__ float s[LEDITS_MAX_HW];
    __shared__ float cell[256];
    __shared__ LeditsSelect sel;
    const int e = blockIdx.x, tid = threadIdx.x, hw = H * W;
    const int cy = H >> 4, cx = W >> 4;                  // used with m1 only, where H and W are multiples of 16
    if (m1 && tid < 256) cell[tid] = m1[e * 256 + tid];
    __syncthreads();
    float* __restrict__ mo = mask + (long long)e * hw;
    if (!rank) {                                         // no threshold: the cell mask spread to the pixels
        for (int p = tid; p < hw; p += 1024) {
            const int y = p / W, x = p - y * W;
            mo[p] = m1 ? cell[(y / cy) * 16 + x / cx] : 1.0f;
        }
        return;
    }
    const float* __restrict__ eu = eps;
    const float* __restrict__ ec = eps + (long long)(1 + e) * C * hw;
    for (int p = tid; p < hw; p += 1024) {
        const int y = p / W, x = p - y * W;
        const float m = m1 ? cell[(y / cy) * 16 + x / cx] : 1.0f;
        float a = 0.0f;                                  // 0 + |d_0| m is |d_0| m exactly
        for (int c = 0; c < C; ++c) {
            const long long i = (long long)c * hw + p;
            a = a + fabsf(ec[i] - eu[i]) * m;
        }
        s[p] = a;
    }
    __syncthreads();
    const float t = ledits_quantile(s, hw, (int)rank[2 * e], rank[2 * e + 1], sel);
    if (tid == 0) thres[e] = t;
    for (int p = tid; p < hw; p += 1024) {
        const int y = p / W, x = p - y * W;
        const float m = m1 ? cell[(y / cy) * 16 + x / cx] : 1.0f;
        mo[p] = (s[p] >= t && m != 0.0f) ? 1.0f : 0.0f;
    }
}

extern "C" int ief_ledits_guidance_mask_f32(const float* eps, const float* m1, const float* rank, float* mask_out, float* thres_out,
                                            int E, int C, int H, int W, void* stream) {
    if (!mask_out || (rank && (!eps || !thres_out))) return IEF_EINVAL;
    if (E < 1 || E > LEDITS_MAX_E || C < 1 || C > LEDITS_MAX_C || H < 1 || W < 1 || H > LEDITS_MAX_HW || W > LEDITS_MAX_HW ||
        (long long)H * W > LEDITS_MAX_HW || (m1 && ((H & 15) || (W & 15))))
        return IEF_ESHAPE;
    if (((uintptr_t)eps | (uintptr_t)m1 | (uintptr_t)rank | (uintptr_t)mask_out | (uintptr_t)thres_out) & 3) return IEF_EALIGN;
    hipLaunchKernelGGL(ledits_guidance_mask_kernel, dim3(E), dim3(1024), 0, (hipStream_t)stream, eps, m1, rank, mask_out, thres_out, C,
                       H, W);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// The step of ONE latent row [C][hw] under E concepts.  g = (..((0 + w_0) + w_1)..) + w_{E-1},  w_e = (scale[e] mask[e][p]) d_e with
// d_e = eps[1 + e] - eps[0]; a concept whose scale is 0 is skipped, so its estimate is not read into the result (0 * inf would be
// NaN).  eps' = eps[0] + g goes through ddpm_mu_of: the mean ief_cfg_ddpm_step_f32 takes, operation for operation -- with E = 1,
// no mask and scale = {g} the two launches agree bit for bit.  A grid-stride loop as there; hw fits 32 bits.
__global__ __launch_bounds__(256) void ledits_ddpm_kernel(const float* __restrict__ eps, const float* __restrict__ mask,
                                                          const float* __restrict__ scale, const float* __restrict__ x,
                                                          float* __restrict__ xo, float* __restrict__ x0o,
                                                          const float* __restrict__ coef, long long row_elems, unsigned hw,
                                                          const float* __restrict__ noise, int noise_rows,
                                                          const int* __restrict__ step, int E) {
    const DdpmCoef c = ddpm_coef(coef);
    const float* __restrict__ z = ddpm_noise_row(noise, noise_rows, step, row_elems);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < row_elems; i += (long long)gridDim.x * 256) {
        const unsigned p = (unsigned)i % hw;             // row_elems <= 16 * 16384
        const float u = eps[i];
        float g = 0.0f;
        for (int e = 0; e < E; ++e) {
            const float sc = scale[e];
            if (sc == 0.0f) continue;
            const float m = mask ? mask[(long long)e * hw + p] : 1.0f;
            g = g + (sc * m) * (eps[(long long)(1 + e) * row_elems + i] - u);
        }
        const float mu = ddpm_mu_of(c, u + g, x[i], x0o, i);
        xo[i] = ddpm_add_noise(c, mu, z, i);
    }
}

extern "C" int ief_ledits_ddpm_step_f32(const float* eps, const float* mask, const float* scale, const float* x, float* x_out,
                                        float* x0_out, const float* coef, long long row_elems, long long hw, const float* noise,
                                        int noise_rows, const int* step, int E, void* stream) {
    if (!eps || !scale || !x || !x_out || !coef || !noise || !step) return IEF_EINVAL;
    if (E < 1 || E > LEDITS_MAX_E || hw < 1 || hw > LEDITS_MAX_HW || row_elems < hw || row_elems % hw != 0 ||
        row_elems / hw > LEDITS_MAX_C || noise_rows <= 0)
        return IEF_ESHAPE;
    if (((uintptr_t)eps | (uintptr_t)mask | (uintptr_t)scale | (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)x0_out | (uintptr_t)coef |
         (uintptr_t)noise | (uintptr_t)step) & 3)
        return IEF_EALIGN;
    const int grid = (int)((row_elems + 255) / 256);     // at most 1024 workgroups
    hipLaunchKernelGGL(ledits_ddpm_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, eps, mask, scale, x, x_out, x0_out, coef,
                       row_elems, (unsigned)hw, noise, noise_rows, step, E);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// The same step at solver order 2 (dpmpp_mu_of, ddpm_step.h): coef = {a_from, a_to, sigma, dir, c2}, and x0_prev [row_elems] carries
// the x0 prediction from one step to the next -- read (only where c2 != 0) and written by the lane that owns the element.  The
// guidance is formed exactly as in ledits_ddpm_kernel; with c2 == 0 the outputs are that kernel's bit for bit.
__global__ __launch_bounds__(256) void ledits_dpmpp_kernel(const float* __restrict__ eps, const float* __restrict__ mask,
                                                           const float* __restrict__ scale, const float* __restrict__ x,
                                                           float* __restrict__ xo, float* __restrict__ x0o,
                                                           float* __restrict__ x0_prev, const float* __restrict__ coef,
                                                           long long row_elems, unsigned hw, const float* __restrict__ noise,
                                                           int noise_rows, const int* __restrict__ step, int E) {
    const DdpmCoef c = ddpm_coef(coef);
    const float c2 = coef[4];
    const float* __restrict__ z = ddpm_noise_row(noise, noise_rows, step, row_elems);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < row_elems; i += (long long)gridDim.x * 256) {
        const unsigned p = (unsigned)i % hw;             // row_elems <= 16 * 16384
        const float u = eps[i];
        float g = 0.0f;
        for (int e = 0; e < E; ++e) {
            const float sc = scale[e];
            if (sc == 0.0f) continue;
            const float m = mask ? mask[(long long)e * hw + p] : 1.0f;
            g = g + (sc * m) * (eps[(long long)(1 + e) * row_elems + i] - u);
        }
        const float x0p = c2 == 0.0f ? 0.0f : x0_prev[i];
        float x0;
        const float mu = dpmpp_mu_of(c, c2, u + g, x[i], x0p, &x0);
        if (x0o) x0o[i] = x0;
        x0_prev[i] = x0;
        xo[i] = ddpm_add_noise(c, mu, z, i);
    }
}

extern "C" int ief_ledits_dpmpp_step_f32(const float* eps, const float* mask, const float* scale, const float* x, float* x_out,
                                         float* x0_out, float* x0_prev, const float* coef, long long row_elems, long long hw,
                                         const float* noise, int noise_rows, const int* step, int E, void* stream) {
    if (!eps || !scale || !x || !x_out || !x0_prev || !coef || !noise || !step) return IEF_EINVAL;
    if (E < 1 || E > LEDITS_MAX_E || hw < 1 || hw > LEDITS_MAX_HW || row_elems < hw || row_elems % hw != 0 ||
        row_elems / hw > LEDITS_MAX_C || noise_rows <= 0)
        return IEF_ESHAPE;
    if (((uintptr_t)eps | (uintptr_t)mask | (uintptr_t)scale | (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)x0_out |
         (uintptr_t)x0_prev | (uintptr_t)coef | (uintptr_t)noise | (uintptr_t)step) & 3)
        return IEF_EALIGN;
    const int grid = (int)((row_elems + 255) / 256);     // at most 1024 workgroups
    hipLaunchKernelGGL(ledits_dpmpp_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, eps, mask, scale, x, x_out, x0_out, x0_prev,
                       coef, row_elems, (unsigned)hw, noise, noise_rows, step, E);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
