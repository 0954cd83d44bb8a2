// Proximal guidance on a negative-prompt-inversion edit (Miyake, Iohara, Saito, Tanaka, "Negative-prompt Inversion"; Han, Yi, Zhang,
// Hu, Deng, Metaxas et al., "Improving Tuning-Free Real Image Editing with Proximal Guidance"): the per-step rule, two launches.
//   prox_threshold      lambda_b = the q-quantile of |eps_c - eps_u| over the elements of batch row b
//   cfg_ddim_prox       the guidance difference thresholded at lambda_b (l0 / l1), the CFG + DDIM update of ddim_step.h, and on the
//                       target rows the pull of the x0 prediction towards the encoded source where the dilated edit mask is off
// The threshold runs ONE workgroup of 1024 threads per row: a row is 1 .. 65536 values, more than the 64 KiB an LDS staging holds,
// so every lane keeps its 4 / 16 / 64 values in registers (one coalesced read of the row) and the radix select of ledits.hip walks
// them four times, a byte at a time.  The values are non-negative, so their bit patterns order as unsigned integers and both order
// statistics are EXACT.  The histogram is 256 bins x 16 copies in LDS (16 KiB), lane l adds to copy l % 16: the top byte of Gaussian
// differences falls into three or four bins, and 64 lanes adding to one word would serialise.  The copies are summed as integers, so
// the result does not depend on the order of the atomics: the same bits from run to run.  No atomics on global memory, no buffer to
// zero, one writer per output.  Plain fp32 on the vector ALU; built without fma contraction (the generic rule of the Makefile).
#include "ief_common.h"
#include "ief_params.h"
#include "ddim_step.h"

#define PROX_MAX_ROW 65536
#define PROX_SUB 16
#define PROX_NONE 0xffffffffu        // not a value: |d| has a clear sign bit

template <int VPT>
__global__ __launch_bounds__(1024) void prox_threshold_kernel(const float* __restrict__ eu, const float* __restrict__ ec,
                                                              const float* __restrict__ rank, float* __restrict__ thres, int n) {
    __shared__ unsigned hist[256 * PROX_SUB];
    __shared__ unsigned wtot[4];
    __shared__ unsigned s_prefix, s_k, s_cnt, s_above;
    const int tid = threadIdx.x, lane = tid & 63, sub = tid & (PROX_SUB - 1);
    const long long row = (long long)blockIdx.x * n;
    unsigned v[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const int p = j * 1024 + tid;
        v[j] = p < n ? __float_as_uint(fabsf(ec[row + p] - eu[row + p])) : PROX_NONE;
    }
    int lo = (int)rank[0];
    lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
    const float frac = rank[1];
    unsigned prefix = 0, k = (unsigned)lo, cnt = (unsigned)n;
    if (tid == 0) s_above = PROX_NONE;
    // Four passes, most significant byte first.  A pass counts, among the values that agree with the bytes chosen so far, the next
    // byte; threads 0 .. 255 sum their bin's copies and scan the 256 counts (a shuffle scan inside each of their four waves, then the
    // wave totals); the one whose bin holds rank k keeps its byte, the rank inside the bin and the bin's count.
    for (int shift = 24; shift >= 0; shift -= 8) {
#pragma unroll
        for (int j = 0; j < 256 * PROX_SUB / 1024; ++j) hist[j * 1024 + tid] = 0;
        __syncthreads();
        const unsigned himask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const unsigned b = v[j];
            if (b != PROX_NONE && (b & himask) == prefix) atomicAdd(&hist[((b >> shift) & 255u) * PROX_SUB + sub], 1u);
        }
        __syncthreads();
        unsigned c = 0, inc = 0;
        if (tid < 256) {
#pragma unroll
            for (int j = 0; j < PROX_SUB; ++j) c += hist[tid * PROX_SUB + ((j + tid) & (PROX_SUB - 1))];
            inc = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned o = __shfl_up(inc, off);
                if (lane >= off) inc += o;
            }
            if (lane == 63) wtot[tid >> 6] = inc;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < (tid >> 6); ++w) inc += wtot[w];
            const unsigned exc = inc - c;
            if (c != 0 && exc <= k && k < inc) {         // exactly one bin: k < the number of values still in play
                s_prefix = prefix | ((unsigned)tid << shift);
                s_k = k - exc;
                s_cnt = c;
            }
        }
        __syncthreads();
        prefix = s_prefix;
        k = s_k;
        cnt = s_cnt;
    }
    // The chosen bytes ARE v_(lo); cnt values equal it and k is its rank among them, so lo - k + cnt values are <= v_(lo).  If that
    // covers rank hi, v_(hi) is v_(lo); otherwise it is the smallest value above v_(lo): an integer minimum, order-free.
    const int hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    unsigned hib = prefix;
    if ((unsigned)hi >= (unsigned)lo - k + cnt) {        // uniform: every operand came out of LDS after a barrier
        unsigned m = PROX_NONE;
#pragma unroll
        for (int j = 0; j < VPT; ++j)
            if (v[j] > prefix && v[j] < m) m = v[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned o = __shfl_xor(m, off);
            m = o < m ? o : m;
        }
        if (lane == 0) atomicMin(&s_above, m);
        __syncthreads();
        hib = s_above;
    }
    if (tid == 0) {
        const float vlo = __uint_as_float(prefix), vhi = __uint_as_float(hib);
        thres[blockIdx.x] = vlo + frac * (vhi - vlo);
    }
}

extern "C" int ief_prox_threshold_f32(const float* eps_u, const float* eps_c, const float* rank, float* thres_out, int B,
                                      long long row_elems, void* stream) {
    if (!eps_u || !eps_c || !rank || !thres_out) return IEF_EINVAL;
    if (B < 1 || row_elems < 1 || row_elems > PROX_MAX_ROW) return IEF_ESHAPE;
    if (((uintptr_t)eps_u | (uintptr_t)eps_c | (uintptr_t)rank | (uintptr_t)thres_out) & 3) return IEF_EALIGN;
    const int n = (int)row_elems;
    if (n <= 4 * 1024)
        hipLaunchKernelGGL(prox_threshold_kernel<4>, dim3(B), dim3(1024), 0, (hipStream_t)stream, eps_u, eps_c, rank, thres_out, n);
    else if (n <= 16 * 1024)
        hipLaunchKernelGGL(prox_threshold_kernel<16>, dim3(B), dim3(1024), 0, (hipStream_t)stream, eps_u, eps_c, rank, thres_out, n);
    else
        hipLaunchKernelGGL(prox_threshold_kernel<64>, dim3(B), dim3(1024), 0, (hipStream_t)stream, eps_u, eps_c, rank, thres_out, n);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// The step.  Element i = b row_elems + c hw + p.  Row 0 (the source branch) is the plain step of ief_cfg_ddim_step_f32, operation
// for operation, whatever the coefficients say; so is every row when coef[3] (prox_on) and coef[4] (eta) are 0.  On rows b >= 1:
//   d = eps_c - eps_u;   prox_on:  l0  d' = |d| > lambda_b ? d : 0;   l1  d' = d > lambda_b ? d - lambda_b : (d < -lambda_b ? d + lambda_b : 0)
//   eps = eps_u + g d';  x0 = ddim_x0(x, eps)
//   eta != 0:  m = prox_on ? any |d| > lambda_b within Chebyshev distance `radius` of p, same row and channel, outside = 0 : 1
//              x0 = m ? x0 : x0 - eta (x0 - z0[c hw + p])
//   x' = ddim_next(x0, eps)
// The stencil reads eps_u and eps_c only (at most 49 x 2 loads of a row that sits in L2), so x_out may be x.
__global__ __launch_bounds__(256) void cfg_ddim_prox_kernel(const float* __restrict__ eu, const float* __restrict__ ec,
                                                            const float* x, float* xo, float* __restrict__ x0o,
                                                            const float* __restrict__ coef, const float* __restrict__ thres,
                                                            const float* __restrict__ z0, long long n, int row_elems, int h, int w,
                                                            int mode, int radius) {
    const DdimCoef c = ddim_coef(coef);
    const bool prox_on = coef[3] != 0.0f;
    const float eta = coef[4];
    const int hw = h * w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / row_elems);
        const int e = (int)(i - (long long)b * row_elems);
        const float u = eu[i];
        const float d = ec[i] - u;
        float dd = d, lam = 0.0f;
        if (b >= 1 && prox_on) {
            lam = thres[b];
            if (mode == 0) dd = fabsf(d) > lam ? d : 0.0f;
            else dd = d > lam ? d - lam : (d < -lam ? d + lam : 0.0f);
        }
        const float eps = u + c.g * dd;
        float x0 = ddim_x0(c, x[i], eps);
        if (b >= 1 && eta != 0.0f) {
            bool m = true;
            if (prox_on) {
                const int p = e % hw, py = p / w, px = p - py * w;
                const long long plane = i - p;            // first element of this row's channel
                m = false;
                for (int dy = -radius; dy <= radius; ++dy) {
                    const int yy = py + dy;
                    if (yy < 0 || yy >= h) continue;
                    for (int dx = -radius; dx <= radius; ++dx) {
                        const int xx = px + dx;
                        if (xx < 0 || xx >= w) continue;
                        const long long q = plane + (long long)yy * w + xx;
                        m = m || fabsf(ec[q] - eu[q]) > lam;
                    }
                }
            }
            if (!m) x0 = x0 - eta * (x0 - z0[e]);
        }
        if (x0o) x0o[i] = x0;
        xo[i] = ddim_next(c, x0, eps);
    }
}

extern "C" int ief_cfg_ddim_step_prox_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out, float* x0_out,
                                          const float* coef, const float* thres, const float* z0, long long n, long long row_elems,
                                          int h, int w, int mode, int radius, void* stream) {
    if (!eps_u || !eps_c || !x || !x_out || !coef || !thres || !z0) return IEF_EINVAL;
    if (n <= 0 || row_elems <= 0 || row_elems > PROX_MAX_ROW || n % row_elems != 0 || h < 1 || w < 1 ||
        (long long)h * w > row_elems || row_elems % ((long long)h * w) != 0 || (mode != 0 && mode != 1) || radius < 0 || radius > 3)
        return IEF_ESHAPE;
    if (((uintptr_t)eps_u | (uintptr_t)eps_c | (uintptr_t)x | (uintptr_t)x_out | (uintptr_t)x0_out | (uintptr_t)coef |
         (uintptr_t)thres | (uintptr_t)z0) & 3)
        return IEF_EALIGN;
    int grid = (int)((n + 255) / 256);
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(cfg_ddim_prox_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, eps_u, eps_c, x, x_out, x0_out, coef, thres,
                       z0, n, (int)row_elems, h, w, mode, radius);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
