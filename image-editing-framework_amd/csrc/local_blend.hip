// Prompt-to-Prompt's word-masked latent blending (`LocalBlend`, p2p/model/ptp_utils.py) on the device: the fused 'p2p' plan
// (control.py) never materialises a cross-attention map, and the blend needs, per prompt row and 16 x 16 pixel, only the EDITED
// map summed over the blend words.  The edit is linear in the two plain softmax rows it mixes, so that sum is
//     sum_l v_i[l] P_i[q][l] + sum_l u_i[l] P_src[q][l]
// with per-step weight vectors (u_i, v_i) the host folds from the edit tables and the blend words (p2p/model/register.py).  The
// first kernel adds that quantity, head-mean, into an accumulator that runs over the five 16 x 16 modules and all steps so far;
// the second turns the accumulator into the masks and blends the latents.  Both are tiny and latency-bound: plain fp32 on the
// vector ALU, a fixed summation order, one writer per element.
#include "ief_common.h"
#include "ief_params.h"

#define BLEND_MAX_HEADS 64
#define BLEND_MAX_ROWS 8

// scores of keys lane and lane + 64 of one head (L <= 128): a sequential fma chain over d, q read as wave-uniform 16-byte
// pieces, k as per-lane ones; then max, exp and the row sum.  Lanes past L hold exp(-inf) = 0.
__device__ __forceinline__ void blend_softmax_row(const float* __restrict__ qh, const float* __restrict__ k0, const float* __restrict__ k1,
                                                  int d, bool in0, bool in1, float scale, float& e0, float& e1, float& den) {
    float s0 = 0.f, s1 = 0.f;
    for (int j = 0; j < d; j += 4) {
        const f32x4 qv = *(const f32x4*)(qh + j);
        const f32x4 a = *(const f32x4*)(k0 + j);
        const f32x4 b = *(const f32x4*)(k1 + j);
#pragma unroll
        for (int i = 0; i < 4; ++i) { s0 = __builtin_fmaf(qv[i], a[i], s0); s1 = __builtin_fmaf(qv[i], b[i], s1); }
    }
    s0 = in0 ? s0 * scale : -INFINITY;
    s1 = in1 ? s1 * scale : -INFINITY;
    const float m = wave_max(fmaxf(s0, s1));
    e0 = expf(s0 - m);
    e1 = expf(s1 - m);
    den = wave_sum(e0 + e1);
}

// One workgroup per query n, one wave per head (up to 8 waves; wave w takes heads w, w + 8, ...).  Per head the source row's
// softmax is computed once and kept in registers; then the wave walks the prompt rows: row i's own softmax (row 0's is the source's),
// the two weighted sums, their quotients by the row sums, added as  own + source  and left in LDS.  Thread i then adds row i's
// heads in head order and accumulates into acc[i][n]: the only writer of that element.
__global__ __launch_bounds__(512) void cross_blend_mass_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ w, float* __restrict__ acc, int row0,
                                                                  int Bp, int heads, int N, int L, int ldw, int d, int ldq, int ldk,
                                                                  long long sQb, long long sKb, float scale) {
    __shared__ float part[BLEND_MAX_ROWS][BLEND_MAX_HEADS];
    const int n = blockIdx.x;                    // grid.x == N
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int l0 = lane, l1 = lane + 64;
    const bool in0 = l0 < L, in1 = l1 < L;
    const long long ko0 = (long long)(in0 ? l0 : 0) * ldk, ko1 = (long long)(in1 ? l1 : 0) * ldk;
    for (int h = wid; h < heads; h += nw) {
        const float* qs = q + (long long)row0 * sQb + (long long)n * ldq + h * d;
        const float* ks = k + (long long)row0 * sKb + h * d;
        float es0, es1, dens;
        blend_softmax_row(qs, ks + ko0, ks + ko1, d, in0, in1, scale, es0, es1, dens);
        for (int i = 0; i < Bp; ++i) {
            const float* wu = w + (long long)(i * 2) * ldw;
            const float* wv = wu + ldw;
            const float u0 = in0 ? wu[l0] : 0.f, u1 = in1 ? wu[l1] : 0.f;
            const float v0 = in0 ? wv[l0] : 0.f, v1 = in1 ? wv[l1] : 0.f;
            float e0 = es0, e1 = es1, den = dens;
            if (i > 0) {
                const float* qi = q + (long long)(row0 + i) * sQb + (long long)n * ldq + h * d;
                const float* ki = k + (long long)(row0 + i) * sKb + h * d;
                blend_softmax_row(qi, ki + ko0, ki + ko1, d, in0, in1, scale, e0, e1, den);
            }
            const float own = wave_sum(v0 * e0 + v1 * e1);
            const float src = wave_sum(u0 * es0 + u1 * es1);
            if (lane == 0) part[i][h] = own / den + src / dens;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < Bp) {
        const int i = threadIdx.x;
        float s = 0.f;
        for (int h = 0; h < heads; ++h) s += part[i][h];
        acc[(long long)i * N + n] += s / (float)heads;
    }
}

extern "C" int ief_cross_blend_mass_f32(const float* q, const float* k, const float* w, float* acc, int row0, int Bp, int heads, int N,
                                        int L, int ldw, int d, int ldq, int ldk, long long sQb, long long sKb, float scale, void* stream) {
    if (!q || !k || !w || !acc) return IEF_EINVAL;
    if (heads <= 0 || heads > BLEND_MAX_HEADS || N <= 0 || L <= 0 || L > 128 || ldw < L || d <= 0 || (d & 7) || row0 < 0 || Bp < 1 ||
        Bp > BLEND_MAX_ROWS)
        return IEF_ESHAPE;
    if ((((uintptr_t)q | (uintptr_t)k) & 15) || ((ldq | ldk) & 3) || ((sQb | sKb) & 3) || (((uintptr_t)w | (uintptr_t)acc) & 3)) return IEF_EALIGN;
    hipLaunchKernelGGL(cross_blend_mass_f32_kernel, dim3(N), dim3(64 * (heads < 8 ? heads : 8)), 0, (hipStream_t)stream, q, k, w, acc,
                       row0, Bp, heads, N, L, ldw, d, ldq, ldk, sQb, sKb, scale);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// One workgroup of 256 threads per (target row i >= 1, channel c).  Thread t is pixel t of the 16 x 16 image: for row 0 and for row
// i it takes the 3 x 3 maximum around its pixel (cells outside the image do not take part: -inf padding), the workgroup takes the
// image maximum (order-free), the pixel is divided by it -- an IEEE division -- and compared with the threshold; 0 / 0 is NaN and
// compares false.  The OR of the two bits stays in LDS as 0.f / 1.f, and the threads then walk the H x W plane:
// x[i] = x[0] + m * (x[i] - x[0]), a subtraction, a multiplication and an addition, each rounded (no contraction in this file).
// Row 0 is only read; plane (i, c) is written by this workgroup alone.
__global__ __launch_bounds__(256) void local_blend_f32_kernel(const float* __restrict__ acc, const float* __restrict__ thres,
                                                             float* __restrict__ x, int C, int H, int W) {
    __shared__ float img[2][256];
    __shared__ float red[2][4];
    __shared__ float msk[256];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int c = blockIdx.x, i = blockIdx.y + 1;
    img[0][tid] = acc[tid];
    img[1][tid] = acc[i * 256 + tid];
    __syncthreads();
    const int py = tid >> 4, px = tid & 15;
    float pooled[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        float m = -INFINITY;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int yy = py + dy, xx = px + dx;
                if (yy >= 0 && yy < 16 && xx >= 0 && xx < 16) m = fmaxf(m, img[r][yy * 16 + xx]);
            }
        pooled[r] = m;
        const float mx = wave_max(m);
        if (lane == 0) red[r][wid] = mx;
    }
    __syncthreads();
    const float th = *thres;
    bool bit = false;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float mx = fmaxf(fmaxf(red[r][0], red[r][1]), fmaxf(red[r][2], red[r][3]));
        bit |= (pooled[r] / mx) > th;
    }
    msk[tid] = bit ? 1.f : 0.f;
    __syncthreads();
    const int HW = H * W, cy = H >> 4, cx = W >> 4;
    const float* x0 = x + (long long)c * HW;
    float* xi = x + ((long long)i * C + c) * HW;
    for (int p = tid; p < HW; p += 256) {
        const int y = p / W, xx = p - y * W;
        const float m = msk[(y / cy) * 16 + xx / cx];
        const float a = x0[p], b = xi[p];
        xi[p] = a + m * (b - a);
    }
}

extern "C" int ief_local_blend_f32(const float* acc, const float* thres, float* x, int Bp, int C, int H, int W, void* stream) {
    if (!acc || !thres || !x) return IEF_EINVAL;
    if (Bp < 2 || Bp > 65535 || C < 1 || C > 65535 || H < 16 || W < 16 || (H & 15) || (W & 15) || H > 16384 || W > 16384) return IEF_ESHAPE;
    if (((uintptr_t)acc | (uintptr_t)thres | (uintptr_t)x) & 3) return IEF_EALIGN;
    hipLaunchKernelGGL(local_blend_f32_kernel, dim3(C, Bp - 1), dim3(256), 0, (hipStream_t)stream, acc, thres, x, C, H, W);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
