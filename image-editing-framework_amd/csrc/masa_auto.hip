// MasaCtrl's masks from cross-attention (`MutualSelfAttentionControlMaskAuto`, masactrl/model/attention_control.py) on the device:
// the fused plan kind 'masactrl_mask_auto' (control.py) never materialises a cross-attention map, so the two numbers per pixel the
// rule needs -- the head-mean map of the cond-source row summed over the reference tokens, that of the cond-target row summed over
// the current tokens -- are computed here from the q and k the cross-attention module already holds, and a second kernel turns
// the maps collected so far in a step into the class bits the class-masked attention launch reads (split_x3.hip, CLS).
// Both are tiny and latency-bound: plain fp32 on the vector ALU, no MFMA, a fixed summation order, one writer per element.
#include "ief_common.h"
#include "ief_params.h"

// One workgroup per (r, query n), one wave per head (up to 8 waves; wave w takes heads w, w + 8, ...): the launch is a chain of
// dependent loads and reductions, so it is paid in latency and the heads are what can run side by side.  Per head: lane l holds the
// scores of keys l and l + 64 (L <= 128) -- a sequential fma chain over d, q read as wave-uniform 16-byte pieces, k as per-lane
// ones -- then max, exp, and the two wave sums  sum_l e_l  and  sum_l w_l e_l ; the head's contribution is their quotient, left in
// LDS, and thread 0 adds the heads in head order.
#define MASS_MAX_HEADS 64
__global__ __launch_bounds__(512) void cross_token_mass_f32_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const float* __restrict__ w, float* __restrict__ out, int row_ref,
                                                                  int row_cur, int heads, int N, int L, int d, int ldq, int ldk,
                                                                  long long sQb, long long sKb, float scale) {
    __shared__ float part[MASS_MAX_HEADS];
    const int r = blockIdx.y, n = blockIdx.x;    // grid.x == N
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int row = r == 0 ? row_ref : row_cur;
    const float* qn = q + (long long)row * sQb + (long long)n * ldq;
    const float* kb = k + (long long)row * sKb;
    const int l0 = lane, l1 = lane + 64;
    const float w0 = l0 < L ? w[r * L + l0] : 0.f, w1 = l1 < L ? w[r * L + l1] : 0.f;
    const float* k0 = kb + (long long)(l0 < L ? l0 : 0) * ldk;
    const float* k1 = kb + (long long)(l1 < L ? l1 : 0) * ldk;
    for (int h = wid; h < heads; h += nw) {
        float s0 = 0.f, s1 = 0.f;
        for (int j = 0; j < d; j += 4) {
            const f32x4 qv = *(const f32x4*)(qn + h * d + j);
            const f32x4 a = *(const f32x4*)(k0 + h * d + j);
            const f32x4 b = *(const f32x4*)(k1 + h * d + j);
#pragma unroll
            for (int i = 0; i < 4; ++i) { s0 = __builtin_fmaf(qv[i], a[i], s0); s1 = __builtin_fmaf(qv[i], b[i], s1); }
        }
        s0 = l0 < L ? s0 * scale : -INFINITY;
        s1 = l1 < L ? s1 * scale : -INFINITY;
        const float m = wave_max(fmaxf(s0, s1));
        const float e0 = expf(s0 - m), e1 = expf(s1 - m);      // exp(-inf) = 0 for the lanes past L
        const float den = wave_sum(e0 + e1);
        const float num = wave_sum(w0 * e0 + w1 * e1);
        if (lane == 0) part[h] = num / den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int h = 0; h < heads; ++h) acc += part[h];
        out[r * N + n] = acc / (float)heads;
    }
}

extern "C" int ief_cross_token_mass_f32(const float* q, const float* k, const float* w, float* out, int row_ref, int row_cur, int heads,
                                        int N, int L, int d, int ldq, int ldk, long long sQb, long long sKb, float scale, void* stream) {
    if (!q || !k || !w || !out) return IEF_EINVAL;
    if (heads <= 0 || heads > MASS_MAX_HEADS || N <= 0 || L <= 0 || L > 128 || d <= 0 || (d & 7) || row_ref < 0 || row_cur < 0) return IEF_ESHAPE;
    if ((((uintptr_t)q | (uintptr_t)k) & 15) || ((ldq | ldk) & 3) || ((sQb | sKb) & 3) || (((uintptr_t)w | (uintptr_t)out) & 3)) return IEF_EALIGN;
    hipLaunchKernelGGL(cross_token_mass_f32_kernel, dim3(N, 2), dim3(64 * (heads < 8 ? heads : 8)), 0, (hipStream_t)stream, q, k, w, out,
                       row_ref, row_cur, heads, N, L, d, ldq, ldk, sQb, sKb, scale);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// One workgroup of 256 threads = the 16 x 16 pixels.  Thread i sums pixel i of the first c slots in slot order and divides by c
// (both rows), the workgroup takes each row's min and max (order-free), every pixel is normalised as (v - min) / (max - min) -- a
// subtraction and an IEEE division, in that order -- and kept in LDS; then token t of the res x res layer looks up its nearest
// source pixel and 32 consecutive tokens pack their (value >= thres) into one word: a wave's ballot is two words.
__global__ __launch_bounds__(256) void masa_auto_classes_kernel(const float* __restrict__ slots, int c, const float* __restrict__ thres,
                                                               int res, unsigned* __restrict__ k_cls, unsigned* __restrict__ q_cls,
                                                               const int* __restrict__ gate) {
    if (gate && *gate == 0) return;              // uniform: nobody reaches a barrier
    __shared__ float img[2][256];
    __shared__ float red[2][2][4];               // [row][min | max][wave]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float v[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        float s = 0.f;
        for (int i = 0; i < c; ++i) s += slots[(i * 2 + r) * 256 + tid];
        v[r] = s / (float)c;
        float mn = v[r], mx = v[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off)); }
        if (lane == 0) { red[r][0][wid] = mn; red[r][1][wid] = mx; }
    }
    __syncthreads();
    bool flat = false;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const float mn = fminf(fminf(red[r][0][0], red[r][0][1]), fminf(red[r][0][2], red[r][0][3]));
        const float mx = fmaxf(fmaxf(red[r][1][0], red[r][1][1]), fmaxf(red[r][1][2], red[r][1][3]));
        flat |= !(mx > mn);
        img[r][tid] = (v[r] - mn) / (mx - mn);
    }
    __syncthreads();
    const float th = *thres;
    const int ntok = res * res;
    for (int t0 = 0; t0 < ntok; t0 += 256) {     // ntok % 32 == 0: a 32-token word is whole or absent; uniform trip count
        const int t = t0 + tid;
        bool kb = false, qb = false;
        if (t < ntok && !flat) {
            const int y = t / res, x = t - y * res;
            const int px = ((y * 16) / res) * 16 + (x * 16) / res;
            kb = img[0][px] >= th;
            qb = img[1][px] >= th;
        }
        const unsigned long long bk = __builtin_amdgcn_ballot_w64(kb), bq = __builtin_amdgcn_ballot_w64(qb);
        if ((lane & 31) == 0 && t < ntok) {       // lanes 0 and 32 each store the word of their 32 tokens
            k_cls[t >> 5] = (unsigned)(bk >> lane);
            q_cls[t >> 5] = (unsigned)(bq >> lane);
        }
    }
}

extern "C" int ief_masa_auto_classes(const float* slots, int c, const float* thres, int res, unsigned* k_cls, unsigned* q_cls,
                                     const int* gate, void* stream) {
    if (!slots || !thres || !k_cls || !q_cls) return IEF_EINVAL;
    if (c < 1 || res < 1 || res > 256 || ((res * res) & 31)) return IEF_ESHAPE;
    if (((uintptr_t)slots | (uintptr_t)thres | (uintptr_t)k_cls | (uintptr_t)q_cls | (uintptr_t)gate) & 3) return IEF_EALIGN;
    hipLaunchKernelGGL(masa_auto_classes_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, slots, c, thres, res, k_cls, q_cls, gate);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
