// DiffEdit (Couairon, Verbeek, Schwenk, Cord, "DiffEdit: Diffusion-based semantic image editing with mask guidance"): the two
// small kernels of the mask inference.  The masked CFG + DDIM step lives next to its siblings in elementwise.hip.
//   diffedit_map_accum   acc[p] += sum over rows and channels of |eps_a - eps_b|, in a fixed order
//   diffedit_mask        d = acc / count;  v = min(max(d, 0), ratio mean(d)) / (ratio mean(d));  mask = v > thres
// Plain fp32 on the vector ALU, one writer per output element, no atomics; built without fma contraction and without reassociation
// (the generic rule of the Makefile), so the summation orders below are the ones the hardware runs.
#include "ief_common.h"
#include "ief_params.h"

// One lane per pixel p, coalesced over p.  For row r: s_r = (..((|d_0| + |d_1|) + |d_2|)..) over the channels in order, then
// acc[p] = acc[p] + s_r, rows in order -- so R rows in one launch and the same rows spread over several launches give the same bits.
// Channels go four at a time: eight independent loads are in flight per lane before the first add needs one of them.
__global__ __launch_bounds__(64) void diffedit_map_accum_kernel(const float* __restrict__ ea, const float* __restrict__ eb,
                                                                float* __restrict__ acc, int R, int C, int hw) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= hw) return;
    float a = acc[p];
    for (int r = 0; r < R; ++r) {
        const float* __restrict__ pa = ea + (long long)r * C * hw + p;
        const float* __restrict__ pb = eb + (long long)r * C * hw + p;
        float s = 0.0f;                      // 0 + |d_0| is |d_0| exactly
        int c = 0;
        for (; c + 4 <= C; c += 4) {
            float va[4], vb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                va[j] = pa[(long long)(c + j) * hw];
                vb[j] = pb[(long long)(c + j) * hw];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) s = s + fabsf(va[j] - vb[j]);
        }
        for (; c < C; ++c) s = s + fabsf(pa[(long long)c * hw] - pb[(long long)c * hw]);
        a = a + s;
    }
    acc[p] = a;
}

extern "C" int ief_diffedit_map_accum_f32(const float* eps_a, const float* eps_b, float* acc, int R, int C, int hw, void* stream) {
    if (!eps_a || !eps_b || !acc) return IEF_EINVAL;
    if (R <= 0 || C <= 0 || hw <= 0) return IEF_ESHAPE;
    if (((uintptr_t)eps_a | (uintptr_t)eps_b | (uintptr_t)acc) & 3) return IEF_EALIGN;
    hipLaunchKernelGGL(diffedit_map_accum_kernel, dim3((hw + 63) / 64), dim3(64), 0, (hipStream_t)stream, eps_a, eps_b, acc, R, C, hw);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}

// One workgroup of 256 lanes (4 waves), any hw >= 1.  The mean of d = acc / count is reduced in a fixed order:
//   1. lane t adds d[t], d[t + 256], d[t + 512], ... in that order (lanes past hw hold 0);
//   2. inside a wave, six butterfly rounds v += shfl_xor(v, 32), 16, 8, 4, 2, 1 (every lane ends with the same sum);
//   3. the four wave sums are added in wave order, ((w_0 + w_1) + w_2) + w_3, by every lane alike;
// then mean = sum / hw, clamp = ratio * mean, v = min(max(d, 0), clamp) / clamp (an IEEE division) and mask = v > thres ? 1 : 0.
// mean == 0 gives v = 0 / 0 = NaN, which compares false: an all-zero mask.
__global__ __launch_bounds__(256) void diffedit_mask_kernel(const float* __restrict__ acc, float* __restrict__ mask, int hw,
                                                            float count, float ratio, float thres) {
    __shared__ float wsum[4];
    float part = 0.0f;
    for (int p = threadIdx.x; p < hw; p += 256) part = part + acc[p] / count;
    part = wave_sum(part);
    if (lane_id() == 0) wsum[threadIdx.x >> 6] = part;
    __syncthreads();
    const float total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    const float clamp = ratio * (total / (float)hw);
    for (int p = threadIdx.x; p < hw; p += 256) {
        float d = acc[p] / count;
        d = d < 0.0f ? 0.0f : d;
        d = d > clamp ? clamp : d;
        mask[p] = d / clamp > thres ? 1.0f : 0.0f;
    }
}

extern "C" int ief_diffedit_mask_f32(const float* acc, float* mask_out, int hw, int count, float ratio, float thres, void* stream) {
    if (!acc || !mask_out) return IEF_EINVAL;
    if (hw <= 0 || count <= 0) return IEF_ESHAPE;
    if (((uintptr_t)acc | (uintptr_t)mask_out) & 3) return IEF_EALIGN;
    hipLaunchKernelGGL(diffedit_mask_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, acc, mask_out, hw, (float)count, ratio, thres);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
