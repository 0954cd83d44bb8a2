// The CFG + DDIM update of one element, shared by every launch that must agree with ief_cfg_ddim_step_f32 bit for bit
// (elementwise.hip: the plain, the rectifying and the masked step; prox.hip: the proximal-guidance step):
//   eps = eps_u + g (eps_c - eps_u);  x0 = (x - sqrt(1-a_f) eps) / sqrt(a_f);  x' = sqrt(a_t) x0 + sqrt(1-a_t) eps
// Same operation order as the reference's scheduler.step / ddim_reverse so fp32 results stay
// within an ulp or two of the eager formula (/root/reference/p2p/model/sd_utils.py:74-76,
// /root/reference/p2p/inversion/ddim.py:14-17).  Every file that includes this is built without fma contraction.
#pragma once
#include <hip/hip_runtime.h>

struct DdimCoef { float sb_f, sa_f, sa_t, sb_t, g; };
__device__ __forceinline__ DdimCoef ddim_coef(const float* __restrict__ coef) {
    const float a_f = coef[0], a_t = coef[1];
    return {sqrtf(1.0f - a_f), sqrtf(a_f), sqrtf(a_t), sqrtf(1.0f - a_t), coef[2]};
}
// the two halves of the update: the x0 prediction from the guided eps, and x' from an x0 (which a caller may have moved) and that eps
__device__ __forceinline__ float ddim_x0(const DdimCoef& c, float x, float e) { return (x - c.sb_f * e) / c.sa_f; }
__device__ __forceinline__ float ddim_next(const DdimCoef& c, float x0, float e) { return c.sa_t * x0 + c.sb_t * e; }
// one element of the step, shared by the plain and the rectifying kernel: x' (returned) and the x0 prediction
__device__ __forceinline__ float cfg_ddim_elem(const DdimCoef& c, const float* __restrict__ eu, const float* __restrict__ ec,
                                               const float* __restrict__ x, float* __restrict__ x0o, long long i) {
    float e = ec[i];
    if (eu) { const float u = eu[i]; e = u + c.g * (e - u); }
    const float x0 = ddim_x0(c, x[i], e);
    if (x0o) x0o[i] = x0;
    return ddim_next(c, x0, e);
}
