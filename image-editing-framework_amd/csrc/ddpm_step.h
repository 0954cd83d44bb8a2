// The mean of the eta = 1 DDPM update, shared by every kernel that steps on, or extracts, an edit-friendly DDPM noise space
// (elementwise.hip: ief_cfg_ddpm_step_f32, ief_ddpm_noise_maps_f32; ledits.hip: ief_ledits_ddpm_step_f32):
//   x0 = (x - sqrt(1-a_f) eps) / sqrt(a_f);  mu = sqrt(a_t) x0 + dir eps;  x' = mu + sigma z
// with sigma and dir = sqrt(1 - a_t - sigma^2) handed in (the host forms them in fp64).  One function for the mean, so a step undoes
// an extraction on the same eps up to the roundings of z itself, whichever guidance rule produced that eps.  The including file is
// built without fma contraction.  dpmpp_mu_of below is the same for the second-order SDE-DPM-Solver++ kernels.
#pragma once
#include "ief_common.h"

struct DdpmCoef { float sb_f, sa_f, sa_t, sigma, dir; };
__device__ __forceinline__ DdpmCoef ddpm_coef(const float* __restrict__ coef) {
    const float a_f = coef[0], a_t = coef[1];
    return {sqrtf(1.0f - a_f), sqrtf(a_f), sqrtf(a_t), coef[2], coef[3]};
}
// the mean from a guided estimate e that the caller has formed
__device__ __forceinline__ float ddpm_mu_of(const DdpmCoef& c, float e, float xi, float* __restrict__ x0o, long long i) {
    const float x0 = (xi - c.sb_f * e) / c.sa_f;
    if (x0o) x0o[i] = x0;
    return c.sa_t * x0 + c.dir * e;
}
// classifier-free guidance with one scale, then the mean
__device__ __forceinline__ float ddpm_mu_elem(const DdpmCoef& c, float g, const float* __restrict__ eu, const float* __restrict__ ec,
                                              const float* __restrict__ x, float* __restrict__ x0o, long long i) {
    float e = ec[i];
    if (eu) { const float u = eu[i]; e = u + g * (e - u); }
    return ddpm_mu_of(c, e, x[i], x0o, i);
}
// The second-order multistep mean (SDE-DPM-Solver++ 2M; Lu et al., "DPM-Solver++", and the solver LEDITS++ runs on): the mean above
// plus one correction on the x0 predictions of two consecutive steps,
//   mu = mu1 + c2 (x0 - x0_prev),   c2 = 1/2 sqrt(a_t) (1 - e^{-2h}) (h / h_prev)   formed by the host in fp64
// (sigma and dir ARE the solver's first-order coefficients: sigma_t^2 (1 - e^{-2h}) = sigma^2, sigma_t e^{-h} = dir).  c2 == 0 is
// an order-1 step: x0_prev is not read into the result, so mu is ddpm_mu_of's bit for bit.  Every kernel that steps or extracts
// at order 2 goes through this one function (elementwise.hip: ief_cfg_dpmpp_step_f32, ief_dpmpp_noise_maps_f32; ledits.hip:
// ief_ledits_dpmpp_step_f32).  *x0_cur receives the step's own x0 prediction, the next step's x0_prev.
__device__ __forceinline__ float dpmpp_mu_of(const DdpmCoef& c, float c2, float e, float xi, float x0_prev, float* x0_cur) {
    const float x0 = (xi - c.sb_f * e) / c.sa_f;
    *x0_cur = x0;
    const float mu1 = c.sa_t * x0 + c.dir * e;
    return c2 == 0.0f ? mu1 : mu1 + c2 * (x0 - x0_prev);
}
// the stored noise row a step reads: chosen by the device step counter, clamped as select_step_kernel clamps it
__device__ __forceinline__ const float* ddpm_noise_row(const float* __restrict__ noise, int noise_rows, const int* __restrict__ step,
                                                       long long row_elems) {
    int row = step[0];
    row = row < 0 ? 0 : (row >= noise_rows ? noise_rows - 1 : row);
    return noise + (long long)row * row_elems;
}
// x' from the mean: sigma == 0 does not read the noise into the result
__device__ __forceinline__ float ddpm_add_noise(const DdpmCoef& c, float mu, const float* __restrict__ z, long long j) {
    return c.sigma == 0.0f ? mu : mu + c.sigma * z[j];
}
