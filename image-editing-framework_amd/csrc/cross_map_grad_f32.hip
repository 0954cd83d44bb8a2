// Pix2Pix-zero cross-attention guidance on the fp32-storage reverse pass (precision "f16x3" / "f32"), one launch per module:
// the gradient w.r.t. the queries of BOTH paths that meet there -- the value path of the attention layer (dO) and the map
// objective (/root/reference/pix2pix-zero/model/sd_utils.py:166-173) -- and the objective's value.
//     P    = softmax_j(scale q.K_j)
//     dP_j = dO.V_j + gcoef (P_j - ref_j)
//     dS_j = P_j (dP_j - sum_i dP_i P_i)
//     dQ   = scale sum_j dS_j K_j                      (overwrites)
//     loss[b][h][workgroup] = loss_coef sum (P - ref)^2
// Plain fp32 FMAs in a fixed order: with <= 106 keys the three products are small (1.2 GFLOP at the 64 x 64 level of SD1.5);
// what the materialised path pays for is eleven launches and four [B heads, N, L] maps through HBM, and no map or score leaves
// the CU here.  Structure of csrc/map_loss.hip: K and V of the (batch, head) sit in LDS as fp32 and are read as broadcasts,
// G = D / DC adjacent lanes own one query, each a DC-wide slice of the head dim (DC = 20 or 16: G = 2, 2, 4, 4, 8 for D = 32, 40,
// 64, 80, 160), a butterfly over the G lanes (data-parallel primitives, no LDS round trip) completes a dot product, and every
// QUERY keeps two columns in LDS -- P_j and dP_j, [L][256 / G] each, conflict free.  The G lanes of a query hold bit-equal
// values (the butterfly adds the same pairs in the same order on every lane), each writes the column entry and reads back what
// it wrote itself.
// LDS: L (8 D + 8 * 256 / G) + 16 bytes -- 1280, 1344, 1024, 1152, 1536 bytes per key for D = 32 .. 160: L <= 106 fits the 160 KiB
// of a CU at every head dim (IEF_CROSS_MAP_GRAD_MAX_L).
#include "cross_f32_common.h"                        // cmg_dc, group_sum: shared with csrc/cross_bwd_f32.hip

struct CmgArgs {
    const float* Q; const float* K; const float* V; const float* dO; const float* ref;
    float* dQ; float* loss;
    int N, L, heads;
    int ldq, ldk, ldv, ldo, lddq;
    float scale, gcoef, loss_coef;
};

static constexpr size_t cmg_lds(int L, int d) { return (size_t)L * (8 * d + 8 * (256 / (d / cmg_dc(d)))) + 16; }
static_assert(cmg_lds(IEF_CROSS_MAP_GRAD_MAX_L, 160) <= 160 * 1024 && cmg_lds(IEF_CROSS_MAP_GRAD_MAX_L + 1, 160) > 160 * 1024,
              "IEF_CROSS_MAP_GRAD_MAX_L is the largest L whose LDS image fits a CU at d = 160");
static_assert(cmg_lds(IEF_CROSS_MAP_GRAD_MAX_L, 32) <= 160 * 1024 && cmg_lds(IEF_CROSS_MAP_GRAD_MAX_L, 40) <= 160 * 1024 &&
              cmg_lds(IEF_CROSS_MAP_GRAD_MAX_L, 64) <= 160 * 1024 && cmg_lds(IEF_CROSS_MAP_GRAD_MAX_L, 80) <= 160 * 1024, "");

// JB keys at a time: their LDS reads and group sums are independent and overlap; each dot product still adds its terms in
// ascending order of the head dim, each accumulation over the keys in ascending order of the key.  A ragged last block of
// keys reads key L - 1 again and drops the result.
template <int D>
__global__ __launch_bounds__(256) void cross_map_grad_f32_kernel(const CmgArgs p) {
    constexpr int DC = cmg_dc(D), G = D / DC, QB = 256 / G, D4 = D / 4, JB = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int L = p.L;
    float* Ks = (float*)smem_raw;                     // [L][D]
    float* Vs = Ks + L * D;                           // [L][D]
    float* SP = Vs + L * D;                           // [L][QB]  scores, then P
    float* SD = SP + L * QB;                          // [L][QB]  dP
    float* red = SD + L * QB;                         // [4]
    const int tid = threadIdx.x;
    const int head = blockIdx.y, b = blockIdx.z;
    // K and V of this (batch, head): L x D floats each, 16-byte pieces (more pieces in flight per thread measured no faster)
    for (int c = tid; c < L * D4; c += 256) {
        const int j = c / D4, c4 = c - j * D4;
        *(f32x4*)(Ks + c * 4) = *(const f32x4*)(p.K + ((long long)b * L + j) * p.ldk + head * D + c4 * 4);
        *(f32x4*)(Vs + c * 4) = *(const f32x4*)(p.V + ((long long)b * L + j) * p.ldv + head * D + c4 * 4);
    }
    __syncthreads();
    const int ql = tid / G, part_id = tid % G;        // query of this workgroup, slice of the head dim
    const int n = blockIdx.x * QB + ql;
    const bool live = n < p.N;
    const int nq = live ? n : p.N - 1;                // dead lanes shadow the last query (they take part in the group sums)
    const int c0 = part_id * DC;
    float* sp = SP + ql;
    float* sd = SD + ql;
    float xv[DC];
    {
        const float* q = p.Q + ((long long)b * p.N + nq) * p.ldq + head * D + c0;
#pragma unroll
        for (int c = 0; c < DC; c += 4) {
            const f32x4 t = *(const f32x4*)(q + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[c + e] = t[e];
        }
    }
    float mx = -3.0e38f;
    for (int j0 = 0; j0 < L; j0 += JB) {
        float a[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float* kr = Ks + min(j0 + u, L - 1) * D + c0;
            a[u] = 0.f;
#pragma unroll
            for (int c = 0; c < DC; c += 4) {
                const f32x4 t = *(const f32x4*)(kr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[u] += xv[c + e] * t[e];
            }
        }
#pragma unroll
        for (int u = 0; u < JB; ++u) a[u] = group_sum<G>(a[u]) * p.scale;
#pragma unroll
        for (int u = 0; u < JB; ++u)
            if (j0 + u < L) {
                sp[(j0 + u) * QB] = a[u];
                mx = fmaxf(mx, a[u]);
            }
    }
    float sum = 0.f;
#pragma unroll 4
    for (int j = 0; j < L; ++j) {
        const float e = expf(sp[j * QB] - mx);
        sp[j * QB] = e;
        sum += e;
    }
    const float inv = 1.f / sum;
    {
        const float* g = p.dO + ((long long)b * p.N + nq) * p.ldo + head * D + c0;
#pragma unroll
        for (int c = 0; c < DC; c += 4) {
            const f32x4 t = *(const f32x4*)(g + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[c + e] = t[e];
        }
    }
    const float* rf = p.ref + (((long long)b * p.heads + head) * p.N + nq) * L;
    float part = 0.f, dot = 0.f;
    for (int j0 = 0; j0 < L; j0 += JB) {
        float a[JB], r[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const int j = min(j0 + u, L - 1);
            r[u] = rf[j];
            const float* vr = Vs + j * D + c0;
            a[u] = 0.f;
#pragma unroll
            for (int c = 0; c < DC; c += 4) {
                const f32x4 t = *(const f32x4*)(vr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[u] += xv[c + e] * t[e];
            }
        }
#pragma unroll
        for (int u = 0; u < JB; ++u) a[u] = group_sum<G>(a[u]);       // dO . V_j
#pragma unroll
        for (int u = 0; u < JB; ++u)
            if (j0 + u < L) {
                const float P = sp[(j0 + u) * QB] * inv;
                const float er = P - r[u];
                const float dP = a[u] + p.gcoef * er;
                part += er * er;
                dot += dP * P;
                sp[(j0 + u) * QB] = P;
                sd[(j0 + u) * QB] = dP;
            }
    }
    if (!live || part_id != 0) part = 0.f;            // one lane per query carries the objective
#pragma unroll
    for (int c = 0; c < DC; ++c) xv[c] = 0.f;
    for (int j0 = 0; j0 < L; j0 += JB) {
        float w[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const int j = min(j0 + u, L - 1);
            w[u] = j0 + u < L ? sp[j * QB] * (sd[j * QB] - dot) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float* kr = Ks + min(j0 + u, L - 1) * D + c0;
#pragma unroll
            for (int c = 0; c < DC; c += 4) {
                const f32x4 t = *(const f32x4*)(kr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[c + e] += w[u] * t[e];
            }
        }
    }
    if (live) {
        float* dq = p.dQ + ((long long)b * p.N + n) * p.lddq + head * D + c0;
#pragma unroll
        for (int c = 0; c < DC; c += 4) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = p.scale * xv[c + e];
            *(f32x4*)(dq + c) = o;
        }
    }
    // loss partial of this workgroup, fixed order
    part = wave_sum(part);
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0 && p.loss)
        p.loss[((long long)b * p.heads + head) * gridDim.x + blockIdx.x] = (red[0] + red[1] + red[2] + red[3]) * p.loss_coef;
}

extern "C" int ief_cross_map_grad_blocks(int N, int d) {
    if (N <= 0 || !cmg_head_dim(d)) return 0;
    const int QB = 256 / (d / cmg_dc(d));
    return (N + QB - 1) / QB;
}

extern "C" int ief_attn_cross_map_grad_f32(const float* Q, const float* K, const float* V, const float* dO, const float* ref, float* dQ,
                                           float* loss, int B, int heads, int N, int L, int d, int ldq, int ldk, int ldv, int ldo,
                                           int lddq, float scale, float gcoef, float loss_coef, void* stream) {
    if (!Q || !K || !V || !dO || !ref || !dQ) return IEF_EINVAL;
    if (B <= 0 || B > 65535 || heads <= 0 || heads > 65535 || N <= 0 || L <= 0 || L > IEF_CROSS_MAP_GRAD_MAX_L || !cmg_head_dim(d))
        return IEF_ESHAPE;
    const int C = heads * d;
    if (C > ldq || C > ldk || C > ldv || C > ldo || C > lddq) return IEF_ESHAPE;
    if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3) || (lddq & 3)) return IEF_EALIGN;
    if ((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)dO | (uintptr_t)dQ) & 15) ||
        (((uintptr_t)ref | (uintptr_t)loss) & 3))
        return IEF_EALIGN;
    CmgArgs p;
    p.Q = Q, p.K = K, p.V = V, p.dO = dO, p.ref = ref, p.dQ = dQ, p.loss = loss;
    p.N = N, p.L = L, p.heads = heads;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddq = lddq;
    p.scale = scale, p.gcoef = gcoef, p.loss_coef = loss_coef;
    const size_t lds = cmg_lds(L, d);
    dim3 grid(ief_cross_map_grad_blocks(N, d), heads, B);
    hipStream_t st = (hipStream_t)stream;
#define CMG_LAUNCH(DD)                                                                                             \
    {                                                                                                              \
        hipError_t e = hipFuncSetAttribute((const void*)cross_map_grad_f32_kernel<DD>,                             \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                  \
        if (e != hipSuccess) return (int)e;                                                                        \
        hipLaunchKernelGGL((cross_map_grad_f32_kernel<DD>), grid, dim3(256), lds, st, p);                          \
    }
    switch (d) {
        case 32: CMG_LAUNCH(32); break;
        case 40: CMG_LAUNCH(40); break;
        case 64: CMG_LAUNCH(64); break;
        case 80: CMG_LAUNCH(80); break;
        default: CMG_LAUNCH(160); break;
    }
#undef CMG_LAUNCH
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
