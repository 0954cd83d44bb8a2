// The complete backward of a short-key cross-attention on the fp32-storage reverse pass (precision "f16x3" / "f32"): what
// null-text inversion optimises flows through K and V of the 77-key modules only
// (/root/reference/p2p/inversion/nti.py:15-33 differentiates /root/reference/p2p/model/register.py:43-51 with autograd).
//     P    = softmax_j(scale q.K_j)
//     dP_j = dO.V_j
//     dS_j = P_j (dP_j - sum_i dP_i P_i)
//     dQ_n = scale sum_j dS_nj K_j                     (optional; overwrites)
//     dK_j = scale sum_n dS_nj Q_n                     (overwrites)
//     dV_j =       sum_n P_nj  dO_n                    (overwrites)
// Plain fp32 FMAs in a fixed order, no map or score leaves the CU.  Two launches:
//   cross_bwd_f32_kernel<D>   one workgroup per (QB queries, head, batch row).
//       QUERY PHASE, the structure of csrc/cross_map_grad_f32.hip: K and V of the (batch, head) in LDS, G = D / DC adjacent lanes
//       own one query, group sums on the data-parallel primitives, every query keeps two columns in LDS -- P_j and dP_j -- and
//       dS_j then replaces dP_j.  The lanes also leave their slices of q and dO in LDS.  A dead lane of a ragged last block
//       shadows query N - 1 for the group sums; its columns and rows are ZEROED, or the key phase would count that query again.
//       KEY PHASE: the [L x QB] . [QB x D] products dS^T Q and P^T dO of the workgroup's own queries.  Thread (kg, c4) owns the
//       4 channels c4 of the keys kg, kg + KG, kg + 2 KG, ... (KG = 256 / (D / 4) key groups) and walks the queries in ascending
//       order, four at a time: their q / dO pieces are read once (16 bytes each, consecutive lanes consecutive pieces) and
//       serve every key the thread owns; per key one 16-byte read per column gives the four queries' dS / P.
//       Column rows are rotated by 4 j floats (cb_col): QB floats are a multiple of 128 bytes, so unrotated every key's row would
//       start in the same bank and the 64 / (D / 4) + 1 keys a wave reads at once would collide; rotated they fall into
//       different 16-byte bank groups, and the per-query walk (lanes = consecutive queries of one key) stays conflict free.
//       The partials go to scratch [B][heads][blocks][2][L][D], dK's already times scale.
//   cross_bwd_reduce_kernel   adds the partials of the blocks in ascending block order and overwrites dK / dV through their
//       leading dimensions.  No floating-point atomics and no hand-off inside a launch: the kernel boundary is the release.
// Row b of every result depends on row b of the operands alone, and on nothing in the launch geometry that B changes.
// LDS: 8 L D (K, V) + 8 L QB (columns) + 8 QB D (q, dO rows) bytes = L (1280, 1344, 1024, 1152, 1536) + (32, 40, 32, 40, 40) KiB for
// D = 32 .. 160; D = 160 sets IEF_CROSS_BWD_MAX_L = 80 (exactly 160 KiB); L = 77: 131,328 / 144,448 / 111,616 / 129,664 / 159,232 bytes.
#include "cross_f32_common.h"

struct CbArgs {
    const float* Q; const float* K; const float* V; const float* dO;
    float* dQ; float* scratch;
    int N, L, heads;
    int ldq, ldk, ldv, ldo, lddq;
    float scale;
};

static constexpr size_t cb_lds(int L, int d) { return 8 * ((size_t)L * d + (size_t)L * cmg_qb(d) + (size_t)cmg_qb(d) * d); }
static_assert(cb_lds(IEF_CROSS_BWD_MAX_L, 160) <= 160 * 1024 && cb_lds(IEF_CROSS_BWD_MAX_L + 1, 160) > 160 * 1024,
              "IEF_CROSS_BWD_MAX_L is the largest L whose LDS image fits a CU at d = 160");
static_assert(cb_lds(IEF_CROSS_BWD_MAX_L, 32) <= 160 * 1024 && cb_lds(IEF_CROSS_BWD_MAX_L, 40) <= 160 * 1024 &&
              cb_lds(IEF_CROSS_BWD_MAX_L, 64) <= 160 * 1024 && cb_lds(IEF_CROSS_BWD_MAX_L, 80) <= 160 * 1024, "");
static_assert(IEF_CROSS_BWD_MAX_L >= 77, "the text encoders' 77 tokens");

// entry (key j, query x of the workgroup) of a [L][QB] column image; x + 4 j stays inside the row (QB is a power of two) and a
// 4-aligned run of four queries stays contiguous and 16-byte aligned
template <int QB>
__device__ __forceinline__ int cb_col(int j, int x) { return j * QB + ((x + 4 * j) & (QB - 1)); }

template <int D>
__global__ __launch_bounds__(256) void cross_bwd_f32_kernel(const CbArgs p) {
    constexpr int DC = cmg_dc(D), G = D / DC, QB = 256 / G, D4 = D / 4, JB = 4;
    constexpr int KG = 256 / D4, ACC = (IEF_CROSS_BWD_MAX_L + KG - 1) / KG;      // key groups; keys per thread in the key phase
    static_assert((QB & (QB - 1)) == 0 && QB % 4 == 0 && KG * D4 <= 256, "");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int L = p.L;
    float* Ks = (float*)smem_raw;                     // [L][D]
    float* Vs = Ks + L * D;                           // [L][D]
    float* SP = Vs + L * D;                           // [L][QB]  scores, then P            (rows rotated: cb_col)
    float* SD = SP + L * QB;                          // [L][QB]  dP, then dS
    float* Qs = SD + L * QB;                          // [QB][D]  q rows of this workgroup, zero past query N - 1
    float* Gs = Qs + QB * D;                          // [QB][D]  dO rows
    const int tid = threadIdx.x;
    const int head = blockIdx.y, b = blockIdx.z;
    for (int c = tid; c < L * D4; c += 256) {
        const int j = c / D4, c4 = c - j * D4;
        *(f32x4*)(Ks + c * 4) = *(const f32x4*)(p.K + ((long long)b * L + j) * p.ldk + head * D + c4 * 4);
        *(f32x4*)(Vs + c * 4) = *(const f32x4*)(p.V + ((long long)b * L + j) * p.ldv + head * D + c4 * 4);
    }
    __syncthreads();
    // ---------------------------------------------------------------- query phase
    const int ql = tid / G, part_id = tid % G;        // query of this workgroup, slice of the head dim
    const int n = blockIdx.x * QB + ql;
    const bool live = n < p.N;
    const int nq = live ? n : p.N - 1;                // dead lanes shadow the last query (they take part in the group sums)
    const int c0 = part_id * DC;
    float xv[DC];
    {
        const float* q = p.Q + ((long long)b * p.N + nq) * p.ldq + head * D + c0;
#pragma unroll
        for (int c = 0; c < DC; c += 4) {
            const f32x4 t = *(const f32x4*)(q + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) xv[c + e] = t[e];
            *(f32x4*)(Qs + ql * D + c0 + c) = live ? t : f32x4{0.f, 0.f, 0.f, 0.f};
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
                SP[cb_col<QB>(j0 + u, ql)] = a[u];
                mx = fmaxf(mx, a[u]);
            }
    }
    float sum = 0.f;
#pragma unroll 4
    for (int j = 0; j < L; ++j) {
        const float e = expf(SP[cb_col<QB>(j, ql)] - mx);
        SP[cb_col<QB>(j, ql)] = e;
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
            *(f32x4*)(Gs + ql * D + c0 + c) = live ? t : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    float dot = 0.f;
    for (int j0 = 0; j0 < L; j0 += JB) {
        float a[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const float* vr = Vs + min(j0 + u, L - 1) * D + c0;
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
                const int ci = cb_col<QB>(j0 + u, ql);
                const float P = SP[ci] * inv;
                dot += a[u] * P;
                SP[ci] = P;
                SD[ci] = a[u];
            }
    }
    // dS over dP; the columns of a dead lane become zero
#pragma unroll 4
    for (int j = 0; j < L; ++j) {
        const int ci = cb_col<QB>(j, ql);
        const float P = SP[ci];
        SD[ci] = live ? P * (SD[ci] - dot) : 0.f;
        if (!live) SP[ci] = 0.f;
    }
    if (p.dQ) {                                       // uniform over the launch
#pragma unroll
        for (int c = 0; c < DC; ++c) xv[c] = 0.f;
        for (int j0 = 0; j0 < L; j0 += JB) {
            float w[JB];
#pragma unroll
            for (int u = 0; u < JB; ++u) w[u] = j0 + u < L ? SD[cb_col<QB>(min(j0 + u, L - 1), ql)] : 0.f;
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
    }
    __syncthreads();
    // ---------------------------------------------------------------- key phase
    const int c4 = tid % D4, kg = tid / D4;
    if (kg >= KG) return;                             // 256 - KG D4 threads (0, 6, 0, 16, 16) own nothing; no barrier follows
    f32x4 ak[ACC], av[ACC];
#pragma unroll
    for (int a = 0; a < ACC; ++a) ak[a] = av[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nl = min(QB, p.N - (int)blockIdx.x * QB);               // live queries; rows up to the next multiple of 4 are zero
    for (int n0 = 0; n0 < nl; n0 += 4) {
        f32x4 qr[4], gr[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            qr[u] = *(const f32x4*)(Qs + (n0 + u) * D + c4 * 4);
            gr[u] = *(const f32x4*)(Gs + (n0 + u) * D + c4 * 4);
        }
#pragma unroll
        for (int a = 0; a < ACC; ++a)
            if (a * KG < L) {                         // uniform; a key past L - 1 reads key L - 1 and is dropped below
                const int ci = cb_col<QB>(min(kg + a * KG, L - 1), n0);
                const f32x4 s = *(const f32x4*)(SD + ci), pr = *(const f32x4*)(SP + ci);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        ak[a][e] += s[u] * qr[u][e];
                        av[a][e] += pr[u] * gr[u][e];
                    }
            }
    }
    float* part = p.scratch + (((long long)b * p.heads + head) * gridDim.x + blockIdx.x) * 2 * L * D;
#pragma unroll
    for (int a = 0; a < ACC; ++a) {
        const int j = kg + a * KG;
        if (j < L) {
            *(f32x4*)(part + j * D + c4 * 4) = ak[a] * p.scale;
            *(f32x4*)(part + (L + j) * D + c4 * 4) = av[a];
        }
    }
}

// dK / dV[b][j][head D + c] = the partials of the blocks, added in ascending block order; one thread per 4 channels
__global__ __launch_bounds__(256) void cross_bwd_reduce_kernel(const float* __restrict__ scratch, float* __restrict__ dK,
                                                               float* __restrict__ dV, long long total, int heads, int L, int d,
                                                               int nblk, int lddk, int lddv) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int D4 = d / 4;
    const int c4 = (int)(i % D4);
    const int j = (int)(i / D4 % L);
    const int m = (int)(i / ((long long)D4 * L) % 2);
    const long long bh = i / ((long long)2 * D4 * L);
    const int head = (int)(bh % heads);
    const long long b = bh / heads;
    const long long step = (long long)2 * L * d;
    const float* src = scratch + bh * nblk * step + ((long long)m * L + j) * d + c4 * 4;
    f32x4 acc = *(const f32x4*)src;
    for (int w = 1; w < nblk; ++w) acc += *(const f32x4*)(src + w * step);
    float* out = m ? dV + (b * L + j) * lddv : dK + (b * L + j) * lddk;
    *(f32x4*)(out + head * d + c4 * 4) = acc;
}

extern "C" int ief_cross_bwd_blocks(int N, int d) {
    if (N <= 0 || !cmg_head_dim(d)) return 0;
    const int QB = cmg_qb(d);
    return (N + QB - 1) / QB;
}

extern "C" long long ief_cross_bwd_scratch_floats(int B, int heads, int N, int L, int d) {
    if (B <= 0 || heads <= 0 || L <= 0) return 0;
    return (long long)B * heads * ief_cross_bwd_blocks(N, d) * 2 * L * d;
}

extern "C" int ief_attn_cross_bwd_f32(const float* Q, const float* K, const float* V, const float* dO, float* dQ, float* dK, float* dV,
                                      float* scratch, int B, int heads, int N, int L, int d, int ldq, int ldk, int ldv, int ldo,
                                      int lddq, int lddk, int lddv, float scale, void* stream) {
    if (!Q || !K || !V || !dO || !dK || !dV || !scratch) return IEF_EINVAL;
    if (B <= 0 || B > 65535 || heads <= 0 || heads > 65535 || N <= 0 || L <= 0 || L > IEF_CROSS_BWD_MAX_L || !cmg_head_dim(d))
        return IEF_ESHAPE;
    const int C = heads * d;
    if (C > ldq || C > ldk || C > ldv || C > ldo || C > lddk || C > lddv || (dQ && C > lddq)) return IEF_ESHAPE;
    if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3) || (lddk & 3) || (lddv & 3) || (dQ && (lddq & 3))) return IEF_EALIGN;
    if (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)dO | (uintptr_t)dQ | (uintptr_t)dK | (uintptr_t)dV |
         (uintptr_t)scratch) & 15)
        return IEF_EALIGN;
    CbArgs p;
    p.Q = Q, p.K = K, p.V = V, p.dO = dO, p.dQ = dQ, p.scratch = scratch;
    p.N = N, p.L = L, p.heads = heads;
    p.ldq = ldq, p.ldk = ldk, p.ldv = ldv, p.ldo = ldo, p.lddq = lddq;
    p.scale = scale;
    const size_t lds = cb_lds(L, d);
    const int nblk = ief_cross_bwd_blocks(N, d);
    dim3 grid(nblk, heads, B);
    hipStream_t st = (hipStream_t)stream;
#define CB_LAUNCH(DD)                                                                                              \
    {                                                                                                              \
        hipError_t e = hipFuncSetAttribute((const void*)cross_bwd_f32_kernel<DD>,                                  \
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                  \
        if (e != hipSuccess) return (int)e;                                                                        \
        hipLaunchKernelGGL((cross_bwd_f32_kernel<DD>), grid, dim3(256), lds, st, p);                               \
    }
    switch (d) {
        case 32: CB_LAUNCH(32); break;
        case 40: CB_LAUNCH(40); break;
        case 64: CB_LAUNCH(64); break;
        case 80: CB_LAUNCH(80); break;
        default: CB_LAUNCH(160); break;
    }
#undef CB_LAUNCH
    IEF_LAUNCH_CHECK();
    const long long total = (long long)2 * B * heads * L * (d / 4);
    hipLaunchKernelGGL(cross_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, scratch, dK, dV, total,
                       heads, L, d, nblk, lddk, lddv);
    IEF_LAUNCH_CHECK();
    return IEF_OK;
}
