/* C-ABI of libief_hip.so — the native boundary under the attention-controlled denoising path.
 *
 * The reference (AY-Liu/Image-Editing-Framework) has no native code and no FFI: its per-step
 * compute is PyTorch/diffusers eager CUDA (last row).  This header is therefore
 * the boundary a maintainer binds INSTEAD of those eager calls; each entry point cites the
 * reference call site whose arithmetic it replaces.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm tensors in our host
 *     code); outputs are caller-allocated; no entry point allocates, frees or synchronises;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it (graph-capturable);
 *   - return 0 on success, <0 for rejected arguments (IEF_E*), >0 = hipError_t of the launch;
 *     nothing throws;
 *   - ief_half = IEEE fp16 storage; all accumulation and statistics are fp32;
 *   - activations are channels-last: [B, H, W, C] == tokens-major [B, H*W, C].
 */
#ifndef IEF_HIP_H
#define IEF_HIP_H
#include <stdint.h>

#ifdef __HIPCC__
typedef _Float16 ief_half;
#else
typedef uint16_t ief_half;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define IEF_ABI_VERSION 4
int ief_abi_version(void);
/* name of the code object's target, e.g. "gfx950" */
const char* ief_target_arch(void);
/* sizeof the parameter structs as compiled (0: IefGemmParams, 1: IefAttnParams, 2: IefCrossParams, 3: IefAttnBwdParams,
 * 4: IefMapLossParams, 5: IefGemmF32Params, 6: IefAttnF32Params, 7: IefGemmX3pParams) */
int ief_struct_size(int which);

/* ------------------------------------------------------------------ GEMM / conv3x3
 * Out[m][n] = ( sum_k A(m,k) W[n][k] + bias[n] + rowvec[m / rows_per_batch][n] + residual[m][n] ) * out_scale
 * replaces: Attention.to_q/to_k/to_v/to_out, proj_in/proj_out, FF linears
 *           (/root/reference/p2p/model/register.py:33,40,41,54) and ResnetBlock2D.conv1/conv2/
 *           conv_shortcut + temb add + skip add (/root/reference/pnp/model/register.py:139-175).
 */
typedef struct IefGemmParams {
    const ief_half* A;        /* dense: [M][lda];  conv: NHWC source 1, C1 channels      */
    const ief_half* A2;       /* conv only: NHWC source 2 (channel concat), C2 channels  */
    const ief_half* W;        /* [N][ldw], K contiguous; conv: [Cout][3][3][C1+C2]        */
    ief_half* Out;            /* [M][ldo]                                                 */
    const float* bias;        /* [N] or NULL                                              */
    const float* rowvec;      /* [M / rows_per_batch][N] or NULL                          */
    const ief_half* residual; /* [M][ldr] or NULL                                         */
    int M, N, K;
    int lda, ldw, ldo, ldr;
    long long strideA, strideW, strideO, strideR; /* per batch index (dense, blockIdx.z) */
    /* conv3x3 geometry (pad 1): logical input H x Wd (after the optional 2x upsample) */
    int H, Wd, C1, C2, Ho, Wo, stride, ups, batch_images;
    int rows_per_batch;
    float out_scale;
    int tile_hint;            /* 0 auto; otherwise a tile id (BM x BN, waves): 1: 128x128, 2: 64x128, 3: 64x64, 4: 128x64,
                               * 5: 64x160, 6: 128x160 (2x2), 7: 128x160 (4x2), 8: 256x128, 9: 128x128 (4x2); 16-21: 7, 9, 8, 5, 3, 6
                               * with 4 / 4 / 4 / 2 / 2 / 2 LOADER waves (extra waves that stage the operands, the others only
                               * multiply); conv3x3 only: 14 / 15 = the halo kernel (256x80; 3x3, stride 1, pad 1, no fused 1x1
                               * range, rows of <= 64 pixels; the input tile stays in LDS across the nine taps), 15 with four
                               * loader waves; 15 also takes ups = 1 (rows of <= 128 pixels, H*Wd a multiple of 256, Wd | 256).  ief_gemm_tile_bm / _bn give BM / BN of an id. */
    /* conv only: extra K range appended after the 9 taps, read at the OUTPUT pixel itself
     * (a fused 1x1 convolution over up to two more NHWC sources, e.g. ResnetBlock2D.conv_shortcut
     * over the un-concatenated [x | skip]); W rows are then [9*(C1+C2) + CE1 + CE2] long.
     * Requires stride 1, no upsample. */
    const ief_half* E1; const ief_half* E2;
    int CE1, CE2;
    /* split-K: `splits` > 1 cuts the K loop into that many slices (grid.y); each slice writes an fp32
     * partial slab ws[slice][M][N] and a second launch sums the slabs and applies the epilogue.
     * ws must hold splits*M*N floats.  Used where M*N alone yields too few tiles for 256 CUs. */
    int splits;
    float* ws;
    /* flags bit 1 (value 2): fused GEGLU epilogue — W rows interleaved in groups of 8 ([8 hidden | 8 gate] ...),
     * Out[m][j] = (h_j + bias) * gelu(g_j + bias), Out has N/2 columns (FeedForward.net[0] of diffusers' GEGLU);
     * `zeros` must point at >= 16 bytes of device zeros (source of padded / out-of-range chunks). */
    int flags;
    const ief_half* zeros;
    int stages;               /* depth of the LDS operand ring: 0/2 (double buffer), 3 or 4 K tiles in flight */
    int pad_hi_only;          /* conv: 1 = zero padding only on the bottom/right edge (pad (0,1,0,1)), as the VAE encoder's
                               * stride-2 Downsample2D uses; 0 = symmetric padding 1 */
    /* LayerNorm folded into the NEXT linear (BasicTransformerBlock.norm1/2/3 -> to_q / to_qkv / ff.net[0]):
     *   LN(x) W^T = rstd (x (W gamma)^T - mu colsum) + beta W^T,   colsum[n] = sum_k (W gamma)[n][k]
     * so the consumer GEMM runs on the RAW residual stream with W gamma as weights and beta W^T folded into its bias, and
     * corrects per row in its epilogue; the row moments come from the epilogue of the GEMM that PRODUCED x.
     * rstat_out: producer side, [M][tiles_n][2] fp32 = (sum, sum of squares) of the fp16-rounded outputs over each N tile
     *            (tiles_n = ceil(N / BN) of the tile this launch uses; ief_gemm_tile_bn(tile_hint) gives BN);
     * rstat_in / rstat_slots / colsum / ln_eps: consumer side, rstat_in = the producer's rstat_out, rstat_slots its tiles_n;
     *            the LayerNorm width is this GEMM's K.  Neither side may use split-K; rstat_out excludes the GEGLU epilogue. */
    float* rstat_out;
    const float* rstat_in;
    int rstat_slots;
    const float* colsum;
    float ln_eps;
    /* GroupNorm statistics from the PRODUCER of its input: cstat_out [ceil(M / BM)][N][2] fp32 = per output channel the
     * (sum, sum of squares) of the fp16-rounded outputs over the BM rows of each M tile, summed in a fixed order
     * (ief_gemm_tile_bm(tile_hint) gives BM; the consumer is ief_groupnorm_cstat_f16).  No split-K, no GEGLU epilogue,
     * dense batch 1. */
    float* cstat_out;
    /* split-K combined INSIDE the launch: cnt points at one zeroed int per output tile (ceil(M/BM) * ceil(N/BN)).  Each
     * K-slice workgroup stores its fp32 slab tile, releases it at agent scope and draws a ticket from cnt[tile]; the
     * workgroup that draws the last ticket acquires, sums the slabs IN SLAB ORDER (so the sum does not depend on who came
     * last), applies the epilogue (and cstat_out, now allowed with splits > 1) and stores 0 back into cnt[tile]: the
     * counters are zero again when the launch ends.  NULL: the slabs are summed by a second launch, as before.  Launches
     * that may run concurrently must not share counters. */
    int* cnt;
} IefGemmParams;

int ief_gemm_f16(const IefGemmParams* p, int batch, void* stream);
/* BN (output columns per workgroup) of a tile id, 0 for an unknown id */
int ief_gemm_tile_bn(int tile_hint);
/* fills M, K, ldw, Ho, Wo, rows_per_batch itself from the geometry fields */
int ief_conv3x3_f16(const IefGemmParams* p, void* stream);

/* conv_in: latent NCHW fp32 [B,Cin,H,W] (Cin<=8) -> NHWC fp16 [B,H,W,Cout]; W [3][3][Cin][Cout] fp16 (k-major).
 * conv_out: NHWC fp16 [B,H,W,C] -> NCHW fp32 [B,Cout,H,W] (Cout<=8); W [Cout][3][3][C] fp16.
 * (UNet2DConditionModel.conv_in / conv_out, called at /root/reference/p2p/model/sd_utils.py:73)
 * conv_in splits Cout into the fewest equal slices (multiples of 8, <= 256 channels) whose fp32 weights fit 64 KiB of LDS.
 * Operands moved 8 halves at a time (w and out of conv_in, x and w of conv_out) must be 16-byte aligned, the fp32 ones 4-byte
 * aligned: IEF_EALIGN otherwise, nothing launched. */
int ief_conv_in_f32(const float* x, const ief_half* w, const float* bias, ief_half* out,
                    int B, int Cin, int H, int Wd, int Cout, void* stream);
int ief_conv_out_f32(const ief_half* x, const ief_half* w, const float* bias, float* out,
                     int B, int C, int H, int Wd, int Cout, void* stream);

/* ------------------------------------------------------------------ normalisation
 * GroupNorm over NHWC (+ optional SiLU): ResnetBlock2D.norm1/norm2 + nonlinearity
 * (/root/reference/pnp/model/register.py:105-110,149-158), Transformer2DModel.norm, conv_norm_out.
 * `partial` is scratch of >= B * (splits + 1) * groups * 2 floats (splits = ief_gn_splits(HW)); on completion its
 * LAST B * groups * 2 floats hold (mean, rstd) per (batch, group) — what ief_groupnorm_bwd_f16 takes as `stats`.
 * Two sources (x, x2) = channel concat [C1 | C2] normalised as one tensor, written to out [.., C1+C2].
 * Alignment (IEF_EALIGN otherwise, nothing launched): the one-workgroup form of GroupNorm moves channel pairs, so x, x2, out,
 * gamma, beta and partial must be 4-byte aligned; its three-launch form, ief_groupnorm_cstat_f16, LayerNorm and GEGLU move 8 halves
 * / 4 floats at a time, so their x, x2, in, out, gamma and beta must be 16-byte aligned.
 */
int ief_gn_splits(int HW);
int ief_groupnorm_silu_f16(const ief_half* x, const ief_half* x2, int C1, int C2, ief_half* out,
                           const float* gamma, const float* beta, float* partial,
                           int B, int HW, int groups, float eps, int apply_silu, void* stream);
/* LayerNorm over the last dim of [rows][C] (BasicTransformerBlock.norm1/2/3) */
int ief_layernorm_f16(const ief_half* x, ief_half* out, const float* gamma, const float* beta,
                      int rows, int C, float eps, void* stream);
/* GEGLU: in [rows][2*Ch] = [hidden | gate] -> out [rows][Ch] = hidden * gelu(gate) (erf form) */
int ief_geglu_f16(const ief_half* in, ief_half* out, int rows, int Ch, void* stream);

/* ------------------------------------------------------------------ attention
 * Fused softmax(Q K^T * scale) V, never materialising the map (flash-style), with per-batch
 * indirection of the Q / K / V source rows.  Identity maps = plain attention
 * (/root/reference/p2p/model/register.py:47-50 when the controller leaves the map alone).
 * q_src/k_src/v_src: DEVICE int32 [B] or NULL; out[b] = softmax(Q[q_src[b]] K[k_src[b]]^T) V[v_src[b]]:
 *   - P2P self-attention replace (attention_base.py:123,132-136): target rows take q_src = k_src = source row;
 *   - MasaCtrl mutual self-attention (/root/reference/masactrl/model/attention_control.py:59-66): k_src = v_src = source row.
 * Q [B][N][ldq], K/V [B][L][ldk/ldv], head h at columns [h*d, (h+1)*d); out [B][N][ldo].  d in {32,40,64,80,160}.
 */
typedef struct IefAttnParams {
    const ief_half* Q; const ief_half* K; const ief_half* V; ief_half* Out;
    int B, heads, N, L, d;
    int ldq, ldk, ldv, ldo;
    float scale;
    const int* q_src; const int* k_src; const int* v_src;
    float* lse;   /* ief_attn_flash_f16 only, may be NULL: fp32 [B][heads][N] row log-sum-exp (log2 units) for ief_attn_bwd_f16 */
    int variant;  /* ief_attn_flash_f16 only: 0 = default (software-pipelined 4-wave kernel), 1 = plain 4-wave kernel,
                     2 = 8-wave ping-pong kernel; same results within fp16 rounding, kept for A/B measurement */
} IefAttnParams;
int ief_attn_flash_f16(const IefAttnParams* p, void* stream);

/* Cross-attention with the Prompt-to-Prompt edit fused in (L <= 96 keys):
 *   P = softmax(Q K^T scale);  for batch rows b with edit_src[b] >= 0:
 *   P'[q][n] = c1[n] * sum_w P_src[q][w] M[w][n] + c2[n] * P_b[q][n];   out = P' V_b
 * which covers AttentionControlEdit.forward's cross branch (attention_base.py:118-121) for
 * replace (M = mapper, c1 = alpha_t, c2 = 1 - alpha_t; attention_control.py:15-16),
 * refine  (M = one-hot gather of mapper, c1 = alpha_t a, c2 = 1 - alpha_t a; :28-31) and
 * reweight (M = diag(equalizer) [x prev edit]; :42-46).
 * edit_src/edit_slot: DEVICE int32 [B]; MT: fp16 [slots][96][96] = M transposed, zero padded;
 * coef: fp32 [slots][2][96] = c1 | c2 of the CURRENT step.  All device memory so a captured
 * graph follows the step-dependent gates without re-capture.
 */
typedef struct IefCrossParams {
    const ief_half* Q; const ief_half* K; const ief_half* V; ief_half* Out;
    int B, heads, N, L, d;
    int ldq, ldk, ldv, ldo;
    float scale;
    const int* edit_src; const int* edit_slot;
    const ief_half* MT; const float* coef;
} IefCrossParams;
int ief_attn_cross_p2p_f16(const IefCrossParams* p, void* stream);

/* Generic hook path (materialised maps for arbitrary Python controllers / AttentionStore):
 * probs [B*heads][N][L] fp16 = softmax(Q K^T scale)  (Attention.get_attention_scores,
 * register.py:47) and out = probs V (torch.bmm + batch_to_head_dim, register.py:50-51). */
int ief_attn_probs_f16(const IefAttnParams* p, ief_half* probs, void* stream);
int ief_attn_apply_f16(const IefAttnParams* p, const ief_half* probs, void* stream);

/* ------------------------------------------------------------------ sampler step
 * Classifier-free guidance + DDIM update (or its inverse) in one launch:
 *   eps = eps_u + g (eps_c - eps_u);  x0 = (x - sqrt(1-a_from) eps)/sqrt(a_from);
 *   x' = sqrt(a_to) x0 + sqrt(1-a_to) eps
 * (/root/reference/p2p/model/sd_utils.py:74-76; inverse: /root/reference/p2p/inversion/ddim.py:9-18).
 * eps_u/eps_c/x/x_out fp32, n elements each; eps_u == NULL => eps = eps_c (no guidance).
 * coef: DEVICE fp32 [3] = {a_from, a_to, guidance}; x0_out optional.
 */
int ief_cfg_ddim_step_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out,
                          float* x0_out, const float* coef, long long n, void* stream);
/* Direct Inversion (Ju et al., "Direct Inversion: Boosting Diffusion-based Editing with 3 Lines of Code"): the same step in the
 * same launch, and batch row 0 (elements i < row_elems, the source branch of a two-branch edit) is moved back onto the stored
 * inversion trajectory:  x_out = x' + (z - x'),  z = traj[min(max(step[0], 0), traj_rows - 1)][i], both operations rounded in fp32.
 * Rows >= 1 of x_out and all of x0_out (the un-rectified x0 prediction) equal ief_cfg_ddim_step_f32's bit for bit.
 * traj: DEVICE fp32 [traj_rows][row_elems]; step: DEVICE int32 [1], read by the kernel and clamped as ief_select_step clamps it.
 * IEF_EINVAL: a null eps_c / x / x_out / coef / traj / step; IEF_ESHAPE: n <= 0, row_elems <= 0, n % row_elems != 0, traj_rows <= 0. */
int ief_cfg_ddim_step_rect_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out, float* x0_out,
                               const float* coef, long long n, long long row_elems,
                               const float* traj, int traj_rows, const int* step, void* stream);
/* Edit-friendly DDPM inversion (Huberman-Spiegelglas, Kulikov, Michaeli, "An Edit Friendly DDPM Noise Space"): CFG with one
 * guidance scale PER BATCH ROW and the eta = 1 update with a stored noise row, in one launch.  For element i of row b = i / row_elems:
 *   eps = eps_u + g_rows[b] (eps_c - eps_u);  x0 = (x - sqrt(1 - a_from) eps) / sqrt(a_from)
 *   mu  = sqrt(a_to) x0 + dir eps;            x_out = mu + sigma z,   z = noise[min(max(step[0], 0), noise_rows - 1)][i - b row_elems]
 * every operation rounded in fp32; sigma == 0 gives x_out = mu (the noise is not read into the result), and with dir = the fp32
 * sqrt(1 - a_to) that is ief_cfg_ddim_step_f32's x_out and x0_out bit for bit.  Every batch row reads the same noise row.
 * coef: DEVICE fp32 [4] = {a_from, a_to, sigma, dir}; g_rows: DEVICE fp32 [n / row_elems]; noise: DEVICE fp32 [noise_rows][row_elems];
 * step: DEVICE int32 [1], read by the kernel and clamped as ief_select_step clamps it.  eps_u == NULL: eps = eps_c, g_rows may be
 * NULL.  x0_out optional (the x0 prediction); x_out == x allowed.
 * IEF_EINVAL: a null eps_c / x / x_out / coef / noise / step, or eps_u without g_rows; IEF_ESHAPE: n <= 0, row_elems <= 0,
 * n % row_elems != 0, noise_rows <= 0. */
int ief_cfg_ddpm_step_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out, float* x0_out, const float* coef,
                          const float* g_rows, long long n, long long row_elems,
                          const float* noise, int noise_rows, const int* step, void* stream);
/* the extraction of the noise maps, R rows at R different timesteps in one launch: with mu as above (the same device function, so
 * the same bits) from row r of x_t and coef_rows[r],  z_out[r] = (x_prev[r] - mu) / sigma_r;  sigma_r == 0 gives a zero row.
 * coef_rows: DEVICE fp32 [R][5] = {a_from, a_to, sigma, dir, g}: the guidance scale of a row is its fifth column (one scale per
 * row, as there is one timestep per row).  eps_u == NULL: eps = eps_c.  All tensors fp32 [R][row_elems].
 * IEF_EINVAL: a null eps_c / x_t / x_prev / z_out / coef_rows; IEF_ESHAPE: R <= 0, row_elems <= 0. */
int ief_ddpm_noise_maps_f32(const float* eps_u, const float* eps_c, const float* x_t, const float* x_prev, float* z_out,
                            const float* coef_rows, int R, long long row_elems, void* stream);
/* The same step at solver order 2 (second-order multistep SDE-DPM-Solver++, the solver LEDITS++ is published with).  sigma and dir of
 * the eta = 1 update ARE the solver's first-order coefficients, so the step is that update plus one correction on the x0 predictions
 * of two consecutive steps:   mu = mu1 + c2 (x0 - x0_prev),   every operation rounded in fp32 in this order;  c2 == 0 (an order-1
 * step) does not read x0_prev into the result and gives ief_cfg_ddpm_step_f32's x_out and x0_out bit for bit.
 * coef: DEVICE fp32 [5] = {a_from, a_to, sigma, dir, c2}; x0_prev: DEVICE fp32 [n], the x0 prediction the previous step of the same
 * batch row wrote -- read and overwritten with this step's x0 by the lane that owns the element (nothing to zero before a first
 * step, whose c2 is 0).  Everything else as ief_cfg_ddpm_step_f32.
 * IEF_EINVAL: a null eps_c / x / x_out / x0_prev / coef / noise / step, or eps_u without g_rows; IEF_ESHAPE: n <= 0, row_elems <= 0,
 * n % row_elems != 0, noise_rows <= 0; IEF_EALIGN: a pointer off the 4-byte grid. */
int ief_cfg_dpmpp_step_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out, float* x0_out, float* x0_prev,
                           const float* coef, const float* g_rows, long long n, long long row_elems,
                           const float* noise, int noise_rows, const int* step, void* stream);
/* the extraction under that mean, R rows at R consecutive timesteps in one launch: z_out[r] = (x_prev[r] - mu_r) / sigma_r with
 * mu_r = mu1_r + c2_r (x0_r - x0_(r-1)), x0_r the x0 prediction of row r's own eps (no chain over stepped latents).  One lane owns
 * element j of every row and walks the rows in order; row 0 takes x0_(-1) from x0_carry (not read into the result where c2_0 == 0)
 * and the last row's x0 is written back to it, so consecutive launches over the rows of one image give the bits of one launch.
 * coef_rows: DEVICE fp32 [R][6] = {a_from, a_to, sigma, dir, g, c2}; x0_carry: DEVICE fp32 [row_elems].  sigma_r == 0 gives a zero
 * row; with c2 == 0 in every row z_out is ief_ddpm_noise_maps_f32's bit for bit.
 * IEF_EINVAL: a null eps_c / x_t / x_prev / z_out / coef_rows / x0_carry; IEF_ESHAPE: R <= 0, row_elems <= 0; IEF_EALIGN: a pointer
 * off the 4-byte grid. */
int ief_dpmpp_noise_maps_f32(const float* eps_u, const float* eps_c, const float* x_t, const float* x_prev, float* z_out,
                             const float* coef_rows, float* x0_carry, int R, long long row_elems, void* stream);
/* DiffEdit (Couairon, Verbeek, Schwenk, Cord, "DiffEdit: Diffusion-based semantic image editing with mask guidance"): the CFG + DDIM
 * step of ief_cfg_ddim_step_f32 in the same launch, and every batch row keeps x' only where ITS binary mask is set; elsewhere the
 * element is put back onto the stored inversion trajectory.  For element i = b row_elems + c hw + p:
 *   x_out = mask[b][p] != 0 ? x' : z[c hw + p],   z = traj[min(max(step[0], 0), traj_rows - 1)]
 * a select, so inside the mask x_out equals ief_cfg_ddim_step_f32's bit for bit and outside it the trajectory's; x0_out (optional) is
 * the un-masked x0 prediction, the plain step's everywhere.  mask: DEVICE fp32 [n / row_elems][hw]; traj: DEVICE fp32
 * [traj_rows][row_elems]; step: DEVICE int32 [1], read by the kernel and clamped as ief_select_step clamps it.  eps_u == NULL:
 * eps = eps_c; x_out == x allowed.
 * IEF_EINVAL: a null eps_c / x / x_out / coef / traj / step / mask; IEF_ESHAPE: n <= 0, row_elems <= 0, n % row_elems != 0, hw <= 0,
 * row_elems % hw != 0, traj_rows <= 0; IEF_EALIGN: a pointer off the 4-byte grid.  Nothing is launched by a refused call. */
int ief_cfg_ddim_step_masked_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out, float* x0_out,
                                 const float* coef, long long n, long long row_elems, long long hw,
                                 const float* traj, int traj_rows, const int* step, const float* mask, void* stream);
/* DiffEdit's difference map: eps_a, eps_b fp32 [R][C][hw], acc fp32 [hw] (zeroed by the caller before the first launch):
 *   acc[p] = (..((acc[p] + s_0) + s_1)..) + s_{R-1},   s_r = (..(|a_r0p - b_r0p| + |a_r1p - b_r1p|)..) + |a_r(C-1)p - b_r(C-1)p|
 * every operation rounded in fp32, rows and channels in order: R rows in one launch and the same rows over several launches give
 * the same bits.  One writer per element, no atomics.
 * IEF_EINVAL: a null pointer; IEF_ESHAPE: R <= 0, C <= 0, hw <= 0; IEF_EALIGN: a pointer off the 4-byte grid. */
int ief_diffedit_map_accum_f32(const float* eps_a, const float* eps_b, float* acc, int R, int C, int hw, void* stream);
/* DiffEdit's mask rule in one workgroup, any hw >= 1: d = acc / count; m = the mean of d over the hw pixels (fixed order: per-lane
 * strided partials of 256 lanes, a butterfly inside each wave, then the four waves in wave order);
 *   v = min(max(d, 0), ratio m) / (ratio m)  (an IEEE division);   mask_out[p] = v > thres ? 1.0f : 0.0f
 * m == 0 gives v = NaN, which compares false: an all-zero mask.  mask_out fp32 [hw], must not overlap acc.
 * IEF_EINVAL: a null pointer; IEF_ESHAPE: hw <= 0, count <= 0; IEF_EALIGN: a pointer off the 4-byte grid. */
int ief_diffedit_mask_f32(const float* acc, float* mask_out, int hw, int count, float ratio, float thres, void* stream);
/* LEDITS++ (Brack et al., "LEDITS++: Limitless Image Editing using Text-to-Image Models", CVPR 2024), three launches
 * (csrc/ledits.hip).  All arithmetic fp32, every operation rounded on its own, in a fixed order; one writer per element, no atomics
 * on global memory.  THE QUANTILE RULE of the two mask launches, for n values v >= 0, a rank lo in [0, n - 1] and a fraction frac
 * in [0, 1):  t = v_(lo) + frac (v_(hi) - v_(lo)),  hi = min(lo + 1, n - 1),  v_(k) the k-th smallest value (k from 0), both order
 * statistics exact (a radix select over the bit patterns); the bit of an element is  value >= t.  rank: DEVICE fp32 [E][2] =
 * {lo, frac} per concept, lo a whole number; the host forms q (n - 1) in double, takes its floor and rounds the remainder to fp32
 * (torch.quantile's linear rule with the arithmetic pinned).
 * ief_ledits_attn_mask_f32: acc fp32 [E][256], the 16 x 16 cross-attention mass of each concept's own tokens.  Per concept a 3 x 3
 * smoothing with the nine fp32 taps, (..((0 + taps[0] a_00) + taps[1] a_01)..) + taps[8] a_22 in row-major tap order, REFLECT
 * padding (index -1 reads 1, index 16 reads 14); then the quantile rule over the 256 smoothed values.  m1_out fp32 [E][256] holds
 * 0.0 / 1.0 and must not overlap acc.  One workgroup per concept.
 * IEF_EINVAL: a null pointer; IEF_ESHAPE: E outside [1, 8]; IEF_EALIGN: a pointer off the 4-byte grid.  Nothing is launched by a
 * refused call (this holds for all three). */
int ief_ledits_attn_mask_f32(const float* acc, const float* taps, const float* rank, float* m1_out, int E, void* stream);
/* eps fp32 [1 + E][C][H W]: row 0 the unconditional estimate, row 1 + e concept e's.  Per concept e and pixel p
 *   s[p] = (..(|d_0p| m + |d_1p| m)..) + |d_(C-1)p| m,   d_cp = eps[1 + e][c][p] - eps[0][c][p],   m = m1[e][cell(p)]
 * with cell = (floor(16 y / H), floor(16 x / W)), the nearest rule of ief_local_blend_f32; m1 == NULL: m = 1.  Then the quantile
 * rule over the H W values of s:  mask_out[e][p] = (s[p] >= t && m != 0) ? 1.0f : 0.0f,  thres_out[e] = t.  rank == NULL: no
 * threshold, mask_out is m1 spread to the pixels (all ones without m1); eps and thres_out are not touched and may be NULL.
 * m1 fp32 [E][256] holding 0.0 / 1.0; mask_out fp32 [E][H W]; thres_out fp32 [E].  One workgroup per concept, s staged in LDS.
 * IEF_EINVAL: a null mask_out, or rank without eps or thres_out; IEF_ESHAPE: E outside [1, 8], C outside [1, 16], H < 1, W < 1,
 * H W > 16384, or m1 given and H or W no multiple of 16; IEF_EALIGN: a pointer off the 4-byte grid. */
int ief_ledits_guidance_mask_f32(const float* eps, const float* m1, const float* rank, float* mask_out, float* thres_out, int E,
                                 int C, int H, int W, void* stream);
/* The masked multi-concept guidance and the eta = 1 update on ONE latent row x fp32 [row_elems] = [C][hw].  For element i, pixel
 * p = i % hw:   g = (..((0 + w_0) + w_1)..) + w_(E-1),   w_e = (scale[e] mask[e][p]) (eps[1 + e][i] - eps[0][i])
 * where a concept with scale[e] == 0 is skipped, not multiplied;  eps' = eps[0][i] + g;  then x0, mu and x_out = mu + sigma z from
 * eps' exactly as ief_cfg_ddpm_step_f32 forms them from its eps (the same device function): with E = 1, mask == NULL and
 * scale = {g} the two launches agree bit for bit.  eps fp32 [1 + E][row_elems]; mask fp32 [E][hw] or NULL (every value 1); scale:
 * DEVICE fp32 [E] for the current step, sign and warm-up / cool-down gate folded in; coef, noise, noise_rows, step as there.
 * x0_out optional; x_out == x allowed.
 * IEF_EINVAL: a null eps / scale / x / x_out / coef / noise / step; IEF_ESHAPE: E outside [1, 8], hw outside [1, 16384],
 * row_elems no multiple of hw or outside [hw, 16 hw], noise_rows <= 0; IEF_EALIGN: a pointer off the 4-byte grid. */
int ief_ledits_ddpm_step_f32(const float* eps, const float* mask, const float* scale, const float* x, float* x_out, float* x0_out,
                             const float* coef, long long row_elems, long long hw, const float* noise, int noise_rows,
                             const int* step, int E, void* stream);
/* The same step at solver order 2: the guidance formed exactly as above, then the mean of ief_cfg_dpmpp_step_f32 (the same device
 * function).  coef: DEVICE fp32 [5] = {a_from, a_to, sigma, dir, c2}; x0_prev: DEVICE fp32 [row_elems], read and overwritten with this
 * step's x0 prediction by the lane that owns the element.  c2 == 0 gives ief_ledits_ddpm_step_f32's outputs bit for bit.
 * IEF_EINVAL: a null eps / scale / x / x_out / x0_prev / coef / noise / step; IEF_ESHAPE and IEF_EALIGN as there. */
int ief_ledits_dpmpp_step_f32(const float* eps, const float* mask, const float* scale, const float* x, float* x_out, float* x0_out,
                              float* x0_prev, const float* coef, long long row_elems, long long hw, const float* noise,
                              int noise_rows, const int* step, int E, void* stream);
/* Proximal guidance on a negative-prompt-inversion edit (Miyake et al., "Negative-prompt Inversion"; Han et al., "Improving
 * Tuning-Free Real Image Editing with Proximal Guidance"), two launches (csrc/prox.hip).  All arithmetic fp32, every operation
 * rounded on its own; one writer per element, no atomics on global memory, no buffer the caller must zero, the same bits from run
 * to run.  The UNet batch is [u_0 .. u_(B-1) | c_0 .. c_(B-1)]; row 0 is the source, rows >= 1 are targets.
 * ief_prox_threshold_f32: thres_out[b] = the quantile of |eps_c - eps_u| over the row_elems elements of batch row b, by THE QUANTILE
 * RULE of the LEDITS++ launches above:  t = v_(lo) + frac (v_(hi) - v_(lo)),  hi = min(lo + 1, row_elems - 1), both order statistics
 * exact.  rank: DEVICE fp32 [2] = {lo, frac}, one pair for every row (the rows have one length), formed on the host as there.
 * eps_u, eps_c fp32 [B][row_elems]; thres_out fp32 [B].  One workgroup per row, the row's values in registers.
 * IEF_EINVAL: a null pointer; IEF_ESHAPE: B < 1, row_elems outside [1, 65536]; IEF_EALIGN: a pointer off the 4-byte grid.  Nothing
 * is launched by a refused call (this holds for both). */
int ief_prox_threshold_f32(const float* eps_u, const float* eps_c, const float* rank, float* thres_out, int B, long long row_elems,
                           void* stream);
/* The CFG + DDIM step under proximal guidance.  For element i = b row_elems + c h w + p, with d = eps_c - eps_u and
 * lambda = thres[b]:
 *   rows b >= 1 with prox_on != 0:   mode 0 (l0)  d' = |d| > lambda ? d : 0
 *                                    mode 1 (l1)  d' = d > lambda ? d - lambda : (d < -lambda ? d + lambda : 0);    otherwise d' = d
 *   eps = eps_u + g d';   x0 = (x - sqrt(1 - a_from) eps) / sqrt(a_from)      (the device function of ief_cfg_ddim_step_f32)
 *   rows b >= 1 with eta != 0:       m = 1 if any element of the same row and channel within Chebyshev distance radius of pixel p
 *                                    has |d| > lambda (pixels outside the image count as 0); with prox_on == 0, m = 1 everywhere;
 *                                    x0 = m ? x0 : x0 - eta (x0 - z0[c h w + p])
 *   x_out = sqrt(a_to) x0 + sqrt(1 - a_to) eps;   x0_out (optional) = the x0 above
 * Row 0 is never thresholded and never pulled: it equals ief_cfg_ddim_step_f32's x_out and x0_out bit for bit, and so does every
 * row when prox_on == 0 and eta == 0.  coef: DEVICE fp32 [5] = {a_from, a_to, g, prox_on, eta}; thres: DEVICE fp32 [n / row_elems]
 * (ief_prox_threshold_f32's output); z0: DEVICE fp32 [row_elems], the encoded source latent; eps_u, eps_c, x, x_out fp32 [n].
 * x_out == x allowed (the stencil reads eps_u and eps_c only); x0_out must not overlap the inputs.
 * IEF_EINVAL: a null eps_u / eps_c / x / x_out / coef / thres / z0; IEF_ESHAPE: n <= 0, row_elems outside [1, 65536],
 * n % row_elems != 0, h < 1, w < 1, row_elems no multiple of h w, mode not 0 or 1, radius outside [0, 3]; IEF_EALIGN: a pointer off
 * the 4-byte grid. */
int ief_cfg_ddim_step_prox_f32(const float* eps_u, const float* eps_c, const float* x, float* x_out, float* x0_out, const float* coef,
                               const float* thres, const float* z0, long long n, long long row_elems, int h, int w, int mode,
                               int radius, void* stream);
/* sinusoidal timestep embedding, flip_sin_to_cos, shift 0: out fp16 [B][dim] = [cos | sin] */
int ief_timestep_embedding_f16(const float* t, ief_half* out, int B, int dim, void* stream);
/* out = a + b elementwise on fp16 (residual add when a hook owns Attention.forward) */
int ief_add_f16(const ief_half* a, const ief_half* b, ief_half* out, long long n, void* stream);
/* out[b][:] = in[src[b]][:] for fp16 [B][row_elems], src a DEVICE int32 [B] with values in [0, B): Plug-and-Play's
 * feature injection (/root/reference/pnp/model/register.py:161-166) as a gather in front of conv2 */
int ief_gather_rows_f16(const ief_half* in, ief_half* out, const int* src, int B, long long row_elems, void* stream);
/* in-place row softmax over the last dim of fp16 [rows][L] (materialised attention of the VAE mid block, d = 512); L a multiple of 8
 * up to 16384 (IEF_ESHAPE), x 16-byte aligned (IEF_EALIGN) */
int ief_softmax_rows_f16(ief_half* x, int rows, int L, void* stream);
/* out[c][r] = in[r][c] for fp16 [R][C] (V^T for the P.V GEMM of the VAE attention) */
int ief_transpose_f16(const ief_half* in, ief_half* out, int R, int C, void* stream);
/* 1x1 convolution on a small fp32 NCHW tensor, Cin, Cout <= 8 (AutoencoderKL.quant_conv / post_quant_conv) */
int ief_pointwise_f32(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW,
                      void* stream);
/* y = silu(x) elementwise on fp16 (ResnetBlock2D time_emb_proj input) */
int ief_silu_f16(const ief_half* x, ief_half* out, long long n, void* stream);
/* fp16 <-> fp32 casts and row gather used to stage per-step tables inside a captured graph:
 * out[r][:] = table[idx[0] (device int32)][r][:], element size `esize` bytes, row bytes `rowbytes` */
int ief_cast_f32_to_f16(const float* x, ief_half* out, long long n, void* stream);
int ief_cast_f16_to_f32(const ief_half* x, float* out, long long n, void* stream);
/* out[:] = table[min(max(step[0], 0), n_rows - 1)][:]: the row index is read from device memory and CLAMPED to the table,
 * so a captured step graph replayed past the end of its schedule re-reads the last row instead of foreign memory */
int ief_select_step(const void* table, void* out, const int* step, long long bytes_per_step, int n_rows, void* stream);
int ief_advance_step(int* step, void* stream);

/* ------------------------------------------------------------------ reference-precision ("exact") mode: fp32 end to end
 * The reference computes in fp32 (/root/reference/p2p/edit_syn.py:38).  These entry points are the same operators on
 * fp32 activations and fp32 weights, contractions on the fp32-input MFMA (csrc/exact_f32.hip); the host picks them by
 * the dtype of the tensors it is handed (hip.py).  Attention in this mode MATERIALISES its maps in HBM as the
 * reference does (/root/reference/p2p/model/register.py:43-51): scores and P.V are two batched launches of ief_gemm_f32
 * with ief_softmax_rows_f32 (and the P2P edit, ief_p2p_cross_edit_f32) between them.
 * Alignment (x3 == 0): ief_gemm_f32 reads W and the conv sources (A, A2, E1, E2) in 16-byte pieces, and A of a linear product
 * unless lda or K is no multiple of 4 floats; ief_attn_flash_f32 reads Q, K, V so.  Those base pointers must be 16-byte aligned
 * and the batched products' sAb / sAh / sWb / sWh multiples of 4 floats: IEF_EALIGN otherwise, nothing launched. */
typedef struct IefGemmF32Params {
    const float* A;         /* [M][K] rows (lda) | conv: NHWC source 1 */
    const float* A2;        /* conv: NHWC source 2 of a channel concat, or NULL */
    const float* W;         /* [N][K] rows (ldw); transb: [K][N] rows (ldw) */
    float* Out;             /* [M][N] rows (ldo) */
    const float* bias;      /* [N] or NULL */
    const float* rowvec;    /* [M / rows_per_batch][N] or NULL */
    const float* residual;  /* [M][N] rows (ldr) or NULL */
    int M, N, K;
    int lda, ldw, ldo, ldr;
    int rows_per_batch;
    float out_scale;        /* out = (acc + bias + rowvec + residual) * out_scale */
    /* 3x3 implicit GEMM (conv != 0): same meaning as the fields of IefGemmParams */
    int conv, H, Wd, C1, C2, Ho, Wo, stride, ups, batch_images, pad_hi_only;
    const float* E1;
    const float* E2;
    int CE1, CE2;
    /* batched product (heads > 0): grid.z = batch * heads; element strides per batch row / head; optional batch-row
     * indirection of the A and W operands (P2P self-replace, MasaCtrl, Plug-and-Play source rows) */
    int batch, heads;
    long long sAb, sAh, sWb, sWh, sOb, sOh;
    const int* a_src;
    const int* w_src;
    int transb;
    int a_scalar;           /* set by the library: A rows are not 16-byte chunked */
    /* split-K (not batched): K cut `splits` ways over grid.y, fp32 slabs ws[splits][M][N], summed in slab order by a second
     * launch that applies the epilogue */
    int splits;
    float* ws;
    /* ABI 3: split-operand contraction (csrc/split_x3.hip).  x3 != 0: every fp32 operand element is split into two fp16
     * numbers (hi + lo of sa * a, of sb * w; sa, sb powers of two) while its tile is staged, the product runs on three
     * fp16 MFMAs per k-step (Ah Bh + Al Bh + Ah Bl, fp32 accumulate) and is divided by sa * sb; same operators, operands,
     * outputs and error codes as x3 == 0 (the fp32-input MFMA); |sa * a|, |sb * w| must stay below 1.3e5 */
    int x3;
    float sa, sb;
    /* set by the library (x3): every epilogue operand allows 16-byte accesses; conv channel counts are all multiples of
     * 32; bytes reachable from A / W / A2 / E1 / E2 (buffer descriptor sizes: each must stay below 4 GiB) */
    int vec_out, al32, fast_ok;
    unsigned bytesA, bytesW, bytesA2, bytesE1, bytesE2;
    /* x3: optional pre-split planes of a WEIGHT operand (made once per tensor by ief_x3_split_weights with scale sb): fp16
     * [2][N][K] contiguous (hi plane, lo plane); W is then not read.  Not for transb / batched products. */
    const void* Wp;
    /* x3, linear only: GEGLU fused into the epilogue -- the weight's rows are interleaved [8 hidden | 8 gate] per 16 columns
     * (the layout of ief_geglu_il_f32); Out is [M][N / 2] = hidden * gelu(gate) of (a . w + bias); no residual / rowvec / split-K */
    int geglu;
} IefGemmF32Params;
int ief_gemm_f32(const IefGemmF32Params* p, void* stream);
/* planes[0][i] = fp16(scale w[i]), planes[1][i] = fp16(scale w[i] - planes[0][i]); n % 4 == 0; w 16-byte aligned, planes 8-byte
 * aligned (IEF_EALIGN otherwise) */
int ief_x3_split_weights(const float* w, void* planes, long long n, float scale, void* stream);
int ief_gemm_x3_bn(int N);    /* x3 != 0: output-tile width (80 or 64) for N columns; ief_gemm_x3_bm(M, N): its row count (128) */
int ief_gemm_x3_bm(int M, int N);
/* the width the launch (conv != 0: 3x3 convolution) actually takes: 160 (8 waves, one workgroup per CU) where that tile is
   the faster one, else ief_gemm_x3_bn(N); the host's split-K policy counts tiles with it */
int ief_gemm_x3_bn_k(int conv, int N, int K);
void ief_gemm_x3_set_variant(int bits);   /* A/B measurements: bit 0 clear = never the 160-wide tile; bit 1 set = 32-key tiles in the fused attention */
int ief_gemm_f32_bn(int N);   /* output-tile width (64 or 128) the library uses for N columns; the M tile is 128 rows */
/* fused fp32 attention (maps never written): out[b] = softmax(scale q[q_src[b]] k[k_src[b]]^T) v[v_src[b]]; q [B][N][heads*d]
 * (row stride ldq, batch stride sQb; likewise k, v over L keys and out); d in {32, 40, 64, 80, 160}; *_src NULL = identity */
typedef struct IefAttnF32Params {
    const float* Q; const float* K; const float* V; float* Out;
    int B, heads, N, L, d;
    int ldq, ldk, ldv, ldo;
    long long sQb, sKb, sVb, sOb;
    float scale;
    const int* q_src; const int* k_src; const int* v_src;
    int x3;                 /* ABI 3: != 0 -> both products on split fp16 operands (csrc/split_x3.hip), softmax in fp32 */
    /* ABI 4 (split-operand kernels only): the output ALSO / ONLY as operand planes for the to_out GEMM (csrc/gemm_x3p.hip):
     * OutP hi plane [B][N][ldp] (batch stride sOPb), lo plane planeO elements further; Out may then be NULL */
    ief_half* OutP;
    long long planeO, sOPb;
    int ldp;
    /* ief_attn_cross_p2p_f32: power-of-two scale of the EDITED maps' hi / lo split, chosen by the host from the plan's
     * coefficients so that scale * max |c1| + |c2| stays below the fp16 range (AttentionReweight: c1 = alpha * equalizer);
     * 0 = 2^14 (maps <= 1) */
    float p_scale;
    /* ABI 4, ief_attn_flash_f32 with x3 != 0 only: Q / K / V given as OPERAND PLANES (the q|k|v GEMM's epilogue writes them) --
     * Qp / Kp / Vp hi planes with the layout of Q / K / V (same ld* and batch strides, in elements), lo planes planeQ / planeK /
     * planeV elements further; Q / K / V are then ignored.  The kernel stages K / V tiles by LDS-DMA and splits nothing
     * (attn_flash_x3p_kernel, csrc/split_x3.hip); d in {40, 64, 80}. */
    const ief_half* Qp; const ief_half* Kp; const ief_half* Vp;
    long long planeQ, planeK, planeV;
    const void* zeros;      /* >= 16 bytes of device zeros (source of key rows past L) when Qp is set */
    /* x3 != 0 only (fp32 Q / K / V or operand planes; with x3 == 0 a non-null lse is IEF_EINVAL): optional [B][heads][N]
     * receiving the row log-sum-exp in log2 units (max + log2 sum exp2) that ief_attn_bwd_x3 consumes; null: not written */
    float* lse;
    /* operand planes in (Qp set) only, appended to ABI 4: key_splits > 1 deals the KEYS of every (b, head, query block) over that
     * many workgroups, each writing an unnormalised partial (O, lazy max, row sum) to ws, and one combine launch merges them in
     * a fixed order (deterministic; for the batch-1 launches whose (query block, head) grid leaves most of the chip idle).  The
     * library clamps the count so that every split owns a key tile; a count that clamps to 1 (and key_splits <= 1) takes the
     * single launch and ws is not looked at.  ws: ief_attn_flash_ws_floats(...) fp32 of scratch, 16-byte aligned, the caller's
     * until the stream passes; ws_floats: its size.  Without Qp or with x3 == 0, key_splits > 1 is IEF_EINVAL; so are a null or
     * short ws; a misaligned one is IEF_EALIGN. */
    int key_splits; float* ws; long long ws_floats;
    /* operand planes in (Qp set) only, ABI 4; both null = the launches above (this pair sits in FRONT of the class words, which
     * sit in front of the gathered-rows fields: those stay the last three of the block; callers set fields by name and the
     * library checks ief_struct_size(6)).  TWO KEY / VALUE SEGMENTS under one softmax: k2_src / v2_src, device int32 [B].  Output
     * row b with k2_src[b] >= 0 attends over the L keys of batch row k_src[b] (identity if k_src is null) FOLLOWED by the L
     * keys of batch row k2_src[b], with the values of rows v_src[b] and v2_src[b] alike: one online softmax over 2 L keys, one
     * normalisation.  A row with k2_src[b] < 0 takes the first segment only and is bit-identical to the launch without the
     * pair; v2_src[b] is then not looked at.  Every entry >= 0 must be a batch row of K / V (the library cannot check device
     * lists).  Both pointers or neither, no lse, no key_splits > 1, no q_idx / k_idx, no q_cls / k_cls, Qp set and x3 != 0:
     * IEF_EINVAL otherwise; a pointer that is not 4-byte aligned: IEF_EALIGN.  Nothing is launched by a refused call.
     * d in {40, 64, 80}. */
    const int* k2_src; const int* v2_src;
    /* operand planes in (Qp set) only, ABI 4; both null = the launches above (the pair sits in FRONT of the gathered-rows
     * fields, which stay the last three of the block; callers set fields by name and the library checks ief_struct_size(6)).  CLASS-MASKED attention: every query
     * and every key carries one class bit, packed one uint32 per 32 consecutive tokens (bit i of word w = token 32 w + i): q_cls
     * [N / 32] and k_cls [L / 32], shared by every batch row of the launch.  A score whose query and key differ in class
     * contributes exactly nothing: query i takes softmax attention over the keys of its own class (a query whose class has no
     * key gets NaN).  All N rows of every batch row of Out / OutP are written; gate as below.  Both pointers or neither, N
     * and L multiples of 32, no lse, no key_splits > 1, no q_idx / k_idx, Qp set and x3 != 0: IEF_EINVAL otherwise; a
     * pointer that is not 4-byte aligned: IEF_EALIGN.  Nothing is launched by a refused call.  d in {40, 64, 80}. */
    const unsigned* k_cls; const unsigned* q_cls;
    /* operand planes in (Qp set) only, appended to ABI 4; all null = the launch above.  Attention over GATHERED token rows:
     * q_idx int32 [N]: query slot i reads row q_idx[i] of Q and its output goes to that same row of Out / OutP (rows not listed
     * are not written); k_idx int32 [L]: key slot j is row k_idx[j] of K and of V.  N and L are the LIST lengths; every index
     * must be a row of the operand it addresses (the library cannot check device lists).  Both lists or neither (IEF_EINVAL);
     * q_src / k_src / v_src select batch rows as ever.  gate: optional device int32; *gate == 0 makes the launch write
     * nothing (a captured step graph keeps the launch, a per-step table switches it).  With lse or key_splits > 1, without
     * Qp or with x3 == 0: IEF_EINVAL; a pointer that is not 4-byte aligned: IEF_EALIGN.  d in {40, 64, 80}. */
    const int* q_idx; const int* k_idx; const int* gate;
} IefAttnF32Params;
int ief_attn_flash_f32(const IefAttnF32Params* p, void* stream);
/* MasaCtrl's masks from cross-attention (masactrl/model/attention_control.py, MutualSelfAttentionControlMaskAuto), two launches.
 * ief_cross_token_mass_f32: out[r][n] = (1 / heads) sum_h sum_l w[r][l] softmax_l(scale q_h[rows[r]][n] . k_h[rows[r]][l]) for
 * r = 0, 1 -- the head-mean cross-attention map of batch row rows[r], summed over prompt tokens with the multiplicities w[r][l]
 * (fp32 [2][L]); q [B][N][heads*d] (row stride ldq, batch stride sQb), k likewise over L <= 128 keys; out fp32 [2][N], every
 * element written once, nothing accumulated.  Plain fp32 arithmetic in a fixed order; d any multiple of 8.  q, k 16-byte
 * aligned with strides that are multiples of 4 floats, w / out 4-byte aligned: IEF_EALIGN otherwise; a null pointer IEF_EINVAL;
 * L > 128, heads > 64, d % 8 != 0 or a non-positive size IEF_ESHAPE.  Nothing is launched by a refused call.
 * ief_masa_auto_classes: slots fp32 [c][2][256] (what c calls of the above wrote for the 16 x 16 level) -> class bits of a layer
 * of res x res tokens: img = (slot 0 + slot 1 + ... in slot order) / c, per row (img - min) / (max - min), token (y, x) reads
 * pixel (floor(16 y / res), floor(16 x / res)) and its bit is (value >= *thres); k_cls from row 0, q_cls from row 1, one
 * uint32 per 32 consecutive tokens (res * res / 32 words each; 1 <= res <= 256 with res * res a multiple of 32 and 1 <= c, else IEF_ESHAPE).  A row with
 * max == min (NaN in the reference) makes EVERY token of both rows background.  thres: device fp32; gate: optional device
 * int32, *gate == 0 writes nothing.  One workgroup. */
int ief_cross_token_mass_f32(const float* q, const float* k, const float* w, float* out, int row_ref, int row_cur, int heads,
                             int N, int L, int d, int ldq, int ldk, long long sQb, long long sKb, float scale, void* stream);
int ief_masa_auto_classes(const float* slots, int c, const float* thres, int res, unsigned* k_cls, unsigned* q_cls,
                          const int* gate, void* stream);
/* Prompt-to-Prompt's LocalBlend on the fused path (p2p/model/ptp_utils.py, LocalBlend.__call__), two launches (csrc/local_blend.hip).
 * ief_cross_blend_mass_f32: for one cross-attention module and the Bp prompt rows row0 .. row0 + Bp - 1 of its batch
 *   acc[i][n] += (1 / heads) sum_h ( sum_l v_i[l] softmax_l(scale q_h[row0 + i][n] . k_h[row0 + i][l])
 *                                   + sum_l u_i[l] softmax_l(scale q_h[row0][n] . k_h[row0][l]) )
 * -- the head-mean of the EDITED map P' = c1 (P_src M) + c2 P_i summed over the blend words, which is linear in the two plain
 * softmax rows: w fp32 [Bp][2][ldw] holds (u_i, v_i) per row, ldw >= L.  q [B][N][heads*d] (row stride ldq, batch stride sQb), k
 * likewise over L <= 128 keys; acc fp32 [Bp][N], every element read and written by one thread.  The source row's softmax is computed
 * once per (query, head).  Plain fp32 arithmetic in a fixed order; d any multiple of 8, Bp <= 8.  q, k 16-byte aligned with strides
 * that are multiples of 4 floats, w / acc 4-byte aligned: IEF_EALIGN otherwise; a null pointer IEF_EINVAL; L > 128, ldw < L, heads >
 * 64, d % 8 != 0, Bp outside [1, 8] or a non-positive size IEF_ESHAPE.  Nothing is launched by a refused call.
 * ief_local_blend_f32: acc fp32 [Bp][256] (16 x 16 images) and latents x fp32 [Bp][C][H][W], updated in place.  Per row: 3 x 3
 * max pool with -inf padding, the image maximum, value / maximum, > *thres (device fp32); an all-zero row gives 0 / 0, which is not
 * greater: its mask is empty.  mask_i = mask_0 OR mask_i; pixel (y, x) reads cell (floor(16 y / H), floor(16 x / W)); for i >= 1
 * x[i] = x[0] + m (x[i] - x[0]) with m in {0, 1}, every operation rounded; row 0 is not written.  H, W multiples of 16, Bp >= 2, C >= 1:
 * IEF_ESHAPE otherwise; a null pointer IEF_EINVAL; a pointer off the 4-byte grid IEF_EALIGN.  One workgroup per (row, channel). */
int ief_cross_blend_mass_f32(const float* q, const float* k, const float* w, float* acc, int row0, int Bp, int heads, int N, int L,
                             int ldw, int d, int ldq, int ldk, long long sQb, long long sKb, float scale, void* stream);
int ief_local_blend_f32(const float* acc, const float* thres, float* x, int Bp, int C, int H, int W, void* stream);
/* fp32 elements of IefAttnF32Params.ws that the launch needs after clamping key_splits; 0 when it would not split */
long long ief_attn_flash_ws_floats(int B, int heads, int N, int L, int d, int key_splits);
int ief_softmax_rows_f32(float* x, long long rows, int L, void* stream);
/* P'[w] = c1[w] * sum_v P_src[v] M[v][w] + c2[w] * P_tgt[w] in place on maps [B*heads][N][L], L <= 96; MT fp32
 * [slots][96][96] (M transposed, zero padded), coef fp32 [slots][2][96]; edit_src / edit_slot as IefCrossParams */
int ief_p2p_cross_edit_f32(float* P, const int* edit_src, const int* edit_slot, const float* MT, const float* coef, int B,
                           int heads, int N, int L, void* stream);
/* the same with P_src guaranteed to be the UNEDITED map of the source row whatever edit_src holds: an edited row that another row
 * names as its source is copied to keep (fp32, P's size, contents undefined afterwards) by a first launch and read from there; where
 * edit_src holds no such row nothing is copied.  keep NULL is ief_p2p_cross_edit_f32: the caller vouches that no source row other
 * than a row's own is edited by the launch. */
int ief_p2p_cross_edit_keep_f32(float* P, float* keep, const int* edit_src, const int* edit_slot, const float* MT, const float* coef,
                                int B, int heads, int N, int L, void* stream);
/* the four launches above (scores, softmax, edit, apply) as ONE: cross-attention over L <= 96 keys with the map edit applied to
 * maps that stay in registers; split-operand arithmetic (p->x3 is not consulted), d in {40, 64, 80, 160}; edit_src NULL: plain
 * attention (csrc/cross_p2p_x3.hip).  q_src (B entries, or NULL): the maps of row b read Q from batch row q_src[b], those of its
 * source row from q_src[edit_src[b]] -- Q may then have fewer batch rows than the launch (a CFG batch whose halves share one query
 * projection); K and V stay on rows b / edit_src[b]: k_src / v_src must be NULL (IEF_EINVAL).  The caller checks the entries. */
int ief_attn_cross_p2p_f32(const IefAttnF32Params* p, const int* edit_src, const int* edit_slot, const float* MT, const float* coef,
                           void* stream);
int ief_groupnorm_silu_f32(const float* x, const float* x2, int C1, int C2, float* out, const float* gamma, const float* beta,
                           int B, int HW, int groups, float eps, int silu, void* stream);
/* the same operator in three row-streaming launches (per-run channel statistics, Chan merge per group, apply); C1, C2
 * multiples of 4; ws: ief_groupnorm_f32_ws_floats(B, HW, C1 + C2) floats of scratch the caller owns until the stream passes */
long long ief_groupnorm_f32_ws_floats(int B, int HW, int C);
int ief_groupnorm_silu_f32_ws(const float* x, const float* x2, int C1, int C2, float* out, const float* gamma, const float* beta,
                              int B, int HW, int groups, float eps, int silu, float* ws, long long ws_floats, void* stream);
/* ABI 4 (added late in round 4; additive): the same operator with the (image, group) slab held in registers: ONE launch, one workgroup
 * of 1024 threads per (image, group), the input read once; out (fp32, nullable) and / or outp (operand planes hi / lo, lo plane
 * `plane` elements further; nullable).  Shapes: ief_groupnorm_reg_fits(C1, C2, HW, groups) != 0 (channels per group even and <= 512,
 * C1 even, HW x channels per group <= 40960).  The small-batch form (UNet batch 1 / 2: DDIM inversion, the null-text loop) of
 * /root/reference's GroupNorm + SiLU of ResnetBlock2D (pnp/model/register.py:149-158 runs them through torch). */
int ief_groupnorm_reg_fits(int C1, int C2, int HW, int groups);
int ief_groupnorm_silu_reg(const float* x, const float* x2, int C1, int C2, float* out, ief_half* outp, long long plane,
                           const float* gamma, const float* beta, int B, int HW, int groups, float eps, int silu, void* stream);
/* dx (, dx2) of the GroupNorm (+SiLU) above given dy; `add` (nullable) is summed into the result; row-streaming, five launches;
 * same shape rules as ief_groupnorm_silu_f32_ws, every pointer 16-byte aligned; ws: ief_groupnorm_bwd_f32_ws_floats floats */
long long ief_groupnorm_bwd_f32_ws_floats(int B, int HW, int C);
int ief_groupnorm_bwd_f32_ws(const float* x, const float* x2, int C1, int C2, const float* dy, const float* add, float* dx, float* dx2,
                             const float* gamma, const float* beta, int B, int HW, int groups, float eps, int silu, float* ws,
                             long long ws_floats, void* stream);
int ief_layernorm_f32(const float* x, float* out, const float* gamma, const float* beta, long long rows, int C, float eps,
                      void* stream);
/* ABI 4: the two normalisations as PRODUCERS of operand planes (hi = fp16(y), lo = fp16(y - hi), lo `plane` elements after hi;
 * csrc/gemm_x3p.hip consumes them): GroupNorm (+SiLU) in the three row-streaming launches (out: optional fp32 copy), LayerNorm
 * over rows of C <= 2560, C % 4 == 0 */
int ief_groupnorm_silu_x3p_ws(const float* x, const float* x2, int C1, int C2, float* out, ief_half* outp, long long plane,
                              const float* gamma, const float* beta, int B, int HW, int groups, float eps, int silu, float* ws,
                              long long ws_floats, void* stream);
/* one launch (a few workgroups per (image, group), each streaming the group's slab for the statistics): small tensors */
int ief_groupnorm_silu_x3p_small(const float* x, const float* x2, int C1, int C2, ief_half* outp, long long plane, const float* gamma,
                                 const float* beta, int B, int HW, int groups, float eps, int silu, void* stream);
int ief_layernorm_x3p(const float* x, ief_half* outp, long long plane, const float* gamma, const float* beta, long long rows, int C,
                      float eps, void* stream);
int ief_add_f32(const float* a, const float* b, float* out, long long n, void* stream);
int ief_silu_f32(const float* x, float* out, long long n, void* stream);
/* hidden * gelu(gate) on the interleaved FF1 layout ([8 hidden | 8 gate] groups): pre [rows][2 Ch] -> out [rows][Ch] */
int ief_geglu_il_f32(const float* pre, float* out, long long rows, int Ch, void* stream);
int ief_timestep_embedding_f32(const float* t, float* out, int B, int dim, void* stream);
int ief_gather_rows_f32(const float* in, float* out, const int* src, int B, long long row_elems, void* stream);
/* boundary convolutions with fp32 activations: fp32 NCHW latents <-> fp32 NHWC; w fp32 [3][3][Cin][Cout] / [Cout][3][3][C].
 * Operands accessed in 16-byte pieces must be 16-byte aligned (IEF_EALIGN otherwise, nothing launched): w and out of conv_in,
 * x and w of conv_out */
int ief_conv_in_f32act(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int Wd, int Cout,
                       void* stream);
int ief_conv_out_f32act(const float* x, const float* w, const float* bias, float* out, int B, int C, int H, int Wd, int Cout,
                        void* stream);
/* ief_conv_in_f32act that ALSO writes the operand planes of its result in the same launch (the split of the stored fp32 value, bit
 * for bit what ief_x3_split_act makes of it at scale 1): outp hi plane [B][H][W][Cout] fp16 (8-byte aligned), lo plane `plane`
 * elements further (plane % 4 == 0).  The fp32 output has the bits of ief_conv_in_f32act. */
int ief_conv_in_f32act_planes(const float* x, const float* w, const float* bias, float* out, ief_half* outp, long long plane, int B,
                              int Cin, int H, int Wd, int Cout, void* stream);
/* batch repeat, dst[r] = src[r % Bp] for r in [0, 2 Bp): up to IEF_REPEAT_MAX_JOBS tensors in ONE launch.  A job is `blocks`
 * blocks of `bytes` contiguous bytes each (`bytes` = the Bp rows of a tensor; operand planes [2][Bp]...: blocks = 2): block k is
 * read at src + k bytes and written at dst + 2 k bytes and again `bytes` further.  src / dst / bytes not multiples of 16:
 * IEF_EALIGN, nothing launched.  src and dst must not overlap. */
#define IEF_REPEAT_MAX_JOBS 4
typedef struct IefRepeatJob { const void* src; void* dst; long long bytes; int blocks; } IefRepeatJob;
int ief_repeat_batch(const IefRepeatJob* jobs, int njobs, void* stream);
/* uint8 image epilogue of latent2image (/root/reference/p2p/model/sd_utils.py:85-88): fp32 NCHW in [-1, 1] -> uint8 NHWC,
 * (x / 2 + 0.5).clamp(0, 1) * 255 truncated */
int ief_image_u8(const float* x, unsigned char* out, int B, int C, int H, int Wd, void* stream);

/* ------------------------------------------------------------------ ABI 4: split-operand contractions on PRE-SPLIT PLANES
 * (csrc/gemm_x3p.hip).  An activation tensor x [rows][C] of the f16x3 mode travels between kernels as two fp16 planes
 *     hi = fp16(x),  lo = fp16(x - hi)            (activation scale 1; weights: scale 2^8, ief_x3_split_weights)
 * the same 4 bytes per element as fp32: the PRODUCER of an activation (GroupNorm / LayerNorm apply, the GEGLU epilogue, the
 * attention epilogues, a GEMM epilogue) writes the planes, so the GEMM that consumes it stages BOTH operands by LDS-DMA
 * (global_load_lds) and its K loop holds no vector work at all: per 32-deep K tile three v_mfma_f32_16x16x32_f16 per fragment
 * pair (Al Bh + Ah Bl + Ah Bh, fp32 accumulate).  A plane pair is addressed as (hi pointer, element offset of the lo plane).
 * Same operator set as IefGemmParams (dense; 3x3 implicit GEMM with channel concat, nearest-2x, stride 2, fused 1x1 range),
 * replaces the same reference call sites: /root/reference/p2p/model/register.py:33-54 (linears),
 * /root/reference/pnp/model/register.py:139-175 (ResnetBlock2D convolutions + shortcut + temb / skip adds). */
typedef struct IefGemmX3pParams {
    const ief_half* A;  long long planeA;     /* dense: [M][lda] hi plane; conv: NHWC source 1 (C1 channels)            */
    const ief_half* A2; long long planeA2;    /* conv: NHWC source 2 of a channel concat (C2 channels) or NULL            */
    const ief_half* E1; long long planeE1;    /* conv: fused 1x1 range, sources sampled at the output pixel (CE1, CE2)     */
    const ief_half* E2; long long planeE2;
    const ief_half* W;  long long planeW;     /* [N][ldw] hi plane of the weight (scale w_scale)                           */
    float* Out;                               /* fp32 [M][ldo] or NULL                                                     */
    ief_half* OutP; long long planeO;         /* planes of the result, [M][ldp] (scale 1) or NULL; at least one of the two */
    const float* bias;                        /* [N] or NULL */
    const float* rowvec;                      /* [M / rows_per_batch][N] or NULL */
    const float* residual;                    /* fp32 [M][ldr] or NULL */
    int M, N, K;
    int lda, ldw, ldo, ldp, ldr;
    int conv, H, Wd, C1, C2, Ho, Wo, stride, ups, batch_images, pad_hi_only, CE1, CE2;
    int rows_per_batch;
    float out_scale;                          /* out = (acc * inv_scale + bias + rowvec + residual) * out_scale */
    float inv_scale;                          /* 1 / (activation scale * weight scale) */
    int tile;                                 /* 1: 128x160 (8 waves), 2: the same + 4 loader waves, 3: 128x80 (4 waves), 4: 256x160 (8 waves),
                                                 5: 64x160 (4 waves), 6: 128x64 (4 waves; widths that are multiples of 64 only), 7: 128x160 on 4 waves (two workgroups per CU), 8: 256x320 (8 waves of 64 x 160; the fewest staged bytes per FLOP: wide N only); 11 / 12: conv3x3_halo_x3p (256x80, 8 waves + 4 loader waves;
                                                 plain 3x3 stride 1 pad 1, rows of <= 64 pixels; 12: nearest-2x fused); 13: nearest-2x in PHASE form
                                                 (ups = 1, W = the planes of ief_x3_upsample_phase_weights, K = 4 (C1 + C2), source rows of <= 64 pixels:
                                                 four 2x2 convolutions of the low-resolution image, the phase in grid.z) */
    int splits;                               /* split-K over grid.y: fp32 slabs ws[splits][M][N] summed in slab order by a second launch */
    float* ws;
    int geglu;                                /* weight rows interleaved [8 hidden | 8 gate]: out [M][N / 2] = hidden * gelu(gate) */
    const void* zeros;                        /* >= 16 bytes of device zeros (source of out-of-range rows / padded taps) */
    /* LayerNorm folded into the NEXT linear (BasicTransformerBlock.norm1/2/3 -> to_q|k|v / to_q / ff.net[0]), in the (count, mean,
     * M2) form merged Chan-style (no E[x^2] - mean^2 cancellation):
     *   producer: rstat_out [M][slots][2] = (mean, M2) of each output row over every 80- (tile 6: 64-) column slice one wave owns;
     *             slots = N / slice width (ief_gemm_x3p_rstat_slots); needs an output (fp32 or planes) and no split-K / GEGLU;
     *   consumer: rstat_in = the producer's rstat_out over THIS launch's K (rstat_slots slices of rstat_cnt columns each); the
     *             launch runs on the planes of the RAW residual stream with W gamma as weight and computes
     *             rstd (acc - mean colsum[n]) + bias[n], colsum[n] = sum_k (W gamma)[n][k] as the planes hold it, bias = b + W beta.
     * cstat_out [ceil(M / BM)][N][2] = (mean, M2) of each output channel over the rows of an M tile (GroupNorm statistics from
     * the producer; M % BM == 0, no split-K). */
    float* rstat_out;
    float* cstat_out;
    const float* rstat_in;
    const float* colsum;
    int rstat_slots, rstat_cnt;
    float ln_eps;
    /* dense, K-CONCATENATED A operand (K1 > 0): out = [A | A2] . W^T -- K columns below K1 are read from A / planeA / lda, the
     * other K - K1 from A2 / planeA2 / lda2; W stays one [N][K] tensor and the K tiles run in the order of a plain launch over the
     * concatenated rows (same bits).  K1 and K - K1 multiples of 32 (IEF_ESHAPE), A2 16-byte aligned with lda2 and planeA2
     * multiples of 8 (IEF_EALIGN); tiles 1, 3, 4 and 6 only, not with conv, geglu or rstat_in (IEF_EINVAL).  Split-K ranges may
     * straddle K1. */
    int K1, lda2;
    /* w_tiled != 0: W points at the planes in the TILED order of ief_x3_tile_weights (the same halves, other addresses: every
     * result keeps its bits).  planeW must be N K (tile 13: 4 N K, each phase matrix tiled on its own; IEF_ESHAPE) and W 256-byte
     * aligned (IEF_EALIGN); ldw is not used beyond its checks. */
    int w_tiled;
} IefGemmX3pParams;
int ief_gemm_x3p(const IefGemmX3pParams* p, void* stream);
/* Weight planes [2][N][K] (row-major, from any producer: ief_x3_split_weights, one phase matrix of ief_x3_upsample_phase_weights,
 * the planes of a folded pair) -> the same halves in the order the LDS-DMA pieces of the planes kernels fetch whole 128-byte lines
 * from: with nk = K / 32, the half at plane pl, row n, column 32 kt + kk goes to half index
 *     pl N K + ((((n >> 2) nk + kt) 4 + (n & 3)) 32 + kk)
 * -- four consecutive rows x one 32-deep K tile are 256 contiguous, 256-byte aligned bytes, the next K tile of the same four rows
 * follows.  A piece's 16 lanes that fetch rows 4a .. 4a + 3 then read two whole lines instead of four half lines.  A plain copy
 * in 16-byte vectors.  N % 4 or K % 32: IEF_ESHAPE; planes_rowmajor not 16-byte or tiled not 256-byte aligned: IEF_EALIGN. */
int ief_x3_tile_weights(const ief_half* planes_rowmajor, ief_half* tiled, int N, int K, void* stream);
/* Two linears with nothing non-linear between them, folded into one (the tail of a Transformer2DModel: FeedForward.net[2] followed
 * by proj_out):  (g W2^T + b2 + h) Wp^T + bp = [g | h] [Wp W2 | Wp]^T + (Wp b2 + bp).  wp fp32 [C][C], w2 fp32 [C][K], b2 / bp fp32
 * [C] or NULL -> wcat fp32 [C][K + C] = [Wp W2 | Wp] and bcat fp32 [C] = Wp b2 + bp; every sum is accumulated in fp64 in
 * increasing index order and rounded once to fp32. */
int ief_x3_fold_linear_pair(const float* wp, const float* w2, const float* b2, const float* bp, float* wcat, float* bcat, int C, int K,
                            void* stream);
/* Upsample2D's weight in PHASE form for tile 13: w fp32 [Cout][3][3][C] (16-byte aligned, C % 4 == 0) -> fp16 planes
 * [2][4 phases (py, px)][Cout][4 taps (sy, sx)][C] at `scale`.  Output pixel (2y + py, 2x + px) of nearest-2x + 3x3 / pad 1 is a 2x2
 * convolution of the low-resolution image over the taps ty = py + sy, tx = px + sx (3x3 indexing: tap t = low-res row y + t - 1);
 * a phase tap is the fp32 sum, in increasing (ky, kx) order, of the original weights that read that low-res pixel
 * (p = 0: t 0 <- k {0}, t 1 <- k {1, 2}; p = 1: t 1 <- k {0, 1}, t 2 <- k {2}), split as ief_x3_split_weights does. */
int ief_x3_upsample_phase_weights(const float* w, void* planes, int Cout, int C, float scale, void* stream);
int ief_gemm_x3p_tile_bm(int tile);
int ief_gemm_x3p_tile_bn(int tile);
/* columns one wave owns in a tile (the width of a row-statistics slice): 80, tile 6: 64 */
int ief_gemm_x3p_tile_wn(int tile);
/* fp32 x [rows][ldx] -> planes hi / lo [rows][ldp] (lo plane `plane` elements after hi); C % 4 == 0, 16-byte aligned rows */
int ief_x3_split_act(const float* x, ief_half* planes, long long plane, long long rows, int C, int ldx, int ldp, float scale,
                     void* stream);

/* ------------------------------------------------------------------ activation gradients of the fp32-storage modes
 * (csrc/backward_f32.hip): the reverse pass of null-text inversion / Pix2Pix-zero at the reference's precision
 * (/root/reference/p2p/inversion/nti.py:15-33 and /root/reference/pix2pix-zero/model/sd_utils.py:160-174 run torch autograd in
 * fp32).  Same formulas as the fp16 entry points below; attention gradients are assembled by the host from ief_gemm_f32
 * products on MATERIALISED fp32 maps plus ief_softmax_bwd_rows_f32 / ief_transpose_batched_f32. */
int ief_groupnorm_bwd_f32(const float* x, const float* x2, int C1, int C2, const float* dy, const float* add, float* dx, float* dx2,
                          const float* gamma, const float* beta, int B, int HW, int groups, float eps, int silu, void* stream);
int ief_layernorm_bwd_f32(const float* x, const float* dy, const float* add, float* dx, const float* gamma, long long rows, int C,
                          float eps, void* stream);
int ief_geglu_il_bwd_f32(const float* pre, const float* dy, float* dpre, long long rows, int Ch, void* stream);
int ief_zero_insert2x_f32(const float* in, float* out, int B, int H, int W, int C, void* stream);   /* [B,H,W,C] -> [B,2H,2W,C] */
int ief_pool2x2_sum_f32(const float* in, float* out, int B, int H, int W, int C, void* stream);     /* [B,2H,2W,C] -> [B,H,W,C] */
int ief_conv_out_bwd_f32w(const float* d_eps, const float* w, float* dh, int B, int C, int H, int W, int Cout, void* stream);
/* in place on dP [rows][L]: dS = scale * P o (dP - sum_j dP_j P_j) */
int ief_softmax_bwd_rows_f32(const float* P, float* dP, long long rows, int L, float scale, void* stream);
int ief_transpose_batched_f32(const float* in, float* out, int R, int N, int L, void* stream);        /* [R][N][L] -> [R][L][N] */
/* Pix2Pix-zero map objective on materialised maps: dP = gcoef (P - ref); loss[block] = loss_coef * sum (P - ref)^2 over the
 * block's rows (ief_map_loss_rows_blocks(rows) blocks, fixed order) */
int ief_map_loss_rows_blocks(long long rows);
int ief_map_loss_rows_f32(const float* P, const float* ref, float* dP, float* loss, long long rows, int L, float gcoef,
                          float loss_coef, void* stream);
/* torch.optim.Adam step with an fp32 gradient (g = grad * stats[1]); hyper = {lr, beta1, beta2, eps}; step[0] += 1 */
int ief_nti_adam_f32g(float* param, float* m, float* v, const float* grad, const float* stats, const float* hyper, int* step, int n,
                      void* stream);

/* ------------------------------------------------------------------ null-text inversion: activation gradients
 * The reference optimises the unconditional embedding with torch autograd through the whole UNet
 * (/root/reference/p2p/inversion/nti.py:15-33: `uncond_embeddings.requires_grad`, `loss.backward()`,
 * `optimizer.step()`), weights frozen.  Only gradients w.r.t. ACTIVATIONS are therefore needed:
 *   - linear / conv3x3 data gradients are ief_gemm_f16 / ief_conv3x3_f16 on transposed (and tap-flipped) weights;
 *   - the entry points below are the backward of everything else on the path.
 * Gradients are fp16 and carry a global scale chosen by ief_nti_loss_grad_f32 (undone in ief_nti_adam_f32).
 */
typedef struct IefAttnBwdParams {
    const ief_half* Q; const ief_half* K; const ief_half* V; const ief_half* dO;
    const float* lse;     /* [B][heads][N] from ief_attn_flash_f16 */
    const float* delta;   /* [B][heads][N] from ief_attn_bwd_delta_f32 */
    ief_half* dQ; ief_half* dK; ief_half* dV;
    int B, heads, N, L, d;
    int ldq, ldk, ldv, ldo, lddq, lddk, lddv;
    float scale;
    float ds_mul;         /* dS is multiplied by this before its fp16 rounding (undone in fp32); > 0 */
    /* dK/dV with few keys (cross-attention: 77) own too few workgroups: kv_splits > 1 cuts the query range into that many
     * slices, each writing fp32 partials to ws (>= 2 * kv_splits * B * L * heads * d floats), summed in a fixed order. */
    int kv_splits;
    float* ws;
} IefAttnBwdParams;
/* delta[b][h][n] = sum_d dO * O  (the softmax-backward row term) */
int ief_attn_bwd_delta_f32(const ief_half* O, const ief_half* dO, float* delta, int B, int heads, int N, int d,
                           int ldo, int lddo, void* stream);
/* what: 1 = dQ, 2 = dK and dV, 3 = all.  d in {32,40,64,80,160}; any N, L >= 1. */
int ief_attn_bwd_f16(const IefAttnBwdParams* p, int what, void* stream);
/* ---- the same gradients in the split-operand ("f16x3") mode: fp32 q / k / v / dO in, fp32 dQ / dK / dV out, P and dS recomputed per
 * tile from the forward's lse (IefAttnF32Params.lse) and never written to HBM; every product on hi / lo fp16 halves (three MFMAs);
 * csrc/attention_bwd_x3.hip.  Rows of batch b start at b * rows * ld (as IefAttnBwdParams).  d in {40, 64}.  Replaces, on the
 * fp32-storage reverse pass, the materialised maps of /root/reference/p2p/model/register.py:43-51's backward. */
typedef struct IefAttnBwdF32Params {
    const float* Q; const float* K; const float* V; const float* dO;
    const float* lse;     /* [B][heads][N], log2 units */
    const float* delta;   /* [B][heads][N] from ief_attn_bwd_delta_f32in */
    float* dQ; float* dK; float* dV;
    int B, heads, N, L, d;
    int ldq, ldk, ldv, ldo, lddq, lddk, lddv;
    float scale;
    float ds_mul;         /* dS is multiplied by this before its hi / lo split (undone in fp32; |dS ds_mul| > 65504 gives non-finite gradients); > 0 */
} IefAttnBwdF32Params;
int ief_attn_bwd_delta_f32in(const float* O, const float* dO, float* delta, int B, int heads, int N, int d, int ldo, int lddo,
                             void* stream);
/* what: 1 = dQ, 2 = dK and dV, 3 = all */
int ief_attn_bwd_x3(const IefAttnBwdF32Params* p, int what, void* stream);
/* Pix2Pix-zero cross-attention guidance (/root/reference/pix2pix-zero/model/sd_utils.py:166-173): for one cross-attention
 * module, loss = mean over (batch, head) of sum_{n,j} (P - ref)^2 with P = softmax(scale Q K^T), and its gradient w.r.t.
 * Q:  dQ (+)= gcoef * scale * dS K,  dS = P * (e - sum_j e_j P_j),  e = P - ref.  The caller passes
 * gcoef = 2 / (B heads) * gradient scale.  ref: fp16 [B*heads][N][L] contiguous (what ief_attn_probs_f16 wrote during
 * the reference pass); loss (optional): one partial per workgroup, [B][heads][ief_map_loss_blocks(N, d)] floats, each
 * already multiplied by loss_coef; L <= 96; d in {32,40,64,80,160}. */
typedef struct IefMapLossParams {
    const ief_half* Q; const ief_half* K; const ief_half* ref;
    ief_half* dQ;
    float* loss;
    int B, heads, N, L, d;
    int ldq, ldk, lddq;
    float scale, gcoef, loss_coef;
    int accumulate;       /* 1: add to the gradient already in dQ; 0: overwrite */
} IefMapLossParams;
int ief_attn_map_loss_bwd_f16(const IefMapLossParams* p, void* stream);
/* workgroups per (batch, head) of the kernel above = loss partials per (batch, head) */
int ief_map_loss_blocks(int N, int d);
/* The same guidance on the fp32-storage reverse pass, fused with the value path of the attention layer: ONE launch per
 * cross-attention module gives the whole gradient w.r.t. its queries and the objective's value (csrc/cross_map_grad_f32.hip).
 * For batch row b, head h, query n, with K / V of (b, h) held in LDS as fp32:
 *     P    = softmax_j(scale q.K_j)
 *     dP_j = dO.V_j + gcoef (P_j - ref_j)          value path + objective (gcoef = 2 / (B heads) * gradient scale)
 *     dS_j = P_j (dP_j - sum_i dP_i P_i)
 *     dQ   = scale sum_j dS_j K_j                  OVERWRITES dQ: the sum of both paths, there is no accumulate flag
 *     loss[b][h][w] = loss_coef sum (P - ref)^2 over the queries of workgroup w, summed in a fixed order
 * Plain fp32 FMAs (no MFMA, no operand splitting); no map and no score is written to global memory.  Q, dO, dQ: fp32 [B][N][heads*d]
 * with row strides ldq / ldo / lddq; K, V: fp32 [B][L][heads*d] with row strides ldk / ldv (column slices of a wider buffer are
 * fine); rows of batch b start at b * rows * ld.  ref: contiguous fp32 [B*heads][N][L].  loss (optional): [B][heads]
 * [ief_cross_map_grad_blocks(N, d)] floats, nothing else is written.  d in {32, 40, 64, 80, 160}; 1 <= L <=
 * IEF_CROSS_MAP_GRAD_MAX_L, the largest L whose LDS image (L (8 d + 8 * 256 / G) + 16 bytes, G = 2, 2, 4, 4, 8 lanes per query)
 * fits the 160 KiB of a CU at d = 160; B, heads <= 65535.  A null Q / K / V / dO / ref / dQ: IEF_EINVAL; any other L, d, a
 * non-positive size or heads * d beyond a row stride: IEF_ESHAPE; Q / K / V / dO / dQ off a 16-byte boundary, a row stride that is
 * no multiple of 4 floats, ref / loss off a 4-byte boundary: IEF_EALIGN.  Nothing is launched by a refused call.  The arguments
 * are passed flat, as ief_cross_blend_mass_f32's are: the entry point adds no parameter struct to the ABI. */
#define IEF_CROSS_MAP_GRAD_MAX_L 106
int ief_attn_cross_map_grad_f32(const float* Q, const float* K, const float* V, const float* dO, const float* ref, float* dQ,
                                float* loss, int B, int heads, int N, int L, int d, int ldq, int ldk, int ldv, int ldo, int lddq,
                                float scale, float gcoef, float loss_coef, void* stream);
/* workgroups per (batch, head) of the kernel above = loss partials per (batch, head); 0 for a head dim it does not take */
int ief_cross_map_grad_blocks(int N, int d);
/* The COMPLETE backward of a short-key cross-attention on the fp32-storage reverse pass, no map in global memory
 * (csrc/cross_bwd_f32.hip): what null-text inversion optimises reaches the context through K and V of these modules
 * (/root/reference/p2p/inversion/nti.py:15-33).  For batch row b, head h, with K / V of (b, h) held in LDS as fp32:
 *     P    = softmax_j(scale q.K_j)
 *     dP_j = dO.V_j
 *     dS_j = P_j (dP_j - sum_i dP_i P_i)
 *     dQ_n = scale sum_j dS_nj K_j                 OVERWRITES dQ; dQ == NULL: not computed (the K walk is skipped)
 *     dK_j = scale sum_n dS_nj Q_n                 OVERWRITES dK
 *     dV_j =       sum_n P_nj  dO_n                OVERWRITES dV
 * Plain fp32 FMAs (no MFMA, no operand splitting).  Two launches: the main kernel reduces the queries of each workgroup into one
 * [L][d] partial per matrix in `scratch` ([B][heads][ief_cross_bwd_blocks(N, d)][2][L][d] floats =
 * ief_cross_bwd_scratch_floats(...), the caller's, 16-byte aligned, contents irrelevant before and after), a reducer adds the
 * partials in ascending block order: no atomics, two calls on the same operands give the same bits, and row b of every result
 * depends on row b of the operands only, whatever B is.  Q, dO, dQ: fp32 [B][N][heads*d] with row strides ldq / ldo / lddq; K, V, dK,
 * dV: fp32 [B][L][heads*d] with row strides ldk / ldv / lddk / lddv (column slices of wider buffers are fine); rows of batch b
 * start at b * rows * ld.  d in {32, 40, 64, 80, 160}; 1 <= L <= IEF_CROSS_BWD_MAX_L, the largest L whose LDS image
 * (8 L d + 8 L QB + 8 QB d bytes: K and V, the two per-query columns, the q and dO rows of the QB = 128, 128, 64, 64, 32 queries of
 * a workgroup) fits the 160 KiB of a CU at every head dim -- d = 160 sets it, at exactly 160 KiB; B, heads <= 65535.  A null
 * Q / K / V / dO / dK / dV / scratch: IEF_EINVAL; any other L, d, a non-positive size or heads * d beyond a row stride: IEF_ESHAPE; a
 * pointer off a 16-byte boundary or a row stride that is no multiple of 4 floats: IEF_EALIGN (lddq counts only with dQ).  Nothing
 * is launched by a refused call.  Safe under stream capture (no allocation, no synchronisation). */
#define IEF_CROSS_BWD_MAX_L 80
int ief_attn_cross_bwd_f32(const float* Q, const float* K, const float* V, const float* dO, float* dQ, float* dK, float* dV,
                           float* scratch, int B, int heads, int N, int L, int d, int ldq, int ldk, int ldv, int ldo, int lddq,
                           int lddk, int lddv, float scale, void* stream);
/* workgroups per (batch, head) of the main kernel above = partials per (batch, head); 0 for a head dim it does not take */
int ief_cross_bwd_blocks(int N, int d);
/* floats of `scratch` for ief_attn_cross_bwd_f32: B * heads * blocks * 2 * L * d; 0 for an unsupported shape.  (long long, the
 * header's one 64-bit return type: every entry point is declared over the types the derived binding knows) */
long long ief_cross_bwd_scratch_floats(int B, int heads, int N, int L, int d);
/* y[i] += a * x[i] (fp32): the plain SGD step on the UNet input (sd_utils.py:160,174) */
int ief_axpy_f32(float* y, const float* x, float a, long long n, void* stream);
/* GroupNorm(+SiLU) whose statistics were left by the kernels that produced x (and x2): cstat1 / cstat2 are those launches'
 * IefGemmParams.cstat_out, bm1 / bm2 their M-tile heights (HW % bm == 0: no tile straddles two images).  One small
 * launch folds the per-tile partials into (mean, rstd) per (batch, group) in `stats` (B * groups * 2 floats), one applies:
 * the statistics pass over x is gone.  replaces the same reference lines as ief_groupnorm_silu_f16. */
int ief_groupnorm_cstat_f16(const ief_half* x, const ief_half* x2, int C1, int C2, ief_half* out, const float* gamma,
                            const float* beta, const float* cstat1, int bm1, const float* cstat2, int bm2, float* stats,
                            int B, int HW, int groups, float eps, int apply_silu, void* stream);
/* BM of a tile id (see ief_gemm_tile_bn) */
int ief_gemm_tile_bm(int tile_hint);
/* GroupNorm(+SiLU) backward w.r.t. the input: x (+x2 channel concat) is the forward INPUT, dy [B][HW][C1+C2] the gradient
 * of the output, `add` (optional, same shape as dy) is added to the result; dx [B][HW][C1], dx2 [B][HW][C2].
 * stats: (mean, rstd) [B][groups][2] saved by the forward, or NULL (recomputed); partial: scratch of
 * >= B * ief_gn_splits(HW) * groups * 2 floats, or NULL (forces the one-workgroup-per-group kernel). */
int ief_groupnorm_bwd_f16(const ief_half* x, const ief_half* x2, int C1, int C2, const ief_half* dy, const ief_half* add,
                          ief_half* dx, ief_half* dx2, const float* gamma, const float* beta, const float* stats,
                          float* partial, int B, int HW, int groups, float eps, int apply_silu, void* stream);
/* LayerNorm backward w.r.t. the input (+ optional `add`) */
int ief_layernorm_bwd_f16(const ief_half* x, const ief_half* dy, const ief_half* add, ief_half* dx, const float* gamma,
                          int rows, int C, float eps, void* stream);
/* GEGLU on the interleaved projection layout of the fused FF1 GEMM ([8 hidden | 8 gate] column groups):
 * forward out[r][8g+e] = pre[r][16g+e] * gelu(pre[r][16g+8+e]) and its backward w.r.t. pre */
int ief_geglu_il_f16(const ief_half* pre, ief_half* out, int rows, int Ch, void* stream);
int ief_geglu_il_bwd_f16(const ief_half* pre, const ief_half* dy, ief_half* dpre, int rows, int Ch, void* stream);
/* stride-2 conv data gradient = stride-1 conv of the zero-inserted gradient: out[b][2i][2j] = in[b][i][j], else 0 */
int ief_zero_insert2x_f16(const ief_half* in, ief_half* out, int B, int H, int W, int C, void* stream);
/* nearest-2x upsample backward: out[b][i][j] = sum of the 2x2 block of in [B][2H][2W][C] */
int ief_pool2x2_sum_f16(const ief_half* in, ief_half* out, int B, int H, int W, int C, void* stream);
/* conv_out data gradient: d_eps fp32 NCHW [B][Cout][H][W], w fp16 [Cout][3][3][C] -> dh fp16 NHWC [B][H][W][C] */
int ief_conv_out_bwd_f32(const float* d_eps, const ief_half* w, ief_half* dh, int B, int C, int H, int W, int Cout,
                         void* stream);
/* NTI objective (nti.py:24-27): rec = DDIM step of x with eps = eps_u + g (eps_c - eps_u); loss = mean((rec - target)^2).
 * coef: DEVICE fp32 {a_from, a_to, g} as for ief_cfg_ddim_step_f32.  Writes stats[0] = loss, stats[1] = factor, and the NORMALISED gradient
 * d_eps = (rec - target) / max|rec - target| * grad_scale, with d loss / d eps_u = d_eps * factor.  n <= 2^20. */
int ief_nti_loss_grad_f32(const float* eps_u, const float* eps_c, const float* x, const float* target, const float* coef,
                          float* d_eps, float* stats, int n, float grad_scale, void* stream);
/* torch.optim.Adam step (nti.py:17,29-30) on fp32 param [n]: g = grad16 * stats[1]; state m, v, DEVICE int step count
 * (incremented here), hyper: DEVICE fp32 {lr, beta1, beta2, eps}; also writes the fp16 copy the next forward reads. */
int ief_nti_adam_f32(float* param, float* m, float* v, const ief_half* grad16, const float* stats, const float* hyper,
                     int* step, ief_half* param16, int n, void* stream);
/* K images at ONE DDIM timestep through the same three steps (`nti.BatchedNullTextOptimizer`): coef, hyper and the step counter
 * are shared, everything else is [K][n] with n elements PER IMAGE.
 * ief_nti_loss_grad_batched_f32: one workgroup per image runs the body of ief_nti_loss_grad_f32 on image k's slice and writes
 * stats[k][0..1]; image k's d_eps and stats are bit-identical to the single-image call on that slice.  n <= 2^20, K >= 1.
 * ief_nti_adam_batched_f32 (fp16 gradient, also writes param16) / ief_nti_adam_batched_f32g (fp32 gradient): image k's Adam
 * step with g = grad[k] * stats[k][1]; active int32 [K]: an image with active[k] == 0 is not touched (param, m, v, param16
 * unwritten).  step[0] += 1 once per call.  A null pointer is IEF_EINVAL, a non-positive size or K > 65535 IEF_ESHAPE, a pointer
 * that is not aligned to its element IEF_EALIGN; nothing is launched by a refused call. */
int ief_nti_loss_grad_batched_f32(const float* eps_u, const float* eps_c, const float* x, const float* target, const float* coef,
                                  float* d_eps, float* stats, int n, int K, float grad_scale, void* stream);
int ief_nti_adam_batched_f32(float* param, float* m, float* v, const ief_half* grad16, const float* stats, const int* active,
                             const float* hyper, int* step, ief_half* param16, int n, int K, void* stream);
int ief_nti_adam_batched_f32g(float* param, float* m, float* v, const float* grad, const float* stats, const int* active,
                              const float* hyper, int* step, int n, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IEF_HIP_H */
