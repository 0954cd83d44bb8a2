// What the short-key fp32 cross-attention kernels share (csrc/cross_map_grad_f32.hip, csrc/cross_bwd_f32.hip): the split of a head
// dim over the G adjacent lanes that own one query, and the sum over those lanes.
#pragma once
#include "ief_common.h"
#include "ief_params.h"

// DC channels per lane: G = D / DC = 2, 2, 4, 4, 8 lanes per query and QB = 256 / G = 128, 128, 64, 64, 32 queries per workgroup
// for D = 32, 40, 64, 80, 160
static constexpr int cmg_dc(int d) { return d % 20 == 0 ? 20 : 16; }
static constexpr int cmg_qb(int d) { return 256 / (d / cmg_dc(d)); }
static bool cmg_head_dim(int d) { return d == 32 || d == 40 || d == 64 || d == 80 || d == 160; }

// sum over the G adjacent lanes of a query, on the data-parallel primitives (no LDS round trip): lane ^ 1, lane ^ 2 inside a quad,
// then the mirror image of the 8-lane half row -- the four lanes of a quad hold one value by then, so lane 7 - i stands for lane i ^ 4.
// Every lane of the group ends with the same bits: each step adds the same two numbers on both sides.
template <int CTRL>
__device__ __forceinline__ float dpp_move(float a) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), CTRL, 0xF, 0xF, true));
}
template <int G>
__device__ __forceinline__ float group_sum(float a) {
    if (G >= 2) a += dpp_move<0xB1>(a);               // quad_perm [1, 0, 3, 2]
    if (G >= 4) a += dpp_move<0x4E>(a);               // quad_perm [2, 3, 0, 1]
    if (G >= 8) a += dpp_move<0x141>(a);              // row_half_mirror
    return a;
}
