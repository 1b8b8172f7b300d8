// The RoPE rotation, its position clamp and the fold of the QKV GEMM's split-K slabs: the ONE definition behind rope_kv_write (rowops.hip, scalar
// and vectorised bodies), the fused decode launch (decode_attn.hip) and the own-token pass (decode_own.hip). The models rely on these agreeing bit
// for bit: the fused launch and the three-launch path append the same K / V^T bits, and the own-token pass rotates q exactly as rope_kv_write would.
#pragma once
#include "common.h"

// a position outside the cos / sin tables reads their first / last row
__device__ __forceinline__ int rope_clamp_pos(int pos, int n_pos) { return pos < 0 ? 0 : (pos >= n_pos ? n_pos - 1 : pos); }

// (x1, x2) = elements (i, i + D/2) of a head, (c, s) = the fp32 table entries of (position, i). The caller handles mode 0 (no rotation) itself.
//   mode 2  HF rotate_half in bf16 arithmetic: tables, products and sum each rounded to bf16. The results are bf16-exact.
//   else    pi0 apply_rope (paligemma_with_expert.py:34-57) in fp32. The results are UNROUNDED: rope_kv_write and the fused launch round them
//           once at their f2bf store; the own-token pass goes on computing with them and rounds them itself (bfround).
// No contraction anywhere in here: torch rounds each product, an FMA would not.
__device__ __forceinline__ void rope_rotate(int mode, float x1, float x2, float c, float s, float& o1, float& o2) {
#pragma clang fp contract(off)
    if (mode == 2) {
        c = bfround(c); s = bfround(s);
        o1 = bfround(bfround(x1 * c) + bfround(-x2 * s));
        o2 = bfround(bfround(x2 * c) + bfround(x1 * s));
    } else {
        o1 = x1 * c - x2 * s;
        o2 = x2 * c + x1 * s;
    }
}

// One q / k / v value from the fp32 slabs of the weight-streaming QKV GEMM: bf16(((0 + slab 0) + slab 1 + ...) + bias), what the projection's
// bf16 output would have been. slab(s) yields the value's entry of slab s, bias() its bias (called only when has_bias).
// HELD: the caller holds slabs 0..HELD-1 already (registers) and yields +0 for an absent one; they are added behind a select instead of a loop
// exit. The sum is never -0 (it starts from +0), so adding +0 is exact and both forms give the same bits.
template <int HELD = 0, class Slab, class Bias>
__device__ __forceinline__ float qkv_fold(int n_splits, Slab slab, bool has_bias, Bias bias) {
    float v = 0.f;
#pragma unroll
    for (int s = 0; s < HELD; ++s) v += s < n_splits ? slab(s) : 0.f;
    for (int s = HELD; s < n_splits; ++s) v += slab(s);
    if (has_bias) v += bias();
    return bfround(v);
}
