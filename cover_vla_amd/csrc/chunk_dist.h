// The distance of two action chunks that coherence.hip (candidate rows against reference chunks) and diverse.hip (the rows of a group
// against each other) share: the step-weighted sum over the steps of the squared, per-dim scaled differences of the six translation /
// rotation values, plus a penalty where the gripper classes differ. Stated once, so the two files cannot drift apart: both results are
// compared with numpy restatements as bit patterns. Contraction is off from here to the end of the including file (hipcc would otherwise
// fuse s * s + e into one v_fma_f32). The values it is given come from chunk_rows.h's chunk_src (the row source and the token rule);
// smooth.hip takes chunk_finite and chunk_load_scale from here and keeps a pair weight of its own.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

__device__ __forceinline__ bool chunk_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// sc[0..5] = dim_scale -> false when an entry is negative or not finite: the launch then has no distance at all
__device__ __forceinline__ bool chunk_load_scale(const float* dim_scale, float* sc) {
    bool usable = true;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        sc[d] = dim_scale[d];
        if (!(sc[d] >= 0.0f) || !chunk_finite(sc[d])) usable = false;
    }
    return usable;
}

// D of one pair of chunks: x(t, d) / y(t, d) give the value of step t, dim d; a value is read only where it enters the sum
template <typename FX, typename FY>
__device__ __forceinline__ float chunk_pair_dist_of(FX x, FY y, int T, const float* sc, const float* step_weight, float penalty) {
    float D = 0.0f;
    for (int t = 0; t < T; ++t) {
        float e = 0.0f;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            if (sc[d] != 0.0f) {   // a dim of scale 0 is not read into the sum: a NaN there is invisible
                const float diff = x(t, d) - y(t, d);
                const float s = diff * sc[d];
                const float sq = s * s;
                e = e + sq;
            }
        }
        if (penalty != 0.0f && ((x(t, 6) >= 0.5f) != (y(t, 6) >= 0.5f))) e = e + penalty;
        const float p = step_weight[t] * e;
        D = D + p;
    }
    return D;
}

// the same where x / y point at the chunks' [T][7] values (step stride 7)
__device__ __forceinline__ float chunk_pair_dist(const float* x, const float* y, int T, const float* sc, const float* step_weight,
                                                 float penalty) {
    return chunk_pair_dist_of([x](int t, int d) { return x[7 * t + d]; }, [y](int t, int d) { return y[7 * t + d]; }, T, sc, step_weight,
                              penalty);
}
