// The candidate rows of one prompt group, as every kernel over them reads them (augment.hip, proposal_prior.hip, refine.hip, smooth.hip,
// coherence.hip, diverse.hip): where element (row, step, dim) lies, what it is worth (aug_value: floats pass through, tokens go through
// the bin centres), the walk that stages rows in LDS, the walk that gathers rows to an output, and what a launch function checks of the
// row description. Stated once, so the families cannot drift apart: every result is compared with a numpy restatement as a bit pattern.
// Contraction is off from here to the end of the including file.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

// the rows of one group: T = int64_t (action tokens) or float (action chunks)
template <typename T>
struct chunk_src {
    const T* in;                    // the group's first row
    long long n_stride, t_stride;   // row and step stride, in elements
    const float* centers;           // tokens: [n_centers] bin centres
    int n_centers, tok_vocab;

    __device__ __forceinline__ T raw(int i, int t, int d) const { return in[(long long)i * n_stride + (long long)t * t_stride + d]; }
    __device__ __forceinline__ float value(int i, int t, int d) const;
};

// what a raw input element is worth: floats pass through, tokens go through the bin centres
template <typename T>
__device__ __forceinline__ float aug_value(const chunk_src<T>& s, float raw) { return raw; }
template <typename T>
__device__ __forceinline__ float aug_value(const chunk_src<T>& s, int64_t token) {
    long long b = (long long)s.tok_vocab - token - 1;   // tokens_to_histories_k's rule
    b = b < 0 ? 0 : (b > s.n_centers - 1 ? s.n_centers - 1 : b);
    return s.centers[b];
}
template <typename T>
__device__ __forceinline__ float chunk_src<T>::value(int i, int t, int d) const { return aug_value(*this, raw(i, t, d)); }

// the source of any family's argument struct: the group whose first row is row `first` of the launch; t_stride is the kernel's parameter
// (7 in the token form, where the struct's field is not read)
template <typename T, typename A>
__device__ __forceinline__ chunk_src<T> chunk_src_of(const A& a, long long t_stride, long long first) {
    return {(const T*)a.src + first * a.n_stride, a.n_stride, t_stride, a.centers, a.n_centers, a.tok_vocab};
}

// `rows` rows from row r0 on, w7 = 7 * steps values each, -> dst[r * stride + 7 t + d], walked by the whole block; the caller synchronises
template <typename T>
__device__ __forceinline__ void chunk_stage_rows(const chunk_src<T>& s, int r0, int rows, int w7, float* dst, int stride) {
    for (int i = threadIdx.x; i < rows * w7; i += blockDim.x) {
        const int r = i / w7, c = i - r * w7, t = c / 7, d = c - t * 7;
        dst[r * stride + c] = s.value(r0 + r, t, d);
    }
}

// output row r < m (contiguous, w7 elements) = input row row_of(r), its first 7 dims verbatim, walked by the whole block
template <typename T, typename F>
__device__ __forceinline__ void chunk_gather_rows(const chunk_src<T>& s, int m, int w7, T* out, F row_of) {
    for (int i = threadIdx.x; i < m * w7; i += blockDim.x) {
        const int r = i / w7, c = i - r * w7, t = c / 7, d = c - t * 7;
        out[i] = s.raw(row_of(r), t, d);
    }
}

// ---- the launch side (host)
// what the token form of any family needs beside its own checks
template <typename A>
static inline bool token_form_ok(const A* a) { return !(a->n_stride < 7 * a->h || !a->centers || a->n_centers < 1); }

// lo <= v (lo < v) with v no larger than the largest finite fp32; a NaN fails both
static inline bool f32_ge(float v, float lo) { return v >= lo && v <= 3.402823466e+38f; }
static inline bool f32_gt(float v, float lo) { return v > lo && v <= 3.402823466e+38f; }

// the rows of one LDS tile of smooth.hip / coherence.hip: what `budget` floats hold at `stride` floats per row, in whole waves of lanes
// (64 .. max_tile), and no more than `count` rows need
static inline int chunk_tile_rows(int stride, int count, int budget, int max_tile) {
    int rows = budget / stride / 64 * 64;
    rows = rows < 64 ? 64 : (rows > max_tile ? max_tile : rows);
    const int need = (count + 63) / 64 * 64;
    return rows > need ? need : rows;
}
