// The draw that augment.hip (rows drawn from the fit of a prompt's policy samples) and refine.hip (rows drawn from the fit of a prompt's
// best-scored rows) share: what an augmented value is stored as, and the walk over the K drawn rows of one group. Stated once, as the fit
// is in augment_fit.h, so the two files cannot drift apart: both results are compared with numpy restatements as bit patterns. Contraction
// is off from here to the end of the including file (hipcc would otherwise fuse mean + s * z into one v_fma_f32). The fitted rows are
// chunk_rows.h's chunk_src, carried by the aug_fit.
#pragma once
#include "augment_fit.h"

#pragma clang fp contract(off)

// what an augmented value is stored as: floats as they are, tokens as the token of the nearest bin centre
__device__ __forceinline__ void aug_store(const chunk_src<float>& a, float v, float* o) { *o = v; }
__device__ __forceinline__ void aug_store(const chunk_src<int64_t>& a, float v, int64_t* o) {
    // first index that minimises |v - centers[b]|: a plain scan (b is uniform over the wave: the table comes through scalar loads)
    float best = fabsf(v - a.centers[0]);
    int bi = 0;
    for (int b = 1; b < a.n_centers; ++b) {
        const float dist = fabsf(v - a.centers[b]);
        if (dist < best) {
            best = dist;
            bi = b;
        }
    }
    *o = (int64_t)a.tok_vocab - 1 - bi;
}

// The K drawn rows of one group, walked by the block in output order (k, t, d) (coalesced stores): out = the first drawn row,
// z = the group's normals [K][h][6], s_mean / s_s / s_jwin = augment_group_stats' arrays (the caller has synchronised behind it),
// the gripper (d == 6) of every drawn row is the fitted row s_jwin[t]'s. The fitted rows (a.src, chunk_rows.h) may be rows of the same
// buffer as `out` as long as they lie outside the K drawn ones.
template <typename T>
__device__ __forceinline__ void augment_draw_rows(const aug_fit<T>& a, T* out, const float* z, int K, float clip_lo, float clip_hi,
                                                  const float* s_mean, const float* s_s, const int* s_jwin) {
    const int h = a.h, w = 7 * h;
    for (int i = threadIdx.x; i < K * w; i += blockDim.x) {
        const int k = i / w, r = i - k * w, t = r / 7, d = r - t * 7;
        if (d == 6) {
            out[i] = a.src.raw(s_jwin[t], t, 6);
            continue;
        }
        const float p = s_s[t * 6 + d] * z[((size_t)k * h + t) * 6 + d];
        float v = s_mean[t * 6 + d] + p;
        v = fminf(fmaxf(v, clip_lo), clip_hi);
        aug_store(a.src, v, out + i);
    }
}
