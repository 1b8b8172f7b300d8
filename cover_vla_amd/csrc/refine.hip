// Verifier-guided refinement (cover_refine_tokens / cover_refine_actions): one round of the cross-entropy method per prompt group. The
// group's rows are ranked by their scores, the n_elite best are gathered to the front of the output verbatim, the diagonal Gaussian of
// augment.hip is fitted to those gathered rows and K new rows are drawn from it behind them. The fit is augment_fit.h's and the draw
// augment_draw.h's, both shared with augment.hip, so the output is what cover_augment_* gives on the gathered rows, bit for bit; the
// order is a sort of unique keys (keysort.h), so it does not depend on the schedule. The input rows and the gather are chunk_rows.h's
// (chunk_src, chunk_gather_rows). The results are compared with a numpy restatement as bit patterns: contraction is off for the whole file.
#include "common.h"
#include "kernels.h"
#include "keysort.h"
#include "augment_fit.h"
#include "augment_draw.h"   // aug_store, augment_draw_rows: the draw, shared with augment.hip

#pragma clang fp contract(off)

#define REFINE_MAX_ROWS 4096

// one block per prompt group: keys -> LDS, sorted; the elites gathered in rank order; statistics of the gathered rows -> LDS; then the
// block walks (k, t, d) of the K drawn rows in output order
template <typename T>
__global__ __launch_bounds__(256) void refine_k(cover_refine_args a, long long t_stride) {
    __shared__ unsigned long long s_key[REFINE_MAX_ROWS];
    __shared__ float s_mean[6 * 64], s_s[6 * 64];
    __shared__ int s_jwin[64];
    const int g = blockIdx.x, S = a.group_rows, m = a.n_elite, K = a.K, h = a.h, w = 7 * h;
    int n2 = 2;
    while (n2 < S) n2 <<= 1;
    // 1. rank: higher score first, equal scores (-0 == +0) by ascending index, a NaN behind every number (desc_key alone would put a
    // positive NaN first); a NaN's high word stays below the dead key because its low word is an index < 4096
    const float* sc = a.scores + (size_t)g * S;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        unsigned long long key = ~0ull;
        if (i < S) {
            const float s = sc[i];
            const uint32_t hi = s != s ? 0xFFFFFFFFu : desc_key(s);
            key = ((unsigned long long)hi << 32) | (uint32_t)i;
        }
        s_key[i] = key;
    }
    __syncthreads();
    bitonic_sort_lds(s_key, n2);   // returns behind a barrier
    // 2. gather: output row r < m is the input row of rank r (m <= S, and the S live keys sort in front of the dead ones: j < S)
    T* out = (T*)a.out + (size_t)g * (m + K) * w;
    chunk_gather_rows(chunk_src_of<T>(a, t_stride, (long long)g * S), m, w, out, [&](int r) { return (int)(uint32_t)s_key[r]; });
    for (int r = threadIdx.x; r < m; r += blockDim.x) {
        const int j = (int)(uint32_t)s_key[r];
        if (a.elite_rows_out) a.elite_rows_out[(size_t)g * m + r] = g * S + j;
        if (a.elite_scores_out) ((uint32_t*)a.elite_scores_out)[(size_t)g * m + r] = ((const uint32_t*)sc)[j];   // the score's bits
    }
    __syncthreads();   // the gathered rows, stored by this block, are what the fit reads
    // 3. fit and draw: cover_augment_*'s second half on the output's own first m rows (row stride 7 h, step stride 7), so the chains run
    // in rank order and a gripper tie goes to the best elite's class
    const aug_fit<T> f = {{out, (long long)w, 7ll, a.centers, a.n_centers, a.tok_vocab}, m, h, a.sigma, a.sd_floor, a.mean_out, a.sd_out, a.votes_out};
    augment_group_stats<T>(f, g, s_mean, s_s, s_jwin);
    __syncthreads();
    augment_draw_rows<T>(f, out + (size_t)m * w, a.normals + (size_t)g * K * 6 * h, K, a.clip_lo, a.clip_hi, s_mean, s_s, s_jwin);
}

static bool refine_args_ok(const cover_refine_args* a) {
    if (a->G < 1 || a->n_elite < 1 || a->n_elite > a->group_rows || a->group_rows > REFINE_MAX_ROWS || a->K < 0 || a->K > 4096 || a->h < 1 ||
        a->h > 64)
        return false;
    if ((long long)a->G * a->group_rows > (1ll << 20) || (long long)a->G * (a->n_elite + a->K) > (1ll << 20)) return false;
    if (!f32_ge(a->sigma, 0.0f) || !f32_ge(a->sd_floor, 0.0f)) return false;
    if (!(a->clip_lo <= a->clip_hi)) return false;
    return a->src && a->scores && a->out && (a->K == 0 || a->normals);
}
hipError_t launch_refine_tokens(const cover_refine_args* a, hipStream_t st) {
    if (!refine_args_ok(a) || !token_form_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refine_k<int64_t>, dim3(a->G), dim3(256), 0, st, *a, 7ll);
    return hipGetLastError();
}
hipError_t launch_refine_actions(const cover_refine_args* a, hipStream_t st) {
    if (!refine_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(refine_k<float>, dim3(a->G), dim3(256), 0, st, *a, a->t_stride);
    return hipGetLastError();
}
