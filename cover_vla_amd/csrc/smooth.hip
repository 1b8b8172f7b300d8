// Neighbourhood-smoothed verifier scores (cover_smooth_scores_tokens / cover_smooth_scores_actions): per prompt group a kernel-weighted
// local mean (Nadaraya-Watson, Epanechnikov weights on a scaled squared distance in the 6-D action space) of one fp32 score per row,
// shrunk towards the group mean. O(S^2 * 6 h) per group: one wave per row n, 16 rows per block, the lanes walk the group's rows j in
// lane-strided order over j-tiles of de-tokenised values staged in LDS; several blocks per group, each block recomputing what it needs
// of the group (its mean), so no thread's result depends on the tiling. The rows are chunk_rows.h's chunk_src, staged through its
// aug_value, so the token form reads what cover_augment_* / cover_refine_* read. The results are compared with a numpy restatement as
// bit patterns: contraction is off for the whole file.
#include "common.h"
#include "kernels.h"
#include "chunk_rows.h"   // chunk_src, chunk_stage_rows: the rows and their way into LDS
#include "chunk_dist.h"   // chunk_finite, chunk_load_scale

#pragma clang fp contract(off)

#define SMOOTH_MAX_ROWS 4096
#define SMOOTH_ROWS_PER_BLOCK 16      // one wave each
#define SMOOTH_TILE_FLOATS 12288      // the LDS budget of one j-tile (48 KiB) while more than 64 rows fit
#define SMOOTH_MAX_TILE 1024          // rows per j-tile at the narrowest row

// the weight of one pair of different rows: xn / xj point at the rows' [h][7] values (step stride 7). NOT chunk_dist.h's
// chunk_pair_dist_of: d2 is one chain over (step, dim) with no per-step subtotal and no step weight, a different sequence of roundings.
__device__ __forceinline__ float smooth_pair_weight(const float* xn, const float* xj, int h, const float* sc, bool split, float radius2) {
    bool same = true;
    float d2 = 0.0f;
    for (int t = 0; t < h; ++t) {
        if (split && ((xn[7 * t + 6] >= 0.5f) != (xj[7 * t + 6] >= 0.5f))) same = false;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            if (sc[d] != 0.0f) {   // a dim of scale 0 is not read into the sum: a NaN there is invisible
                const float diff = xn[7 * t + d] - xj[7 * t + d];
                const float s = diff * sc[d];
                const float sq = s * s;
                d2 = d2 + sq;
            }
        }
    }
    float w = 0.0f;
    if (d2 < radius2) {            // a NaN d2 fails the comparison
        const float q = d2 / radius2;
        w = 1.0f - q;
    }
    return same ? w : 0.0f;
}

// block b: rows n0 .. n0 + 15 of group g, n0 = 16 * (b % tiles); LDS = 16 own rows, then one j-tile of TJ rows, `stride` floats per row
// (7 h, made odd: the lanes of a wave read rows jj, jj + 1, ... at one column, so an odd stride is conflict-free)
template <typename T>
__global__ __launch_bounds__(1024) void smooth_k(cover_smooth_args a, long long t_stride, int TJ, int stride) {
    extern __shared__ float s_lds[];
    float* s_own = s_lds;
    float* s_x = s_lds + SMOOTH_ROWS_PER_BLOCK * stride;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int S = a.group_rows, h = a.h, w7 = 7 * h;
    const int tiles = (S + SMOOTH_ROWS_PER_BLOCK - 1) / SMOOTH_ROWS_PER_BLOCK;
    const int g = blockIdx.x / tiles, n0 = (blockIdx.x - g * tiles) * SMOOTH_ROWS_PER_BLOCK;
    const int n = n0 + wv;
    const bool live = n < S;
    const chunk_src<T> in = chunk_src_of<T>(a, t_stride, (long long)g * S);
    const float* score = a.scores + (size_t)g * S;
    float sc[6];
    const bool usable = chunk_load_scale(a.dim_scale, sc);   // a negative or non-finite scale: every pair weight is 0
    const bool split = a.split_gripper != 0;
    chunk_stage_rows(in, n0, min(SMOOTH_ROWS_PER_BLOCK, S - n0), w7, s_own, stride);
    // the group mean: a lane-strided chain over the finite scores, the butterfly, one divide
    float msum = 0.0f;
    int mcnt = 0;
    for (int j = lane; j < S; j += 64) {
        const float s = score[j];
        if (chunk_finite(s)) {
            msum = msum + s;
            mcnt += 1;
        }
    }
    msum = wave_sum(msum);
    mcnt = wave_sum_int(mcnt);
    const float m0 = mcnt > 0 ? msum / (float)mcnt : 0.0f;
    if (a.group_mean_out && n0 == 0 && threadIdx.x == 0) a.group_mean_out[g] = m0;

    const float* xn = s_own + wv * stride;
    float num = 0.0f, den = 0.0f, dsum = 0.0f;
    int cnt = 0;
    for (int j0 = 0; j0 < S; j0 += TJ) {
        __syncthreads();           // the previous tile has been read (first pass: nothing to wait for but the own rows' stores)
        const int rows = min(TJ, S - j0);
        chunk_stage_rows(in, j0, rows, w7, s_x, stride);
        __syncthreads();
        if (live) {
            for (int jj = lane; jj < rows; jj += 64) {
                const int j = j0 + jj;
                float w = 1.0f;    // the self pair, by definition
                if (j != n) w = usable ? smooth_pair_weight(xn, s_x + jj * stride, h, sc, split, a.radius2) : 0.0f;
                if (w > 0.0f) {
                    dsum = dsum + w;
                    cnt += 1;
                    const float s = score[j];
                    if (chunk_finite(s)) {
                        den = den + w;
                        const float prod = w * s;
                        num = num + prod;
                    }
                }
            }
        }
    }
    num = wave_sum(num);
    den = wave_sum(den);
    dsum = wave_sum(dsum);
    cnt = wave_sum_int(cnt);
    if (live && lane == 0) {
        const size_t o = (size_t)g * S + n;
        const float own = score[n];
        if (!chunk_finite(own)) {
            ((uint32_t*)a.smoothed_out)[o] = ((const uint32_t*)score)[n];   // bit for bit, a NaN keeps its payload
        } else if (a.shrink == 0.0f) {
            a.smoothed_out[o] = num / den;
        } else {
            const float tm = a.shrink * m0;
            const float nn = num + tm;
            const float dd = den + a.shrink;
            a.smoothed_out[o] = nn / dd;
        }
        if (a.density_out) a.density_out[o] = dsum / (float)S;
        if (a.neighbours_out) a.neighbours_out[o] = cnt;
    }
}

static bool smooth_args_ok(const cover_smooth_args* a) {
    if (a->G < 1 || a->group_rows < 1 || a->group_rows > SMOOTH_MAX_ROWS || a->h < 1 || a->h > 64) return false;
    if ((long long)a->G * a->group_rows > (1ll << 20)) return false;
    if (!f32_gt(a->radius2, 0.0f) || !f32_ge(a->shrink, 0.0f)) return false;
    return a->src && a->scores && a->dim_scale && a->smoothed_out;
}
template <typename T>
static hipError_t smooth_launch(const cover_smooth_args* a, long long t_stride, hipStream_t st) {
    const int S = a->group_rows, stride = (7 * a->h) | 1;
    const int TJ = chunk_tile_rows(stride, S, SMOOTH_TILE_FLOATS, SMOOTH_MAX_TILE);
    const size_t lds = (size_t)(SMOOTH_ROWS_PER_BLOCK + TJ) * stride * sizeof(float);   // <= 80 * 449 * 4 = 143,680 B at h = 64
    const hipError_t e = LDS_ATTR_FOR(smooth_k<T>, lds);
    if (e != hipSuccess) return e;
    const int tiles = (S + SMOOTH_ROWS_PER_BLOCK - 1) / SMOOTH_ROWS_PER_BLOCK;
    hipLaunchKernelGGL(smooth_k<T>, dim3(a->G * tiles), dim3(64 * SMOOTH_ROWS_PER_BLOCK), lds, st, *a, t_stride, TJ, stride);
    return hipGetLastError();
}
hipError_t launch_smooth_scores_tokens(const cover_smooth_args* a, hipStream_t st) {
    if (!smooth_args_ok(a) || !token_form_ok(a)) return hipErrorInvalidValue;
    return smooth_launch<int64_t>(a, 7ll, st);
}
hipError_t launch_smooth_scores_actions(const cover_smooth_args* a, hipStream_t st) {
    if (!smooth_args_ok(a)) return hipErrorInvalidValue;
    return smooth_launch<float>(a, a->t_stride, st);
}
