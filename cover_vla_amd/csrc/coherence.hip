// Chunk-coherence prior (cover_coherence_prior_tokens / cover_coherence_prior_actions): per candidate row the negated, signed-weighted sum
// of its step-weighted squared distances to a set of reference chunks -- Bidirectional Decoding's backward coherence (one reference: the
// unexecuted tail of the chunk committed last time) and forward contrast (strong rows with positive, weak rows with negative weights) in
// one form. O(S * R * 6 T) per group: one wave per candidate row n, 16 rows per block, the lanes walk the references r in lane-strided
// order over r-tiles staged in LDS; several blocks per group. A lane's chain order is a function of r alone, so no result depends on the
// tiling. The candidate rows are chunk_rows.h's chunk_src, staged through its aug_value, so the token form reads what cover_augment_* /
// cover_refine_* / cover_smooth_scores_* read. The results are compared with a numpy restatement as bit patterns: contraction is off for
// the whole file.
#include "common.h"
#include "kernels.h"
#include "chunk_rows.h"   // chunk_src, chunk_stage_rows: the rows and their way into LDS
#include "chunk_dist.h"   // chunk_pair_dist: the pair distance, shared with diverse.hip

#pragma clang fp contract(off)

#define COHERENCE_MAX_ROWS 4096
#define COHERENCE_MAX_REFS 4096
#define COHERENCE_ROWS_PER_BLOCK 16   // one wave each
#define COHERENCE_TILE_FLOATS 12288   // the LDS budget of one r-tile (48 KiB) while more than 64 references fit
#define COHERENCE_MAX_TILE 1024       // references per r-tile at the narrowest row

// the lexicographic (D, r) minimum; r < 0 is "none yet"
__device__ __forceinline__ void coherence_take_min(float& bd, int& br, float d, int r) {
    if (r >= 0 && (br < 0 || d < bd || (d == bd && r < br))) {
        bd = d;
        br = r;
    }
}

// block b: rows n0 .. n0 + 15 of group g, n0 = 16 * (b % tiles); LDS = 16 own rows, then one r-tile of TR reference rows, `stride` floats
// per row (7 T, made odd: the lanes of a wave read rows rr, rr + 1, ... at one column, so an odd stride is conflict-free), then T step weights
template <typename T>
__global__ __launch_bounds__(1024) void coherence_k(cover_coherence_args a, long long t_stride, int TR, int stride) {
    extern __shared__ float s_lds[];
    float* s_own = s_lds;
    float* s_y = s_lds + COHERENCE_ROWS_PER_BLOCK * stride;
    float* s_sw = s_y + (size_t)TR * stride;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int S = a.group_rows, R = a.R;
    const int To = min(a.h, a.hr - a.shift), w7 = 7 * To;                  // the overlap
    const int tiles = (S + COHERENCE_ROWS_PER_BLOCK - 1) / COHERENCE_ROWS_PER_BLOCK;
    const int g = blockIdx.x / tiles, n0 = (blockIdx.x - g * tiles) * COHERENCE_ROWS_PER_BLOCK;
    const int n = n0 + wv;
    const bool live = n < S;
    const chunk_src<T> in = chunk_src_of<T>(a, t_stride, (long long)g * S);
    const float* ref = a.ref + (long long)g * a.ref_g_stride + 7 * a.shift;   // candidate step t meets reference step t + shift
    const float* wt = a.ref_weight + (long long)g * a.w_g_stride;
    float sc[6];
    const bool usable = chunk_load_scale(a.dim_scale, sc);   // a negative or non-finite scale: every prior of the launch is NaN
    chunk_stage_rows(in, n0, min(COHERENCE_ROWS_PER_BLOCK, S - n0), w7, s_own, stride);
    for (int i = threadIdx.x; i < To; i += blockDim.x) s_sw[i] = a.step_weight[i];

    const float* x = s_own + wv * stride;
    float acc = 0.0f, bd = 0.0f;
    int br = -1;
    for (int r0 = 0; r0 < R; r0 += TR) {
        __syncthreads();           // the previous tile has been read (first pass: nothing to wait for but the own rows' stores)
        const int rows = min(TR, R - r0);
        for (int i = threadIdx.x; i < rows * w7; i += blockDim.x) {
            const int r = i / w7, c = i - r * w7;
            s_y[r * stride + c] = ref[(long long)(r0 + r) * a.ref_r_stride + c];
        }
        __syncthreads();
        if (live && usable) {
            for (int rr = lane; rr < rows; rr += 64) {
                const int r = r0 + rr;
                const float w = wt[r];
                if (w != 0.0f) {   // a reference of weight 0 is never read into a sum
                    const float D = chunk_pair_dist(x, s_y + rr * stride, To, sc, s_sw, a.gripper_penalty);
                    const float prod = w * D;
                    acc = acc + prod;
                    if (D == D) coherence_take_min(bd, br, D, r);   // a NaN D is never the minimum; r ascends within a lane
                }
            }
        }
    }
    acc = wave_sum(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(bd, o);
        const int orr = __shfl_xor(br, o);
        coherence_take_min(bd, br, od, orr);
    }
    if (live && lane == 0) {
        const size_t o = (size_t)g * S + n;
        uint32_t bits = __float_as_uint(acc) ^ 0x80000000u;               // -acc: the sign bit flipped, so 0.0f stores 0x80000000
        if (!usable || acc != acc) bits = 0x7FC00000u;                     // every NaN prior is this one NaN
        ((uint32_t*)a.prior_out)[o] = bits;
        if (a.min_dist_out) ((uint32_t*)a.min_dist_out)[o] = br < 0 ? 0x7F800000u : __float_as_uint(bd);
        if (a.nearest_out) a.nearest_out[o] = br;
    }
}

static bool coherence_args_ok(const cover_coherence_args* a) {
    if (a->G < 1 || a->group_rows < 1 || a->group_rows > COHERENCE_MAX_ROWS || a->R < 1 || a->R > COHERENCE_MAX_REFS) return false;
    if (a->h < 1 || a->h > 64 || a->hr < 1 || a->hr > 64 || a->shift < 0 || a->shift >= a->hr) return false;
    if ((long long)a->G * a->group_rows > (1ll << 20)) return false;
    if (a->ref_r_stride < 7ll * a->hr) return false;
    if (a->ref_g_stride != 0) {    // >= (R - 1) * ref_r_stride + 7 hr, without forming a product that could overflow
        const long long gap = a->ref_g_stride - 7ll * a->hr;
        if (gap < 0 || (a->R > 1 && gap / (a->R - 1) < a->ref_r_stride)) return false;
    }
    if (a->w_g_stride != 0 && a->w_g_stride != a->R) return false;
    if (!f32_ge(a->gripper_penalty, 0.0f)) return false;
    return a->src && a->ref && a->ref_weight && a->step_weight && a->dim_scale && a->prior_out;
}
template <typename T>
static hipError_t coherence_launch(const cover_coherence_args* a, long long t_stride, hipStream_t st) {
    const int S = a->group_rows, R = a->R, To = a->h < a->hr - a->shift ? a->h : a->hr - a->shift, stride = (7 * To) | 1;
    const int TR = chunk_tile_rows(stride, R, COHERENCE_TILE_FLOATS, COHERENCE_MAX_TILE);
    const size_t lds = ((size_t)(COHERENCE_ROWS_PER_BLOCK + TR) * stride + To) * sizeof(float);   // <= (80 * 449 + 64) * 4 = 143,936 B at T = 64
    const hipError_t e = LDS_ATTR_FOR(coherence_k<T>, lds);
    if (e != hipSuccess) return e;
    const int tiles = (S + COHERENCE_ROWS_PER_BLOCK - 1) / COHERENCE_ROWS_PER_BLOCK;
    hipLaunchKernelGGL(coherence_k<T>, dim3(a->G * tiles), dim3(64 * COHERENCE_ROWS_PER_BLOCK), lds, st, *a, t_stride, TR, stride);
    return hipGetLastError();
}
hipError_t launch_coherence_prior_tokens(const cover_coherence_args* a, hipStream_t st) {
    if (!coherence_args_ok(a) || !token_form_ok(a)) return hipErrorInvalidValue;
    return coherence_launch<int64_t>(a, 7ll, st);
}
hipError_t launch_coherence_prior_actions(const cover_coherence_args* a, hipStream_t st) {
    if (!coherence_args_ok(a)) return hipErrorInvalidValue;
    return coherence_launch<float>(a, a->t_stride, st);
}
