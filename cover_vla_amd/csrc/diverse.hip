// Diverse candidate subsets (cover_diverse_subset_tokens / cover_diverse_subset_actions): per prompt group the greedy selection of at
// most m of its S rows by quality + weight * (distance to the nearest row already chosen), with a covering distance that leaves out rows
// a pick already covers -- pruning before the verifier, deduplication and the maximal-marginal-relevance shortlist in one loop. The picks
// depend on each other, so one 1024-thread block owns a group for the whole loop: thread tid keeps mind / assign of rows tid + 1024 q
// (q < 4) in registers, the newest pick's row is staged in LDS and read as a broadcast, and the block arg-max is a min over unique 64-bit
// keys (desc_key(v) << 32 | row), so no result depends on the schedule. O(m * S * 6 h) per group, latency-bound by design: two barriers
// per pick. The distance is chunk_dist.h's, shared with coherence.hip; the rows are chunk_rows.h's chunk_src, read through its aug_value,
// so the token form reads what cover_augment_* / cover_refine_* / cover_coherence_prior_* read. The results are compared with a numpy
// restatement as bit patterns: contraction is off for the whole file. The staging and gather walks are written out here, with the
// block's fixed step, and not taken from chunk_rows.h: with the shared walks the compiler laid the pick loop out differently and the
// resident path measured 3 - 21 % slower (docs/OPTIMISATION_LOG.md); as written the kernels compile to the instructions they had.
#include "common.h"
#include "kernels.h"
#include "keysort.h"       // desc_key
#include "chunk_rows.h"    // chunk_src, aug_value; token_form_ok, f32_ge
#include "chunk_dist.h"

#pragma clang fp contract(off)

#define DIVERSE_MAX_ROWS 4096
#define DIVERSE_THREADS 1024
#define DIVERSE_ROWS_PER_THREAD (DIVERSE_MAX_ROWS / DIVERSE_THREADS)
#define DIVERSE_LDS_BUDGET (160 * 1024 - 256)   // bytes of rows, pick, step weights and slots: the CU's 160 KiB less the 16 partials and slack
#define DIVERSE_PART_BYTES (DIVERSE_THREADS / 64 * 8)
#define DIVERSE_NONE (~0ull)                    // no candidate: above every live key (desc_key gives 0xFFFFFFFF to a NaN only)

__device__ __forceinline__ unsigned long long diverse_wave_min(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), o);
        const unsigned long long other = ((unsigned long long)hi << 32) | lo;
        k = other < k ? other : k;
    }
    return k;
}

// block g = group g. Dynamic LDS (all of it: a kernel with static LDS cannot be given the full 160 KiB): the 16 waves' partial keys, the
// newest pick's row [stride], the step weights [h], the picked rows' indices [m] and, with RES, the group's values [S][stride];
// `stride` = 7 h made odd (thread i reads row i at one column: an odd stride is conflict-free)
template <typename T, bool RES>
__global__ __launch_bounds__(DIVERSE_THREADS) void diverse_k(cover_diverse_args a, long long t_stride, int stride) {
    extern __shared__ unsigned long long s_part[];
    float* s_pick = (float*)(s_part + DIVERSE_THREADS / 64);
    float* s_sw = s_pick + stride;
    int* s_slot = (int*)(s_sw + a.h);
    float* s_rows = (float*)(s_slot + a.m);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = blockIdx.x, S = a.group_rows, m = a.m, h = a.h, w7 = 7 * h;
    const T* in = (const T*)a.src + (long long)g * S * a.n_stride;
    const chunk_src<T> f = {in, a.n_stride, t_stride, a.centers, a.n_centers, a.tok_vocab};
    float sc[6];
    const bool usable = chunk_load_scale(a.dim_scale, sc);   // a negative or non-finite scale: no row is eligible
    const float penalty = a.gripper_penalty, weight = a.weight, cover = a.cover_dist;

    const auto load = [&](int i, int t, int d) -> float { return aug_value(f, in[(long long)i * a.n_stride + (long long)t * t_stride + d]); };
    for (int c = tid; c < h; c += DIVERSE_THREADS) s_sw[c] = a.step_weight[c];
    if (RES)
        for (int idx = tid; idx < S * w7; idx += DIVERSE_THREADS) {
            const int i = idx / w7, c = idx - i * w7, t = c / 7;
            s_rows[i * stride + c] = load(i, t, c - t * 7);
        }
    __syncthreads();
    // the value (t, d) of row i, and D(row i, the staged pick)
    const auto row = [&](int i) {
        return [&, i](int t, int d) -> float {
            if constexpr (RES) return s_rows[i * stride + 7 * t + d];
            else return load(i, t, d);
        };
    };
    const auto pick = [&](int t, int d) -> float { return s_pick[7 * t + d]; };

    float q[DIVERSE_ROWS_PER_THREAD], mind[DIVERSE_ROWS_PER_THREAD];
    int asg[DIVERSE_ROWS_PER_THREAD];
    unsigned elig = 0, taken = 0;                            // bit qq: row tid + 1024 qq
#pragma unroll
    for (int qq = 0; qq < DIVERSE_ROWS_PER_THREAD; ++qq) {
        const int i = tid + DIVERSE_THREADS * qq;
        q[qq] = 0.0f;
        mind[qq] = __uint_as_float(0x7F800000u);
        asg[qq] = -1;
        if (i < S) {
            if (a.quality) q[qq] = a.quality[(size_t)g * S + i];
            if (usable) {
                const float self = chunk_pair_dist_of(row(i), row(i), h, sc, s_sw, penalty);
                if (q[qq] == q[qq] && self == self) elig |= 1u << qq;
            }
        }
    }

    int count = 0;
    for (int k = 0; k < m; ++k) {
        // 1. the lexicographic (v descending, row ascending) maximum over the candidates, as the minimum of unique keys
        unsigned long long best = DIVERSE_NONE;
#pragma unroll
        for (int qq = 0; qq < DIVERSE_ROWS_PER_THREAD; ++qq) {
            const int i = tid + DIVERSE_THREADS * qq;
            if (i < S && ((elig & ~taken) >> qq & 1u) && mind[qq] > cover) {
                float v = q[qq];
                if (k > 0 && weight != 0.0f) {
                    const float prod = weight * mind[qq];
                    v = q[qq] + prod;
                }
                if (v == v) {
                    const unsigned long long key = ((unsigned long long)desc_key(v) << 32) | (uint32_t)i;
                    best = key < best ? key : best;
                }
            }
        }
        best = diverse_wave_min(best);
        if (lane == 0) s_part[wv] = best;
        __syncthreads();
        unsigned long long win = s_part[0];
#pragma unroll
        for (int w = 1; w < DIVERSE_THREADS / 64; ++w) win = s_part[w] < win ? s_part[w] : win;
        if (win == DIVERSE_NONE) break;                      // the same in every thread
        const int p = (int)(uint32_t)win;
        // 2. its owner records it; the block stages its row
        if ((p & (DIVERSE_THREADS - 1)) == tid) {
#pragma unroll
            for (int qq = 0; qq < DIVERSE_ROWS_PER_THREAD; ++qq)
                if (qq == p / DIVERSE_THREADS) {
                    float v = q[qq];
                    if (k > 0 && weight != 0.0f) {
                        const float prod = weight * mind[qq];
                        v = q[qq] + prod;
                    }
                    taken |= 1u << qq;
                    s_slot[k] = p;
                    a.picked_rows_out[(size_t)g * m + k] = g * S + p;
                    if (a.pick_value_out) a.pick_value_out[(size_t)g * m + k] = v;
                    if (a.pick_dist_out) a.pick_dist_out[(size_t)g * m + k] = mind[qq];
                }
        }
        for (int c = tid; c < w7; c += DIVERSE_THREADS) {
            const int t = c / 7;
            s_pick[c] = row(p)(t, c - t * 7);
        }
        __syncthreads();
        // 3. every row meets the new pick
#pragma unroll
        for (int qq = 0; qq < DIVERSE_ROWS_PER_THREAD; ++qq) {
            const int i = tid + DIVERSE_THREADS * qq;
            if (i < S) {
                const float d = chunk_pair_dist_of(row(i), pick, h, sc, s_sw, penalty);
                if (d < mind[qq]) {                          // strict; a NaN d never enters
                    mind[qq] = d;
                    asg[qq] = k;
                }
            }
        }
        count = k + 1;
    }
    __syncthreads();

    if (tid == 0 && a.count_out) a.count_out[g] = count;
    for (int k = count + tid; k < m; k += DIVERSE_THREADS) {
        a.picked_rows_out[(size_t)g * m + k] = -1;
        if (a.pick_value_out) ((uint32_t*)a.pick_value_out)[(size_t)g * m + k] = 0x7FC00000u;
        if (a.pick_dist_out) ((uint32_t*)a.pick_dist_out)[(size_t)g * m + k] = 0x7F800000u;
    }
#pragma unroll
    for (int qq = 0; qq < DIVERSE_ROWS_PER_THREAD; ++qq) {
        const int i = tid + DIVERSE_THREADS * qq;
        if (i < S) {
            if (a.assign_out) a.assign_out[(size_t)g * S + i] = asg[qq];
            if (a.row_dist_out) a.row_dist_out[(size_t)g * S + i] = mind[qq];
        }
    }
    if (a.out) {   // the picked rows verbatim; an unfilled slot repeats slot 0, a group with no pick its input row 0
        T* out = (T*)a.out + (size_t)g * m * w7;
        for (int idx = tid; idx < m * w7; idx += DIVERSE_THREADS) {
            const int r = idx / w7, c = idx - r * w7, t = c / 7, d = c - t * 7;
            const int j = r < count ? s_slot[r] : (count > 0 ? s_slot[0] : 0);
            out[idx] = in[(long long)j * a.n_stride + (long long)t * t_stride + d];
        }
    }
}

static bool diverse_args_ok(const cover_diverse_args* a) {
    if (a->G < 1 || a->m < 1 || a->m > a->group_rows || a->group_rows > DIVERSE_MAX_ROWS || a->h < 1 || a->h > 64) return false;
    if ((long long)a->G * a->group_rows > (1ll << 20)) return false;
    if (!f32_ge(a->weight, 0.0f) || !f32_ge(a->gripper_penalty, 0.0f)) return false;
    if (!f32_ge(a->cover_dist, -INFINITY)) return false;                                    // NaN and +inf; -inf is "off"
    return a->src && a->step_weight && a->dim_scale && a->picked_rows_out;
}
template <typename T>
static hipError_t diverse_launch(const cover_diverse_args* a, long long t_stride, hipStream_t st) {
    const int S = a->group_rows, stride = (7 * a->h) | 1;
    const size_t fixed = ((size_t)stride + a->h + a->m) * sizeof(float), rows = (size_t)S * stride * sizeof(float);
    const bool resident = fixed + rows <= DIVERSE_LDS_BUDGET;   // a function of (S, m, h) alone
    const size_t lds = DIVERSE_PART_BYTES + fixed + (resident ? rows : 0);
    if (resident) {
        const hipError_t e = LDS_ATTR_FOR((diverse_k<T, true>), lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((diverse_k<T, true>), dim3(a->G), dim3(DIVERSE_THREADS), lds, st, *a, t_stride, stride);
    } else {
        hipLaunchKernelGGL((diverse_k<T, false>), dim3(a->G), dim3(DIVERSE_THREADS), lds, st, *a, t_stride, stride);
    }
    return hipGetLastError();
}
hipError_t launch_diverse_subset_tokens(const cover_diverse_args* a, hipStream_t st) {
    if (!diverse_args_ok(a) || !token_form_ok(a)) return hipErrorInvalidValue;
    return diverse_launch<int64_t>(a, 7ll, st);
}
hipError_t launch_diverse_subset_actions(const cover_diverse_args* a, hipStream_t st) {
    if (!diverse_args_ok(a)) return hipErrorInvalidValue;
    return diverse_launch<float>(a, a->t_stride, st);
}
