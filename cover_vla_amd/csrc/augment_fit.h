// The per-prompt fit that augment.hip (the rows drawn from it) and proposal_prior.hip (its log-density at every row) share: per
// (step, dim < 6) the chain mean and s = sigma * fmaxf(sqrtf(var), sd_floor) of a group's first n rows, per step their gripper vote.
// Stated once, so the two files cannot drift apart: both results are compared with numpy restatements as bit patterns. Contraction is
// off from here to the end of the including file (hipcc would otherwise fuse dev * dev + ss into one v_fma_f32).
#pragma once
#include "common.h"

#pragma clang fp contract(off)

// what the fit needs of either launch's arguments
struct aug_fit {
    const float* centers;           // tokens: [n_centers] bin centres
    int n_centers, tok_vocab;
    long long n_stride;             // row stride of the input, in elements
    int n, h;                       // rows fitted to, steps
    float sigma, sd_floor;
    float* mean_out; float* sd_out; // [G][h][6], optional
    int* votes_out;                 // [G][h][2], optional
};

// what a raw input element is worth: floats pass through, tokens go through the bin centres
__device__ __forceinline__ float aug_value(const aug_fit& a, float raw) { return raw; }
__device__ __forceinline__ float aug_value(const aug_fit& a, int64_t token) {
    long long b = (long long)a.tok_vocab - token - 1;   // tokens_to_histories_k's rule
    b = b < 0 ? 0 : (b > a.n_centers - 1 ? a.n_centers - 1 : b);
    return a.centers[b];
}

// The statistics of one prompt group, left in LDS: for item i = t * 6 + d < 6 h the mean and s = sigma * sd of (step t, dim d), for
// step t the index of the sample whose gripper the augmented rows take and, with s_votes, the (class-0, class-1) counts at
// s_votes[2 t], s_votes[2 t + 1]. `in` is the group's first row; element (j, t, d) at in[j * n_stride + t * t_stride + d]. One thread
// per item, the samples in index order. The caller synchronises before it reads the arrays.
template <typename T>
__device__ void augment_group_stats(const aug_fit& a, const T* in, long long t_stride, int g, float* s_mean, float* s_s, int* s_jwin,
                                    int* s_votes = nullptr) {
    const int n = a.n, h = a.h;
    for (int i = threadIdx.x; i < 7 * h; i += blockDim.x) {
        if (i < 6 * h) {
            const int t = i / 6, d = i - t * 6;
            const T* x = in + (long long)t * t_stride + d;
            float sum = 0.0f;
            for (int j = 0; j < n; ++j) sum = sum + aug_value(a, x[(long long)j * a.n_stride]);
            const float mean = sum / (float)n;
            float ss = 0.0f;
            for (int j = 0; j < n; ++j) {
                const float dev = aug_value(a, x[(long long)j * a.n_stride]) - mean;
                const float sq = dev * dev;
                ss = ss + sq;
            }
            const float var = n > 1 ? ss / (float)(n - 1) : 0.0f;
            const float sd = fmaxf(sqrtf(var), a.sd_floor);
            s_mean[i] = mean;
            s_s[i] = a.sigma * sd;
            if (a.mean_out) a.mean_out[(size_t)g * 6 * h + i] = mean;
            if (a.sd_out) a.sd_out[(size_t)g * 6 * h + i] = sd;
        } else {
            const int t = i - 6 * h;
            const T* x = in + (long long)t * t_stride + 6;
            int ones = 0, first0 = -1, first1 = -1;
            for (int j = 0; j < n; ++j) {
                const bool c1 = aug_value(a, x[(long long)j * a.n_stride]) >= 0.5f;
                ones += c1 ? 1 : 0;
                if (c1 && first1 < 0) first1 = j;
                if (!c1 && first0 < 0) first0 = j;
            }
            const int zeros = n - ones;
            const bool win1 = ones > zeros || (ones == zeros && first1 == 0);   // a tie goes to the class of sample 0
            s_jwin[t] = win1 ? first1 : first0;
            if (s_votes) {
                s_votes[2 * t] = zeros;
                s_votes[2 * t + 1] = ones;
            }
            if (a.votes_out) {
                a.votes_out[((size_t)g * h + t) * 2] = zeros;
                a.votes_out[((size_t)g * h + t) * 2 + 1] = ones;
            }
        }
    }
}
