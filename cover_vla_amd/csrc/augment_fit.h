// The per-prompt fit that augment.hip (the rows drawn from it) and proposal_prior.hip (its log-density at every row) share: per
// (step, dim < 6) the chain mean and s = sigma * fmaxf(sqrtf(var), sd_floor) of a group's first n rows, per step their gripper vote.
// Stated once, so the two files cannot drift apart: both results are compared with numpy restatements as bit patterns. Contraction is
// off from here to the end of the including file (hipcc would otherwise fuse dev * dev + ss into one v_fma_f32). The rows come from
// chunk_rows.h's chunk_src, which holds aug_value (the token rule) for every file that reads candidate rows.
#pragma once
#include "chunk_rows.h"

#pragma clang fp contract(off)

// what the fit needs: the rows fitted to, how many, and where the statistics go
template <typename T>
struct aug_fit {
    chunk_src<T> src;               // the group; the fitted rows are its first n
    int n, h;                       // rows fitted to, steps
    float sigma, sd_floor;
    float* mean_out; float* sd_out; // [G][h][6], optional
    int* votes_out;                 // [G][h][2], optional
};

// The statistics of one prompt group, left in LDS: for item i = t * 6 + d < 6 h the mean and s = sigma * sd of (step t, dim d), for
// step t the index of the sample whose gripper the augmented rows take and, with s_votes, the (class-0, class-1) counts at
// s_votes[2 t], s_votes[2 t + 1]. One thread per item, the samples in index order. The caller synchronises before it reads the arrays.
template <typename T>
__device__ void augment_group_stats(const aug_fit<T>& a, int g, float* s_mean, float* s_s, int* s_jwin, int* s_votes = nullptr) {
    const int n = a.n, h = a.h;
    const chunk_src<T>& s = a.src;
    for (int i = threadIdx.x; i < 7 * h; i += blockDim.x) {
        if (i < 6 * h) {
            const int t = i / 6, d = i - t * 6;
            const T* x = s.in + (long long)t * s.t_stride + d;   // row 0's element: the chains below walk the rows from it
            float sum = 0.0f;
            for (int j = 0; j < n; ++j) sum = sum + aug_value(s, x[(long long)j * s.n_stride]);
            const float mean = sum / (float)n;
            float ss = 0.0f;
            for (int j = 0; j < n; ++j) {
                const float dev = aug_value(s, x[(long long)j * s.n_stride]) - mean;
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
            const T* x = s.in + (long long)t * s.t_stride + 6;
            int ones = 0, first0 = -1, first1 = -1;
            for (int j = 0; j < n; ++j) {
                const bool c1 = aug_value(s, x[(long long)j * s.n_stride]) >= 0.5f;
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
