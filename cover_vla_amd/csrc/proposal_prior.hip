// Proposal log-density prior (cover_proposal_prior_tokens / cover_proposal_prior_actions): the unnormalised log-density of every row
// of a prompt group under the diagonal Gaussian fitted to the group's first n_fit rows -- the distribution augment.hip draws its rows
// from -- plus, optionally, the log share of the row's gripper class among the fitted rows. One fp32 per row, the [N] prior
// cover_prior_select takes with steps = 1. The fit is augment_fit.h's, shared with augment.hip, the rows are chunk_rows.h's chunk_src;
// the results are compared with a numpy restatement as bit patterns, so contraction is off for the whole file and no logarithm is taken
// here (log_share comes from the host).
#include "common.h"
#include "kernels.h"
#include "augment_fit.h"

#pragma clang fp contract(off)

// one block per prompt group: statistics and vote counts -> LDS, then one thread per row (stride 256) runs the row's chain
template <typename T>
__global__ __launch_bounds__(256) void proposal_prior_k(cover_proposal_prior_args a, long long t_stride) {
    __shared__ float s_mean[6 * 64], s_s[6 * 64];
    __shared__ int s_jwin[64], s_votes[2 * 64];
    const int g = blockIdx.x, S = a.group_rows, h = a.h;
    const aug_fit<T> f = {chunk_src_of<T>(a, t_stride, (long long)g * S), a.n_fit, a.h, a.sigma, a.sd_floor, a.mean_out, a.sd_out, a.votes_out};
    const chunk_src<T>& x = f.src;
    augment_group_stats<T>(f, g, s_mean, s_s, s_jwin, s_votes);
    __syncthreads();
    for (int r = threadIdx.x; r < S; r += blockDim.x) {
        float acc = 0.0f;
        for (int t = 0; t < h; ++t)
            for (int d = 0; d < 6; ++d) {
                const float dev = x.value(r, t, d) - s_mean[t * 6 + d];
                const float z = dev / s_s[t * 6 + d];   // s > 0: the launch function checks sigma * sd_floor > 0
                const float sq = z * z;
                acc = acc + sq;
            }
        float p = -0.5f * acc;
        if (a.log_share)
            for (int t = 0; t < h; ++t) {
                const int c1 = x.value(r, t, 6) >= 0.5f ? 1 : 0;
                p = p + a.log_share[s_votes[2 * t + c1]];   // a count is 0..n_fit: inside the table
            }
        a.prior_out[(size_t)g * S + r] = p;
    }
}

static bool proposal_prior_args_ok(const cover_proposal_prior_args* a) {
    if (a->G < 1 || a->n_fit < 1 || a->n_fit > a->group_rows || a->group_rows > 4096 || a->h < 1 || a->h > 64) return false;
    if ((long long)a->G * a->group_rows > (1ll << 20)) return false;
    if (!f32_gt(a->sigma, 0.0f) || !f32_gt(a->sd_floor, 0.0f)) return false;
    const volatile float lowest = a->sigma * a->sd_floor;   // the smallest s a launch can divide by, rounded to fp32 as the kernel rounds it
    if (!(lowest > 0.0f)) return false;
    return a->src && a->prior_out;
}
hipError_t launch_proposal_prior_tokens(const cover_proposal_prior_args* a, hipStream_t st) {
    if (!proposal_prior_args_ok(a) || !token_form_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(proposal_prior_k<int64_t>, dim3(a->G), dim3(256), 0, st, *a, 7ll);
    return hipGetLastError();
}
hipError_t launch_proposal_prior_actions(const cover_proposal_prior_args* a, hipStream_t st) {
    if (!proposal_prior_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(proposal_prior_k<float>, dim3(a->G), dim3(256), 0, st, *a, a->t_stride);
    return hipGetLastError();
}
