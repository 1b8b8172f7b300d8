// Gaussian proposal augmentation (cover_augment_tokens / cover_augment_actions): K verifier candidates per prompt from the prompt's n
// policy samples -- per (step, dim) a diagonal Gaussian fitted to the samples, the gripper by majority vote. The results are compared
// with a numpy restatement as bit patterns, so every value is a fixed sequence of fp32 roundings (the house rule of select.hip): plain
// operators with contraction off for the whole file, because hipcc would otherwise fuse d * d + ss and mean + s * z into one v_fma_f32.
#include "common.h"
#include "kernels.h"
#include "augment_fit.h"   // augment_group_stats: the fit, shared with proposal_prior.hip and refine.hip; the rows are chunk_rows.h's chunk_src
#include "augment_draw.h"  // aug_store, augment_draw_rows: the draw, shared with refine.hip

#pragma clang fp contract(off)

// one block per prompt group: statistics -> LDS, the n originals copied, then the block walks (k, t, d) of the K augmented rows in
// output order (coalesced stores)
template <typename T>
__global__ __launch_bounds__(256) void augment_k(cover_augment_args a, long long t_stride) {
    __shared__ float s_mean[6 * 64], s_s[6 * 64];
    __shared__ int s_jwin[64];
    const int g = blockIdx.x, n = a.n, K = a.K, h = a.h, w = 7 * h;
    T* out = (T*)a.out + (size_t)g * (n + K) * w;
    const aug_fit<T> f = {chunk_src_of<T>(a, t_stride, (long long)g * n), a.n, a.h, a.sigma, a.sd_floor, a.mean_out, a.sd_out, a.votes_out};
    augment_group_stats<T>(f, g, s_mean, s_s, s_jwin);
    chunk_gather_rows(f.src, n, w, out, [](int r) { return r; });
    __syncthreads();
    augment_draw_rows<T>(f, out + (size_t)n * w, a.normals + (size_t)g * K * 6 * h, K, a.clip_lo, a.clip_hi, s_mean, s_s, s_jwin);
}

static bool augment_args_ok(const cover_augment_args* a) {
    if (a->G < 1 || a->n < 1 || a->n > 4096 || a->K < 0 || a->K > 4096 || a->h < 1 || a->h > 64) return false;
    if ((long long)a->G * (a->n + a->K) > (1ll << 20)) return false;
    if (!f32_ge(a->sigma, 0.0f) || !f32_ge(a->sd_floor, 0.0f)) return false;
    if (!(a->clip_lo <= a->clip_hi)) return false;
    return a->src && a->out && (a->K == 0 || a->normals);
}
hipError_t launch_augment_tokens(const cover_augment_args* a, hipStream_t st) {
    if (!augment_args_ok(a) || !token_form_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(augment_k<int64_t>, dim3(a->G), dim3(256), 0, st, *a, 7ll);
    return hipGetLastError();
}
hipError_t launch_augment_actions(const cover_augment_args* a, hipStream_t st) {
    if (!augment_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(augment_k<float>, dim3(a->G), dim3(256), 0, st, *a, a->t_stride);
    return hipGetLastError();
}
