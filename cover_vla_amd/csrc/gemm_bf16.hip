// bf16 GEMM for gfx950, the entry point: C[M,N] = epi(A[M,K] . W[N,K]^T). launch_gemm_bf16 asks the planner for a GemmPlan, hands it to the
// kernel family the plan names, and completes a split-K launch. No kernel lives here:
//   gemm_plan.hip    plan_gemm: which family, tile, grid and K split, and what completes it (host only)
//   gemm_pack.hip    the packed weight layout every family reads, its packers, the e4m3 row quantiser
//   gemm_stream.hip  weight streaming, M <= 64: gemm_skinny / gemm_skinny2 / gemm_skinny3 (GK_SKINNY*), launch_gemm_skinny_partial
//   gemm_tiled.hip   LDS-tiled: gemm_tiled / gemm_tiled_pc (GK_TILED / GK_TILED_PC)
//   gemm_v3.hip      self-loading 8-wave tiles (GK_V3)
//   gemm_fp8.hip     tiles on the MX-scaled fp8 matrix instruction (GK_F8_PC / GK_F8_V3)
//   gemm_reduce.hip  split-K completions: splitk_reduce / splitk_reduce_norm, the norm as its own launch
//   gemm_common.h    the epilogue shared by all of them, GemmPlan, launch_kernel, and the declarations of the launchers used here
#include <hip/hip_ext.h>
#include "common.h"
#include "kernels.h"
#include "gemm_common.h"

// the LDS-tiled kernels of a GK_TILED / GK_TILED_PC / GK_V3 / GK_F8_* plan
static hipError_t launch_tiles(const GemmPlan& p, const bf16_t* A, int lda, const bf16_t* Wp, void* C, int ldc, int M, int N, int K, int Kp,
                               const EpiDev& epi, float* partial, int variant, hipStream_t st) {
    // profiling: the GEMM kernel's own start / stop stamps; class 4 = LLM-sized weight matrix (prefill), 1 = ViT-sized, 7 = fp8 tiles
    const int tcls = (double)N * (double)Kp >= 16.0e6 ? 4 : 1;
    const double twork = 2.0 * (double)M * (double)N * (double)K;
    plan_hit(p.slot);
    if (p.kind == GK_F8_PC || p.kind == GK_F8_V3) return launch_gemm_fp8_tiled(p, epi, C, ldc, M, N, Kp, partial, twork, st);
    if (p.kind == GK_V3) {
        // an unsplit launch with a plain fp32 output IS one split-K slab: take the raw-slab epilogue (LDS-staged 16-byte stores of the fp32 sums;
        // the consumer -- the qkv fold of the attention launch -- rounds them exactly as it rounds a sum of slabs)
        if (p.S == 1 && epi.out_f32 && !epi.bias && !epi.residual && !epi.lscale && epi.act == ACT_NONE && epi.out_scale == 1.0f && !epi.glu &&
            !epi.norm_out && ldc == N)
            partial = (float*)C;
        return launch_gemm_v3(p, A, lda, Wp, C, ldc, M, N, Kp, epi, partial, tcls, twork, st);
    }
    return launch_gemm_tiled(p, A, lda, Wp, C, ldc, M, N, Kp, epi, partial, variant, tcls, twork, st);
}

hipError_t launch_gemm_bf16(const bf16_t* A, int lda, const bf16_t* Wp, void* C, int ldc, int M, int N, int K,
                            const cover_gemm_epi* epi_in, float* ws, size_t ws_bytes, int variant, hipStream_t st, int* splits_out) {
    if (splits_out) *splits_out = 0;
    const EpiDev epi = make_epi(epi_in);
    GemmPlan p;
    hipError_t e = plan_gemm(p, lda, C, ldc, M, N, K, epi, ws, ws_bytes, variant, splits_out != nullptr);
    if (e != hipSuccess || p.kind == GK_NONE) return e;
    const int Kp = (K + 127) / 128 * 128;
    float* partial = p.S > 1 ? ws : nullptr;
    switch (p.kind) {
        case GK_SKINNY3: e = launch_skinny3(p.p3, A, lda, Wp, C, ldc, M, N, Kp, epi, partial, st); break;
        case GK_SKINNY2: e = launch_skinny2(p.p2, A, lda, Wp, ws, M, N, K, Kp, epi.w8, epi.w8s, epi.w8_kl, st); break;
        case GK_SKINNY: e = launch_skinny1(p, A, lda, Wp, ws, M, N, K, Kp, st); break;
        default: e = launch_tiles(p, A, lda, Wp, C, ldc, M, N, K, Kp, epi, partial, variant, st); break;
    }
    if (e != hipSuccess) return e;
    if (p.done == GD_SLABS) {
        *splits_out = p.S;
        return e;
    }
    return complete_splitk(p, epi, ws, C, ldc, M, N, st);
}
