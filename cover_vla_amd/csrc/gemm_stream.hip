// Weight-streaming bf16 GEMM kernels for gfx950 (M <= 64: decode / denoise steps; GK_SKINNY / GK_SKINNY2 / GK_SKINNY3 plans). HBM-bound:
// the activation K-chunk lives in LDS in fragment-major form (xs[k-step][m-fragment][lane][16 B]) and every wave streams whole 1 KiB weight
// blocks of the packed layout (top of gemm_pack.hip) straight into VGPRs, with no LDS round trip for the streamed operand. Operands SWAPPED:
// lane (r = lane&15, g = lane>>4) holds C[m = r][n = 4g .. 4g+3]. The e4m3 weight twin (W8) is 1 KiB per 16 n x 64 k block.
//
//   gemm_skinny   first generation: split-K over grid.y, fp32 partials [S][M][N] (tools/bench_kernels.py, variant 5)
//   gemm_skinny2  8 waves = NG n-groups x KS k-slices, KS-way LDS reduction, KS-times fewer grid-level slabs
//   gemm_skinny3  M <= 32, whole K per block through an LDS double buffer, fused epilogue (or raw slabs when split)
// Slabs are completed by gemm_reduce.hip or by the consumer (launch_gemm_skinny_partial). Compile-time switch here: COVER_SK_DEBUG
// (cover_sk_debug, stamps in gemm_skinny3).
#include <hip/hip_ext.h>
#include "common.h"
#include "kernels.h"
#include "gemm_common.h"

// k offset (inside a 64-aligned chunk) of the 8-wide run that lane group gg multiplies in 32-deep step kst. The bf16 image and the default e4m3
// image hold k = 32 kst + 8 gg there; the k-linear e4m3 image (cover_pack_weight_fp8_klinear: the 16 bytes of a lane in a 64-deep block are 16
// CONSECUTIVE k -- the matrix instruction's own k order, in which an MX block scale covers 32 neighbouring columns) holds k = 64 (kst / 2) + 16 gg + 8 (kst % 2).
template <bool W8>
__device__ __forceinline__ int x_run_k(int kst, int gg, int kl) {
    if constexpr (W8) return kl ? ((kst >> 1) << 6) + gg * 16 + (kst & 1) * 8 : kst * 32 + gg * 8;
    else return kst * 32 + gg * 8;
}

// MFMA weight fragment of 32-deep step u of a 256-deep item: bf16 items hold it as loaded; e4m3 items (16 bytes per lane = the
// 8-wide k runs of steps 2j and 2j + 1) are converted with v_cvt_scalef32_pk_bf16_fp8 (scale 1: exact, every e4m3 value is a
// bf16 value)
template <bool W8, int NLD>
__device__ __forceinline__ bf16x8 wfrag(const u32x4 (&v)[NLD], int u) {
    if constexpr (!W8) {
        return __builtin_bit_cast(bf16x8, v[u]);
    } else {
        const u32x4 q = v[u >> 1];
        const uint32_t lo = (u & 1) ? q.z : q.x, hi = (u & 1) ? q.w : q.y;
        uint32_t o[4];
        o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false));
        o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true));
        o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false));
        o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true));
        return __builtin_bit_cast(bf16x8, (u32x4){o[0], o[1], o[2], o[3]});
    }
}

// slab store of 4 consecutive columns of a split-K partial
__device__ __forceinline__ void slab_store4(float* o, const float (&v)[4], int n, int N) {
    if (n + 3 < N && ((((uintptr_t)o) & 15) == 0)) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int e = 0; e < 4; ++e)
            if (n + e < N) o[e] = v[e];
    }
}

// ---------------------------------------------------------------------------------------------------
// Weight-streaming kernel (M <= 64)
// ---------------------------------------------------------------------------------------------------
// grid = (ceil(N16 / nb_per_block), S); block = 512 threads (8 waves). LDS = MF*16 rows x KC x 2 B, fragment-major:
//   xs[ks][f][lane][16 B].  partial[s][m][n] fp32.
template <int MF>
__global__ __launch_bounds__(512) void gemm_skinny(const bf16_t* __restrict__ A, int lda,
                                                   const bf16_t* __restrict__ Wp, float* __restrict__ partial, int M,
                                                   int N, int Kp, int KC, int nb_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = blockIdx.y;
    const int k0 = s * KC;
    const int kc = min(KC, Kp - k0);  // multiple of 128
    const int K32 = Kp >> 5;
    const int N16 = (N + 15) >> 4;

    // ---- stage the activation chunk: coalesced 16-B reads along k, scattered into fragment-major LDS ----
    {
        const int cpr = kc >> 3;  // 16-B chunks per row
        const int total = MF * 16 * cpr;
        for (int c = tid; c < total; c += 512) {
            const int row = c / cpr, kc8 = c - row * cpr;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (row < M) v = *(const uint4*)(A + (size_t)row * lda + k0 + kc8 * 8);
            const int ks = kc8 >> 2, gg = kc8 & 3, f = row >> 4, rr = row & 15;
            *(uint4*)(smem + (((ks * MF + f) * 64) + rr + 16 * gg) * 16) = v;
        }
    }
    __syncthreads();

    const int nb_begin = blockIdx.x * nb_per_block;
    const int nb_end = min(N16, nb_begin + nb_per_block);
    const int nbatch = kc >> 7;  // batches of 4 k-steps (128 k)
    const int r = lane & 15, g = lane >> 4;

    // One continuous stream over (n-block, k-batch): loads run two batches (8 KiB per wave) ahead and keep flowing
    // across n-block boundaries, so the HBM pipe never drains while a wave finishes one block of output columns.
    const int n_nb = (nb_end - nb_begin - w + 7) / 8;  // n-blocks of this wave: nb_begin + w + 8*i
    const int total = n_nb > 0 ? n_nb * nbatch : 0;
    const u32x4* wbase = (const u32x4*)(Wp + ((size_t)(nb_begin + w) * K32 + (k0 >> 5)) * 512) + lane;
    const size_t nb_stride = (size_t)8 * K32 * 64;  // u32x4 units between consecutive n-blocks of this wave
    f32x4 acc[MF];
#pragma unroll
    for (int f = 0; f < MF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    u32x4 b0[4], b1[4], b2[4];
    auto load4 = [&](u32x4(&dst)[4], int fidx) {
        const int i = fidx / nbatch, b = fidx - i * nbatch;
        const u32x4* src = wbase + (size_t)i * nb_stride + (size_t)b * 4 * 64;
#pragma unroll
        for (int u = 0; u < 4; ++u) dst[u] = __builtin_nontemporal_load(src + u * 64);
    };
    auto comp4 = [&](u32x4(&src)[4], int fidx) {
        const int i = fidx / nbatch, b = fidx - i * nbatch;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ks = b * 4 + u;
            const bf16x8 wf = __builtin_bit_cast(bf16x8, src[u]);
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const bf16x8 xf = as_bf16x8(*(const uint4*)(smem + ((ks * MF + f) * 64 + lane) * 16));
                acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[f], 0, 0, 0);
            }
        }
        if (b == nbatch - 1) {  // finished this n-block's K-slice: partial[s][m][n], lane holds m = f*16 + r, n = nb*16 + 4g..
            const int nb = nb_begin + w + 8 * i;
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const int m = f * 16 + r;
                const int n = nb * 16 + 4 * g;
                if (m < M && n < N) {
                    const float v[4] = {acc[f][0], acc[f][1], acc[f][2], acc[f][3]};
                    slab_store4(partial + ((size_t)s * M + m) * N + n, v, n, N);
                }
                acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    };
    if (total > 0) load4(b0, 0);
    if (total > 1) load4(b1, 1);
    for (int fi = 0; fi < total; fi += 3) {
        if (fi + 2 < total) load4(b2, fi + 2);
        comp4(b0, fi);
        if (fi + 1 < total) {
            if (fi + 3 < total) load4(b0, fi + 3);
            comp4(b1, fi + 1);
        }
        if (fi + 2 < total) {
            if (fi + 4 < total) load4(b1, fi + 4);
            comp4(b2, fi + 2);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Weight-streaming kernel, second generation: the 8 waves of a block are NG n-groups x KS k-slices. A wave streams
// NBW n-blocks over ITS 256-wide k-slice of the block's K chunk (KC = 256*KS, staged once in LDS), keeps one
// accumulator set per n-block, and the KS slices are summed through LDS at the end. Same parallelism as the first
// generation with KS-times fewer grid-level K splits => KS-times less fp32 partial traffic for the reduce kernel.
// ---------------------------------------------------------------------------------------------------
template <int MF, int KS, int NBW, bool W8 = false>
__global__ __launch_bounds__(512) void gemm_skinny2(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ Wp,
                                                    float* __restrict__ partial, int M, int N, int Kp, const float* __restrict__ wscale, int kl) {
    constexpr int NG = 8 / KS, KC = 256 * KS, NBPB = NG * NBW;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ks = w % KS, ng = w / KS;
    const int s = blockIdx.y;
    const int k0 = s * KC;
    const int kc = min(KC, Kp - k0);  // multiple of 128
    const int K32 = Kp >> 5;
    const int N16 = (N + 15) >> 4;
    const int nb_begin = blockIdx.x * NBPB;
    const int kw0 = ks * 256;               // this wave's k-slice inside the chunk
    const int nsteps = max(0, min(8, (kc - kw0) >> 5));
    f32x4 acc[NBW][MF];
#pragma unroll
    for (int i = 0; i < NBW; ++i)
#pragma unroll
        for (int f = 0; f < MF; ++f) acc[i][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    constexpr int NLD = W8 ? 4 : 8;               // 16-byte loads per lane per 256-deep item (see gemm_skinny3)
    auto wsrc = [&](int nb, int k) -> const u32x4* {
        if constexpr (W8) return (const u32x4*)((const uint8_t*)Wp + ((size_t)nb * (Kp >> 6) + (k >> 6)) * 1024) + lane;
        else return (const u32x4*)(Wp + ((size_t)nb * K32 + (k >> 5)) * 512) + lane;
    };
    u32x4 buf[2][NLD];
    auto load8 = [&](u32x4(&dst)[NLD], int i) {
        int nb = nb_begin + ng + NG * i;
        nb = nb < N16 ? nb : N16 - 1;
        const u32x4* src = wsrc(nb, k0 + kw0);
        if (nsteps == 8) {   // whole k-slice: straight-line issue (per-load branches cost ~20 % of the stream rate)
#pragma unroll
            for (int u = 0; u < NLD; ++u) dst[u] = __builtin_nontemporal_load(src + u * 64);
        } else {
#pragma unroll
            for (int u = 0; u < NLD; ++u)
                if (u * (8 / NLD) < nsteps) dst[u] = __builtin_nontemporal_load(src + u * 64);
        }
    };
    constexpr int NFR = (KC / 32) * MF;
    bool items_done = false;
    if (kc == KC && nsteps == 8 && NBW > 1) {
        // whole chunk, whole k-slice: the activation fragments are requested BEFORE the weight blocks (loads return in order:
        // behind the weights they would hold the first MFMA back until both blocks have landed), without per-element
        // conditions (rows beyond M re-read row M-1; their outputs are never stored)
        constexpr int XL = NFR / 8;
        uint4 xr[XL];
        const int rr = lane & 15, gg = lane >> 4;
#pragma unroll
        for (int j = 0; j < XL; ++j) {
            const int fi = j * 8 + w, kst = fi / MF, f = fi - kst * MF;
            int row = f * 16 + rr;
            row = row < M ? row : M - 1;
            xr[j] = *(const uint4*)(A + (size_t)row * lda + k0 + x_run_k<W8>(kst, gg, kl));
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int nb = nb_begin + ng + NG * i;
            nb = nb < N16 ? nb : N16 - 1;
            const u32x4* src = wsrc(nb, k0 + kw0);
#pragma unroll
            for (int u = 0; u < NLD; ++u) buf[i][u] = __builtin_nontemporal_load(src + u * 64);
        }
#pragma unroll
        for (int j = 0; j < XL; ++j) *(uint4*)(smem + (j * 8 + w) * 1024 + lane * 16) = xr[j];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS-only: the weight blocks stay in flight
        // the items straight-line as well (fixed step count, unconditional refills): s_waitcnt then counts the younger block
        // still in flight instead of draining both before the first MFMA
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bf16x8 wf = wfrag<W8>(buf[i & 1], u);
                const int kst = (kw0 >> 5) + u;
#pragma unroll
                for (int f = 0; f < MF; ++f) {
                    const bf16x8 xf = as_bf16x8(*(const uint4*)(smem + ((kst * MF + f) * 64 + lane) * 16));
                    acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[i][f], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (i + 2 < NBW) {
                int nb = nb_begin + ng + NG * (i + 2);
                nb = nb < N16 ? nb : N16 - 1;
                const u32x4* src = wsrc(nb, k0 + kw0);
#pragma unroll
                for (int u = 0; u < NLD; ++u) buf[i & 1][u] = __builtin_nontemporal_load(src + u * 64);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        items_done = true;
    } else {
        load8(buf[0], 0);  // the first two weight blocks are in flight while the activation chunk is staged
        if (NBW > 1) load8(buf[1], 1);
        {   // stage the activation chunk (fragment-major), zero beyond kc: wave w moves fragments fi = w, w + 8, ... (fi =
            // kst*MF + f); lane (rr, gg) owns row f*16 + rr, k = kst*32 + gg*8 -> lane-linear, conflict-free LDS stores
            const int rr = lane & 15, gg = lane >> 4;
#pragma unroll 4
            for (int fi = w; fi < NFR; fi += 8) {
                const int kst = fi / MF, f = fi - kst * MF;
                const int row = f * 16 + rr, kk = x_run_k<W8>(kst, gg, kl);
                uint4 v = make_uint4(0, 0, 0, 0);
                if (row < M && kk < kc) v = *(const uint4*)(A + (size_t)row * lda + k0 + kk);
                *(uint4*)(smem + fi * 1024 + lane * 16) = v;
            }
        }
        __syncthreads();
    }
    auto comp8 = [&](u32x4(&src)[NLD], f32x4(&a)[MF]) {
        auto step = [&](int u) {
            const bf16x8 wf = wfrag<W8>(src, u);
            const int kst = (kw0 >> 5) + u;
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const bf16x8 xf = as_bf16x8(*(const uint4*)(smem + ((kst * MF + f) * 64 + lane) * 16));
                a[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, a[f], 0, 0, 0);
            }
        };
        if (nsteps == 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) step(u);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < nsteps) step(u);
        }
    };
    if (!items_done) {
#pragma unroll
        for (int i = 0; i < NBW; ++i) {
            comp8(buf[i & 1], acc[i]);
            if (i + 2 < NBW) load8(buf[i & 1], i + 2);  // refill the buffer just consumed: two blocks stay in flight
        }
    }
    // ---- sum the KS k-slices through LDS (the X chunk is dead now), RB n-blocks per round (<= 64 KiB of LDS) ----
    constexpr int RB = (8 / MF) < NBW ? (8 / MF) : NBW;
    const int r = lane & 15, g = lane >> 4;
    float* red = (float*)smem;  // [w][ii][f][4][64]
#pragma unroll
    for (int i0 = 0; i0 < NBW; i0 += RB) {
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < RB; ++ii)
            if (i0 + ii < NBW) {
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int e = 0; e < 4; ++e) red[(((w * RB + ii) * MF + f) * 4 + e) * 64 + lane] = acc[(i0 + ii) < NBW ? (i0 + ii) : 0][f][e];
            }
        __syncthreads();
        constexpr int NFRAG = NG * RB * MF;
        for (int j = w; j < NFRAG; j += 8) {
            const int f = j % MF, ii = (j / MF) % RB, gsel = j / (MF * RB);
            if (i0 + ii >= NBW) continue;
            const int nb = nb_begin + gsel + NG * (i0 + ii);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int ww = gsel * KS + kk;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += red[(((ww * RB + ii) * MF + f) * 4 + e) * 64 + lane];
            }
            const int m = f * 16 + r, n = nb * 16 + 4 * g;
            if constexpr (W8) {   // per-channel power-of-two scale (packed channel order): exact in fp32, commutes with the slab sum
                const float4 sc = *(const float4*)(wscale + (size_t)(nb < N16 ? nb : N16 - 1) * 16 + 4 * g);
                v[0] *= sc.x; v[1] *= sc.y; v[2] *= sc.z; v[3] *= sc.w;
            }
            if (nb < N16 && m < M && n < N) slab_store4(partial + ((size_t)s * M + m) * N + n, v, n, N);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Weight-streaming kernel, third generation (M <= 32): NO grid-level split-K. A block owns NG*NBW n-blocks for the WHOLE
// K range, so the output leaves through the fused epilogue (bias / activation / GLU / residual, bf16 or fp32) and the
// fp32 partial slabs plus the splitk_reduce launch disappear. The activation panel does not fit LDS at once
// (32 x 4096 bf16 = 256 KiB): it is streamed in KC-wide chunks through a DOUBLE buffer -- the global loads of chunk c+1
// are issued before chunk c's MFMAs and written to the other buffer after them, one barrier per chunk -- while the
// weight stream (NBUF x 8 KiB per wave in flight, non-temporal) runs across chunk boundaries without draining.
// Waves: NG n-groups x KS k-slices of 256 inside every chunk, accumulators live across chunks, KS-way LDS reduction at
// the end as in the second generation. grid = ceil(N16 / (NG*NBW)).
// ---------------------------------------------------------------------------------------------------
#ifdef COVER_SK_DEBUG
__device__ unsigned long long g_sk_dbg[1024 * 4];   // per block: start, chunk 0 staged, last MFMA done, end (100 MHz wall clock)
extern "C" int cover_sk_debug(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_sk_dbg), sizeof(g_sk_dbg));
}
#define SKT(slot) do { if (threadIdx.x == 0) g_sk_dbg[((blockIdx.y * gridDim.x + blockIdx.x) & 1023) * 4 + (slot)] = wall_clock64(); } while (0)
#else
#define SKT(slot) do { } while (0)
#endif
template <int MF, int KS, int NBW, int NBUF, bool W8 = false>
__global__ __launch_bounds__(512) void gemm_skinny3(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ Wp,
                                                    void* C, int ldc, int M, int N, int Kp, EpiDev epi,
                                                    float* __restrict__ partial, int kper, const float* __restrict__ wscale, int kl) {
    SKT(0);
    constexpr int NG = 8 / KS, KC = 256 * KS, NBPB = NG * NBW;
    constexpr int XB = MF * 16 * KC * 2;          // bytes of one activation chunk (fragment-major)
    constexpr int XL = XB / (512 * 16);           // 16-B loads per thread per chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][XB]; the reduction buffer aliases it at the end
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ks = w % KS, ng = w / KS;
    const int K32 = Kp >> 5;
    const int N16 = (N + 15) >> 4;
    const int nb_begin = blockIdx.x * NBPB;
    // optional grid-level split-K (narrow outputs: n-blocks alone cannot fill the chip): slice s = blockIdx.y owns
    // k in [kb, ke) and leaves raw fp32 partial sums [s][M][N] for the reduction / the fused decode attention
    const int kb = blockIdx.y * kper;
    const int ke = min(Kp, kb + kper);
    const int nchunks = (ke - kb + KC - 1) / KC;
    const int kw0 = ks * 256;                     // this wave's k-slice inside every chunk
    f32x4 acc[NBW][MF];
#pragma unroll
    for (int i = 0; i < NBW; ++i)
#pragma unroll
        for (int f = 0; f < MF; ++f) acc[i][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // weight stream: item t = (chunk c = t / NBW, n-block i = t % NBW) -> 8 x 1 KiB (this wave's 256 k of that chunk)
    const int items = nchunks * NBW;
    auto steps_of = [&](int c) { return max(0, min(8, (min(KC, ke - kb - c * KC) - kw0) >> 5)); };
    // W8: e4m3 weights (cover_pack_weight_fp8: 1 KiB per 16 n x 64 k block, a lane's 16 bytes = its 8-wide k runs of two
    // consecutive 32-deep steps): half the bytes per item, de-quantised to bf16 fragments in registers (exact), the
    // power-of-two per-channel scale applied to the fp32 sums after the k-slice reduction (exact)
    constexpr int NLD = W8 ? 4 : 8;               // 16-byte loads per lane per 256-deep item
    auto wsrc = [&](int nb, int k) -> const u32x4* {
        if constexpr (W8) return (const u32x4*)((const uint8_t*)Wp + ((size_t)nb * (Kp >> 6) + (k >> 6)) * 1024) + lane;
        else return (const u32x4*)(Wp + ((size_t)nb * K32 + (k >> 5)) * 512) + lane;
    };
    u32x4 buf[NBUF][NLD];
    auto load8 = [&](u32x4(&dst)[NLD], int t) {
        const int c = t / NBW, i = t - c * NBW;
        int nb = nb_begin + ng + NG * i;
        nb = nb < N16 ? nb : N16 - 1;
        const int nst = steps_of(c);
        const u32x4* src = wsrc(nb, kb + c * KC + kw0);
        if (nst == 8) {   // whole k-slice (every chunk but a ragged last one): straight-line issue
#pragma unroll
            for (int u = 0; u < NLD; ++u) dst[u] = __builtin_nontemporal_load(src + u * 64);
        } else {
#pragma unroll
            for (int u = 0; u < NLD; ++u)
                if (u * (8 / NLD) < nst) dst[u] = __builtin_nontemporal_load(src + u * 64);
        }
    };
    // activation chunk staging through registers: wave w moves fragments fi = j*8 + w (fi = kst*MF + f); lane
    // (rr, gg) = (lane & 15, lane >> 4) owns the 16 bytes of row f*16 + rr, k = kst*32 + gg*8, so the LDS image of a
    // fragment is lane-linear and a wave's 16-byte stores are one contiguous KiB (a row-major thread map lands 16 lanes
    // of every store on one bank)
    static_assert(XL * 8 == (KC / 32) * MF, "fragments must split evenly over the waves");
    uint4 xr[XL];
    const int srr = lane & 15, sgg = lane >> 4;
    auto x_load = [&](int c) {
        const int k0 = kb + c * KC, kc = min(KC, ke - k0);
#pragma unroll
        for (int j = 0; j < XL; ++j) {
            const int fi = j * 8 + w, kst = fi / MF, f = fi - kst * MF;
            const int row = f * 16 + srr, kk = x_run_k<W8>(kst, sgg, kl);
            xr[j] = make_uint4(0, 0, 0, 0);
            if (row < M && kk < kc) xr[j] = *(const uint4*)(A + (size_t)row * lda + k0 + kk);
        }
    };
    auto x_write = [&](int b) {
#pragma unroll
        for (int j = 0; j < XL; ++j) *(uint4*)(smem + b * XB + (j * 8 + w) * 1024 + lane * 16) = xr[j];
    };
    auto comp8 = [&](u32x4(&src)[NLD], f32x4(&a)[MF], int c) {
        const int nst = steps_of(c);
        const char* xb = smem + (c & 1) * XB;
        auto step = [&](int u) {
            const bf16x8 wf = wfrag<W8>(src, u);
            const int kst = (kw0 >> 5) + u;
#pragma unroll
            for (int f = 0; f < MF; ++f) {
                const bf16x8 xf = as_bf16x8(*(const uint4*)(xb + ((kst * MF + f) * 64 + lane) * 16));
                a[f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, a[f], 0, 0, 0);
            }
        };
        if (nst == 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) step(u);
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < nst) step(u);
        }
    };

    // prologue. The activation chunk is requested BEFORE the first NBUF weight items: loads return in order, so with the
    // weights first the chunk (and with it the first MFMA, and with that the first REFILL of a weight buffer) would wait for
    // all NBUF x 8 KiB per wave to land -- the stream would drain its whole initial window before issuing anything new.
    if (items >= NBUF && min(KC, ke - kb) == KC) {   // straight-line: the compiler counts the weight loads behind the chunk's
        {   // whole first chunk: no per-element conditions (rows beyond M re-read row M-1; their outputs are never stored)
#pragma unroll
            for (int j = 0; j < XL; ++j) {
                const int fi = j * 8 + w, kst = fi / MF, f = fi - kst * MF;
                int row = f * 16 + srr;
                row = row < M ? row : M - 1;
                xr[j] = *(const uint4*)(A + (size_t)row * lda + kb + x_run_k<W8>(kst, sgg, kl));
            }
        }
#pragma unroll
        for (int b = 0; b < NBUF; ++b) {
            int nb = nb_begin + ng + NG * b;
            nb = nb < N16 ? nb : N16 - 1;
            const u32x4* src = wsrc(nb, kb + kw0);
#pragma unroll
            for (int u = 0; u < NLD; ++u) buf[b][u] = __builtin_nontemporal_load(src + u * 64);
        }
        x_write(0);
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS-only: the weight items stay in flight
        SKT(1);
    } else {
#pragma unroll
        for (int b = 0; b < NBUF; ++b)
            if (b < items) load8(buf[b], b);
        x_load(0);
        x_write(0);
        __syncthreads();
    }
    // Steady state: chunk c is full and so is chunk c+1. Everything in the body is straight-line (unconditional loads, fixed
    // step counts), so the compiler's s_waitcnt before the first MFMA of an item counts exactly the loads issued after that
    // item's (two younger items + the next activation chunk stay in flight). With the refill behind an `if`, it emitted
    // vmcnt(0) at every item: the wave drained its whole window 3-4 times per chunk.
    int c0 = 0;
    if (items >= NBUF && min(KC, ke - kb) == KC) {
        const bool last_full = ((ke - kb) % KC) == 0;
        const int nfast = last_full ? nchunks - 1 : nchunks - 2;   // chunks whose successor is a full chunk
        for (; c0 < nfast; ++c0) {
            const int k1 = kb + (c0 + 1) * KC;
#pragma unroll
            for (int j = 0; j < XL; ++j) {
                const int fi = j * 8 + w, kst = fi / MF, f = fi - kst * MF;
                int row = f * 16 + srr;
                row = row < M ? row : M - 1;
                xr[j] = *(const uint4*)(A + (size_t)row * lda + k1 + x_run_k<W8>(kst, sgg, kl));
            }
            __builtin_amdgcn_sched_barrier(0);   // (the scheduler otherwise hoists the first MFMAs of all items and sinks the refills)
            const char* xb = smem + (c0 & 1) * XB;
#pragma unroll
            for (int i = 0; i < NBW; ++i) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bf16x8 wf = wfrag<W8>(buf[i % NBUF], u);
                    const int kst = (kw0 >> 5) + u;
#pragma unroll
                    for (int f = 0; f < MF; ++f) {
                        const bf16x8 xf = as_bf16x8(*(const uint4*)(xb + ((kst * MF + f) * 64 + lane) * 16));
                        acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[i][f], 0, 0, 0);
                    }
                }
                int nb = nb_begin + ng + NG * i;
                nb = nb < N16 ? nb : N16 - 1;
                const u32x4* src = wsrc(nb, k1 + kw0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < NLD; ++u) buf[i % NBUF][u] = __builtin_nontemporal_load(src + u * 64);
                __builtin_amdgcn_sched_barrier(0);
            }
            x_write((c0 + 1) & 1);
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
        if (last_full && c0 == nchunks - 1) {   // the last chunk, full: the same straight-line items without refills
            const char* xb = smem + (c0 & 1) * XB;
#pragma unroll
            for (int i = 0; i < NBW; ++i) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const bf16x8 wf = wfrag<W8>(buf[i % NBUF], u);
                    const int kst = (kw0 >> 5) + u;
#pragma unroll
                    for (int f = 0; f < MF; ++f) {
                        const bf16x8 xf = as_bf16x8(*(const uint4*)(xb + ((kst * MF + f) * 64 + lane) * 16));
                        acc[i][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[i][f], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            ++c0;
        }
    }
    // remaining chunks (ragged last chunk and its predecessor, or everything for short K): generic bookkeeping
    int t = c0 * NBW;
    for (int c = c0; c < nchunks; ++c) {
        if (c + 1 < nchunks) x_load(c + 1);            // lands underneath this chunk's weight stream
#pragma unroll
        for (int i = 0; i < NBW; ++i, ++t) {
            // buffer of item t is t % NBUF; NBW % NBUF == 0 keeps it static per i
            comp8(buf[i % NBUF], acc[i], c);
            if (t + NBUF < items) load8(buf[i % NBUF], t + NBUF);
        }
        if (c + 1 < nchunks) {
            x_write((c + 1) & 1);                      // the other buffer: nobody reads it during chunk c
            // chunk c+1 visible, chunk c's buffer free for c+2. LDS-only barrier: __syncthreads() would also drain
            // vmcnt, i.e. the NBUF weight items in flight, at every chunk boundary.
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
    }

    SKT(2);
    // ---- sum the KS k-slices through LDS, RB n-blocks per round, and leave through the fused epilogue ----
    constexpr int RB = (8 / MF) < NBW ? (8 / MF) : NBW;
    const int r = lane & 15, g = lane >> 4;
    float* red = (float*)smem;  // [w][ii][f][4][64]
#pragma unroll
    for (int i0 = 0; i0 < NBW; i0 += RB) {
        __syncthreads();
#pragma unroll
        for (int ii = 0; ii < RB; ++ii)
            if (i0 + ii < NBW) {
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int e = 0; e < 4; ++e) red[(((w * RB + ii) * MF + f) * 4 + e) * 64 + lane] = acc[(i0 + ii) < NBW ? (i0 + ii) : 0][f][e];
            }
        __syncthreads();
        auto slice_sum = [&](int gsel, int ii, int f, float (&v)[4]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 0.f;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int ww = gsel * KS + kk;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += red[(((ww * RB + ii) * MF + f) * 4 + e) * 64 + lane];
            }
            if constexpr (W8) {   // per-channel power-of-two scale (packed channel order): exact in fp32
                const int nbs = nb_begin + gsel + NG * (i0 + ii);
                const float4 sc = *(const float4*)(wscale + (size_t)(nbs < N16 ? nbs : N16 - 1) * 16 + 4 * g);
                v[0] *= sc.x; v[1] *= sc.y; v[2] *= sc.z; v[3] *= sc.w;
            }
        };
        if (partial) {   // split-K slice: raw sums, the epilogue belongs to whoever folds the slabs
            constexpr int NFRAG = NG * RB * MF;
            for (int j = w; j < NFRAG; j += 8) {
                const int f = j % MF, ii = (j / MF) % RB, gsel = j / (MF * RB);
                if (i0 + ii >= NBW) continue;
                const int nb = nb_begin + gsel + NG * (i0 + ii);
                const int m = f * 16 + r, n = nb * 16 + 4 * g;
                if (nb < N16 && m < M && n < N) {
                    float v[4];
                    slice_sum(gsel, ii, f, v);
                    slab_store4(partial + ((size_t)blockIdx.y * M + m) * N + n, v, n, N);
                }
            }
        } else if (epi.glu) {   // n-groups 0 / 1 hold the gate / up block of one output block (NG == 2, even nb_begin)
            constexpr int NFRAG = RB * MF;
            for (int j = w; j < NFRAG; j += 8) {
                const int f = j % MF, ii = j / MF;
                if (i0 + ii >= NBW) continue;
                const int nb = nb_begin + NG * (i0 + ii);   // gate block (even), up = nb + 1
                const int m = f * 16 + r;
                if (nb + 1 < N16 + (N16 & 1) && nb < N16 && m < M) {
                    float gv[4], uv[4];
                    slice_sum(0, ii, f, gv);
                    slice_sum(1, ii, f, uv);
                    epi_store4_glu(epi, C, ldc, m, (nb >> 1) * 16 + 4 * g, N >> 1, gv, uv);
                }
            }
        } else {
            constexpr int NFRAG = NG * RB * MF;
            for (int j = w; j < NFRAG; j += 8) {
                const int f = j % MF, ii = (j / MF) % RB, gsel = j / (MF * RB);
                if (i0 + ii >= NBW) continue;
                const int nb = nb_begin + gsel + NG * (i0 + ii);
                const int m = f * 16 + r;
                if (nb < N16 && m < M) {
                    float v[4];
                    slice_sum(gsel, ii, f, v);
                    epi_store4(epi, C, ldc, m, nb * 16 + 4 * g, N, v);
                }
            }
        }
    }
    SKT(3);
}

// ---------------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------------
// first-generation weight streaming
hipError_t launch_skinny1(const GemmPlan& p, const bf16_t* A, int lda, const bf16_t* Wp, float* ws, int M, int N, int K, int Kp, hipStream_t st) {
    plan_hit(PLAN_SKINNY);
    hipError_t e;
    switch (p.p1.MF) {
#define SK1(MF_) launch_kernel<gemm_skinny<MF_>>(sk_class(N, K), 2.0 * (double)N * (double)K, dim3(p.p1.gx, p.S), dim3(512), p.lds, st, A, lda, Wp, ws, M, N, Kp, \
                                                 p.p1.KC, p.p1.nbpb)
        case 1: e = SK1(1); break;
        case 2: e = SK1(2); break;
        case 3: e = SK1(3); break;
        default: e = SK1(4); break;
#undef SK1
    }
    if (e == hipSuccess) e = hipGetLastError();
    return e;
}

// second-generation weight streaming; e4m3 weights for M <= 32 when a twin is given
hipError_t launch_skinny2(const Skinny2Plan& p, const bf16_t* A, int lda, const bf16_t* Wp, float* ws, int M, int N, int K, int Kp,
                          const uint8_t* w8, const float* w8s, int kl, hipStream_t st) {
    const dim3 grid(p.gx, p.S), block(512);
    plan_hit(PLAN_SKINNY2);
#define SK2(MF_, KS_, NBW_, W8_) launch_kernel<gemm_skinny2<MF_, KS_, NBW_, W8_>>(sk_class(N, K), (W8_ ? 1.0 : 2.0) * (double)N * (double)K, grid, block, p.lds, st, \
                                                                                   A, lda, W8_ ? (const bf16_t*)w8 : Wp, ws, M, N, Kp, w8s, kl)
#define SK2_NBW(MF_, W8_) (p.NBW == 6 ? SK2(MF_, 4, 6, W8_) : p.NBW == 4 ? SK2(MF_, 4, 4, W8_) : p.NBW == 3 ? SK2(MF_, 4, 3, W8_) : SK2(MF_, 4, 2, W8_))
    hipError_t e;
    if (w8 && w8s && p.MF <= 2) e = p.MF == 1 ? SK2_NBW(1, true) : SK2_NBW(2, true);
    else if (p.MF == 1) e = SK2_NBW(1, false);
    else if (p.MF == 2) e = SK2_NBW(2, false);
    else if (p.MF == 3) e = SK2(3, 2, 2, false);
    else e = SK2(4, 2, 2, false);
#undef SK2_NBW
#undef SK2
    if (e == hipSuccess) e = hipGetLastError();
    return e;
}

// third-generation weight streaming; e4m3 weights when the epilogue carries a twin
hipError_t launch_skinny3(const Skinny3Plan& p, const bf16_t* A, int lda, const bf16_t* Wp, void* C, int ldc, int M, int N,
                          int Kp, const EpiDev& epi, float* partial, hipStream_t st) {
    const dim3 grid(p.gx, p.S), block(512);
    plan_hit(PLAN_SKINNY3);
#define SK3(MF_, NBW_, W8_) launch_kernel<gemm_skinny3<MF_, 4, NBW_, NBW_, W8_>>(sk_class(N, Kp), (W8_ ? 1.0 : 2.0) * (double)N * (double)Kp, grid, block, p.lds, st, \
                                                                                  A, lda, W8_ ? (const bf16_t*)epi.w8 : Wp, C, ldc, M, N, Kp, epi, partial, p.kper, epi.w8s, epi.w8_kl)
#define SK3_NBW(MF_, W8_) (p.NBW == 4 ? SK3(MF_, 4, W8_) : p.NBW == 3 ? SK3(MF_, 3, W8_) : SK3(MF_, 2, W8_))
    hipError_t e;
    if (epi.w8) e = p.MF == 1 ? SK3_NBW(1, true) : SK3_NBW(2, true);   // e4m3 weight stream
    else e = p.MF == 1 ? SK3_NBW(1, false) : SK3_NBW(2, false);
#undef SK3_NBW
#undef SK3
    if (e == hipSuccess) e = hipGetLastError();
    return e;
}

// Weight-streaming GEMM WITHOUT its reduction: leaves fp32 partials [S][M][N] in ws for a consumer that folds them
// (the decoder fuses the QKV reduction into rope_kv_write). Returns the number of K slices through *S_out.
hipError_t launch_gemm_skinny_partial(const bf16_t* A, int lda, const bf16_t* Wp, float* ws, size_t ws_bytes, int M, int N,
                                      int K, int* S_out, hipStream_t st, const void* w8, const float* w8s) {
    if (M <= 0 || M > 64 || N <= 0) return hipErrorInvalidValue;
    const int Kp = (K + 127) / 128 * 128;
    GemmPlan p = GemmPlan{};
    hipError_t e = plan_streaming(p, M, N, Kp, ws, ws_bytes, false, true);
    if (e != hipSuccess) return e;
    if (p.kind == GK_SKINNY3) {
        EpiDev none = make_epi(nullptr);
        if (w8 && w8s) { none.w8 = (const uint8_t*)w8; none.w8s = w8s; }
        e = launch_skinny3(p.p3, A, lda, Wp, nullptr, 0, M, N, Kp, none, ws, st);
    } else {
        e = launch_skinny2(p.p2, A, lda, Wp, ws, M, N, K, Kp, (const uint8_t*)w8, w8s, 0, st);
    }
    *S_out = p.S;
    return e;
}
