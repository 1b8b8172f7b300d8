// Split-K completions of the GEMM kernels (GemmPlan.done): the fp32 slabs [S][M][N] that a tiled or weight-streaming launch left in the
// workspace are summed in slab order and leave through gemm_common.h's epilogue arithmetic (epi_value4 and its bf16 rounding points).
//
//   splitk_reduce       one thread per 4 output columns, every epilogue form (GLU: gate / up columns 16 apart, as the packed layout at the
//                       top of gemm_pack.hip interleaves them)
//   splitk_reduce_norm  one 512-thread block per output row, additionally writes norm_out = rmsnorm / layernorm of the bf16-rounded row
//                       (and its e4m3 twin): N % 8 == 0, N <= 8192, no GLU, bf16 output
// Compile-time switches, all here: COVER_RN_DEBUG (cover_rn_debug), COVER_RN_RES_EARLY, COVER_RN_BIAS_EARLY.
#include <hip/hip_ext.h>
#include "common.h"
#include "kernels.h"
#include "gemm_common.h"

// out = epi(sum_s partial[s]) AND norm_out = rmsnorm(out) / layernorm(out): one 512-thread block per output row
// (N % 8 == 0, N <= 8192, no GLU, bf16 output). The statistics are taken over the bf16-ROUNDED outputs, i.e. exactly what
// the separate norm kernel would read back, with that kernel's arithmetic.
// block sum of a 512-thread block through LDS with an LDS-ONLY barrier: __syncthreads() would also wait for the stores
// of C still in flight (their acknowledgement is ~1 us on the critical path of a kernel that lasts ~6). `red` is written
// once per call: a second call in the same kernel takes a different slice.
__device__ __forceinline__ float block_sum_lds(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i];
    return t;
}

#ifdef COVER_RN_DEBUG
__device__ unsigned long long g_rn_dbg[512 * 8];   // per block (thread 0): start, slabs landed, epilogue done, before / after the block sum, end
extern "C" int cover_rn_debug(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rn_dbg), sizeof(g_rn_dbg)); }
#define RNT(slot) do { if (threadIdx.x == 0) g_rn_dbg[(blockIdx.x & 511) * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define RNT(slot) do { } while (0)
#endif
#ifndef COVER_RN_RES_EARLY
#define COVER_RN_RES_EARLY 1   // 0 = the operand loads BEHIND the slab sums (rounds 1-5), for A/B builds
#endif
// (one row by one 512-thread block; red = 16 floats of LDS)
__device__ __forceinline__ void reduce_norm_row(const float* __restrict__ partial, int S, bf16_t* C, int ldc, int M, int N, const EpiDev& epi,
                                                const int m, float* red) {
    RNT(0);
    float vals[2][8];
    float q = 0.f;
    // the norm weights do not depend on anything: requested first, so their latency hides under the slab loads instead
    // of following the block reduction (the stores to C in between keep the compiler from hoisting them itself)
    float4 nw[2][2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n0 = (threadIdx.x + c * 512) * 8;
        if (n0 < N) {
            nw[c][0] = *(const float4*)(epi.norm_w + n0);
            nw[c][1] = *(const float4*)(epi.norm_w + n0 + 4);
        }
    }
    // Round 6: with a residual-only epilogue (decoder o_proj / down: x += slab sums, bf16 residual -- two of these launches per layer-step of
    // every decode pass) the residual chunk is requested in the SAME batch as the first slab loads instead of by epi_value4 behind the slab
    // sums: the kernel was two dependent memory round trips (slabs 1.1 us, residual 1.1 us of 3.6 us in the per-block timeline,
    // tools/dbg/rn_timeline.py), now one: 3.6 -> 2.6 us in-kernel, headline 34.31 -> 33.49 ms over three same-box alternations
    // (profiles/r06_reduce_residual_early_ab.txt). Same arithmetic and rounding points as epi_value4. A general form (bias / layer scale / fp32
    // residual requested early through uniform branches) measured NO gain on the same decision: the branches cost what the round trip saves.
    // (A round-2 note here said a 16-byte residual load AHEAD of the slabs had measured slower; behind the first slab batch it does not.)
    const bool res_only = COVER_RN_RES_EARLY != 0 && epi.residual && !epi.res_f32 && !epi.bias && !epi.lscale && epi.act == ACT_NONE && epi.out_scale == 1.0f &&
                          (N & 7) == 0 && (((uintptr_t)epi.residual) & 15) == 0 && ((epi.ldr * 2) & 15) == 0;
#ifndef COVER_RN_BIAS_EARLY
#define COVER_RN_BIAS_EARLY 1
#endif
    // the same for the ViT towers' proj / fc2 reductions (SigLIP, SigLIP2: bias + bf16 residual, no layer scale)
    const bool res_bias = COVER_RN_BIAS_EARLY != 0 && !res_only && epi.residual && !epi.res_f32 && epi.bias && !epi.lscale && epi.act == ACT_NONE &&
                          epi.out_scale == 1.0f && (N & 7) == 0 && (((uintptr_t)epi.residual) & 15) == 0 && ((epi.ldr * 2) & 15) == 0 &&
                          (((uintptr_t)epi.bias) & 15) == 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n0 = (threadIdx.x + c * 512) * 8;
        if (n0 < N) {
            float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            const float* p0 = partial + (size_t)m * N + n0;
            const size_t sstride = (size_t)M * N;
            uint4 rr = make_uint4(0, 0, 0, 0);
            float4 bq0 = make_float4(0.f, 0.f, 0.f, 0.f), bq1 = bq0;
            const bf16_t* rsrc = (const bf16_t*)epi.residual + (size_t)m * epi.ldr + n0;
            int s = 0;
            for (; s + 4 <= S; s += 4) {  // four slices in flight
                float4 a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = *(const float4*)(p0 + (s + j) * sstride);
                    b[j] = *(const float4*)(p0 + (s + j) * sstride + 4);
                }
                if (res_only && s == 0) rr = *(const uint4*)rsrc;
                if (res_bias && s == 0) { rr = *(const uint4*)rsrc; bq0 = *(const float4*)(epi.bias + n0); bq1 = *(const float4*)(epi.bias + n0 + 4); }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[0] += a[j].x; v[1] += a[j].y; v[2] += a[j].z; v[3] += a[j].w;
                    v[4] += b[j].x; v[5] += b[j].y; v[6] += b[j].z; v[7] += b[j].w;
                }
            }
            for (; s < S; ++s) {
                const float4 a = *(const float4*)(p0 + s * sstride), b = *(const float4*)(p0 + s * sstride + 4);
                if (res_only && s == 0) rr = *(const uint4*)rsrc;      // (fewer than four slabs)
                if (res_bias && s == 0) { rr = *(const uint4*)rsrc; bq0 = *(const float4*)(epi.bias + n0); bq1 = *(const float4*)(epi.bias + n0 + 4); }
                v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
            }
            if (c == 0) RNT(1);
            if (res_only) {   // epi_value4's arithmetic for a residual-only epilogue: bf16(sum) + residual
                const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] = bfround(v[2 * i]) + bf2f((bf16_t)(rw[i] & 0xffffu));
                    v[2 * i + 1] = bfround(v[2 * i + 1]) + bf2f((bf16_t)(rw[i] >> 16));
                }
            } else if (res_bias) {   // bf16(sum + bias) + residual
                const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
                const float bv[8] = {bq0.x, bq0.y, bq0.z, bq0.w, bq1.x, bq1.y, bq1.z, bq1.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[2 * i] = bfround(v[2 * i] + bv[2 * i]) + bf2f((bf16_t)(rw[i] & 0xffffu));
                    v[2 * i + 1] = bfround(v[2 * i + 1] + bv[2 * i + 1]) + bf2f((bf16_t)(rw[i] >> 16));
                }
            } else {
                epi_value4(epi, m, n0, N, v);
                epi_value4(epi, m, n0 + 4, N, v + 4);
            }
            if (c == 0) RNT(2);
            uint4 u;
            u.x = pack_bf2(v[0], v[1]); u.y = pack_bf2(v[2], v[3]); u.z = pack_bf2(v[4], v[5]); u.w = pack_bf2(v[6], v[7]);
            *(uint4*)(C + (size_t)m * ldc + n0) = u;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                vals[c][i] = bfround(v[i]);
                q += vals[c][i] * vals[c][i];
            }
        }
    }
    float mean = 0.f, rstd;
    if (epi.norm_style == 2) {   // LayerNorm (layernorm_bf16_k arithmetic: mean, then the centred second moment)
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if ((int)(threadIdx.x + c * 512) * 8 < N)
#pragma unroll
                for (int i = 0; i < 8; ++i) sum += vals[c][i];
        mean = block_sum_lds(sum, red) / N;
        float q2 = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if ((int)(threadIdx.x + c * 512) * 8 < N)
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float d = vals[c][i] - mean;
                    q2 += d * d;
                }
        rstd = rsqrtf(block_sum_lds(q2, red + 8) / N + epi.norm_eps);
    } else {
        RNT(3);
        rstd = rsqrtf(block_sum_lds(q, red) / N + epi.norm_eps);
        RNT(4);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n0 = (threadIdx.x + c * 512) * 8;
        if (n0 < N) {
            float o[8];
            const float wv[8] = {nw[c][0].x, nw[c][0].y, nw[c][0].z, nw[c][0].w, nw[c][1].x, nw[c][1].y, nw[c][1].z, nw[c][1].w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float ww = wv[i];
                if (epi.norm_style == 2) o[i] = (vals[c][i] - mean) * rstd * ww + (epi.norm_b ? epi.norm_b[n0 + i] : 0.f);
                else o[i] = epi.norm_style == 1 ? ww * bfround(vals[c][i] * rstd) : vals[c][i] * rstd * (epi.norm_w_offset + ww);
            }
            uint4 u;
            u.x = pack_bf2(o[0], o[1]); u.y = pack_bf2(o[2], o[3]); u.z = pack_bf2(o[4], o[5]); u.w = pack_bf2(o[6], o[7]);
            *(uint4*)(epi.norm_out + (size_t)m * epi.ld_norm_out + n0) = u;
            if (epi.nq8) {
#pragma unroll
                for (int i = 0; i < 8; ++i) vals[c][i] = bfround(o[i]);   // the stored bf16 row is what gets quantised
            }
        }
    }
    if (epi.nq8) {   // e4m3 twin of the norm_out row (cover_quantize_act_fp8's arithmetic on the stored bf16 values)
        float mx = 0.f;
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if ((int)(threadIdx.x + c * 512) * 8 < N)
#pragma unroll
                for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(vals[c][i]));
        mx = wave_max(mx);
        if ((threadIdx.x & 63) == 0) red[8 + (threadIdx.x >> 6)] = mx;     // (red[0..7] belong to the block sum above)
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) t = fmaxf(t, red[8 + i]);
        const float sc = e4m3_pow2_scale(t), inv = 1.0f / sc;
        if (threadIdx.x == 0) epi.nq8s[m] = sc;
        uint8_t* qrow = epi.nq8 + (size_t)m * epi.ldnq8;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int n0 = (threadIdx.x + c * 512) * 8;
            if (n0 < N) store_q8_chunk(qrow, n0, vals[c], inv);
        }
        // zero padding up to the row pitch's 128-multiple is the caller's (N % 128 == 0 for the decoder widths this serves)
    }
    RNT(5);
}
__global__ __launch_bounds__(512) void splitk_reduce_norm(const float* __restrict__ partial, int S, bf16_t* C, int ldc, int M,
                                                          int N, EpiDev epi) {
    __shared__ float red[16];
    reduce_norm_row(partial, S, C, ldc, M, N, epi, blockIdx.x, red);
}

// out = epi(sum_s partial[s]) ; one thread per 4 output columns
__global__ __launch_bounds__(256) void splitk_reduce(const float* __restrict__ partial, int S, void* C, int ldc, int M,
                                                     int N, EpiDev epi) {
    const int Nout = epi.glu ? (N >> 1) : N;
    const int groups = (Nout + 3) >> 2;
    const long long total = (long long)M * groups;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(idx / groups);
        const int j0 = (int)(idx - (long long)m * groups) * 4;
        if (epi.glu) {
            const int ng = (j0 >> 4) * 32 + (j0 & 15);  // gate columns; up = +16
            float gv[4] = {0, 0, 0, 0}, uv[4] = {0, 0, 0, 0};
            for (int s = 0; s < S; ++s) {
                const float* p = partial + ((size_t)s * M + m) * N + ng;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (j0 + i < Nout) {
                        gv[i] += p[i];
                        uv[i] += p[16 + i];
                    }
            }
            epi_store4_glu(epi, C, ldc, m, j0, Nout, gv, uv);
        } else {
            float v[4] = {0, 0, 0, 0};
            const float* p0 = partial + (size_t)m * N + j0;
            const size_t sstride = (size_t)M * N;
            if (j0 + 3 < N && ((((uintptr_t)p0) | (sstride * sizeof(float))) & 15) == 0) {
                // whole group of four columns: 16-byte loads, four slabs in flight (a rolled loop with guarded scalar loads is a
                // chain of S dependent round trips), summed in slab order
                int s = 0;
                for (; s + 4 <= S; s += 4) {
                    float4 a[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[j] = *(const float4*)(p0 + (s + j) * sstride);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { v[0] += a[j].x; v[1] += a[j].y; v[2] += a[j].z; v[3] += a[j].w; }
                }
                for (; s < S; ++s) {
                    const float4 a = *(const float4*)(p0 + s * sstride);
                    v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
                }
            } else {
                for (int s = 0; s < S; ++s) {
                    const float* p = partial + ((size_t)s * M + m) * N + j0;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (j0 + i < N) v[i] += p[i];
                }
            }
            epi_store4(epi, C, ldc, m, j0, N, v);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Host launchers
// ---------------------------------------------------------------------------------------------------
// the norm requested through the epilogue, as its own launch (paths that cannot fold it into a split-K reduction)
static hipError_t run_norm(const EpiDev& epi, void* C, int ldc, int M, int Nout, hipStream_t st) {
    if (epi.norm_style == 2)
        return launch_layernorm_bf16((const bf16_t*)C, ldc, epi.norm_w, epi.norm_b, epi.norm_out, epi.ld_norm_out, M, Nout, epi.norm_eps, st);
    return launch_rmsnorm(C, 0, ldc, epi.norm_w, epi.norm_w_offset, epi.norm_style, epi.norm_out, epi.ld_norm_out, M, Nout, epi.norm_eps, st,
                          epi.nq8, epi.ldnq8, epi.nq8s);
}

// the completion of a planned launch: the split-K reduction (with the norm folded in, or followed by its own norm launch)
hipError_t complete_splitk(const GemmPlan& p, const EpiDev& epi, const float* ws, void* C, int ldc, int M, int N, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (p.done == GD_REDUCE_NORM) {
        e = launch_kernel<splitk_reduce_norm>(p.rcls, 0.0, dim3(M), dim3(512), 0, st, ws, p.S, (bf16_t*)C, ldc, M, N, epi);
    } else if (p.done == GD_REDUCE) {
        const int Nout = epi.glu ? N / 2 : N;
        const long long total = (long long)M * ((Nout + 3) / 4);
        int rb = (int)((total + 255) / 256);
        if (rb > 2048) rb = 2048;
        e = launch_kernel<splitk_reduce>(p.rcls, 0.0, dim3(rb), dim3(256), 0, st, ws, p.S, C, ldc, M, N, epi);
    }
    if (e == hipSuccess && p.done != GD_NONE) e = hipGetLastError();
    if (e == hipSuccess && p.norm_launch) e = run_norm(epi, C, ldc, M, epi.glu ? N / 2 : N, st);
    return e;
}
