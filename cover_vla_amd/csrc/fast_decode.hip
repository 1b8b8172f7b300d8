// pi0-FAST de-tokeniser (cover_fast_decode): generated PaliGemma ids -> FAST ids -> the pieces' code points -> quantised DCT coefficients
// -> one fp32 action chunk [H][D] per row. One 256-thread block per row: the first terminator is a block-wide minimum, the symbols'
// places come from a block-wide exclusive scan of the pieces' lengths (wave64 shuffles, LDS across the four waves, a running carry when
// L exceeds the block), every thread copies its own piece into the coefficient slots in LDS, and one thread per (t, d) runs the IDCT
// chain over k. The expansion is integer arithmetic, so no order enters it; the IDCT is one fixed chain per output. The results are
// compared with a numpy restatement as bit patterns: contraction is off for the whole file.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

#define FAST_THREADS 256
#define FAST_WAVES (FAST_THREADS / WAVE)
#define FAST_MAX_L 4096
#define FAST_MAX_H 128
#define FAST_MAX_D 32
#define FAST_LDS_BUDGET (64 * 1024)   // c and, where it fits beside it, the basis

// Fatal bits: a row that carries one of them decodes to zeros (the reference's `except: zeros`)
#define FAST_FATAL (COVER_FAST_MISMATCH | COVER_FAST_STRAY | COVER_FAST_UNDECODABLE)

__device__ __forceinline__ bool fast_id_in(long long t, const long long* ids, int n) {
    bool hit = false;
    for (int i = 0; i < n; ++i) hit = hit || t == ids[i];
    return hit;
}

// inclusive scan of v over the wave's lanes
__device__ __forceinline__ int fast_wave_scan(int v, int lane) {
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    return v;
}

// LDS: H * D floats (the coefficients: their int32 bits first, then c), then H * H floats of the basis when basis_lds
__global__ __launch_bounds__(FAST_THREADS) void fast_decode_k(cover_fast_decode_args a, int basis_lds) {
    extern __shared__ float s_lds[];
    __shared__ int s_stop[FAST_WAVES], s_tot[FAST_WAVES], s_flag[FAST_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x, L = a.L, H = a.H, D = a.D, HD = H * D;
    float* s_c = s_lds;
    float* s_b = s_lds + HD;
    const int64_t* tok = a.tokens + (long long)b * a.tok_row_stride;

    for (int i = tid; i < HD; i += FAST_THREADS) s_c[i] = __int_as_float(0);
    if (basis_lds)
        for (int i = tid; i < H * H; i += FAST_THREADS) s_b[i] = a.basis[i];

    // ---- 1. the first terminator
    int stop = L;
    for (int p = tid; p < L; p += FAST_THREADS)
        if (fast_id_in(tok[(long long)p * a.tok_step_stride], a.stop_ids, a.n_stop)) stop = min(stop, p);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) stop = min(stop, __shfl_xor(stop, o));
    if (lane == 0) s_stop[wv] = stop;
    __syncthreads();                       // also: the zeroed coefficients are in place
    stop = s_stop[0];
#pragma unroll
    for (int w = 1; w < FAST_WAVES; ++w) stop = min(stop, s_stop[w]);
    int flags = stop == L ? COVER_FAST_NO_TERMINATOR : 0;   // the same in every thread

    // ---- 2, 3, 4. classify, scan, copy the pieces
    int carry = 0;                         // symbols of the positions before this pass
    for (int p0 = 0; p0 < stop; p0 += FAST_THREADS) {
        const int p = p0 + tid;
        int len = 0, first = 0;
        if (p < stop) {
            const long long t = tok[(long long)p * a.tok_step_stride];
            const long long f = a.band_hi - 1 - t;          // in the band: 0 <= f < band_hi - band_lo
            if (t >= a.band_lo && t < a.band_hi && f < a.n_pieces) {
                first = a.piece_off[f];
                len = a.piece_off[f + 1] - first;
                if (len > 0 && a.piece_sym[first] < 0) {
                    flags |= COVER_FAST_UNDECODABLE;
                    len = 0;
                }
                len = max(len, 0);
            } else if (!fast_id_in(t, a.skip_ids, a.n_skip)) {
                flags |= COVER_FAST_STRAY;
            }
        }
        const int incl = fast_wave_scan(len, lane);
        if (lane == WAVE - 1) s_tot[wv] = incl;
        __syncthreads();
        int off = carry + incl - len, total = 0;
#pragma unroll
        for (int w = 0; w < FAST_WAVES; ++w) {
            if (w < wv) off += s_tot[w];
            total += s_tot[w];
        }
        carry += total;
        // (unsigned: a sum that left the int range, which the caller's limit excludes, writes nothing instead of out of bounds)
        for (int j = 0; j < len && (unsigned)(off + j) < (unsigned)HD; ++j) s_c[off + j] = __int_as_float(a.piece_sym[first + j] + a.min_token);
        __syncthreads();                   // s_tot is rewritten by the next pass
    }
    const int n = carry;

    // ---- the row's status
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o);
    if (lane == 0) s_flag[wv] = flags;
    __syncthreads();                       // also: every piece is in its slots
#pragma unroll
    for (int w = 0; w < FAST_WAVES; ++w) flags |= s_flag[w];
    if (a.relaxed) flags |= n > HD ? COVER_FAST_TRUNCATED : n < HD ? COVER_FAST_PADDED : 0;
    else if (n != HD) flags |= COVER_FAST_MISMATCH;
    const bool zeroed = (flags & FAST_FATAL) != 0;
    if (tid == 0) {
        if (a.n_symbols) a.n_symbols[b] = n;
        if (a.status) a.status[b] = flags;
    }

    // ---- 5, 6, 8a. the coefficients, and c = q / scale in their place
    for (int i = tid; i < HD; i += FAST_THREADS) {
        const int q = zeroed ? 0 : __float_as_int(s_c[i]);
        if (a.coeff_out) a.coeff_out[(size_t)b * HD + i] = q;
        s_c[i] = (float)q / a.scale;
    }
    __syncthreads();

    // ---- 8b. the IDCT: one chain over k per (t, d)
    const float* basis = basis_lds ? s_b : a.basis;
    float* out = a.out + (long long)b * a.out_n_stride;
    for (int i = tid; i < HD; i += FAST_THREADS) {
        const int t = i / D, d = i - t * D;
        const float* row = basis + t * H;
        float acc = 0.0f;
        for (int k = 0; k < H; ++k) {
            const float prod = row[k] * s_c[k * D + d];
            acc = acc + prod;
        }
        out[(long long)t * a.out_t_stride + d] = acc;
    }
}

static bool fast_decode_args_ok(const cover_fast_decode_args* a) {
    if (a->B < 1 || a->B > (1 << 20) || a->L < 1 || a->L > FAST_MAX_L) return false;
    if (a->H < 1 || a->H > FAST_MAX_H || a->D < 1 || a->D > FAST_MAX_D || a->n_pieces < 1) return false;
    if (a->band_lo < 0 || a->band_hi < a->band_lo) return false;
    if (a->n_stop < 0 || a->n_stop > 4 || a->n_skip < 0 || a->n_skip > 8) return false;
    if (a->min_token < -(1 << 30) || a->min_token > (1 << 30)) return false;
    if (!(a->scale - a->scale == 0.0f) || a->scale == 0.0f) return false;          // finite and != 0
    if (a->relaxed != 0 && a->relaxed != 1) return false;
    if (a->tok_row_stride < 0 || a->tok_step_stride < 0) return false;
    if (a->out_t_stride < a->D) return false;
    if (a->B > 1) {                        // out_n_stride >= (H - 1) * out_t_stride + D, without forming a product that could overflow
        const long long gap = a->out_n_stride - a->D;
        if (gap < 0 || (a->H > 1 && gap / (a->H - 1) < a->out_t_stride)) return false;
    }
    return a->tokens && a->piece_off && a->piece_sym && a->basis && a->out;
}
hipError_t launch_fast_decode(const cover_fast_decode_args* a, hipStream_t st) {
    if (!fast_decode_args_ok(a)) return hipErrorInvalidValue;
    const size_t c_bytes = (size_t)a->H * a->D * sizeof(float), b_bytes = (size_t)a->H * a->H * sizeof(float);   // <= 16 KiB, <= 64 KiB
    const int basis_lds = c_bytes + b_bytes <= FAST_LDS_BUDGET;
    const size_t lds = c_bytes + (basis_lds ? b_bytes : 0);
    hipLaunchKernelGGL(fast_decode_k, dim3(a->B), dim3(FAST_THREADS), lds, st, *a, basis_lds);
    return hipGetLastError();
}
