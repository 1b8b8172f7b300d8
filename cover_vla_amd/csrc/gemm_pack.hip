// Weight packers of the GEMM kernels and the e4m3 row quantiser.
//
// Weight layout (cover_pack_weight_bf16): Wp[nb = n/16][kb = k/32][lane = (n%16) + 16*((k%32)/8)][8 bf16]
//   -> one 16x32 block = 1 KiB contiguous = exactly the MFMA operand of one wave, lane-linear.
// Operands are SWAPPED (first MFMA operand = weight fragment, second = activation fragment), so the
// accumulator of lane (r = lane&15, g = lane>>4) holds C[m = r][n = 4g .. 4g+3]: four consecutive output
// columns per lane -> 8/16-byte epilogue stores, bias/residual loads are vector loads too.
// A GLU weight is packed with gate and up blocks interleaved (block 2i = gate rows, 2i+1 = the matching up rows). The kernels of
// gemm_tiled.hip, gemm_stream.hip, gemm_v3.hip and gemm_reduce.hip rely on this layout; the e4m3 images are described further down.
#include <hip/hip_ext.h>
#include "common.h"
#include "kernels.h"
#include "gemm_common.h"

// ---------------------------------------------------------------------------------------------------
// Weight packing: W[N, ldw] row-major -> fragment-major. One thread per 16-B chunk of the packed image.
// ---------------------------------------------------------------------------------------------------
__global__ void pack_weight(const bf16_t* __restrict__ W, int ldw, int N, int K, bf16_t* __restrict__ Wp, int Kp,
                            int glu) {
    const int K32 = Kp >> 5;
    const int N16 = (N + 15) >> 4;
    const long long total = (long long)N16 * K32 * 64;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(idx & 63);
        const long long blk = idx >> 6;
        const int kb = (int)(blk % K32);
        const int nb = (int)(blk / K32);
        int n = nb * 16 + (lane & 15);
        if (glu) {  // packed block 2i = gate rows [16i,16i+16), block 2i+1 = up rows N/2 + [16i,16i+16)
            const int half = N >> 1;
            const int i = nb >> 1;
            n = ((nb & 1) ? half : 0) + i * 16 + (lane & 15);
            if (i * 16 + (lane & 15) >= half) n = N;  // out of range -> zeros
        }
        const int k = kb * 32 + (lane >> 4) * 8;
        bf16_t v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (n < N && k + e < K) ? W[(size_t)n * ldw + k + e] : (bf16_t)0;
        *(uint4*)(Wp + idx * 8) = *(const uint4*)v;
    }
}

// ---------------------------------------------------------------------------------------------------
// e4m3 weights (BASELINE config 5). Per OUTPUT CHANNEL scale s_n = the smallest power of two with max_k |W[n,k]| / s_n <= 448
// (the e4m3 maximum); q = RNE_e4m3(W / s_n). A power-of-two scale makes (a) the division exact, (b) s_n * q exactly
// representable in bf16 (3 mantissa bits of e4m3 inside bf16's 7) -- so the SAME quantised weight exists as an e4m3 image for
// the HBM-bound weight-streaming kernels (half the bytes) and as a bf16 image for the MFMA-bound tiled kernels, and both
// give bit-identical GEMM results (products and sums just scale by 2^e).
//   quantize_rows_fp8_k : W bf16 [N, ldw] -> scales[N] fp32, Wdq bf16 [N, ldw] (= s_n * q, the de-quantised twin)
//   pack_weight_fp8_k   : Wdq + scales -> packed e4m3 image [n/16][k/64][lane = n%16 + 16*((k%32)/8)][16 B = the lane's 8-wide k run
//                         of the two 32-deep steps of the 64-block] and the scales in PACKED channel order
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantize_rows_fp8_k(const bf16_t* __restrict__ W, int ldw, int K, float* __restrict__ scales,
                                                           bf16_t* __restrict__ Wdq) {
    __shared__ float red[16];
    const int n = blockIdx.x;
    const bf16_t* w = W + (size_t)n * ldw;
    float mx = 0.f;
    for (int k = threadIdx.x; k < K; k += blockDim.x) mx = fmaxf(mx, fabsf(bf2f(w[k])));
    mx = block_max(mx, red);
    // smallest power of two s with mx / s <= 448: s = 2^ceil(log2(mx / 448)); frexp gives mx / 448 = f * 2^e with f in [0.5, 1)
    float s = 1.0f;
    if (mx > 0.f) {
        int e;
        const float f = frexpf(mx / 448.0f, &e);
        s = ldexpf(1.0f, f == 0.5f ? e - 1 : e);
    }
    if (threadIdx.x == 0) scales[n] = s;
    const float inv = 1.0f / s;   // exact (power of two)
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float x = bf2f(w[k]) * inv;
        const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(x, 0.0f, 0, false);      // RNE to OCP e4m3 (gfx950)
        const f32x2_t back = __builtin_amdgcn_cvt_pk_f32_fp8((uint32_t)pk, false);
        Wdq[(size_t)n * ldw + k] = f2bf(back[0] * s);                           // exact: e4m3 value times a power of two
    }
}

__global__ void pack_weight_fp8_k(const bf16_t* __restrict__ Wdq, int ldw, const float* __restrict__ scales, int N, int K,
                                  uint8_t* __restrict__ Wq, float* __restrict__ scales_packed, int Kp, int glu, int kl) {
    const int K64 = Kp >> 6;
    const int N16 = (N + 15) >> 4;
    const long long total = (long long)N16 * K64 * 64;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int lane = (int)(idx & 63);
        const long long blk = idx >> 6;
        const int kb = (int)(blk % K64);
        const int nb = (int)(blk / K64);
        int n = nb * 16 + (lane & 15);
        if (glu) {  // packed block 2i = gate rows [16i,16i+16), block 2i+1 = up rows N/2 + [16i,16i+16)  (as pack_weight)
            const int half = N >> 1, i = nb >> 1;
            n = ((nb & 1) ? half : 0) + i * 16 + (lane & 15);
            if (i * 16 + (lane & 15) >= half) n = N;
        }
        const float s = n < N ? scales[n] : 1.0f, inv = 1.0f / s;
        if (kb == 0 && (lane >> 4) == 0) scales_packed[nb * 16 + (lane & 15)] = s;
        uint32_t o[4];
#pragma unroll
        for (int half_ = 0; half_ < 2; ++half_) {      // k32 step 0 / 1 of the 64-block
            // default image: the lane's 8-wide runs of the two 32-deep steps of the 64-block; k-linear image: the lane's 16 consecutive k of the block
            const int k = kl ? kb * 64 + (lane >> 4) * 16 + half_ * 8 : kb * 64 + half_ * 32 + (lane >> 4) * 8;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (n < N && k + e < K) ? bf2f(Wdq[(size_t)n * ldw + k + e]) * inv : 0.f;
            int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
            int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
            o[2 * half_] = (uint32_t)lo;
            o[2 * half_ + 1] = (uint32_t)hi;
        }
        *(uint4*)(Wq + idx * 16) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

hipError_t launch_quantize_rows_fp8(const bf16_t* W, int ldw, int N, int K, float* scales, bf16_t* Wdq, hipStream_t st) {
    if (N <= 0) return hipSuccess;
    hipLaunchKernelGGL(quantize_rows_fp8_k, dim3(N), dim3(256), 0, st, W, ldw, K, scales, Wdq);
    return hipGetLastError();
}
hipError_t launch_pack_weight_fp8(const bf16_t* Wdq, int ldw, const float* scales, int N, int K, uint8_t* Wq, float* scales_packed,
                                  int Kpad, int glu, hipStream_t st, int kl) {
    const long long total = (long long)((N + 15) / 16) * (Kpad / 64) * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(pack_weight_fp8_k, dim3(blocks), dim3(256), 0, st, Wdq, ldw, scales, N, K, Wq, scales_packed, Kpad, glu, kl);
    return hipGetLastError();
}

hipError_t launch_pack_weight_bf16(const bf16_t* W, int ldw, int N, int K, bf16_t* Wp, int Kpad, int glu,
                                   hipStream_t st) {
    const long long total = (long long)((N + 15) / 16) * (Kpad / 32) * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(pack_weight, dim3(blocks), dim3(256), 0, st, W, ldw, N, K, Wp, Kpad, glu);
    return hipGetLastError();
}
