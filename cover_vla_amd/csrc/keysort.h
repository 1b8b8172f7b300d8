// Sorting by unique 64-bit keys in LDS, shared by beam.hip (the per-group merges) and sample.hip (cover_gumbel_topn):
//   key = (descending-order image of an fp32 score) << 32 | index        a dead entry: all ones
// The low half makes every key unique and IS the tie rule (lower index first), so the network's result does not depend on how it is scheduled.
#pragma once
#include "common.h"

__device__ __forceinline__ uint32_t desc_key(float s) {
    if (s == 0.0f) s = 0.0f;                                   // -0 and +0 are one score
    const uint32_t u = __float_as_uint(s);
    const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // larger float -> larger unsigned
    return ~asc;
}
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// Ascending bitonic sort of key[0, n2), n2 a power of two >= 2: log2(n2) (log2(n2) + 1) / 2 compare-exchange stages (36 at 256, 78 at
// 4096). Every thread of the block calls this after a barrier behind the last write of key; it returns behind a barrier.
__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* key, int n2) {
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n2 >> 1); t += blockDim.x) {
                const int i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), p = i | stride;
                const bool up = (i & size) == 0;
                const unsigned long long x = key[i], y = key[p];
                if ((x > y) == up) {
                    key[i] = y;
                    key[p] = x;
                }
            }
            __syncthreads();
        }
}
