// Beam search pieces (cover_beam_merge, cover_beam_merge_gumbel, cover_kv_gather_slots, cover_beam_backtrack): the merge of the B x B continuations of a prompt
// group, the slot-to-slot copy of each parent's own-token K/V into its child's slot, and the walk back through the parents.
// Conventions of sample.hip / select.hip: a bad host argument is hipErrorInvalidValue; nothing a device buffer holds can take a load or a
// store out of bounds (a bad slot or parent skips its row); every result is a fixed function of the inputs -- no atomics, the one sort has
// unique keys; every store is a per-lane vector store.
#include "common.h"
#include "kernels.h"
#include "keysort.h"

// ---------------------------------------------------------------------------------------------------
// merge: one block per group, a bitonic sort of the B * B candidates (padded to a power of two n2 <= 4096) in LDS on 64-bit keys
//   key = (descending-order image of the fp32 score) << 32 | (b * B + j)        a dead candidate: all ones
// The low half makes every key unique and IS the tie rule (lower b, then lower j), so the network's result does not depend on how it is
// scheduled. 78 compare-exchange stages at n2 = 4096 against B * B * B * B comparisons for a rank by counting (16.7 M at B = 64).
// KEYED (cover_beam_merge_gumbel): the score is the stored cand_g in place of cum + cand_lp, it is written to g_out, and the key behind
// the B kept ones is the group's kappa. cover_beam_merge runs the same kernel on its own fields, cand_g / g_out / kappa_out unset.
// ---------------------------------------------------------------------------------------------------
template <bool KEYED>
__global__ __launch_bounds__(1024) void beam_merge_k(cover_beam_merge_gumbel_args a, int n2) {
    __shared__ unsigned long long key[4096];
    const int B = a.B, g = blockIdx.x;
    const long long row0 = (long long)g * B;
    for (int c = threadIdx.x; c < n2; c += blockDim.x) {
        unsigned long long k = ~0ull;
        if (c < B * B) {
            const int b = c / B, j = c - b * B;
            const float cum = a.cum[row0 + b];
            const float lp = a.cand_lp[(row0 + b) * a.ld_lp + j];
            const long long tk = a.cand_tok[(row0 + b) * a.ld_tok + j];
            float score = cum + lp;
            bool live = finite_f(cum) && finite_f(lp) && tk >= 0;
            if constexpr (KEYED) {
                score = a.cand_g[(row0 + b) * a.ld_g + j];
                live = live && finite_f(score);
            }
            if (live) k = ((unsigned long long)desc_key(score) << 32) | (unsigned)c;
        }
        key[c] = k;
    }
    __syncthreads();
    bitonic_sort_lds(key, n2);
    for (int r = threadIdx.x; r < B; r += blockDim.x) {
        const unsigned long long k = key[r];
        int parent = -1;
        long long tok = -1, feed = a.feed_pad;
        float cum = -INFINITY, lp = -INFINITY, gk = -INFINITY;
        if (k != ~0ull) {
            const int c = (int)(unsigned)k;            // < B * B: written above from a live candidate
            parent = c / B;
            const int j = c - parent * B;
            lp = a.cand_lp[(row0 + parent) * a.ld_lp + j];
            tok = a.cand_tok[(row0 + parent) * a.ld_tok + j];
            cum = a.cum[row0 + parent] + lp;
            feed = tok;
            if constexpr (KEYED) gk = a.cand_g[(row0 + parent) * a.ld_g + j];
        }
        a.parent_out[row0 + r] = parent;
        a.token_out[row0 + r] = tok;
        a.feed_out[row0 + r] = feed;
        a.cum_out[row0 + r] = cum;
        a.step_lp_out[row0 + r] = lp;
        if constexpr (KEYED) a.g_out[row0 + r] = gk;
    }
    if constexpr (KEYED) {
        if (threadIdx.x == 0 && a.kappa_out) {         // n2 > B: n2 >= 2 and n2 >= B * B
            const unsigned long long k = key[B];
            float kappa = -INFINITY;
            if (k != ~0ull) {
                const int c = (int)(unsigned)k, b = c / B;
                kappa = a.cand_g[(row0 + b) * a.ld_g + (c - b * B)];
            }
            a.kappa_out[g] = kappa;
        }
    }
}
template <bool KEYED>
static hipError_t launch_merge(const cover_beam_merge_gumbel_args& a, hipStream_t st) {
    if (a.groups < 0 || a.B < 1 || a.B > 64 || a.ld_tok < a.B || a.ld_lp < a.B || a.feed_pad < 0) return hipErrorInvalidValue;
    if (!a.cum || !a.cand_tok || !a.cand_lp || !a.parent_out || !a.token_out || !a.feed_out || !a.cum_out || !a.step_lp_out)
        return hipErrorInvalidValue;
    if (KEYED && (!a.cand_g || !a.g_out || a.ld_g < a.B)) return hipErrorInvalidValue;
    if (a.cum == a.cum_out) return hipErrorInvalidValue;
    if (a.groups == 0) return hipSuccess;
    int n2 = 2;
    while (n2 < a.B * a.B) n2 <<= 1;
    const int threads = n2 / 2 < 64 ? 64 : (n2 / 2 > 1024 ? 1024 : n2 / 2);
    hipLaunchKernelGGL(beam_merge_k<KEYED>, dim3(a.groups), dim3(threads), 0, st, a, n2);
    return hipGetLastError();
}
hipError_t launch_beam_merge(const cover_beam_merge_args* a, hipStream_t st) {
    cover_beam_merge_gumbel_args b{};
    b.cum = a->cum; b.cand_tok = a->cand_tok; b.ld_tok = a->ld_tok; b.cand_lp = a->cand_lp; b.ld_lp = a->ld_lp;
    b.feed_pad = a->feed_pad; b.groups = a->groups; b.B = a->B;
    b.parent_out = a->parent_out; b.token_out = a->token_out; b.feed_out = a->feed_out; b.cum_out = a->cum_out; b.step_lp_out = a->step_lp_out;
    return launch_merge<false>(b, st);
}
hipError_t launch_beam_merge_gumbel(const cover_beam_merge_gumbel_args* a, hipStream_t st) { return launch_merge<true>(*a, st); }

// ---------------------------------------------------------------------------------------------------
// gather: block (row, layer, part) copies 16-byte chunks of one slot of one layer. K [slot][t][Hkv][D]: the n_t token rows are ONE run of
// n_t * Hkv * D elements at the head of the slot, copied exactly. V^T [slot][Hkv][D][cap]: the first ceil(n_t / 8) chunks of each of the
// Hkv * D rows -- up to 7 columns past n_t, inside the destination slot (cap is a multiple of 8).
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kv_gather_slots_k(cover_kv_gather_slots_args a, int nk, int nvc) {
    const int row = blockIdx.x, layer = blockIdx.y;
    const int src = a.src_slot[row], dst = a.dst_slot[row];
    if (src < 0 || src >= a.n_slots || dst < 0 || dst >= a.n_slots || src == dst) return;
    const bf16_t* kb = (const bf16_t*)a.k_base[layer];
    const bf16_t* vb = (const bf16_t*)a.vt_base[layer];
    if (!kb || !vb || (((uintptr_t)kb | (uintptr_t)vb) & 15)) return;
    const uint4* ks = (const uint4*)(kb + a.k_offset + (long long)src * a.k_slot_stride);
    uint4* kd = (uint4*)((bf16_t*)kb + a.k_offset + (long long)dst * a.k_slot_stride);
    const bf16_t* vs = vb + a.vt_offset + (long long)src * a.vt_slot_stride;
    bf16_t* vd = (bf16_t*)vb + a.vt_offset + (long long)dst * a.vt_slot_stride;
    const int nv = a.Hkv * a.D * nvc;
    for (int i = blockIdx.z * 256 + threadIdx.x; i < nk + nv; i += 256 * gridDim.z) {
        if (i < nk) {
            kd[i] = ks[i];
        } else {
            const int v = i - nk, r = v / nvc, c = v - r * nvc;
            const long long o = (long long)r * a.cap + 8 * c;
            *(uint4*)(vd + o) = *(const uint4*)(vs + o);
        }
    }
}
hipError_t launch_kv_gather_slots(const cover_kv_gather_slots_args* a, hipStream_t st) {
    if (!a->k_base || !a->vt_base || !a->src_slot || !a->dst_slot) return hipErrorInvalidValue;
    if (a->n_layers < 1 || a->n_layers > 65535 || a->rows < 0 || a->n_slots < 1 || a->Hkv < 1 || a->D < 1 || a->cap < 8 || (a->cap & 7))
        return hipErrorInvalidValue;
    const long long hd = (long long)a->Hkv * a->D, slot = hd * a->cap;
    if ((hd & 7) || slot >= (1ll << 31) || a->n_t < 0 || a->n_t > a->cap) return hipErrorInvalidValue;
    if (a->k_offset < 0 || a->vt_offset < 0 || ((a->k_offset | a->vt_offset | a->k_slot_stride | a->vt_slot_stride) & 7) ||
        a->k_slot_stride < slot || a->vt_slot_stride < slot)
        return hipErrorInvalidValue;   // 16-byte chunks (the allocations themselves are aligned far beyond that)
    if (a->rows == 0 || a->n_t == 0) return hipSuccess;
    const int nk = (int)(a->n_t * hd / 8), nvc = (a->n_t + 7) / 8;
    const long long chunks = nk + hd * nvc;
    const int parts = (int)(chunks / 2048 < 1 ? 1 : (chunks / 2048 > 8 ? 8 : chunks / 2048));
    hipLaunchKernelGGL(kv_gather_slots_k, dim3(a->rows, a->n_layers, parts), dim3(256), 0, st, *a, nk, nvc);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// backtrack: one thread per final beam, a chain of `steps` dependent loads (7 for an OpenVLA action)
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void beam_backtrack_k(cover_beam_backtrack_args a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const int g = r / a.B;
    int cur = r - g * a.B;
    for (int s = a.steps - 1; s >= 0; --s) {
        long long tok = -1;
        float lp = -INFINITY;
        if (cur >= 0) {
            const long long i = (long long)s * a.rows + (long long)g * a.B + cur;
            tok = a.token[i];
            lp = a.step_lp[i];
            const int p = a.parent[i];
            cur = (p >= 0 && p < a.B) ? p : -1;
        }
        a.tokens_out[(long long)r * a.steps + s] = tok;
        a.logprobs_out[(long long)r * a.steps + s] = lp;
    }
}
hipError_t launch_beam_backtrack(const cover_beam_backtrack_args* a, hipStream_t st) {
    if (!a->parent || !a->token || !a->step_lp || !a->tokens_out || !a->logprobs_out) return hipErrorInvalidValue;
    if (a->steps < 1 || a->rows < 0 || a->B < 1 || a->rows % a->B != 0) return hipErrorInvalidValue;
    if (a->rows == 0) return hipSuccess;
    hipLaunchKernelGGL(beam_backtrack_k, dim3((a->rows + 255) / 256), dim3(256), 0, st, *a);
    return hipGetLastError();
}
