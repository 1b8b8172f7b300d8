// Filtered inverse-CDF token sampling over a wide logits row (temperature -> top-k -> top-p -> pick, the order of Hugging Face's
// logits warpers). One 1024-thread block per row, no workspace, nothing data-dependent in the launch: recordable into a hipGraph.
//
// Determinism and the summation order (the house rule of select.hip: a sum that decides an index has a fixed result).
//   Every mass in this file is an EXACT INTEGER sum. A token's weight w = expf((l - max) / T) (fp32, 0 <= w <= 1) is converted once to
//   Q43 fixed point, q = rint(w * 2^43) (exact for w >= 2^-19, rounded to the nearest 2^-43 below that), and all masses -- total,
//   per-bin, per-tile, running -- are uint64 sums of q. hi - lo <= 2^20 terms of at most 2^43 cannot overflow 2^63. Integer
//   addition is associative, so the order in which lanes and waves add (LDS integer atomics) cannot change a result; there is no
//   floating-point sum anywhere. Error against exact arithmetic on the same fp32 weights: at most 2^-44 per term, 2^-24 of the
//   mass for 2^20 terms (the kept mass is >= 2^43: the row maximum has w = 1 and every filter keeps it). Thresholds are
//   compared as integers: top-p keeps the shortest prefix with mass >= ceil(top_p * M) (double product of the fp32 top_p and the
//   uint64 M); the pick is the first kept index whose running mass is >= floor(u * M_kept) + 1.
//   Counts are integers as well. Selections (k-th largest logit, the top-p cut, the index of the pick) are radix selections:
//   a histogram (count and mass per bin, LDS integer atomics) over one digit of an order-preserving 32-bit key, then one wave walks
//   the bins in key order -- lane j owns a contiguous run of bins, runs are combined with an inclusive shuffle scan, the lane that
//   holds the crossing walks its run -- and the next digit repeats this inside the chosen bin. Keys: the logit's bits mapped to
//   an unsigned order (top-k: a comparison of input floats, no arithmetic), the weight's bits (top-p; equal weights by ascending
//   index), the column index (pick; its first digit -- the mass of each tile of 1024 columns -- is reduced per wave with shuffles on the row).
//   Candidates: when the first digit shows that at most 4096 elements lie at or above the bin holding the threshold, those elements
//   are compacted into LDS (in whatever order the atomics grant; every consumer is one of the order-independent integer
//   reductions above) and the remaining digits run over that list instead of the row: a language model's row needs two or three
//   passes over its 1 MB, a flat row (cut in the tail, huge k) falls back to one pass per digit.
//   Top-n and entropy (token_topn_k): the ranks are one more radix selection, over the logit keys restricted to the kept set (count
//   only), ties at the n-th rank cut by the index walk of the top-p tie; the at most 64 selected entries are ordered by one wave.
//   The entropy H = -sum p_i log p_i over the kept set, with p_i = w_i / W and x_i = (l_i - max) / T = log w_i, is
//   log W + (sum w_i * -x_i) / W. The second sum is integer as well: S = sum rint(w_i * -x_i * 2^43), the fp32 product (<= 1/e)
//   converted once as q43 converts a weight; 2^20 terms below 2^42 cannot overflow. H = fp32(log(M / 2^43) + S / M) in double, once
//   per row, M the Q43 kept mass. Error: M as above; each term of S carries the fp32 rounding of x (twice), of expf and of the product.
#include "common.h"
#include "kernels.h"
#include "keysort.h"

typedef unsigned long long u64;
#define SMP_BINS 2048
#define SMP_CAP 4096
#define SMP_T 1024

struct SampleShared {
    unsigned cnt[SMP_BINS];
    u64 mass[SMP_BINS];
    float list_l[SMP_CAP];
    int list_i[SMP_CAP];
    float red[16];
    unsigned n_list;
    // result of scan_bins
    int r_bin;
    unsigned r_cnt_before, r_cnt_bin, r_cnt_total;
    u64 r_mass_before, r_mass_bin, r_mass_total, r_need;
};

// order-preserving image of a float: a > b  <=>  lkey(a) > lkey(b) (-0 == +0)
__device__ __forceinline__ unsigned lkey(float l) {
    unsigned u = __float_as_uint(l);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float weight_of(float l, float m, float t) {
    const float w = expf((l - m) / t);
    return (w == w) ? w : 0.f;
}
// order-preserving key of a weight (>= 0): its bits without the sign bit, so the first digit spans 8 exponent + 3 mantissa bits
__device__ __forceinline__ unsigned wkey(float w) { return __float_as_uint(w) << 1; }
__device__ __forceinline__ u64 q43(float w) { return (u64)__float2ull_rn(w * 8796093022208.0f); }

__device__ __forceinline__ u64 shfl_up64(u64 v, int o) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl_up(lo, o);
    hi = __shfl_up(hi, o);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int l) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl(lo, l);
    hi = __shfl(hi, l);
    return ((u64)hi << 32) | lo;
}
// the sum of v over the 64 lanes of a wave, in every lane (exact: integers)
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        lo = __shfl_xor(lo, o);
        hi = __shfl_xor(hi, o);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}

// The elements a stage iterates: columns [0, n) of the row (rel = column - lo), or the compacted candidates in LDS.
template <bool ALLOW>
struct SampleSrcT {
    const float* p;   // row + lo
    int n;
    bool list;
    static constexpr bool allow = false;
};
// The allowed variant (cover_token_*_rows_allowed): the row restricted to the columns whose bit is set in the row's allow set. A column
// whose bit is clear never reaches a per-element functor, so counts, masses, the candidate list and the tile digit see allowed
// columns only; the compacted list holds allowed elements and needs no mask afterwards.
template <>
struct SampleSrcT<true> {
    const float* p;
    int n;
    bool list;
    const unsigned* bits;   // the row's set: bit (c & 31) of word (c >> 5) for the ABSOLUTE column c
    int lo;                 // column of rel 0
    int cnt;                // allowed columns in [lo, hi): what n is wherever n is a count
    int first;              // rel of the first allowed column
    static constexpr bool allow = true;
};
typedef SampleSrcT<false> SampleSrc;
typedef SampleSrcT<true> SampleSrcAllow;

// the number of elements a filter can keep: the columns of the range, or the allowed ones among them
template <class Src>
__device__ __forceinline__ int src_count(const Src& src) {
    if constexpr (Src::allow) return src.cnt;
    else return src.n;
}
// is column rel allowed (one word read)
template <class Src>
__device__ __forceinline__ bool allow1(const Src& src, int rel) {
    if constexpr (Src::allow) {
        const unsigned a = (unsigned)(src.lo + rel);
        return (src.bits[a >> 5] >> (a & 31u)) & 1u;
    } else {
        return true;
    }
}
// bits 0..3: are columns rel .. rel + 3 allowed (all four inside the range). lo and the alignment head are arbitrary, so the four may
// straddle a word: the covering word, and the next one only then, are read once for the group.
template <class Src>
__device__ __forceinline__ unsigned allow4(const Src& src, int rel) {
    if constexpr (Src::allow) {
        const unsigned a = (unsigned)(src.lo + rel), sh = a & 31u;
        const unsigned* w = src.bits + (a >> 5);
        unsigned m = w[0] >> sh;
        if (sh > 28u) m |= w[1] << (32u - sh);
        return m & 15u;
    } else {
        return 15u;
    }
}

// What a row function is handed next to the range: nothing, or the row's set as allow_row found it.
template <bool ALLOW>
struct AllowRow {};
template <>
struct AllowRow<true> {
    const unsigned* bits;
    int cnt, first;
};
template <bool ALLOW>
__device__ __forceinline__ SampleSrcT<ALLOW> make_src(const float* p, int n, int lo, const AllowRow<ALLOW>& ar) {
    if constexpr (ALLOW) return SampleSrcT<true>{p, n, false, ar.bits, lo, ar.cnt, ar.first};
    else return SampleSrcT<false>{p, n, false};
}

// f(logit, rel) for every element. Row: scalar head up to the first 16-byte boundary, float4 body (four loads in flight per lane),
// scalar tail -- any lo / ld works, aligned rows take the vector path. One walk for both sources: without a set allow1 / allow4 are the
// constants true / 15, so the unmasked instantiation carries no test.
template <class Src, class F>
__device__ __forceinline__ void for_each(const SampleShared& s, const Src& src, F f) {
    const int tid = threadIdx.x;
    if (src.list) {
        const int nl = (int)s.n_list;
        for (int c = tid; c < nl; c += SMP_T) f(s.list_l[c], s.list_i[c]);
        return;
    }
    const float* p = src.p;
    const int n = src.n;
    int head = (int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
    head = head < n ? head : n;
    for (int c = tid; c < head; c += SMP_T)
        if (allow1(src, c)) f(p[c], c);
    const int n4 = (n - head) >> 2;
    const float4* v = (const float4*)(p + head);
    auto take = [&](const float4& x, unsigned m, int c) {
        const int i0 = head + 4 * c;
        if (m & 1u) f(x.x, i0);
        if (m & 2u) f(x.y, i0 + 1);
        if (m & 4u) f(x.z, i0 + 2);
        if (m & 8u) f(x.w, i0 + 3);
    };
    int c = tid;
    for (; c + 3 * SMP_T < n4; c += 4 * SMP_T) {   // the mask words of a group are loaded with its float4, all in flight together
        const unsigned m0 = allow4(src, head + 4 * c), m1 = allow4(src, head + 4 * (c + SMP_T)),
                       m2 = allow4(src, head + 4 * (c + 2 * SMP_T)), m3 = allow4(src, head + 4 * (c + 3 * SMP_T));
        const float4 x0 = v[c], x1 = v[c + SMP_T], x2 = v[c + 2 * SMP_T], x3 = v[c + 3 * SMP_T];
        take(x0, m0, c); take(x1, m1, c + SMP_T); take(x2, m2, c + 2 * SMP_T); take(x3, m3, c + 3 * SMP_T);
    }
    for (; c < n4; c += SMP_T) {
        const unsigned m = allow4(src, head + 4 * c);
        take(v[c], m, c);
    }
    for (int t = head + 4 * n4 + tid; t < n; t += SMP_T)
        if (allow1(src, t)) f(p[t], t);
}
// the same for rel in [r0, r1) only
template <class Src, class F>
__device__ __forceinline__ void for_each_in(const SampleShared& s, const Src& src, int r0, int r1, F f) {
    const int tid = threadIdx.x;
    if (src.list) {
        const int nl = (int)s.n_list;
        for (int c = tid; c < nl; c += SMP_T) {
            const int rel = s.list_i[c];
            if (rel >= r0 && rel < r1) f(s.list_l[c], rel);
        }
        return;
    }
    r1 = r1 < src.n ? r1 : src.n;
    for (int c = r0 + tid; c < r1; c += SMP_T)
        if (allow1(src, c)) f(src.p[c], c);
}

__device__ __forceinline__ void hist_zero(SampleShared& s) {
    __syncthreads();
    for (int b = threadIdx.x; b < SMP_BINS; b += SMP_T) {
        s.cnt[b] = 0u;
        s.mass[b] = 0ull;
    }
    __syncthreads();
}
__device__ __forceinline__ void hist_add(SampleShared& s, int bin, u64 q) {
    atomicAdd(&s.cnt[bin], 1u);
    if (q) atomicAdd(&s.mass[bin], q);
}

// Walk the histogram in key order (DESC: from the top bin down) and find the first bin at which the running count (or mass)
// reaches `need`. mode 0: need as given; 1: need = ceil(frac * total mass); 2: need = floor(frac * total mass) + 1. need is
// clamped to [1, total]. Results in s.r_* (the running sums BEFORE the bin, the bin's own, the totals, the need used).
// Wave 0 works, everyone waits. nbins is a multiple of 64.
template <bool DESC, bool BY_MASS>
__device__ __forceinline__ void scan_bins(SampleShared& s, int nbins, u64 need, int mode = 0, double frac = 0.0) {
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x, per = nbins >> 6;
        auto bin_at = [&](int pos) { return DESC ? nbins - 1 - pos : pos; };
        unsigned c = 0;
        u64 m = 0;
        for (int j = 0; j < per; ++j) {
            const int b = bin_at(lane * per + j);
            c += s.cnt[b];
            m += s.mass[b];
        }
        unsigned ci = c;
        u64 mi = m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned oc = __shfl_up(ci, o);
            const u64 om = shfl_up64(mi, o);
            if (lane >= o) {
                ci += oc;
                mi += om;
            }
        }
        const unsigned ctot = __shfl(ci, 63);
        const u64 mtot = shfl64(mi, 63);
        if (mode == 1) need = (u64)ceil(frac * (double)mtot);
        if (mode == 2) need = (u64)floor(frac * (double)mtot) + 1ull;
        const u64 tot = BY_MASS ? mtot : (u64)ctot;
        if (need > tot) need = tot;
        if (need < 1ull) need = 1ull;
        if (lane == 0) {   // what a caller reads if nothing crosses (empty histogram): the first bin of the walk, nothing before it
            s.r_bin = bin_at(0);
            s.r_cnt_before = 0u; s.r_cnt_bin = 0u; s.r_cnt_total = ctot;
            s.r_mass_before = 0ull; s.r_mass_bin = 0ull; s.r_mass_total = mtot;
            s.r_need = need;
        }
        const u64 inc = BY_MASS ? mi : (u64)ci;
        const u64 exc = inc - (BY_MASS ? m : (u64)c);
        if (exc < need && need <= inc) {   // exactly one lane
            unsigned cc = ci - c;
            u64 mm = mi - m;
            for (int j = 0; j < per; ++j) {
                const int b = bin_at(lane * per + j);
                const unsigned nc = s.cnt[b];
                const u64 nm = s.mass[b];
                const u64 run = BY_MASS ? mm : (u64)cc, v = BY_MASS ? nm : (u64)nc;
                if (run + v >= need) {
                    s.r_bin = b;
                    s.r_cnt_before = cc; s.r_cnt_bin = nc;
                    s.r_mass_before = mm; s.r_mass_bin = nm;
                    break;
                }
                cc += nc;
                mm += nm;
            }
        }
    }
    __syncthreads();
}

// digits of a 32-bit key, most significant first: 11 + 11 + 10 bits
__device__ __forceinline__ int key_shift(int lev) { return lev == 0 ? 21 : (lev == 1 ? 10 : 0); }
__device__ __forceinline__ int key_bins(int lev) { return lev == 2 ? 1024 : 2048; }
__device__ __forceinline__ bool key_in_prefix(unsigned key, unsigned prefix, int lev) {
    return lev == 0 || (key >> key_shift(lev - 1)) == (prefix >> key_shift(lev - 1));
}
__device__ __forceinline__ int key_digit(unsigned key, int lev) { return (int)((key >> key_shift(lev)) & (unsigned)(key_bins(lev) - 1)); }

// Compacts the elements with pred(l, rel) into LDS, in whatever order the atomics grant, and switches src to that list. The caller has
// counted them (a first-digit histogram): at most SMP_CAP, the slot guard only keeps a miscount inside the arrays. s.n_list is 0 on
// entry (kept_set zeroes it, and a row is compacted at most once). Every thread of the block calls this; block-uniform.
template <class Src, class P>
__device__ __forceinline__ void compact_to_list(SampleShared& s, Src& src, P pred) {
    for_each(s, src, [&](float l, int rel) {
        if (pred(l, rel)) {
            const unsigned slot = atomicAdd(&s.n_list, 1u);
            if (slot < SMP_CAP) {
                s.list_l[slot] = l;
                s.list_i[slot] = rel;
            }
        }
    });
    __syncthreads();
    src.list = true;
}

// The r-th smallest rel (r >= 1) among the elements with pred(l, rel): a count selection over two 10-bit digits of rel. Every thread
// of the block calls this; block-uniform.
template <class Src, class P>
__device__ __forceinline__ int nth_index(SampleShared& s, const Src& src, u64 r, P pred) {
    int ip = 0;
    for (int lev = 0; lev < 2; ++lev) {
        const int sh = lev == 0 ? 10 : 0;
        hist_zero(s);
        for_each(s, src, [&](float l, int rel) {
            if (!pred(l, rel)) return;
            if (lev == 1 && (rel >> 10) != (ip >> 10)) return;
            hist_add(s, (rel >> sh) & 1023, 0ull);
        });
        scan_bins<false, false>(s, 1024, r);
        ip |= s.r_bin << sh;
        r -= (u64)s.r_cnt_before;
    }
    return ip;
}

// The kept set of one row (steps 1-3 of cover_token_sample), as every entry point of this file sees it: column rel of [lo, hi) with logit l
// is kept  <=>  lkey(l) >= tk  and  ( wkey(w) > wstar  or  (wkey(w) == wstar and rel <= idx_cut) ),  w = weight_of(l, m, T).
// A pure function of (l, rel) and five block-uniform values, so the sampler (which walks the row or the compacted list) and the
// scorer (which looks at one given column) cannot disagree about membership.
struct KeptSet {
    float m, T;          // row maximum, temperature
    unsigned tk;         // key of the k-th largest logit (0: top-k off)
    unsigned wstar;      // key of the weight at the top-p cut (0: top-p off)
    int idx_cut;         // last kept index among the tokens that weigh exactly w* (0x7fffffff: all of them)
    __device__ __forceinline__ bool kept(float l, int rel, u64& q) const {
        if (lkey(l) < tk) return false;
        const float w = weight_of(l, m, T);
        const unsigned wb = wkey(w);
        if (wb < wstar || (wb == wstar && rel > idx_cut)) return false;
        q = q43(w);
        return true;
    }
};

// Steps 1-3: row maximum, k-th value, top-p cut. May compact the candidates into LDS and switch src to that list (src.list);
// every thread of the block calls this, the result is block-uniform.
template <class Src>
__device__ __forceinline__ KeptSet kept_set(SampleShared& s, Src& src, int top_k, float top_p, float T) {
    const int tid = threadIdx.x;
    const int n = src_count(src);
    const bool use_k = top_k > 0 && top_k < n;
    const bool use_p = top_p < 1.0f;
    if (tid == 0) s.n_list = 0u;

    // ---- pass 1: the row maximum; with top-k also the first digit of the logit keys (the probe that sizes the candidate list)
    float m = -INFINITY;
    if (use_k) {
        hist_zero(s);
        for_each(s, src, [&](float l, int rel) {
            m = fmaxf(m, l);
            hist_add(s, key_digit(lkey(l), 0), 0ull);
        });
    } else {
        for_each(s, src, [&](float l, int rel) { m = fmaxf(m, l); });
    }
    m = block_max(m, s.red);

    // ---- top-k: tk = key of the k-th largest logit; everything with lkey >= tk stays (ties with the k-th value included)
    unsigned tk = 0u;
    if (use_k) {
        scan_bins<true, false>(s, key_bins(0), (u64)top_k);
        const int b0 = s.r_bin;
        if (s.r_cnt_before + s.r_cnt_bin <= SMP_CAP)   // block-uniform
            compact_to_list(s, src, [&](float l, int rel) { return key_digit(lkey(l), 0) >= b0; });
        unsigned prefix = 0u;
        u64 need = (u64)top_k;
        for (int lev = 0; lev < 3; ++lev) {
            hist_zero(s);
            for_each(s, src, [&](float l, int rel) {
                const unsigned key = lkey(l);
                if (key_in_prefix(key, prefix, lev)) hist_add(s, key_digit(key, lev), 0ull);
            });
            scan_bins<true, false>(s, key_bins(lev), need);
            prefix |= (unsigned)s.r_bin << key_shift(lev);
            need -= (u64)s.r_cnt_before;
        }
        tk = prefix;
    }

    // ---- top-p: cut = (w*, idx*): kept <=> w > w*  or  (w == w* and rel <= idx*), among the tokens top-k kept
    unsigned wstar = 0u;
    int idx_cut = 0x7fffffff;
    if (use_p) {
        u64 target = 0ull;   // ceil(top_p * mass kept by top-k); 0 = not known yet
        if (!src.list) {
            // probe on the row: first digit of the weights, the mass of everything, and whether the cut's bin and the bins above fit the list
            hist_zero(s);
            for_each(s, src, [&](float l, int rel) {
                if (lkey(l) < tk) return;
                const float w = weight_of(l, m, T);
                hist_add(s, key_digit(wkey(w), 0), q43(w));
            });
            scan_bins<true, true>(s, key_bins(0), 0ull, 1, (double)top_p);
            target = s.r_need;
            const int b0 = s.r_bin;
            if (s.r_cnt_before + s.r_cnt_bin <= SMP_CAP)
                compact_to_list(s, src, [&](float l, int rel) { return lkey(l) >= tk && key_digit(wkey(weight_of(l, m, T)), 0) >= b0; });
        }
        unsigned prefix = 0u;
        u64 need = target, q_tie = 0ull;
        unsigned n_tie = 0u;
        for (int lev = 0; lev < 3; ++lev) {
            hist_zero(s);
            for_each(s, src, [&](float l, int rel) {
                if (lkey(l) < tk) return;
                const float w = weight_of(l, m, T);
                const unsigned key = wkey(w);
                if (key_in_prefix(key, prefix, lev)) hist_add(s, key_digit(key, lev), q43(w));
            });
            if (lev == 0 && target == 0ull) scan_bins<true, true>(s, key_bins(lev), 0ull, 1, (double)top_p);
            else scan_bins<true, true>(s, key_bins(lev), need);
            if (lev == 0 && target == 0ull) need = s.r_need;
            prefix |= (unsigned)s.r_bin << key_shift(lev);
            need -= s.r_mass_before;
            n_tie = s.r_cnt_bin;
            q_tie = n_tie ? s.r_mass_bin / (u64)n_tie : 0ull;
        }
        wstar = prefix;
        // n_tie tokens share the weight at the cut; the first r of them in index order complete the prefix
        u64 r = q_tie ? (need + q_tie - 1ull) / q_tie : 1ull;
        r = r < 1ull ? 1ull : (r > (u64)n_tie ? (u64)n_tie : r);
        if (r < (u64)n_tie)   // block-uniform; idx* = the r-th smallest index among the tied tokens
            idx_cut = nth_index(s, src, r, [&](float l, int rel) { return lkey(l) >= tk && wkey(weight_of(l, m, T)) == wstar; });
    }
    return KeptSet{m, T, tk, wstar, idx_cut};
}

// Count and Q43 mass of the kept tokens per tile of 1024 columns, into the histogram (the caller scans it: the totals are the size and
// the mass of the kept set, the crossing tile is the first digit of the pick). Returns the tile shift: tile of rel = (rel + shift) >> 10.
// Tiles are cut where the row's float4 body starts (tile 0 = the scalar head, if any), so the 256 columns one wave loads together
// lie in one tile: on the row, a wave adds its kept masses and count with shuffles (exact: integers) and one lane adds them to
// the tile -- per-element atomics on one address would serialise 64 lanes.
template <class Src>
__device__ __forceinline__ int kept_tiles(SampleShared& s, const Src& src, const KeptSet& ks) {
    const int tid = threadIdx.x;
    const int n = src.n;
    int head = 0;
    if (!src.list) {
        head = (int)(((16u - (unsigned)((uintptr_t)src.p & 15u)) & 15u) >> 2);
        head = head < n ? head : n;
    }
    const int shift = (1024 - head) & 1023;                 // at most 1025 tiles
    hist_zero(s);
    if (src.list) {
        for_each(s, src, [&](float l, int rel) {
            u64 q;
            if (ks.kept(l, rel, q)) hist_add(s, (rel + shift) >> 10, q);
        });
    } else {
        const float* p = src.p;
        const int lane = tid & 63;
        auto one = [&](float l, int rel) {
            u64 q;
            if (ks.kept(l, rel, q)) hist_add(s, (rel + shift) >> 10, q);
        };
        for (int c = tid; c < head; c += SMP_T)
            if (allow1(src, c)) one(p[c], c);
        const int n4 = (n - head) >> 2;
        const float4* v = (const float4*)(p + head);
        // packed per-lane sum: mass of <= 4 weights (< 2^46) in the low 52 bits, their count above; 64 lanes: mass < 2^52, count <= 256
        auto packed = [&](const float4& x, int c) -> u64 {
            const int i0 = head + 4 * c;
            u64 acc = 0ull, q;
            const unsigned m = allow4(src, i0);
            if ((m & 1u) && ks.kept(x.x, i0, q)) acc += q + (1ull << 52);
            if ((m & 2u) && ks.kept(x.y, i0 + 1, q)) acc += q + (1ull << 52);
            if ((m & 4u) && ks.kept(x.z, i0 + 2, q)) acc += q + (1ull << 52);
            if ((m & 8u) && ks.kept(x.w, i0 + 3, q)) acc += q + (1ull << 52);
            return acc;
        };
        auto flush = [&](u64 acc, int cb) {   // cb: the wave's first float4 of this load
            acc = wave_sum64(acc);
            if (lane == 0 && acc) {
                const int bin = (head + 4 * cb + shift) >> 10;
                atomicAdd(&s.cnt[bin], (unsigned)(acc >> 52));
                const u64 q = acc & ((1ull << 52) - 1ull);
                if (q) atomicAdd(&s.mass[bin], q);
            }
        };
        const float4 none = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int cb = tid - lane; cb < n4; cb += 4 * SMP_T) {   // cb is wave-uniform: every lane takes part in the shuffles
            const int c = cb + lane;
            const bool h0 = c < n4, h1 = c + SMP_T < n4, h2 = c + 2 * SMP_T < n4, h3 = c + 3 * SMP_T < n4;
            const float4 x0 = h0 ? v[c] : none, x1 = h1 ? v[c + SMP_T] : none, x2 = h2 ? v[c + 2 * SMP_T] : none,
                         x3 = h3 ? v[c + 3 * SMP_T] : none;
            flush(h0 ? packed(x0, c) : 0ull, cb);
            flush(h1 ? packed(x1, c + SMP_T) : 0ull, cb + SMP_T);
            flush(h2 ? packed(x2, c + 2 * SMP_T) : 0ull, cb + 2 * SMP_T);
            flush(h3 ? packed(x3, c + 3 * SMP_T) : 0ull, cb + 3 * SMP_T);
        }
        for (int c = head + 4 * n4 + tid; c < n; c += SMP_T)
            if (allow1(src, c)) one(p[c], c);
    }
    return shift;
}

// lp = x_t - log(sum over KEPT of exp(x_i)) for a column of the row with logit l at rel, -inf if it is not kept. x_t is the fp32 exponent the
// weights are made of, the sum is the exact Q43 mass of the kept set (>= 2^43: the row maximum weighs 1 and is always kept); the
// logarithm and the difference are taken in double, once per row, and rounded to fp32 once.
__device__ __forceinline__ float kept_logprob(const KeptSet& ks, float l, int rel, u64 mass) {
    u64 q;
    if (!ks.kept(l, rel, q)) return -INFINITY;
    const float x = (l - ks.m) / ks.T;
    return (float)((double)x - (log((double)mass) - 43.0 * 0.693147180559945309417232121458));
}

// The reference score of a pick (cover_token_sample_rows_ref): lp of column `pick` (logit l, both held by thread 0) under temperature
// t_ref with both filters off, over the columns of row_src. The calls are logprob_row's at (t_ref, 0, 1) -- kept_tiles and scan_bins with
// the KeptSet that kept_set returns for those parameters (the row maximum does not depend on them) -- so the value is that kernel's, bit
// for bit. A row whose own kept set already is the reference's (unfiltered at t_ref) reuses its mass: no pass. Every thread of the
// block calls this after the row's own outputs are stored; block-uniform.
template <class Src>
__device__ __forceinline__ void ref_logprob(SampleShared& s, const Src& row_src, const KeptSet& ks, u64 mass, float t_ref, float l, int pick,
                                            int row, float* ref_out) {
    const KeptSet kr{ks.m, t_ref, 0u, 0u, 0x7fffffff};
    if (!(ks.T == t_ref && ks.tk == 0u && ks.wstar == 0u && ks.idx_cut == 0x7fffffff)) {
        kept_tiles(s, row_src, kr);
        scan_bins<false, true>(s, SMP_BINS, 1ull);
        mass = s.r_mass_total;
    }
    if (threadIdx.x == 0) ref_out[row] = kept_logprob(kr, l, pick, mass);
}

// One row of the sampler: steps 1-4 of cover_token_sample over columns [lo, hi) of lg with the uniform u. Every thread of the block calls
// this; thread 0 stores. logprob_out == nullptr: no score. token_sample_k and token_sample_rows_k are this function with the launch's and
// the row's parameters respectively, so a row means the same in both.
// REF (cover_token_sample_rows_ref): ref_out[row] = the log-probability of the same pick under the reference distribution -- temperature
// t_ref, both filters off, over the same columns -- i.e. logprob_row at (t_ref, 0, 1) on the pick, bit for bit (ref_logprob below).
template <bool ALLOW = false, bool REF = false>
__device__ __forceinline__ void sample_row(SampleShared& s, const float* lg, int lo, int hi, float temperature, int top_k, float top_p, float u,
                                           int row, int64_t* token_out, float* logit_out, int* kept_out, float* logprob_out,
                                           const AllowRow<ALLOW>& ar = AllowRow<ALLOW>{}, float t_ref = 1.0f, float* ref_out = nullptr) {
    const int tid = threadIdx.x;
    const int n = hi - lo;
    SampleSrcT<ALLOW> src = make_src<ALLOW>(lg + lo, n, lo, ar);
    const SampleSrcT<ALLOW> row_src = src;   // kept_set may switch src to the compacted list; the reference mass needs the whole row
    const KeptSet ks = kept_set(s, src, top_k, top_p, temperature);

    // ---- pick: running mass of the kept tokens in index order; tiles of 1024 columns first, then the columns of the crossing tile
    const int shift = kept_tiles(s, src, ks);
    scan_bins<false, true>(s, SMP_BINS, 0ull, 2, (double)u);
    const int tile = s.r_bin;
    const unsigned kept = s.r_cnt_total;
    const u64 mass = s.r_mass_total;
    const u64 need2 = s.r_need - s.r_mass_before;
    const int t0 = (tile << 10) - shift;
    hist_zero(s);
    for_each_in(s, src, t0 < 0 ? 0 : t0, t0 + 1024, [&](float l, int rel) {
        u64 q;
        if (ks.kept(l, rel, q)) hist_add(s, (rel + shift) & 1023, q);
    });
    scan_bins<false, true>(s, 1024, need2);
    int pick = 0;
    float l = 0.f;
    if (tid == 0) {
        pick = t0 + s.r_bin;
        pick = pick < 0 ? 0 : (pick < n ? pick : n - 1);
        if constexpr (ALLOW)   // a row without mass (its allowed columns all NaN or -inf) crosses nowhere: the first allowed column
            if (!allow1(src, pick)) pick = src.first;
        token_out[row] = lo + pick;
        l = lg[lo + pick];
        if (logit_out) logit_out[row] = l;
        if (kept_out) kept_out[row] = (int)kept;
        if (logprob_out) logprob_out[row] = kept_logprob(ks, l, pick, mass);
    }
    if constexpr (REF) ref_logprob(s, row_src, ks, mass, t_ref, l, pick, row, ref_out);
}

template <bool SCORED>
__global__ __launch_bounds__(SMP_T) void token_sample_k(cover_token_sample_args a, float* logprob_out) {
    __shared__ SampleShared s;
    const int row = blockIdx.x;
    sample_row(s, a.logits + (size_t)row * a.ld, a.lo, a.hi, a.temperature, a.top_k, a.top_p, a.uniform[row], row, a.token_out, a.logit_out,
               a.kept_out, SCORED ? logprob_out : nullptr);
}

// Scores given tokens: the kept set and its mass as the sampler computes them (the same two device functions), no pick.
template <bool ALLOW = false>
__device__ __forceinline__ void logprob_row(SampleShared& s, const float* lg, int lo, int hi, float temperature, int top_k, float top_p,
                                            int row, const int64_t* token, float* logprob_out, int* kept_out,
                                            const AllowRow<ALLOW>& ar = AllowRow<ALLOW>{}) {
    const int n = hi - lo;
    SampleSrcT<ALLOW> src = make_src<ALLOW>(lg + lo, n, lo, ar);
    const KeptSet ks = kept_set(s, src, top_k, top_p, temperature);
    kept_tiles(s, src, ks);
    scan_bins<false, true>(s, SMP_BINS, 1ull);
    if (threadIdx.x == 0) {
        const long long t = (long long)token[row];
        float lp = -INFINITY;
        if (t >= (long long)lo && t < (long long)hi && allow1(src, (int)(t - lo)))   // a token that is not allowed: nothing is read for it
            lp = kept_logprob(ks, lg[t], (int)(t - lo), s.r_mass_total);
        logprob_out[row] = lp;
        if (kept_out) kept_out[row] = (int)s.r_cnt_total;
    }
}
__global__ __launch_bounds__(SMP_T) void token_logprob_k(cover_token_logprob_args a) {
    __shared__ SampleShared s;
    const int row = blockIdx.x;
    logprob_row(s, a.logits + (size_t)row * a.ld, a.lo, a.hi, a.temperature, a.top_k, a.top_p, row, a.token, a.logprob_out, a.kept_out);
}

// The n most probable kept tokens of a row with their log-probabilities, and the entropy of the kept distribution. The kept set and
// its mass are token_logprob_k's (the same device functions in the same order), so a reported log-probability is that kernel's value.
struct TopnShared {
    u64 ent;             // S: Q43 sum of w * (-x) over the kept set
    unsigned cnt;
    float l[64];
    int rel[64];
};

// One row of cover_token_topn; a carries the row's (temperature, top_k, top_p): the launch's in token_topn_k, the row's own in token_topn_rows_k.
template <bool ALLOW = false>
__device__ __forceinline__ void topn_row(SampleShared& s, TopnShared& t, const cover_token_topn_args& a, int row,
                                         const AllowRow<ALLOW>& ar = AllowRow<ALLOW>{}) {
    const int tid = threadIdx.x, lane = tid & 63;
    const float* lg = a.logits + (size_t)row * a.ld;
    const int n = a.hi - a.lo;
    SampleSrcT<ALLOW> src = make_src<ALLOW>(lg + a.lo, n, a.lo, ar);
    const KeptSet ks = kept_set(s, src, a.top_k, a.top_p, a.temperature);
    kept_tiles(s, src, ks);
    scan_bins<false, true>(s, SMP_BINS, 1ull);
    const unsigned kept = s.r_cnt_total;
    const u64 mass = s.r_mass_total;
    if (tid == 0) {
        t.ent = 0ull;
        t.cnt = 0u;
    }

    // ---- rank selection: thr = key of the want-th largest logit of the kept set (three digits of lkey); the first pass also sums S
    const unsigned want = kept < (unsigned)a.n ? kept : (unsigned)a.n;
    unsigned prefix = 0u, n_tie = 0u;
    u64 need = (u64)want;
    for (int lev = 0; lev < 3; ++lev) {
        u64 ent = 0ull;
        hist_zero(s);
        for_each(s, src, [&](float l, int rel) {
            u64 q;
            if (!ks.kept(l, rel, q)) return;
            const unsigned key = lkey(l);
            if (key_in_prefix(key, prefix, lev)) hist_add(s, key_digit(key, lev), 0ull);
            if (lev == 0) {
                const float x = (l - ks.m) / ks.T, w = weight_of(l, ks.m, ks.T);
                if (w > 0.f) ent += q43(w * -x);   // w == 0: an -inf logit (or x < -104), the term is 0 and 0 * inf is not formed
            }
        });
        if (lev == 0) {   // per wave: integer shuffles, then one LDS atomic
            ent = wave_sum64(ent);
            if (lane == 0 && ent) atomicAdd(&t.ent, ent);
        }
        scan_bins<true, false>(s, key_bins(lev), need);
        prefix |= (unsigned)s.r_bin << key_shift(lev);
        need -= (u64)s.r_cnt_before;
        n_tie = s.r_cnt_bin;
        if (lev == 0 && !src.list && s.r_cnt_before + s.r_cnt_bin <= SMP_CAP) {   // block-uniform; the list is free: kept_set left the row in place
            const int b0 = s.r_bin;
            compact_to_list(s, src, [&](float l, int rel) {
                u64 q;
                return ks.kept(l, rel, q) && key_digit(lkey(l), 0) >= b0;
            });
        }
    }
    const unsigned thr = prefix;
    // n_tie kept tokens share the logit at the threshold; the first `need` of them in index order complete the ranks
    int idx_cut = 0x7fffffff;
    if (need < (u64)n_tie)   // block-uniform; the need-th smallest index among them (as kept_set's idx_cut)
        idx_cut = nth_index(s, src, need < 1ull ? 1ull : need, [&](float l, int rel) {
            u64 q;
            return lkey(l) == thr && ks.kept(l, rel, q);
        });

    // ---- exactly `want` entries reach LDS (in whatever order the atomics grant); one wave ranks them
    for_each(s, src, [&](float l, int rel) {
        u64 q;
        const unsigned key = lkey(l);
        if (key < thr || (key == thr && rel > idx_cut) || !ks.kept(l, rel, q)) return;
        const unsigned slot = atomicAdd(&t.cnt, 1u);
        if (slot < 64u) {
            t.l[slot] = l;
            t.rel[slot] = rel;
        }
    });
    __syncthreads();
    if (tid < 64) {
        const int cnt = (int)(t.cnt < 64u ? t.cnt : 64u);
        const bool have = tid < cnt;
        const float l = have ? t.l[tid] : 0.f;
        const int rel = have ? t.rel[tid] : 0x7fffffff;
        const unsigned key = have ? lkey(l) : 0u;
        int rank = 0;
        for (int e = 0; e < 64; ++e) {   // (key descending, index ascending): rank = the number of entries ahead of this one
            const unsigned ke = __shfl(key, e);
            const int re = __shfl(rel, e);
            if (e < cnt && (ke > key || (ke == key && re < rel))) ++rank;
        }
        int64_t* tok = a.token_out + (size_t)row * a.ld_tok;
        float* lp = a.logprob_out + (size_t)row * a.ld_lp;
        if (have && rank < a.n) {
            tok[rank] = (int64_t)(a.lo + rel);
            lp[rank] = kept_logprob(ks, l, rel, mass);
        }
        if (tid >= cnt && tid < a.n) {
            tok[tid] = -1;
            lp[tid] = -INFINITY;
        }
        if (tid == 0) {
            if (a.entropy_out) {
                // H = log(sum w) + (sum w * -x) / (sum w) over the kept set: both sums exact integers, the rest double, one fp32 rounding
                const double M = (double)mass;
                a.entropy_out[row] = mass ? (float)(log(M) - 43.0 * 0.693147180559945309417232121458 + (double)t.ent / M) : 0.f;
            }
            if (a.kept_out) a.kept_out[row] = (int)kept;
        }
    }
}
__global__ __launch_bounds__(SMP_T) void token_topn_k(cover_token_topn_args a) {
    __shared__ SampleShared s;
    __shared__ TopnShared t;
    topn_row(s, t, a, blockIdx.x);
}

// ---- parameters per row (cover_token_*_rows) --------------------------------------------------------------------------------
// A row's (temperature, top_k, top_p) come from device arrays; everything else is the scalar kernels' row functions above, so a row
// computes what the scalar kernel computes for it. Block-uniform: every thread reads the same three words.
struct RowParams {
    float T;
    int k;
    float p;
    int mode;   // 0: sampled, 1: greedy (temperature 0; T / k / p are then 1 / 0 / 1, what a greedy pick is scored under), 2: invalid
};
__device__ __forceinline__ RowParams row_params(const float* temperature, const int* top_k, const float* top_p, int row) {
    RowParams r{1.0f, 0, 1.0f, 0};
    const float T = temperature[row];
    if (T == 0.0f) {   // top_k[row] / top_p[row] are not read
        r.mode = 1;
        return r;
    }
    if (!(T > 0.0f)) {   // negative or NaN
        r.mode = 2;
        return r;
    }
    r.T = T;
    if (top_k) r.k = top_k[row];
    if (top_p) r.p = top_p[row];
    if (r.k < 0 || !(r.p > 0.0f)) r.mode = 2;
    return r;
}

// ---- allowed-token sets per row (cover_token_*_rows_allowed) ------------------------------------------------------------------
// The row's set: counts the allowed columns of [lo, hi) and finds the first of them (one pass over the words that cover the range, edge
// words trimmed to it; integer LDS atomics). false: the row is invalid (set index outside [0, n_sets), or no allowed column in range).
// Every thread of the block calls this; block-uniform.
__device__ __forceinline__ bool allow_row(SampleShared& s, const cover_token_allow& al, int lo, int hi, int row, AllowRow<true>& ar) {
    const int tid = threadIdx.x;
    const int set = al.set_of_row ? al.set_of_row[row] : 0;
    if (set < 0 || set >= al.n_sets) return false;
    const unsigned* bits = al.bits + (size_t)set * (size_t)al.ld_words;
    if (tid == 0) {
        s.r_cnt_total = 0u;
        s.r_bin = 0x7fffffff;
    }
    __syncthreads();
    const int w0 = lo >> 5, w1 = (hi - 1) >> 5;
    unsigned cnt = 0u;
    int first = 0x7fffffff;
    for (int w = w0 + tid; w <= w1; w += SMP_T) {   // ascending per thread: its first hit is its lowest
        unsigned v = bits[w];
        if (w == w0) v &= 0xffffffffu << (lo & 31);
        if (w == w1 && (hi & 31)) v &= (1u << (hi & 31)) - 1u;
        cnt += (unsigned)__popc(v);
        if (v && first == 0x7fffffff) first = (w << 5) + (__ffs((int)v) - 1) - lo;
    }
    if (cnt) {
        atomicAdd(&s.r_cnt_total, cnt);
        atomicMin(&s.r_bin, first);
    }
    __syncthreads();
    ar.bits = bits;
    ar.cnt = (int)s.r_cnt_total;
    ar.first = s.r_bin;
    __syncthreads();   // the row functions write s.r_* again
    return ar.cnt > 0;
}

// ---- one block of a *_rows launch ---------------------------------------------------------------------------------------------
// What an invalid row (row_params' mode 2; with sets also a set index outside [0, n_sets) or no allowed column in range) stores in place
// of a result. Thread 0 stores (top-n: the first n threads); block-uniform.
__device__ __forceinline__ void invalid_logprob_row(const cover_token_logprob_rows_args& a, int row) {
    if (threadIdx.x == 0) {
        a.logprob_out[row] = NAN;
        if (a.kept_out) a.kept_out[row] = 0;
    }
}
__device__ __forceinline__ void invalid_topn_row(const cover_token_topn_rows_args& a, int row) {
    const int tid = threadIdx.x;
    if (tid < a.n) {
        a.token_out[(size_t)row * a.ld_tok + tid] = -1;
        a.logprob_out[(size_t)row * a.ld_lp + tid] = -INFINITY;
    }
    if (tid == 0) {
        if (a.entropy_out) a.entropy_out[row] = NAN;
        if (a.kept_out) a.kept_out[row] = 0;
    }
}

// Row blockIdx.x of a launch with parameters per row: the row's parameters, with ALLOW its set, then the scalar kernels' row function on
// them, so a row computes what the scalar kernel computes for it in every entry point. al is read only with ALLOW.
template <bool ALLOW>
__device__ __forceinline__ void logprob_rows_block(SampleShared& s, const cover_token_logprob_rows_args& a, const cover_token_allow& al) {
    const int row = blockIdx.x;
    const RowParams rp = row_params(a.temperature, a.top_k, a.top_p, row);
    AllowRow<ALLOW> ar;
    bool valid = rp.mode != 2;
    if constexpr (ALLOW) valid = valid && allow_row(s, al, a.lo, a.hi, row, ar);
    if (!valid) {
        invalid_logprob_row(a, row);
        return;
    }
    logprob_row<ALLOW>(s, a.logits + (size_t)row * a.ld, a.lo, a.hi, rp.T, rp.k, rp.p, row, a.token, a.logprob_out, a.kept_out, ar);
}
template <bool ALLOW>
__device__ __forceinline__ void topn_rows_block(SampleShared& s, TopnShared& t, const cover_token_topn_rows_args& a,
                                                const cover_token_allow& al) {
    const int row = blockIdx.x;
    const RowParams rp = row_params(a.temperature, a.top_k, a.top_p, row);
    AllowRow<ALLOW> ar;
    bool valid = rp.mode != 2;
    if constexpr (ALLOW) valid = valid && allow_row(s, al, a.lo, a.hi, row, ar);
    if (!valid) {
        invalid_topn_row(a, row);
        return;
    }
    cover_token_topn_args b;
    b.logits = a.logits; b.ld = a.ld; b.rows = a.rows; b.lo = a.lo; b.hi = a.hi;
    b.temperature = rp.T; b.top_k = rp.k; b.top_p = rp.p; b.n = a.n;
    b.token_out = a.token_out; b.ld_tok = a.ld_tok; b.logprob_out = a.logprob_out; b.ld_lp = a.ld_lp;
    b.entropy_out = a.entropy_out; b.kept_out = a.kept_out;
    topn_row<ALLOW>(s, t, b, row, ar);
}

// The kernels: one per entry point, each the block function above at its <ALLOW, REF>. Kernels of their own (not one kernel with run-time
// flags), so adding an entry point leaves the instructions of the others as they were.
__global__ __launch_bounds__(SMP_T) void token_sample_rows_k(cover_token_sample_rows_args a) {
    __shared__ SampleShared s;
    __shared__ int first;
    const int row = blockIdx.x, tid = threadIdx.x;
    const RowParams rp = row_params(a.temperature, a.top_k, a.top_p, row);
    if (rp.mode == 2) {   // block-uniform
        if (tid == 0) {
            a.token_out[row] = -1;
            if (a.logit_out) a.logit_out[row] = NAN;
            if (a.kept_out) a.kept_out[row] = 0;
            if (a.logprob_out) a.logprob_out[row] = NAN;
        }
        return;
    }
    const float* lg = a.logits + (size_t)row * a.ld;
    if (rp.mode == 0) {
        sample_row(s, lg, a.lo, a.hi, rp.T, rp.k, rp.p, a.uniform[row], row, a.token_out, a.logit_out, a.kept_out, a.logprob_out);
        return;
    }
    // greedy: the first arg-max of the input floats; its log-probability is logprob_row's at temperature 1, unfiltered (the same calls)
    const int n = a.hi - a.lo;
    SampleSrc src{lg + a.lo, n, false};
    if (tid == 0) first = 0x7fffffff;
    const KeptSet ks = kept_set(s, src, 0, 1.0f, 1.0f);   // the row maximum (NaNs never win, as in token_select_k); syncs the block
    kept_tiles(s, src, ks);
    scan_bins<false, true>(s, SMP_BINS, 1ull);
    int mine = 0x7fffffff;
    for_each(s, src, [&](float l, int rel) {
        if (l == ks.m && rel < mine) mine = rel;
    });
    if (mine != 0x7fffffff) atomicMin(&first, mine);
    __syncthreads();
    if (tid == 0) {
        int pick = first;
        pick = pick < n ? pick : 0;   // a row of NaNs has no maximum
        a.token_out[row] = a.lo + pick;
        const float l = lg[a.lo + pick];
        if (a.logit_out) a.logit_out[row] = l;
        if (a.kept_out) a.kept_out[row] = n;
        if (a.logprob_out) a.logprob_out[row] = kept_logprob(ks, l, pick, s.r_mass_total);
    }
}
__global__ __launch_bounds__(SMP_T) void token_logprob_rows_k(cover_token_logprob_rows_args a) {
    __shared__ SampleShared s;
    logprob_rows_block<false>(s, a, cover_token_allow{});
}
__global__ __launch_bounds__(SMP_T) void token_topn_rows_k(cover_token_topn_rows_args a) {
    __shared__ SampleShared s;
    __shared__ TopnShared t;
    topn_rows_block<false>(s, t, a, cover_token_allow{});
}
__global__ __launch_bounds__(SMP_T) void token_sample_rows_allowed_k(cover_token_sample_rows_args a, cover_token_allow al) {
    __shared__ SampleShared s;
    __shared__ int first;
    const int row = blockIdx.x, tid = threadIdx.x;
    const RowParams rp = row_params(a.temperature, a.top_k, a.top_p, row);
    AllowRow<true> ar;
    if (rp.mode == 2 || !allow_row(s, al, a.lo, a.hi, row, ar)) {   // block-uniform
        if (tid == 0) {
            a.token_out[row] = -1;
            if (a.logit_out) a.logit_out[row] = NAN;
            if (a.kept_out) a.kept_out[row] = 0;
            if (a.logprob_out) a.logprob_out[row] = NAN;
        }
        return;
    }
    const float* lg = a.logits + (size_t)row * a.ld;
    if (rp.mode == 0) {
        sample_row<true>(s, lg, a.lo, a.hi, rp.T, rp.k, rp.p, a.uniform[row], row, a.token_out, a.logit_out, a.kept_out, a.logprob_out, ar);
        return;
    }
    // greedy: the first arg-max of the input floats; its log-probability is logprob_row's at temperature 1, unfiltered (the same calls)
    const int n = a.hi - a.lo;
    SampleSrcT<true> src = make_src<true>(lg + a.lo, n, a.lo, ar);
    if (tid == 0) first = 0x7fffffff;
    const KeptSet ks = kept_set(s, src, 0, 1.0f, 1.0f);   // the row maximum (NaNs never win, as in token_select_k); syncs the block
    kept_tiles(s, src, ks);
    scan_bins<false, true>(s, SMP_BINS, 1ull);
    int mine = 0x7fffffff;
    for_each(s, src, [&](float l, int rel) {
        if (l == ks.m && rel < mine) mine = rel;
    });
    if (mine != 0x7fffffff) atomicMin(&first, mine);
    __syncthreads();
    if (tid == 0) {
        int pick = first;
        pick = pick < n ? pick : src.first;   // allowed columns all NaN: no maximum
        a.token_out[row] = a.lo + pick;
        const float l = lg[a.lo + pick];
        if (a.logit_out) a.logit_out[row] = l;
        if (a.kept_out) a.kept_out[row] = src_count(src);
        if (a.logprob_out) a.logprob_out[row] = kept_logprob(ks, l, pick, s.r_mass_total);
    }
}

// cover_token_sample_rows_ref: token_sample_rows_k (ALLOW: token_sample_rows_allowed_k; al is then the launch's sets, otherwise unused) with
// one more store per row, ref.logprob_out[row] = lp(pick) at ref.temperature, unfiltered (ref_logprob). Kernels of their own, so the two
// above compile to what they compiled to before this one existed; every other output is theirs, from the same row functions.
template <bool ALLOW>
__global__ __launch_bounds__(SMP_T) void token_sample_rows_ref_k(cover_token_sample_rows_args a, cover_token_allow al, cover_token_ref ref) {
    __shared__ SampleShared s;
    __shared__ int first;
    const int row = blockIdx.x, tid = threadIdx.x;
    const RowParams rp = row_params(a.temperature, a.top_k, a.top_p, row);
    AllowRow<ALLOW> ar;
    bool valid = rp.mode != 2;
    if constexpr (ALLOW) valid = valid && allow_row(s, al, a.lo, a.hi, row, ar);
    if (!valid) {   // block-uniform
        if (tid == 0) {
            a.token_out[row] = -1;
            if (a.logit_out) a.logit_out[row] = NAN;
            if (a.kept_out) a.kept_out[row] = 0;
            if (a.logprob_out) a.logprob_out[row] = NAN;
            ref.logprob_out[row] = NAN;
        }
        return;
    }
    const float* lg = a.logits + (size_t)row * a.ld;
    if (rp.mode == 0) {
        sample_row<ALLOW, true>(s, lg, a.lo, a.hi, rp.T, rp.k, rp.p, a.uniform[row], row, a.token_out, a.logit_out, a.kept_out, a.logprob_out, ar,
                                ref.temperature, ref.logprob_out);
        return;
    }
    // greedy: as in the kernels above; the pick's own score is taken at temperature 1, unfiltered, which is the reference's when ref.temperature == 1
    const int n = a.hi - a.lo;
    SampleSrcT<ALLOW> src = make_src<ALLOW>(lg + a.lo, n, a.lo, ar);
    if (tid == 0) first = 0x7fffffff;
    const KeptSet ks = kept_set(s, src, 0, 1.0f, 1.0f);
    kept_tiles(s, src, ks);
    scan_bins<false, true>(s, SMP_BINS, 1ull);
    const u64 mass = s.r_mass_total;
    int mine = 0x7fffffff;
    for_each(s, src, [&](float l, int rel) {
        if (l == ks.m && rel < mine) mine = rel;
    });
    if (mine != 0x7fffffff) atomicMin(&first, mine);
    __syncthreads();
    int pick = 0;
    float l = 0.f;
    if (tid == 0) {
        pick = first;
        if constexpr (ALLOW) pick = pick < n ? pick : src.first;
        else pick = pick < n ? pick : 0;
        a.token_out[row] = a.lo + pick;
        l = lg[a.lo + pick];
        if (a.logit_out) a.logit_out[row] = l;
        if (a.kept_out) a.kept_out[row] = src_count(src);
        if (a.logprob_out) a.logprob_out[row] = kept_logprob(ks, l, pick, mass);
    }
    ref_logprob(s, src, ks, mass, ref.temperature, l, pick, row, ref.logprob_out);
}
__global__ __launch_bounds__(SMP_T) void token_logprob_rows_allowed_k(cover_token_logprob_rows_args a, cover_token_allow al) {
    __shared__ SampleShared s;
    logprob_rows_block<true>(s, a, al);
}
__global__ __launch_bounds__(SMP_T) void token_topn_rows_allowed_k(cover_token_topn_rows_args a, cover_token_allow al) {
    __shared__ SampleShared s;
    __shared__ TopnShared t;
    topn_rows_block<true>(s, t, a, al);
}

// ---- cover_gumbel_topn: one step of stochastic beam search for one beam (the formula: include/cover_hip.h) ------------------------------
// The log-probabilities are token_logprob_k's: kept_set / kept_tiles / scan_bins at (temperature, 0, 1) in that kernel's order, then
// kept_logprob per column. Behind them the histogram and the candidate list are free, and the same LDS holds the columns' keys and
// perturbed scores (at most SMP_CAP = 4 * SMP_T columns: four per thread, in registers between the two block reductions).
union GumbelShared {
    SampleShared s;
    struct {
        u64 key[SMP_CAP];     // (descending image of g~) << 32 | column; a dead child: all ones
        float g[SMP_CAP];     // g~ by column
    } t;
};
__global__ __launch_bounds__(SMP_T) void gumbel_topn_k(cover_gumbel_topn_args a, int n2) {
    __shared__ GumbelShared sh;
    __shared__ float red[16];
    const int row = blockIdx.x, tid = threadIdx.x, n = a.hi - a.lo;
    int64_t* tok_o = a.token_out + (size_t)row * a.ld_tok;
    float* lp_o = a.logprob_out + (size_t)row * a.ld_lp;
    float* g_o = a.perturbed_out + (size_t)row * a.ld_g;
    const float phi = a.phi[row], G = a.g_parent[row];
    if (!finite_f(phi) || !finite_f(G)) {   // a dead beam (block-uniform): nothing of the row is read
        if (tid < a.n) {
            tok_o[tid] = -1;
            lp_o[tid] = -INFINITY;
            g_o[tid] = -INFINITY;
        }
        return;
    }
    const float* lg = a.logits + (size_t)row * a.ld + a.lo;
    SampleSrc src{lg, n, false};
    const KeptSet ks = kept_set(sh.s, src, 0, 1.0f, a.temperature);
    kept_tiles(sh.s, src, ks);
    scan_bins<false, true>(sh.s, SMP_BINS, 1ull);
    const u64 mass = sh.s.r_mass_total;
    __syncthreads();   // every thread holds the mass: sh.s is dead from here, sh.t takes its place

    const float* ur = a.uniform + (size_t)row * a.ld_u;
    float gv[SMP_CAP / SMP_T];
    float z = -INFINITY;
#pragma unroll
    for (int k = 0; k < SMP_CAP / SMP_T; ++k) {
        const int c = tid + k * SMP_T;
        float g = -INFINITY;
        if (c < n) {
            const float lp = kept_logprob(ks, lg[c], c, mass);
            if (finite_f(lp)) {
                const float u = fminf(fmaxf(ur[c], 0x1p-24f), 1.0f - 0x1p-24f);   // fmaxf drops a NaN
                g = (phi + lp) - logf(-logf(u));
                if (!finite_f(g)) g = -INFINITY;
            }
        }
        gv[k] = g;
        z = fmaxf(z, g);
    }
    z = block_max(z, red);
#pragma unroll
    for (int k = 0; k < SMP_CAP / SMP_T; ++k) {
        const int c = tid + k * SMP_T;
        if (c >= n2) continue;
        const float g = gv[k];
        float gt = -INFINITY;
        if (g > -INFINITY) {
            gt = G;   // g == z: the maximum inherits its parent's score, whatever expf and log1pf make of the formula there
            if (g != z) {
                const float v = G - g + log1pf(-expf(g - z));
                gt = G - fmaxf(0.0f, v) - log1pf(expf(-fabsf(v)));
            }
            if (!finite_f(gt)) gt = -INFINITY;
        }
        sh.t.key[c] = gt > -INFINITY ? ((u64)desc_key(gt) << 32) | (unsigned)c : ~0ull;
        if (c < n) sh.t.g[c] = gt;
    }
    __syncthreads();
    bitonic_sort_lds(sh.t.key, n2);
    if (tid < a.n) {
        const u64 k = tid < n2 ? sh.t.key[tid] : ~0ull;
        long long tok = -1;
        float lp = -INFINITY, gt = -INFINITY;
        if (k != ~0ull) {
            const int c = (int)(unsigned)k;   // < n: written above from a live column
            tok = a.lo + c;
            lp = kept_logprob(ks, lg[c], c, mass);
            gt = sh.t.g[c];
        }
        tok_o[tid] = tok;
        lp_o[tid] = lp;
        g_o[tid] = gt;
    }
}

__global__ void fill_i32_k(int* p, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ---- launches: every check fails with hipErrorInvalidValue ------------------------------------------------------------------------
static bool range_ok(int lo, int hi, int rows) { return hi > lo && lo >= 0 && hi - lo <= (1 << 20) && rows >= 0; }
static bool sample_params_ok(int lo, int hi, int rows, float temperature, int top_k, float top_p) {
    return range_ok(lo, hi, rows) && temperature > 0.f && top_p > 0.f && top_k >= 0;
}
static bool topn_shape_ok(int n, int ld_tok, int ld_lp) { return n >= 1 && n <= 64 && ld_tok >= n && ld_lp >= n; }
// The *_rows families. The per-row parameters live on the device: only the pointers and the launch's own shape are checked here, a bad
// row reports itself (see row_params).
static bool sample_rows_ok(const cover_token_sample_rows_args* a) {
    return a->logits && a->uniform && a->temperature && a->token_out && range_ok(a->lo, a->hi, a->rows);
}
static bool logprob_rows_ok(const cover_token_logprob_rows_args* a) {
    return a->logits && a->temperature && a->token && a->logprob_out && range_ok(a->lo, a->hi, a->rows);
}
static bool topn_rows_ok(const cover_token_topn_rows_args* a) {
    return a->logits && a->temperature && a->token_out && a->logprob_out && range_ok(a->lo, a->hi, a->rows) &&
           topn_shape_ok(a->n, a->ld_tok, a->ld_lp);
}
// the set itself lives on the device as well: the launch checks its shape, a row whose set index or set is unusable reports itself
static bool allow_ok(const cover_token_allow* al, int hi) {
    if (!al || !al->bits || ((uintptr_t)al->bits & 3u)) return false;
    return al->n_sets >= 1 && al->ld_words >= (long long)((hi + 31) / 32);
}
// one 1024-thread block per row; no rows: nothing is launched
template <class K, class... A>
static hipError_t launch_rows(K kernel, int rows, hipStream_t st, const A&... args) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3(rows), dim3(SMP_T), 0, st, args...);
    return hipGetLastError();
}

hipError_t launch_token_logprob(const cover_token_logprob_args* a, hipStream_t st) {
    if (!a->logits || !a->token || !a->logprob_out) return hipErrorInvalidValue;
    if (!sample_params_ok(a->lo, a->hi, a->rows, a->temperature, a->top_k, a->top_p)) return hipErrorInvalidValue;
    return launch_rows(token_logprob_k, a->rows, st, *a);
}

hipError_t launch_token_topn(const cover_token_topn_args* a, hipStream_t st) {
    if (!a->logits || !a->token_out || !a->logprob_out) return hipErrorInvalidValue;
    if (!sample_params_ok(a->lo, a->hi, a->rows, a->temperature, a->top_k, a->top_p)) return hipErrorInvalidValue;
    if (!topn_shape_ok(a->n, a->ld_tok, a->ld_lp)) return hipErrorInvalidValue;
    return launch_rows(token_topn_k, a->rows, st, *a);
}

// logprob_out == nullptr: cover_token_sample; otherwise cover_token_sample_scored (the same launch with one more store per row)
static hipError_t launch_token_sample_impl(const cover_token_sample_args* a, float* logprob_out, hipStream_t st) {
    if (!a->logits || !a->uniform || !a->token_out) return hipErrorInvalidValue;
    if (!sample_params_ok(a->lo, a->hi, a->rows, a->temperature, a->top_k, a->top_p)) return hipErrorInvalidValue;
    if (a->rows == 0) return hipSuccess;
    const int n = a->hi - a->lo;
    const bool filtered = (a->top_k > 0 && a->top_k < n) || a->top_p < 1.0f;
    if (!filtered && n <= 4096) {   // the unfiltered narrow range is cover_token_select's, bit for bit
        cover_token_select_args b;
        b.logits = a->logits; b.ld = a->ld; b.rows = a->rows; b.lo = a->lo; b.hi = a->hi;
        b.uniform = a->uniform; b.temperature = a->temperature; b.token_out = a->token_out; b.logit_out = a->logit_out;
        hipError_t e = launch_token_select(&b, st);
        if (e != hipSuccess) return e;
        if (logprob_out) {   // cover_token_select keeps no mass: score its picks in a second launch (which also writes the kept count)
            cover_token_logprob_args c;
            c.logits = a->logits; c.ld = a->ld; c.rows = a->rows; c.lo = a->lo; c.hi = a->hi;
            c.temperature = a->temperature; c.top_k = a->top_k; c.top_p = a->top_p;
            c.token = a->token_out; c.logprob_out = logprob_out; c.kept_out = a->kept_out;
            return launch_token_logprob(&c, st);
        }
        if (a->kept_out) hipLaunchKernelGGL(fill_i32_k, dim3((a->rows + 255) / 256), dim3(256), 0, st, a->kept_out, a->rows, n);
        return hipGetLastError();
    }
    if (logprob_out) return launch_rows(token_sample_k<true>, a->rows, st, *a, logprob_out);
    return launch_rows(token_sample_k<false>, a->rows, st, *a, logprob_out);
}

hipError_t launch_token_sample_rows(const cover_token_sample_rows_args* a, hipStream_t st) {
    if (!sample_rows_ok(a)) return hipErrorInvalidValue;
    return launch_rows(token_sample_rows_k, a->rows, st, *a);
}

hipError_t launch_token_logprob_rows(const cover_token_logprob_rows_args* a, hipStream_t st) {
    if (!logprob_rows_ok(a)) return hipErrorInvalidValue;
    return launch_rows(token_logprob_rows_k, a->rows, st, *a);
}

hipError_t launch_token_topn_rows(const cover_token_topn_rows_args* a, hipStream_t st) {
    if (!topn_rows_ok(a)) return hipErrorInvalidValue;
    return launch_rows(token_topn_rows_k, a->rows, st, *a);
}

hipError_t launch_token_sample_rows_allowed(const cover_token_sample_rows_args* a, const cover_token_allow* al, hipStream_t st) {
    if (!sample_rows_ok(a) || !allow_ok(al, a->hi)) return hipErrorInvalidValue;
    return launch_rows(token_sample_rows_allowed_k, a->rows, st, *a, *al);
}

// al == nullptr: the unmasked kernel. The reference temperature travels by value: a captured launch keeps the one it was recorded with.
hipError_t launch_token_sample_rows_ref(const cover_token_sample_rows_args* a, const cover_token_allow* al, const cover_token_ref* ref,
                                        hipStream_t st) {
    if (!sample_rows_ok(a) || (al && !allow_ok(al, a->hi))) return hipErrorInvalidValue;
    if (!ref || !ref->logprob_out || !(ref->temperature > 0.f) || !(ref->temperature < INFINITY)) return hipErrorInvalidValue;
    if (al) return launch_rows(token_sample_rows_ref_k<true>, a->rows, st, *a, *al, *ref);
    return launch_rows(token_sample_rows_ref_k<false>, a->rows, st, *a, cover_token_allow{}, *ref);
}

hipError_t launch_token_logprob_rows_allowed(const cover_token_logprob_rows_args* a, const cover_token_allow* al, hipStream_t st) {
    if (!logprob_rows_ok(a) || !allow_ok(al, a->hi)) return hipErrorInvalidValue;
    return launch_rows(token_logprob_rows_allowed_k, a->rows, st, *a, *al);
}

hipError_t launch_token_topn_rows_allowed(const cover_token_topn_rows_args* a, const cover_token_allow* al, hipStream_t st) {
    if (!topn_rows_ok(a) || !allow_ok(al, a->hi)) return hipErrorInvalidValue;
    return launch_rows(token_topn_rows_allowed_k, a->rows, st, *a, *al);
}

hipError_t launch_token_sample(const cover_token_sample_args* a, hipStream_t st) { return launch_token_sample_impl(a, nullptr, st); }

hipError_t launch_token_sample_scored(const cover_token_sample_scored_args* a, hipStream_t st) {
    if (!a->logprob_out) return hipErrorInvalidValue;
    cover_token_sample_args b;
    b.logits = a->logits; b.ld = a->ld; b.rows = a->rows; b.lo = a->lo; b.hi = a->hi;
    b.uniform = a->uniform; b.temperature = a->temperature; b.top_k = a->top_k; b.top_p = a->top_p;
    b.token_out = a->token_out; b.logit_out = a->logit_out; b.kept_out = a->kept_out;
    return launch_token_sample_impl(&b, a->logprob_out, st);
}

hipError_t launch_gumbel_topn(const cover_gumbel_topn_args* a, hipStream_t st) {
    if (!a->logits || !a->phi || !a->g_parent || !a->uniform || !a->token_out || !a->logprob_out || !a->perturbed_out) return hipErrorInvalidValue;
    if (!sample_params_ok(a->lo, a->hi, a->rows, a->temperature, 0, 1.0f) || a->hi - a->lo > SMP_CAP) return hipErrorInvalidValue;
    if (!topn_shape_ok(a->n, a->ld_tok, a->ld_lp) || a->ld_g < a->n || a->ld_u < a->hi - a->lo) return hipErrorInvalidValue;
    int n2 = 2;
    while (n2 < a->hi - a->lo) n2 <<= 1;
    return launch_rows(gumbel_topn_k, a->rows, st, *a, n2);
}
