// LDS-tiled bf16 GEMM kernels for gfx950 (GK_TILED / GK_TILED_PC plans): C[M,N] = epi(A[M,K] . W[N,K]^T), fp32 accumulate on
// v_mfma_f32_16x16x32_bf16. Weights in the packed fragment-major layout described at the top of gemm_pack.hip; operands SWAPPED, so the
// accumulator of lane (r = lane&15, g = lane>>4) holds C[m = r][n = 4g .. 4g+3].
//
//   gemm_tiled     (WGM*WM*16) x (WGN*WN*16) x 64 tile (64x64 up to 256x128 / 128x256), LDS ring of 2-4 stages. A tile staged with an XOR chunk swizzle
//                  (conflict-free ds_read_b128), W tile staged lane-linear straight from the packed layout. Staging either async
//                  global->LDS (global_load_lds, 16 B/lane) or through registers (variant 2).
//   gemm_tiled_pc  the same tile with NL loader waves that own every LDS-DMA of the block and 4 MFMA waves that only compute.
// Both take an optional split-K over gridDim.y (raw fp32 slabs [S][M][N], completed by gemm_reduce.hip) and leave through gemm_common.h's
// staged epilogue, which stamps slots 4-6 of the COVER_PC_DEBUG timeline through PCTL: PCTL is defined BEFORE that header is included.
// Compile-time switches, all here: COVER_PC_DEBUG (cover_pc_debug / cover_pc_timeline), COVER_PC_ABL, COVER_PC_PRIO.
#include <hip/hip_ext.h>
#include "common.h"
#include "kernels.h"

#ifdef COVER_PC_DEBUG
__device__ unsigned long long g_pc_tl[1024 * 8];   // per block (thread 0): start, loop start, loop end, end, epilogue stamps (100 MHz wall clock)
#define PCTL(slot) do { if (threadIdx.x == 0) g_pc_tl[((blockIdx.y * gridDim.x + blockIdx.x) & 1023) * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define PCTL(slot) do { } while (0)
#endif

#include "gemm_common.h"


// ---------------------------------------------------------------------------------------------------
// Tiled kernel: tile = (2*WM*16) x (2*WN*16) x 64, 4 waves in 2x2, each wave WM x WN MFMA fragments.
//   <4,4> 128x128 (large GEMMs), <2,4> 64x128, <2,2> 64x64 (ViT-sized GEMMs whose 128x128 grid cannot fill 256 CUs).
// Optional split-K over gridDim.y: slice s accumulates k-tiles [s*kt_per, ...) and stores raw fp32 partials
// [S][M][N] that splitk_reduce folds with the epilogue.
// ---------------------------------------------------------------------------------------------------

template <int WM, int WN, bool GLDS, int NST_ = 2, int WGM = 2, int WGN = 2>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_tiled(const bf16_t* __restrict__ A, int lda,
                                                  const bf16_t* __restrict__ Wp, void* C, int ldc, int M, int N,
                                                  int Kp, EpiDev epi, int tiles_m, int tiles_n, int kt_per,
                                                  float* __restrict__ partial) {
    constexpr int NW = WGM * WGN;                // waves: a WGM x WGN grid of (WM*16) x (WN*16) wave tiles
    constexpr int BM_ = WGM * WM * 16, BN_ = WGN * WN * 16;
    constexpr int A_BYTES = BM_ * BK * 2, B_BYTES = BN_ * BK * 2;
    constexpr int AI = BM_ / (8 * NW), BI = BN_ / (8 * NW);  // 1-KiB staging instructions per wave per tile
    constexpr int NST = GLDS ? NST_ : 2;         // LDS stages (NST - 1 k-tiles stay in flight across the barrier)
    PCTL(0);
    static_assert(BM_ % (8 * NW) == 0 && BN_ % (8 * NW) == 0, "tile rows must split evenly over the waves");
    static_assert((NST - 2) * (AI + BI) <= 63, "counted vmcnt must fit its 6-bit field");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                   // [NST][A_BYTES]
    char* Bs = smem + NST * A_BYTES;   // [NST][B_BYTES]

    // XCD-aware bijective remap of the linear block id: blocks dispatched round-robin over the 8 XCDs get a
    // contiguous range of tiles each, so the m-tiles that share one weight tile hit the same L2.
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    {
        const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        bid = base + (bid >> 3);
    }
    const int tn = bid / tiles_m, tm = bid % tiles_m;
    const int m0 = tm * BM_, n0 = tn * BN_;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w / WGN, wn = w % WGN;
    const int K32 = Kp >> 5;
    const int N16 = (N + 15) >> 4;
    const int nk_total = Kp / BK;
    const int kt0 = blockIdx.y * kt_per;
    const int nk = min(kt_per, nk_total - kt0);

    // ---- staging addresses ----
    // A: LDS chunk position p = j*64 + lane: row = p>>3, c = p&7 holds global chunk c ^ (row&7)
    const bf16_t* a_src[AI];
    const bf16_t* b_src[BI];
#pragma unroll
    for (int i = 0; i < AI; ++i) {
        const int j = w * AI + i;
        const int row = j * 8 + (lane >> 3), c = lane & 7;
        int gr = m0 + row;
        gr = gr < M ? gr : M - 1;
        a_src[i] = A + (size_t)gr * lda + (size_t)kt0 * BK + ((c ^ (row & 7)) << 3);
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
        const int j = w * BI + i;
        const int nbi = j >> 1, kbi = j & 1;
        int nb = (n0 >> 4) + nbi;
        nb = nb < N16 ? nb : N16 - 1;
        b_src[i] = Wp + ((size_t)nb * K32 + (size_t)kt0 * 2 + kbi) * 512 + lane * 8;
    }

    f32x4 acc[WN][WM];  // [n-block b][m-frag f]
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
        for (int f = 0; f < WM; ++f) acc[b][f] = (f32x4){0.f, 0.f, 0.f, 0.f};

    uint4 ra[AI], rb[BI];
    const uint32_t as_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(As) + w * AI * 1024);
    const uint32_t bs_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(Bs) + w * BI * 1024);
    auto stage_glds = [&](int buf, int kt) {
#pragma unroll
        for (int i = 0; i < AI; ++i) glds16_asm(a_src[i] + kt * BK, as_u32 + buf * A_BYTES + i * 1024);
#pragma unroll
        for (int i = 0; i < BI; ++i) glds16_asm(b_src[i] + (size_t)kt * 2 * 512, bs_u32 + buf * B_BYTES + i * 1024);
    };
    auto stage_load = [&](int kt) {
#pragma unroll
        for (int i = 0; i < AI; ++i) ra[i] = *(const uint4*)(a_src[i] + kt * BK);
#pragma unroll
        for (int i = 0; i < BI; ++i) rb[i] = *(const uint4*)(b_src[i] + (size_t)kt * 2 * 512);
    };
    auto stage_write = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AI; ++i) *(uint4*)(As + buf * A_BYTES + (w * AI + i) * 1024 + lane * 16) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *(uint4*)(Bs + buf * B_BYTES + (w * BI + i) * 1024 + lane * 16) = rb[i];
    };
    const int r = lane & 15, g = lane >> 4;
    auto compute = [&](int buf) {
        const char* Ab = As + buf * A_BYTES;
        const char* Bb = Bs + buf * B_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 xf[WM], wf[WN];
#pragma unroll
            for (int f = 0; f < WM; ++f) {
                const int row = wm * (WM * 16) + f * 16 + r;
                const int c = (ks * 4 + g) ^ (row & 7);
                xf[f] = as_bf16x8(*(const uint4*)(Ab + (row * 8 + c) * 16));
            }
#pragma unroll
            for (int b = 0; b < WN; ++b)
                wf[b] = as_bf16x8(*(const uint4*)(Bb + (((wn * WN + b) * 2 + ks) * 64 + lane) * 16));
#pragma unroll
            for (int b = 0; b < WN; ++b)
#pragma unroll
                for (int f = 0; f < WM; ++f)
                    acc[b][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[b], xf[f], acc[b][f], 0, 0, 0);
        }
    };

    PCTL(1);
    if (GLDS) {
        // 3-stage ring, two k-tiles in flight: tile kt is waited for with a COUNTED vmcnt (the AI+BI loads of tile kt+1
        // stay outstanding across the barrier), a raw s_barrier publishes it, then tile kt+2 is issued into the stage
        // that compute(kt-1) has just released. __syncthreads() would drain vmcnt to 0 here.
        if (NST >= 3) {
            // NST-stage ring, NST-1 k-tiles in flight: tile kt is waited for with a COUNTED vmcnt (the loads of the younger
            // tiles stay outstanding across the barrier), a raw s_barrier publishes it, then tile kt+NST-1 is issued
            // into the stage that compute(kt-1) has just released. __syncthreads() would drain vmcnt to 0 here.
#pragma unroll
            for (int s = 0; s < NST - 1; ++s)
                if (s < nk) stage_glds(s, s);
            int cur = 0;
            for (int kt = 0; kt < nk; ++kt) {
                const int younger = nk - 1 - kt;   // tiles issued after kt that may stay in flight
                if (NST >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (AI + BI)) : "memory");
                else if (younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + BI) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (kt + NST - 1 < nk) stage_glds(cur == 0 ? NST - 1 : cur - 1, kt + NST - 1);  // stage (kt-1) % NST
                compute(cur);
                cur = cur == NST - 1 ? 0 : cur + 1;
            }
        } else {  // 2 stages: smaller LDS footprint -> one more resident block per CU (better when L2->LDS bandwidth-bound)
            stage_glds(0, 0);
            for (int kt = 0; kt < nk; ++kt) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (kt + 1 < nk) stage_glds((kt + 1) & 1, kt + 1);
                compute(kt & 1);
            }
        }
    } else {
        stage_load(0);
        stage_write(0);
        for (int kt = 0; kt < nk; ++kt) {
            __syncthreads();
            if (kt + 1 < nk) stage_load(kt + 1);
            compute(kt & 1);
            if (kt + 1 < nk) stage_write((kt + 1) & 1);
        }
    }

    // ---- epilogue ----
    PCTL(2);
    tiled_epilogue_staged<WM, WN, BM_, BN_>(acc, epi, C, ldc, M, N, m0, n0, m0 + wm * (WM * 16), n0 + wn * (WN * 16), r, g, partial, smem,
                                            NST * (A_BYTES + B_BYTES), tid, 64 * NW);
    PCTL(3);
}

// ---------------------------------------------------------------------------------------------------
// Producer / consumer variant of the tiled kernel: 4 MFMA waves (2 x 2) + NL loader waves per block.
// Cycle counters in gemm_tiled's k-loop (64x128, M = 448) show an MFMA wave spending ~30 % of every k-tile ISSUING its
// LDS-DMA instructions (the CU's address path is shared, and all waves issue right after their barriers) and ~40 %
// waiting for the tile issued one iteration earlier. Here the loader waves own every LDS-DMA of the block (piece j of a
// tile belongs to loader j mod NL) and run NST-1 k-tiles ahead with a counted vmcnt; the MFMA waves only pass one barrier
// per k-tile and compute:
//   loader:   wait (own pieces of tile kt landed) -> barrier kt -> issue tile kt+NST-1 into the stage of tile kt-1
//   consumer: barrier kt sits in the MIDDLE of tile kt-1 (see the software pipeline below); a consumer reaching it holds
//             every fragment of tile kt-1 in registers, so that stage is free
// LDS-DMA data is ordered for the consumers by the loaders' vmcnt waits followed by the barrier they pass.
// ---------------------------------------------------------------------------------------------------
#ifdef COVER_PC_DEBUG
__device__ unsigned long long g_pc_dbg[8];   // loader: wait, barrier, issue; consumer: barrier, rest; counts
extern "C" int cover_pc_debug(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pc_dbg), sizeof(g_pc_dbg)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_pc_dbg), z, sizeof(z)); }
    return 0;
}
#define PCT() __builtin_readcyclecounter()
extern "C" int cover_pc_timeline(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pc_tl), sizeof(g_pc_tl)); }
#endif
#ifdef COVER_PC_ABL
// Ablation builds (tools/dbg/abl_prefill.sh, -DCOVER_PC_ABL=<bits>, compile-time): bit 0 = the MFMA waves skip their MFMAs, bit 1 = they
// skip the LDS fragment reads, bit 2 = the loaders skip the weight pieces, bit 3 = the loaders skip the activation pieces.
// Results are garbage by design. (A run-time flag trips a backend bug: "V_CMP_NE_U32 0, $src_shared_base: incorrect register class".)
#define PC_ABL(bit) ((COVER_PC_ABL) & (bit))
#else
#define PC_ABL(bit) 0
#endif
template <int WM, int WN, int NST, int NL = 1, int CGM = 2, int CGN = 2>
__global__ __launch_bounds__(64 * (CGM * CGN + NL)) void gemm_tiled_pc(const bf16_t* __restrict__ A, int lda, const bf16_t* __restrict__ Wp,
                                                     void* C, int ldc, int M, int N, int Kp, EpiDev epi, int tiles_m,
                                                     int tiles_n, int kt_per, float* __restrict__ partial) {
    PCTL(0);
    constexpr int NCW = CGM * CGN;                            // MFMA waves: a CGM x CGN grid of (WM*16) x (WN*16) wave tiles
    constexpr int BM_ = CGM * WM * 16, BN_ = CGN * WN * 16;
    constexpr int A_BYTES = BM_ * BK * 2, B_BYTES = BN_ * BK * 2;
    constexpr int AT = A_BYTES / 1024, BT = B_BYTES / 1024;   // 1-KiB LDS-DMA instructions per k-tile (all by the loaders)
    static_assert((NST - 2) * ((AT + BT) / NL) <= 63, "counted vmcnt must fit its 6-bit field");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;                   // [NST][A_BYTES]
    char* Bs = smem + NST * A_BYTES;   // [NST][B_BYTES]
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    {
        const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
        const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        bid = base + (bid >> 3);
    }
    const int tn = bid / tiles_m, tm = bid % tiles_m;
    const int m0 = tm * BM_, n0 = tn * BN_;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int K32 = Kp >> 5;
    const int N16 = (N + 15) >> 4;
    const int nk_total = Kp / BK;
    const int kt0 = blockIdx.y * kt_per;
    const int nk = min(kt_per, nk_total - kt0);

    if (w >= NCW) {   // ---------------- loader waves: NL of them, loader l owns the pieces j = l, l + NL, ... of every tile ----------------
        // (one wave issues an LDS-DMA piece every ~60 cycles; the CU's vector memory path takes 1 KiB per 16 cycles, so a
        // single loader caps the fill at a quarter of what the CU can pull)
        constexpr int PT = (AT + BT) / NL;
        static_assert((AT + BT) % NL == 0 && AT % NL == 0, "pieces must split evenly over the loader waves");
        static_assert((NST - 2) * PT <= 63, "counted vmcnt must fit its 6-bit field");
        const int l = w - NCW;
        const bf16_t* src[PT];
        uint32_t dst[PT];
        size_t step[PT];
        const uint32_t as_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(As));
        const uint32_t bs_u32 = __builtin_amdgcn_readfirstlane(lds_addr_u32(Bs));
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const int j = l + i * NL;
            if (j < AT) {   // A: LDS chunk position p = j*64 + lane: row = p>>3, c = p&7 holds global chunk c ^ (row&7)
                const int row = j * 8 + (lane >> 3), c = lane & 7;
                int gr = m0 + row;
                gr = gr < M ? gr : M - 1;
                src[i] = A + (size_t)gr * lda + (size_t)kt0 * BK + ((c ^ (row & 7)) << 3);
                dst[i] = as_u32 + j * 1024;
                step[i] = BK;
            } else {
                const int jb = j - AT;
                const int nbi = jb >> 1, kbi = jb & 1;
                int nb = (n0 >> 4) + nbi;
                nb = nb < N16 ? nb : N16 - 1;
                src[i] = Wp + ((size_t)nb * K32 + (size_t)kt0 * 2 + kbi) * 512 + lane * 8;
                dst[i] = bs_u32 + jb * 1024;
                step[i] = 2 * 512;
            }
        }
        // (Register-staged loaders -- plain global loads into two register sets, ds_write_b128 into a 2-stage ring -- were
        // built and measured: 64x128 o_proj 45 -> 62 us, down 87 -> 151 us, 128x256 at M = 2624 831 -> 641 TF. The LDS-DMA
        // piece stays, at 64-100 cycles of issue per wave: cycle counters (-DCOVER_PC_DEBUG, tools/exp_pc_debug.py) give per
        // k-tile of the 128x256 kernel: loader issue 770-1200, data wait 70-100, barrier 270-500; MFMA wave: 900 compute +
        // 540-690 at the barrier. s_setprio 3 on the loaders changes nothing.)
        auto issue = [&](int buf, int kt) {
#pragma unroll
            for (int i = 0; i < PT; ++i) {
                const bool is_a = (l + i * NL) < AT;
                if (!((PC_ABL(4) && !is_a) || (PC_ABL(8) && is_a)))
                    glds16_asm(src[i] + kt * step[i], dst[i] + buf * (is_a ? A_BYTES : B_BYTES));
            }
        };
#pragma unroll
        for (int s = 0; s < NST - 1; ++s)
            if (s < nk) issue(s, s);
        int cur = 0;
#ifdef COVER_PC_DEBUG
        unsigned long long tw = 0, tb = 0, ti = 0;
#endif
        for (int kt = 0; kt < nk; ++kt) {
#ifdef COVER_PC_DEBUG
            const unsigned long long c0 = PCT();
#endif
            const int younger = min(nk - 1 - kt, NST - 2);   // tiles issued after kt that may stay in flight
            if (NST >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PT) : "memory");
            else if (younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PT) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef COVER_PC_DEBUG
            const unsigned long long c1 = PCT();
#endif
            __builtin_amdgcn_s_barrier();
#ifdef COVER_PC_DEBUG
            const unsigned long long c2 = PCT();
#endif
            if (kt + NST - 1 < nk) issue(cur == 0 ? NST - 1 : cur - 1, kt + NST - 1);   // stage (kt-1) % NST
            cur = cur == NST - 1 ? 0 : cur + 1;
#ifdef COVER_PC_DEBUG
            const unsigned long long c3 = PCT();
            tw += c1 - c0; tb += c2 - c1; ti += c3 - c2;
#endif
        }
#ifdef COVER_PC_DEBUG
        if (lane == 0 && l == 0) { atomicAdd(&g_pc_dbg[0], tw); atomicAdd(&g_pc_dbg[1], tb); atomicAdd(&g_pc_dbg[2], ti); atomicAdd(&g_pc_dbg[5], (unsigned long long)nk); }
#endif
        return;
    }
    // ---------------- MFMA waves ----------------
    const int wm = w / CGN, wn = w % CGN;
    const int r = lane & 15, g = lane >> 4;
    f32x4 acc[WN][WM];  // [n-block b][m-frag f]
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
        for (int f = 0; f < WM; ++f) acc[b][f] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // Software-pipelined over the two 32-wide k-steps of a tile: the fragments of the NEXT step (the next tile's first step
    // after the mid-tile barrier) are read from LDS before the MFMAs of the current one, so a wave alone on its SIMD
    // never exposes LDS latency or the barrier between its MFMA groups.
    //   prologue: barrier 0, read(tile 0, step 0) -> set A
    //   tile kt:  read(kt, 1) -> B | MFMA(A) | reads returned, barrier kt+1, read(kt+1, 0) -> A | MFMA(B)
    // A consumer reaching barrier kt+1 holds every fragment of tile kt - 1 and of tile kt in registers (lgkmcnt drained), so
    // the loader may refill stage (kt-1) % NST... and stage kt % NST is only refilled after barrier kt+2.
    // The LDS reads are inline asm with hand-counted lgkmcnt waits (the compiler's own bookkeeping drains lgkmcnt to 0
    // before the first MFMA of a group, i.e. it also waits for the fragments just requested for the NEXT group).
    const uint32_t a_addr0 = lds_addr_u32(As) + ((wm * (WM * 16) + r) * 8 + ((0 * 4 + g) ^ (r & 7))) * 16;
    const uint32_t a_addr1 = lds_addr_u32(As) + ((wm * (WM * 16) + r) * 8 + ((1 * 4 + g) ^ (r & 7))) * 16;
    const uint32_t b_addr = lds_addr_u32(Bs) + (wn * WN * 2 * 64 + lane) * 16;
    auto read_frags = [&](int stage, int ks, u32x4(&xf)[WM], u32x4(&wf)[WN]) {
        const uint32_t aa = (ks ? a_addr1 : a_addr0) + stage * A_BYTES;
        const uint32_t ba = b_addr + stage * B_BYTES + ks * 1024;
        if (!PC_ABL(2)) {
#pragma unroll
            for (int f = 0; f < WM; ++f) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(xf[f]) : "v"(aa), "n"(f * 2048));
#pragma unroll
            for (int b = 0; b < WN; ++b) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(wf[b]) : "v"(ba), "n"(b * 2048));
        }
    };
    auto landed = [&](u32x4(&xf)[WM], u32x4(&wf)[WN]) {   // ties the fragments to the wait that precedes this call
#pragma unroll
        for (int f = 0; f < WM; ++f) asm volatile("" : "+v"(xf[f]));
#pragma unroll
        for (int b = 0; b < WN; ++b) asm volatile("" : "+v"(wf[b]));
    };
    auto mfmas = [&](const u32x4(&xf)[WM], const u32x4(&wf)[WN]) {
        if (!PC_ABL(1)) {
#pragma unroll
            for (int b = 0; b < WN; ++b)
#pragma unroll
                for (int f = 0; f < WM; ++f)
                    acc[b][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wf[b]), __builtin_bit_cast(bf16x8, xf[f]), acc[b][f], 0, 0, 0);
        }
    };
#ifdef COVER_PC_ABL
    u32x4 xa[WM] = {}, wa[WN] = {}, xb[WM] = {}, wb[WN] = {};   // (the read-skipping arm multiplies whatever is here)
#else
    u32x4 xa[WM], wa[WN], xb[WM], wb[WN];
#endif
    int cur = 0;
#if defined(COVER_PC_PRIO) && COVER_PC_PRIO
    __builtin_amdgcn_s_setprio(COVER_PC_PRIO);   // experiment: static issue priority for the MFMA waves over the loader waves (guide T5, static form)
#endif
    __builtin_amdgcn_s_barrier();
    PCTL(1);
#ifdef COVER_PC_DEBUG
    unsigned long long dbg_bar = 0;
    const unsigned long long dbg_t0 = PCT();
    const unsigned long long dbg_w0 = wall_clock64();
#endif
    read_frags(0, 0, xa, wa);
    for (int kt = 0; kt < nk; ++kt) {
        read_frags(cur, 1, xb, wb);
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(WM + WN));   // set A (older) has landed, set B stays in flight
        landed(xa, wa);
        mfmas(xa, wa);
        __builtin_amdgcn_sched_barrier(0);
        cur = cur == NST - 1 ? 0 : cur + 1;
        if (kt + 1 < nk) {
#ifdef COVER_PC_DEBUG
            const unsigned long long c0 = PCT();
#endif
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#ifdef COVER_PC_DEBUG
            dbg_bar += PCT() - c0;
#endif
            read_frags(cur, 0, xa, wa);
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(WM + WN));
        } else {
            asm volatile("s_waitcnt lgkmcnt(0)");
        }
        landed(xb, wb);
        mfmas(xb, wb);
        __builtin_amdgcn_sched_barrier(0);
    }
#ifdef COVER_PC_DEBUG
    if (lane == 0 && w == 0) { atomicAdd(&g_pc_dbg[3], dbg_bar); atomicAdd(&g_pc_dbg[4], PCT() - dbg_t0); atomicAdd(&g_pc_dbg[6], wall_clock64() - dbg_w0); }
#endif
    PCTL(2);
    tiled_epilogue_staged<WM, WN, BM_, BN_>(acc, epi, C, ldc, M, N, m0, n0, m0 + wm * (WM * 16), n0 + wn * (WN * 16), r, g, partial, smem,
                                            NST * (A_BYTES + B_BYTES), tid, 64 * NCW);
    PCTL(3);
}

// the launch of a GK_TILED / GK_TILED_PC plan (launch_gemm_bf16 routes here; the plan counter is the router's)
hipError_t launch_gemm_tiled(const GemmPlan& p, const bf16_t* A, int lda, const bf16_t* Wp, void* C, int ldc, int M, int N, int Kp, const EpiDev& epi,
                             float* partial, int variant, int tcls, double twork, hipStream_t st) {
    const dim3 grid(p.tiles_m * p.tiles_n, p.S), block(p.block);
#define T(KFN) launch_kernel<KFN>(tcls, twork, grid, block, p.lds, st, A, lda, Wp, C, ldc, M, N, Kp, epi, p.tiles_m, p.tiles_n, p.kt_per, partial)
    hipError_t e;
    if (p.kind == GK_TILED_PC) {
        e = T((gemm_tiled_pc<2, 4, 4, 4>));   // 64 x 128 tile, four loader waves + four MFMA waves, four stages (narrow outputs on a long K at a few hundred rows)
    } else if (variant == 2) {
        e = p.pick == TP_128x128 ? T((gemm_tiled<4, 4, false, 2, 2, 2>)) : p.pick == TP_64x128 ? T((gemm_tiled<2, 4, false, 2, 2, 2>)) : T((gemm_tiled<2, 2, false, 2, 2, 2>));
    } else {
        switch (p.pick) {
            case TP_128x128: e = T((gemm_tiled<4, 4, true, 2, 2, 2>)); break;
            case TP_64x128: e = T((gemm_tiled<2, 4, true, 2, 2, 2>)); break;
            case TP_64x64: e = T((gemm_tiled<2, 2, true, 3, 2, 2>)); break;
            case TP_128x128_S4: e = T((gemm_tiled<4, 4, true, 4, 2, 2>)); break;
            case TP_256x128: e = T((gemm_tiled<4, 4, true, 3, 4, 2>)); break;
            case TP_128x256: e = T((gemm_tiled<4, 4, true, 3, 2, 4>)); break;
            case TP_64x128_S3: e = T((gemm_tiled<2, 4, true, 3, 2, 2>)); break;
            case TP_128x128_S3: e = T((gemm_tiled<4, 4, true, 3, 2, 2>)); break;
            default: e = T((gemm_tiled<2, 4, true, 4, 4, 2>)); break;   // TP_128x128_W8
        }
    }
#undef T
    if (e == hipSuccess) e = hipGetLastError();
    return e;
}
