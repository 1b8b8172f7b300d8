// The GEMM planner: which kernel family, tile, grid and K split launch_gemm_bf16 (gemm_bf16.hip) takes for a problem, and what completes
// it. Host code only and no HIP call: cover_gemm_plan answers from here without a GPU, and the launchers in gemm_stream.hip / gemm_tiled.hip /
// gemm_v3.hip / gemm_fp8.hip / gemm_reduce.hip carry out the GemmPlan (gemm_common.h) they are handed. The measurement comments are the record of why each rule exists.
#include <stdlib.h>
#include <atomic>
#include "gemm_common.h"

// which plan every GEMM launch took since the last reset (cover_gemm_plan_counts: tests assert the tile a shape really ran on): GemmPlan.slot
static std::atomic<long long> g_plan_counts[COVER_GEMM_PLANS];
void plan_hit(int i) { g_plan_counts[i].fetch_add(1, std::memory_order_relaxed); }
void gemm_plan_counts(long long* out, int n, int reset) {
    for (int i = 0; i < COVER_GEMM_PLANS; ++i) {
        const long long v = reset ? g_plan_counts[i].exchange(0, std::memory_order_relaxed) : g_plan_counts[i].load(std::memory_order_relaxed);
        if (out && i < n) out[i] = v;
    }
}

// ---- the knobs, in one place. All are experiment knobs; these are read once per process ...
struct PlanKnobs {
    const char* tile_pick;   // COVER_TILE_PICK: a row of the tile table, by its digit / letter ('a' = 10 ... 'i' = 18, 'n' = 23 ... 'u' = 30; b .. i: fp8 operands only)
    int tile_split;          // COVER_TILE_SPLIT: force the number of K slices of a tiled GEMM (0: not set)
    bool v3_f8;              // COVER_V3_F8: 0 keeps the loader-wave form of the self-loading fp8 tiles
    int sk_slots;            // COVER_SK_SLOTS: resident blocks the second streaming generation sizes its grid for (2 blocks per CU x 256 CUs)
    bool skinny3;            // COVER_SKINNY3: 0 disables the automatic choice of the third streaming generation
};
static const PlanKnobs& plan_knobs() {
    auto off = [](const char* v) { return v && v[0] == '0'; };
    auto num = [](const char* v, int unset) { return v ? atoi(v) : unset; };
    static const PlanKnobs k = {getenv("COVER_TILE_PICK"), num(getenv("COVER_TILE_SPLIT"), 0), !off(getenv("COVER_V3_F8")),
                                num(getenv("COVER_SK_SLOTS"), 512), !off(getenv("COVER_SKINNY3"))};
    return k;
}
// ... and COVER_FP8_MFMA per call (a test flips it mid-process): 0 keeps the bf16 MFMA path on fp8 operands
static bool fp8_mfma_on(const EpiDev& epi) {
    const char* f8_env = epi.a8 ? getenv("COVER_FP8_MFMA") : nullptr;
    return epi.a8 && !(f8_env && f8_env[0] == '0');
}

// ---- weight streaming (M <= 64)
// what the third generation can run at all: two 16-row fragments, an even number of 16-column blocks, two 1024-wide chunks per block
static bool skinny3_legal(int M, int N, int Kp) { return !(M > 32 || (((N + 15) / 16) & 1) || Kp < 2048); }

// Third-generation plan: NBW n-blocks per wave (x NG = 2 n-groups) and S grid-level K slices such that the grid is as close
// to ONE block per CU (128 KiB of LDS) as possible; every block must see at least two 1024-wide chunks (otherwise the
// second generation does the same work with two blocks per CU).
static Skinny3Plan plan_skinny3(int M, int N, int Kp) {
    Skinny3Plan best = {};   // (zeroed: gemm_workspace_bytes and plan_streaming read S / ws_bytes of a plan that is not ok)
    best.MF = (M + 15) / 16;
    const int N16 = (N + 15) / 16;
    if (!skinny3_legal(M, N, Kp)) return best;
    int best_blocks = 0;
    const int nbws[3] = {4, 3, 2};
    for (int bi = 0; bi < 3; ++bi) {
        const int nbw = nbws[bi];
        const int gx = (N16 + 2 * nbw - 1) / (2 * nbw);
        for (int S = 1; S <= 8; ++S) {
            if ((long long)gx * S > 256) break;
            // slice width: whole 1024-wide chunks when that still leaves work for the last slice (every chunk of the other
            // slices then runs through the straight-line loop; down of a 7B decoder: 24.65 -> 24.0 us), else 256-granular
            const int kraw = (Kp + S - 1) / S;
            int kper = (kraw + 1023) / 1024 * 1024;
            if ((long long)kper * (S - 1) >= Kp) kper = (kraw + 255) / 256 * 256;
            if (kper < 2048) break;                      // fewer than two chunks per block
            if ((long long)kper * (S - 1) >= Kp) continue;  // an empty last slice
            const int blocks = gx * S;
            // more blocks first; then fewer slices (less partial traffic); then more n-blocks per wave (longer streams)
            if (blocks > best_blocks) {
                best_blocks = blocks;
                best.ok = true; best.NBW = nbw; best.S = S; best.kper = kper; best.gx = gx;
            }
        }
    }
    if (!best.ok || best_blocks < 190) { best.ok = false; return best; }
    best.lds = (size_t)2 * best.MF * 16 * 1024 * 2;
    best.ws_bytes = best.S > 1 ? (size_t)best.S * M * N * sizeof(float) : 0;
    return best;
}

static SkinnyPlan plan_skinny(int M, int N, int Kp) {
    SkinnyPlan p;
    p.MF = (M + 15) / 16;
    const int N16 = (N + 15) / 16;
    p.nbpb = N16 >= 1024 ? 16 : 8;
    p.gx = (N16 + p.nbpb - 1) / p.nbpb;
    const int kc_max = (64 * 1024) / (p.MF * 16 * 2) / 128 * 128;  // LDS <= 64 KiB -> 2 blocks per CU
    int S = (512 + p.gx - 1) / p.gx;
    int kb = Kp / 128;
    if (S > kb) S = kb;
    if (S < 1) S = 1;
    int KC = ((kb + S - 1) / S) * 128;
    if (KC > kc_max) KC = kc_max;
    p.KC = KC;
    p.S = (Kp + KC - 1) / KC;
    p.lds = (size_t)p.MF * 16 * KC * 2;
    p.ws_bytes = (size_t)p.S * M * N * sizeof(float);
    return p;
}

static Skinny2Plan plan_skinny2(int M, int N, int Kp) {
    Skinny2Plan p;
    p.MF = (M + 15) / 16;
    p.KS = p.MF <= 2 ? 4 : 2;
    const int KC = 256 * p.KS, NG = 8 / p.KS;
    p.S = (Kp + KC - 1) / KC;
    const int N16 = (N + 15) / 16;
    // NBW (n-blocks per wave): the smallest of {2,3,4,6} for which the whole grid is ONE wave of resident blocks
    // (2 blocks per CU x 256 CUs): a second, partially filled wave of blocks leaves CUs idle while the last blocks stream.
    const int slots = plan_knobs().sk_slots;
    if (p.MF <= 2) {
        const int cand[4] = {2, 3, 4, 6};
        p.NBW = 4;
        bool found = false;
        for (int c = 0; c < 4 && !found; ++c) {
            const long long blocks = (long long)((N16 + NG * cand[c] - 1) / (NG * cand[c])) * p.S;
            if (blocks <= slots) { p.NBW = cand[c]; found = true; }
        }
    } else {
        p.NBW = 2;  // the LDS reduction buffer (8 * NBW * MF KiB per round) and the accumulators bound it
    }
    p.gx = (N16 + NG * p.NBW - 1) / (NG * p.NBW);
    const int rb = (8 / p.MF) < p.NBW ? (8 / p.MF) : p.NBW;
    const size_t x = (size_t)p.MF * 16 * KC * 2, red = (size_t)8 * rb * p.MF * 4 * 64 * 4;
    p.lds = x > red ? x : red;
    p.ws_bytes = (size_t)p.S * M * N * sizeof(float);
    return p;
}

// The third generation (full-K chunk loop per block, one block per CU) whenever its plan fills the chip and its slabs fit,
// else the second generation (in-block k-slices).
hipError_t plan_streaming(GemmPlan& p, int M, int N, int Kp, const float* ws, size_t ws_bytes, bool forced3, bool all_slabs) {
    p.pick = -1;
    Skinny3Plan p3 = plan_skinny3(M, N, Kp);
    if (forced3 && !p3.ok) {
        if (!skinny3_legal(M, N, Kp)) return hipErrorInvalidValue;
        p3.ok = true; p3.NBW = 3; p3.S = 1; p3.kper = Kp; p3.gx = ((N + 15) / 16 + 5) / 6;
        p3.lds = (size_t)2 * p3.MF * 16 * 1024 * 2; p3.ws_bytes = 0;
    }
    const size_t need3 = all_slabs ? (size_t)p3.S * M * N * sizeof(float) : p3.ws_bytes;
    if (p3.ok && need3 > 0 && (ws == nullptr || ws_bytes < need3)) p3.ok = false;
    if (p3.ok && (forced3 || plan_knobs().skinny3)) {
        p.kind = GK_SKINNY3; p.slot = PLAN_SKINNY3; p.p3 = p3; p.S = p3.S; p.lds = p3.lds;
        return hipSuccess;
    }
    if (forced3 || M > 64) return hipErrorInvalidValue;
    const Skinny2Plan p2 = plan_skinny2(M, N, Kp);
    if (ws == nullptr || ws_bytes < p2.ws_bytes) return hipErrorInvalidValue;
    p.kind = GK_SKINNY2; p.slot = PLAN_SKINNY2; p.p2 = p2; p.S = p2.S; p.lds = p2.lds;
    return hipSuccess;
}

// ---- the LDS-tiled kernels: tile configurations {wave tile (WM, WN) in 16-row units, wave grid, stages}, indexed by TilePick, and the ONE
// statement of which rows are forms of the same tile: v3 = the self-loading form (gemm_v3.hip) of a loader-wave row, f8 = the fp8 tile
// (gemm_fp8.hip numbers its kernels by loader-wave row) that a self-loading row becomes on fp8 operands; -1 = none
struct TileCfg { int wm, wn, wgm, wgn, nst, v3 = -1, f8 = -1; };
static const TileCfg k_tiles[32] = {
    {4, 4, 2, 2, 2},   // TP_128x128:     4 waves of 64x64, 2 stages (64 KiB)
    {2, 4, 2, 2, 2},   // TP_64x128:      4 waves of 32x64, 2 stages (48 KiB)
    {2, 2, 2, 2, 3},   // TP_64x64:       4 waves of 32x32, 3 stages (48 KiB)
    {4, 4, 2, 2, 4},   // TP_128x128_S4:  4 waves, 4 stages (128 KiB, one block per CU, three k-tiles in flight)
    {4, 4, 4, 2, 3},   // TP_256x128:     8 waves of 64x64, 3 stages (144 KiB)
    {4, 4, 2, 4, 3},   // TP_128x256:     8 waves of 64x64, 3 stages (144 KiB)
    {2, 4, 4, 2, 4},   // TP_128x128_W8:  8 waves of 32x64, 4 stages (128 KiB)
    {2, 4, 2, 2, 3},   // TP_64x128_S3:   4 waves, 3 stages (72 KiB, two blocks per CU, two k-tiles in flight each)
    {4, 4, 2, 2, 3},   // TP_128x128_S3:  4 waves, 3 stages (96 KiB, one block per CU)
    {2, 4, 2, 2, 3},   // TP_PC_64x128_S3:  loader wave + 4 MFMA waves, 3 stages (72 KiB)
    {2, 4, 2, 2, 4},   // TP_PC_64x128:     loader wave + 4 MFMA waves, 4 stages (96 KiB)
    {4, 4, 2, 2, 3},   // TP_PC_128x128:    loader wave + 4 MFMA waves, 3 stages (96 KiB)
    {4, 4, 4, 2, 3, TP_V3_256x128},   // TP_PC_256x128:    4 loader waves + 8 MFMA waves of 64x64, 3 stages (144 KiB)
    {4, 4, 2, 4, 3, TP_V3_128x256},   // TP_PC_128x256:    4 loader waves + 8 MFMA waves of 64x64, 3 stages (144 KiB)
    // 224-row tiles (M = 448 = 2 x 224: no row padding, and the column width is chosen per GEMM so that the whole tile
    // grid is ONE round of <= 256 blocks): 4 loader waves + MFMA waves of 112 x 48 / 112 x 32
    {7, 3, 2, 2, 4},   // TP_PC_224x96_W4:  4 MFMA waves of 112x48 + 4 loaders, 4 stages (160 KiB)
    {7, 2, 2, 4, 3, TP_V3_224x128},   // TP_PC_224x128:    8 MFMA waves of 112x32 + 4 loaders, 3 stages (132 KiB)
    {7, 3, 2, 4, 3, TP_V3_224x192},   // TP_PC_224x192:    8 MFMA waves of 112x48 + 4 loaders, 3 stages (156 KiB)
    {7, 2, 2, 3, 4, TP_V3K_224x96},   // TP_PC_224x96:     6 MFMA waves of 112x32 + 4 loaders, 4 stages (160 KiB); (round 6: self-loading on k-split wave pairs)
    {4, 3, 2, 4, 3},   // TP_PC_128x192:    8 MFMA waves of 64x48 + 4 loaders, 3 stages (120 KiB) -- fp8 instantiation only (gemm_fp8.hip)
    {}, {}, {}, {},    // (19..22: plan-counter slots of the weight-streaming / fp8 kernels)
    // self-loading 8-wave tiles (gemm_v3.hip): no loader waves, fragment reads and LDS-DMA pieces interleaved with the MFMAs
    {7, 3, 2, 4, 3},                      // TP_V3_224x192: 8 waves of 112x48, 3 stages (156 KiB); no fp8 instantiation (registers)
    {7, 2, 2, 4, 3, -1, TP_PC_224x128},   // TP_V3_224x128: 8 waves of 112x32, 3 stages (132 KiB)
    {8, 2, 2, 4, 3, -1, TP_PC_256x128},   // TP_V3_256x128: 8 waves of 128x32, 3 stages (144 KiB)
    {4, 4, 2, 4, 3, -1, TP_PC_128x256},   // TP_V3_128x256: 8 waves of 64x64,  3 stages (144 KiB)
    {7, 3, 2, 2, 4, -1, TP_PC_224x96},    // TP_V3_224x96:  4 waves of 112x48 (one per SIMD), 4 stages (160 KiB)
    {}, {},            // (28, 29: 112x128 and 224x128 on four waves -- measured slower in round 5, removed in round 6)
    // k-split wave pairs (gemm_v3.hip gemm_tiled_v3k): 2 x 2 wave tiles, each owned by the two waves of a SIMD, which split every k-tile
    {7, 3, 2, 2, 4},   // TP_V3K_224x96: 4 wave pairs of 112x48, 4 stages (160 KiB); no f8 column: on fp8 operands it has always fallen to 64 x 128
    {},                // (31: 224x128 on wave pairs of 112x64 and 224x64 on pairs of 112x32 were built and not kept; gemm_v3.hip)
};
static inline bool f8_self_loading(int pick) { return pick == TP_PC_256x128 || pick == TP_PC_128x256 || pick == TP_PC_224x128 || pick == TP_PC_128x192; }
static inline int tile_bm(int pick) { return k_tiles[pick].wm * k_tiles[pick].wgm * 16; }
static inline int tile_bn(int pick) { return k_tiles[pick].wn * k_tiles[pick].wgn * 16; }

static const int kSplitBelowBlocks = 192;   // a tile grid of fewer blocks than this (three quarters of the 256 CUs) doubles its K slices
static const int kRoundBlocks = 256;        // one round of blocks: one per CU for the one-block-per-CU tiles
static const int kMaxSplit = 8;             // K slices at most

// One tiled problem (variants 1 / 2) as every step sees it: plan_tiles's arguments, the per-call knob, and which families are open to it
struct TileJob {
    int lda, M, N, Kp, variant;
    const EpiDev& epi;
    const float* ws; size_t ws_bytes;
    bool mx_any;
    bool f8_on;   // both operands e4m3 and COVER_FP8_MFMA not 0: the fp8 kernels
    bool v3_on;   // the self-loading bf16 kernels (gemm_v3.hip): they address an activation piece with a 32-bit lane offset; the bf16 loader-wave
                  // forms of these tiles (rounds 2-4) live in docs/experiments/r06_pruned_variants.patch
    long long blocks(int pick) const { return (long long)((M + tile_bm(pick) - 1) / tile_bm(pick)) * ((N + tile_bn(pick) - 1) / tile_bn(pick)); }
};
struct TileChoice { int pick, S; };   // S = 0: no K split chosen with the tile (step 7's grid rule decides)

// Step 2: the default tile by grid size.
static int default_tile(const TileJob& j) {
    // Measured on MI355X (tools/bench_kernels.py, M = 441): this single-barrier-per-k-tile structure is latency-bound per
    // block, so residency beats tile size until the tile grid oversubscribes the chip several times over, while 64x64
    // tiles on a wide N become L2-traffic-bound (the activation panel is re-read N/64 times).
    int pick = TP_128x128;
    // (tools/exp_tiles.py re-reads one weight matrix, i.e. measures Infinity-Cache-warm: there 128x128 wins already at 688
    // tiles (N = 22016, M = 449); inside the decision, with cold weights, it does not -- 137 vs ~130 us -- so 1024 stays)
    if (j.blocks(TP_128x128) < 1024) pick = (j.blocks(TP_64x128) >= 384) ? TP_64x128 : TP_64x64;
    // a 64x128 grid of about one block per CU on a long K (M = 448: o_proj / down of a 7B decoder) is latency-bound per block:
    // deeper rings beat the 64x64 tile there (cold weights, down / o_proj: 64x64 90.9 / 35.7 us, 64x128 3-stage 81.9 / 35.6,
    // 64x128 with a loader wave and 4 stages 78.2 / 34.6). For the multi-round grids (qkv, gate_up) neither the deeper ring
    // nor the loader wave helps (they cost a resident block per CU): 2 stages x 3 blocks stays.
    if (pick == TP_64x64 && j.blocks(TP_64x128) >= 192 && j.Kp >= 4096) pick = TP_PC_64x128;   // 4 stages: 83.4 -> 78.2 us (down), 35.9 -> 34.6 (o_proj)
    // 8 MFMA waves of 64x64 + 4 loader waves on 256x128 / 128x256 tiles (3 stages, one block per CU): per k-tile a SIMD has 1024
    // cycles of MFMA against 768 cycles of LDS-DMA on the CU's address path, and none of the DMA issue sits in an MFMA wave.
    // Cold weights: M = 2624 qkv 715 -> 867 TF, gate_up 792 -> 1026 TF, down 660 -> 833 TF (M = 448 in isolation: qkv 80.5 ->
    // 75.1 us, gate_up 125.8 -> 119.1 us). Narrow outputs keep the smaller tiles (o_proj: 664 vs 701 TF at M = 2624).
    // (at M = 448 the micro-benchmark gain does not survive inside the decision -- 41.22 vs 40.98 ms -- so: long panels only)
    // M = 512 (decode rows of BASELINE config 5: N = 512 candidates) is two 256-row tiles: qkv 75.4 -> 60.2 us, gate_up 135.9 -> 116.9,
    // down 73.1 -> 48.4 + 13.5 (four K slices + reduction); o_proj stays on the 64 x 128 tiles (29.0 vs 25.4 + 13.5).
    if (j.variant != 2 && j.Kp >= 2048 && j.M >= 512) {
        if (j.N > 4096 && j.blocks(TP_PC_128x256) >= 176) pick = j.N >= 16384 ? TP_PC_256x128 : TP_PC_128x256;
        else if (j.N <= 4096 && j.Kp >= 8192 && (j.blocks(TP_PC_256x128) >= 256 || (j.M < 1024 && j.ws != nullptr))) pick = TP_PC_256x128;
    }
    return pick;
}

// Step 3: the fp8 tile by grid-coverage cost.
static int fp8_tile(const TileJob& j, int pick) {
    // fp8 operands (config 5, M = 512 decode rows): with half the bytes per FLOP the 12-wave tiles are bound by how evenly the tile grid
    // covers the 256 CUs, not by the fill: qkv (N = 12288) is 192 tiles of 256 x 128 / 128 x 256 -- a quarter of the chip idle -- but
    // exactly 256 tiles of 128 x 192; gate_up (N = 22016) is 344 tiles (two rounds, the second a third full) or 460 of 128 x 192
    // (two rounds of a 0.79 x tile). Cost = rounds x (0.55 area + 0.45 perimeter), normalised to the 256 x 128 tile; measured at
    // M = 512: qkv 35 -> 28 us, gate_up 70 -> 54 us.
    if (!(j.f8_on && j.variant != 2 && j.Kp >= 2048 && j.M >= 512 && j.N > 4096)) return pick;
    const int idx[3] = {TP_PC_256x128, TP_PC_128x256, TP_PC_128x192};
    double best = 1e30;
    for (int c = 0; c < 3; ++c) {
        const int bm_ = tile_bm(idx[c]), bn_ = tile_bn(idx[c]);
        if (j.epi.glu && (bn_ % 32)) continue;
        const long long rounds = (j.blocks(idx[c]) + kRoundBlocks - 1) / kRoundBlocks;
        const double cost = rounds * (0.55 * (double)bm_ * bn_ / 32768.0 + 0.45 * (double)(bm_ + bn_) / 384.0);
        if (cost < best) { best = cost; pick = idx[c]; }
    }
    return pick;
}

// Step 4: the 224-row tile AND its K split, by the fitted cost model.
static TileChoice tile_224(const TileJob& j, TileChoice ch) {
    // 224-row tiles: M = 448 -- the OpenVLA prefill pass: 256 patch rows + 8 prompts x 24 text rows -- is exactly two
    // of them, where 128-row tiles pad 12.5 % and 64 x 128 tiles need 1.3-2.7 rounds of blocks. The column width and the number of
    // K slices are chosen per GEMM so that the grid is ONE round of <= 256 blocks, with a cost model fitted to per-block timelines
    // (tools/dbg/pc_timeline.py; us per 64-deep k-tile: 224x96 0.67, 224x128 0.70, 224x192 1.05; ~5 us of prologue + epilogue
    // per block; split-K reduction ~4 us + slab bytes at 3 TB/s). Cold weights, M = 448, kernel timestamps, before -> after:
    // qkv 81.5 -> 52 us (224x96/128), gate_up 138 -> 78.5 us (224x192, 1.03 PFLOP/s), down 72.6 + norm -> 43 + 10 us (224x128, 4 slices).
    const int M = j.M, N = j.N, Kp = j.Kp, t224 = (M + 223) / 224, waste224 = t224 * 224 - M;
    if (!(j.variant != 2 && Kp >= 2048 && M >= 400 && waste224 * 10 <= M && (j.v3_on || j.f8_on))) return ch;
    // loader-wave kernels (gemm_tiled_pc): 224x96 (6 MFMA waves) / 224x128 / 224x192; self-loading kernels (gemm_v3.hip, round 5,
    // in-kernel probe of workgroup 0 at M = 448 / 2232): 224x96 with one wave of 112x48 per SIMD 0.62 us per k-tile, 224x128
    // 0.69-0.78, 224x192 0.91-1.02; prologue + epilogue 6 / 7 / 10 us
    // (round 6: 224x96 on k-split wave pairs instead of one wave per SIMD)
    const int cand[3] = {TP_PC_224x96, TP_PC_224x128, TP_PC_224x192};   // (their self-loading forms: the tile table's v3 column)
    const double kt_pc[3] = {0.67, 0.70, 1.05}, kt_v3[3] = {0.60, 0.72, 0.93}, fix_v3[3] = {6.0, 7.0, 10.0};
    double best = 1e30;
    for (int c = 0; c < 3; ++c) {
        const int bn = tile_bn(cand[c]);
        if (j.epi.glu && (bn % 32)) continue;
        if (j.f8_on && bn == 192) continue;   // no fp8 instantiation of the 224 x 192 tile (registers)
        if (j.mx_any && bn == 96) continue;   // (the fp8 224 x 96 tile is a loader-wave kernel: no block scales)
        for (int S = 1; S <= kMaxSplit; S *= 2) {
            if (S > 1 && (j.ws == nullptr || (size_t)S * M * N * sizeof(float) > j.ws_bytes || j.epi.glu || (Kp / BK) / S < 8)) break;
            const long long blocks = (long long)t224 * ((N + bn - 1) / bn) * S;
            const long long rounds = (blocks + kRoundBlocks - 1) / kRoundBlocks;
            double us = rounds * ((j.v3_on ? kt_v3[c] : kt_pc[c]) * ((Kp / BK + S - 1) / S) + (j.v3_on ? fix_v3[c] : 5.0));
            if (S > 1) us += 4.0 + (double)S * M * N * 4.0 / 3.0e6;
            else if (j.epi.norm_w != nullptr && j.epi.norm_out != nullptr) us += 6.0;   // the norm is its own launch without a reduction to ride on
            if (us < best) { best = us; ch.pick = j.v3_on ? k_tiles[cand[c]].v3 : cand[c]; ch.S = S; }
        }
    }
    return ch;
}

// Step 5: the forced pick (COVER_TILE_PICK). Odd but kept: the knob is applied BEFORE the family resolution, so a forced 'c' (loader-wave
// 256 x 128) becomes the self-loading tile on bf16 operands; and a set knob drops the model's K split even when its letter names no row.
static TileChoice forced_tile(TileChoice ch) {
    const char* force = plan_knobs().tile_pick;
    if (!force) return ch;
    ch.S = 0;
    if (force[0] >= '0' && force[0] <= '9') ch.pick = force[0] - '0';
    if (force[0] >= 'a' && force[0] <= 'i') ch.pick = 10 + (force[0] - 'a');
    if (force[0] >= 'n' && force[0] <= 'u' && force[0] != 's' && force[0] != 't') ch.pick = 10 + (force[0] - 'a');
    return ch;
}

// Step 6: the kernel family that realises the chosen tile. The rules run in this order (a later one sees the earlier one's result).
static hipError_t resolve_family(const TileJob& j, int& pick) {
    if (j.v3_on) {
        // the 256 x 128 / 128 x 256 tiles (M >= 512 with more than 10 % of 224-row padding: config 4's 704-row prefill) run on the self-loading
        // kernel. (Only these two: a FORCED loader-wave 224-row pick is not promoted, it falls to 128 x 128 below -- kept.)
        if (pick == TP_PC_256x128 || pick == TP_PC_128x256) pick = k_tiles[pick].v3;
    } else if (pick >= TP_V3_224x192) {
        // a self-loading pick (forced) where the bf16 self-loading kernels are off: its fp8 tile, 64 x 128 where it has none; 128 x 128 on bf16 operands
        if (!j.f8_on) pick = TP_128x128;
        else pick = k_tiles[pick].f8 >= 0 ? k_tiles[pick].f8 : TP_PC_64x128;
    }
    if (j.mx_any) {
        if (!j.f8_on) return hipErrorInvalidValue;   // (COVER_FP8_MFMA=0 with block-scaled operands)
        // any M on the 128 x 256 self-loading tile (the 64 x 128 loader-wave tile reads block scales too)
        if (!f8_self_loading(pick) && !(pick == TP_PC_64x128 && j.epi.a8mx && !j.epi.o8)) pick = TP_PC_128x256;
    }
    // bf16 operands: of the loader-wave tiles only the 64 x 128 four-stage one is still a default; the others exist as fp8 kernels
    const bool f8_only = (pick >= TP_PC_128x128 && pick <= TP_PC_128x192) || pick == TP_PC_64x128_S3;
    if (f8_only && !(j.f8_on && gemm_fp8_tiled_supported(pick))) pick = (j.variant == 2 || pick == TP_PC_64x128_S3) ? TP_64x128 : TP_128x128;
    if (j.variant == 2 && pick > TP_64x64) pick = TP_128x128;   // the register-staged A/B kernels exist for the three default tiles only
    return hipSuccess;
}

// Step 7: the K split of the resolved tile: the one chosen with the tile, else the grid rule, then COVER_TILE_SPLIT, then out8 => 1.
static int split_k(const TileJob& j, const TileChoice& ch) {
    const int nk_total = j.Kp / BK;
    const size_t slab = (size_t)j.M * j.N * sizeof(float);
    int S = 1;
    if (ch.S > 0) {
        S = ch.S;
    } else if (j.ws != nullptr) {
        while (j.blocks(ch.pick) * S < kSplitBelowBlocks && S < kMaxSplit && nk_total / (S * 2) >= 8 && (size_t)(S * 2) * slab <= j.ws_bytes) S *= 2;
        const int forced = plan_knobs().tile_split;
        if (forced >= 1 && (size_t)forced * slab <= j.ws_bytes) S = forced;
    }
    if (j.epi.o8) S = 1;   // (the block-scaled GLU output is written by the GEMM's own epilogue, not by a split-K reduction)
    return S;
}

// The workspace a caller sizes for one GEMM. It is a policy beside split_k, not a bound split_k relies on: split_k and tile_224 never split
// beyond the workspace they are given, so a GEMM this function gives nothing simply does not split.
size_t gemm_workspace_bytes(int M, int N, int K) {
    const int Kp = (K + 127) / 128 * 128;
    if (M > 64) {
        // blocks64, the smallest default tile's grid: below the threshold it implies split_k's `blocks(pick) < kSplitBelowBlocks` for every tile (a
        // larger tile has fewer blocks); a GEMM whose chosen tile alone is below it gets nothing here and stays unsplit. blocks224, the 224 x 128
        // grid, stands for tile_224's model, which splits the K of narrow outputs that leave part of a round (kRoundBlocks) idle. Either way:
        // room for kMaxSplit slabs, more than either step may take.
        const long long blocks64 = (long long)((M + 63) / 64) * ((N + 63) / 64);
        const long long blocks224 = (long long)((M + 223) / 224) * ((N + 127) / 128);
        return (blocks64 < kSplitBelowBlocks || blocks224 < kSplitBelowBlocks) ? (size_t)kMaxSplit * M * N * sizeof(float) : 0;
    }
    const size_t a = plan_skinny(M, N, Kp).ws_bytes, b = plan_skinny2(M, N, Kp).ws_bytes;
    size_t c = plan_skinny3(M, N, Kp).ws_bytes;
    const size_t one = (size_t)M * N * sizeof(float);   // launch_gemm_skinny_partial with an unsplit third-generation plan
    if (c < one) c = one;
    const size_t ab = a > b ? a : b;
    return ab > c ? ab : c;
}

// Step 8: the geometry of the launch, and the checks that need the resolved family.
static hipError_t tile_geometry(GemmPlan& p, const TileJob& j, int pick, int S) {
    const EpiDev& epi = j.epi;
    const TileCfg cd = k_tiles[pick];
    const int bm = tile_bm(pick), bn = tile_bn(pick);
    p.pick = pick;
    p.tiles_m = (j.M + bm - 1) / bm;
    p.tiles_n = (j.N + bn - 1) / bn;
    // stages: measured at M = 441 (tools/bench_kernels.py): the 64x64 tile gains 40-55 % from a third stage (48 KiB, still
    // 3 blocks/CU); 64x128 and 128x128 are bound by the bytes a CU keeps in flight (LDS capacity x resident blocks) over
    // the load latency (~12.8 TB/s chip-wide at 2 stages => 42.7 / 64 FLOP per byte).
    const int nst = j.variant == 2 ? 2 : cd.nst;
    p.lds = (size_t)nst * (bm + bn) * BK * 2;
    p.block = 64 * cd.wgm * cd.wgn;
    p.slot = pick;
    const bool f8 = j.f8_on && gemm_fp8_tiled_supported(pick);
    const int nk = f8 ? j.Kp / 128 : j.Kp / BK;   // K slices of whole k-tiles
    p.kt_per = (nk + S - 1) / S;
    p.S = (nk + p.kt_per - 1) / p.kt_per;
    if (f8) {
        // both operands e4m3: the MX-scaled matrix instruction, 128 k per k-tile (same LDS bytes per tile as 64 k of bf16), K slices of whole 128-deep tiles
        if (epi.lda8 < j.Kp || (epi.lda8 & 15)) return hipErrorInvalidValue;
        const bool v3f8 = plan_knobs().v3_f8 && (size_t)j.M * epi.lda8 + 4096 < ((size_t)1 << 31);
        p.kind = v3f8 && f8_self_loading(pick) ? GK_F8_V3 : GK_F8_PC;
        // MX block scales (operand or output) exist on the self-loading kernels and, for a8_mx, on the 64 x 128 loader-wave tile
        if (j.mx_any && p.kind != GK_F8_V3 && !(pick == TP_PC_64x128 && epi.a8mx && !epi.o8)) return hipErrorInvalidValue;
        if (epi.a8mx) p.lds += p.kind == GK_F8_V3 ? 3 * 1024 : 4 * 256;   // (+ the block-scale ring)
        if (p.kind == GK_F8_PC) p.block += 256;
        p.slot = PLAN_FP8;
        return hipSuccess;
    }
    if (pick >= TP_V3_224x192) {
        if ((size_t)j.M * j.lda * 2 + 4096 >= ((size_t)1 << 31)) return hipErrorInvalidValue;   // 32-bit lane offsets of the activation pieces
        p.kind = GK_V3;
        if (pick == TP_V3K_224x96) p.block *= 2;   // two waves per wave tile
    } else if (pick == TP_PC_64x128) {
        p.kind = GK_TILED_PC;
        p.block += 256;   // four loader waves
    } else {
        p.kind = GK_TILED;
    }
    return hipSuccess;
}

// The tile, the K split and the kernel family of an LDS-tiled GEMM (variants 1 / 2): the steps above in the one order that decides which
// override wins.
static hipError_t plan_tiles(GemmPlan& p, int lda, int M, int N, int Kp, const EpiDev& epi, const float* ws, size_t ws_bytes, int variant, bool mx_any) {
    const bool f8_on = fp8_mfma_on(epi);                                                                    // 1 (the per-call knob; the others: plan_knobs)
    const bool v3_on = !f8_on && variant != 2 && (size_t)M * lda * 2 + 4096 < ((size_t)1 << 31);
    const TileJob j = {lda, M, N, Kp, variant, epi, ws, ws_bytes, mx_any, f8_on, v3_on};
    TileChoice ch = {default_tile(j), 0};                                                                   // 2
    ch.pick = fp8_tile(j, ch.pick);                                                                         // 3
    ch = tile_224(j, ch);                                                                                   // 4
    ch = forced_tile(ch);                                                                                   // 5
    const hipError_t e = resolve_family(j, ch.pick);                                                        // 6
    if (e != hipSuccess) return e;
    return tile_geometry(p, j, ch.pick, split_k(j, ch));                                                    // 7, 8
}

hipError_t plan_gemm(GemmPlan& p, int lda, const void* C, int ldc, int M, int N, int K, const EpiDev& epi, const float* ws, size_t ws_bytes,
                     int variant, bool want_slabs) {
    p = GemmPlan{};
    p.kind = GK_NONE; p.slot = -1; p.pick = -1;
    if (M <= 0 || N <= 0) return hipSuccess;
    const int Kp = (K + 127) / 128 * 128;
    if (variant == 0) variant = (M <= 64 && ws != nullptr) ? 3 : 1;
    // MX block scales (cover_gemm_epi.a8_mx / out8): the self-loading fp8 tiles only
    const bool mx_any = epi.a8mx != nullptr || epi.o8 != nullptr;
    if (mx_any) {
        if (variant != 1 || !epi.a8 || !epi.w8 || M <= 64 || (size_t)M * epi.lda8 + 4096 >= ((size_t)1 << 31)) return hipErrorInvalidValue;
        if (epi.a8mx && (!epi.w8_kl || epi.glu)) return hipErrorInvalidValue;
        if (epi.o8 && (!epi.glu || (epi.act != ACT_SILU && epi.act != ACT_GELU_TANH) || ((N / 2) % 32) != 0 || epi.ldo8 < N / 2 || (epi.ldo8 & 15) || epi.out_f32))
            return hipErrorInvalidValue;
        if (epi.o8 && ((((uintptr_t)C) & 15) || (ldc % 8))) return hipErrorInvalidValue;   // (the bf16 tile stores the out8 epilogue stages)
    }
    // a k-linear e4m3 twin needs block-scaled activations on the fp8 tiles: per-row a8 would be read in the default image's k order
    if (epi.w8_kl && epi.a8 && !epi.a8mx && M > 64) return hipErrorInvalidValue;
    hipError_t e;
    if (variant == 3 || variant == 6) e = plan_streaming(p, M, N, Kp, ws, ws_bytes, variant == 6, false);
    else if (variant == 5) {   // first-generation weight streaming (grid-level split-K only), kept for A/B measurements
        if (M > 64) return hipErrorInvalidValue;
        p.p1 = plan_skinny(M, N, Kp);
        if (ws == nullptr || ws_bytes < p.p1.ws_bytes) return hipErrorInvalidValue;
        p.kind = GK_SKINNY; p.slot = PLAN_SKINNY; p.S = p.p1.S; p.lds = p.p1.lds;
        e = hipSuccess;
    } else e = plan_tiles(p, lda, M, N, Kp, epi, ws, ws_bytes, variant, mx_any);
    if (e != hipSuccess) return e;
    // completion: weight streaming always reduces its slabs (but an unsplit third-generation launch, which runs the fused epilogue);
    // a tiled launch reduces them when it splits K, unless the caller folds them itself
    const bool want_norm = epi.norm_w != nullptr && epi.norm_out != nullptr;
    const bool streaming = p.kind == GK_SKINNY || p.kind == GK_SKINNY2 || p.kind == GK_SKINNY3;
    const bool split = streaming ? !(p.kind == GK_SKINNY3 && p.S == 1) : p.S > 1;
    const bool norm_fusable = want_norm && !epi.glu && !epi.out_f32 && (N % 8) == 0 && N <= 8192 && (ldc % 8) == 0 && (epi.ld_norm_out % 8) == 0 &&
                              (((uintptr_t)epi.norm_w) & 15) == 0;   // the reduction launch that can carry the norm (splitk_reduce_norm)
    p.rcls = streaming ? 5 : p.kind == GK_F8_PC || p.kind == GK_F8_V3 ? 9 : (double)N * (double)Kp >= 16.0e6 ? 8 : 6;
    if (!split) p.done = GD_NONE;
    else if (!streaming && want_slabs && !epi.residual && !epi.lscale && epi.act == ACT_NONE && epi.out_scale == 1.0f && !epi.glu && !epi.norm_out)
        p.done = GD_SLABS;   // the caller folds the slabs (+ bias, bf16 rounding) itself
    else p.done = norm_fusable ? GD_REDUCE_NORM : GD_REDUCE;
    p.norm_launch = want_norm && p.done != GD_REDUCE_NORM;
    return hipSuccess;
}

hipError_t gemm_plan_query(const bf16_t* A, int lda, const bf16_t* Wp, const void* C, int ldc, int M, int N, int K, const cover_gemm_epi* epi_in,
                           const float* ws, size_t ws_bytes, int variant, int* plan) {
    GemmPlan p;
    const hipError_t e = plan_gemm(p, lda, C, ldc, M, N, K, make_epi(epi_in), ws, ws_bytes, variant, false);
    if (e != hipSuccess) return e;
    const int out[6] = {p.slot, p.pick, p.kind == GK_F8_V3 ? 1 : 0, p.S, p.done == GD_NONE ? 0 : p.done == GD_REDUCE ? 1 : 2, p.norm_launch ? 1 : 0};
    for (int i = 0; i < 6; ++i) plan[i] = out[i];
    return hipSuccess;
}
