/*
 * libcover_hip — C ABI of the MI355X (gfx950) kernels behind CoVer's candidate-sampling-and-verification
 * hot path.
 *
 * The reference (cover-vla/cover-vla) has NO FFI / plugin interface: its boundary is two Python classes
 * (PI0Policy.select_action, lerobot_custom/lerobot/common/policies/pi0/modeling_pi0.py:263-307, and
 * EfficientEnsembleMerged.compute_max_similarity_scores_batch,
 * bridge_verifier/ensemble_eval/efficient_ensemble_merged.py:309-454) whose arithmetic is eager PyTorch.
 * This header is therefore the set of entry points a ctypes binding UNDER those two classes needs
 * (INTEGRATION.md shows the binding); every entry cites the reference arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a raw DEVICE pointer unless the name ends in _host; the caller owns all buffers
 *   - bf16 tensors are uint16 storage ("bf16" in comments); fp32 tensors are float
 *   - leading dimensions / strides are in ELEMENTS
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); none synchronises or allocates
 *   - return value: 0 = ok, negative = cover_status; cover_last_error() gives the message (thread-local)
 *   - not thread-safe per stream; one process per GPU
 */
#ifndef COVER_HIP_H
#define COVER_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COVER_ABI_VERSION 1

enum cover_status { COVER_OK = 0, COVER_EINVAL = -1, COVER_EHIP = -2, COVER_EWORKSPACE = -3, COVER_EUNSUPPORTED = -4 };
enum cover_act { COVER_ACT_NONE = 0, COVER_ACT_GELU_TANH = 1, COVER_ACT_GELU_ERF = 2, COVER_ACT_SILU = 3, COVER_ACT_RELU = 4 };

int cover_abi_version(void);
const char* cover_last_error(void);
/* number of devices visible / properties of device `dev` (CU count, total memory): plumbing for bench + tests */
int cover_device_info(int dev, int* n_cu, size_t* total_mem, char* name, int name_len);

/* ------------------------------------------------------------------------------------------------
 * bf16 GEMM on MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate.
 * Replaces every nn.Linear on the path: q/k/v/o projections and gated MLPs
 * (paligemma_with_expert.py:273-276,327-341), SigLIP/DINOv2/SigLIP2 ViT linears (un-vendored HF/timm
 * modules called at paligemma_with_expert.py:229-230 and finetune_trajectory_bridge_ddp.py:314-316),
 * multimodal projector, lm_head.
 *
 * Weights are packed once (cover_pack_weight_bf16) into the MFMA fragment-major layout
 *   Wp[n/16][k/32][lane = (n%16) + 16*((k%32)/8)][8]        (1 KiB per 16x32 block, K padded to Kpad)
 * so that both the LDS-tiled kernel and the weight-streaming (M <= 64) kernel read 1 KiB fully
 * coalesced per wave instruction.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cover_gemm_epi {
    const float* bias;        /* [N] fp32 or NULL */
    const void* residual;     /* bf16 [M, ld_residual] or NULL: out = residual + (layer_scale *) val */
    const float* layer_scale; /* [N] fp32 or NULL (DINOv2 LayerScale) */
    int ld_residual;
    int residual_f32;         /* 1: residual is fp32 [M, ld_residual] (pi0 expert layer 0: the un-rounded suffix
                                 embedding is the residual, paligemma_with_expert.py:319-332) */
    int act;                  /* cover_act, applied after bias */
    int glu;                  /* 1: weight rows interleaved gate/up in 16-row blocks (pack with glu_interleave=1):
                                 out[m, j] = act(gate[m, j]) * up[m, j], output has N/2 columns */
    int out_f32;              /* 0: bf16 output, 1: fp32 output */
    float out_scale;          /* final multiply (1.0f = none) */
    /* Optional fused RMSNorm / LayerNorm of the (bf16) output rows into a second tensor: norm_out = norm(C) exactly as
     * cover_rmsnorm_bf16 / cover_layernorm_bf16 compute it from the stored bf16 C. Whenever the GEMM runs split-K it is
     * folded into the reduction (one launch less per GEMM); otherwise the library runs the norm kernel after the GEMM. */
    const float* norm_w;      /* [N] or NULL = no fused norm */
    void* norm_out;           /* bf16 [M, ld_norm_out] */
    int ld_norm_out;
    int norm_style;           /* cover_rmsnorm_bf16 style (0 Gemma, 1 Llama), or 2 = LayerNorm as cover_layernorm_bf16 computes it */
    float norm_w_offset;
    float norm_eps;
    const float* norm_b;      /* [N] LayerNorm bias (norm_style 2) or NULL */
    /* Optional e4m3 twin of the SAME (quantised) weight, cover_pack_weight_fp8, with its packed-order per-channel scales: the
     * weight-streaming kernels (M <= 32, HBM-bound) read it instead of the bf16 image -- half the bytes, bit-identical results
     * (power-of-two scales). NULL = bf16 only. */
    const void* w8;
    const float* w8_scale;
    /* Optional e4m3 twin of the ACTIVATION rows (cover_quantize_act_fp8: per-row power-of-two scales, k order of the MFMA operand)
     * with its row scales. When BOTH twins are given and the problem runs on the LDS-tiled kernels (M > 64), the GEMM runs on the
     * MX-scaled fp8 matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 (2x the bf16 rate): C = epi(a8_scale[m] * w8_scale[n] *
     * sum_k a8[m,k] * w8[n,k]); A / Wp are then not read. NULL = bf16 activations. */
    const void* a8;
    const float* a8_scale;
    int ld_a8;               /* row pitch of a8 in BYTES (>= cover_packed_k(K), multiple of 16) */
    int ld_norm_out8;        /* row pitch of norm_out8 in BYTES */
    /* Optional e4m3 twin of norm_out (RMSNorm styles only): norm_out8 / norm_out8_scale receive exactly what cover_quantize_act_fp8
     * would make of the stored bf16 norm_out rows -- the next GEMM's fp8 operand without another launch. */
    void* norm_out8;
    float* norm_out8_scale;
    /* MX block-scaled activations (config 5, the GLU output that feeds down_proj; no reference arithmetic -- SURVEY.md 7 step 9).
     * w8_klinear = 1: w8 is the k-linear image of cover_pack_weight_fp8_klinear, read by every kernel that takes w8.
     * a8_mx: e8m0 block scales of a8 as cover_quantize_act_fp8_mx lays them out ([cover_packed_k(K) / 128][M][4] bytes, byte = 127 + log2 of the
     *   power-of-two scale of 32 consecutive k of a row); a8 is then plain row-major e4m3 (pitch ld_a8), a8_scale is not read, and w8 must be the
     *   k-linear image. C = epi(w8_scale[n] * sum_blocks 2^(mx - 127) * sum_k a8 * w8) on v_mfma_scale_f32_16x16x128_f8f6f4's own block scales.
     * out8 / out8_mx / ld_out8 (glu = 1, act SiLU / tanh-GELU, N / 2 a multiple of 32, M > 64 on the fp8 tiles): the GEMM writes its output rows
     *   in exactly that form -- what cover_quantize_act_fp8_mx makes of the bf16 rows it would have stored -- INSTEAD of C. Only the N / 2 real
     *   columns and their scale bytes are written: when N / 2 is not a multiple of 128, zero the pad columns of out8 and set the pad scale bytes to 127
     *   once (the consuming GEMM reads whole 128-deep k-tiles; an E8M0 byte 255 is a NaN). */
    const void* a8_mx;
    void* out8;
    void* out8_mx;
    int ld_out8;
    int w8_klinear;
} cover_gemm_epi;

/* bytes needed for the packed form of an [N, K] weight (K padded to a multiple of 128, N to 16) */
size_t cover_packed_weight_bytes(int N, int K);
int cover_packed_k(int K);
/* W: bf16 [N, ldw] row-major (PyTorch nn.Linear layout) -> Wp. glu_interleave=1 expects W = [gate(N/2 rows); up(N/2 rows)]
 * and emits 16-row blocks gate0,up0,gate1,up1,... */
int cover_pack_weight_bf16(const void* W, int ldw, int N, int K, void* Wp, int glu_interleave, void* stream);

/* e4m3 weights (BASELINE.json config 5; the reference has no fp8 path -- SURVEY.md 7 step 9). Per-output-channel
 * POWER-OF-TWO scales: s_n = smallest 2^e with max_k |W[n,k]| / s_n <= 448, q = RNE_e4m3(W / s_n).
 * cover_quantize_rows_fp8: W bf16 [N, ldw] -> scales[N] fp32 and Wdq bf16 [N, ldw] = s_n * q (exactly representable: pack it with
 *   cover_pack_weight_bf16 for the MFMA-bound kernels).
 * cover_pack_weight_fp8: Wdq + scales -> the e4m3 image (cover_packed_weight_fp8_bytes) for the HBM-bound weight-streaming
 *   kernels and the scales in packed channel order [ceil(N/16)*16] (glu_interleave as cover_pack_weight_bf16). */
size_t cover_packed_weight_fp8_bytes(int N, int K);
int cover_quantize_rows_fp8(const void* W, int ldw, int N, int K, float* scales, void* Wdq, void* stream);
int cover_pack_weight_fp8(const void* Wdq, int ldw, const float* scales, int N, int K, void* Wq, float* scales_packed,
                          int glu_interleave, void* stream);

/* Dynamic per-row e4m3 quantisation of bf16 activation rows for the fp8 tiled GEMM (config 5; no reference arithmetic -- SURVEY.md 7
 * step 9): scales[m] = smallest 2^e with max_k |X[m,k]| / 2^e <= 448, out8[m] = RNE_e4m3(X[m] / scales[m]) in the k order of the
 * MX MFMA operand (inside every 64-wide block, byte 16 g + 8 h + e holds k = 32 h + 8 g + e), zero padded to cover_packed_k(K).
 * ld8 in BYTES. */
int cover_quantize_act_fp8(const void* X, int ldx, int M, int K, void* out8, int ld8, float* scales, void* stream);
/* The MX form of the same (config 5's down_proj input): out8[m] = RNE_e4m3(X[m] / s) in PLAIN row-major order (zero padded to cover_packed_k(K),
 * ld8 in BYTES), one power-of-two scale per 32 consecutive k of a row -- s = smallest 2^e (e >= -126) with amax_block / 2^e <= 448, 2^0 for an
 * all-zero block -- stored as e8m0 bytes (127 + e) in mx[cover_packed_k(K) / 128][M][4] (k-tile major: what one workgroup of the consuming GEMM
 * reads per 128-deep k-tile is one contiguous run of dwords). The weight of the consuming GEMM must be packed with cover_pack_weight_fp8_klinear. */
int cover_quantize_act_fp8_mx(const void* X, int ldx, int M, int K, void* out8, int ld8, void* mx, void* stream);
/* cover_pack_weight_fp8 with the k-linear operand order: block [n/16][k/64] of the image holds, for lane (n % 16, g), the 16 CONSECUTIVE bytes
 * k = 64 (k/64) + 16 g + 0..15 (the default image: two 8-wide runs 32 apart) -- the k order of v_mfma_scale_f32_16x16x128_f8f6f4 itself, in which one
 * MX block scale covers 32 neighbouring k. No glu interleave (down / o projections). */
int cover_pack_weight_fp8_klinear(const void* Wdq, int ldw, const float* scales, int N, int K, void* Wq, float* scales_packed, void* stream);

/* variant: 0 = auto, 1 = LDS-tiled with async global->LDS (global_load_lds), 2 = LDS-tiled register-staged,
 *          3 = weight-streaming (requires M <= 64; the library picks the second-generation split-K kernel or, for
 *              M <= 32 when its plan fills the chip, the third-generation full-K chunk-loop kernel),
 *          5 = first-generation weight streaming (kept for A/B measurements), 6 = third generation forced (tests).
 *          K = TRUE reduction length (A has >= cover_packed_k(K) readable, zero-padded columns when K is not a
 *          multiple of 128).
 * splitk_ws: fp32 scratch (cover_gemm_workspace_bytes) used by the weight-streaming variants and by split-K tiles. */
size_t cover_gemm_workspace_bytes(int M, int N, int K);
int cover_gemm_bf16(const void* A, int lda, const void* Wp, void* C, int ldc, int M, int N, int K,
                    const cover_gemm_epi* epi, void* splitk_ws, size_t splitk_ws_bytes, int variant, void* stream);
/* Which kernel plan every GEMM launch of this process took since the last reset (test / audit hook: a parity test can assert
 * that a shape really ran on the tile it means to cover). counts[i], i = index into the tile table of launch_gemm_bf16 (gemm_plan.hip):
 *   [0..8]  gemm_tiled: 0 128x128, 1 64x128, 2 64x64 (3 stages), 3 128x128 (4 stages), 4 256x128, 5 128x256, 6 128x128 (8 waves), 7 64x128 (3 stages),
 *           8 128x128 (3 stages)        [10] gemm_tiled_pc 64x128, four loader waves, 4 stages (bf16; 9, 11..18 exist as fp8 kernels only and count in [21])
 *   [19] second-generation weight streaming (gemm_skinny2)   [20] third generation (gemm_skinny3)   [21] fp8 MFMA tiles (any)   [22] first generation
 *   self-loading tiles (gemm_v3.hip), 8 waves: [23] 224x192, [24] 224x128, [25] 256x128, [26] 128x256; 4 waves (one per SIMD): [27] 224x96,
 *   k-split wave pairs (gemm_tiled_v3k): [30] 224x96 ([28], [29], [31]: 112x128 / 224x128 on four waves and 224x128 on wave pairs -- built, measured
 *   slower, not instantiated).
 * Copies min(n, 32) counters, returns 32. */
int cover_gemm_plan_counts(long long* counts, int n, int reset);
/* The plan cover_gemm_bf16 would take for these arguments, without launching anything (test / audit hook). Same arguments as cover_gemm_bf16
 * with the stream replaced by plan[6]; pointers are only checked for null and alignment, never dereferenced. Returns COVER_OK or COVER_EINVAL
 * exactly when cover_gemm_bf16 would. plan = {plan-counter slot (the map above; -1: nothing to launch), tile pick (-1: weight streaming),
 * fp8 self-loading form (0/1), K slices, completion (0 none / 1 splitk_reduce / 2 splitk_reduce_norm), separate norm launch (0/1)}. */
int cover_gemm_plan(const void* A, int lda, const void* Wp, void* C, int ldc, int M, int N, int K,
                    const cover_gemm_epi* epi, void* splitk_ws, size_t splitk_ws_bytes, int variant, int plan[6]);
/* In-kernel probe of the most recent launch of the self-loading tiled GEMM (gemm_v3.hip; plan counters 23..30), written by one thread of
 * its first workgroup: out[0..3] = 100 MHz wall-clock stamps at kernel start / k-loop start / k-loop end / kernel end, out[4..5] = shader
 * cycle counter at k-loop start / end, out[6] = k-tiles of the loop. (out[5] - out[4]) / (out[2] - out[1]) / 10 ns = the clock the loop ran
 * at; out[12..14] = stamps inside the LDS-staged epilogue (pipeline stages released / LDS tile filled / tile published, the store loop runs
 * from out[14] to out[3]). Synchronous read of 16 device words (synchronise the stream first). Measurement hook: nothing on the product
 * path reads it. */
int cover_gemm_probe(unsigned long long* out);

/* ------------------------------------------------------------------------------------------------
 * Flash-style attention on MFMA, fp32 softmax, over up to 3 KV segments per query row.
 * Replaces eager_attention_forward (paligemma_with_expert.py:376-434: fp32 QK^T, scale after the matmul,
 * masked positions get zero probability, probabilities rounded to bf16 before PV) and the HF/timm ViT
 * attention inside the towers. Masks are generated from lengths, never materialised
 * (make_att_2d_masks, modeling_pi0.py:98-128).
 * K is read row-major [slot][t][h][d]; V is read TRANSPOSED [slot][h][d][t] (written by cover_rope_kv_write),
 * so both MFMA operands are 16-byte contiguous per lane with no LDS transpose.
 *
 * Alignment (checked; COVER_EINVAL and nothing runs otherwise): q, every segment's k and vt are loaded 16 bytes at a time -- bases on 16 bytes,
 * every q / k / vt stride a multiple of 8 elements; `out` is stored 8 bytes at a time -- base on 8 bytes (NULL passes), every o_*_stride a
 * multiple of 4 (elements, or bytes with out8); the state's o tensors move as float4 -- state_in_o / state_out_o on 16 bytes, the (m, l)
 * pairs state_in_ml / state_out_ml on 8.
 * V^T capacity: the cache is read in whole 32-key tiles, so every [d] row of vt must have readable elements up to the next multiple of 32 past the
 * segment's (largest) length: vt_d_stride >= ceil(len / 32) * 32 for a dense cache. K rows at or past the length are never read (the load
 * index is clamped to len - 1), K rows between a causal / vis_len bound and the length are.
 * Tail values: a masked key's probability is exactly 0 and is MULTIPLIED with the V^T element, so any FINITE value in the V^T tail (stale
 * keys, +-3e38) leaves the output bits unchanged; a NaN or an infinity there turns the whole output row into NaN (0 * inf). Nothing clears
 * or tests for it: keep the tail of a V^T cache finite (cover_rope_kv_write only ever writes finite values into a zero-initialised cache).
 * Masked K rows inside the length may hold anything finite as well: their scores are replaced by -inf before the softmax.
 * ------------------------------------------------------------------------------------------------ */
enum cover_mask_mode { COVER_MASK_LEN = 0, COVER_MASK_CAUSAL = 1, COVER_MASK_VISLEN = 2 };
typedef struct cover_kv_segment {
    const void* k;  /* bf16 */
    const void* vt; /* bf16, t contiguous */
    long long k_slot_stride, k_t_stride, k_h_stride;
    long long vt_slot_stride, vt_h_stride, vt_d_stride;
    const int* slot_of_batch; /* [B] or NULL (slot = b) */
    const int* len_of_batch;  /* [B] or NULL (use len) */
    const int* vis_len;       /* [Tq] for COVER_MASK_VISLEN: keys [0, vis_len[t]) visible to query token t */
    int len;
    int mask_mode;
    int causal_offset;        /* COVER_MASK_CAUSAL: key j visible iff j <= t + causal_offset */
    int _pad;
} cover_kv_segment;

typedef struct cover_attn_args {
    const void* q; /* bf16 [B][Tq][Hq][D] via strides */
    void* out;     /* bf16 [B][Tq][Hq][D] via strides */
    long long q_b_stride, q_t_stride, q_h_stride;
    long long o_b_stride, o_t_stride, o_h_stride;
    int B, Tq, Hq, Hkv, D;
    float scale;
    int n_seg;
    int _pad;
    cover_kv_segment seg[3];
    /* Optional chaining of calls over different KV segments (flash-decoding style): state = per (b, t, h) the
     * normalised output so far (fp32 [B][Tq][Hq][D]) and its softmax statistics (fp32 [B][Tq][Hq][2] = running max in
     * scaled-log2 units, running sum). state_in seeds the online softmax; state_out receives the result INSTEAD of `out`
     * (which may then be NULL). Used by the decoder to attend a KV segment shared by every candidate once per 16
     * candidates instead of once per candidate. */
    const float* state_in_o; const float* state_in_ml;
    float* state_out_o; float* state_out_ml;
    /* Optional MX block-scaled output INSTEAD of `out` (config 5: the o_proj operand without a quantiser launch; no reference arithmetic):
     * out8 = e4m3 rows addressed with the o_*_stride values in BYTES, out8_mx = E8M0 scales [Hq * D / 128][out8_rows][4] as cover_quantize_act_fp8_mx
     * lays them out (row = byte offset of (b, t) / o_t_stride), exactly what that function makes of the bf16 rows `out` would have received.
     * MHA, D = 128, o_h_stride = 128, o_t_stride = Hq * 128, o_b_stride a multiple of o_t_stride, no state_out, B and Tq not 0, and either at most
     * 1023 query tiles (4095 with state_in) or a problem that takes the shared-keys form (cover_attention_plan form 3: any number of tiles):
     * otherwise COVER_EINVAL. */
    void* out8; void* out8_mx;
    int out8_rows; int _pad2;
} cover_attn_args;
int cover_attention_bf16(const cover_attn_args* args, void* stream);
/* The launch form cover_attention_bf16 would take for these arguments, without launching anything (test / audit hook; pointers are only checked
 * for null and alignment, never dereferenced). Returns COVER_OK or COVER_EINVAL exactly when cover_attention_bf16 would.
 * plan[0] = form: -1 nothing to launch (B or Tq is 0), 0 one wave per 16 query rows walking every key, 1 key tiles split over the 4 waves of a
 *   workgroup (at most 1023 query tiles = ceil(Tq * Hq / Hkv / 16) * Hkv * B; 4095 when resumed from state_in at D <= 128), 2 the same over 8 waves
 *   (experiment knob only), 3 workgroup-shared keys (D = 128, MHA, COVER_MASK_LEN segments only, Tq >= 48, ceil(Tq / 64) * Hq * B >= 128);
 * plan[1] = 1 for block-scaled output (out8); plan[2] = workgroups; plan[3] = waves per workgroup. */
int cover_attention_plan(const cover_attn_args* args, int plan[4]);
/* Two independent problems. ONE launch exactly when: same D in {64, 96, 128}, same Hkv, neither problem empty, each at most 1023 query tiles
 * (state_in does not raise that bound here), neither has out8. Nothing else is looked at: the one launch runs form 1's arithmetic (keys split over 4
 * waves) for both problems, also for a problem that alone would take the shared form (form 3) -- same result up to the order of the fp32 sums.
 * Otherwise two launches, each as cover_attention_bf16 would run it. Both problems are validated before anything runs.
 * cover_attention_pair_plan: *dual = 1 for the one launch, 0 for two; same status as cover_attention_bf16_pair. */
int cover_attention_bf16_pair(const cover_attn_args* a0, const cover_attn_args* a1, void* stream);
int cover_attention_pair_plan(const cover_attn_args* a0, const cover_attn_args* a1, int* dual);

/* Fused single-token decode attention (OpenVLA-style candidate decode): RoPE + KV append + attention over
 * [seg[0]: ONE slot (slot 0) shared by all N candidates | seg[1]: per-prompt slot | seg[2]: the candidate's own tokens,
 * including the one written here at position write_t] in ONE launch. q/k/v come from the bf16 qkv buffer, or (n_splits > 0)
 * straight from the split-K partial sums of the weight-streaming QKV GEMM. Requirements: one new token per candidate,
 * Hq == Hkv == H, D in {64,128}, COVER_MASK_LEN segments. Same results as cover_rope_kv_write + cover_attention_bf16. */
typedef struct cover_decode_attn_args {
    const void* qkv; int ld_qkv;           /* bf16 [N][3*H*D] (used when n_splits == 0) */
    int n_splits;
    const float* partial; const float* bias; /* fp32 [n_splits][N][3*H*D], bias [3*H*D] or NULL */
    int N, H, D;
    float scale;
    const int* positions; const float* cos_table; const float* sin_table; int n_pos; int rope_mode;
    cover_kv_segment seg[3];               /* k/vt pointers are the segment bases */
    int write_t; int _pad;                 /* position of the new token inside seg[2] (slot = seg[2].slot_of_batch[n] or n) */
    void* out; long long out_row_stride;   /* bf16 [N][H*D] */
} cover_decode_attn_args;
int cover_decode_attention_fused(const cover_decode_attn_args* args, void* stream);

/* Candidate decode at large N (BASELINE config 5): RoPE + KV append + attention over every candidate's OWN generated tokens, one wave
 * per (candidate, head) on the VALU (no reuse there: pure HBM streaming), leaving the (o, m, l) softmax state that
 * cover_attention_bf16 resumes (state_in_*) over the shared image prefix and the prompt's text keys. Own-token cache layout:
 * K and V both [slot][h][t][d] (head-major, NOT transposed), bf16 or -- fp8 = 1, the "fp8 KV" of config 5 -- e4m3 with one
 * power-of-two fp32 scale per (slot, h, t) row at k_scale / v_scale[(slot * H + h) * t_cap + t]. q is rotated in place in qkv.
 * Same arithmetic as cover_rope_kv_write + cover_attention_bf16 on the de-quantised values (scores scaled after the product, fp32
 * softmax, probabilities rounded to bf16 before PV). No reference arithmetic for the fp8 cache.
 * Requirements: one new token per candidate, Hq == Hkv == H, D in {64, 128}, write_t < t_cap <= 64 (bf16, D = 128). */
typedef struct cover_own_attn_args {
    void* qkv; int ld_qkv;                  /* bf16 [N][3*H*D] */
    int N, H, D;
    float scale;
    const int* positions; const float* cos_table; const float* sin_table; int n_pos; int rope_mode;
    void* k; void* v;                       /* own-token regions */
    float* k_scale; float* v_scale;         /* fp8 only */
    int fp8; int t_cap;
    long long slot_stride;                  /* ELEMENTS between two slots = H * t_cap * D */
    const int* slot_of_batch;               /* [N] or NULL (slot = n) */
    int write_t; int _pad;                  /* position of the appended token; keys 0..write_t are attended */
    float* state_o; float* state_ml;        /* fp32 [N][H][D] (normalised), [N][H][2] (max in scaled-log2 units, sum) */
} cover_own_attn_args;
int cover_decode_own_attention(const cover_own_attn_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row kernels (HBM-bound, wave-shuffle reductions, 16-byte vector access)
 * ------------------------------------------------------------------------------------------------ */
/* nn.LayerNorm in fp32 math, bf16 in/out (ViT blocks) */
int cover_layernorm_bf16(const void* x, int ldx, const float* w, const float* b, void* y, int ldy, int rows, int dim,
                         float eps, void* stream);
/* RMSNorm: y = x * rsqrt(mean(x^2)+eps) * (w_offset + w); Gemma uses w_offset=1 (HF GemmaRMSNorm, called at
 * paligemma_with_expert.py:268,335,355), Llama w_offset=0. */
/* style 0: y = bf16(x*rstd*(w_offset+w)) (Gemma); style 1: y = bf16(w * bf16(x*rstd)) (HF LlamaRMSNorm).
 * x_f32 = 1: x is fp32 (pi0 suffix embeddings enter the expert's first norm un-rounded). */
int cover_rmsnorm_bf16(const void* x, int x_f32, int ldx, const float* w, float w_offset, int style, void* y, int ldy,
                       int rows, int dim, float eps, void* stream);
/* The same launch with the e4m3 twin of the y rows the decoder's fp8 profile uses: q8 [rows, ld8] holds e4m3(y / q8s[row]) in
 * cover_quantize_act_fp8's byte order (same bytes and scales as that call on y), q8s [rows] the power-of-two row scales.
 * dim % 128 == 0, ld8 >= dim, ld8 % 16 == 0; bytes past dim of a q8 row are not written. */
int cover_rmsnorm_bf16_q8(const void* x, int x_f32, int ldx, const float* w, float w_offset, int style, void* y, int ldy,
                          int rows, int dim, float eps, void* q8, int ld8, float* q8s, void* stream);
/* The norm launches read and write 16 bytes per lane: x, y (and the embedding table / out of cover_embed_gather) must be 16-byte
 * aligned and the row strides multiples of 8 elements (4 for fp32 x); anything else returns COVER_EINVAL and nothing runs. */

/* RoPE + KV placement. Replaces apply_rope (paligemma_with_expert.py:34-57) and the dict/concat KV cache
 * (:288-308) with in-place appends into a static cache. qkv rows = [B*T][ (Hq+2*Hkv)*D ].
 * cos/sin: fp32 [n_pos][D/2] tables built on the host with the reference's own expressions.
 * rope_mode 0: no rotation (ViT: only V^T is produced); 1: fp32 rotate, one rounding (pi0);
 *           2: bf16 cos/sin and bf16 intermediate roundings (HF Llama rotate_half arithmetic). */
typedef struct cover_rope_args {
    void* qkv; int ld_qkv;       /* bf16; q is rotated IN PLACE */
    int B, T, Hq, Hkv, D;
    const int* positions;        /* [B*T] position ids or NULL */
    const float* cos_table; const float* sin_table; int n_pos;
    int rope_mode;
    void* k_cache;               /* bf16 [slot][t][Hkv][D] or NULL (leave K in the qkv buffer, rotated in place) */
    long long k_slot_stride, k_t_stride, k_h_stride;
    void* vt_cache;              /* bf16 [slot][Hkv][D][t_cap] (required) */
    long long vt_slot_stride, vt_h_stride, vt_d_stride;
    const int* slot_of_batch;    /* [B] or NULL */
    const int* t_offset_of_batch;/* [B] or NULL */
    int t_offset;
    int n_splits;                /* > 0: the q/k/v values are NOT read from qkv but formed on the fly as
                                    bf16(sum_s partial[s][row][col] + bias[col]) from the split-K partials of the QKV
                                    GEMM (fuses the reduction into this kernel on the weight-streaming path); q is still
                                    written to qkv (rotated), k/v go to the caches */
    const float* partial;        /* fp32 [n_splits][B*T][ld_qkv-compatible N = (Hq+2Hkv)*D] */
    const float* bias;           /* [N] or NULL */
} cover_rope_args;
int cover_rope_kv_write(const cover_rope_args* args, void* stream);
/* two row groups of one pass in one launch (the decoder's prefill): the same cells as two cover_rope_kv_write calls */
int cover_rope_kv_write_pair(const cover_rope_args* args0, const cover_rope_args* args1, void* stream);

/* token embedding gather (K4: modeling_pi0.py:549-553): out[i] = bf16(table[ids[i]] * scale) */
int cover_embed_gather(const void* table, int dim, const int64_t* ids, int n, float scale, void* out, int ldo,
                       void* stream);

/* image -> patch rows for the patch-embedding GEMM (im2col-free conv, K1): out[p][c*ps*ps+py*ps+px] =
 * bf16(pix*mul[c]+add[c]), zero padded to ld_out columns. in_u8_hwc=1: uint8 [H][W][3]; 0: fp32 [3][H][W] */
typedef struct cover_patchify_args {
    const void* img; int in_u8_hwc; int H, W, patch; int n_img; long long img_stride;
    float mul[3]; float add[3];
    void* out; int ld_out;
} cover_patchify_args;
int cover_patchify(const cover_patchify_args* args, void* stream);

/* row gather/scatter copy: dst[dst_row_idx[i]] = src[src_row_idx[i]] (NULL idx = identity) */
int cover_copy_rows_bf16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, const int* src_row_idx,
                         const int* dst_row_idx, void* stream);
/* x[r] += add[r % add_rows] (position embeddings) with bf16 rounding */
int cover_add_rows_bf16(void* x, int ldx, const void* add, int ld_add, int rows, int cols, int add_rows, void* stream);
/* x = bf16(bf16(x / pre_div) * post_mul): the image-token double rounding of modeling_pi0.py:534-538 (Appendix A.3) */
int cover_scale_bf16(void* x, int ldx, int rows, int cols, float pre_div, float post_mul, void* stream);
int cover_cast_f32_to_bf16(const float* x, int ldx, void* y, int ldy, int rows, int cols, void* stream);
int cover_cast_bf16_to_f32(const void* x, int ldx, float* y, int ldy, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp32 kernels: verifier heads (model.py:7-112, efficient_ensemble_merged.py:194-247) and the pi0 suffix
 * projections (modeling_pi0.py:569-629,748-751), which the reference keeps in fp32.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cover_gemm_f32_args {
    const float* A; long long a_row_stride, a_k_stride;   /* A[m,k] */
    const float* B; long long b_row_stride, b_k_stride;   /* B[n,k]  (nn.Linear weight: row stride K, k stride 1) */
    float* C; long long c_row_stride;                     /* C[m,n] */
    const float* bias;      /* [N] or NULL */
    const float* residual;  /* [M, ld_residual] or NULL: C = residual + val. Row stride ld_residual (need not equal c_row_stride); batch z
                             * reads residual + z * c_batch_stride: the residual shares C's BATCH stride (it may be C itself) */
    long long ld_residual;
    int M, N, K;
    int act;
    float alpha;            /* C = residual + alpha * act(A.B^T + bias) */
    int batch; long long a_batch_stride, b_batch_stride, c_batch_stride;
    long long bias_batch_stride; /* bias of batch z = bias + z * bias_batch_stride (0: one bias for every batch) */
} cover_gemm_f32_args;
int cover_gemm_f32(const cover_gemm_f32_args* args, void* stream);
/* The kernel cover_gemm_f32 would run for these arguments, without launching anything and without a GPU (test / audit hook; pointers
 * are only checked for null and alignment, never dereferenced). plan[0] = COVER_GEMM_F32_* (-1: M or N <= 0, nothing to launch),
 * plan[1] = 1 when the direct kernel takes the eight-step window of the COVER_F32_UNR=8 experiment knob. Reads COVER_F32_DIRECT_MAX per
 * call, as cover_gemm_f32 does. */
enum {
    COVER_GEMM_F32_DIRECT_FM1 = 0,   /* gemm_f32_direct_k<1>: k-contiguous aligned operands, K % 16 == 0, K >= 64, M <= 16 */
    COVER_GEMM_F32_DIRECT_FM2 = 1,   /* gemm_f32_direct_k<2>: the same, M > 16 */
    COVER_GEMM_F32_TILE64 = 2,       /* gemm_f32_k<64,64,32>: any strides, >= 256 blocks of 64x64 */
    COVER_GEMM_F32_TILE32_K128 = 3,  /* gemm_f32_k<32,32,128>: small grid, K >= 256 */
    COVER_GEMM_F32_TILE32_K32 = 4    /* gemm_f32_k<32,32,32> */
};
int cover_gemm_f32_plan(const cover_gemm_f32_args* args, int plan[2]);
int cover_layernorm_f32(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int rows, int dim,
                        float eps, void* stream);
/* the same over stacked row groups with their own affine parameters (ensemble members batched into one launch):
 * row r uses w + (r / rows_per_group) * wb_group_stride (and b likewise) */
int cover_layernorm_f32_grouped(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int rows, int dim,
                                float eps, int rows_per_group, long long wb_group_stride, void* stream);
/* in place: x[r] = softmax(x[r] * scale) */
int cover_softmax_rows_f32(float* x, int ldx, int rows, int cols, float scale, void* stream);
/* y[r] = x[r] / ||x[r]||_2  (finetune_trajectory_bridge_ddp.py:329-330,352-354; efficient_ensemble_merged.py:223,245) */
int cover_l2norm_rows_f32(const float* x, int ldx, float* y, int ldy, int rows, int cols, void* stream);
/* y = a + b[r % b_rows] */
int cover_add_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int rows, int cols, int b_rows,
                  void* stream);
/* small multi-head attention in fp32 (nn.MultiheadAttention core, after the in-projections):
 * q [B][Tq][H*Dh], k/v [B][Tk][H*Dh] via strides, optional key padding mask (1 = ignore key) [B][Tk] */
typedef struct cover_mha_f32_args {
    const float* q; long long q_b_stride, q_t_stride;
    const float* k; long long k_b_stride, k_t_stride;
    const float* v; long long v_b_stride, v_t_stride;
    float* out; long long o_b_stride, o_t_stride;
    const uint8_t* key_pad; /* [B][Tk] or NULL */
    int B, Tq, Tk, H, Dh;
    float scale;
} cover_mha_f32_args;
/* y = act(x) elementwise (COVER_ACT_*): the ReLU between LayerNorm and the second Linear of the verifier's MLP action encoder
 * (`complex_action_encoder`, bridge_verifier/ensemble_eval/efficient_ensemble_merged.py:148-184, 241-243). */
/* Contrastive evaluation statistics: loss[r] = logsumexp(logits[r, :]) - logits[r, r] (F.cross_entropy against labels arange(B),
 * reduction left to the caller) and rank[r] = how many entries of row r rank ahead of its diagonal (top-k hit <=> rank < k).
 * Replaces the per-batch F.cross_entropy + torch.topk of bridge_verifier/ensemble_eval/finetune_trajectory_bridge_ddp.py:446-469,
 * :1081-1090 (validation forward). rows <= cols. */
int cover_xent_diag_f32(const float* logits, int ld, int rows, int cols, float* loss, int* rank, void* stream);
int cover_act_f32(const float* x, int ldx, float* y, int ldy, int rows, int cols, int act, void* stream);
int cover_mha_f32(const cover_mha_f32_args* args, void* stream);
/* masked mean over T (efficient_ensemble_merged.py:236-240): y[b] = sum_t x[b,t]*(1-pad) / max(sum(1-pad), 1e-9) */
int cover_masked_mean_f32(const float* x, const uint8_t* pad, float* y, int B, int T, int D, void* stream);
/* create_sinusoidal_pos_embedding (modeling_pi0.py:71-89) evaluated in float64 on the device, cast to bf16 */
int cover_sincos_time_embed(const float* time, int B, int dim, double min_period, double max_period, void* out, int ldo,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Selection kernels
 * ------------------------------------------------------------------------------------------------ */
/* Action-token decode head (OpenVLA profile; the 256-bin arithmetic the reference carries at
 * INT-ACT/src/experiments/policies/policy_wrapper.py:259-266). logits fp32 [rows][ld]; greedy: first arg-max over
 * [lo, hi); sampling: softmax((logits - max)/temperature) over [lo, hi), inverse CDF in index order with the
 * host-supplied uniform u[row].
 * NaN rule of every arg-max in this library (here, cover_group_argmax and the greedy row of cover_token_sample_rows): a NaN
 * never wins a comparison, and if nothing wins the pick is the first index of the range. Greedy: NaNs among numbers are passed
 * over; a row whose [lo, hi) holds only NaNs gives token_out = lo and logit_out = logits[row][lo] (that NaN's own bits) -- always
 * an id inside [lo, hi). logit_out carries the bits of the picked logit in every case (so -0.0 stays -0.0).
 * Sampling: a row that contains a NaN is unspecified beyond "token_out is in [lo, hi), logit_out is the logit at that token and
 * the other rows of the launch are unaffected".
 * COVER_EINVAL, and nothing launched: hi <= lo; with a uniform, hi - lo > 4096 or a temperature that is not > 0 (a NaN included).
 * rows <= 0 succeeds and writes nothing. */
typedef struct cover_token_select_args {
    const float* logits; long long ld; int rows; int lo, hi;
    const float* uniform;   /* [rows] in [0,1) or NULL for greedy */
    float temperature;
    int64_t* token_out;     /* [rows] */
    float* logit_out;       /* [rows] selected logit (optional, may be NULL) */
} cover_token_select_args;
int cover_token_select(const cover_token_select_args* args, void* stream);

/* Filtered sampling over a wide row (pi0-FAST: the 257 152-entry PaliGemma vocabulary; OpenVLA: the 256 action bins): what
 * Hugging Face's generate(do_sample=True) applies, in its order -- TemperatureLogitsWarper, TopKLogitsWarper,
 * TopPLogitsWarper -- followed by this library's inverse-CDF pick with a host-supplied uniform. Per row, over columns [lo, hi)
 * (hi - lo <= 2^20, any lo / ld):
 *   1. m = max l_i, weight w_i = expf((l_i - m) / temperature)                                     (temperature > 0)
 *   2. top_k > 0: keep the tokens whose logit is >= the k-th largest logit (a comparison of the input floats: every token
 *      tied with the k-th value stays, as in TopKLogitsWarper); top_k == 0 or >= hi - lo keeps all
 *   3. top_p < 1: order the kept tokens by descending weight, equal weights by ascending index, and keep the shortest prefix
 *      whose mass reaches top_p x (mass kept by step 2); at least one token stays (TopPLogitsWarper, min_tokens_to_keep = 1);
 *      top_p >= 1 keeps all                                                                            (top_p > 0)
 *   4. running sum of the kept weights in index order; token = the first kept index whose running sum exceeds
 *      uniform[row] x (kept mass), the last kept index if rounding lets none exceed it.
 * Deterministic: the same row, uniform and parameters give the same token in every launch and at every row position. All masses
 * are exact integer sums of Q43 fixed-point weights (rint(w x 2^43)), so no summation order can change a result; the error
 * against exact sums of the fp32 weights is below 2^-24 of the kept mass (csrc/sample.hip states the scheme in full).
 * One launch, no workspace, no host round trip: recordable into a hipGraph. With both filters off and hi - lo <= 4096 the call
 * is cover_token_select's sampling path, bit for bit. kept_out (optional) receives the size of the kept set. */
typedef struct cover_token_sample_args {
    const float* logits; long long ld; int rows; int lo, hi;
    const float* uniform;   /* [rows] in [0,1), required */
    float temperature;
    int top_k;              /* 0 = off */
    float top_p;            /* >= 1 = off */
    int64_t* token_out;     /* [rows] */
    float* logit_out;       /* [rows] selected raw logit (optional) */
    int* kept_out;          /* [rows] size of the kept set (optional) */
} cover_token_sample_args;
int cover_token_sample(const cover_token_sample_args* args, void* stream);

/* Per-token log-probabilities under the distribution cover_token_sample draws from (what Hugging Face's
 * compute_transition_scores gives on the processed scores: the warpers set filtered logits to -inf before the softmax).
 * Per row, over columns [lo, hi) with the parameters and steps of cover_token_sample:
 *   x_i   = (l_i - m) / temperature,  m = max l_i over [lo, hi)
 *   KEPT  = the set steps 2-3 keep (top-k with ties, then top-p); all of [lo, hi) with both filters off
 *   lp(t) = x_t - log( sum_{i in KEPT} exp(x_i) )     if t is in KEPT
 *         = -inf                                      if t is in [lo, hi) but not in KEPT, or t is outside [lo, hi)
 * The sampler and the scorer share one implementation of KEPT (csrc/sample.hip), so membership means the same in both. The sum is
 * the exact integer Q43 mass of the kept set; x_t is the fp32 exponent of the weights; the logarithm and the difference are
 * taken in double once per row and rounded to fp32 once. No floating-point sum over columns: the value cannot depend on a
 * summation order, a row position or a launch. Error against exact arithmetic on the fp32 logits:
 * 5.1e-6 + 2^-23 |x_t| + 2^-24 |lp| (tests/logprob_ref.py derives it).
 *
 * cover_token_sample_scored: cover_token_sample (the same pick, logit_out and kept_out, bit for bit) plus
 * logprob_out[row] = lp(pick). The same single launch, except with both filters off and hi - lo <= 4096: cover_token_select
 * makes that pick and keeps no mass, so its picks are scored by a second small launch (cover_token_logprob's kernel). */
typedef struct cover_token_sample_scored_args {
    const float* logits; long long ld; int rows; int lo, hi;
    const float* uniform;   /* [rows] in [0,1), required */
    float temperature;
    int top_k;              /* 0 = off */
    float top_p;            /* >= 1 = off */
    int64_t* token_out;     /* [rows] */
    float* logit_out;       /* [rows] selected raw logit (optional) */
    int* kept_out;          /* [rows] size of the kept set (optional) */
    float* logprob_out;     /* [rows] lp(pick), required */
} cover_token_sample_scored_args;
int cover_token_sample_scored(const cover_token_sample_scored_args* args, void* stream);

/* Scores given tokens (teacher-forced sequences, greedy picks): logprob_out[row] = lp(token[row]). No uniform, no pick. A token
 * outside [lo, hi) (a pad id, a negative id) yields -inf and reads nothing. One block per row, one launch, no workspace:
 * recordable into a hipGraph; hi - lo <= 2^20, any lo / ld. On the scored sampler's own picks the result is that call's
 * logprob_out, bit for bit. */
typedef struct cover_token_logprob_args {
    const float* logits; long long ld; int rows; int lo, hi;
    float temperature;
    int top_k;              /* 0 = off */
    float top_p;            /* >= 1 = off */
    const int64_t* token;   /* [rows] */
    float* logprob_out;     /* [rows] */
    int* kept_out;          /* [rows] size of the kept set (optional) */
} cover_token_logprob_args;
int cover_token_logprob(const cover_token_logprob_args* args, void* stream);

/* The n most probable tokens of each row under the distribution cover_token_sample draws from, with their log-probabilities, and the
 * entropy of that distribution (a sampler's top_logprobs). Per row, over columns [lo, hi) with KEPT, x_i and lp() of
 * cover_token_logprob for the same (temperature, top_k, top_p):
 *   ranking       the columns of KEPT by descending input logit (a comparison of the input floats, -0 == +0, no arithmetic), equal
 *                 logits by ascending index;
 *   token_out[row, j]   = the absolute column id of rank j            for j < min(n, |KEPT|),   -1   for the remaining slots
 *   logprob_out[row, j] = lp(token_out[row, j]), bit for bit the value cover_token_logprob returns for that token with the same
 *                         parameters (the same code on the same integer mass),                  -inf for the remaining slots
 *   entropy_out[row]    = H = -sum_{i in KEPT} p_i log p_i in nats, p_i = exp(lp(i))            (optional)
 *   kept_out[row]       = |KEPT|, cover_token_logprob's                                          (optional)
 * H has no floating-point sum over columns: with w_i = expf(x_i), M = sum rint(w_i 2^43) (the kept mass) and
 * S = sum rint(w_i (-x_i) 2^43) (the fp32 product converted once), both exact integer sums,
 * H = fp32( log(M / 2^43) + S / M ) in double, once per row. Error against exact arithmetic on the fp32 logits:
 * 5.2e-6 + (1.05e-5 + 2^-24) H (tests/topn_ref.py derives it). 0 <= H <= log |KEPT| up to that error.
 * One 1024-thread block per row, one launch, no workspace, nothing data-dependent in the launch: recordable into a hipGraph and
 * deterministic (the same row and parameters give the same outputs at every row position, base alignment and launch).
 * 1 <= n <= 64; hi - lo <= 2^20, any lo / ld; token_out / logprob_out are [rows, n] with unit column stride and row strides
 * ld_tok / ld_lp >= n (elements), e.g. a step's slab of a [steps, rows, n] buffer. */
typedef struct cover_token_topn_args {
    const float* logits; long long ld; int rows; int lo, hi;
    float temperature;
    int top_k;              /* 0 = off */
    float top_p;            /* >= 1 = off */
    int n;                  /* alternatives per row, 1..64 */
    int64_t* token_out; long long ld_tok;     /* [rows, n] */
    float* logprob_out; long long ld_lp;      /* [rows, n] */
    float* entropy_out;     /* [rows] (optional) */
    int* kept_out;          /* [rows] size of the kept set (optional) */
} cover_token_topn_args;
int cover_token_topn(const cover_token_topn_args* args, void* stream);

/* Sampling parameters per row: cover_token_sample_scored, cover_token_logprob and cover_token_topn with temperature / top_k / top_p
 * read from device arrays [rows], so one launch serves a ladder of proposal distributions (one greedy candidate per prompt, the other
 * samples at rising temperatures or looser filters) and a captured graph does not depend on the values. One 1024-thread block per row,
 * one launch, no workspace, no host round trip, nothing data-dependent in the launch: recordable. hi - lo <= 2^20, any lo / ld.
 * What a row computes depends on that row's logits, uniform and parameters alone -- never on the other rows of the launch, the row's
 * position or the width of the range (there is no cover_token_select detour for narrow unfiltered rows):
 *   temperature[r] > 0    a sampled row: steps 1-4 of cover_token_sample with (temperature[r], top_k[r], top_p[r]) on the Q43 integer
 *                         masses. token_out / logit_out / kept_out / logprob_out are what cover_token_sample_scored writes for that row
 *                         wherever that call runs its own kernel (a filtered row, or hi - lo > 4096), bit for bit; logprob_out is
 *                         cover_token_logprob of the pick with the row's parameters, bit for bit, always.
 *   temperature[r] == 0   a greedy row: token_out = the first arg-max of the input floats over [lo, hi) (cover_token_select's greedy rule:
 *                         the lowest index among equal maxima, lo and its NaN for a row of NaNs), logit_out its logit, kept_out = hi - lo, logprob_out = lp(token) at
 *                         temperature 1 with both filters off (cover_token_logprob's value, bit for bit). top_k[r], top_p[r] and
 *                         uniform[r] are not read. cover_token_logprob_rows / cover_token_topn_rows score and rank a greedy row at
 *                         temperature 1, unfiltered.
 *   invalid               temperature[r] < 0 or NaN, top_p[r] <= 0 or NaN, top_k[r] < 0 (the arrays live on the device: the host cannot
 *                         validate them). The row reads no logits and writes token_out = -1, logit_out = logprob_out = NaN, kept_out = 0
 *                         (topn: every slot -1 / -inf, entropy_out = NaN, kept_out = 0). No trap; the other rows are unaffected.
 *                         The id -1 is the caller's to handle before an embedding lookup: cover_decode_feedback turns it into a zero
 *                         row, cover_embed_gather checks no id.
 * Null required pointers and a bad lo / hi / rows / n / stride return COVER_EINVAL, as in the scalar calls. */
typedef struct cover_token_sample_rows_args {
    const float* logits; long long ld; int rows; int lo, hi;
    const float* uniform;       /* [rows] in [0,1), required; a greedy row ignores its entry */
    const float* temperature;   /* [rows], required; 0.0f marks a greedy row */
    const int* top_k;           /* [rows] or NULL = 0 for every row */
    const float* top_p;         /* [rows] or NULL = 1 for every row */
    int64_t* token_out;         /* [rows] */
    float* logit_out;           /* [rows] selected raw logit (optional) */
    int* kept_out;              /* [rows] size of the kept set (optional) */
    float* logprob_out;         /* [rows] lp(pick) (optional) */
} cover_token_sample_rows_args;
int cover_token_sample_rows(const cover_token_sample_rows_args* args, void* stream);

typedef struct cover_token_logprob_rows_args {
    const float* logits; long long ld; int rows; int lo, hi;
    const float* temperature;   /* [rows], required; 0.0f: scored at temperature 1, unfiltered */
    const int* top_k;           /* [rows] or NULL = 0 for every row */
    const float* top_p;         /* [rows] or NULL = 1 for every row */
    const int64_t* token;       /* [rows] */
    float* logprob_out;         /* [rows] */
    int* kept_out;              /* [rows] size of the kept set (optional) */
} cover_token_logprob_rows_args;
int cover_token_logprob_rows(const cover_token_logprob_rows_args* args, void* stream);

typedef struct cover_token_topn_rows_args {
    const float* logits; long long ld; int rows; int lo, hi;
    const float* temperature;   /* [rows], required; 0.0f: ranked at temperature 1, unfiltered */
    const int* top_k;           /* [rows] or NULL = 0 for every row */
    const float* top_p;         /* [rows] or NULL = 1 for every row */
    int n;                      /* alternatives per row, 1..64 */
    int64_t* token_out; long long ld_tok;     /* [rows, n] */
    float* logprob_out; long long ld_lp;      /* [rows, n] */
    float* entropy_out;         /* [rows] (optional) */
    int* kept_out;              /* [rows] size of the kept set (optional) */
} cover_token_topn_rows_args;
int cover_token_topn_rows(const cover_token_topn_rows_args* args, void* stream);

/* Allowed-token sets per row: cover_token_sample_rows, cover_token_logprob_rows and cover_token_topn_rows restricted to the columns a
 * row may draw (Hugging Face's prefix_allowed_tokens_fn / suppress_tokens / bad_words_ids for single ids), inside the kernels: no
 * masked copy of the [rows, vocabulary] slab is written or read. The argument structs are the unmasked calls', unchanged.
 * An allow set is a bitmask over ABSOLUTE column ids: bit (c & 31) of word (c >> 5) is 1 when column c may be drawn. A launch carries
 * n_sets sets, ld_words words apart, and set_of_row[rows] (NULL: every row uses set 0). For a row with set A each call computes what
 * the unmasked _rows call computes on the row restricted to the columns of [lo, hi) that are in A, column ids unchanged:
 *   disallowed columns    never reach the arithmetic: they may hold NaN, +-inf or 3e38 without changing one output bit.
 *   sampled row           maximum, top-k (ties with the k-th value stay), top-p cut and the inverse-CDF pick run over the allowed columns
 *                         only, on the same Q43 integer masses. kept_out counts allowed columns only, so top_k >= |A n [lo, hi)| keeps
 *                         every allowed column. logprob_out = lp(pick) under that restricted distribution. If no allowed column has
 *                         mass (all NaN or -inf), the pick is the first allowed column.
 *   greedy row            the first arg-max among the allowed columns, scored at temperature 1, unfiltered, over the allowed columns;
 *                         kept_out = |A n [lo, hi)|.
 *   scorer                a token outside [lo, hi) or not in A gets -inf and nothing is read for it.
 *   top-n                 only allowed columns are ranked; slots beyond min(n, kept) are -1 / -inf; the entropy is that of the
 *                         restricted kept set.
 *   invalid               additionally to the unmasked calls' conditions: set_of_row[r] outside [0, n_sets), or a set without a column
 *                         in [lo, hi) (both live on the device). Reported as an invalid row is there: token -1, logit_out = logprob_out =
 *                         NaN, kept_out = 0 (topn: every slot -1 / -inf, entropy NaN, kept 0). No trap; the other rows are unaffected.
 * What a row computes depends on its logits, uniform, parameters and the CONTENTS of its set alone -- never on the set's index, the
 * other rows or the row's position. Token, selected logit and log-probability equal the unmasked call's on a copy of the row with -inf
 * in the disallowed columns, bit for bit; an all-ones set gives the unmasked call's outputs, bit for bit.
 * One 1024-thread block per row, one launch, no workspace, recordable: a replay follows the current contents of bits and set_of_row.
 * COVER_EINVAL, and nothing launched: everything the unmasked call refuses; a null allow or null bits; n_sets < 1; ld_words <
 * ceil(hi / 32); bits not 4-byte aligned. */
typedef struct cover_token_allow {
    const uint32_t* bits;   /* [n_sets][ld_words], 4-byte aligned */
    long long ld_words;     /* words between two sets, >= ceil(hi / 32) */
    int n_sets;             /* >= 1 */
    int _pad;
    const int* set_of_row;  /* [rows] or NULL = set 0 for every row */
} cover_token_allow;
int cover_token_sample_rows_allowed(const cover_token_sample_rows_args* args, const cover_token_allow* allow, void* stream);
int cover_token_logprob_rows_allowed(const cover_token_logprob_rows_args* args, const cover_token_allow* allow, void* stream);
int cover_token_topn_rows_allowed(const cover_token_topn_rows_args* args, const cover_token_allow* allow, void* stream);

/* A common yardstick for a ladder of proposal distributions: cover_token_sample_rows (allow == NULL) or cover_token_sample_rows_allowed
 * with one more output per row, the log-probability of the SAME pick under one reference distribution shared by every row of the
 * launch: temperature ref->temperature, both filters off, over the same range [lo, hi) and the same allowed-token set. For a valid
 * row with pick t, logit l_t and row maximum m (over the allowed columns):
 *     ref->logprob_out[r] = x_ref(t) - log(M_ref),   x_ref = (l_t - m) / T_ref,   M_ref = sum of q43(w(l, m, T_ref)) over every (allowed)
 *     column of [lo, hi), an exact uint64 sum of the Q43 weights like every other mass of these calls; logarithm and difference in double,
 *     one rounding to fp32.
 * That is cover_token_logprob_rows (cover_token_logprob_rows_allowed) of the pick at (T_ref, top_k 0, top_p 1), bit for bit: the sums are
 * integers, so the summation order cannot matter. The per-step log-probabilities of a ladder (logprob_out) are each taken under
 * their own row's distribution and do not compare across rungs; this column does, and is what cover_prior_select should be fed
 * under a ladder. The reference is unfiltered on purpose: a filtered one would score the picks of looser rungs -inf.
 * Every other output (token_out, logit_out, kept_out, logprob_out) is the underlying call's, bit for bit. A row whose own distribution
 * already is the reference (unfiltered with temperature[r] == T_ref; a greedy row when T_ref == 1) reuses its mass, every other row makes
 * one more pass over its columns. An invalid row (bad parameters, bad set index, empty set) writes NaN; a row without mass writes what
 * cover_token_logprob_rows(_allowed) writes for that pick. One launch, no workspace, recordable; T_ref travels by value, so a
 * captured launch keeps the one it was recorded with.
 * COVER_EINVAL, and nothing launched: everything the underlying call refuses; a null ref or ref->logprob_out; ref->temperature <= 0,
 * NaN or infinite. */
typedef struct cover_token_ref {
    float temperature;    /* > 0, finite: the reference temperature */
    int _pad;
    float* logprob_out;   /* [rows], required */
} cover_token_ref;
int cover_token_sample_rows_ref(const cover_token_sample_rows_args* args, const cover_token_allow* allow /* NULL: unmasked */,
                                const cover_token_ref* ref, void* stream);

/* The bookkeeping between two steps of an autoregressive decode loop (pi0-FAST generate_tokens), one launch, one block per
 * candidate row, no workspace: recordable into a hipGraph. Per row b, in this order:
 *   t = force ? force[b * force_stride] : pick[b];  lp_out[b * ld_lp] = done[b] ? 0.0f : lp[b];  if (done[b]) t = pad;
 *   tok_out[b * ld_tok] = t;  done[b] |= (t == eos);  x_out[b][:] = bf16(table[t][:] * scale);  *live += !done[b];
 * tok_out / lp_out point at this step's column of row-major [rows, ld] buffers. x_out is cover_embed_gather's arithmetic on the
 * emitted ids, except that an id outside [0, vocab) yields a zero row and reads nothing. live (optional) is this step's counter of
 * rows still running, zeroed by the caller: reading it back replaces a reduction over done. */
typedef struct cover_decode_feedback_args {
    const int64_t* pick;      /* [rows] this step's selection */
    const int64_t* force;     /* [rows] with element stride force_stride: teacher-forced tokens (optional) */
    long long force_stride;
    const float* lp;          /* [rows] log-probability of pick (optional, together with lp_out) */
    float* lp_out; long long ld_lp;
    uint8_t* done;            /* [rows] bytes 0 / 1, updated in place */
    int64_t* tok_out; long long ld_tok;
    long long eos, pad;
    const void* table;        /* bf16 [vocab][dim], 16-byte aligned (required with x_out) */
    int vocab, dim; float scale;
    void* x_out; int ldo;     /* bf16 [rows][ldo] next step's input rows; NULL: none (the last step) */
    int* live;                /* optional */
    int rows;
} cover_decode_feedback_args;
int cover_decode_feedback(const cover_decode_feedback_args* args, void* stream);
/* cover_decode_feedback with a second log-probability column (the reference score of cover_token_sample_rows_ref): the same kernel,
 * and additionally lp2_out[b * ld_lp2] = done[b] ? 0.0f : lp2[b], with done as it was before this step's update, exactly as lp_out.
 * lp2 [rows] and lp2_out are required; every other rule is cover_decode_feedback's. */
int cover_decode_feedback_lp2(const cover_decode_feedback_args* args, const float* lp2, float* lp2_out, long long ld_lp2, void* stream);
/* Token grammars on the device: cover_decode_feedback that also advances one finite automaton per row on the emitted token and writes the
 * index of the allowed-token set the row's NEXT pick draws from, so a cover_token_*_rows_allowed launch whose allow->set_of_row is
 * fsm->set_of_row follows a per-step grammar with no host round trip ("at least m action tokens, then the terminator, then EOS only").
 * The automaton is regular and per row: states, token classes, one transition table; no stack, nothing across rows.
 * Per row b, with t the token cover_decode_feedback emits (forced token and pad after EOS included) and done[b] as it was before the step:
 *   if (!done[b] && 0 <= t < args->vocab)  state[b] = trans[state[b] * n_classes + class_of_token[t]];
 *   otherwise the state is unchanged: a finished row stops moving, an id outside the vocabulary (the -1 of an invalid row) reads nothing
 *   from class_of_token; a class id >= n_classes (outside the contract) leaves the state unchanged too;
 *   set_of_row[b] = set_of_state[state[b]], always.
 * A state[b] outside [0, n_states) lives on the device and cannot be refused on the host: it is left unchanged, no table is read for it and
 * set_of_row[b] = -1, which the _allowed kernels report as an invalid row. No trap; the other rows are unaffected.
 * args->vocab is the length of class_of_token and is required here with or without x_out. Every other output (tok_out, lp_out, done,
 * x_out, live) is cover_decode_feedback's, bit for bit; with lp2 / lp2_out (optional, together) the second column is
 * cover_decode_feedback_lp2's. One launch, one block per row, no workspace, recordable: a replay follows the current contents of the tables.
 * COVER_EINVAL, and nothing launched: everything cover_decode_feedback refuses; a null fsm or any null member; n_states < 1; n_classes < 1
 * or > 256; vocab < 1; lp2 without lp2_out or the reverse. */
typedef struct cover_token_fsm {
    const uint8_t* class_of_token;  /* [vocab] class id of every token, < n_classes */
    const int*     trans;           /* [n_states][n_classes] next state, each in [0, n_states) */
    const int*     set_of_state;    /* [n_states] allowed-set index that a row in this state draws from */
    int n_states, n_classes;
    int* state;                     /* [rows] in/out: current state of each row */
    int* set_of_row;                /* [rows] out: set_of_state[state[b]] after the update;
                                       the array the next cover_token_*_rows_allowed launch reads */
} cover_token_fsm;
int cover_decode_feedback_fsm(const cover_decode_feedback_args* args, const cover_token_fsm* fsm,
                              const float* lp2 /* optional */, float* lp2_out, long long ld_lp2, void* stream);

/* K20: fuse + score + grouped arg-max (efficient_ensemble_merged.py:404-448). it: [n_members][512] image-text
 * embeddings (unit rows), act: [n_members][N][512]; scores_out [N]; result_out int32 [4] =
 * {global_idx, group_idx, idx_in_group, 0}; best_out float [2] = {max_score, best_group_mean}. First index wins ties
 * (torch.max semantics). */
typedef struct cover_score_select_args {
    const float* it; const float* act;
    int n_members, N, dim, group_size;
    float* scores_out; int* result_out; float* best_out;
    float* fused_it_out;   /* [dim] optional */
    float* fused_act_out;  /* [N][dim] optional */
} cover_score_select_args;
int cover_score_select(const cover_score_select_args* args, void* stream);
/* De-tokenise action tokens and assemble the verifier's candidate histories on the device (no host round trip between
 * sampler and verifier). For candidate n: hist[n] = [pad rows (= pad_value) | past[0..n_past) | new row], 10 rows total
 * (efficient_ensemble_merged.py:378-390 front padding), new row d = centers[clip(tok_vocab - token[n][d] - 1, 0, n_centers-1)]
 * (256-bin arithmetic of policy_wrapper.py:259-266) with the gripper (last dim) mapped to 0/1 at 0.5
 * (BridgeSimplerAdapter.postprocess_gripper_verifier, simpler.py:222-226). centers: fp32 table computed on the host in
 * float64. pad_out[n][t] = 1 for padding rows. */
int cover_tokens_to_histories(const int64_t* tokens, int ld_tokens, int N, int tok_vocab, const float* centers, int n_centers,
                              const float* past, int n_past, float pad_value, float* hist_out, uint8_t* pad_out, void* stream);

/* The same for a flow-matching policy's action chunks (pi0): candidate n contributes the first n_use actions of its chunk
 * (actions fp32 [N][chunk][>=7], strides in elements) after the verifier post-processing of the reference adapter
 * (INT-ACT .../simpler.py:96-121, base.py:20-31): dims 0-5 un-normalised (a + 1) / 2 * (hi - lo) + lo with the dataset's
 * p01 / p99 (lo_hi = fp32 [12] = lo[6] | hi[6], NULL = pass through), gripper 0 if a < 0.5 else 1.
 * hist[n] = [pad rows | past[0..n_past) | n_use chunk rows], n_past + n_use <= 10. fp32 arithmetic (the reference does this
 * in float64 on the host and converts: results agree to fp32 rounding). */
/* the same for an action-chunk horizon > 1: the first n_use 7-token actions of every candidate become its n_use newest history rows
 * (the driver scores n_action_steps future steps, run_simpler_eval_with_openpi.py:338-341) */
int cover_tokens_to_histories_steps(const int64_t* tokens, int ld_tokens, int N, int tok_vocab, const float* centers, int n_centers,
                                    const float* past, int n_past, int n_use, float pad_value, float* hist_out, uint8_t* pad_out,
                                    void* stream);
int cover_actions_to_histories(const float* actions, long long n_stride, long long t_stride, int N, int n_use, const float* lo_hi,
                               const float* past, int n_past, float pad_value, float* hist_out, uint8_t* pad_out, void* stream);

/* grouped arg-max over already-computed (e.g. all-gathered) scores: same selection rule as above. Group mean = index-order fp32 sum /
 * (float)group_size; the first maximal mean wins, then the first maximal score inside that group. NaN rule (cover_token_select's): a
 * NaN never wins and if nothing wins the pick is index 0 -- a group holding a NaN has a NaN mean and is passed over; if every group
 * mean is a NaN, group 0 is taken; if every score of the taken group is a NaN, its candidate 0. result_out is therefore always in
 * range. best_out = {scores[result_out[0]], mean of group result_out[1]}, their own bits, NaNs included. */
int cover_group_argmax(const float* scores, int N, int group_size, int* result_out, float* best_out, void* stream);

/* Prior-weighted selection: the grouped arg-max of combined[n] = scores[n] + beta * prior[n], where prior[n] is the candidate's sequence
 * log-probability under the policy, summed here from its per-step values, plus the best top_m members of the winning group in rank
 * order. One launch, no workspace, recordable. Arithmetic (every sum that decides an index has a fixed result):
 *   prior[n]    = fp32 sum of the counted logprobs[n][t] in step order t = 0, 1, ..., one chain of adds from 0.0f; a step is counted
 *                 unless `tokens` is given and tokens[n][t] == pad_token_id; with length_normalize the sum is divided once by
 *                 (float)max(count, 1); a candidate with no counted step has prior 0.0. steps = 1 takes a prior that is summed already.
 *   combined[n] = scores[n] exactly when beta == 0.0f (no product: a -inf prior cannot make a NaN), else
 *                 round(scores[n] + round(beta * prior[n])): two fp32 roundings, never an fma. A -inf prior gives -inf.
 *   groups      = cover_group_argmax on combined (the same device code): group mean = index-order fp32 sum / group_size, first
 *                 maximum wins; a group holding a -inf has mean -inf; if every group does, group 0 wins. NaNs in combined follow
 *                 cover_group_argmax's rule: never a winner, and group 0 / candidate 0 if nothing wins.
 *   ranked[r]   = global index of the member of the winning group with rank r < top_m in (descending combined, ascending index)
 *                 order, so ranked[0] == result_out[0].
 * The two stride pairs (in elements) read candidate-major [N][steps] and step-major [steps][N] buffers alike, without a copy.
 * COVER_EINVAL unless N >= 1, group_size >= 1, N % group_size == 0, N / group_size <= 4096, group_size <= 4096, 1 <= steps <= 4096,
 * 0 <= top_m <= min(group_size, 64), beta finite and >= 0, the required pointers non-null and ranked_out non-null when top_m > 0. */
typedef struct cover_prior_select_args {
    const float* scores;            /* [N] verifier scores */
    const float* logprobs;          /* element (n, t) at logprobs[n * lp_n_stride + t * lp_t_stride] */
    long long lp_n_stride, lp_t_stride;
    const int64_t* tokens;          /* optional, element (n, t) at tokens[n * tok_n_stride + t * tok_t_stride] */
    long long tok_n_stride, tok_t_stride;
    long long pad_token_id;         /* with tokens: steps whose token equals it are not counted */
    int N, steps, group_size, top_m;
    float beta; int length_normalize;
    float* prior_out;               /* [N] */
    float* combined_out;            /* [N] */
    float* group_mean_out;          /* [N / group_size], optional */
    int* result_out;                /* int32 [4] = {global_idx, group_idx, idx_in_group, 0}, as cover_group_argmax */
    float* best_out;                /* float [2] = {combined of the winner, mean of its group} */
    int* ranked_out;                /* int32 [top_m] global indices, optional when top_m == 0 */
} cover_prior_select_args;
int cover_prior_select(const cover_prior_select_args* args, void* stream);

/* Per-member scores of the verifier ensemble and a disagreement-aware score. cover_score_select keeps one number per candidate, the
 * cosine of the member-AVERAGED embeddings; this entry scores every candidate under every member on its own (it / act are the per-member
 * unit rows cover_score_select takes, so a dot product is that member's cosine) and derives from them the ensemble's mean, spread and
 * worst member, a robust score, the grouped arg-max of the robust score and each member's own grouped arg-max. Two launches behind each
 * other, no workspace, no atomics, recordable. All arithmetic is fp32, one rounding per operation, never an fma; for candidate n:
 *   s_m       = member m's score: lane l of a 64-lane wave runs p = 0.0f; for d = l, l + 64, ... < dim: prod = it[m][d] * act[m][n][d];
 *               p = p + prod (a lane with no d keeps 0.0f); the 64 partials are added by the xor butterfly v = v + v[lane ^ o],
 *               o = 32, 16, 8, 4, 2, 1. member_scores_out[m * N + n] = s_m.
 *   mean      = (((0.0f + s_0) + s_1) + ... + s_{M-1}) / (float)M
 *   spread    = sqrtf(ss / (float)M), ss the same chain over dv * dv, dv = s_m - mean: the POPULATION form (the members are the whole
 *               ensemble); M == 1 gives exactly 0.
 *   min       = the smallest s_m, min_member the first m that attains it (s_m < min replaces, so a NaN never does).
 *   robust    = mode 0 (lcb): scores[n] exactly when kappa == 0.0f (no product is formed), else round(scores[n] - round(kappa * spread));
 *               mode 1 (min): min.
 *   result_out / best_out               = cover_group_argmax on robust (the same device code)
 *   member_result_out[m] / member_best_out[m] = cover_group_argmax on member_scores_out + m * N
 *   (NaN scores included: cover_group_argmax's rule, every index in range)
 * scores = the [N] fused scores cover_score_select wrote; read only.
 * COVER_EINVAL, and nothing launched, unless 1 <= n_members <= 16, N >= 1, group_size >= 1, N % group_size == 0, N / group_size <= 4096,
 * 1 <= dim <= 4096, kappa finite and >= 0, mode 0 or 1, kappa == 0 in mode 1 and every pointer non-null. */
typedef struct cover_member_scores_args {
    const float* it;                /* [n_members][dim] */
    const float* act;               /* [n_members][N][dim] */
    const float* scores;            /* [N] fused scores */
    int n_members, N, dim, group_size;
    float kappa; int mode;          /* COVER_MEMBER_LCB / COVER_MEMBER_MIN */
    float* member_scores_out;       /* [n_members][N] */
    float* mean_out;                /* [N] */
    float* spread_out;              /* [N] */
    float* min_out;                 /* [N] */
    int* min_member_out;            /* int32 [N] */
    float* robust_out;              /* [N] */
    int* result_out;                /* int32 [4], as cover_group_argmax on robust */
    float* best_out;                /* float [2] */
    int* member_result_out;         /* int32 [n_members][4] */
    float* member_best_out;         /* float [n_members][2] */
} cover_member_scores_args;
enum { COVER_MEMBER_LCB = 0, COVER_MEMBER_MIN = 1 };
int cover_member_scores(const cover_member_scores_args* args, void* stream);

/* Gaussian proposal augmentation: K cheap verifier candidates per prompt from the prompt's n policy samples. Candidates of a prompt are
 * contiguous (candidate i belongs to prompt i / n); the output has S = n + K rows per prompt: rows 0..n-1 are the policy's own samples
 * copied unchanged (token ids verbatim, floats bit for bit), rows n..S-1 are drawn from a diagonal Gaussian fitted to the samples'
 * translation / rotation dims with the gripper taken by majority vote, so downstream code sees the same tensor with group_size = S.
 * One block per prompt, one launch, no workspace, no atomics, recordable. All arithmetic is fp32, one rounding per operation, never an
 * fma; for group g, step t < h and dim d < 6, with x_j the value of sample j:
 *   mean  = (((0.0f + x_0) + x_1) + ... + x_{n-1}) / (float)n                       one chain of adds in sample order, one divide
 *   ss    = the same chain over (x_j - mean) * (x_j - mean);  var = ss / (float)(n - 1), 0 when n == 1
 *   sd    = fmaxf(sqrtf(var), sd_floor)
 *   row k : s = sigma * sd;  p = s * z[g][k][t][d];  v = mean + p;  v = fminf(fmaxf(v, clip_lo), clip_hi)
 *           (a NaN z therefore lands on clip_lo; clip_lo = -inf / clip_hi = +inf mean no clip on that side)
 * z = normals, fp32 [G][K][h][6], supplied by the caller like the samplers' uniforms: the same z gives the same bits.
 * Gripper (d == 6), per step: the class of sample j is (x_j >= 0.5f), the verifier's rule; the majority class wins, a tie goes to the
 * class of sample 0; every augmented row takes the gripper token / float of the lowest-index sample in the winning class.
 * cover_augment_tokens: src = int64 tokens, element (row, t, d) at src[row * n_stride + t * 7 + d] (n_stride >= 7 h; t_stride unused),
 *   x_j = centers[clamp(tok_vocab - token - 1, 0, n_centers - 1)] (cover_tokens_to_histories' rule); out = int64 [G * S][7 h]; an
 *   augmented value v is stored as tok_vocab - 1 - b, b the FIRST index that minimises fabsf(v - centers[b]) over all n_centers.
 * cover_augment_actions: src = fp32, element (row, t, d) at src[row * n_stride + t * t_stride + d] (strides in elements, unit last
 *   stride: a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place); centers unused; out = contiguous fp32 [G * S][h][7], v stored.
 * Optional outputs (NULL = not written): mean_out / sd_out fp32 [G][h][6] (sd after the floor), votes_out int32 [G][h][2] =
 * (class-0 count, class-1 count).
 * COVER_EINVAL unless G >= 1, 1 <= n <= 4096, 0 <= K <= 4096, 1 <= h <= 64, G * (n + K) <= 2^20, sigma and sd_floor finite and >= 0,
 * clip_lo <= clip_hi, src / out non-null, normals non-null when K > 0 and, for tokens, n_stride >= 7 h, centers non-null, n_centers >= 1.
 * K == 0 copies the originals only. */
typedef struct cover_augment_args {
    const void* src;                /* int64 tokens or fp32 actions, see above */
    long long n_stride, t_stride;   /* in elements */
    const float* normals;           /* [G][K][h][6] */
    const float* centers;           /* tokens: [n_centers] bin centres */
    int n_centers, tok_vocab;
    int G, n, K, h;
    float sigma, sd_floor, clip_lo, clip_hi;
    void* out;                      /* int64 [G * (n + K)][7 h] or fp32 [G * (n + K)][h][7] */
    float* mean_out; float* sd_out; /* [G][h][6], optional */
    int* votes_out;                 /* [G][h][2], optional */
} cover_augment_args;
int cover_augment_tokens(const cover_augment_args* args, void* stream);
int cover_augment_actions(const cover_augment_args* args, void* stream);

/* Proposal log-density prior: for every row of a prompt group, the unnormalised log-density under the diagonal Gaussian fitted to the
 * group's first n_fit rows (the distribution cover_augment_* draws its rows from; with group_rows == n_fit, how typical a policy sample
 * is among its siblings), plus optionally the log share of the row's gripper class. A group is group_rows (S) contiguous rows, row i
 * belongs to group i / S; the output is fp32 [G * S], the summed prior cover_prior_select takes with steps = 1. One block per group, one
 * launch, no workspace, no atomics, recordable. All arithmetic is fp32, one rounding per operation, never an fma, and no logarithm is
 * taken on the device. For group g, step t < h and dim d < 6:
 *   mean, sd = cover_augment_*'s fit over rows 0..n_fit-1 (the same device function: chain mean, var with n_fit - 1, 0 for one row,
 *              sd = fmaxf(sqrtf(var), sd_floor));  s = sigma * sd
 *   row r   : acc = 0.0f;  for t in step order, d = 0..5:  dev = x - mean;  z = dev / s;  sq = z * z;  acc = acc + sq
 *             p = -0.5f * acc
 *             log_share != NULL: for t in step order: c = the count, among rows 0..n_fit-1 at step t, of the class (x_6 >= 0.5f) row r
 *             has at step t;  p = p + log_share[c]
 *             prior_out[g * S + r] = p
 * The -sum log s term of the log-density is NOT included (it is the same for every row of a group). log_share = fp32 [n_fit + 1],
 * supplied by the caller (host.vote_log_shares); an entry may be -inf. A NaN element gives a NaN prior for its own row when the row is
 * not among the fitted ones.
 * cover_proposal_prior_tokens: src = int64 tokens, element (row, t, d) at src[row * n_stride + t * 7 + d] (t_stride unused),
 *   x = centers[clamp(tok_vocab - token - 1, 0, n_centers - 1)].
 * cover_proposal_prior_actions: src = fp32, element (row, t, d) at src[row * n_stride + t * t_stride + d] (strides in elements, unit
 *   last stride); centers unused.
 * Optional outputs (NULL = not written): mean_out / sd_out fp32 [G][h][6] (sd after the floor), votes_out int32 [G][h][2], as
 * cover_augment_* writes them.
 * COVER_EINVAL unless G >= 1, 1 <= n_fit <= group_rows <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, sigma and sd_floor finite and > 0
 * with an fp32 product > 0 (so s > 0 and dev / s is never 0 / 0), src / prior_out non-null and, for tokens, n_stride >= 7 h, centers
 * non-null, n_centers >= 1. */
typedef struct cover_proposal_prior_args {
    const void* src;                /* int64 tokens or fp32 actions, see above */
    long long n_stride, t_stride;   /* in elements */
    const float* centers;           /* tokens: [n_centers] bin centres */
    const float* log_share;         /* [n_fit + 1], optional */
    int n_centers, tok_vocab;
    int G, group_rows, n_fit, h;
    float sigma, sd_floor;
    float* prior_out;               /* [G * group_rows] */
    float* mean_out; float* sd_out; /* [G][h][6], optional */
    int* votes_out;                 /* [G][h][2], optional */
} cover_proposal_prior_args;
int cover_proposal_prior_tokens(const cover_proposal_prior_args* args, void* stream);
int cover_proposal_prior_actions(const cover_proposal_prior_args* args, void* stream);

/* Verifier-guided refinement: one round of the cross-entropy method per prompt group, on the device. A group is group_rows (S) contiguous
 * candidate rows (row i belongs to group i / S) with one fp32 score per row -- whatever the decision was made on: the verifier's scores,
 * cover_member_scores' robust or cover_prior_select's combined. Per group the n_elite (m) best-scored rows are kept, the diagonal Gaussian
 * of cover_augment_* is refitted on them and K new rows are drawn from it; the output has m + K rows per group, so downstream code sees
 * what cover_augment_* would have given it, with group_size = m + K and n_fit = m. One 256-thread block per group, one launch, no
 * workspace, no atomics, recordable.
 * Ranking: row j of the group ranks before row j' when its score is higher, or the scores are equal (-0.0 and +0.0 are one score) and
 *   j < j'. A NaN score (either sign) ranks behind every number, -inf included; NaNs among themselves rank by ascending index. (A bitonic
 *   sort in LDS of the unique 64-bit keys (descending-order image of the score, all ones for a NaN) << 32 | j, padded to a power of two
 *   with all-ones keys: the order is this rule whatever the schedule.)
 * Gather: output row r < m of group g is the input row of rank r, verbatim -- tokens: the ids of its first 7 h columns; actions: the
 *   first 7 dims of every step, bit for bit. elite_rows_out[g][r] = g * S + j, that row's index in the input; elite_scores_out[g][r] =
 *   scores[g * S + j], bit for bit (a NaN keeps its payload).
 * Fit and draw: rows m..m+K-1 of group g are EXACTLY rows n..n+K-1 that cover_augment_tokens / cover_augment_actions give with
 *   src = the group's m gathered rows (n = m, n_stride = 7 h, t_stride = 7), the same normals, sigma, sd_floor, clip and centre table --
 *   the same device functions, so rounding by rounding, with x_r the value of the elite of rank r:
 *   mean  = (((0.0f + x_0) + x_1) + ... + x_{m-1}) / (float)m                       one chain of adds in RANK order, best elite first
 *   ss    = the same chain over (x_r - mean) * (x_r - mean);  var = ss / (float)(m - 1), 0 when m == 1
 *   sd    = fmaxf(sqrtf(var), sd_floor)
 *   row k : s = sigma * sd;  p = s * z[g][k][t][d];  v = mean + p;  v = fminf(fmaxf(v, clip_lo), clip_hi)
 *   all fp32, one rounding per operation, never an fma. Gripper (d == 6), per step: the majority class (x >= 0.5f) of the elites wins, a
 *   tie goes to the class of the BEST elite; every drawn row takes the gripper token / float of the best-ranked elite in the winning class.
 * cover_refine_tokens: src = int64 tokens, element (row, t, d) at src[row * n_stride + t * 7 + d] (n_stride >= 7 h; t_stride unused);
 *   out = int64 [G * (m + K)][7 h]; values through centers / tok_vocab as in cover_augment_tokens.
 * cover_refine_actions: src = fp32, element (row, t, d) at src[row * n_stride + t * t_stride + d] (strides in elements, unit last
 *   stride: a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place); centers unused; out = contiguous fp32 [G * (m + K)][h][7].
 * Only the cells named above are read: nothing of src outside the [rows][h][7] view. out must not overlap src.
 * Optional outputs (NULL = not written): elite_rows_out int32 [G][m], elite_scores_out fp32 [G][m], mean_out / sd_out fp32 [G][h][6]
 * (sd after the floor), votes_out int32 [G][h][2] = (class-0 count, class-1 count) among the elites.
 * COVER_EINVAL, and nothing launched, unless G >= 1, 1 <= n_elite <= group_rows <= 4096, 0 <= K <= 4096, 1 <= h <= 64,
 * G * group_rows <= 2^20, G * (n_elite + K) <= 2^20, sigma and sd_floor finite and >= 0, clip_lo <= clip_hi, src / scores / out non-null,
 * normals non-null when K > 0 and, for tokens, n_stride >= 7 h, centers non-null, n_centers >= 1. K == 0 is a pure top-m gather. */
typedef struct cover_refine_args {
    const void* src;                /* int64 tokens or fp32 actions, see above */
    long long n_stride, t_stride;   /* in elements */
    const float* scores;            /* [G * group_rows] */
    const float* normals;           /* [G][K][h][6] */
    const float* centers;           /* tokens: [n_centers] bin centres */
    int n_centers, tok_vocab;
    int G, group_rows, n_elite, K, h, _pad;
    float sigma, sd_floor, clip_lo, clip_hi;
    void* out;                      /* int64 [G * (n_elite + K)][7 h] or fp32 [G * (n_elite + K)][h][7] */
    int* elite_rows_out;            /* int32 [G][n_elite], optional */
    float* elite_scores_out;        /* [G][n_elite], optional */
    float* mean_out; float* sd_out; /* [G][h][6], optional */
    int* votes_out;                 /* [G][h][2], optional */
} cover_refine_args;
int cover_refine_tokens(const cover_refine_args* args, void* stream);
int cover_refine_actions(const cover_refine_args* args, void* stream);

/* Neighbourhood-smoothed scores: per prompt group a kernel-weighted local mean (Nadaraya-Watson) of one fp32 score per row over the rows'
 * positions in the 6-D action space, shrunk towards the group mean where a row has few neighbours. A group is group_rows (S) contiguous
 * rows (row i belongs to group i / S) with one fp32 score per row -- the verifier's scores or cover_member_scores' robust; the output is
 * fp32 [G * S] and goes where those go (cover_group_argmax, cover_prior_select, cover_refine_*). One wave per row, 16 rows per block,
 * several blocks per group; the group's values pass through LDS in tiles of rows. One launch, no workspace, no atomics, recordable; no
 * result depends on the tiling. All arithmetic is fp32, one rounding per operation, never an fma.
 * Pair weight of row n and row j != n of one group, x the rows' values:
 *   d2 = 0.0f;  for t in step order, d = 0..5 with dim_scale[d] != 0:  diff = x_n - x_j;  sc = diff * dim_scale[d];  sq = sc * sc;
 *   d2 = d2 + sq   (a dim whose scale is 0 is not read into the sum: a NaN there is invisible)
 *   w = (d2 < radius2) ? 1.0f - d2 / radius2 : 0.0f   a divide, then a subtract; a NaN d2 fails the comparison, so w = 0
 *   split_gripper != 0: if the classes (x_6 >= 0.5f) of n and j differ at any step, w = 0. Dim 6 never enters d2.
 *   The self pair j == n has w = 1.0f by definition. A dim_scale entry that is negative or not finite makes every pair weight 0 (the
 *   self pair keeps 1); there is no trap.
 * Row sums, lane l of the row's wave: num = den = dsum = 0.0f, cnt = 0; for j = l, l + 64, ... < S in ascending order, where w > 0:
 *   dsum = dsum + w;  cnt += 1;  and if scores[j] is finite:  den = den + w;  prod = w * scores[j];  num = num + prod
 *   (where w == 0 no product is formed). The 64 partials of num, den and dsum each meet in the xor butterfly v = v + v[lane ^ o],
 *   o = 32, 16, ..., 1; cnt is an integer sum.
 * Group mean m0: the same lane-strided chain (sum = sum + scores[j] over the finite scores) and butterfly, divided once by (float)count
 *   of the finite scores; with no finite score in the group no divide is made, m0 is unused and group_mean_out holds 0.0f.
 * Result: a row whose own score is not finite (NaN, +-inf) stores its score bit for bit (a NaN keeps its payload; a -inf from a prior
 *   stays -inf). Every other row has den >= 1 through its self term:
 *   shrink == 0:  smoothed = num / den   (no product is formed)
 *   otherwise  :  tm = shrink * m0;  nn = num + tm;  dd = den + shrink;  smoothed = nn / dd
 * cover_smooth_scores_tokens: src = int64 tokens, element (row, t, d) at src[row * n_stride + t * 7 + d] (n_stride >= 7 h; t_stride
 *   unused), x = centers[clamp(tok_vocab - token - 1, 0, n_centers - 1)] (cover_tokens_to_histories' rule).
 * cover_smooth_scores_actions: src = fp32, element (row, t, d) at src[row * n_stride + t * t_stride + d] (strides in elements, unit last
 *   stride: a [B, steps, 7] view of a [B, chunk, 32] buffer, or a padded history tensor [N, 10, 7], is read in place); centers unused.
 * Only the cells named above are read: nothing of src outside the [rows][h][7] view.
 * Optional outputs (NULL = not written): density_out fp32 [G * S] = dsum / (float)S, neighbours_out int32 [G * S] = cnt (self included),
 * group_mean_out fp32 [G].
 * COVER_EINVAL, and nothing launched, unless G >= 1, 1 <= group_rows <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, radius2 finite and
 * > 0, shrink finite and >= 0, src / scores / dim_scale / smoothed_out non-null and, for tokens, n_stride >= 7 h, centers non-null,
 * n_centers >= 1. dim_scale is device memory: the caller validates its values (finite, >= 0). */
typedef struct cover_smooth_args {
    const void* src;                /* int64 tokens or fp32 actions, see above */
    long long n_stride, t_stride;   /* in elements */
    const float* scores;            /* [G * group_rows] */
    const float* dim_scale;         /* [6], device */
    const float* centers;           /* tokens: [n_centers] bin centres */
    int n_centers, tok_vocab;
    int G, group_rows, h, split_gripper;
    float radius2, shrink;
    float* smoothed_out;            /* [G * group_rows] */
    float* density_out;             /* [G * group_rows], optional */
    int* neighbours_out;            /* int32 [G * group_rows], optional */
    float* group_mean_out;          /* [G], optional */
} cover_smooth_args;
int cover_smooth_scores_tokens(const cover_smooth_args* args, void* stream);
int cover_smooth_scores_actions(const cover_smooth_args* args, void* stream);

/* Chunk-coherence prior: per candidate row the negated, signed-weighted sum of its step-weighted squared distances to a set of reference
 * chunks. With one reference of weight 1 -- the unexecuted tail of the chunk committed at the last decision -- it is the backward
 * coherence of Bidirectional Decoding (Liu et al., 2024); with a group's strong rows at positive and a weak policy's rows at negative
 * weights it is the forward contrast. A group is group_rows (S) contiguous candidate rows (row i belongs to group i / S); the output is
 * fp32 [G * S], a prior (higher = more coherent) that goes where priors go: cover_prior_select's prior. One wave per row, 16 rows per
 * block, several blocks per group; the reference rows pass through LDS in tiles. One launch, no workspace, no atomics, recordable; no
 * result depends on the tiling. All arithmetic is fp32, one rounding per operation, never an fma.
 * Candidate step t is compared with reference step t + shift; the overlap is T = min(h, hr - shift) steps.
 * Pair (row n, reference r), x the candidate value and y the reference value:
 *   D = 0.0f
 *   for t = 0..T-1 in order:
 *     e = 0.0f
 *     for d = 0..5 with dim_scale[d] != 0:  diff = x - y;  s = diff * dim_scale[d];  sq = s * s;  e = e + sq
 *       (a dim whose scale is 0 is not read into the sum: a NaN there is invisible)
 *     if gripper_penalty != 0 and the classes (x_6 >= 0.5f) and (y_6 >= 0.5f) differ:  e = e + gripper_penalty
 *     p = step_weight[t] * e;  D = D + p
 * Row n, lane l of the row's wave:
 *   acc = 0.0f;  for r = l, l + 64, ... < R ascending, where w_r != 0:  prod = w_r * D;  acc = acc + prod
 *   (a reference of weight 0 is never read into a sum, so a NaN there is invisible). The 64 partials meet in the xor butterfly
 *   v = v + v[lane ^ o], o = 32, 16, ..., 1.
 *   prior_out[g * S + n] = -acc as a sign-bit flip: a candidate that equals its only reference stores 0x80000000. A NaN acc stores the
 *   one NaN 0x7FC00000 (the payload and sign of an arithmetic NaN are not specified). A NaN candidate element inside the overlap, in a
 *   dim of non-zero scale, gives its row a NaN prior (given a reference of non-zero weight) and no other row.
 *   A dim_scale entry that is negative or not finite makes every prior of the launch 0x7FC00000, every min_dist +inf and every nearest
 *   -1; there is no trap.
 * Optional outputs (NULL = not written): min_dist_out fp32 [G * S], the smallest D over the references with w_r != 0 whose D is not NaN
 *   (+inf when there is none); nearest_out int32 [G * S], the index r of that reference, the lowest r on a tie (-1 when there is none).
 *   It is the lexicographic (D, r) minimum, so it does not depend on the schedule.
 * cover_coherence_prior_tokens: src = int64 tokens, element (row, t, d) at src[row * n_stride + t * 7 + d] (n_stride >= 7 h; t_stride
 *   unused), x = centers[clamp(tok_vocab - token - 1, 0, n_centers - 1)] (cover_tokens_to_histories' rule).
 * cover_coherence_prior_actions: src = fp32, element (row, t, d) at src[row * n_stride + t * t_stride + d] (strides in elements, unit last
 *   stride: a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place); centers unused.
 * ref is fp32 in both forms: element (g, r, t, d) at ref[g * ref_g_stride + r * ref_r_stride + t * 7 + d], R rows of hr steps;
 *   ref_g_stride == 0 is one reference set shared by all groups. ref_weight is fp32, signed: element (g, r) at
 *   ref_weight[g * w_g_stride + r], w_g_stride 0 or R. step_weight fp32 [h] (the caller's, made on the host: the device takes no pow),
 *   dim_scale fp32 [6]; all of them device memory.
 * Only the cells named above are read: nothing of src outside the first T steps of its [rows][h][7] view, nothing of ref outside steps
 * shift .. shift + T - 1 of its [R][hr][7] rows.
 * COVER_EINVAL, and nothing launched, unless G >= 1, 1 <= group_rows <= 4096, 1 <= R <= 4096, 1 <= h <= 64, 1 <= hr <= 64,
 * 0 <= shift < hr, G * group_rows <= 2^20, ref_g_stride == 0 or >= (R - 1) * ref_r_stride + 7 hr, ref_r_stride >= 7 hr, w_g_stride 0 or
 * R, gripper_penalty finite and >= 0, src / ref / ref_weight / step_weight / dim_scale / prior_out non-null and, for tokens,
 * n_stride >= 7 h, centers non-null, n_centers >= 1. */
typedef struct cover_coherence_args {
    const void* src;                /* int64 tokens or fp32 actions, see above */
    long long n_stride, t_stride;   /* in elements */
    const float* centers;           /* tokens: [n_centers] bin centres */
    int n_centers, tok_vocab;
    const float* ref;               /* fp32 reference chunks */
    long long ref_g_stride, ref_r_stride;   /* in elements */
    const float* ref_weight;        /* signed, [R] or [G][R] */
    long long w_g_stride;           /* 0 or R */
    const float* step_weight;       /* [h] */
    const float* dim_scale;         /* [6] */
    int G, group_rows, h, R, hr, shift;
    float gripper_penalty;
    float* prior_out;               /* [G * group_rows] */
    float* min_dist_out;            /* [G * group_rows], optional */
    int* nearest_out;               /* int32 [G * group_rows], optional */
} cover_coherence_args;
int cover_coherence_prior_tokens(const cover_coherence_args* args, void* stream);
int cover_coherence_prior_actions(const cover_coherence_args* args, void* stream);

/* Diverse candidate subsets: per prompt group a greedy selection of at most m of its S rows by quality plus weight times the distance to
 * the rows already chosen (maximal marginal relevance; with no quality, the farthest-point traversal), with an optional covering
 * distance that leaves out rows already covered by a pick. A group is group_rows (S) contiguous rows (row i belongs to group i / S).
 * The picks are sequential, so the whole loop is one launch: one 1024-thread block per group, thread tid owning rows tid + 1024 q. One
 * launch, no workspace, no atomics, recordable; no result depends on the schedule. All arithmetic is fp32, one rounding per operation,
 * never an fma.
 * Pair distance D(i, j) of two rows of one group: cover_coherence_prior's D with T = h and shift = 0, x / y the rows' values:
 *   D = 0.0f
 *   for t = 0..h-1 in order:
 *     e = 0.0f
 *     for d = 0..5 with dim_scale[d] != 0:  diff = x - y;  s = diff * dim_scale[d];  sq = s * s;  e = e + sq
 *       (a dim whose scale is 0 is not read into the sum: a NaN there is invisible)
 *     if gripper_penalty != 0 and the classes (x_6 >= 0.5f) and (y_6 >= 0.5f) differ:  e = e + gripper_penalty
 *     p = step_weight[t] * e;  D = D + p
 * quality: fp32 [G * S], optional; NULL = every quality is 0.0f. weight: the factor of the distance term.
 * Per group:
 *   Row i is ELIGIBLE iff quality[i] is not NaN and D(i, i) is not NaN (so: every element the distance reads is finite; a NaN in dim 6
 *   or in a dim of scale 0 is invisible). A dim_scale entry that is negative or not finite makes no row eligible; there is no trap.
 *   mind[i] = +inf, assign[i] = -1 for every row.
 *   Pick 0: the eligible row of the largest quality, the lowest index on a tie (-0 == +0). Its value v is its quality.
 *   Pick k >= 1: row i is a CANDIDATE iff it is eligible, not picked yet and mind[i] > cover_dist. Its value is
 *     weight == 0:  v = quality[i]          (no product is formed)
 *     otherwise  :  prod = weight * mind[i];  v = quality[i] + prod
 *     and a row whose v is NaN is no candidate at this step. The pick is the lexicographic (v descending with -0 == +0, index
 *     ascending) maximum over the candidates. With no candidate the selection ends: count = k.
 *   After every pick, slot k holding row p, EVERY row i of the group (picked, ineligible and row p itself included) is updated:
 *     d = D(i, p);  if d < mind[i]: mind[i] = d, assign[i] = k     (strict: an equal distance keeps the earlier slot; a NaN d never
 *     enters). The update after the last pick runs too, so assign and row_dist are final.
 *   cover_dist < 0 switches the covering rule off (mind >= 0 > cover_dist for every row, +inf included); cover_dist == 0 leaves out
 *   rows at distance 0 of a pick (exact duplicates in the dims that count); cover_dist = r > 0 ends the selection once every eligible row
 *   lies within r of a pick, so count adapts to the group.
 * Outputs (NULL = not written, except picked_rows_out; every cell of a given output is stored, unfilled slots k >= count included):
 *   picked_rows_out int32 [G][m]   the global row g * S + p of slot k                       unfilled: -1
 *   count_out       int32 [G]      the number of picks made
 *   pick_value_out  fp32 [G][m]    v at pick time (the value's bits)                        unfilled: 0x7FC00000
 *   pick_dist_out   fp32 [G][m]    mind[p] at pick time; +inf for slot 0                    unfilled: +inf
 *   assign_out      int32 [G * S]  the slot of the nearest pick, -1 where there is none
 *   row_dist_out    fp32 [G * S]   the final mind
 *   out             int64 [G * m][7 h] (tokens) or fp32 [G * m][h][7] (actions): the picked rows verbatim, as cover_refine_* gathers its
 *                   elites; an unfilled slot repeats the group's slot-0 row, a group with no pick stores its input row 0 in every slot.
 * cover_diverse_subset_tokens: src = int64 tokens, element (row, t, d) at src[row * n_stride + t * 7 + d] (n_stride >= 7 h; t_stride
 *   unused), x = centers[clamp(tok_vocab - token - 1, 0, n_centers - 1)] (cover_tokens_to_histories' rule).
 * cover_diverse_subset_actions: src = fp32, element (row, t, d) at src[row * n_stride + t * t_stride + d] (strides in elements, unit last
 *   stride: a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place); centers unused.
 * Only the cells named above are read: nothing of src outside its [rows][h][7] view. step_weight fp32 [h] (the caller's, made on the
 * host), dim_scale fp32 [6]; both device memory.
 * The group's values stay in LDS (row stride 7 h | 1 floats) when 4 * ((S + 1) * (7 h | 1) + h + m) <= 160 KiB - 256 B, and are read
 * from src again at every distance otherwise; the choice is a function of (S, m, h) alone and both paths run the same arithmetic.
 * COVER_EINVAL, and nothing launched, unless G >= 1, 1 <= m <= group_rows <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, weight finite
 * and >= 0, cover_dist not NaN and < +inf, gripper_penalty finite and >= 0, src / step_weight / dim_scale / picked_rows_out non-null
 * and, for tokens, n_stride >= 7 h, centers non-null, n_centers >= 1. */
typedef struct cover_diverse_args {
    const void* src;                /* int64 tokens or fp32 actions, see above */
    long long n_stride, t_stride;   /* in elements */
    const float* centers;           /* tokens: [n_centers] bin centres */
    int n_centers, tok_vocab;
    const float* quality;           /* [G * group_rows], optional */
    const float* step_weight;       /* [h] */
    const float* dim_scale;         /* [6] */
    int G, group_rows, m, h;
    float weight, cover_dist, gripper_penalty, _pad;
    int* picked_rows_out;           /* int32 [G][m] */
    int* count_out;                 /* int32 [G], optional */
    float* pick_value_out;          /* [G][m], optional */
    float* pick_dist_out;           /* [G][m], optional */
    int* assign_out;                /* int32 [G * group_rows], optional */
    float* row_dist_out;            /* [G * group_rows], optional */
    void* out;                      /* int64 [G * m][7 h] or fp32 [G * m][h][7], optional */
} cover_diverse_args;
int cover_diverse_subset_tokens(const cover_diverse_args* args, void* stream);
int cover_diverse_subset_actions(const cover_diverse_args* args, void* stream);

/* pi0-FAST de-tokeniser: generated PaliGemma ids -> FAST ids -> the pieces' code points -> quantised DCT coefficients -> an fp32 action
 * chunk [H][D] per row, the layout the *_actions entries above read in place. The semantics are defined on ids (no text round trip): a
 * FAST id decodes to a fixed piece of code points, and a row's symbol string is the concatenation of its pieces in position order.
 * One launch, one 256-thread block per row, no workspace, no atomics, no host read-back: recordable. The expansion is integer-exact, the
 * IDCT all fp32, one rounding per operation, never an fma; no result depends on the schedule.
 * tokens: int64, element (b, p) at tokens[b * tok_row_stride + p * tok_step_stride] (strides in elements, >= 0): a candidate-major
 *   [B][L] tensor and a step-major [L][B] buffer are read in place, as cover_prior_select reads them.
 * The piece table (device memory): piece_off int32 [n_pieces + 1], non-decreasing from 0; piece_sym int32 [piece_off[n_pieces]], the
 *   code points FAST id f decodes to at piece_sym[piece_off[f] .. piece_off[f + 1]). A piece whose FIRST symbol is negative marks an id
 *   the caller's BPE could not decode. L * (the longest piece) < 2^31 is the caller's to keep (ops.fast_piece_table: at most 2^18
 *   symbols in all).
 * Per row b:
 *   1. stop = the first position p whose token is one of stop_ids[0 .. n_stop), or L when there is none; then status bit 32.
 *   2. Every position p < stop, token t:
 *        band_lo <= t < band_hi and f = band_hi - 1 - t < n_pieces:  the piece of f. Undecodable: status bit 16, no symbols.
 *                                                                      Otherwise len_p = piece_off[f + 1] - piece_off[f] symbols (0 is fine).
 *        else t one of skip_ids[0 .. n_skip):                        nothing
 *        else:                                                        status bit 8 (an id outside the band, f >= n_pieces, a negative id)
 *   3. n = the integer sum of len_p; a piece's symbols start at the exclusive prefix sum of len_p over the positions before it.
 *   4. q[s] = sym + min_token for symbol s < H * D of the concatenation, q[s] = 0 for n <= s < H * D. relaxed: n > H * D sets bit 1
 *      (truncated, possibly inside a piece), n < H * D bit 2 (padded). Not relaxed: n != H * D sets bit 4.
 *   5. If any of the bits 4, 8, 16 is set, every q is 0.
 *   6. coeff_out[b][s] = q[s], n_symbols[b] = n (before truncation), status[b] = the bits.
 *   7. The coefficient matrix is q as [H][D], frequency-major: k = s / D, d = s % D.
 *   8. c[k][d] = (float)q[k][d] / scale;  acc = 0.0f;  for k = 0 .. H-1 in order: prod = basis[t][k] * c[k][d];  acc = acc + prod;
 *      out(b, t, d) = acc at out[b * out_n_stride + t * out_t_stride + d]. The chain always runs, so a zeroed row stores +0.0f.
 *   9. Every (t, d) of every row is stored, and no other cell of out: the first D columns of a [B][chunk][32] buffer can be the target.
 * basis: fp32 [H][H], basis[t][k] = the orthonormal inverse DCT-II (DCT-III) matrix, made on the host (host.fast_idct_basis): the device
 *   takes no cosine. It is staged in LDS next to c when 4 * (H * D + H * H) <= 64 KiB and read from memory otherwise; both run the same
 *   arithmetic.
 * Optional outputs (NULL = not written): coeff_out int32 [B][H * D], n_symbols int32 [B], status int32 [B].
 * COVER_EINVAL, and nothing launched, unless 1 <= B <= 2^20, 1 <= L <= 4096, 1 <= H <= 128, 1 <= D <= 32, n_pieces >= 1,
 * 0 <= band_lo <= band_hi, 0 <= n_stop <= 4, 0 <= n_skip <= 8, |min_token| <= 2^30, scale finite and != 0, relaxed 0 or 1, token strides
 * >= 0, out_t_stride >= D, out_n_stride >= (H - 1) * out_t_stride + D (when B > 1), tokens / piece_off / piece_sym / basis / out non-null. */
#define COVER_FAST_TRUNCATED 1
#define COVER_FAST_PADDED 2
#define COVER_FAST_MISMATCH 4
#define COVER_FAST_STRAY 8
#define COVER_FAST_UNDECODABLE 16
#define COVER_FAST_NO_TERMINATOR 32
typedef struct cover_fast_decode_args {
    const int64_t* tokens;          /* element (b, p) at tokens[b * tok_row_stride + p * tok_step_stride] */
    long long tok_row_stride, tok_step_stride;
    long long band_lo, band_hi;     /* the half-open band of PaliGemma ids that carry FAST ids */
    long long stop_ids[4];
    long long skip_ids[8];
    int n_stop, n_skip;
    const int* piece_off;           /* int32 [n_pieces + 1] */
    const int* piece_sym;           /* int32 [piece_off[n_pieces]] */
    const float* basis;             /* fp32 [H][H] */
    int B, L, n_pieces, min_token;
    int H, D, relaxed;
    float scale;
    float* out;                     /* element (b, t, d) at out[b * out_n_stride + t * out_t_stride + d] */
    long long out_n_stride, out_t_stride;
    int* coeff_out;                 /* int32 [B][H * D], optional */
    int* n_symbols;                 /* int32 [B], optional */
    int* status;                    /* int32 [B], optional */
} cover_fast_decode_args;
int cover_fast_decode(const cover_fast_decode_args* args, void* stream);

/* Beam search: the three launches a step-synchronous beam search adds to top-n lists (cover_token_topn) and a decode pass. No
 * workspace, nothing data-dependent in a launch (recordable), every result a fixed function of the inputs.
 *
 * cover_beam_merge: one step of `groups` prompt groups x B beams (1 <= B <= 64); row g * B + b is beam b of group g.
 *   cum[row]               the beam's score so far; -inf or NaN marks a dead beam
 *   cand_tok / cand_lp     [groups * B, >= B] with row strides ld_tok / ld_lp: the row's top-B list exactly as cover_token_topn writes it
 *                          (descending logit, equal logits by ascending id, padded with -1 / -inf)
 *   candidate (b, j)       score = cum[b] + cand_lp[b][j], ONE fp32 add; live iff cum[b] is finite, cand_tok[b][j] >= 0 and
 *                          cand_lp[b][j] is finite
 *   output beam r          the r-th live candidate of the group in the order: higher score first (-0 == +0), then lower b, then lower j
 *   parent_out[row]        b of the chosen candidate (the row index INSIDE the group)        -1   when fewer than r + 1 are live
 *   token_out[row]         its cand_tok                                                      -1
 *   feed_out[row]          token_out, what the next embedding gather may safely read         feed_pad (a valid token id, >= 0)
 *   cum_out[row]           its score                                                         -inf
 *   step_lp_out[row]       its cand_lp                                                       -inf
 * cum and cum_out must not alias (COVER_EINVAL when they are the same pointer). One block per group: a bitonic sort of the B * B
 * 64-bit keys (score image, b * B + j) in LDS; the keys are unique, so the order is the rule above whatever the schedule. */
typedef struct cover_beam_merge_args {
    const float* cum;                          /* [groups * B] */
    const int64_t* cand_tok; long long ld_tok; /* [groups * B, B] */
    const float* cand_lp; long long ld_lp;     /* [groups * B, B] */
    long long feed_pad;
    int groups, B;
    int* parent_out; int64_t* token_out; int64_t* feed_out; float* cum_out; float* step_lp_out;   /* [groups * B] each */
} cover_beam_merge_args;
int cover_beam_merge(const cover_beam_merge_args* args, void* stream);

/* cover_kv_gather_slots: rows x n_layers slot-to-slot copies inside ONE region of the per-layer bf16 K / V^T caches, one launch.
 * k_base / vt_base are DEVICE tables [n_layers] of the layers' cache allocations (16-byte aligned); the region starts k_offset /
 * vt_offset elements into each and holds n_slots slots, K [slot][t][Hkv][D] and V^T [slot][Hkv][D][cap] (dense inside a slot, slot
 * strides in elements). For every row, K rows t < n_t and V^T columns t < n_t of slot dst_slot[row] become those of slot
 * src_slot[row], in every layer. A row whose src_slot or dst_slot is outside [0, n_slots) is skipped; several rows may name one source.
 * THE CALLER GUARANTEES that no destination slot is also a source and that the destinations are distinct (the copies of a launch run
 * in no order). K is copied exactly; V^T in whole 16-byte runs, so up to 7 columns past n_t of a DESTINATION slot may be overwritten
 * with the source's -- nothing outside destination slots is written. n_t == 0 and rows == 0 are legal no-ops.
 * COVER_EINVAL unless 1 <= n_layers <= 65535, n_slots >= 1, cap a positive multiple of 8, Hkv * D a multiple of 8,
 * Hkv * D * cap < 2^31, 0 <= n_t <= cap, offsets >= 0, offsets and slot strides multiples of 8 and slot strides >= Hkv * D * cap. */
typedef struct cover_kv_gather_slots_args {
    const void* const* k_base; const void* const* vt_base;   /* device tables [n_layers] */
    long long k_offset, vt_offset, k_slot_stride, vt_slot_stride;
    const int* src_slot; const int* dst_slot;                /* device int32 [rows] */
    int n_layers, rows, n_slots, cap, Hkv, D, n_t, _pad;
} cover_kv_gather_slots_args;
int cover_kv_gather_slots(const cover_kv_gather_slots_args* args, void* stream);

/* cover_beam_backtrack: parent int32, token int64, step_lp fp32, all step-major [steps, rows] as cover_beam_merge wrote them step by
 * step (rows = groups * B) -> candidate-major tokens_out int64 [rows, steps] and logprobs_out fp32 [rows, steps]: the sequence that ends
 * in each final beam. Final beam r's entries of the last step are its own; parent[s][.] then names the beam of step s - 1 inside the
 * group. A parent outside [0, B) anywhere leaves the candidate's remaining EARLIER steps as -1 / -inf. rows % B == 0, steps >= 1. */
typedef struct cover_beam_backtrack_args {
    const int* parent; const int64_t* token; const float* step_lp;   /* [steps, rows] */
    int steps, rows, B, _pad;
    int64_t* tokens_out; float* logprobs_out;                        /* [rows, steps] */
} cover_beam_backtrack_args;
int cover_beam_backtrack(const cover_beam_backtrack_args* args, void* stream);

/* Stochastic beam search (Kool, van Hoof and Welling, 2019): the two launches that turn the beam search above into a sample of B distinct
 * sequences WITHOUT REPLACEMENT from the policy's sequence distribution at a temperature. A beam carries phi, its cumulative
 * log-probability, and G, its perturbed score (the root of a group: phi = 0, G = 0). cover_kv_gather_slots and cover_beam_backtrack are
 * used as they are. No workspace, nothing data-dependent in a launch (recordable), no atomic decides a result.
 *
 * cover_gumbel_topn: per row (one beam) the n children with the largest perturbed score. Over columns [lo, hi), hi - lo <= 4096, with
 * one uniform u_v per column (uniform[row * ld_u + v - lo]), all fp32:
 *   lp_v = log softmax(logits / temperature)_v over [lo, hi): cover_token_logprob's value at (temperature, top_k 0, top_p 1), bit for bit
 *   u'_v = fminf(fmaxf(u_v, 2^-24), 1 - 2^-24)                          (a NaN uniform is 2^-24)
 *   g_v  = (phi + lp_v) - logf(-logf(u'_v))                             a column whose lp_v or g_v is not finite is a dead child
 *   Z    = max_v g_v
 *   v_v  = G - g_v + log1pf(-expf(g_v - Z))                             -inf at g_v == Z
 *   g~_v = G - fmaxf(0, v_v) - log1pf(expf(-|v_v|))                     every column with g_v == Z gets g~_v == G, bit for bit
 * token_out (absolute ids) / logprob_out (lp_v) / perturbed_out (g~_v), each [rows, n] with its row stride, hold the live children in the
 * order (g~ descending, column ascending) on the fp32 g~ values of the launch itself (-0 == +0); slots past them are -1 / -inf / -inf.
 * A row whose phi or g_parent is not finite is a dead beam: no logit and no uniform of it is read, its outputs are all padding.
 * One 1024-thread block per row; the order is a bitonic sort of unique 64-bit keys (g~ image, column) in LDS.
 * COVER_EINVAL unless every pointer is set, 0 <= lo < hi, hi - lo <= 4096, rows >= 0, temperature > 0, 1 <= n <= 64,
 * ld_u >= hi - lo and ld_tok, ld_lp, ld_g >= n. */
typedef struct cover_gumbel_topn_args {
    const float* logits; long long ld;           /* fp32 [rows, >= hi] */
    int rows, lo, hi;
    float temperature;
    const float* phi; const float* g_parent;     /* [rows] */
    const float* uniform; long long ld_u;        /* [rows, hi - lo] */
    int n, _pad;
    int64_t* token_out; long long ld_tok;        /* [rows, n] */
    float* logprob_out; long long ld_lp;         /* [rows, n] */
    float* perturbed_out; long long ld_g;        /* [rows, n] */
} cover_gumbel_topn_args;
int cover_gumbel_topn(const cover_gumbel_topn_args* args, void* stream);

/* cover_beam_merge_gumbel: cover_beam_merge ordered by a stored key in place of the score. cand_g [groups * B, >= B] (row stride ld_g)
 * is the lists' perturbed_out. Candidate (b, j) is live iff cum[b] is finite, cand_tok[b][j] >= 0 and cand_lp[b][j] and cand_g[b][j]
 * are finite. Output beam r is the r-th live candidate in the order: higher cand_g first (the stored float, -0 == +0; no arithmetic is
 * done on it), then lower b, then lower j. parent_out / token_out / feed_out / cum_out (= cum[b] + cand_lp[b][j], ONE fp32 add) /
 * step_lp_out and their padding are cover_beam_merge's;
 *   g_out[row]       the chosen candidate's cand_g                                       -inf when fewer than r + 1 are live
 *   kappa_out[g]     optional, [groups]: the cand_g of the (B + 1)-th candidate of the group in that order, -inf when fewer than B + 1 are
 *                    live: the threshold of the paper's importance weights -- a returned sequence s was included with probability
 *                    q(s) = 1 - exp(-exp(phi_s - kappa)), so sum_s p(s) / q(s) f(s) estimates E_p[f]. It falls out of the same sort.
 * cum and cum_out must not alias. Errors as cover_beam_merge, and ld_g >= B. */
typedef struct cover_beam_merge_gumbel_args {
    const float* cum;                          /* [groups * B] */
    const int64_t* cand_tok; long long ld_tok; /* [groups * B, B] */
    const float* cand_lp; long long ld_lp;     /* [groups * B, B] */
    const float* cand_g; long long ld_g;       /* [groups * B, B] */
    long long feed_pad;
    int groups, B;
    int* parent_out; int64_t* token_out; int64_t* feed_out; float* cum_out; float* step_lp_out; float* g_out;   /* [groups * B] each */
    float* kappa_out;                          /* [groups], optional */
} cover_beam_merge_gumbel_args;
int cover_beam_merge_gumbel(const cover_beam_merge_gumbel_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Composite forwards: the per-layer Python loops of the reference (18-layer loop in
 * paligemma_with_expert.py:258-349, HF/timm encoder loops) run here in C++ so that a whole tower / prefill /
 * decode step is one call (and one hipGraph when captured). Weight tables are plain HOST arrays of device
 * pointers filled by the Python host.
 * ------------------------------------------------------------------------------------------------ */
typedef struct cover_workspace { void* ptr; size_t bytes; } cover_workspace;

typedef struct cover_vit_layer {
    const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    const void* qkv_w; const float* qkv_b;   /* packed [3*H*Dp, dim] */
    const void* proj_w; const float* proj_b; /* packed [dim, H*Dp] */
    const void* fc1_w; const float* fc1_b;   /* packed [mlp_p, dim] */
    const void* fc2_w; const float* fc2_b;   /* packed [dim, mlp_p] */
    const float *ls1, *ls2;                  /* LayerScale or NULL */
} cover_vit_layer;
typedef struct cover_vit_desc {
    int dim, heads, head_dim_p, mlp_p, n_layers, act; /* head_dim_p / mlp_p = zero-padded sizes (72->96, 4304->4352) */
    float ln_eps, attn_scale;                         /* attn_scale = TRUE head_dim ** -0.5 */
    const cover_vit_layer* layers_host;               /* HOST array [n_layers] */
    int last_attn_only; /* 1: the LAST listed block stops after its attention out-projection and that (pre-residual)
                           tensor is written to attn_out: the forward-hook feature of
                           finetune_trajectory_bridge_ddp.py:272-274 */
    int _pad;
} cover_vit_desc;
/* x: bf16 [n_seq*T, dim] token embeddings, updated in place through the blocks; attn_out bf16 [n_seq*T, dim]
 * (only with last_attn_only). */
size_t cover_vit_workspace_bytes(const cover_vit_desc* d, int n_seq, int T);
int cover_vit_forward(const cover_vit_desc* d, void* x, int n_seq, int T, void* attn_out, cover_workspace ws,
                      int gemm_variant, void* stream);

typedef struct cover_dec_layer {
    const float* in_norm_w; const float* post_norm_w;
    const void* qkv_w; const float* qkv_b;   /* packed [(Hq+2Hkv)*D, dim] */
    const void* o_w;                          /* packed [dim, Hq*D] */
    const void* gate_up_w;                    /* packed, glu-interleaved [2*mlp, dim] */
    const void* down_w;                       /* packed [dim, mlp] */
    void* k_cache; void* vt_cache;            /* this layer's cache bases (bf16) */
    /* optional e4m3 twins (cover_pack_weight_fp8) + packed-order scales of the four projections; NULL = bf16 only */
    const void* qkv_w8; const float* qkv_s; const void* o_w8; const float* o_s;
    const void* gate_up_w8; const float* gate_up_s; const void* down_w8; const float* down_s;
    int down_klinear;                         /* 1: down_w8 is the k-linear image (cover_pack_weight_fp8_klinear): MX block-scaled down_proj input */
    int o_klinear;                            /* the same for o_w8: MX block-scaled attention output */
} cover_dec_layer;
typedef struct cover_dec_desc {
    int dim, Hq, Hkv, D, mlp, n_layers, act;  /* act: COVER_ACT_GELU_TANH (Gemma) / COVER_ACT_SILU (Llama) */
    int norm_style;                           /* cover_rmsnorm_bf16 style */
    float norm_eps, norm_w_offset, attn_scale;
    int rope_mode; int n_pos; int _pad;
    const float* cos_table; const float* sin_table;
    const float* final_norm_w;
    const cover_dec_layer* layers_host;       /* HOST array [n_layers] */
} cover_dec_desc;
/* A pass pushes up to two GROUPS of rows through all layers with ONE read of the weights. Group g holds
 * B x T new tokens laid out [b][t]; rows of group 1 follow group 0 in x. Per layer, each group's K/V are
 * appended to segment `write_seg` of the layer cache (slot = write_slot_of_batch[b] or b,
 * t = write_t_offset (+ write_t_offset_of_batch[b]) + t) and its queries attend its `segs` in order.
 * The k/vt pointers inside `segs` are IGNORED: per layer they are layer.k_cache + seg_k_offset[i] /
 * layer.vt_cache + seg_vt_offset[i] (element offsets), so one description serves every layer.
 * pi0 denoise steps attend their own suffix K/V without keeping it (paligemma_with_expert.py:305-308): give
 * them a scratch segment that the next step overwrites. */
typedef struct cover_dec_group {
    int B, T;
    const int* positions;  /* [B*T] */
    int n_seg; int write_seg;
    cover_kv_segment segs[3];
    long long seg_k_offset[3], seg_vt_offset[3];
    const int* write_slot_of_batch; const int* write_t_offset_of_batch;
    int write_t_offset;
    int seg0_shared;   /* 1: segs[0] is the SAME slot and length for every batch row and T == 1 (decode): it is attended
                          with the batch rows as query rows of one tile (K/V read once per 16 candidates) and chained into
                          the per-row segments through the attention state */
    /* Large-N candidate decode (T == 1, n_seg == 3, write_seg == 2, seg0_shared): own_kv_mode 1 / 2 keeps the write segment in the
     * head-major layout of cover_decode_own_attention (1: bf16, 2: e4m3 + row scales stored behind the data in the region's
     * second half: own_region_elems = slots * cap * Hkv * D of that region) and runs   own-token pass (VALU)  ->  ONE MFMA pass over
     * [segs[0] | segs[1]] with the candidates of a prompt as the query rows of a batch entry. That needs the regular structure
     * the sampler has: rows [i * seg1_group, (i + 1) * seg1_group) share segs[1]'s slot seg1_slot_of_group[i] (NULL: i) and length
     * seg1_len_of_group[i] (NULL: segs[1].len). The mode is a property of the cache, not of a step: use it for every pass. */
    int own_kv_mode; int seg1_group;
    const int* seg1_slot_of_group; const int* seg1_len_of_group;
    long long own_region_elems;
} cover_dec_group;
typedef struct cover_dec_pass {
    int n_groups; int final_norm;      /* final_norm: apply final_norm_w to x at the end */
    const float* x_f32;                /* optional fp32 [rows, dim] layer-0 input (norm input AND first residual) */
    cover_dec_group groups[2];
} cover_dec_pass;
size_t cover_decoder_workspace_bytes(const cover_dec_desc* d, int rows);
/* x: bf16 [rows, dim] input embeddings, overwritten with the output hidden states */
int cover_decoder_forward(const cover_dec_desc* d, const cover_dec_pass* p, void* x, cover_workspace ws,
                          int gemm_variant, void* stream);

/* hipGraph capture helpers: everything launched on `stream` between begin/end becomes one replayable graph */
int cover_graph_begin(void* stream);
int cover_graph_end(void* stream, void** graph_exec_out);
int cover_graph_launch(void* graph_exec, void* stream);
int cover_graph_destroy(void* graph_exec);

/* Timing on the stream the kernels run on (torch.cuda.Event only sees torch's current stream): opaque hipEvent
 * pairs. cover_timer_stop synchronises the stop event and returns elapsed milliseconds. */
int cover_timer_create(void** timer_out);
int cover_timer_start(void* timer, void* stream);
int cover_timer_stop(void* timer, void* stream, float* ms_out);
int cover_timer_destroy(void* timer);
int cover_stream_sync(void* stream);

/* ---- image resampling on the device (the pre-processing either side of the hot path; cover_vla_amd/imaging.py builds the
 * span tables with the restated filter-bank code) --------------------------------------------------------------------------
 * cover_resample_axis: one separable pass along H (axis 0) or W (axis 1) of an HWC image:
 *   out[o] = sum_{j < bounds[2o+1]} coefs[o*ksize + j] * in[bounds[2o] + j].
 *   fixed_point = 1: Pillow's 8-bit path (int32 coefficients with 22 fractional bits, accumulator seeded with 1 << 21,
 *   clip8(ss >> 22); uint8 -> uint8) = torchvision Resize on a PIL image = open_clip's SigLIP2 preprocess, replaces the
 *   `self.preprocess(image)` call of bridge_verifier/ensemble_eval/efficient_ensemble_merged.py:338.
 *   fixed_point = 0: TensorFlow ScaleAndTranslate float path (fp32 coefficients, sequential accumulation; a uint8 output is
 *   the truncating cast) = tf.image.resize(bilinear, antialias=True) of process_raw_image_to_jpg,
 *   CoVer_VLA/inference/experiments/robot/simpler/eval_utils.py:273-283.
 * cover_u8_hwc_to_f32_chw_norm: ToTensor + Normalize, ((x / 255) - mean) / std, HWC uint8 -> CHW fp32.
 * cover_resize_bilinear_pad_f32: F.interpolate(bilinear, align_corners=False) of an fp32 [NC, Hin, Win] stack to Hr x Wr,
 *   placed at (pad_top, pad_left) of an Hout x Wout canvas filled with pad_value = resize_with_pad,
 *   lerobot_custom/lerobot/common/policies/pi0/modeling_pi0.py:131-150. */
/* fixed_point = 2: OpenCV's 8-bit fixed-point resize arithmetic (imgproc resize.cpp; cv2.resize(..., INTER_LANCZOS4) of the policy-side
 *   adapter, INT-ACT/src/experiments/env_adapters/simpler.py:48-52): int32 coefficients holding shorts with 11 fractional bits;
 *   first pass uint8 -> int32 exact sums (out kind 2), second pass int32 (in kind 2) -> uint8 = saturate((sum + (1 << 21)) >> 22).
 *   The in / out kinds are 0 = uint8, 1 = fp32, 2 = int32 (this mode only).
 * cover_u8_hwc_to_f32_chw_scale_norm: ((float)x * scale - mean) / std, HWC uint8 -> CHW fp32: process_images of
 *   INT-ACT/src/utils/pipeline.py:55-67 (rescale by multiplication, then normalise). */
int cover_u8_hwc_to_f32_chw_scale_norm(const uint8_t* in, float* out, int H, int W, float scale, const float* mean3, const float* std3, void* stream);
int cover_resample_axis(const void* in, int in_is_f32, void* out, int out_is_f32, int Hin, int Win, int C, int Hout, int Wout,
                        int axis, const int* bounds, const void* coefs, int ksize, int fixed_point, void* stream);
int cover_u8_hwc_to_f32_chw_norm(const uint8_t* in, float* out, int H, int W, const float* mean3, const float* std3, void* stream);
int cover_resize_bilinear_pad_f32(const float* in, float* out, int NC, int Hin, int Win, int Hr, int Wr, int Hout, int Wout,
                                  int pad_top, int pad_left, float pad_value, void* stream);

/* Per-launch kernel timing for bench.py's roofline objects: between begin/end every GEMM / attention launch issued by
 * this library carries a hipEvent pair stamped with the kernel's own start / stop on its stream. Classes:
 *   0 weight-streaming GEMM with >= 16 MB of weights (work = weight bytes)   1 LDS-tiled GEMM, ViT-sized (work = FLOPs)
 *   2 attention (work = 0)   3 small weight-streaming GEMMs (work = weight bytes)
 *   4 LDS-tiled GEMM, LLM-sized (N*K >= 16 M; work = FLOPs)   5 split-K reductions behind a weight-streaming GEMM (work = 0)
 *   7 LDS-tiled GEMM on the MX-scaled fp8 matrix instruction (work = FLOPs; priced against the 5 PFLOP/s fp8 peak)
 *   6 / 8 / 9 split-K reductions behind a class-1 / class-4 / class-7 GEMM (work = 0): every reduction is charged to the GEMM class it completes
 * Thread-safe (records are claimed atomically). Launches replayed from a hipGraph are not seen (neither time nor work).
 * end_n() synchronises the device and fills ms[n], count[n], work[n] (n <= COVER_PROF_CLASSES); it returns
 * COVER_EWORKSPACE when more launches were issued than max_events (sums incomplete). end() = end_n(.., 4). */
#define COVER_PROF_CLASSES 10
int cover_profile_begin(int max_events);
int cover_profile_end(double* ms, long long* count, double* work);
int cover_profile_end_n(double* ms, long long* count, double* work, int n_classes);

/* sizeof() of every struct above by name ("cover_attn_args", ...): lets a foreign-language binding check its
 * mirrored layouts at load time. Returns 0 for unknown names. */
size_t cover_sizeof(const char* struct_name);

#ifdef __cplusplus
}
#endif
#endif
