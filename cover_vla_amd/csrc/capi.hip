// extern "C" surface of libcover_hip (include/cover_hip.h): thin wrappers over the launchers, graphs and timers. The composite tower / decoder
// forwards are in forward.hip. Host code only; kernels live in the sibling .hip files.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "kernels.h"

static thread_local std::string g_err;
int fail(int code, const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}
#define ST(s) ((hipStream_t)(s))

extern "C" {

int cover_abi_version(void) { return COVER_ABI_VERSION; }
const char* cover_last_error(void) { return g_err.c_str(); }

int cover_device_info(int dev, int* n_cu, size_t* total_mem, char* name, int name_len) {
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, dev), "hipGetDeviceProperties");
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (total_mem) *total_mem = p.totalGlobalMem;
    if (name && name_len > 0) {
        strncpy(name, p.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    return COVER_OK;
}

int cover_packed_k(int K) { return (K + 127) / 128 * 128; }
size_t cover_packed_weight_bytes(int N, int K) {
    return (size_t)((N + 15) / 16) * 16 * (size_t)cover_packed_k(K) * 2;
}
int cover_pack_weight_bf16(const void* W, int ldw, int N, int K, void* Wp, int glu, void* stream) {
    if (!W || !Wp || N <= 0 || K <= 0) return fail(COVER_EINVAL, "cover_pack_weight_bf16: bad arguments");
    if (glu && ((N / 2) % 16 != 0 || (N & 1))) return fail(COVER_EINVAL, "cover_pack_weight_bf16: glu needs N/2 % 16 == 0");
    HIPCHK(launch_pack_weight_bf16((const bf16_t*)W, ldw, N, K, (bf16_t*)Wp, cover_packed_k(K), glu, ST(stream)),
           "pack_weight");
    return COVER_OK;
}
size_t cover_packed_weight_fp8_bytes(int N, int K) { return (size_t)((N + 15) / 16) * 16 * (size_t)cover_packed_k(K); }
int cover_quantize_rows_fp8(const void* W, int ldw, int N, int K, float* scales, void* Wdq, void* stream) {
    if (!W || !scales || !Wdq || N <= 0 || K <= 0) return fail(COVER_EINVAL, "cover_quantize_rows_fp8: bad arguments");
    HIPCHK(launch_quantize_rows_fp8((const bf16_t*)W, ldw, N, K, scales, (bf16_t*)Wdq, ST(stream)), "quantize_rows_fp8");
    return COVER_OK;
}
int cover_pack_weight_fp8(const void* Wdq, int ldw, const float* scales, int N, int K, void* Wq, float* scales_packed, int glu,
                          void* stream) {
    if (!Wdq || !scales || !Wq || !scales_packed || N <= 0 || K <= 0) return fail(COVER_EINVAL, "cover_pack_weight_fp8: bad arguments");
    if (glu && ((N / 2) % 16 != 0 || (N & 1))) return fail(COVER_EINVAL, "cover_pack_weight_fp8: glu needs N/2 % 16 == 0");
    HIPCHK(launch_pack_weight_fp8((const bf16_t*)Wdq, ldw, scales, N, K, (uint8_t*)Wq, scales_packed, cover_packed_k(K), glu, ST(stream)),
           "pack_weight_fp8");
    return COVER_OK;
}
int cover_pack_weight_fp8_klinear(const void* Wdq, int ldw, const float* scales, int N, int K, void* Wq, float* scales_packed, void* stream) {
    if (!Wdq || !scales || !Wq || !scales_packed || N <= 0 || K <= 0) return fail(COVER_EINVAL, "cover_pack_weight_fp8_klinear: bad arguments");
    HIPCHK(launch_pack_weight_fp8((const bf16_t*)Wdq, ldw, scales, N, K, (uint8_t*)Wq, scales_packed, cover_packed_k(K), 0, ST(stream), 1),
           "pack_weight_fp8 (k-linear)");
    return COVER_OK;
}
int cover_quantize_act_fp8_mx(const void* X, int ldx, int M, int K, void* out8, int ld8, void* mx, void* stream) {
    if (!X || !out8 || !mx || M < 0 || K <= 0) return fail(COVER_EINVAL, "cover_quantize_act_fp8_mx: bad arguments");
    HIPCHK(launch_quantize_act_fp8_mx((const bf16_t*)X, ldx, M, K, (uint8_t*)out8, ld8, (uint8_t*)mx, ST(stream)),
           "quantize_act_fp8_mx (ld8 >= padded K, ld8 % 16 == 0, ldx % 8 == 0)");
    return COVER_OK;
}
int cover_quantize_act_fp8(const void* X, int ldx, int M, int K, void* out8, int ld8, float* scales, void* stream) {
    if (!X || !out8 || !scales || M < 0 || K <= 0) return fail(COVER_EINVAL, "cover_quantize_act_fp8: bad arguments");
    HIPCHK(launch_quantize_act_fp8((const bf16_t*)X, ldx, M, K, (uint8_t*)out8, ld8, scales, ST(stream)),
           "quantize_act_fp8 (ld8 >= padded K, ld8 % 16 == 0, ldx % 8 == 0)");
    return COVER_OK;
}
size_t cover_gemm_workspace_bytes(int M, int N, int K) { return gemm_workspace_bytes(M, N, K); }
int cover_gemm_probe(unsigned long long* out) {
    if (!out) return fail(COVER_EINVAL, "cover_gemm_probe: null pointer");
    if (gemm_v3_probe(out) != 0) return fail(COVER_EHIP, "cover_gemm_probe: could not read the probe words");
    return COVER_OK;
}
int cover_gemm_plan_counts(long long* counts, int n, int reset) {
    if (n < 0 || (n > 0 && !counts)) return fail(COVER_EINVAL, "cover_gemm_plan_counts: bad arguments");
    gemm_plan_counts(counts, n, reset);
    return COVER_GEMM_PLANS;
}
// cover_gemm_bf16's own argument checks (shared with cover_gemm_plan); nullptr when they pass
static const char* gemm_args_error(const void* A, int lda, const void* Wp, const void* C, int N, int K, const cover_gemm_epi* epi) {
    if (!A || !Wp || !C) return "cover_gemm_bf16: null pointer";
    if (lda % 8) return "cover_gemm_bf16: lda must be a multiple of 8 elements";
    if (lda < cover_packed_k(K)) return "cover_gemm_bf16: lda < padded K";
    if (epi && epi->glu && (N % 32)) return "cover_gemm_bf16: glu needs N % 32 == 0";
    return nullptr;
}
int cover_gemm_plan(const void* A, int lda, const void* Wp, void* C, int ldc, int M, int N, int K,
                    const cover_gemm_epi* epi, void* ws, size_t ws_bytes, int variant, int plan[6]) {
    if (!plan) return fail(COVER_EINVAL, "cover_gemm_plan: null plan");
    if (const char* why = gemm_args_error(A, lda, Wp, C, N, K, epi)) return fail(COVER_EINVAL, why);
    HIPCHK(gemm_plan_query((const bf16_t*)A, lda, (const bf16_t*)Wp, C, ldc, M, N, K, epi, (const float*)ws, ws_bytes, variant, plan), "gemm_plan");
    return COVER_OK;
}
int cover_gemm_bf16(const void* A, int lda, const void* Wp, void* C, int ldc, int M, int N, int K,
                    const cover_gemm_epi* epi, void* ws, size_t ws_bytes, int variant, void* stream) {
    if (const char* why = gemm_args_error(A, lda, Wp, C, N, K, epi)) return fail(COVER_EINVAL, why);
    HIPCHK(launch_gemm_bf16((const bf16_t*)A, lda, (const bf16_t*)Wp, C, ldc, M, N, K, epi, (float*)ws, ws_bytes, variant,
                            ST(stream)),
           "gemm_bf16");
    return COVER_OK;
}

int cover_attention_bf16(const cover_attn_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_attention_bf16: null args");
    HIPCHK(launch_attention_bf16(a, ST(stream)), "attention_bf16 (D must be 64/96/128/256, 1..3 segments)");
    return COVER_OK;
}

int cover_attention_plan(const cover_attn_args* a, int* plan) {
    if (!a || !plan) return fail(COVER_EINVAL, "cover_attention_plan: null pointer");
    HIPCHK(attention_plan(a, plan), "attention_bf16 (D must be 64/96/128/256, 1..3 segments)");
    return COVER_OK;
}
int cover_attention_bf16_pair(const cover_attn_args* a0, const cover_attn_args* a1, void* stream) {
    if (!a0 || !a1) return fail(COVER_EINVAL, "cover_attention_bf16_pair: null args");
    HIPCHK(launch_attention_bf16_pair(a0, a1, ST(stream)), "attention_bf16_pair (D must be 64/96/128/256, 1..3 segments)");
    return COVER_OK;
}
int cover_attention_pair_plan(const cover_attn_args* a0, const cover_attn_args* a1, int* dual) {
    if (!a0 || !a1 || !dual) return fail(COVER_EINVAL, "cover_attention_pair_plan: null pointer");
    HIPCHK(attention_pair_plan(a0, a1, dual), "attention_bf16_pair (D must be 64/96/128/256, 1..3 segments)");
    return COVER_OK;
}
int cover_decode_attention_fused(const cover_decode_attn_args* a, void* stream) {
    if (!a || !a->out || (a->n_splits <= 0 && !a->qkv) || (a->n_splits > 0 && !a->partial))
        return fail(COVER_EINVAL, "cover_decode_attention_fused: null pointer");
    HIPCHK(launch_decode_attention_fused(a, ST(stream)), "decode_attention_fused (D in {64,128}, COVER_MASK_LEN segments, 0 <= write_t < seg[2].len)");
    return COVER_OK;
}

int cover_decode_own_attention(const cover_own_attn_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_decode_own_attention: null args");
    HIPCHK(launch_decode_own_attention(a, ST(stream)), "decode_own_attention (D in {64,128}, 0 <= write_t < t_cap, at most 16 loads per lane per pass)");
    return COVER_OK;
}

int cover_layernorm_bf16(const void* x, int ldx, const float* w, const float* b, void* y, int ldy, int rows, int dim,
                         float eps, void* stream) {
    HIPCHK(launch_layernorm_bf16((const bf16_t*)x, ldx, w, b, (bf16_t*)y, ldy, rows, dim, eps, ST(stream)), "layernorm_bf16");
    return COVER_OK;
}
int cover_rmsnorm_bf16(const void* x, int x_f32, int ldx, const float* w, float w_offset, int style, void* y, int ldy,
                       int rows, int dim, float eps, void* stream) {
    HIPCHK(launch_rmsnorm(x, x_f32, ldx, w, w_offset, style, (bf16_t*)y, ldy, rows, dim, eps, ST(stream)), "rmsnorm_bf16");
    return COVER_OK;
}
int cover_rmsnorm_bf16_q8(const void* x, int x_f32, int ldx, const float* w, float w_offset, int style, void* y, int ldy,
                          int rows, int dim, float eps, void* q8, int ld8, float* q8s, void* stream) {
    if (!q8 || !q8s) return fail(COVER_EINVAL, "cover_rmsnorm_bf16_q8: null q8 / q8s");
    HIPCHK(launch_rmsnorm(x, x_f32, ldx, w, w_offset, style, (bf16_t*)y, ldy, rows, dim, eps, ST(stream), (uint8_t*)q8, ld8, q8s), "rmsnorm_bf16_q8");
    return COVER_OK;
}
int cover_rope_kv_write(const cover_rope_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_rope_kv_write: null args");
    HIPCHK(launch_rope_kv_write(a, ST(stream)), "rope_kv_write");
    return COVER_OK;
}
int cover_rope_kv_write_pair(const cover_rope_args* a0, const cover_rope_args* a1, void* stream) {
    if (!a0 || !a1) return fail(COVER_EINVAL, "cover_rope_kv_write_pair: null args");
    HIPCHK(launch_rope_kv_write_pair(a0, a1, ST(stream)), "rope_kv_write_pair");
    return COVER_OK;
}
int cover_embed_gather(const void* table, int dim, const int64_t* ids, int n, float scale, void* out, int ldo,
                       void* stream) {
    HIPCHK(launch_embed_gather((const bf16_t*)table, dim, ids, n, scale, (bf16_t*)out, ldo, ST(stream)), "embed_gather");
    return COVER_OK;
}
int cover_patchify(const cover_patchify_args* a, void* stream) {
    if (!a || a->patch <= 0 || a->H % a->patch || a->W % a->patch || a->ld_out < 3 * a->patch * a->patch)
        return fail(COVER_EINVAL, "cover_patchify: bad geometry");
    HIPCHK(launch_patchify(a, ST(stream)), "patchify");
    return COVER_OK;
}
int cover_copy_rows_bf16(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, const int* sidx,
                         const int* didx, void* stream) {
    HIPCHK(launch_copy_rows_bf16((const bf16_t*)src, ld_src, (bf16_t*)dst, ld_dst, rows, cols, sidx, didx, ST(stream)),
           "copy_rows");
    return COVER_OK;
}
int cover_add_rows_bf16(void* x, int ldx, const void* add, int ld_add, int rows, int cols, int add_rows, void* stream) {
    if (add_rows <= 0) return fail(COVER_EINVAL, "cover_add_rows_bf16: add_rows <= 0");
    HIPCHK(launch_add_bias_rows_bf16((bf16_t*)x, ldx, (const bf16_t*)add, ld_add, rows, cols, add_rows, ST(stream)), "add_rows");
    return COVER_OK;
}
int cover_scale_bf16(void* x, int ldx, int rows, int cols, float pre_div, float post_mul, void* stream) {
    HIPCHK(launch_scale_bf16((bf16_t*)x, ldx, rows, cols, pre_div, post_mul, ST(stream)), "scale_bf16");
    return COVER_OK;
}
int cover_cast_f32_to_bf16(const float* x, int ldx, void* y, int ldy, int rows, int cols, void* stream) {
    HIPCHK(launch_cast_f32_to_bf16(x, ldx, (bf16_t*)y, ldy, rows, cols, ST(stream)), "cast_f32_to_bf16");
    return COVER_OK;
}
int cover_cast_bf16_to_f32(const void* x, int ldx, float* y, int ldy, int rows, int cols, void* stream) {
    HIPCHK(launch_cast_bf16_to_f32((const bf16_t*)x, ldx, y, ldy, rows, cols, ST(stream)), "cast_bf16_to_f32");
    return COVER_OK;
}

int cover_gemm_f32(const cover_gemm_f32_args* a, void* stream) {
    if (!a || !a->A || !a->B || !a->C) return fail(COVER_EINVAL, "cover_gemm_f32: null pointer");
    HIPCHK(launch_gemm_f32(a, ST(stream)), "gemm_f32");
    return COVER_OK;
}
int cover_gemm_f32_plan(const cover_gemm_f32_args* a, int* plan) {
    if (!a || !plan) return fail(COVER_EINVAL, "cover_gemm_f32_plan: null pointer");
    if (!a->A || !a->B || !a->C) return fail(COVER_EINVAL, "cover_gemm_f32: null pointer");
    int deep = 0;
    plan[0] = (a->M <= 0 || a->N <= 0) ? -1 : gemm_f32_plan(a, &deep);
    plan[1] = deep;
    return COVER_OK;
}
int cover_layernorm_f32(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int rows, int dim,
                        float eps, void* stream) {
    HIPCHK(launch_layernorm_f32(x, ldx, w, b, y, ldy, rows, dim, eps, ST(stream)), "layernorm_f32");
    return COVER_OK;
}
int cover_layernorm_f32_grouped(const float* x, int ldx, const float* w, const float* b, float* y, int ldy, int rows, int dim,
                                float eps, int rows_per_group, long long wb_group_stride, void* stream) {
    if (rows_per_group <= 0) return fail(COVER_EINVAL, "cover_layernorm_f32_grouped: rows_per_group");
    HIPCHK(launch_layernorm_f32(x, ldx, w, b, y, ldy, rows, dim, eps, ST(stream), rows_per_group, wb_group_stride), "layernorm_f32_grouped");
    return COVER_OK;
}
int cover_softmax_rows_f32(float* x, int ldx, int rows, int cols, float scale, void* stream) {
    HIPCHK(launch_softmax_rows_f32(x, ldx, rows, cols, scale, ST(stream)), "softmax_rows_f32");
    return COVER_OK;
}
int cover_l2norm_rows_f32(const float* x, int ldx, float* y, int ldy, int rows, int cols, void* stream) {
    HIPCHK(launch_l2norm_rows_f32(x, ldx, y, ldy, rows, cols, ST(stream)), "l2norm_rows_f32");
    return COVER_OK;
}
int cover_add_f32(const float* a, int lda, const float* b, int ldb, float* y, int ldy, int rows, int cols, int b_rows,
                  void* stream) {
    if (b_rows <= 0) return fail(COVER_EINVAL, "cover_add_f32: b_rows <= 0");
    HIPCHK(launch_add_f32(a, lda, b, ldb, y, ldy, rows, cols, b_rows, ST(stream)), "add_f32");
    return COVER_OK;
}
int cover_xent_diag_f32(const float* logits, int ld, int rows, int cols, float* loss, int* rank, void* stream) {
    if (!logits || !loss || !rank) return fail(COVER_EINVAL, "cover_xent_diag_f32: null pointer");
    if (rows > cols) return fail(COVER_EINVAL, "cover_xent_diag_f32: row r is labelled r, so rows <= cols");
    HIPCHK(launch_xent_diag_f32(logits, ld, rows, cols, loss, rank, ST(stream)), "xent_diag_f32");
    return COVER_OK;
}
int cover_act_f32(const float* x, int ldx, float* y, int ldy, int rows, int cols, int act, void* stream) {
    if (!x || !y) return fail(COVER_EINVAL, "cover_act_f32: null pointer");
    HIPCHK(launch_act_f32(x, ldx, y, ldy, rows, cols, act, ST(stream)), "act_f32");
    return COVER_OK;
}
int cover_mha_f32(const cover_mha_f32_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_mha_f32: null args");
    HIPCHK(launch_mha_f32(a, ST(stream)), "mha_f32 (Tq*Tk <= 8192)");
    return COVER_OK;
}
int cover_masked_mean_f32(const float* x, const uint8_t* pad, float* y, int B, int T, int D, void* stream) {
    HIPCHK(launch_masked_mean_f32(x, pad, y, B, T, D, ST(stream)), "masked_mean_f32");
    return COVER_OK;
}
int cover_sincos_time_embed(const float* time, int B, int dim, double min_period, double max_period, void* out, int ldo,
                            void* stream) {
    if (dim % 2) return fail(COVER_EINVAL, "cover_sincos_time_embed: dimension must be divisible by 2");
    HIPCHK(launch_sincos_time_embed(time, B, dim, min_period, max_period, (bf16_t*)out, ldo, ST(stream)), "sincos_time_embed");
    return COVER_OK;
}

int cover_token_select(const cover_token_select_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_select: null args");
    HIPCHK(launch_token_select(a, ST(stream)), "token_select (sampling width <= 4096, temperature > 0)");
    return COVER_OK;
}
int cover_token_sample(const cover_token_sample_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_sample: null args");
    HIPCHK(launch_token_sample(a, ST(stream)),
           "token_sample (uniform required, temperature > 0, top_p > 0, top_k >= 0, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_sample_scored(const cover_token_sample_scored_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_sample_scored: null args");
    HIPCHK(launch_token_sample_scored(a, ST(stream)),
           "token_sample_scored (uniform and logprob_out required, temperature > 0, top_p > 0, top_k >= 0, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_logprob(const cover_token_logprob_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_logprob: null args");
    HIPCHK(launch_token_logprob(a, ST(stream)),
           "token_logprob (token and logprob_out required, temperature > 0, top_p > 0, top_k >= 0, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_topn(const cover_token_topn_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_topn: null args");
    HIPCHK(launch_token_topn(a, ST(stream)),
           "token_topn (token_out and logprob_out required, 1 <= n <= 64, ld_tok >= n, ld_lp >= n, temperature > 0, top_p > 0, top_k >= 0, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_sample_rows(const cover_token_sample_rows_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_sample_rows: null args");
    HIPCHK(launch_token_sample_rows(a, ST(stream)), "token_sample_rows (uniform, temperature and token_out required, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_logprob_rows(const cover_token_logprob_rows_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_logprob_rows: null args");
    HIPCHK(launch_token_logprob_rows(a, ST(stream)), "token_logprob_rows (temperature, token and logprob_out required, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_topn_rows(const cover_token_topn_rows_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_topn_rows: null args");
    HIPCHK(launch_token_topn_rows(a, ST(stream)),
           "token_topn_rows (temperature, token_out and logprob_out required, 1 <= n <= 64, ld_tok >= n, ld_lp >= n, 0 < hi - lo <= 2^20)");
    return COVER_OK;
}
int cover_token_sample_rows_allowed(const cover_token_sample_rows_args* a, const cover_token_allow* al, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_sample_rows_allowed: null args");
    HIPCHK(launch_token_sample_rows_allowed(a, al, ST(stream)),
           "token_sample_rows_allowed (as token_sample_rows; allow and bits required, bits 4-byte aligned, n_sets >= 1, ld_words >= ceil(hi / 32))");
    return COVER_OK;
}
int cover_token_logprob_rows_allowed(const cover_token_logprob_rows_args* a, const cover_token_allow* al, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_logprob_rows_allowed: null args");
    HIPCHK(launch_token_logprob_rows_allowed(a, al, ST(stream)),
           "token_logprob_rows_allowed (as token_logprob_rows; allow and bits required, bits 4-byte aligned, n_sets >= 1, ld_words >= ceil(hi / 32))");
    return COVER_OK;
}
int cover_token_topn_rows_allowed(const cover_token_topn_rows_args* a, const cover_token_allow* al, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_topn_rows_allowed: null args");
    HIPCHK(launch_token_topn_rows_allowed(a, al, ST(stream)),
           "token_topn_rows_allowed (as token_topn_rows; allow and bits required, bits 4-byte aligned, n_sets >= 1, ld_words >= ceil(hi / 32))");
    return COVER_OK;
}
int cover_token_sample_rows_ref(const cover_token_sample_rows_args* a, const cover_token_allow* al, const cover_token_ref* ref, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_token_sample_rows_ref: null args");
    HIPCHK(launch_token_sample_rows_ref(a, al, ref, ST(stream)),
           "token_sample_rows_ref (as token_sample_rows, with allow as token_sample_rows_allowed; ref and ref->logprob_out required, ref->temperature > 0 and finite)");
    return COVER_OK;
}
int cover_decode_feedback_lp2(const cover_decode_feedback_args* a, const float* lp2, float* lp2_out, long long ld_lp2, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_decode_feedback_lp2: null args");
    HIPCHK(launch_decode_feedback_lp2(a, lp2, lp2_out, ld_lp2, ST(stream)), "decode_feedback_lp2 (as decode_feedback; lp2 and lp2_out required)");
    return COVER_OK;
}
int cover_decode_feedback_fsm(const cover_decode_feedback_args* a, const cover_token_fsm* fsm, const float* lp2, float* lp2_out, long long ld_lp2,
                              void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_decode_feedback_fsm: null args");
    HIPCHK(launch_decode_feedback_fsm(a, fsm, lp2, lp2_out, ld_lp2, ST(stream)),
           "decode_feedback_fsm (as decode_feedback; fsm and every member required, n_states >= 1, 1 <= n_classes <= 256, vocab > 0, lp2 and lp2_out together)");
    return COVER_OK;
}
int cover_decode_feedback(const cover_decode_feedback_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_decode_feedback: null args");
    HIPCHK(launch_decode_feedback(a, ST(stream)),
           "decode_feedback (pick, done and tok_out required, lp and lp_out together, x_out needs a 16-byte aligned table, dim % 8 == 0, ldo % 8 == 0, vocab > 0)");
    return COVER_OK;
}
int cover_score_select(const cover_score_select_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_score_select: null args");
    HIPCHK(launch_score_select(a, ST(stream)), "score_select (N % group_size == 0, fused_*_out required)");
    return COVER_OK;
}
int cover_tokens_to_histories(const int64_t* tokens, int ld_tokens, int N, int tok_vocab, const float* centers, int n_centers,
                              const float* past, int n_past, float pad_value, float* hist_out, uint8_t* pad_out, void* stream) {
    if (!tokens || !centers || !hist_out || !pad_out || (n_past > 0 && !past)) return fail(COVER_EINVAL, "cover_tokens_to_histories: null pointer");
    HIPCHK(launch_tokens_to_histories(tokens, ld_tokens, N, tok_vocab, centers, n_centers, past, n_past, pad_value, hist_out, pad_out, ST(stream)),
           "tokens_to_histories (0 <= n_past <= 9)");
    return COVER_OK;
}
int cover_tokens_to_histories_steps(const int64_t* tokens, int ld_tokens, int N, int tok_vocab, const float* centers, int n_centers,
                                    const float* past, int n_past, int n_use, float pad_value, float* hist_out, uint8_t* pad_out, void* stream) {
    if (!tokens || !centers || !hist_out || !pad_out || (n_past > 0 && !past)) return fail(COVER_EINVAL, "cover_tokens_to_histories_steps: null pointer");
    HIPCHK(launch_tokens_to_histories(tokens, ld_tokens, N, tok_vocab, centers, n_centers, past, n_past, pad_value, hist_out, pad_out, ST(stream), n_use),
           "tokens_to_histories_steps (n_use >= 1, n_past + n_use <= 10, ld_tokens >= 7 n_use)");
    return COVER_OK;
}
int cover_actions_to_histories(const float* actions, long long n_stride, long long t_stride, int N, int n_use, const float* lo_hi,
                               const float* past, int n_past, float pad_value, float* hist_out, uint8_t* pad_out, void* stream) {
    if (!actions || !hist_out || !pad_out || (n_past > 0 && !past)) return fail(COVER_EINVAL, "cover_actions_to_histories: null pointer");
    HIPCHK(launch_actions_to_histories(actions, n_stride, t_stride, N, n_use, lo_hi, past, n_past, pad_value, hist_out, pad_out, ST(stream)),
           "actions_to_histories (n_use >= 1, n_past + n_use <= 10)");
    return COVER_OK;
}
int cover_group_argmax(const float* scores, int N, int group_size, int* result_out, float* best_out, void* stream) {
    HIPCHK(launch_group_argmax(scores, N, group_size, result_out, best_out, ST(stream)), "group_argmax");
    return COVER_OK;
}
int cover_prior_select(const cover_prior_select_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_prior_select: null args");
    HIPCHK(launch_prior_select(a, ST(stream)),
           "prior_select (N % group_size == 0, N / group_size <= 4096, group_size <= 4096, 1 <= steps <= 4096, 0 <= top_m <= min(group_size, 64), "
           "beta finite and >= 0, scores / logprobs / prior_out / combined_out / result_out / best_out required, ranked_out with top_m > 0)");
    return COVER_OK;
}
int cover_member_scores(const cover_member_scores_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_member_scores: null args");
    HIPCHK(launch_member_scores(a, ST(stream)),
           "member_scores (1 <= n_members <= 16, N % group_size == 0, N / group_size <= 4096, 1 <= dim <= 4096, kappa finite and >= 0, "
           "mode 0 (lcb) or 1 (min, with kappa == 0), every pointer required)");
    return COVER_OK;
}
#define AUGMENT_LIMITS "G >= 1, 1 <= n <= 4096, 0 <= K <= 4096, 1 <= h <= 64, G * (n + K) <= 2^20, sigma and sd_floor finite and >= 0, " \
                       "clip_lo <= clip_hi, src / out required, normals with K > 0"
int cover_augment_tokens(const cover_augment_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_augment_tokens: null args");
    HIPCHK(launch_augment_tokens(a, ST(stream)), "augment_tokens (" AUGMENT_LIMITS ", n_stride >= 7 h, centers required, n_centers >= 1)");
    return COVER_OK;
}
int cover_augment_actions(const cover_augment_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_augment_actions: null args");
    HIPCHK(launch_augment_actions(a, ST(stream)), "augment_actions (" AUGMENT_LIMITS ")");
    return COVER_OK;
}
#define PROPOSAL_PRIOR_LIMITS "G >= 1, 1 <= n_fit <= group_rows <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, sigma and sd_floor finite " \
                              "and > 0 with an fp32 product > 0, src / prior_out required"
int cover_proposal_prior_tokens(const cover_proposal_prior_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_proposal_prior_tokens: null args");
    HIPCHK(launch_proposal_prior_tokens(a, ST(stream)), "proposal_prior_tokens (" PROPOSAL_PRIOR_LIMITS ", n_stride >= 7 h, centers required, n_centers >= 1)");
    return COVER_OK;
}
int cover_proposal_prior_actions(const cover_proposal_prior_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_proposal_prior_actions: null args");
    HIPCHK(launch_proposal_prior_actions(a, ST(stream)), "proposal_prior_actions (" PROPOSAL_PRIOR_LIMITS ")");
    return COVER_OK;
}
#define REFINE_LIMITS "G >= 1, 1 <= n_elite <= group_rows <= 4096, 0 <= K <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, " \
                      "G * (n_elite + K) <= 2^20, sigma and sd_floor finite and >= 0, clip_lo <= clip_hi, src / scores / out required, " \
                      "normals with K > 0"
int cover_refine_tokens(const cover_refine_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_refine_tokens: null args");
    HIPCHK(launch_refine_tokens(a, ST(stream)), "refine_tokens (" REFINE_LIMITS ", n_stride >= 7 h, centers required, n_centers >= 1)");
    return COVER_OK;
}
int cover_refine_actions(const cover_refine_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_refine_actions: null args");
    HIPCHK(launch_refine_actions(a, ST(stream)), "refine_actions (" REFINE_LIMITS ")");
    return COVER_OK;
}
#define SMOOTH_LIMITS "G >= 1, 1 <= group_rows <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, radius2 finite and > 0, shrink finite and " \
                      ">= 0, src / scores / dim_scale / smoothed_out required"
int cover_smooth_scores_tokens(const cover_smooth_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_smooth_scores_tokens: null args");
    HIPCHK(launch_smooth_scores_tokens(a, ST(stream)), "smooth_scores_tokens (" SMOOTH_LIMITS ", n_stride >= 7 h, centers required, n_centers >= 1)");
    return COVER_OK;
}
int cover_smooth_scores_actions(const cover_smooth_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_smooth_scores_actions: null args");
    HIPCHK(launch_smooth_scores_actions(a, ST(stream)), "smooth_scores_actions (" SMOOTH_LIMITS ")");
    return COVER_OK;
}
#define COHERENCE_LIMITS "G >= 1, 1 <= group_rows <= 4096, 1 <= R <= 4096, 1 <= h <= 64, 1 <= hr <= 64, 0 <= shift < hr, G * group_rows <= 2^20, " \
                         "ref_g_stride 0 or >= (R - 1) * ref_r_stride + 7 hr, ref_r_stride >= 7 hr, w_g_stride 0 or R, gripper_penalty finite " \
                         "and >= 0, src / ref / ref_weight / step_weight / dim_scale / prior_out required"
int cover_coherence_prior_tokens(const cover_coherence_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_coherence_prior_tokens: null args");
    HIPCHK(launch_coherence_prior_tokens(a, ST(stream)), "coherence_prior_tokens (" COHERENCE_LIMITS ", n_stride >= 7 h, centers required, n_centers >= 1)");
    return COVER_OK;
}
int cover_coherence_prior_actions(const cover_coherence_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_coherence_prior_actions: null args");
    HIPCHK(launch_coherence_prior_actions(a, ST(stream)), "coherence_prior_actions (" COHERENCE_LIMITS ")");
    return COVER_OK;
}
#define DIVERSE_LIMITS "G >= 1, 1 <= m <= group_rows <= 4096, 1 <= h <= 64, G * group_rows <= 2^20, weight finite and >= 0, cover_dist not " \
                       "NaN and < +inf, gripper_penalty finite and >= 0, src / step_weight / dim_scale / picked_rows_out required"
int cover_diverse_subset_tokens(const cover_diverse_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_diverse_subset_tokens: null args");
    HIPCHK(launch_diverse_subset_tokens(a, ST(stream)), "diverse_subset_tokens (" DIVERSE_LIMITS ", n_stride >= 7 h, centers required, n_centers >= 1)");
    return COVER_OK;
}
int cover_diverse_subset_actions(const cover_diverse_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_diverse_subset_actions: null args");
    HIPCHK(launch_diverse_subset_actions(a, ST(stream)), "diverse_subset_actions (" DIVERSE_LIMITS ")");
    return COVER_OK;
}
int cover_fast_decode(const cover_fast_decode_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_fast_decode: null args");
    HIPCHK(launch_fast_decode(a, ST(stream)),
           "fast_decode (1 <= B <= 2^20, 1 <= L <= 4096, 1 <= H <= 128, 1 <= D <= 32, n_pieces >= 1, 0 <= band_lo <= band_hi, 0 <= n_stop <= 4, "
           "0 <= n_skip <= 8, |min_token| <= 2^30, scale finite and != 0, relaxed 0 or 1, token strides >= 0, out_t_stride >= D, "
           "out_n_stride >= (H - 1) * out_t_stride + D, tokens / piece_off / piece_sym / basis / out required)");
    return COVER_OK;
}

int cover_beam_merge(const cover_beam_merge_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_beam_merge: null args");
    HIPCHK(launch_beam_merge(a, ST(stream)),
           "beam_merge (groups >= 0, 1 <= B <= 64, ld_tok >= B, ld_lp >= B, feed_pad >= 0, every pointer required, cum_out != cum)");
    return COVER_OK;
}
int cover_beam_merge_gumbel(const cover_beam_merge_gumbel_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_beam_merge_gumbel: null args");
    HIPCHK(launch_beam_merge_gumbel(a, ST(stream)),
           "beam_merge_gumbel (groups >= 0, 1 <= B <= 64, ld_tok >= B, ld_lp >= B, ld_g >= B, feed_pad >= 0, every pointer but kappa_out required, "
           "cum_out != cum)");
    return COVER_OK;
}
int cover_gumbel_topn(const cover_gumbel_topn_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_gumbel_topn: null args");
    HIPCHK(launch_gumbel_topn(a, ST(stream)),
           "gumbel_topn (every pointer required, 0 <= lo < hi, hi - lo <= 4096, temperature > 0, 1 <= n <= 64, ld_u >= hi - lo, ld_tok / ld_lp / ld_g >= n)");
    return COVER_OK;
}
int cover_kv_gather_slots(const cover_kv_gather_slots_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_kv_gather_slots: null args");
    HIPCHK(launch_kv_gather_slots(a, ST(stream)),
           "kv_gather_slots (tables and slot arrays required, 1 <= n_layers <= 65535, n_slots >= 1, cap and Hkv * D multiples of 8, "
           "Hkv * D * cap < 2^31, 0 <= n_t <= cap, offsets >= 0, offsets and slot strides multiples of 8, slot strides >= Hkv * D * cap)");
    return COVER_OK;
}
int cover_beam_backtrack(const cover_beam_backtrack_args* a, void* stream) {
    if (!a) return fail(COVER_EINVAL, "cover_beam_backtrack: null args");
    HIPCHK(launch_beam_backtrack(a, ST(stream)), "beam_backtrack (every pointer required, steps >= 1, B >= 1, rows >= 0, rows % B == 0)");
    return COVER_OK;
}

int cover_resample_axis(const void* in, int in_is_f32, void* out, int out_is_f32, int Hin, int Win, int C, int Hout, int Wout,
                        int axis, const int* bounds, const void* coefs, int ksize, int fixed_point, void* stream) {
    if (!in || !out || !bounds || !coefs || ksize <= 0 || (axis != 0 && axis != 1)) return fail(COVER_EINVAL, "cover_resample_axis: bad arguments");
    if ((axis == 0 && Win != Wout) || (axis == 1 && Hin != Hout)) return fail(COVER_EINVAL, "cover_resample_axis: the other axis must keep its size");
    HIPCHK(launch_resample_axis(in, in_is_f32, out, out_is_f32, Hin, Win, C, Hout, Wout, axis, bounds, coefs, ksize, fixed_point, ST(stream)),
           "resample_axis (fixed point: uint8 -> uint8 only)");
    return COVER_OK;
}
int cover_u8_hwc_to_f32_chw_norm(const uint8_t* in, float* out, int H, int W, const float* mean3, const float* std3, void* stream) {
    if (!in || !out || !mean3 || !std3) return fail(COVER_EINVAL, "cover_u8_hwc_to_f32_chw_norm: null pointer");
    HIPCHK(launch_u8_to_chw_norm(in, out, H, W, 3, mean3, std3, ST(stream)), "u8_hwc_to_f32_chw_norm");
    return COVER_OK;
}
int cover_u8_hwc_to_f32_chw_scale_norm(const uint8_t* in, float* out, int H, int W, float scale, const float* mean3, const float* std3, void* stream) {
    if (!in || !out || !mean3 || !std3) return fail(COVER_EINVAL, "cover_u8_hwc_to_f32_chw_scale_norm: null pointer");
    HIPCHK(launch_u8_to_chw_scale_norm(in, out, H, W, 3, scale, mean3, std3, ST(stream)), "u8_hwc_to_f32_chw_scale_norm");
    return COVER_OK;
}
int cover_resize_bilinear_pad_f32(const float* in, float* out, int NC, int Hin, int Win, int Hr, int Wr, int Hout, int Wout, int pad_top,
                                  int pad_left, float pad_value, void* stream) {
    if (!in || !out) return fail(COVER_EINVAL, "cover_resize_bilinear_pad_f32: null pointer");
    HIPCHK(launch_bilinear_pad(in, out, NC, Hin, Win, Hr, Wr, Hout, Wout, pad_top, pad_left, pad_value, ST(stream)), "resize_bilinear_pad_f32");
    return COVER_OK;
}

// ---------------------------------------------------------------------------------------------------
// graphs, timers
// ---------------------------------------------------------------------------------------------------
int cover_graph_begin(void* stream) {
    HIPCHK(hipStreamBeginCapture(ST(stream), hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    return COVER_OK;
}
int cover_graph_end(void* stream, void** out) {
    hipGraph_t g = nullptr;
    HIPCHK(hipStreamEndCapture(ST(stream), &g), "hipStreamEndCapture");
    hipGraphExec_t ge = nullptr;
    hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    HIPCHK(e, "hipGraphInstantiate");
    *out = (void*)ge;
    return COVER_OK;
}
int cover_graph_launch(void* ge, void* stream) {
    HIPCHK(hipGraphLaunch((hipGraphExec_t)ge, ST(stream)), "hipGraphLaunch");
    return COVER_OK;
}
int cover_graph_destroy(void* ge) {
    HIPCHK(hipGraphExecDestroy((hipGraphExec_t)ge), "hipGraphExecDestroy");
    return COVER_OK;
}

struct Timer { hipEvent_t a, b; };
int cover_timer_create(void** out) {
    Timer* t = new Timer;
    hipError_t e = hipEventCreate(&t->a);
    if (e == hipSuccess) e = hipEventCreate(&t->b);
    if (e != hipSuccess) { delete t; return fail(COVER_EHIP, "hipEventCreate", e); }
    *out = t;
    return COVER_OK;
}
int cover_timer_start(void* timer, void* stream) {
    HIPCHK(hipEventRecord(((Timer*)timer)->a, ST(stream)), "hipEventRecord");
    return COVER_OK;
}
int cover_timer_stop(void* timer, void* stream, float* ms) {
    Timer* t = (Timer*)timer;
    HIPCHK(hipEventRecord(t->b, ST(stream)), "hipEventRecord");
    HIPCHK(hipEventSynchronize(t->b), "hipEventSynchronize");
    HIPCHK(hipEventElapsedTime(ms, t->a, t->b), "hipEventElapsedTime");
    return COVER_OK;
}
int cover_timer_destroy(void* timer) {
    Timer* t = (Timer*)timer;
    (void)hipEventDestroy(t->a);
    (void)hipEventDestroy(t->b);
    delete t;
    return COVER_OK;
}
int cover_stream_sync(void* stream) {
    HIPCHK(hipStreamSynchronize(ST(stream)), "hipStreamSynchronize");
    return COVER_OK;
}

size_t cover_sizeof(const char* n) {
#define SZ(T) if (!strcmp(n, #T)) return sizeof(T)
    SZ(cover_gemm_epi); SZ(cover_kv_segment); SZ(cover_attn_args); SZ(cover_rope_args); SZ(cover_patchify_args);
    SZ(cover_gemm_f32_args); SZ(cover_mha_f32_args); SZ(cover_token_select_args); SZ(cover_token_sample_args); SZ(cover_score_select_args);
    SZ(cover_prior_select_args); SZ(cover_token_sample_scored_args); SZ(cover_token_logprob_args); SZ(cover_token_topn_args); SZ(cover_token_sample_rows_args); SZ(cover_token_logprob_rows_args); SZ(cover_token_topn_rows_args); SZ(cover_token_allow); SZ(cover_token_ref); SZ(cover_decode_feedback_args); SZ(cover_token_fsm);
    SZ(cover_workspace); SZ(cover_vit_layer); SZ(cover_vit_desc); SZ(cover_dec_layer); SZ(cover_dec_desc);
    SZ(cover_dec_group); SZ(cover_dec_pass); SZ(cover_decode_attn_args); SZ(cover_own_attn_args);
    SZ(cover_beam_merge_args); SZ(cover_kv_gather_slots_args); SZ(cover_beam_backtrack_args);
    SZ(cover_gumbel_topn_args); SZ(cover_beam_merge_gumbel_args); SZ(cover_augment_args); SZ(cover_proposal_prior_args);
    SZ(cover_member_scores_args); SZ(cover_refine_args); SZ(cover_smooth_args); SZ(cover_coherence_args);
    SZ(cover_diverse_args); SZ(cover_fast_decode_args);
#undef SZ
    return 0;
}

}  // extern "C"
