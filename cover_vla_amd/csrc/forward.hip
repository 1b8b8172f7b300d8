// The composite forwards of libcover_hip: cover_vit_forward / cover_decoder_forward run every layer of a tower / decoder pass from one C call.
// Host code (+ zero_u32_k); the kernels live in the sibling .hip files, fail() in capi.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include "kernels.h"

// ---- workspace layout: one carve per forward. With base == nullptr only `bytes` is meaningful (the *_workspace_bytes path).
struct Carver {
    char* base;
    size_t off;
    void* take(size_t bytes) {
        off = (off + 255) / 256 * 256;
        void* p = base ? base + off : nullptr;
        off += bytes;
        return p;
    }
};
// split-K scratch of a layer: the largest need of its four GEMMs at M rows
static size_t layer_gemm_ws(int M, const int (&ns)[4], const int (&ks)[4]) {
    size_t most = 0;
    for (int i = 0; i < 4; ++i) {
        const size_t b = gemm_workspace_bytes(M, ns[i], ks[i]);
        most = b > most ? b : most;
    }
    return most;
}

struct VitWs {
    void *h, *qkv, *attn, *mlp, *vt, *sk;
    size_t sk_bytes, bytes;
    int tcap;
};
static VitWs vit_ws(const cover_vit_desc* d, int n_seq, int T, void* base) {
    const size_t R = (size_t)n_seq * T;
    const int HD = d->heads * d->head_dim_p;
    Carver c{(char*)base, 0};
    VitWs w;
    w.tcap = (T + 31) / 32 * 32;
    w.h = c.take(R * d->dim * 2);
    w.qkv = c.take(R * 3 * HD * 2);
    w.attn = c.take(R * HD * 2);
    w.mlp = c.take(R * d->mlp_p * 2);
    w.vt = c.take((size_t)n_seq * HD * w.tcap * 2);
    const int ns[4] = {3 * HD, d->dim, d->mlp_p, d->dim}, ks[4] = {d->dim, HD, d->dim, d->mlp_p};
    w.sk_bytes = layer_gemm_ws((int)R, ns, ks);
    w.sk = c.take(w.sk_bytes);
    w.bytes = c.off + 256;
    return w;
}

struct DecWs {
    void *h, *qkv, *attn, *mlp, *st_o, *st_ml, *q8, *q8s, *q8mx, *sk;
    size_t sk_bytes, bytes;
};
static DecWs dec_ws(const cover_dec_desc* d, int rows, void* base) {
    const int nqkv = (d->Hq + 2 * d->Hkv) * d->D, HD = d->Hq * d->D;
    Carver c{(char*)base, 0};
    DecWs w;
    w.h = c.take((size_t)rows * d->dim * 2);
    w.qkv = c.take((size_t)rows * nqkv * 2);
    w.attn = c.take((size_t)rows * HD * 2);
    w.mlp = c.take((size_t)rows * d->mlp * 2);
    w.st_o = c.take((size_t)rows * HD * 4);   // attention state (seg0_shared decode)
    w.st_ml = c.take((size_t)rows * d->Hq * 2 * 4);
    // e4m3 twin of the current GEMM input (rows > 64 with fp8 weights: the MX-scaled fp8 tiled GEMM) + its row scales
    int kmax = d->dim > d->mlp ? d->dim : d->mlp;
    kmax = kmax > HD ? kmax : HD;
    w.q8 = c.take((size_t)rows * ((kmax + 127) / 128 * 128));
    w.q8s = c.take((size_t)rows * 4);
    w.q8mx = c.take((size_t)rows * ((kmax + 127) / 128 * 4));   // MX block scales of the down_proj input ([k-tile][row][4])
    const int ns[4] = {nqkv, d->dim, 2 * d->mlp, d->dim}, ks[4] = {d->dim, HD, d->dim, d->mlp};
    w.sk_bytes = layer_gemm_ws(rows, ns, ks);
    w.sk = c.take(w.sk_bytes);
    w.bytes = c.off + 256;
    return w;
}

// ---- GEMM epilogues
static cover_gemm_epi epi_plain() {
    cover_gemm_epi e;
    memset(&e, 0, sizeof e);
    e.out_scale = 1.0f;
    return e;
}
// the norm of the NEXT GEMM's input rides on the GEMM that produces those rows (cover_gemm_epi.norm_*)
static void epi_norm(cover_gemm_epi& e, const float* w, const float* b, void* out, int ld_out, int style, float w_offset, float eps) {
    e.norm_w = w; e.norm_b = b; e.norm_out = out; e.ld_norm_out = ld_out;
    e.norm_style = style; e.norm_w_offset = w_offset; e.norm_eps = eps;
}

// ---- ViT tower
extern "C" __global__ void zero_u32_k(unsigned* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}

extern "C" size_t cover_vit_workspace_bytes(const cover_vit_desc* d, int n_seq, int T) { return vit_ws(d, n_seq, T, nullptr).bytes; }

extern "C" int cover_vit_forward(const cover_vit_desc* d, void* x, int n_seq, int T, void* attn_out, cover_workspace ws, int variant,
                                 void* stream) {
    if (!d || !x || !d->layers_host) return fail(COVER_EINVAL, "cover_vit_forward: null pointer");
    if (d->last_attn_only && !attn_out) return fail(COVER_EINVAL, "cover_vit_forward: last_attn_only needs attn_out");
    hipStream_t st = (hipStream_t)stream;
    const VitWs w = vit_ws(d, n_seq, T, ws.ptr);
    if (!ws.ptr || ws.bytes < w.bytes) return fail(COVER_EWORKSPACE, "cover_vit_forward: workspace too small");
    const int R = n_seq * T, dim = d->dim, H = d->heads, Dp = d->head_dim_p, HD = H * Dp, tcap = w.tcap;
    // the transposed-V scratch must be finite where keys >= T are read under a zero probability
    // (a kernel, not hipMemsetAsync: this forward is replayed inside hipGraphs, and a memset NODE was seen to run unordered with the kernel
    //  nodes around it on ROCm 7.2)
    if (tcap != T) {
        const size_t words = (size_t)n_seq * HD * tcap / 2;   // bf16 elements / 2 (HD is even)
        hipLaunchKernelGGL(zero_u32_k, dim3((unsigned)((words + 1023) / 1024 < 2048 ? (words + 1023) / 1024 : 2048)), dim3(256), 0, st, (unsigned*)w.vt, words);
        HIPCHK(hipGetLastError(), "zero vt");
    }

    // ln1 of layer 0 is its own launch; every later LayerNorm rides on the GEMM that produces its input (folded into the
    // split-K reduction whenever that GEMM splits K, which the dim-wide outputs of ViT-sized problems do)
    HIPCHK(launch_layernorm_bf16((const bf16_t*)x, dim, d->layers_host[0].ln1_w, d->layers_host[0].ln1_b, (bf16_t*)w.h, dim, R, dim, d->ln_eps, st), "vit ln1");
    for (int l = 0; l < d->n_layers; ++l) {
        const cover_vit_layer& L = d->layers_host[l];
        cover_gemm_epi e = epi_plain();
        e.bias = L.qkv_b;
        HIPCHK(launch_gemm_bf16((const bf16_t*)w.h, dim, (const bf16_t*)L.qkv_w, w.qkv, 3 * HD, R, 3 * HD, dim, &e, (float*)w.sk, w.sk_bytes, variant, st), "vit qkv");
        cover_rope_args ra;
        memset(&ra, 0, sizeof ra);
        ra.qkv = w.qkv; ra.ld_qkv = 3 * HD; ra.B = n_seq; ra.T = T; ra.Hq = H; ra.Hkv = H; ra.D = Dp; ra.rope_mode = 0;
        ra.vt_cache = w.vt; ra.vt_slot_stride = (long long)HD * tcap; ra.vt_h_stride = (long long)Dp * tcap; ra.vt_d_stride = tcap;
        HIPCHK(launch_rope_kv_write(&ra, st), "vit v-transpose");
        cover_attn_args aa;
        memset(&aa, 0, sizeof aa);
        aa.q = w.qkv; aa.q_b_stride = (long long)T * 3 * HD; aa.q_t_stride = 3 * HD; aa.q_h_stride = Dp;
        aa.out = w.attn; aa.o_b_stride = (long long)T * HD; aa.o_t_stride = HD; aa.o_h_stride = Dp;
        aa.B = n_seq; aa.Tq = T; aa.Hq = H; aa.Hkv = H; aa.D = Dp; aa.scale = d->attn_scale; aa.n_seg = 1;
        aa.seg[0].k = (const bf16_t*)w.qkv + HD; aa.seg[0].k_slot_stride = (long long)T * 3 * HD; aa.seg[0].k_t_stride = 3 * HD; aa.seg[0].k_h_stride = Dp;
        aa.seg[0].vt = w.vt; aa.seg[0].vt_slot_stride = (long long)HD * tcap; aa.seg[0].vt_h_stride = (long long)Dp * tcap; aa.seg[0].vt_d_stride = tcap;
        aa.seg[0].len = T; aa.seg[0].mask_mode = COVER_MASK_LEN;
        HIPCHK(launch_attention_bf16(&aa, st), "vit attention");
        e = epi_plain();
        e.bias = L.proj_b;
        if (d->last_attn_only && l == d->n_layers - 1) {
            HIPCHK(launch_gemm_bf16((const bf16_t*)w.attn, HD, (const bf16_t*)L.proj_w, attn_out, dim, R, dim, HD, &e, (float*)w.sk, w.sk_bytes, variant, st), "vit proj (tap)");
            break;
        }
        e.residual = x; e.ld_residual = dim; e.layer_scale = L.ls1;
        epi_norm(e, L.ln2_w, L.ln2_b, w.h, dim, 2, 0.0f, d->ln_eps);
        HIPCHK(launch_gemm_bf16((const bf16_t*)w.attn, HD, (const bf16_t*)L.proj_w, x, dim, R, dim, HD, &e, (float*)w.sk, w.sk_bytes, variant, st), "vit proj (+ln2)");
        e = epi_plain();
        e.bias = L.fc1_b; e.act = d->act;
        HIPCHK(launch_gemm_bf16((const bf16_t*)w.h, dim, (const bf16_t*)L.fc1_w, w.mlp, d->mlp_p, R, d->mlp_p, dim, &e, (float*)w.sk, w.sk_bytes, variant, st), "vit fc1");
        e = epi_plain();
        e.bias = L.fc2_b; e.residual = x; e.ld_residual = dim; e.layer_scale = L.ls2;
        if (l + 1 < d->n_layers) {
            const cover_vit_layer& Ln = d->layers_host[l + 1];
            epi_norm(e, Ln.ln1_w, Ln.ln1_b, w.h, dim, 2, 0.0f, d->ln_eps);
        }
        HIPCHK(launch_gemm_bf16((const bf16_t*)w.mlp, d->mlp_p, (const bf16_t*)L.fc2_w, x, dim, R, dim, d->mlp_p, &e, (float*)w.sk, w.sk_bytes, variant, st), "vit fc2 (+next ln1)");
    }
    return COVER_OK;
}

// ---- decoder pass
// fp8 profile with more rows than the weight-streaming kernels take (config 5: M = 512 decode rows, and its prefill): the
// projections run on the MX-scaled fp8 matrix instruction -- the input rows of every GEMM are quantised to e4m3 (per-row
// power-of-two scale) right before it, into one shared buffer. Sizes below the fp8 tiles' (tests on small geometries) stay on the bf16 kernels.
struct Fp8Mode {
    bool f8;             // the above
    bool f8q;            // the norms that produce h also emit its e4m3 twin (RMSNorm widths that are multiples of 128): two quantise launches per layer less
    bool mx, mx_fused;   // MX block scales for the down_proj input (its weight twin is the k-linear image); fused: the GLU epilogue of gate_up writes e4m3
                         // rows + one E8M0 scale per 32 columns INTO THE mlp BUFFER (no bf16 GLU output, no quantiser launch). COVER_FP8_MX_FUSE=0 keeps the
                         // bf16 output and runs cover_quantize_act_fp8_mx on it (same bytes, one launch more: the A/B of the fusion)
    bool mxo;            // the same for the o_proj input (a head = one 128-deep k-tile of o_proj) ...
    bool mxo_may_fuse;   // ... which the attention kernel of the large-N decode pass may write INTO THE attn BUFFER when attention_mx_ok accepts (per
                         // layer); every other pass (prefill: two groups) keeps the bf16 rows and quantises them with one launch
};
// the two env strings are read per call by the caller (the tests and bench.py's agreement run toggle them inside one process)
static Fp8Mode fp8_mode(const cover_dec_desc* d, int rows, int n_groups, const char* f8_env, const char* mxf_env) {
    const cover_dec_layer& L0 = d->layers_host[0];
    const bool fuse = !(mxf_env && mxf_env[0] == '0');
    Fp8Mode m;
    m.f8 = rows > 64 && L0.qkv_w8 && L0.o_w8 && L0.gate_up_w8 && L0.down_w8 && !(f8_env && f8_env[0] == '0');
    m.f8q = m.f8 && (d->dim % 128) == 0;
    m.mx = m.f8 && L0.down_klinear != 0 && rows >= 400 && d->dim >= 2048 && d->mlp >= 2048 && (d->mlp % 128) == 0 &&
           (d->act == COVER_ACT_SILU || d->act == COVER_ACT_GELU_TANH);
    m.mx_fused = m.mx && fuse;
    m.mxo = m.f8 && L0.o_klinear != 0 && rows >= 400 && d->dim >= 2048 && d->D == 128 && d->Hq == d->Hkv;
    m.mxo_may_fuse = m.mxo && n_groups == 1 && fuse;
    return m;
}

enum DecAttnRoute { OWN_KV, FUSED_DECODE, SHARED_THEN_OWN, PLAIN };

// single-token candidate decode over a shared first segment: never part of the two-group launches
static bool shared_decode(const cover_dec_group& G) { return G.seg0_shared && G.T == 1; }
// both groups in one RoPE and one attention launch: plain multi-token groups only (no shared-prefix phase split)
static bool dec_pair_ok(const cover_dec_pass* p, int qkv_splits) {
    return p->n_groups == 2 && qkv_splits == 0 && !shared_decode(p->groups[0]) && !shared_decode(p->groups[1]);
}
// The route of a group is the same in every layer. Where dec_pair_ok holds no group is a shared_decode one, so every group is PLAIN.
// FUSED_DECODE is one block per (16 candidates, head) and re-reads the shared segment per block; with many units
// AND long own-token segments (config 5: N = 512, up to 56 own keys, several serial tiles per pool-C wave) the
// three-launch path SHARED_THEN_OWN -- shared segment as ONE flash pass over all candidates, then the per-candidate segments seeded
// with its state -- is faster (N = 512: fused 109 / 163 / 362 us per layer at 1 / 16 / 56 own keys, crossover ~20;
// decision 1045 -> 950 ms). At <= 8 own keys the fused launch wins at every N measured (N = 128 / 256 / 512).
static DecAttnRoute dec_attn_route(const cover_dec_desc* d, const cover_dec_group& G, int da_max) {
    if (G.own_kv_mode > 0) return OWN_KV;
    const bool da_long = ((G.B + 15) / 16) * d->Hq >= 768 && G.segs[2].len > 16;
    if (G.T == 1 && G.seg0_shared && G.n_seg == 3 && G.write_seg == 2 && d->Hq == d->Hkv && (d->D == 64 || d->D == 128) && G.B <= da_max && !da_long &&
        G.segs[0].mask_mode == COVER_MASK_LEN && G.segs[1].mask_mode == COVER_MASK_LEN && G.segs[2].mask_mode == COVER_MASK_LEN &&
        G.write_t_offset_of_batch == nullptr && G.segs[2].len_of_batch == nullptr && G.segs[0].len_of_batch == nullptr)
        return FUSED_DECODE;
    if (G.seg0_shared && G.T == 1 && G.n_seg >= 2 && G.segs[0].mask_mode == COVER_MASK_LEN) return SHARED_THEN_OWN;
    return PLAIN;
}
// what OWN_KV needs of its group. (The parent of this check also asked for a QKV GEMM that left no split-K partials: implied, both
// partial-leaving QKV paths below require own_kv_mode == 0.)
static bool own_kv_group_ok(const cover_dec_desc* d, const cover_dec_group& G) {
    return G.T == 1 && G.n_seg == 3 && G.write_seg == 2 && G.seg0_shared && d->Hq == d->Hkv && G.seg1_group > 0 && G.B % G.seg1_group == 0 &&
           G.write_t_offset_of_batch == nullptr && G.segs[0].mask_mode == COVER_MASK_LEN && G.segs[1].mask_mode == COVER_MASK_LEN;
}

// everything a pass decides once, and the buffers its steps share
struct DecCtx {
    const cover_dec_desc* d;
    const cover_dec_pass* p;
    DecWs w;
    Fp8Mode m;
    hipStream_t st;
    int variant, rows, row0[2], nqkv, HD;
    DecAttnRoute route[2];

    // e4m3 twin of a GEMM's K-wide input rows: already in the shared buffer / quantised into it now / emitted by this GEMM's fused norm
    void use_q8(int K, cover_gemm_epi& e) const { e.a8 = w.q8; e.a8_scale = (const float*)w.q8s; e.ld_a8 = (K + 127) / 128 * 128; }
    hipError_t quant(const void* src, int K, cover_gemm_epi& e) const {
        use_q8(K, e);
        return launch_quantize_act_fp8((const bf16_t*)src, K, rows, K, (uint8_t*)w.q8, e.ld_a8, (float*)w.q8s, st);
    }
    void norm_q8(cover_gemm_epi& e) const { if (m.f8q) { e.norm_out8 = w.q8; e.norm_out8_scale = (float*)w.q8s; e.ld_norm_out8 = d->dim; } }
    hipError_t gemm(const void* A, int K, const void* W, void* C, int ldc, int N, const cover_gemm_epi& e, int* splits_out = nullptr) const {
        return launch_gemm_bf16((const bf16_t*)A, K, (const bf16_t*)W, C, ldc, rows, N, K, &e, (float*)w.sk, w.sk_bytes, variant, st, splits_out);
    }
    bf16_t* q_of(int g) const { return (bf16_t*)w.qkv + (size_t)row0[g] * nqkv; }
    bf16_t* out_of(int g) const { return (bf16_t*)w.attn + (size_t)row0[g] * HD; }
    float* state_o_of(int g) const { return (float*)w.st_o + (size_t)row0[g] * HD; }
    float* state_ml_of(int g) const { return (float*)w.st_ml + (size_t)row0[g] * d->Hq * 2; }
};

// the first n segments of a group in layer L's cache
static void bind_segments(cover_kv_segment* dst, const cover_dec_group& G, const cover_dec_layer& L, int n) {
    for (int s = 0; s < n; ++s) {
        dst[s] = G.segs[s];
        dst[s].k = (const bf16_t*)L.k_cache + G.seg_k_offset[s];
        dst[s].vt = (const bf16_t*)L.vt_cache + G.seg_vt_offset[s];
    }
}
static cover_rope_args group_rope_args(const DecCtx& c, const cover_dec_layer& L, int g, int qkv_splits) {
    const cover_dec_desc* d = c.d;
    const cover_dec_group& G = c.p->groups[g];
    const cover_kv_segment& W = G.segs[G.write_seg];
    cover_rope_args ra;
    memset(&ra, 0, sizeof ra);
    ra.qkv = c.q_of(g); ra.ld_qkv = c.nqkv; ra.B = G.B; ra.T = G.T; ra.Hq = d->Hq; ra.Hkv = d->Hkv; ra.D = d->D;
    ra.positions = G.positions; ra.cos_table = d->cos_table; ra.sin_table = d->sin_table; ra.n_pos = d->n_pos;
    ra.rope_mode = d->rope_mode;
    ra.k_cache = (bf16_t*)L.k_cache + G.seg_k_offset[G.write_seg];
    ra.k_slot_stride = W.k_slot_stride; ra.k_t_stride = W.k_t_stride; ra.k_h_stride = W.k_h_stride;
    ra.vt_cache = (bf16_t*)L.vt_cache + G.seg_vt_offset[G.write_seg];
    ra.vt_slot_stride = W.vt_slot_stride; ra.vt_h_stride = W.vt_h_stride; ra.vt_d_stride = W.vt_d_stride;
    ra.slot_of_batch = G.write_slot_of_batch; ra.t_offset_of_batch = G.write_t_offset_of_batch; ra.t_offset = G.write_t_offset;
    if (qkv_splits > 0) { ra.n_splits = qkv_splits; ra.partial = (const float*)c.w.sk; ra.bias = L.qkv_b; }
    return ra;
}
static cover_attn_args group_attn_args(const DecCtx& c, const cover_dec_layer& L, int g) {
    const cover_dec_desc* d = c.d;
    const cover_dec_group& G = c.p->groups[g];
    cover_attn_args aa;
    memset(&aa, 0, sizeof aa);
    aa.q = c.q_of(g); aa.q_b_stride = (long long)G.T * c.nqkv; aa.q_t_stride = c.nqkv; aa.q_h_stride = d->D;
    aa.out = c.out_of(g); aa.o_b_stride = (long long)G.T * c.HD; aa.o_t_stride = c.HD; aa.o_h_stride = d->D;
    aa.B = G.B; aa.Tq = G.T; aa.Hq = d->Hq; aa.Hkv = d->Hkv; aa.D = d->D; aa.scale = d->attn_scale; aa.n_seg = G.n_seg;
    bind_segments(aa.seg, G, L, G.n_seg);
    return aa;
}

// OWN_KV, large-N candidate decode: own-token pass on the VALU (RoPE + append + attention over the candidate's own keys, state out), then ONE
// MFMA pass over [shared prefix | the prompt's text] with the samples of a prompt as the query rows of a batch entry, resumed from that state
static int attn_own_kv(const DecCtx& c, const cover_dec_layer& L, int g, bool* mxo_fused) {
    const cover_dec_desc* d = c.d;
    const cover_dec_group& G = c.p->groups[g];
    cover_own_attn_args oa;
    memset(&oa, 0, sizeof oa);
    oa.qkv = c.q_of(g); oa.ld_qkv = c.nqkv; oa.N = G.B; oa.H = d->Hq; oa.D = d->D; oa.scale = d->attn_scale;
    oa.positions = G.positions; oa.cos_table = d->cos_table; oa.sin_table = d->sin_table; oa.n_pos = d->n_pos; oa.rope_mode = d->rope_mode;
    oa.slot_stride = G.segs[G.write_seg].k_slot_stride;
    oa.fp8 = G.own_kv_mode == 2; oa.t_cap = (int)(oa.slot_stride / ((long long)d->Hkv * d->D));
    char* kb = (char*)L.k_cache + 2 * G.seg_k_offset[2];
    char* vb = (char*)L.vt_cache + 2 * G.seg_vt_offset[2];
    oa.k = kb; oa.v = vb;
    if (oa.fp8) { oa.k_scale = (float*)(kb + G.own_region_elems); oa.v_scale = (float*)(vb + G.own_region_elems); }
    oa.slot_of_batch = G.write_slot_of_batch ? G.write_slot_of_batch : G.segs[2].slot_of_batch;
    oa.write_t = G.write_t_offset;
    oa.state_o = c.state_o_of(g); oa.state_ml = c.state_ml_of(g);
    HIPCHK(launch_decode_own_attention(&oa, c.st), "dec own-token attention");
    cover_attn_args sa;
    memset(&sa, 0, sizeof sa);
    const int S = G.seg1_group;
    sa.q = c.q_of(g); sa.q_b_stride = (long long)S * c.nqkv; sa.q_t_stride = c.nqkv; sa.q_h_stride = d->D;
    sa.out = c.out_of(g); sa.o_b_stride = (long long)S * c.HD; sa.o_t_stride = c.HD; sa.o_h_stride = d->D;
    sa.B = G.B / S; sa.Tq = S; sa.Hq = d->Hq; sa.Hkv = d->Hkv; sa.D = d->D; sa.scale = d->attn_scale; sa.n_seg = 2;
    bind_segments(sa.seg, G, L, 2);
    sa.seg[1].slot_of_batch = G.seg1_slot_of_group; sa.seg[1].len_of_batch = G.seg1_len_of_group;
    sa.state_in_o = oa.state_o; sa.state_in_ml = oa.state_ml;
    if (c.m.mxo_may_fuse) {
        sa.out8 = c.w.attn; sa.out8_mx = c.w.q8mx; sa.out8_rows = c.rows;
        if (attention_mx_ok(&sa)) *mxo_fused = true;
        else { sa.out8 = nullptr; sa.out8_mx = nullptr; }
    }
    HIPCHK(launch_attention_bf16(&sa, c.st), "dec attention (shared prefix + prompt text, resumed from the own-token state)");
    return COVER_OK;
}
// FUSED_DECODE, single-token candidate decode: RoPE + KV append + 3-segment attention in ONE launch
static int attn_fused_decode(const DecCtx& c, const cover_dec_layer& L, int g, int qkv_splits) {
    const cover_dec_desc* d = c.d;
    const cover_dec_group& G = c.p->groups[g];
    cover_decode_attn_args da;
    memset(&da, 0, sizeof da);
    da.qkv = c.q_of(g); da.ld_qkv = c.nqkv;
    if (qkv_splits > 0) { da.n_splits = qkv_splits; da.partial = (const float*)c.w.sk; da.bias = L.qkv_b; }
    da.N = G.B; da.H = d->Hq; da.D = d->D; da.scale = d->attn_scale;
    da.positions = G.positions; da.cos_table = d->cos_table; da.sin_table = d->sin_table; da.n_pos = d->n_pos;
    da.rope_mode = d->rope_mode;
    bind_segments(da.seg, G, L, 3);
    da.seg[2].slot_of_batch = G.write_slot_of_batch ? G.write_slot_of_batch : G.segs[2].slot_of_batch;
    da.write_t = G.write_t_offset;
    da.out = c.out_of(g); da.out_row_stride = c.HD;
    HIPCHK(launch_decode_attention_fused(&da, c.st), "dec fused decode attention");
    return COVER_OK;
}
// SHARED_THEN_OWN: RoPE / KV placement, the shared segment once for all candidates, then each candidate's own segments
static int attn_shared_then_own(const DecCtx& c, const cover_dec_layer& L, int g, int qkv_splits) {
    const cover_dec_group& G = c.p->groups[g];
    const cover_rope_args ra = group_rope_args(c, L, g, qkv_splits);
    cover_attn_args aa = group_attn_args(c, L, g);
    HIPCHK(launch_rope_kv_write(&ra, c.st), "dec rope/kv");
    // phase A: the shared segment, candidates as the query rows of one "sequence"
    cover_attn_args pa = aa;
    pa.B = 1; pa.Tq = G.B; pa.q_b_stride = 0; pa.q_t_stride = c.nqkv;
    pa.n_seg = 1;
    pa.out = nullptr;
    pa.state_out_o = c.state_o_of(g); pa.state_out_ml = c.state_ml_of(g);
    HIPCHK(launch_attention_bf16(&pa, c.st), "dec attention (shared segment)");
    // phase B: each candidate's own segments, seeded with the phase-A state
    for (int s = 1; s < G.n_seg; ++s) aa.seg[s - 1] = aa.seg[s];
    aa.n_seg = G.n_seg - 1;
    aa.state_in_o = pa.state_out_o; aa.state_in_ml = pa.state_out_ml;
    HIPCHK(launch_attention_bf16(&aa, c.st), "dec attention");
    return COVER_OK;
}
// PLAIN: RoPE / KV placement, then attention over the group's segments
static int attn_plain(const DecCtx& c, const cover_dec_layer& L, int g, int qkv_splits) {
    const cover_rope_args ra = group_rope_args(c, L, g, qkv_splits);
    const cover_attn_args aa = group_attn_args(c, L, g);
    HIPCHK(launch_rope_kv_write(&ra, c.st), "dec rope/kv");
    HIPCHK(launch_attention_bf16(&aa, c.st), "dec attention");
    return COVER_OK;
}
// two row groups of one pass (prefill: shared-prefix rows + the prompts' text rows): RoPE / KV placement of both,
// then attention of both, one launch each -- the second group attends keys the first one writes
static int attn_pair(const DecCtx& c, const cover_dec_layer& L) {
    const cover_rope_args ra0 = group_rope_args(c, L, 0, 0), ra1 = group_rope_args(c, L, 1, 0);
    const cover_attn_args aa0 = group_attn_args(c, L, 0), aa1 = group_attn_args(c, L, 1);
    HIPCHK(launch_rope_kv_write_pair(&ra0, &ra1, c.st), "dec rope/kv (both groups)");
    HIPCHK(launch_attention_bf16_pair(&aa0, &aa1, c.st), "dec attention (both groups)");
    return COVER_OK;
}
// attention of every group of the pass in layer L
static int dec_attention(const DecCtx& c, const cover_dec_layer& L, int qkv_splits, bool* mxo_fused) {
    const cover_dec_group* G = c.p->groups;
    // (pair_ok with one empty group: the other one alone, below)
    if (dec_pair_ok(c.p, qkv_splits) && G[0].B * G[0].T != 0 && G[1].B * G[1].T != 0) return attn_pair(c, L);
    for (int g = 0; g < c.p->n_groups; ++g) {
        if (G[g].B * G[g].T == 0) continue;
        const DecAttnRoute r = c.route[g];
        const int rc = r == OWN_KV ? attn_own_kv(c, L, g, mxo_fused) : r == FUSED_DECODE ? attn_fused_decode(c, L, g, qkv_splits) :
                       r == SHARED_THEN_OWN ? attn_shared_then_own(c, L, g, qkv_splits) : attn_plain(c, L, g, qkv_splits);
        if (rc != COVER_OK) return rc;
    }
    return COVER_OK;
}

extern "C" size_t cover_decoder_workspace_bytes(const cover_dec_desc* d, int rows) { return dec_ws(d, rows, nullptr).bytes; }

extern "C" int cover_decoder_forward(const cover_dec_desc* d, const cover_dec_pass* p, void* x, cover_workspace ws, int variant,
                                     void* stream) {
    if (!d || !p || !x || !d->layers_host) return fail(COVER_EINVAL, "cover_decoder_forward: null pointer");
    if (p->n_groups < 1 || p->n_groups > 2) return fail(COVER_EINVAL, "cover_decoder_forward: 1 or 2 groups");
    DecCtx c;
    c.d = d; c.p = p; c.st = (hipStream_t)stream; c.variant = variant; c.rows = 0; c.row0[0] = c.row0[1] = 0;
    for (int g = 0; g < p->n_groups; ++g) {
        const cover_dec_group& G = p->groups[g];
        if (G.n_seg < 1 || G.n_seg > 3 || G.write_seg < 0 || G.write_seg >= G.n_seg)
            return fail(COVER_EINVAL, "cover_decoder_forward: bad segment description");
        c.row0[g] = c.rows;
        c.rows += G.B * G.T;
    }
    c.w = dec_ws(d, c.rows, ws.ptr);
    if (!ws.ptr || ws.bytes < c.w.bytes) return fail(COVER_EWORKSPACE, "cover_decoder_forward: workspace too small");
    const int rows = c.rows, dim = d->dim, mlp = d->mlp, nqkv = c.nqkv = (d->Hq + 2 * d->Hkv) * d->D, HD = c.HD = d->Hq * d->D, mlp_p = (mlp + 127) / 128 * 128;
    const DecWs& w = c.w;
    const Fp8Mode m = c.m = fp8_mode(d, rows, p->n_groups, getenv("COVER_FP8_MFMA"), getenv("COVER_FP8_MX_FUSE"));
    static const char* da_max_env = getenv("COVER_DA_FUSED_MAX_N");   // experiment knob: force the three-launch path above N
    const int da_max = da_max_env ? atoi(da_max_env) : (1 << 30);
    for (int g = 0; g < p->n_groups; ++g) {
        const cover_dec_group& G = p->groups[g];
        c.route[g] = dec_attn_route(d, G, da_max);
        if (c.route[g] == OWN_KV && G.B * G.T != 0 && !own_kv_group_ok(d, G))
            return fail(COVER_EINVAL, "cover_decoder_forward: own_kv_mode needs T == 1, three segments (shared | per prompt | own), MHA, a regular seg1_group");
    }
    // weight-streaming path: leave the split-K partials of the QKV GEMM for rope_kv_write to fold (one launch and one pass less)
    const cover_dec_group& G0 = p->groups[0];
    const bool qkv_partial = rows <= 64 && p->n_groups == 1 && (variant == 0 || variant == 3) && G0.own_kv_mode == 0;
    // few-token groups on the LDS tiles (the pi0 action expert: 200 rows, T = 5): a split-K launch leaves its slabs for
    // rope_kv_write to fold as well (same sums, same order, same rounding as the reduction launch it replaces)
    const char* fold_env = getenv("COVER_QKV_FOLD");   // A/B knob (read per call: the tests toggle it): 0 keeps the reduction launch
    const bool qkv_fold = rows > 64 && p->n_groups == 1 && G0.own_kv_mode == 0 && G0.T < 16 && !m.f8 && !shared_decode(G0) && !(fold_env && fold_env[0] == '0');

    // h = in_norm_0(x); afterwards every norm is folded into the epilogue of the GEMM that produces its input
    const bool f32in = p->x_f32 != nullptr;
    HIPCHK(launch_rmsnorm(f32in ? (const void*)p->x_f32 : (const void*)x, f32in ? 1 : 0, dim, d->layers_host[0].in_norm_w,
                          d->norm_w_offset, d->norm_style, (bf16_t*)w.h, dim, rows, dim, d->norm_eps, c.st,
                          m.f8q ? (uint8_t*)w.q8 : nullptr, m.f8q ? (dim + 127) / 128 * 128 : 0, m.f8q ? (float*)w.q8s : nullptr), "dec in_norm");
    for (int l = 0; l < d->n_layers; ++l) {
        const cover_dec_layer& L = d->layers_host[l];
        const cover_dec_layer* next = l + 1 < d->n_layers ? &d->layers_host[l + 1] : nullptr;   // its input norm rides on this layer's down GEMM
        // 1. qkv GEMM
        cover_gemm_epi e = epi_plain();
        e.bias = L.qkv_b;
        e.w8 = L.qkv_w8; e.w8_scale = L.qkv_s;
        if (m.f8q) c.use_q8(dim, e);                               // h8 came with the norm that produced h
        else if (m.f8) HIPCHK(c.quant(w.h, dim, e), "dec quantise (qkv input)");
        int qkv_splits = 0;
        if (qkv_partial)
            HIPCHK(launch_gemm_skinny_partial((const bf16_t*)w.h, dim, (const bf16_t*)L.qkv_w, (float*)w.sk, w.sk_bytes, rows, nqkv, dim, &qkv_splits, c.st,
                                              L.qkv_w8, L.qkv_s), "dec qkv (partials)");
        else
            HIPCHK(c.gemm(w.h, dim, L.qkv_w, w.qkv, nqkv, nqkv, e, qkv_fold ? &qkv_splits : nullptr), "dec qkv");
        // 2. attention of the groups (mxo_fused: the kernel wrote o_proj's block-scaled operand itself)
        bool mxo_fused = false;
        if (const int rc = dec_attention(c, L, qkv_splits, &mxo_fused)) return rc;
        // 3. o_proj (+post_norm)
        const bool first_f32 = l == 0 && f32in;
        e = epi_plain();
        e.residual = first_f32 ? (const void*)p->x_f32 : (const void*)x; e.residual_f32 = first_f32 ? 1 : 0; e.ld_residual = dim;
        epi_norm(e, L.post_norm_w, nullptr, w.h, dim, d->norm_style, d->norm_w_offset, d->norm_eps);
        e.w8 = L.o_w8; e.w8_scale = L.o_s; e.w8_klinear = L.o_klinear;
        if (m.mxo) {
            if (!mxo_fused) HIPCHK(launch_quantize_act_fp8_mx((const bf16_t*)w.attn, HD, rows, HD, (uint8_t*)w.q8, HD, (uint8_t*)w.q8mx, c.st), "dec quantise (o_proj input, MX)");
            e.a8 = mxo_fused ? w.attn : w.q8; e.ld_a8 = HD; e.a8_mx = w.q8mx;
        } else if (m.f8 && !L.o_klinear) {
            HIPCHK(c.quant(w.attn, HD, e), "dec quantise (o_proj input)");
        }   // (a k-linear twin below the MX sizes: bf16 operands on the bf16 image)
        c.norm_q8(e);
        HIPCHK(c.gemm(w.attn, HD, L.o_w, x, dim, dim, e), "dec o_proj (+post_norm)");
        // 4. gate_up
        e = epi_plain();
        e.act = d->act; e.glu = 1;
        e.w8 = L.gate_up_w8; e.w8_scale = L.gate_up_s;
        if (m.f8q) c.use_q8(dim, e);
        else if (m.f8) HIPCHK(c.quant(w.h, dim, e), "dec quantise (gate_up input)");
        if (m.mx_fused) { e.out8 = w.mlp; e.out8_mx = w.q8mx; e.ld_out8 = mlp_p; }
        HIPCHK(c.gemm(w.h, dim, L.gate_up_w, w.mlp, mlp, 2 * mlp, e), "dec gate_up");
        // 5. down (+next in_norm)
        e = epi_plain();
        e.residual = x; e.ld_residual = dim;
        if (next) epi_norm(e, next->in_norm_w, nullptr, w.h, dim, d->norm_style, d->norm_w_offset, d->norm_eps);
        e.w8 = L.down_w8; e.w8_scale = L.down_s; e.w8_klinear = L.down_klinear;
        if (m.mx) {
            if (!m.mx_fused) HIPCHK(launch_quantize_act_fp8_mx((const bf16_t*)w.mlp, mlp, rows, mlp, (uint8_t*)w.q8, mlp_p, (uint8_t*)w.q8mx, c.st), "dec quantise (down input, MX)");
            e.a8 = m.mx_fused ? w.mlp : w.q8; e.ld_a8 = mlp_p; e.a8_mx = w.q8mx;
        } else if (m.f8 && !L.down_klinear) {
            HIPCHK(c.quant(w.mlp, mlp, e), "dec quantise (down input)");
        }   // (a k-linear twin below the MX sizes: bf16 operands on the bf16 image)
        if (next) c.norm_q8(e);
        HIPCHK(c.gemm(w.mlp, mlp, L.down_w, x, dim, dim, e), "dec down (+next in_norm)");
    }
    if (p->final_norm)
        HIPCHK(launch_rmsnorm(x, 0, dim, d->final_norm_w, d->norm_w_offset, d->norm_style, (bf16_t*)x, dim, rows, dim, d->norm_eps, c.st), "dec final_norm");
    return COVER_OK;
}
