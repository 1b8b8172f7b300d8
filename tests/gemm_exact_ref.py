"""Order-independent exact references for cover_gemm_bf16 (bf16 operands): the case table, the input builders and the float64 references of
tests/test_gemm_exact_cpu.py / tests/test_gemm_exact_gpu.py.

Operands are small integers (A in [-4, 4], W in [-4, 4] times a power of two): every product and every partial sum is an integer multiple of
that power of two below 2^24 of it, so an fp32 accumulation is exact in ANY order and across ANY K split, and every kernel form -- tiled,
split-K, wave pairs, weight streaming -- must produce the same bits. The reference is a float64 matmul of the same values (exact: |sum| < 2^53).

The epilogue reference follows epi_value4 / epi_store4_glu (csrc/gemm_common.h), whose rounding points the code states as intended:
    x = bf16(acc + bias)            "nn.Linear output rounding point"
    x = bf16(act(x))                when an activation is set
    x = bf16(x * layer_scale[n])    when a layer scale is set
    x = x + residual                fp32
    x = x * out_scale
    C = x (fp32 output) or bf16(x)
    GLU: C = bf16(bf16(act(bf16(gate))) * bf16(up))
With the integer / power-of-two operands of the exact kinds every value in front of a rounding is exactly representable in fp32 (asserted
below), so each rounding is one well-defined RNE and the comparison is bit for bit (integer views: the sign of a zero included).
One path differs by design: an unsplit self-loading launch (slots 23..30) with a plain fp32 output and ldc == N stores the raw fp32 sums
(launch_tiles: "an unsplit launch with a plain fp32 output IS one split-K slab") -- mirrored for exactly that path in reference()."""
import math
from collections import namedtuple

import torch

# kind: the '+'-joined epilogue parts of test_gemm_plan_cpu.epi_for (what the planner sees). mods: what the planner does not see:
#   relu / silu / gelu_tanh / gelu_erf (activation), ls (power-of-two layer scale), oscale (out_scale = 0.5), res_f32 (fp32 residual),
#   inplace (out aliases the bf16 residual), noact (a GLU without activation: exact), style0 (Gemma RMSNorm instead of Llama's for res_norm)
# variant: cover_gemm_bf16's. ws: 'sized' = cover_gemm_workspace_bytes (what ops.gemm allocates), 'tiny' = 4 bytes (no room to split K).
# wide: a.stride(0) = padded K + 128 (NaN behind the padded K) and out = columns 8 .. 8 + n_out of a buffer 24 columns wider.
# plan: (plan-counter slot, K slices, completion 0 none / 1 splitk_reduce / 2 splitk_reduce_norm, separate norm launch), pinned.
Case = namedtuple("Case", "name M N K kind mods variant ws wide plan")

SENTINEL = 768.0   # exact in bf16

# Tile of each slot (rows x columns); the M / N edges of a family are taken around it.
#   0 128x128, 1 64x128, 2 64x64 (gemm_tiled; variant 2 = the register-staged form of the same picks), 10 64x128 (loader waves),
#   19 / 20 / 22 weight streaming (16-row fragments x 16-column blocks, M <= 64 / 32 / 64), 23 224x192, 24 224x128, 25 256x128, 26 128x256,
#   30 224x96 (wave pairs).
# Out of scope: picks 3..8 and slot 27 (reachable only through the COVER_TILE_PICK knob), slot 21 (fp8 operands).
# Cases above ~50M MACs. The 1 .. 17 GMAC ones are the one smallest shape the planner sends to that slot AND completion (searched over M, N,
# K, variant, workspace): (0, split-K) 3.3G, (0, reduce + norm) 4.3G, (23, none) 13.7G, (23, split-K) 13G, (24, none) 10G, (24, split-K) and
# (24, reduce + norm) 3.8G, (25, none) 17G, (26, none) 9.7G -- slot 0 needs >= 1024 tiles of 128x128 (or variant 2 behind the loader-wave rule),
# the 224-row tiles need M >= 400, K >= 2048 and a grid on which their column width wins the cost model, 25 / 26 need M >= 512 and N > 4096.
# Slots 0, 1 and 10 are reached below 0.1G only with ONE row (N >= 24568 columns): t128_m129 (1.1G), t64x128_m65 / t64x128_v2 (0.2 / 0.6G) and
# pc64_m65 (3.4G) are their only cases with a second, ragged row tile, a strided layout or the register-staged form. The rest stay below 0.5G.
# Measured: the whole of test_gemm_exact_gpu.py, float64 references included, runs in 9 s on the MI355X host (budget: two minutes).
_ROWS = [
    # ---- slot 2: 64x64, variants 1 (global->LDS DMA) and 2 (register staged)
    ("t64_m1", 1, 64, 128, "plain", "", 1, "sized", 0),
    ("t64_m63_bias", 63, 72, 384, "bias", "", 1, "sized", 0),
    ("t64_m64_res_kodd", 64, 136, 200, "res", "", 1, "sized", 1),
    ("t64_m65_relu", 65, 64, 128, "bias", "relu", 1, "sized", 0),
    ("t64_m150_all", 150, 136, 640, "bias+res", "ls oscale", 1, "sized", 1),
    ("t64_f32", 65, 72, 384, "f32", "", 1, "sized", 1),
    ("t64_res_f32", 63, 136, 128, "res", "res_f32", 1, "sized", 0),
    ("t64_inplace", 150, 72, 384, "bias+res", "inplace", 1, "sized", 1),
    ("t64_glu", 65, 160, 384, "glu", "noact", 1, "sized", 0),
    ("t64_splitk", 150, 136, 2176, "bias+res", "", 1, "sized", 1),
    ("t64_splitk_f32", 65, 72, 2100, "f32", "", 1, "sized", 0),
    ("t64_splitk_norm", 150, 136, 2176, "res_norm", "inplace", 1, "sized", 0),
    ("t64_splitk_ln", 129, 264, 2176, "res_ln", "inplace", 1, "sized", 0),
    ("t64_v2_m1", 1, 64, 128, "plain", "", 2, "sized", 0),
    ("t64_v2_m65_bias", 65, 136, 384, "bias", "", 2, "sized", 1),
    ("t64_v2_m150_res", 150, 72, 200, "res", "", 2, "sized", 0),
    ("t64_v2_splitk", 127, 136, 2176, "bias+res", "ls", 2, "sized", 0),
    # ---- slot 1: 64x128 (>= 384 tiles of 64x128, < 1024 of 128x128)
    ("t64x128_m1_k384_relu", 1, 65536, 384, "bias", "relu", 1, "sized", 0),
    ("t64x128_m65", 65, 24584, 128, "bias+res", "", 1, "sized", 1),
    ("t64x128_v2", 63, 49160, 200, "res", "", 2, "sized", 0),
    # ---- slot 0: 128x128 (>= 1024 tiles)
    ("t128_m1", 1, 131072, 128, "plain", "", 1, "sized", 0),
    ("t128_m129", 129, 65544, 128, "bias+res", "", 1, "sized", 1),
    ("t128_v2_m1", 1, 131080, 200, "bias", "", 2, "sized", 0),
    ("t128_v2_splitk", 65, 12280, 4096, "bias+res", "", 2, "sized", 0),
    ("t128_v2_splitk_norm", 129, 8184, 4096, "res_norm", "inplace", 2, "sized", 0),
    # ---- slot 10: 64x128, four loader waves
    ("pc64_m1", 1, 24568, 4096, "plain", "", 1, "sized", 0),
    ("pc64_m65", 65, 12280, 4224, "bias+res", "", 1, "tiny", 1),
    # ---- slot 19: second-generation weight streaming (16-row fragments MF = 1..4; always reduced)
    ("sk2_m1", 1, 16, 128, "plain", "", 3, "sized", 0),
    ("sk2_m15_bias", 15, 40, 384, "bias", "", 3, "sized", 1),
    ("sk2_m16_res_kodd", 16, 264, 200, "res", "", 3, "sized", 0),
    ("sk2_m17_all", 17, 136, 1152, "bias+res", "ls oscale", 3, "sized", 1),
    ("sk2_m33_relu", 33, 520, 640, "bias", "relu", 3, "sized", 0),
    ("sk2_m49_f32", 49, 136, 128, "f32", "", 3, "sized", 1),
    ("sk2_m64_big", 64, 1376, 2176, "bias+res", "inplace", 3, "sized", 0),
    ("sk2_m32_glu", 32, 416, 2176, "glu", "noact", 3, "sized", 0),
    ("sk2_m5_norm", 5, 1024, 512, "res_norm", "inplace", 3, "sized", 0),
    ("sk2_m51_norm", 51, 1024, 2048, "res_norm", "inplace style0", 3, "sized", 0),
    # ---- slot 22: first-generation weight streaming
    ("sk1_m1", 1, 16, 128, "plain", "", 5, "sized", 0),
    ("sk1_m17_bias_res", 17, 136, 1152, "bias+res", "", 5, "sized", 1),
    ("sk1_m38_kodd", 38, 264, 200, "res", "res_f32", 5, "sized", 0),
    ("sk1_m64_f32", 64, 520, 640, "f32", "", 5, "sized", 0),
    ("sk1_m1_norm", 1, 3008, 2048, "res_norm", "inplace", 5, "sized", 0),
    # ---- slot 20: third-generation weight streaming (M <= 32, an even number of 16-column blocks, K >= 2048)
    ("sk3_m1", 1, 32, 2048, "plain", "", 6, "sized", 0),
    ("sk3_m16_bias_res", 16, 96, 2176, "bias+res", "ls", 6, "sized", 1),
    ("sk3_m17_f32", 17, 160, 4224, "f32", "", 6, "sized", 0),
    ("sk3_m32_relu", 32, 416, 2100, "bias", "relu", 6, "sized", 1),
    ("sk3_m27_glu", 27, 416, 2176, "glu", "noact", 6, "sized", 0),
    ("sk3_m1_norm_launch", 1, 64, 2176, "res_norm", "inplace", 6, "sized", 0),
    ("sk3_auto_split", 5, 6144, 2176, "bias+res", "", 0, "sized", 0),
    ("sk3_auto_split_norm", 25, 6144, 2176, "res_norm", "inplace", 0, "sized", 0),
    # ---- slot 30: 224x96 on k-split wave pairs (M within 10 % under a multiple of 224)
    ("v3k_m447", 447, 16, 2048, "plain", "", 0, "tiny", 0),
    ("v3k_m448_f32_raw", 448, 96, 2048, "f32", "", 0, "tiny", 0),
    ("v3k_m448_f32_wide", 448, 104, 2176, "f32", "", 0, "tiny", 1),
    ("v3k_m408_all", 408, 104, 2100, "bias+res", "ls oscale", 0, "tiny", 1),
    ("v3k_m611_relu", 611, 296, 2176, "bias", "relu", 0, "tiny", 0),
    ("v3k_glu", 447, 224, 2048, "glu", "noact", 0, "sized", 0),
    ("v3k_splitk", 448, 104, 2176, "bias+res", "inplace", 0, "sized", 1),
    ("v3k_splitk_f32", 447, 16, 2048, "f32", "", 0, "sized", 0),
    ("v3k_splitk_norm", 611, 296, 2304, "res_norm", "inplace", 0, "sized", 0),
    # ---- slots 23..26: the 8-wave self-loading tiles (smallest reaching shapes)
    ("v3_224x128", 815, 6152, 2048, "bias+res", "", 0, "sized", 0),
    ("v3_224x128_splitk", 1232, 504, 6144, "bias", "relu", 0, "sized", 0),
    ("v3_224x128_splitk_norm", 1232, 504, 6144, "res_norm", "inplace", 0, "sized", 0),
    ("v3_224x192", 815, 8200, 2048, "bias+res", "", 0, "sized", 0),
    ("v3_224x192_splitk", 1024, 1544, 8192, "f32", "", 0, "sized", 0),
    ("v3_256x128", 512, 16384, 2048, "bias+res", "", 0, "sized", 0),
    ("v3_256x128_splitk", 512, 16, 8192, "bias+res", "ls", 0, "sized", 1),
    ("v3_256x128_splitk_kodd", 513, 24, 8320, "f32", "", 0, "sized", 0),
    ("v3_256x128_splitk_norm", 512, 16, 8192, "res_norm", "inplace", 0, "sized", 0),
    ("v3_128x256", 513, 9208, 2048, "bias+res", "", 0, "sized", 0),
]
# (the pinned plans, in the order of _ROWS)
_PLANS = [
    (2, 1, 0, 0),   # t64_m1
    (2, 1, 0, 0),   # t64_m63_bias
    (2, 1, 0, 0),   # t64_m64_res_kodd
    (2, 1, 0, 0),   # t64_m65_relu
    (2, 1, 0, 0),   # t64_m150_all
    (2, 1, 0, 0),   # t64_f32
    (2, 1, 0, 0),   # t64_res_f32
    (2, 1, 0, 0),   # t64_inplace
    (2, 1, 0, 0),   # t64_glu
    (2, 4, 1, 0),   # t64_splitk
    (2, 4, 1, 0),   # t64_splitk_f32
    (2, 4, 2, 0),   # t64_splitk_norm
    (2, 4, 2, 0),   # t64_splitk_ln
    (2, 1, 0, 0),   # t64_v2_m1
    (2, 1, 0, 0),   # t64_v2_m65_bias
    (2, 1, 0, 0),   # t64_v2_m150_res
    (2, 4, 1, 0),   # t64_v2_splitk
    (1, 1, 0, 0),   # t64x128_m1_k384_relu
    (1, 1, 0, 0),   # t64x128_m65
    (1, 1, 0, 0),   # t64x128_v2
    (0, 1, 0, 0),   # t128_m1
    (0, 1, 0, 0),   # t128_m129
    (0, 1, 0, 0),   # t128_v2_m1
    (0, 2, 1, 0),   # t128_v2_splitk
    (0, 2, 2, 0),   # t128_v2_splitk_norm
    (10, 1, 0, 0),   # pc64_m1
    (10, 1, 0, 0),   # pc64_m65
    (19, 1, 1, 0),   # sk2_m1
    (19, 1, 1, 0),   # sk2_m15_bias
    (19, 1, 1, 0),   # sk2_m16_res_kodd
    (19, 2, 1, 0),   # sk2_m17_all
    (19, 2, 1, 0),   # sk2_m33_relu
    (19, 1, 1, 0),   # sk2_m49_f32
    (19, 5, 1, 0),   # sk2_m64_big
    (19, 3, 1, 0),   # sk2_m32_glu
    (19, 1, 2, 0),   # sk2_m5_norm
    (19, 4, 2, 0),   # sk2_m51_norm
    (22, 1, 1, 0),   # sk1_m1
    (22, 9, 1, 0),   # sk1_m17_bias_res
    (22, 2, 1, 0),   # sk1_m38_kodd
    (22, 5, 1, 0),   # sk1_m64_f32
    (22, 16, 2, 0),   # sk1_m1_norm
    (20, 1, 0, 0),   # sk3_m1
    (20, 1, 0, 0),   # sk3_m16_bias_res
    (20, 1, 0, 0),   # sk3_m17_f32
    (20, 1, 0, 0),   # sk3_m32_relu
    (20, 1, 0, 0),   # sk3_m27_glu
    (20, 1, 0, 1),   # sk3_m1_norm_launch
    (20, 2, 1, 0),   # sk3_auto_split
    (20, 2, 2, 0),   # sk3_auto_split_norm
    (30, 1, 0, 0),   # v3k_m447
    (30, 1, 0, 0),   # v3k_m448_f32_raw
    (30, 1, 0, 0),   # v3k_m448_f32_wide
    (30, 1, 0, 0),   # v3k_m408_all
    (30, 1, 0, 0),   # v3k_m611_relu
    (30, 1, 0, 0),   # v3k_glu
    (30, 4, 1, 0),   # v3k_splitk
    (30, 4, 1, 0),   # v3k_splitk_f32
    (30, 4, 2, 0),   # v3k_splitk_norm
    (24, 1, 0, 0),   # v3_224x128
    (24, 8, 1, 0),   # v3_224x128_splitk
    (24, 8, 2, 0),   # v3_224x128_splitk_norm
    (23, 1, 0, 0),   # v3_224x192
    (23, 4, 1, 0),   # v3_224x192_splitk
    (25, 1, 0, 0),   # v3_256x128
    (25, 8, 1, 0),   # v3_256x128_splitk
    (25, 8, 1, 0),   # v3_256x128_splitk_kodd
    (25, 8, 2, 0),   # v3_256x128_splitk_norm
    (26, 1, 0, 0),   # v3_128x256
]
CASES = [Case(r[0], r[1], r[2], r[3], r[4], tuple(r[5].split()), r[6], r[7], bool(r[8]), p) for r, p in zip(_ROWS, _PLANS)]
assert len(_PLANS) == len(_ROWS)

# Inexact epilogues (gelu_tanh / gelu_erf / silu, GLU with silu / gelu_tanh) on exact accumulators scaled to a standard deviation of about 2:
# the tiled, streaming, wave-pair and 8-wave forms, unsplit and through splitk_reduce
INEXACT_ROWS = [
    # name, M, N, K, kind, mods, variant, ws, wide
    ("t64_gelu_tanh", 150, 136, 384, "gelu", "", 1, "sized", 1),
    ("t64_gelu_erf", 65, 72, 640, "bias", "gelu_erf", 1, "sized", 0),
    ("t64_silu_splitk", 150, 136, 2176, "bias", "silu", 1, "sized", 0),
    ("t64_v2_glu_silu", 65, 160, 384, "glu", "", 2, "sized", 0),
    ("t64_glu_gelu", 150, 288, 640, "glu_gelu", "", 1, "sized", 1),
    ("sk2_gelu_tanh", 17, 136, 1152, "gelu", "", 3, "sized", 0),
    ("sk2_glu_silu", 32, 416, 2176, "glu", "", 3, "sized", 0),
    ("sk1_silu", 38, 264, 640, "bias", "silu", 5, "sized", 0),
    ("sk3_glu_gelu", 27, 416, 2176, "glu_gelu", "", 6, "sized", 0),
    ("sk3_gelu_erf", 16, 96, 2176, "bias", "gelu_erf", 6, "sized", 0),
    ("v3k_gelu_tanh", 447, 104, 2048, "gelu", "", 0, "tiny", 0),
    ("v3k_glu_silu", 447, 224, 2048, "glu", "", 0, "sized", 0),
    ("v3k_silu_splitk", 448, 104, 2176, "bias", "silu", 0, "sized", 1),
    ("v3_256x128_glu_gelu", 512, 32, 8192, "glu_gelu", "", 0, "sized", 0),
]
_INEXACT_PLANS = [
    (2, 1, 0, 0),   # t64_gelu_tanh
    (2, 1, 0, 0),   # t64_gelu_erf
    (2, 4, 1, 0),   # t64_silu_splitk
    (2, 1, 0, 0),   # t64_v2_glu_silu
    (2, 1, 0, 0),   # t64_glu_gelu
    (19, 2, 1, 0),   # sk2_gelu_tanh
    (19, 3, 1, 0),   # sk2_glu_silu
    (22, 5, 1, 0),   # sk1_silu
    (20, 1, 0, 0),   # sk3_glu_gelu
    (20, 1, 0, 0),   # sk3_gelu_erf
    (30, 1, 0, 0),   # v3k_gelu_tanh
    (30, 1, 0, 0),   # v3k_glu_silu
    (30, 4, 1, 0),   # v3k_silu_splitk
    (25, 8, 1, 0),   # v3_256x128_glu_gelu
]
INEXACT_CASES = [Case(r[0], r[1], r[2], r[3], r[4], tuple(r[5].split()), r[6], r[7], bool(r[8]), p) for r, p in zip(INEXACT_ROWS, _INEXACT_PLANS)]
assert len(_INEXACT_PLANS) == len(INEXACT_ROWS)

NORM_CASES = [c for c in CASES if "res_norm" in c.kind or "res_ln" in c.kind]


def position_cases():
    """one per slot: an exact case of the slot (more than one row fragment and a K beyond one k-tile where the slot has such a case, then
    the fewest MACs), as a plain bf16-output GEMM on the same shape, variant, workspace and layout -- the same plan"""
    best = {}
    key = lambda c: (c.M < 15, c.K == 128, c.M * c.N * c.K)   # noqa: E731
    for c in CASES:
        if c.kind in ("plain", "bias", "res", "bias+res") and (c.plan[0] not in best or key(c) < key(best[c.plan[0]])):
            best[c.plan[0]] = c
    return [best[s]._replace(name="pos_" + best[s].name, kind="plain", mods=()) for s in sorted(best)]


def kp(K):
    return (K + 127) // 128 * 128


def n_out(c):
    return c.N // 2 if "glu" in c.kind else c.N


def ldc_of(c):
    return n_out(c) + 24 if c.wide else n_out(c)


def parts(c):
    return set(c.kind.split("+"))


def act_of(c):
    for a in ("relu", "silu", "gelu_tanh", "gelu_erf"):
        if a in c.mods:
            return a
    p = parts(c)
    if "gelu" in p or "glu_gelu" in p:
        return "gelu_tanh"
    if "glu" in p and "noact" not in c.mods:
        return "silu"
    return "none"


def bf16_exact(x64):
    """RNE to bf16 of float64 values that are exactly representable in fp32 (asserted): ONE well-defined rounding"""
    f = x64.to(torch.float32)
    assert bool((f.to(torch.float64) == x64).all()), "a value in front of a rounding point is not exact in fp32"
    return f.to(torch.bfloat16).to(torch.float64)


def f32_exact(x64):
    f = x64.to(torch.float32)
    assert bool((f.to(torch.float64) == x64).all()), "the exact result is not representable in fp32"
    return f


def build_inputs(c, mode="int", seed=0):
    """CPU operands of a case (fp32 tensors of bf16-exact values). mode 'int': A, W integers in [-4, 4], W times 2^-2; 'scaled': W times the
    power of two that puts the pre-activations at a standard deviation of about 2 (integers times <= 2^-6); 'pos': one-hot A rows at
    k = (7 m + 3) mod K and W[n, k] = ((n K + k) mod 251) - 125, so that out[m, n] names the W element that was read."""
    g = torch.Generator().manual_seed(1000 + seed + c.M * 7 + c.N * 3 + c.K)
    M, N, K = c.M, c.N, c.K
    d = {}
    if mode == "pos":
        a = torch.zeros(M, K)
        km = (7 * torch.arange(M) + 3) % K
        a[torch.arange(M), km] = 1.0
        idx = torch.arange(N, dtype=torch.int64)[:, None] * K + torch.arange(K, dtype=torch.int64)[None, :]
        w = ((idx % 251) - 125).to(torch.float32)
        d["k_of_row"] = km
    else:
        a = torch.randint(-4, 5, (M, K), generator=g).to(torch.float32)
        w = torch.randint(-4, 5, (N, K), generator=g).to(torch.float32)
        if mode == "scaled":   # sum of K products of two uniform integers in [-4, 4]: standard deviation (20 / 3) sqrt(K)
            w = w * 2.0 ** min(-6, -round(math.log2(20.0 / 3.0 * math.sqrt(K) / 2.0)))
        else:
            w = w * 0.25
    d["a"], d["w"] = a, w
    p, no = parts(c), n_out(c)
    if p & {"bias", "gelu", "res_ln"}:
        d["bias"] = torch.randint(-8, 9, (N,), generator=g).to(torch.float32) * (0.125 if mode == "scaled" else 1.0)
    if p & {"res", "res_norm", "res_ln"}:
        d["res"] = torch.randint(-128, 129, (M, no), generator=g).to(torch.float32) * (2.0 ** -5 if mode == "scaled" else 1.0)
    if "ls" in c.mods or "res_ln" in p:
        d["ls"] = 2.0 ** torch.randint(-2, 2, (N,), generator=g).to(torch.float32)
    if p & {"res_norm", "res_ln"}:
        d["nw"] = torch.randn(N, generator=g) * 0.2 + (0.0 if "style0" in c.mods else 1.0)
        if "res_ln" in p:
            d["nb"] = torch.randn(N, generator=g) * 0.1
    d["oscale"] = 0.5 if "oscale" in c.mods else 1.0
    return d


ACT64 = {
    "none": lambda x: x,
    "relu": lambda x: torch.clamp(x, min=0.0),
    "silu": lambda x: x * torch.sigmoid(x),
    "gelu_erf": lambda x: 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0))),
    "gelu_tanh": lambda x: 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))),
}


def accumulators(d):
    """float64 matmul of the integer-valued operands: exact"""
    return d["a"].to(torch.float64) @ d["w"].to(torch.float64).T


def reference(c, d, acc=None):
    """float64 value of C in front of its final store for an EXACT case (every intermediate exact in fp32, asserted), following the rounding
    points of epi_value4 / epi_store4_glu; the un-rounded sums on the one path that stores them raw (module docstring)."""
    acc = accumulators(d) if acc is None else acc
    p = parts(c)
    act = act_of(c)
    assert act in ("none", "relu"), "inexact activation in an exact case"
    if "glu" in p:
        h = c.N // 2
        g, u = bf16_exact(acc[:, :h]), bf16_exact(acc[:, h:])
        return g * u
    raw = c.plan[0] >= 23 and c.plan[1] == 1 and c.kind == "f32" and not c.mods and not c.wide
    if raw:
        return acc
    x = acc + d["bias"].to(torch.float64) if "bias" in d else acc
    x = bf16_exact(x)
    x = ACT64[act](x)
    if "ls" in d:
        x = bf16_exact(x * d["ls"].to(torch.float64))
    if "res" in d:
        x = x + d["res"].to(torch.float64)
    return x * d["oscale"]


def reference_inexact(c, d, acc=None):
    """float64 reference of an inexact epilogue on exact accumulators: act(bf16(acc + bias)) (* bf16(up) for GLU): the pre-activation
    rounding is the kernel's stated nn.Linear rounding point, everything behind it is un-rounded float64. Returns (ref, up): up = bf16(up)
    of a GLU (what an absolute error of the activation is multiplied by), None otherwise."""
    acc = accumulators(d) if acc is None else acc
    act = ACT64[act_of(c)]
    if "glu" in c.kind:
        h = c.N // 2
        up = bf16_exact(acc[:, h:])
        return act(bf16_exact(acc[:, :h])) * up, up
    x = acc + d["bias"].to(torch.float64) if "bias" in d else acc
    return act(bf16_exact(x)), None


def norm_reference(c, d, x_stored):
    """float64 norm of the kernel's own stored bf16 residual-stream rows (what cover_rmsnorm_bf16 / cover_layernorm_bf16 define norm_out from)"""
    x = x_stored.to(torch.float64)
    nw = d["nw"].to(torch.float64)
    if "res_ln" in c.kind:
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) * torch.rsqrt(var + 1e-6) * nw + d["nb"].to(torch.float64)
    rstd = torch.rsqrt((x ** 2).mean(-1, keepdim=True) + 1e-6)
    return x * rstd * ((1.0 + nw) if "style0" in c.mods else nw)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _where(bad):
    idx = torch.nonzero(bad)
    rows, cols = torch.unique(idx[:, 0]), torch.unique(idx[:, 1])
    return (int(idx[0][0]), int(idx[0][1]),
            f"bad rows {rows[:8].tolist()}{'...' if rows.numel() > 8 else ''} ({rows.numel()}), bad columns {cols[:8].tolist()}{'...' if cols.numel() > 8 else ''} ({cols.numel()})")


def first_mismatch(got, want, what, extra=None):
    """None when got and want (same dtype, bf16 or fp32) hold the same BITS -- the sign of a zero included; else a message naming the first
    bad (m, n) with the expected and received values"""
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = _bits(got) != _bits(want)
    if not bool(bad.any()):
        return None
    m, n, where = _where(bad)
    msg = (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at (m={m}, n={n}): expected {float(want[m, n])!r}, "
           f"received {float(got[m, n])!r}; {where}")
    return msg if extra is None else msg + "; " + extra(m, n)


def first_violation(out, ref, bound, what):
    """None when |out - ref| <= bound everywhere (a NaN violates); else a message naming the first (m, n) beyond its bound"""
    err = (out.to(torch.float64) - ref).abs()
    bad = ~(err <= bound)
    if not bool(bad.any()):
        return None
    m, n, where = _where(bad)
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond their bound; first at (m={m}, n={n}): received {float(out[m, n])!r}, "
            f"float64 reference {float(ref[m, n])!r}, |difference| {float(err[m, n]):.3e} > bound {float(bound[m, n]):.3e}; {where}")
