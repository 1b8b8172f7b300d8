"""The GEMM planner on its own (cover_gemm_plan, no GPU): the kernel family, tile, K split and completion cover_gemm_bf16 would take
for every GEMM the shipped profiles issue, every shape a GPU test asserts a plan counter for, and a seeded sweep of the planner's
inputs, pinned against literal tables. The tables were recorded from the planner as it was before it was split from the launch code
(a dry-run exit in front of each launch), so they pin the dispatch that ran before, not the one that runs now.

Pointers are fake, aligned addresses: the planner only checks them for null and alignment."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

from cover_vla_amd import _lib

EINVAL = -1   # COVER_EINVAL

# fake device addresses (never dereferenced)
_A, _W, _C, _WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000
_BIAS, _RES, _LS, _NW, _NOUT, _NB = 0x51000000, 0x52000000, 0x53000000, 0x54000000, 0x55000000, 0x56000000
_W8, _W8S, _A8, _A8S, _A8MX, _O8, _O8MX = 0x61000000, 0x62000000, 0x63000000, 0x64000000, 0x65000000, 0x66000000, 0x67000000

ACT = {"none": 0, "gelu_tanh": 1, "gelu_erf": 2, "silu": 3}


def kp(K):
    return (K + 127) // 128 * 128


def epi_for(kind, M, N, K):
    """kind = '+'-joined parts: plain, bias, gelu (bias + gelu_tanh), res_norm (residual + RMSNorm), res_ln (bias + residual + layer scale +
    LayerNorm), res (residual), f32 (fp32 output), glu (GLU, act silu), glu_gelu (GLU, act gelu_tanh); fp8 operands: w8 (e4m3 weight twin),
    a8 (+ per-row e4m3 activations), mx (k-linear twin + MX block-scaled activations), out8 (GLU output written block-quantised),
    a8kl (k-linear twin with PER-ROW activations: rejected on the fp8 tiles)"""
    e = _lib.GemmEpi()
    e.out_scale = 1.0
    parts = kind.split("+")
    nout = N // 2 if ("glu" in parts or "glu_gelu" in parts) else N
    for p in parts:
        if p == "plain":
            pass
        elif p == "bias":
            e.bias = _BIAS
        elif p == "gelu":
            e.bias, e.act = _BIAS, ACT["gelu_tanh"]
        elif p == "res":
            e.residual, e.ld_residual = _RES, N
        elif p == "res_norm":
            e.residual, e.ld_residual = _RES, N
            e.norm_w, e.norm_out, e.ld_norm_out, e.norm_style, e.norm_eps = _NW, _NOUT, N, 1, 1e-6
        elif p == "res_ln":
            e.bias, e.residual, e.ld_residual, e.layer_scale = _BIAS, _RES, N, _LS
            e.norm_w, e.norm_b, e.norm_out, e.ld_norm_out, e.norm_style, e.norm_eps = _NW, _NB, _NOUT, N, 2, 1e-6
        elif p == "f32":
            e.out_f32 = 1
        elif p in ("glu", "glu_gelu"):
            e.glu, e.act = 1, ACT["silu"] if p == "glu" else ACT["gelu_tanh"]
        elif p == "w8":
            e.w8, e.w8_scale = _W8, _W8S
        elif p == "a8":
            e.w8, e.w8_scale, e.a8, e.a8_scale, e.ld_a8 = _W8, _W8S, _A8, _A8S, kp(K)
        elif p == "mx":
            e.w8, e.w8_scale, e.w8_klinear, e.a8, e.a8_mx, e.ld_a8 = _W8, _W8S, 1, _A8, _A8MX, kp(K)
        elif p == "a8kl":
            e.w8, e.w8_scale, e.w8_klinear, e.a8, e.a8_scale, e.ld_a8 = _W8, _W8S, 1, _A8, _A8S, kp(K)
        elif p == "out8":
            e.out8, e.out8_mx, e.ld_out8 = _O8, _O8MX, kp(nout)
        else:
            raise ValueError(p)
    return e, nout


def plan(M, N, K, kind, variant, ws_bytes, C_ptr=_C, ldc=None, lda=None, ld_a8=None):
    h = _lib.lib()
    e, nout = epi_for(kind, M, N, K)
    if ld_a8 is not None and e.a8:
        e.ld_a8 = ld_a8
    out = (C.c_int * 6)()
    rc = h.cover_gemm_plan(_A, kp(K) if lda is None else lda, _W, C_ptr, nout if ldc is None else ldc, M, N, K, C.byref(e),
                           _WS if ws_bytes else None, ws_bytes, variant, out)
    assert rc in (0, EINVAL), rc
    return tuple(out) if rc == 0 else None


def ws_of(M, shapes):
    """the workspace a layer sizes: the largest cover_gemm_workspace_bytes over its GEMMs at M rows"""
    return max(_lib.lib().cover_gemm_workspace_bytes(M, n, k) for n, k in shapes)


def model_cases():
    """(label, M, N, K, kind, variant, ws_bytes, f8_off): the GEMMs of the shipped profiles as the layer code issues them
    (cover_vla_amd/synth.py sizes; the decoder / tower workspace = the largest over the layer's four GEMMs, as forward.hip sizes it)"""
    cases = []

    def decoder(tag, M, dim, Hq, Hkv, D, mlp, act, fp8=False, f8_off=False):
        nqkv, hd = (Hq + 2 * Hkv) * D, Hq * D
        ws = ws_of(M, [(nqkv, dim), (dim, hd), (2 * mlp, dim), (dim, mlp)])
        glu = "glu" if act == "silu" else "glu_gelu"
        if fp8:   # config 5 at M >= 400: per-row a8 for qkv, MX block scales for o / down, gate_up writes the down operand (out8)
            q, o, gu, dn = "a8", "res_norm+mx", glu + "+a8+out8", "res_norm+mx"
        else:
            q, o, gu, dn = "plain", "res_norm", glu, "res_norm"
        for name, n, k, kind in (("qkv", nqkv, dim, q), ("o", dim, hd, o), ("gate_up", 2 * mlp, dim, gu), ("down", dim, mlp, dn)):
            cases.append((f"{tag} {name}", M, n, k, kind, 0, ws, f8_off))

    def tower(tag, R, dim, heads, mlp, act_kind="gelu"):
        dp = next(c for c in (64, 96, 128, 256) if dim // heads <= c)
        hd, mlp_p = heads * dp, kp(mlp)
        ws = ws_of(R, [(3 * hd, dim), (dim, hd), (mlp_p, dim), (dim, mlp_p)])
        for name, n, k, kind in (("qkv", 3 * hd, dim, "bias"), ("proj", dim, hd, "res_ln"), ("fc1", mlp_p, dim, act_kind),
                                 ("fc2", dim, mlp_p, "res_ln")):
            cases.append((f"{tag} {name}", R, n, k, kind, 0, ws, False))

    # OpenVLA-7B (Llama-2 7B decoder): prefill 448 rows (704 with two cameras), decode 32 / 16 rows
    for M in (448, 704, 32, 16):
        decoder(f"openvla M={M}", M, 4096, 32, 32, 128, 11008, "silu")
    # config 5: 512 decode rows on e4m3 weights, and the same with COVER_FP8_MFMA=0
    decoder("config5 M=512", 512, 4096, 32, 32, 128, 11008, "silu", fp8=True)
    decoder("config5 M=512 fp8-mfma off", 512, 4096, 32, 32, 128, 11008, "silu", fp8=True, f8_off=True)
    # config 5's qkv / gate_up without the MX forms (per-row a8 only) and its e4m3 weight stream at decode sizes
    cases.append(("config5 gate_up per-row", 512, 22016, 4096, "glu+a8", 0, ws_of(512, [(22016, 4096), (4096, 11008)]), False))
    cases.append(("config5 gate_up per-row fp8-mfma off", 512, 22016, 4096, "glu+a8", 0, ws_of(512, [(22016, 4096), (4096, 11008)]), True))
    for M in (16, 32):
        for name, n, k, kind in (("qkv", 12288, 4096, "w8"), ("o", 4096, 4096, "res_norm+w8"), ("gate_up", 22016, 4096, "glu+w8"),
                                 ("down", 4096, 11008, "res_norm+w8")):
            cases.append((f"e4m3 stream M={M} {name}", M, n, k, kind, 0, ws_of(M, [(12288, 4096), (4096, 4096), (22016, 4096), (4096, 11008)]), False))
    # OpenVLA heads (fp32 logits)
    for M in (16, 32, 64):
        cases.append((f"openvla lm_head M={M}", M, 32064, 4096, "f32", 0, _lib.lib().cover_gemm_workspace_bytes(M, 32064, 4096), False))
    # pi0 (PaliGemma Gemma-2B prefix, 300M action expert): prefix 8 prompts x (256 + 72) rows, expert 40 x 5 rows
    decoder("pi0 prefix M=2624", 2624, 2048, 8, 1, 256, 16384, "gelu_tanh")
    decoder("pi0 expert M=200", 200, 1024, 8, 1, 256, 4096, "gelu_tanh")
    # vision towers: DINOv2-L (256 patches + 5 prefix tokens), SigLIP-So400m (OpenVLA: one camera; pi0: 8 images), SigLIP2-L (verifier, 384^2)
    tower("dinov2 R=261", 261, 1024, 16, 4096)
    tower("siglip R=256", 256, 1152, 16, 4304)
    tower("siglip R=2048", 2048, 1152, 16, 4304)
    tower("siglip2 R=576", 576, 1024, 16, 4096)
    return cases


def gpu_test_cases():
    """(label, M, N, K, kind, variant, ws_bytes, f8_off): the shapes test_kernels_gpu.py / test_fp8_gpu.py assert a plan counter for, with
    ops.gemm's own workspace; the decoder of test_fp8_gpu.py's MX test as its layer issues it"""
    cases = []
    wsb = lambda M, N, K: _lib.lib().cover_gemm_workspace_bytes(M, N, K)   # noqa: E731
    shapes = [(448, 12288, 4096, "bias+res"), (448, 12288, 4096, "f32"), (440, 12288 - 16, 4096 + 64, "bias+res"), (448, 3072, 2048, "plain"),
              (2232, 2560, 2048, "plain"), (672, 1536, 4096, "res_norm"),                                 # test_gemm_k_split_wave_pairs
              (448, 22016, 4096, "glu"), (448, 4096, 4096, "res_norm"), (448, 4096, 11008, "res_norm")]   # test_gemm_headline_prefill_tiles_m448_bf16
    for M, N, K, norm in ((512, 4096, 11008, True), (448, 4096, 11008, True), (200, 4096, 4096, False), (530, 1040, 2304, False),
                          (1024, 8192, 2304, False)):                                                     # test_fp8_mx_tiled_gemm_matches_fp32_...
        shapes += [(M, N, K, "bias+res_norm+mx" if norm else "bias+mx"), (M, N, K, "bias+res_norm+a8" if norm else "bias+a8")]
    for M, N, K, glu in ((512, 22016, 4096, "glu"), (448, 22016, 4096, "glu"), (300, 2 * 2080, 2304, "glu_gelu")):
        shapes += [(M, N, K, glu + "+a8"), (M, N, K, glu + "+a8+out8")]                                   # test_glu_gemm_writes_the_mx_form_...
    for M, N, K, kind in shapes:
        cases.append((f"gpu test M={M} N={N} K={K} {kind}", M, N, K, kind, 0, wsb(M, N, K), False))
    # test_decoder_mx_down_input_fused_equals_unfused_and_matches_oracle: 2048 wide, 16 heads of 128, MLP 4096, 448 rows, e4m3 weights
    ws = max(wsb(448, n, k) for n, k in ((6144, 2048), (2048, 2048), (8192, 2048), (2048, 4096)))
    for name, n, k, kind in (("qkv", 6144, 2048, "a8"), ("o", 2048, 2048, "res_norm+mx"), ("gate_up", 8192, 2048, "glu+a8+out8"),
                             ("gate_up unfused", 8192, 2048, "glu+a8"), ("down", 2048, 4096, "res_norm+mx")):
        cases.append((f"gpu test mx decoder {name}", 448, n, k, kind, 0, ws, False))
    return cases


def sweep_cases(n=360, seed=20261016):
    """seeded sweep of M, N, K, epilogue, variant and workspace (after tools/dbg/fuzz_gemm.py)"""
    rnd = random.Random(seed)
    out = []
    for c in range(n):
        kind = rnd.choice(["plain", "bias", "gelu", "res", "res_norm", "res_ln", "f32", "glu", "w8", "res_norm+w8", "glu+w8", "a8", "res_norm+a8",
                           "glu+a8", "mx", "res_norm+mx", "glu+a8+out8"])
        M = rnd.choice([rnd.randint(1, 64), rnd.randint(65, 300), rnd.randint(301, 1200), rnd.choice([1, 16, 17, 32, 33, 64, 65, 224, 225, 448, 449, 512, 704, 2624])])
        K = 128 * rnd.choice([1, 2, 3, 5, 8, 9, 16, 17, 32, 33, 43, 86])
        N = 8 * rnd.randint(1, 1400) if rnd.random() < 0.7 else rnd.choice([16, 32, 64, 1024, 4096, 4304, 12288, 11008, 22016])
        if "glu" in kind:
            N = max(32, N // 32 * 32)
        variant = rnd.choice([0, 0, 0, 1, 2, 3, 5, 6])
        ws = rnd.choice(["none", "sized", "sized"])
        wsb = 0 if ws == "none" else _lib.lib().cover_gemm_workspace_bytes(M, N, K)
        out.append((f"sweep {c}", M, N, K, kind, variant, wsb))
    return out


def test_cover_gemm_plan_rejects_the_invalid_forms():
    # k-linear e4m3 weight with PER-ROW activation scales on the fp8 tiles: the kernel would read the wrong k order
    assert plan(512, 4096, 11008, "res_norm+a8kl", 0, 8 * 512 * 4096 * 4) is None
    assert plan(128, 4096, 4096, "a8kl", 1, 0) is None
    assert plan(64, 4096, 4096, "a8kl", 0, 64 * 4096 * 4 * 8) is not None    # (weight streaming reads the k-linear twin itself)
    # out8 needs a 16-byte aligned C and ldc % 8 == 0
    ws = 8 * 512 * 22016 * 4
    assert plan(512, 22016, 4096, "glu+a8+out8", 0, ws) is not None
    assert plan(512, 22016, 4096, "glu+a8+out8", 0, ws, C_ptr=_C + 8) is None
    assert plan(512, 22016, 4096, "glu+a8+out8", 0, ws, ldc=11008 + 4) is None
    # the MX rules: block scales on the self-loading fp8 tiles only (variant 1 / auto, M > 64, a k-linear twin, a GLU with silu / gelu_tanh
    # and N / 2 % 32 == 0 for out8, no fp32 output)
    assert plan(512, 4096, 4096, "mx", 2, ws) is None
    assert plan(64, 4096, 4096, "mx", 0, ws) is None
    assert plan(512, 4096, 4096, "mx+glu", 0, ws) is None
    assert plan(512, 22016, 4096, "glu+a8+out8+f32", 0, ws) is None
    assert plan(512, 4096, 4096, "a8+out8", 0, ws) is None
    e, _ = epi_for("mx", 512, 4096, 4096)
    e.w8_klinear = 0
    out = (C.c_int * 6)()
    assert _lib.lib().cover_gemm_plan(_A, 4096, _W, _C, 4096, 512, 4096, 4096, C.byref(e), _WS, ws, 0, out) == EINVAL
    # cover_gemm_bf16's own argument checks
    e, _ = epi_for("plain", 64, 64, 64)
    assert _lib.lib().cover_gemm_plan(None, 128, _W, _C, 64, 64, 64, 64, C.byref(e), None, 0, 0, out) == EINVAL
    assert _lib.lib().cover_gemm_plan(_A, 120, _W, _C, 64, 64, 64, 64, C.byref(e), None, 0, 0, out) == EINVAL
    assert _lib.lib().cover_gemm_plan(_A, 64, _W, _C, 64, 64, 64, 200, C.byref(e), None, 0, 0, out) == EINVAL
    assert _lib.lib().cover_gemm_plan(_A, 128, _W, _C, 64, 64, 64, 64, C.byref(e), None, 0, 0, None) == EINVAL


def test_cover_gemm_plan_fp8_mfma_knob_is_read_per_call(monkeypatch):
    ws = 8 * 512 * 22016 * 4
    on = plan(512, 22016, 4096, "glu+a8", 0, ws)
    monkeypatch.setenv("COVER_FP8_MFMA", "0")
    off = plan(512, 22016, 4096, "glu+a8", 0, ws)
    monkeypatch.delenv("COVER_FP8_MFMA")
    assert on[0] == 21 and off[0] != 21


def _check(cases, expected, monkeypatch):
    assert len(cases) == len(expected)
    bad = []
    for case, want in zip(cases, expected):
        label, M, N, K, kind, variant, wsb = case[:7]
        if len(case) > 7 and case[7]:
            monkeypatch.setenv("COVER_FP8_MFMA", "0")
        else:
            monkeypatch.delenv("COVER_FP8_MFMA", raising=False)
        assert want[0] == label
        got = plan(M, N, K, kind, variant, wsb)
        if got != want[1]:
            bad.append(f"{label} (M={M} N={N} K={K} {kind} v{variant} ws={wsb}): {got} != {want[1]}")
    assert not bad, "\n".join(bad)


def test_gemm_plan_of_every_model_gemm(monkeypatch):
    _check(model_cases(), MODEL_PLANS, monkeypatch)


def test_gemm_plan_of_the_gpu_tests_shapes(monkeypatch):
    _check(gpu_test_cases(), GPU_TEST_PLANS, monkeypatch)


def test_gemm_plan_sweep(monkeypatch):
    _check(sweep_cases(), SWEEP_PLANS, monkeypatch)


# ---- the wide sweep and the once-per-process knobs. Expectations: tests/golden/gemm_plan_pinned.txt, recorded from a build of the commit BEFORE
# the planner moved to gemm_plan.hip (its library loaded through COVER_LIB_PATH), never from the tree under test. The file holds the distinct plans
# ("plan <code> <6-tuple, or - for COVER_EINVAL>"), then two characters per case: "wide" lines in wide_cases() order, one "knob" line per setting in
# KNOB_SHAPES order; "cases" is the hash of the generated inputs, so the codes cannot drift away from the cases they were recorded for.
TESTS = os.path.dirname(os.path.abspath(__file__))
WIDE_KINDS = ["plain", "bias", "gelu", "res", "res_norm", "res_ln", "f32", "glu", "glu_gelu", "w8", "res_norm+w8", "glu+w8", "a8", "res_norm+a8", "glu+a8",
              "mx", "bias+mx", "res_norm+mx", "glu+a8+out8", "glu_gelu+a8+out8", "a8kl", "res_norm+a8kl"]
# the boundaries plan_tiles's steps branch on: the 64-row streaming limit, M >= 400 / >= 512 / < 1024, 224-row padding of just over / just under
# 10 % (407 | 408, 493 | 494, 610 | 611; none: 448, all but a row: 449), the headline row counts
WIDE_M = [64, 65, 399, 400, 448, 511, 512, 704, 1023, 1024, 2624, 407, 408, 449, 493, 494, 610, 611, 672, 2232, 1, 16, 17, 32, 33]
WIDE_K = [1920, 2048, 4096, 8192, 128, 1024, 2304, 11008]                                  # (all their own Kp)
WIDE_N = [4088, 4096, 4104, 16376, 16384, 16392, 12288, 22016, 11008, 8192, 3072, 2560, 1536, 1024, 64, 32]
WS_MODES = ["none", "small", "sized", "ample"]   # absent | a byte short of two slices | cover_gemm_workspace_bytes | room for eight slices
PANEL = (1 << 31) - 4096                          # the self-loading kernels' 32-bit lane offset: M * lda * 2 (bf16) or M * ld_a8 (e4m3) below this


def ws_bytes_of(mode, M, N, K):
    sized = _lib.lib().cover_gemm_workspace_bytes(M, N, K)
    return {"none": 0, "small": 2 * M * N * 4 - 4, "sized": sized, "ample": max(sized, 8 * M * N * 4)}[mode]


def panel_ld(side, M, K, esz, gran):
    """a leading dimension (multiple of gran, >= Kp) that puts the M-row activation panel just below / just above the lane-offset limit"""
    below = (PANEL - 1) // (M * esz) // gran * gran
    return max(kp(K), below if side == "below" else below + gran)


def wide_cases(seed=20261020):
    """(M, N, K, kind, variant, ws mode, lda, ld_a8): a cross of the boundary values at variant 0, then a seeded sweep of everything"""
    out = []
    for M in WIDE_M[:18]:
        for K in WIDE_K[:4]:
            for N in (4096, 4104, 16384, 12288):
                for kind in ("plain", "res_norm", "glu", "a8", "res_norm+mx", "glu+a8+out8"):
                    for ws in ("none", "small", "ample"):
                        out.append((M, N, K, kind, 0, ws, kp(K), kp(K)))
    rnd = random.Random(seed)
    for _ in range(3000):
        kind = rnd.choice(WIDE_KINDS)
        M = rnd.choice(WIDE_M) if rnd.random() < 0.7 else rnd.randint(1, 2700)
        K = rnd.choice(WIDE_K) if rnd.random() < 0.7 else 128 * rnd.randint(1, 90) - rnd.choice([0, 0, 64])
        N = rnd.choice(WIDE_N) if rnd.random() < 0.6 else 8 * rnd.randint(1, 2800)
        if "glu" in kind:
            N = max(32, N // 32 * 32)
        variant = rnd.choice([0, 0, 0, 1, 1, 2, 3, 5, 6])
        lda = ld_a8 = kp(K)
        if M > 64 and rnd.random() < 0.15:      # the activation panel on both sides of the 2^31-byte limit
            lda = panel_ld(rnd.choice(["below", "above"]), M, K, 2, 8)
        if M > 64 and rnd.random() < 0.15:
            ld_a8 = panel_ld(rnd.choice(["below", "above"]), M, K, 1, 16)
        out.append((M, N, K, kind, variant, rnd.choice(WS_MODES), lda, ld_a8))
    return out


def plan_text(case):
    M, N, K, kind, variant, ws, lda, ld_a8 = case
    got = plan(M, N, K, kind, variant, ws_bytes_of(ws, M, N, K), lda=lda, ld_a8=ld_a8)
    return "-" if got is None else " ".join(str(x) for x in got)


def pinned():
    """(plan of each wide case, {setting: plan of each knob shape}) as recorded"""
    plans, wide, knobs = {}, "", {}
    with open(os.path.join(TESTS, "golden", "gemm_plan_pinned.txt")) as f:
        for line in f.read().splitlines():
            tag, rest = line.split(" ", 1)
            if tag == "cases":
                assert rest == hashlib.sha256(repr((wide_cases(), KNOB_SHAPES)).encode()).hexdigest(), "the cases are not the recorded ones"
            elif tag == "plan":
                plans[rest[:2]] = rest[3:]
            elif tag == "wide":
                wide += rest
            else:
                knobs[tuple(rest.split(" ")[0].split("="))] = rest.split(" ")[1]
    unpack = lambda codes: [plans[codes[i:i + 2]] for i in range(0, len(codes), 2)]   # noqa: E731
    return unpack(wide), {k: unpack(v) for k, v in knobs.items()}


def differing(cases, got, want):
    assert len(cases) == len(got) == len(want)
    return [f"{c}: {g}   (recorded: {w})" for c, g, w in zip(cases, got, want) if g != w]


def test_gemm_plan_wide_sweep(monkeypatch):
    monkeypatch.delenv("COVER_FP8_MFMA", raising=False)
    cases = wide_cases()
    assert len(cases) >= 5000
    bad = differing(cases, [plan_text(c) for c in cases], pinned()[0])
    assert not bad, f"{len(bad)} plans differ:\n" + "\n".join(bad[:40])


# (M, N, K, kind, variant, ws mode): 224-row, 256-row and small tiles, fp8 / MX forms, the A/B variant, weight streaming of all generations
KNOB_SHAPES = [
    (448, 12288, 4096, "plain", 0, "sized"), (448, 4096, 4096, "res_norm", 0, "sized"), (448, 4096, 11008, "res_norm", 0, "none"),
    (448, 22016, 4096, "glu", 0, "sized"), (448, 3072, 2048, "plain", 0, "ample"), (2232, 2560, 2048, "plain", 0, "sized"),
    (704, 12288, 4096, "bias", 0, "sized"), (704, 4096, 11008, "res_norm", 0, "sized"), (2624, 32768, 2048, "glu_gelu", 0, "none"),
    (200, 4096, 4096, "res_norm", 0, "sized"), (261, 1024, 4096, "res_ln", 0, "sized"), (576, 4096, 1024, "gelu", 0, "sized"),
    (2048, 4608, 1152, "bias", 0, "none"), (1024, 8192, 2304, "plain", 1, "ample"), (448, 4096, 4096, "res_norm", 2, "sized"),
    (300, 1024, 1024, "plain", 2, "ample"), (512, 12288, 4096, "a8", 0, "sized"), (512, 22016, 4096, "glu+a8", 0, "sized"),
    (512, 22016, 4096, "glu+a8+out8", 0, "sized"), (512, 4096, 11008, "res_norm+mx", 0, "sized"), (448, 4096, 11008, "res_norm+a8", 0, "sized"),
    (448, 22016, 4096, "glu+a8", 0, "sized"), (200, 4096, 4096, "bias+mx", 0, "sized"), (1024, 8192, 2304, "bias+a8", 0, "sized"),
    (530, 1040, 2304, "bias+a8", 0, "ample"), (16, 12288, 4096, "plain", 0, "sized"), (32, 4096, 11008, "res_norm+w8", 0, "sized"),
    (64, 32064, 4096, "f32", 0, "sized"), (48, 1024, 2048, "plain", 0, "sized"), (16, 22016, 4096, "glu", 3, "sized"),
    (32, 4096, 4096, "plain", 5, "sized"), (16, 4096, 4096, "plain", 6, "sized"),
]
KNOB_SETTINGS = ([("COVER_TILE_PICK", c) for c in "345678abcdefghinopqru"] + [("COVER_TILE_SPLIT", s) for s in "124"] +
                 [("COVER_V3_F8", "0"), ("COVER_SKINNY3", "0"), ("COVER_SK_SLOTS", "256")])
KNOBS = ("COVER_TILE_PICK", "COVER_TILE_SPLIT", "COVER_V3_F8", "COVER_SKINNY3", "COVER_SK_SLOTS", "COVER_FP8_MFMA")


@pytest.fixture(scope="module")
def knob_children():
    """one fresh child per setting (the knobs are read once per process), eight at a time; the children only plan: no GPU call"""
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    cmd = [sys.executable, "-c", "from tests.test_gemm_plan_cpu import *\nfor s in KNOB_SHAPES: print(plan_text(s + (kp(s[2]), kp(s[2]))))"]
    root = os.path.dirname(TESTS)
    def child(kv):
        p = subprocess.run(cmd, cwd=root, env=dict(base, **{kv[0]: kv[1]}), capture_output=True, text=True)
        return p.stdout, p.stderr, p.returncode
    with ThreadPoolExecutor(8) as pool:
        return dict(zip(KNOB_SETTINGS, pool.map(child, KNOB_SETTINGS)))


@pytest.mark.parametrize("setting", KNOB_SETTINGS, ids=lambda kv: "=".join(kv))
def test_gemm_plan_under_a_once_per_process_knob(knob_children, setting):
    stdout, stderr, rc = knob_children[setting]
    assert rc == 0, stderr
    bad = differing(KNOB_SHAPES, stdout.splitlines(), pinned()[1][setting])
    assert not bad, "\n".join(bad)


def test_gemm_workspace_bytes_unchanged():
    h = _lib.lib()
    got = [h.cover_gemm_workspace_bytes(M, N, K) for M, N, K in WORKSPACE_SHAPES]
    assert got == WORKSPACE_BYTES


# ---- the pass workspaces (forward.hip: dec_ws / vit_ws). The tables were recorded from the library as it was when both layouts were still carved
# through out-parameters in capi.hip, so they pin the parent's sizes. Only the scalar geometry of a desc is read: no device, no layer array.
DEC_WS_ROWS = (1, 16, 64, 65, 200, 512)   # 65 crosses the rows > 64 boundary behind which the fp8 buffers are used
DEC_WS_BYTES = {   # (dim, Hq, Hkv, D, mlp): synth.OPENVLA_SMALL, the tests' TINY pi0 (prefix, expert), synth.OPENVLA_7B, synth.PI0_FULL (prefix, expert)
    (256, 4, 4, 64, 512): [14336, 214272, 855552, 2467072, 7588608, 19425536],
    (256, 4, 1, 64, 512): [13568, 201984, 806400, 2417152, 7435008, 19032320],
    (128, 4, 1, 64, 256): [6400, 87296, 347136, 1285120, 3951872, 10115328],
    (4096, 32, 32, 128, 11008): [620032, 9910272, 50911232, 51707136, 159097344, 113686784],
    (2048, 8, 1, 256, 16384): [596224, 9528832, 38113792, 9955840, 30631680, 78416128],
    (1024, 8, 1, 256, 4096): [294912, 4705792, 18821632, 19116288, 58817280, 58296576],
}
VIT_WS_SHAPES = ((1, 32), (2, 33), (4, 256))   # (n_seq, T); T = 33: the V^T scratch is padded to tcap = 64 != T
VIT_WS_BYTES = {   # (dim, heads, head_dim_p, mlp_p): the SigLIP tower of synth.OPENVLA_SMALL, SigLIP-So400m (synth.OPENVLA_7B / PI0_FULL)
    (128, 2, 64, 256): [114944, 962304, 14680320],
    (1152, 16, 96, 4352): [6152448, 11663104, 177996032],
}


def test_pass_workspace_bytes_unchanged():
    h = _lib.lib()
    for (dim, Hq, Hkv, D, mlp), want in DEC_WS_BYTES.items():
        d = _lib.DecDesc()
        d.dim, d.Hq, d.Hkv, d.D, d.mlp = dim, Hq, Hkv, D, mlp
        assert [h.cover_decoder_workspace_bytes(C.byref(d), r) for r in DEC_WS_ROWS] == want, (dim, Hq, Hkv, D, mlp)
    for (dim, heads, dp, mlp_p), want in VIT_WS_BYTES.items():
        d = _lib.VitDesc()
        d.dim, d.heads, d.head_dim_p, d.mlp_p = dim, heads, dp, mlp_p
        assert [h.cover_vit_workspace_bytes(C.byref(d), n, T) for n, T in VIT_WS_SHAPES] == want, (dim, heads, dp, mlp_p)


# ---- recorded from the planner before it was split from the launch code: (label, plan or None for COVER_EINVAL)
MODEL_PLANS = [
    ('openvla M=448 qkv', (30, 30, 0, 1, 0, 0)),
    ('openvla M=448 o', (24, 24, 0, 4, 2, 0)),
    ('openvla M=448 gate_up', (23, 23, 0, 1, 0, 0)),
    ('openvla M=448 down', (24, 24, 0, 4, 2, 0)),
    ('openvla M=704 qkv', (26, 26, 0, 1, 0, 0)),
    ('openvla M=704 o', (10, 10, 0, 1, 0, 1)),
    ('openvla M=704 gate_up', (25, 25, 0, 1, 0, 0)),
    ('openvla M=704 down', (25, 25, 0, 2, 2, 0)),
    ('openvla M=32 qkv', (20, -1, 0, 2, 1, 0)),
    ('openvla M=32 o', (19, -1, 0, 4, 2, 0)),
    ('openvla M=32 gate_up', (20, -1, 0, 1, 0, 0)),
    ('openvla M=32 down', (20, -1, 0, 4, 2, 0)),
    ('openvla M=16 qkv', (20, -1, 0, 2, 1, 0)),
    ('openvla M=16 o', (19, -1, 0, 4, 2, 0)),
    ('openvla M=16 gate_up', (20, -1, 0, 1, 0, 0)),
    ('openvla M=16 down', (20, -1, 0, 4, 2, 0)),
    ('config5 M=512 qkv', (21, 18, 1, 1, 0, 0)),
    ('config5 M=512 o', (21, 10, 0, 1, 0, 1)),
    ('config5 M=512 gate_up', (21, 18, 1, 1, 0, 0)),
    ('config5 M=512 down', (21, 12, 1, 4, 2, 0)),
    ('config5 M=512 fp8-mfma off qkv', (26, 26, 0, 1, 0, 0)),
    ('config5 M=512 fp8-mfma off o', None),
    ('config5 M=512 fp8-mfma off gate_up', None),
    ('config5 M=512 fp8-mfma off down', None),
    ('config5 gate_up per-row', (21, 18, 1, 1, 0, 0)),
    ('config5 gate_up per-row fp8-mfma off', (25, 25, 0, 1, 0, 0)),
    ('e4m3 stream M=16 qkv', (20, -1, 0, 2, 1, 0)),
    ('e4m3 stream M=16 o', (19, -1, 0, 4, 2, 0)),
    ('e4m3 stream M=16 gate_up', (20, -1, 0, 1, 0, 0)),
    ('e4m3 stream M=16 down', (20, -1, 0, 4, 2, 0)),
    ('e4m3 stream M=32 qkv', (20, -1, 0, 2, 1, 0)),
    ('e4m3 stream M=32 o', (19, -1, 0, 4, 2, 0)),
    ('e4m3 stream M=32 gate_up', (20, -1, 0, 1, 0, 0)),
    ('e4m3 stream M=32 down', (20, -1, 0, 4, 2, 0)),
    ('openvla lm_head M=16', (20, -1, 0, 1, 0, 0)),
    ('openvla lm_head M=32', (20, -1, 0, 1, 0, 0)),
    ('openvla lm_head M=64', (19, -1, 0, 8, 1, 0)),
    ('pi0 prefix M=2624 qkv', (24, 24, 0, 1, 0, 0)),
    ('pi0 prefix M=2624 o', (24, 24, 0, 1, 0, 1)),
    ('pi0 prefix M=2624 gate_up', (23, 23, 0, 1, 0, 0)),
    ('pi0 prefix M=2624 down', (24, 24, 0, 1, 0, 1)),
    ('pi0 expert M=200 qkv', (2, 2, 0, 2, 1, 0)),
    ('pi0 expert M=200 o', (2, 2, 0, 4, 2, 0)),
    ('pi0 expert M=200 gate_up', (2, 2, 0, 1, 0, 0)),
    ('pi0 expert M=200 down', (2, 2, 0, 4, 2, 0)),
    ('dinov2 R=261 qkv', (2, 2, 0, 1, 0, 0)),
    ('dinov2 R=261 proj', (2, 2, 0, 2, 2, 0)),
    ('dinov2 R=261 fc1', (2, 2, 0, 1, 0, 0)),
    ('dinov2 R=261 fc2', (2, 2, 0, 4, 2, 0)),
    ('siglip R=256 qkv', (2, 2, 0, 1, 0, 0)),
    ('siglip R=256 proj', (2, 2, 0, 2, 2, 0)),
    ('siglip R=256 fc1', (2, 2, 0, 1, 0, 0)),
    ('siglip R=256 fc2', (2, 2, 0, 4, 2, 0)),
    ('siglip R=2048 qkv', (1, 1, 0, 1, 0, 0)),
    ('siglip R=2048 proj', (2, 2, 0, 1, 0, 1)),
    ('siglip R=2048 fc1', (1, 1, 0, 1, 0, 0)),
    ('siglip R=2048 fc2', (30, 30, 0, 2, 2, 0)),
    ('siglip2 R=576 qkv', (2, 2, 0, 1, 0, 0)),
    ('siglip2 R=576 proj', (2, 2, 0, 2, 2, 0)),
    ('siglip2 R=576 fc1', (2, 2, 0, 1, 0, 0)),
    ('siglip2 R=576 fc2', (2, 2, 0, 2, 2, 0)),
]
GPU_TEST_PLANS = [
    ('gpu test M=448 N=12288 K=4096 bias+res', (30, 30, 0, 1, 0, 0)),
    ('gpu test M=448 N=12288 K=4096 f32', (30, 30, 0, 1, 0, 0)),
    ('gpu test M=440 N=12272 K=4160 bias+res', (30, 30, 0, 1, 0, 0)),
    ('gpu test M=448 N=3072 K=2048 plain', (30, 30, 0, 4, 1, 0)),
    ('gpu test M=2232 N=2560 K=2048 plain', (24, 24, 0, 1, 0, 0)),
    ('gpu test M=672 N=1536 K=4096 res_norm', (30, 30, 0, 4, 2, 0)),
    ('gpu test M=448 N=22016 K=4096 glu', (23, 23, 0, 1, 0, 0)),
    ('gpu test M=448 N=4096 K=4096 res_norm', (24, 24, 0, 4, 2, 0)),
    ('gpu test M=448 N=4096 K=11008 res_norm', (24, 24, 0, 4, 2, 0)),
    ('gpu test M=512 N=4096 K=11008 bias+res_norm+mx', (21, 12, 1, 4, 2, 0)),
    ('gpu test M=512 N=4096 K=11008 bias+res_norm+a8', (21, 12, 1, 4, 2, 0)),
    ('gpu test M=448 N=4096 K=11008 bias+res_norm+mx', (21, 15, 1, 4, 2, 0)),
    ('gpu test M=448 N=4096 K=11008 bias+res_norm+a8', (21, 15, 1, 4, 2, 0)),
    ('gpu test M=200 N=4096 K=4096 bias+mx', (21, 13, 1, 8, 1, 0)),
    ('gpu test M=200 N=4096 K=4096 bias+a8', (2, 2, 0, 1, 0, 0)),
    ('gpu test M=530 N=1040 K=2304 bias+mx', (21, 13, 1, 4, 1, 0)),
    ('gpu test M=530 N=1040 K=2304 bias+a8', (2, 2, 0, 2, 1, 0)),
    ('gpu test M=1024 N=8192 K=2304 bias+mx', (21, 15, 1, 1, 0, 0)),
    ('gpu test M=1024 N=8192 K=2304 bias+a8', (21, 17, 0, 1, 0, 0)),
    ('gpu test M=512 N=22016 K=4096 glu+a8', (21, 18, 1, 1, 0, 0)),
    ('gpu test M=512 N=22016 K=4096 glu+a8+out8', (21, 18, 1, 1, 0, 0)),
    ('gpu test M=448 N=22016 K=4096 glu+a8', (21, 17, 0, 1, 0, 0)),
    ('gpu test M=448 N=22016 K=4096 glu+a8+out8', (21, 15, 1, 1, 0, 0)),
    ('gpu test M=300 N=4160 K=2304 glu_gelu+a8', (2, 2, 0, 1, 0, 0)),
    ('gpu test M=300 N=4160 K=2304 glu_gelu+a8+out8', (21, 13, 1, 1, 0, 0)),
    ('gpu test mx decoder qkv', (21, 17, 0, 1, 0, 0)),
    ('gpu test mx decoder o', (21, 15, 1, 4, 2, 0)),
    ('gpu test mx decoder gate_up', (21, 15, 1, 1, 0, 0)),
    ('gpu test mx decoder gate_up unfused', (21, 17, 0, 1, 0, 0)),
    ('gpu test mx decoder down', (21, 15, 1, 8, 2, 0)),
]
SWEEP_PLANS = [
    ('sweep 0', (1, 1, 0, 1, 0, 1)),
    ('sweep 1', None),
    ('sweep 2', (19, -1, 0, 4, 1, 0)),
    ('sweep 3', (2, 2, 0, 1, 0, 0)),
    ('sweep 4', None),
    ('sweep 5', None),
    ('sweep 6', (19, -1, 0, 1, 1, 0)),
    ('sweep 7', None),
    ('sweep 8', (22, -1, 0, 17, 1, 0)),
    ('sweep 9', (22, -1, 0, 6, 1, 0)),
    ('sweep 10', None),
    ('sweep 11', (2, 2, 0, 1, 0, 0)),
    ('sweep 12', (2, 2, 0, 1, 0, 1)),
    ('sweep 13', (2, 2, 0, 1, 0, 0)),
    ('sweep 14', (20, -1, 0, 2, 1, 0)),
    ('sweep 15', None),
    ('sweep 16', (1, 1, 0, 1, 0, 0)),
    ('sweep 17', (19, -1, 0, 4, 1, 1)),
    ('sweep 18', (2, 2, 0, 2, 1, 0)),
    ('sweep 19', (2, 2, 0, 1, 0, 0)),
    ('sweep 20', (22, -1, 0, 2, 1, 0)),
    ('sweep 21', None),
    ('sweep 22', (19, -1, 0, 4, 2, 0)),
    ('sweep 23', (2, 2, 0, 8, 1, 0)),
    ('sweep 24', (22, -1, 0, 3, 1, 1)),
    ('sweep 25', (2, 2, 0, 8, 1, 0)),
    ('sweep 26', (0, 0, 0, 1, 0, 0)),
    ('sweep 27', None),
    ('sweep 28', (1, 1, 0, 1, 0, 0)),
    ('sweep 29', (1, 1, 0, 1, 0, 0)),
    ('sweep 30', None),
    ('sweep 31', None),
    ('sweep 32', (21, 13, 1, 2, 1, 0)),
    ('sweep 33', (19, -1, 0, 22, 1, 0)),
    ('sweep 34', (22, -1, 0, 1, 1, 0)),
    ('sweep 35', None),
    ('sweep 36', (1, 1, 0, 1, 0, 0)),
    ('sweep 37', (22, -1, 0, 11, 1, 0)),
    ('sweep 38', (10, 10, 0, 1, 0, 0)),
    ('sweep 39', (2, 2, 0, 2, 1, 0)),
    ('sweep 40', (1, 1, 0, 1, 0, 0)),
    ('sweep 41', (26, 26, 0, 1, 0, 1)),
    ('sweep 42', (2, 2, 0, 1, 0, 0)),
    ('sweep 43', None),
    ('sweep 44', None),
    ('sweep 45', (2, 2, 0, 8, 1, 0)),
    ('sweep 46', (1, 1, 0, 1, 0, 0)),
    ('sweep 47', (2, 2, 0, 2, 2, 0)),
    ('sweep 48', None),
    ('sweep 49', (10, 10, 0, 1, 0, 1)),
    ('sweep 50', (19, -1, 0, 3, 1, 0)),
    ('sweep 51', None),
    ('sweep 52', None),
    ('sweep 53', (1, 1, 0, 1, 0, 0)),
    ('sweep 54', (19, -1, 0, 1, 1, 0)),
    ('sweep 55', (2, 2, 0, 1, 0, 0)),
    ('sweep 56', (2, 2, 0, 2, 1, 0)),
    ('sweep 57', None),
    ('sweep 58', (2, 2, 0, 1, 0, 0)),
    ('sweep 59', (2, 2, 0, 1, 0, 0)),
    ('sweep 60', (2, 2, 0, 2, 1, 1)),
    ('sweep 61', None),
    ('sweep 62', (2, 2, 0, 1, 0, 0)),
    ('sweep 63', (1, 1, 0, 1, 0, 1)),
    ('sweep 64', (2, 2, 0, 1, 0, 0)),
    ('sweep 65', (1, 1, 0, 1, 0, 0)),
    ('sweep 66', (21, 13, 1, 1, 0, 1)),
    ('sweep 67', None),
    ('sweep 68', (2, 2, 0, 1, 0, 1)),
    ('sweep 69', None),
    ('sweep 70', (1, 1, 0, 1, 0, 1)),
    ('sweep 71', None),
    ('sweep 72', (2, 2, 0, 1, 0, 0)),
    ('sweep 73', None),
    ('sweep 74', (2, 2, 0, 1, 0, 0)),
    ('sweep 75', (2, 2, 0, 1, 0, 1)),
    ('sweep 76', (2, 2, 0, 1, 0, 0)),
    ('sweep 77', (1, 1, 0, 1, 0, 0)),
    ('sweep 78', (2, 2, 0, 1, 0, 0)),
    ('sweep 79', (21, 13, 1, 1, 0, 0)),
    ('sweep 80', (1, 1, 0, 1, 0, 0)),
    ('sweep 81', (19, -1, 0, 2, 1, 0)),
    ('sweep 82', (21, 13, 1, 1, 0, 0)),
    ('sweep 83', (2, 2, 0, 4, 1, 0)),
    ('sweep 84', None),
    ('sweep 85', (2, 2, 0, 2, 2, 0)),
    ('sweep 86', None),
    ('sweep 87', (1, 1, 0, 1, 0, 1)),
    ('sweep 88', (1, 1, 0, 1, 0, 0)),
    ('sweep 89', None),
    ('sweep 90', (19, -1, 0, 11, 1, 1)),
    ('sweep 91', (2, 2, 0, 1, 0, 0)),
    ('sweep 92', (2, 2, 0, 1, 0, 0)),
    ('sweep 93', None),
    ('sweep 94', (21, 12, 1, 1, 0, 1)),
    ('sweep 95', (2, 2, 0, 1, 0, 0)),
    ('sweep 96', (2, 2, 0, 1, 0, 0)),
    ('sweep 97', (2, 2, 0, 1, 0, 1)),
    ('sweep 98', (2, 2, 0, 8, 2, 0)),
    ('sweep 99', (2, 2, 0, 1, 0, 0)),
    ('sweep 100', (19, -1, 0, 5, 1, 0)),
    ('sweep 101', None),
    ('sweep 102', (1, 1, 0, 1, 0, 1)),
    ('sweep 103', None),
    ('sweep 104', None),
    ('sweep 105', (2, 2, 0, 1, 0, 0)),
    ('sweep 106', (2, 2, 0, 1, 0, 0)),
    ('sweep 107', None),
    ('sweep 108', (2, 2, 0, 1, 0, 1)),
    ('sweep 109', None),
    ('sweep 110', (10, 10, 0, 1, 0, 0)),
    ('sweep 111', (2, 2, 0, 1, 0, 0)),
    ('sweep 112', None),
    ('sweep 113', (2, 2, 0, 1, 0, 0)),
    ('sweep 114', (1, 1, 0, 1, 0, 0)),
    ('sweep 115', None),
    ('sweep 116', (26, 26, 0, 1, 0, 0)),
    ('sweep 117', (1, 1, 0, 1, 0, 0)),
    ('sweep 118', (20, -1, 0, 3, 2, 0)),
    ('sweep 119', (2, 2, 0, 1, 0, 0)),
    ('sweep 120', (2, 2, 0, 1, 0, 0)),
    ('sweep 121', None),
    ('sweep 122', (19, -1, 0, 2, 1, 0)),
    ('sweep 123', (21, 13, 1, 1, 0, 0)),
    ('sweep 124', (19, -1, 0, 1, 1, 0)),
    ('sweep 125', (21, 13, 1, 1, 0, 0)),
    ('sweep 126', (2, 2, 0, 1, 0, 0)),
    ('sweep 127', (19, -1, 0, 2, 1, 0)),
    ('sweep 128', None),
    ('sweep 129', (22, -1, 0, 9, 1, 0)),
    ('sweep 130', (30, 30, 0, 4, 1, 0)),
    ('sweep 131', (2, 2, 0, 1, 0, 1)),
    ('sweep 132', (2, 2, 0, 1, 0, 0)),
    ('sweep 133', None),
    ('sweep 134', (0, 0, 0, 1, 0, 0)),
    ('sweep 135', None),
    ('sweep 136', (2, 2, 0, 1, 0, 1)),
    ('sweep 137', (2, 2, 0, 1, 0, 1)),
    ('sweep 138', None),
    ('sweep 139', (1, 1, 0, 1, 0, 0)),
    ('sweep 140', (2, 2, 0, 1, 0, 1)),
    ('sweep 141', (21, 12, 1, 1, 0, 1)),
    ('sweep 142', None),
    ('sweep 143', (2, 2, 0, 2, 1, 0)),
    ('sweep 144', None),
    ('sweep 145', (2, 2, 0, 1, 0, 0)),
    ('sweep 146', (20, -1, 0, 2, 2, 0)),
    ('sweep 147', None),
    ('sweep 148', (19, -1, 0, 2, 1, 0)),
    ('sweep 149', (2, 2, 0, 1, 0, 0)),
    ('sweep 150', None),
    ('sweep 151', None),
    ('sweep 152', None),
    ('sweep 153', (2, 2, 0, 1, 0, 0)),
    ('sweep 154', (1, 1, 0, 1, 0, 0)),
    ('sweep 155', (21, 13, 1, 1, 0, 0)),
    ('sweep 156', (21, 12, 1, 1, 0, 0)),
    ('sweep 157', (30, 30, 0, 2, 1, 0)),
    ('sweep 158', None),
    ('sweep 159', None),
    ('sweep 160', (1, 1, 0, 1, 0, 0)),
    ('sweep 161', None),
    ('sweep 162', None),
    ('sweep 163', (2, 2, 0, 2, 1, 0)),
    ('sweep 164', None),
    ('sweep 165', (26, 26, 0, 1, 0, 0)),
    ('sweep 166', (2, 2, 0, 1, 0, 0)),
    ('sweep 167', None),
    ('sweep 168', None),
    ('sweep 169', (2, 2, 0, 1, 0, 0)),
    ('sweep 170', None),
    ('sweep 171', (2, 2, 0, 1, 0, 0)),
    ('sweep 172', (19, -1, 0, 2, 1, 0)),
    ('sweep 173', None),
    ('sweep 174', (21, 12, 1, 1, 0, 1)),
    ('sweep 175', (2, 2, 0, 4, 1, 0)),
    ('sweep 176', (2, 2, 0, 8, 1, 0)),
    ('sweep 177', None),
    ('sweep 178', (20, -1, 0, 3, 1, 0)),
    ('sweep 179', (2, 2, 0, 4, 1, 0)),
    ('sweep 180', (2, 2, 0, 1, 0, 0)),
    ('sweep 181', (10, 10, 0, 1, 0, 1)),
    ('sweep 182', (2, 2, 0, 1, 0, 0)),
    ('sweep 183', (2, 2, 0, 1, 0, 0)),
    ('sweep 184', (21, 15, 1, 1, 0, 1)),
    ('sweep 185', (21, 13, 1, 1, 0, 0)),
    ('sweep 186', None),
    ('sweep 187', (1, 1, 0, 1, 0, 0)),
    ('sweep 188', None),
    ('sweep 189', None),
    ('sweep 190', None),
    ('sweep 191', None),
    ('sweep 192', (2, 2, 0, 1, 0, 1)),
    ('sweep 193', (2, 2, 0, 1, 0, 0)),
    ('sweep 194', (22, -1, 0, 43, 1, 0)),
    ('sweep 195', (20, -1, 0, 2, 1, 0)),
    ('sweep 196', (19, -1, 0, 4, 1, 0)),
    ('sweep 197', (1, 1, 0, 1, 0, 0)),
    ('sweep 198', (19, -1, 0, 8, 1, 0)),
    ('sweep 199', (2, 2, 0, 1, 0, 1)),
    ('sweep 200', None),
    ('sweep 201', None),
    ('sweep 202', (10, 10, 0, 1, 0, 0)),
    ('sweep 203', (20, -1, 0, 5, 1, 0)),
    ('sweep 204', None),
    ('sweep 205', (2, 2, 0, 1, 0, 0)),
    ('sweep 206', None),
    ('sweep 207', (2, 2, 0, 2, 1, 0)),
    ('sweep 208', None),
    ('sweep 209', (21, 13, 1, 1, 0, 0)),
    ('sweep 210', None),
    ('sweep 211', (2, 2, 0, 1, 0, 0)),
    ('sweep 212', None),
    ('sweep 213', None),
    ('sweep 214', (2, 2, 0, 4, 1, 0)),
    ('sweep 215', (19, -1, 0, 11, 1, 0)),
    ('sweep 216', (19, -1, 0, 1, 1, 0)),
    ('sweep 217', (2, 2, 0, 1, 0, 0)),
    ('sweep 218', (2, 2, 0, 1, 0, 1)),
    ('sweep 219', (1, 1, 0, 1, 0, 1)),
    ('sweep 220', (21, 13, 1, 1, 0, 1)),
    ('sweep 221', (1, 1, 0, 1, 0, 0)),
    ('sweep 222', (2, 2, 0, 1, 0, 0)),
    ('sweep 223', (2, 2, 0, 2, 1, 0)),
    ('sweep 224', (2, 2, 0, 1, 0, 1)),
    ('sweep 225', (1, 1, 0, 1, 0, 0)),
    ('sweep 226', (2, 2, 0, 1, 0, 0)),
    ('sweep 227', (2, 2, 0, 1, 0, 1)),
    ('sweep 228', None),
    ('sweep 229', (21, 13, 1, 2, 1, 0)),
    ('sweep 230', (20, -1, 0, 1, 0, 1)),
    ('sweep 231', (2, 2, 0, 1, 0, 1)),
    ('sweep 232', None),
    ('sweep 233', (2, 2, 0, 1, 0, 0)),
    ('sweep 234', (21, 13, 1, 4, 1, 0)),
    ('sweep 235', None),
    ('sweep 236', None),
    ('sweep 237', (21, 13, 1, 1, 0, 0)),
    ('sweep 238', None),
    ('sweep 239', (1, 1, 0, 1, 0, 1)),
    ('sweep 240', (2, 2, 0, 1, 0, 0)),
    ('sweep 241', (19, -1, 0, 11, 1, 0)),
    ('sweep 242', (2, 2, 0, 1, 0, 0)),
    ('sweep 243', (21, 13, 1, 1, 0, 0)),
    ('sweep 244', (19, -1, 0, 4, 1, 0)),
    ('sweep 245', (30, 30, 0, 8, 1, 0)),
    ('sweep 246', (19, -1, 0, 4, 1, 0)),
    ('sweep 247', None),
    ('sweep 248', (2, 2, 0, 1, 0, 0)),
    ('sweep 249', (1, 1, 0, 1, 0, 1)),
    ('sweep 250', (1, 1, 0, 1, 0, 0)),
    ('sweep 251', (19, -1, 0, 1, 1, 0)),
    ('sweep 252', (2, 2, 0, 1, 0, 0)),
    ('sweep 253', None),
    ('sweep 254', None),
    ('sweep 255', None),
    ('sweep 256', (23, 23, 0, 1, 0, 0)),
    ('sweep 257', None),
    ('sweep 258', (2, 2, 0, 1, 0, 0)),
    ('sweep 259', (0, 0, 0, 1, 0, 1)),
    ('sweep 260', (1, 1, 0, 1, 0, 0)),
    ('sweep 261', (0, 0, 0, 1, 0, 0)),
    ('sweep 262', (2, 2, 0, 1, 0, 0)),
    ('sweep 263', (0, 0, 0, 1, 0, 0)),
    ('sweep 264', (1, 1, 0, 1, 0, 0)),
    ('sweep 265', (21, 18, 1, 1, 0, 1)),
    ('sweep 266', None),
    ('sweep 267', (1, 1, 0, 1, 0, 0)),
    ('sweep 268', (2, 2, 0, 2, 1, 0)),
    ('sweep 269', (2, 2, 0, 1, 0, 0)),
    ('sweep 270', (26, 26, 0, 1, 0, 1)),
    ('sweep 271', (2, 2, 0, 1, 0, 0)),
    ('sweep 272', (2, 2, 0, 1, 0, 0)),
    ('sweep 273', None),
    ('sweep 274', (2, 2, 0, 1, 0, 0)),
    ('sweep 275', None),
    ('sweep 276', (21, 13, 1, 1, 0, 1)),
    ('sweep 277', None),
    ('sweep 278', (2, 2, 0, 1, 0, 0)),
    ('sweep 279', None),
    ('sweep 280', None),
    ('sweep 281', (19, -1, 0, 1, 1, 0)),
    ('sweep 282', None),
    ('sweep 283', (2, 2, 0, 1, 0, 0)),
    ('sweep 284', (1, 1, 0, 1, 0, 0)),
    ('sweep 285', None),
    ('sweep 286', None),
    ('sweep 287', (2, 2, 0, 2, 2, 0)),
    ('sweep 288', (22, -1, 0, 22, 1, 0)),
    ('sweep 289', None),
    ('sweep 290', (22, -1, 0, 16, 2, 0)),
    ('sweep 291', None),
    ('sweep 292', None),
    ('sweep 293', None),
    ('sweep 294', (21, 13, 1, 1, 0, 0)),
    ('sweep 295', None),
    ('sweep 296', None),
    ('sweep 297', (1, 1, 0, 1, 0, 0)),
    ('sweep 298', None),
    ('sweep 299', (21, 13, 1, 2, 1, 0)),
    ('sweep 300', None),
    ('sweep 301', (19, -1, 0, 8, 1, 1)),
    ('sweep 302', None),
    ('sweep 303', None),
    ('sweep 304', (2, 2, 0, 1, 0, 1)),
    ('sweep 305', None),
    ('sweep 306', None),
    ('sweep 307', (1, 1, 0, 1, 0, 0)),
    ('sweep 308', None),
    ('sweep 309', None),
    ('sweep 310', (2, 2, 0, 1, 0, 1)),
    ('sweep 311', None),
    ('sweep 312', (2, 2, 0, 1, 0, 0)),
    ('sweep 313', (2, 2, 0, 1, 0, 0)),
    ('sweep 314', (19, -1, 0, 3, 1, 0)),
    ('sweep 315', None),
    ('sweep 316', None),
    ('sweep 317', (19, -1, 0, 8, 1, 0)),
    ('sweep 318', (23, 23, 0, 2, 1, 0)),
    ('sweep 319', (19, -1, 0, 5, 1, 0)),
    ('sweep 320', (22, -1, 0, 8, 1, 0)),
    ('sweep 321', None),
    ('sweep 322', (2, 2, 0, 1, 0, 0)),
    ('sweep 323', None),
    ('sweep 324', None),
    ('sweep 325', (22, -1, 0, 3, 2, 0)),
    ('sweep 326', (2, 2, 0, 1, 0, 0)),
    ('sweep 327', (1, 1, 0, 1, 0, 1)),
    ('sweep 328', (21, 13, 1, 7, 2, 0)),
    ('sweep 329', None),
    ('sweep 330', None),
    ('sweep 331', None),
    ('sweep 332', (21, 10, 0, 1, 0, 0)),
    ('sweep 333', (2, 2, 0, 4, 1, 0)),
    ('sweep 334', (22, -1, 0, 6, 1, 1)),
    ('sweep 335', None),
    ('sweep 336', (19, -1, 0, 4, 1, 0)),
    ('sweep 337', None),
    ('sweep 338', (2, 2, 0, 8, 1, 0)),
    ('sweep 339', (30, 30, 0, 4, 1, 0)),
    ('sweep 340', (2, 2, 0, 1, 0, 0)),
    ('sweep 341', (1, 1, 0, 1, 0, 1)),
    ('sweep 342', (1, 1, 0, 1, 0, 1)),
    ('sweep 343', None),
    ('sweep 344', (19, -1, 0, 2, 1, 0)),
    ('sweep 345', None),
    ('sweep 346', (2, 2, 0, 1, 0, 0)),
    ('sweep 347', None),
    ('sweep 348', (2, 2, 0, 1, 0, 1)),
    ('sweep 349', (26, 26, 0, 1, 0, 1)),
    ('sweep 350', (2, 2, 0, 1, 0, 1)),
    ('sweep 351', None),
    ('sweep 352', None),
    ('sweep 353', None),
    ('sweep 354', (1, 1, 0, 1, 0, 0)),
    ('sweep 355', (19, -1, 0, 2, 1, 0)),
    ('sweep 356', (1, 1, 0, 1, 0, 0)),
    ('sweep 357', None),
    ('sweep 358', (2, 2, 0, 1, 0, 0)),
    ('sweep 359', None),
]
WORKSPACE_SHAPES = [
    (1, 64, 2176), (1, 1832, 128), (1, 3008, 2048), (1, 7976, 1152), (2, 6144, 256), (2, 6960, 384), (3, 4392, 640), (5, 7200, 4096),
    (5, 9016, 4224), (5, 10704, 128), (6, 10568, 2048), (6, 11160, 2176), (7, 5536, 128), (7, 9864, 5504), (8, 3904, 384), (10, 6384, 384),
    (10, 7488, 2176), (10, 10880, 4096), (12, 9584, 4096), (13, 9176, 4096), (14, 5552, 11008), (14, 11168, 640), (15, 2824, 128), (16, 1328, 4096),
    (16, 1744, 4096), (16, 3672, 4096), (16, 4096, 4096), (16, 4096, 11008), (16, 4944, 1024), (16, 5616, 384), (16, 5728, 1152), (16, 6048, 2048),
    (16, 6464, 4096), (16, 7720, 2176), (16, 8000, 11008), (16, 11008, 256), (16, 12288, 4096), (16, 22016, 4096), (16, 32064, 4096), (17, 2856, 640),
    (17, 3552, 2048), (17, 3736, 2048), (17, 6944, 1024), (17, 7192, 5504), (17, 9888, 256), (17, 11008, 11008), (19, 3872, 4224), (19, 4696, 11008),
    (22, 1024, 2176), (23, 8920, 4096), (23, 12288, 5504), (25, 4096, 4224), (25, 4304, 11008), (26, 1376, 4096), (26, 4576, 5504), (26, 7344, 1024),
    (26, 7384, 256), (27, 1024, 2176), (28, 3536, 256), (29, 4096, 4224), (30, 64, 4224), (30, 4256, 4096), (31, 1024, 1024), (32, 16, 2048),
    (32, 64, 1152), (32, 224, 640), (32, 3208, 256), (32, 3616, 256), (32, 4096, 4096), (32, 4096, 11008), (32, 4656, 2048), (32, 10624, 256),
    (32, 10720, 128), (32, 12288, 4096), (32, 22016, 4096), (32, 22016, 11008), (32, 32064, 4096), (33, 16, 256), (33, 32, 2048), (33, 64, 11008),
    (33, 952, 384), (33, 1024, 5504), (33, 4304, 2048), (33, 4696, 5504), (33, 8416, 4224), (33, 8560, 1024), (33, 9496, 2048), (33, 9584, 4096),
    (34, 4096, 2176), (34, 4896, 2048), (35, 1120, 1152), (35, 11008, 1024), (37, 12288, 128), (38, 16, 1024), (38, 2728, 128), (38, 7480, 640),
    (40, 12288, 384), (40, 12288, 2176), (40, 22016, 640), (41, 6048, 640), (44, 4096, 11008), (46, 1024, 5504), (46, 4304, 1152), (47, 4128, 1152),
    (47, 5360, 11008), (47, 5696, 2048), (48, 8472, 4096), (48, 10448, 5504), (49, 512, 1024), (49, 9600, 5504), (50, 8312, 384), (51, 1024, 2048),
    (53, 4768, 5504), (53, 4784, 4224), (53, 10672, 256), (54, 5800, 640), (54, 6080, 4096), (54, 9920, 1024), (54, 22016, 2048), (56, 1024, 1152),
    (56, 4304, 2048), (56, 7504, 1024), (57, 5888, 256), (57, 22016, 11008), (59, 64, 4224), (59, 4096, 1152), (59, 9632, 384), (60, 1504, 256),
    (60, 2640, 640), (60, 3824, 11008), (60, 8152, 256), (62, 11008, 1024), (64, 1648, 256), (64, 4096, 2048), (64, 4416, 2048), (64, 7576, 4096),
    (64, 8144, 5504), (64, 10056, 2048), (64, 10208, 11008), (64, 32064, 4096), (65, 1024, 5504), (65, 4992, 4096), (65, 7328, 2048), (65, 9976, 1152),
    (65, 10208, 4224), (65, 10288, 1152), (65, 10456, 640), (65, 12288, 128), (68, 7040, 5504), (71, 1024, 256), (73, 496, 640), (76, 8888, 4224),
    (80, 9416, 4224), (82, 8152, 4224), (83, 32, 4096), (84, 4808, 5504), (85, 8520, 4224), (90, 7168, 4224), (98, 9216, 256), (99, 32, 11008),
    (108, 64, 2176), (109, 8272, 11008), (119, 2112, 2048), (119, 6032, 5504), (119, 10328, 384), (127, 2240, 384), (127, 8496, 1024), (129, 2808, 4224),
    (129, 4096, 128), (132, 5296, 128), (143, 2304, 640), (144, 800, 256), (144, 2592, 384), (144, 11064, 1152), (146, 6872, 1152), (147, 7384, 1152),
    (153, 11008, 2176), (158, 192, 1152), (164, 64, 2048), (165, 6496, 1152), (171, 9680, 1024), (173, 5808, 4096), (175, 1024, 5504), (177, 3488, 1152),
    (182, 11008, 640), (183, 9792, 384), (184, 8904, 1152), (185, 2432, 11008), (186, 5008, 256), (200, 1024, 2048), (200, 1024, 4096), (200, 2560, 1024),
    (200, 4096, 4096), (200, 8192, 1024), (201, 2736, 4096), (204, 432, 384), (204, 1760, 1024), (204, 7584, 1024), (205, 22016, 256), (206, 4296, 4096),
    (212, 2536, 256), (214, 22016, 384), (215, 8376, 256), (223, 4304, 128), (224, 2120, 5504), (224, 2528, 128), (224, 3232, 1024), (224, 6432, 4224),
    (224, 9792, 2048), (224, 10368, 384), (225, 4304, 1152), (225, 5672, 1152), (225, 6800, 4096), (225, 12288, 4224), (228, 22016, 1024), (232, 22016, 128),
    (235, 4096, 384), (237, 4096, 5504), (237, 10128, 384), (237, 22016, 5504), (239, 3264, 2176), (239, 9360, 4224), (240, 6784, 1024), (242, 7264, 4224),
    (246, 224, 384), (247, 1024, 1152), (247, 3304, 256), (248, 9912, 4096), (251, 1216, 4224), (252, 4896, 2048), (253, 64, 640), (254, 7296, 1024),
    (256, 1152, 1536), (256, 1152, 4352), (256, 4352, 1152), (256, 4608, 1152), (257, 3776, 384), (261, 1024, 1024), (261, 1024, 4096), (261, 3072, 1024),
    (261, 4096, 1024), (262, 64, 128), (263, 5088, 1152), (263, 6048, 1152), (267, 3816, 128), (267, 8312, 5504), (271, 9216, 128), (275, 3568, 2176),
    (278, 4304, 5504), (278, 22016, 11008), (283, 264, 4224), (283, 1744, 4224), (285, 5296, 128), (286, 12288, 640), (294, 10384, 256), (300, 4160, 2304),
    (303, 12288, 4224), (307, 3232, 2048), (328, 6304, 384), (341, 288, 2176), (344, 1152, 1024), (355, 10392, 2176), (356, 5760, 128), (376, 4096, 128),
    (376, 7280, 384), (389, 9672, 384), (396, 168, 256), (413, 5376, 1152), (423, 6584, 4096), (426, 4736, 2048), (429, 9616, 640), (435, 5480, 1024),
    (440, 12272, 4160), (444, 2040, 4224), (448, 2048, 2048), (448, 2048, 4096), (448, 3072, 2048), (448, 3808, 4096), (448, 4096, 4096), (448, 4096, 11008),
    (448, 6088, 640), (448, 6144, 2048), (448, 8192, 2048), (448, 8312, 128), (448, 9728, 4096), (448, 10072, 256), (448, 12288, 4096), (448, 22016, 4096),
    (449, 16, 256), (449, 64, 5504), (449, 800, 4224), (449, 1024, 5504), (449, 3584, 11008), (449, 4096, 4096), (449, 4576, 256), (449, 5008, 1024),
    (449, 6736, 11008), (449, 8928, 384), (449, 9064, 4096), (449, 9856, 384), (450, 10336, 4096), (469, 1024, 256), (474, 5056, 2176), (479, 6016, 640),
    (493, 9536, 11008), (512, 64, 256), (512, 1024, 640), (512, 4096, 4096), (512, 4096, 5504), (512, 4096, 11008), (512, 4336, 640), (512, 9112, 256),
    (512, 10688, 640), (512, 12288, 4096), (512, 22016, 4096), (517, 64, 4096), (529, 4096, 384), (530, 1040, 2304), (552, 5976, 1152), (555, 8376, 2176),
    (558, 11008, 5504), (575, 9984, 640), (576, 1024, 1024), (576, 1024, 4096), (576, 3072, 1024), (576, 4096, 1024), (576, 10128, 640), (584, 4480, 384),
    (594, 8136, 384), (600, 9344, 11008), (610, 10392, 640), (617, 32, 2048), (623, 1592, 256), (633, 3480, 4224), (650, 6008, 11008), (652, 9856, 256),
    (672, 1536, 4096), (677, 10656, 4224), (704, 64, 384), (704, 64, 5504), (704, 2528, 11008), (704, 4096, 4096), (704, 4096, 11008), (704, 4416, 2176),
    (704, 5256, 384), (704, 10576, 256), (704, 12288, 4096), (704, 22016, 1024), (704, 22016, 4096), (707, 1024, 4224), (722, 10848, 384), (728, 3232, 1024),
    (730, 4304, 1024), (730, 12288, 640), (738, 22016, 4096), (761, 4592, 384), (802, 7168, 640), (803, 12288, 5504), (807, 9912, 4224), (813, 2448, 11008),
    (816, 64, 4224), (817, 264, 4224), (840, 4096, 4096), (861, 4288, 256), (877, 4584, 2048), (912, 4304, 256), (957, 1024, 2176), (974, 6112, 128),
    (985, 10304, 2048), (989, 10552, 640), (992, 10104, 5504), (1002, 4728, 1152), (1005, 7584, 4224), (1010, 22016, 11008), (1019, 4096, 5504), (1020, 8312, 4224),
    (1024, 8192, 2304), (1038, 1440, 1152), (1039, 4320, 2048), (1049, 4192, 256), (1065, 8360, 640), (1113, 32, 2176), (1127, 9872, 128), (1131, 9840, 256),
    (1132, 5560, 4096), (1143, 2400, 11008), (1161, 5296, 11008), (1163, 4304, 1024), (1167, 7584, 1024), (1169, 3888, 256), (1172, 640, 4096), (1183, 3608, 5504),
    (1183, 11008, 2176), (1185, 5952, 5504), (1190, 9120, 256), (1190, 12288, 4096), (1192, 6368, 2048), (2048, 1152, 1536), (2048, 1152, 4352), (2048, 4352, 1152),
    (2048, 4608, 1152), (2232, 2560, 2048), (2624, 32, 256), (2624, 64, 1024), (2624, 1024, 128), (2624, 1496, 4096), (2624, 2048, 2048), (2624, 2048, 16384),
    (2624, 2080, 1024), (2624, 2560, 2048), (2624, 2904, 1152), (2624, 3496, 128), (2624, 4096, 256), (2624, 4672, 2048), (2624, 8584, 4224), (2624, 10024, 1024),
    (2624, 11008, 1152), (2624, 11008, 5504), (2624, 32768, 2048),
]
WORKSPACE_BYTES = [
    4352, 7328, 192512, 287136, 98304, 167040, 263520, 1152000, 1262240, 214080,
    1521792, 1607040, 155008, 1933344, 374784, 766080, 2695680, 3046400, 3220224, 3817216,
    3420032, 3127040, 169440, 2719744, 3571712, 3760128, 4194304, 3932160, 2531328, 1078272,
    3299328, 3096576, 4550656, 4446720, 5632000, 1409024, 4718592, 8454144, 10260480, 971040,
    3864576, 4064768, 3777536, 4401504, 1344768, 8233984, 5002624, 4639648, 1531904, 6565120,
    6782976, 4505600, 6456000, 4579328, 7138560, 6110208, 1535872, 1880064, 792064, 5226496,
    253440, 8171520, 1015808, 32768, 73728, 143360, 821248, 925696, 8388608, 7864320,
    4767744, 2719744, 1372160, 9437184, 16908288, 30998528, 20520960, 4224, 67584, 726528,
    376992, 5812224, 9090048, 6818592, 9998208, 9039360, 7520832, 10120704, 5013504, 5326848,
    1411200, 6164480, 1818624, 19456, 414656, 5684800, 5898240, 11796480, 17612800, 4959360,
    15859712, 8101888, 7127424, 6984576, 22168960, 8566784, 13012992, 22066176, 802816, 20697600,
    4987200, 3342336, 11118976, 11156288, 4524928, 6264000, 14446080, 8570880, 28532736, 2064384,
    15425536, 13447168, 2684928, 110432256, 498432, 8699904, 6819456, 721920, 3168000, 20190720,
    3912960, 10919936, 843776, 16777216, 9043968, 15515648, 22933504, 15446016, 57491456, 65667072,
    2129920, 10383360, 15242240, 20750080, 21232640, 21399040, 21748480, 25559040, 15319040, 2326528,
    1158656, 21615616, 24104960, 21390848, 84992, 12923904, 23174400, 20643840, 28901376, 101376,
    221184, 28852736, 8042496, 22969856, 39329024, 9103360, 34527744, 11591424, 16908288, 22370304,
    10543104, 3686400, 11943936, 50982912, 32105984, 34734336, 53895168, 970752, 335872, 34298880,
    52968960, 32153088, 5734400, 19756032, 64110592, 57341952, 52426752, 14397440, 29807616, 6553600,
    6553600, 16384000, 26214400, 52428800, 17597952, 2820096, 11489280, 49508352, 144424960, 28319232,
    17204224, 150765568, 57626880, 30713344, 15196160, 18120704, 23166976, 46104576, 70189056, 74317824,
    30988800, 40838400, 48960000, 0, 0, 0, 30801920, 31064064, 76810752, 0,
    24963072, 71585280, 52101120, 56252416, 1763328, 8093696, 26114816, 78661632, 9766912, 39481344,
    518144, 59301888, 9437184, 9437184, 35651584, 37748736, 31053824, 8552448, 8552448, 25657344,
    34209792, 536576, 42820608, 50899968, 32603904, 71017728, 79921152, 31398400, 38288384, 0,
    2390784, 15793664, 48299520, 0, 97692672, 39936000, 0, 31751168, 66166784, 3142656,
    12681216, 118053120, 65617920, 49283072, 87592960, 120397056, 2128896, 71049216, 89121024, 64561152,
    132008448, 76281600, 0, 28984320, 29360128, 29360128, 44040192, 54591488, 58720256, 58720256,
    87277568, 88080384, 117440512, 119160832, 139460608, 144392192, 0, 0, 229888, 919552,
    11494400, 14712832, 51494912, 58851328, 65747968, 71954944, 96782848, 0, 0, 0,
    0, 15368192, 76689408, 92213248, 0, 1048576, 16777216, 67108864, 67108864, 67108864,
    71041024, 0, 0, 0, 0, 1058816, 69337088, 17638400, 105560064, 0,
    0, 0, 18874368, 18874368, 56623104, 75497472, 0, 83722240, 0, 0,
    0, 631808, 31738112, 70490880, 124966400, 0, 33030144, 0, 1441792, 1441792,
    56950784, 92274688, 92274688, 99483648, 118407168, 0, 0, 0, 0, 23166976,
    0, 75292672, 100541440, 0, 0, 111824384, 0, 0, 0, 63687168,
    1671168, 6902016, 110100480, 118142976, 128645376, 125607936, 31358976, 0, 0, 0,
    0, 151598592, 0, 0, 133562368, 0, 0, 47831040, 143631360, 140717056,
    0, 1139712, 0, 0, 0, 87782400, 0, 0, 0, 145442304,
    24002560, 136584448, 0, 0, 0, 0, 0, 75497472, 75497472, 0,
    0, 0, 2686976, 5373952, 85983232, 125616128, 0, 0, 0, 0,
    0, 0, 0, 0, 0, 0, 0, 0, 0,
]
