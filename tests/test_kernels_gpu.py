"""Kernel-level parity: every HIP kernel (through the C ABI, via cover_vla_amd.ops) against a plain fp32 PyTorch
restatement of the same op on the CPU. bf16 kernels: inputs are rounded to bf16 first, the reference computes in
fp32 and the comparison allows bf16 output rounding. fp32 kernels: atol/rtol 2e-5. Index outputs: exact."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from cover_vla_amd import ops  # noqa: E402


def bf(x):
    return x.to(torch.bfloat16)


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


ACT_REF = {
    "none": lambda x: x,
    "gelu_tanh": lambda x: torch.nn.functional.gelu(x, approximate="tanh"),
    "gelu_erf": lambda x: torch.nn.functional.gelu(x),
    "silu": torch.nn.functional.silu,
    "relu": torch.relu,
}


# ------------------------------------------------------------------------------------------------ bf16 GEMM
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("M,N,K", [(200, 256, 256), (333, 1152, 640), (128, 384, 1024), (1, 128, 128), (257, 136, 384)])
def test_gemm_tiled(dev, variant, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.05)
    bias = torch.randn(N, generator=g)
    lin = ops.pack_linear(w.to(dev), bias.to(dev))
    out = ops.gemm(a.to(dev), lin, variant=variant)
    ref = a.float() @ w.float().T + bias
    assert rel_l2(out, ref) < 6e-3
    assert torch.allclose(out.float().cpu(), ref, atol=0.05, rtol=2e-2)


@pytest.mark.parametrize("M,N,K,glu", [(1100, 6144, 2048, False), (1037, 16384, 2048, True), (2304, 4096, 8192, False), (1025, 4352, 2176, False),
                                       (512, 12288, 4096, False), (512, 22016, 4096, True), (512, 4096, 11008, False), (704, 12288, 4096, False),
                                       (530, 6144, 2048, False)])
def test_gemm_long_panel_tiles(dev, M, N, K, glu):
    # M >= 512 (config-5 decode rows, two-camera prefill) and M >= 1024: the 12-wave kernels (8 MFMA waves on 128x256 / 256x128 tiles + 4 loader waves), ragged M and N tiles,
    # bias / activation / GLU / residual epilogues -- against fp32 matmul of the same bf16 operands (computed on the device)
    g = torch.Generator(device=dev).manual_seed(M + N)
    a = (torch.randn(M, K, device=dev, generator=g)).bfloat16()
    w = (torch.randn(N, K, device=dev, generator=g) * 0.03).bfloat16()
    y = a.float() @ w.float().T
    if glu:
        lin = ops.pack_linear(w, glu=True)
        out = ops.gemm(a, lin, act="silu")
        ref = torch.nn.functional.silu(y[:, : N // 2]) * y[:, N // 2:]
    else:
        bias = torch.randn(N, device=dev, generator=g) * 0.3
        res = torch.randn(M, N, device=dev, generator=g).bfloat16()
        lin = ops.pack_linear(w, bias)
        out = ops.gemm(a, lin, residual=res)
        ref = res.float() + y + bias
    assert rel_l2(out, ref) < 6e-3
    d = (out.float() - ref).abs()
    assert (d <= 0.06 + 2e-2 * ref.abs()).all()


@pytest.mark.parametrize("M,N,K,kind", [(448, 12288, 4096, "bias_residual"), (448, 12288, 4096, "f32"), (440, 12288 - 16, 4096 + 64, "bias_residual"),
                                        (448, 3072, 2048, "plain"), (2232, 2560, 2048, "plain"), (672, 1536, 4096, "norm")])
def test_gemm_k_split_wave_pairs(dev, M, N, K, kind):
    """gemm_tiled_v3k (round 6): the 224 x 96 tile on four wave PAIRS -- the two waves of a SIMD own one 112 x 48 wave tile and split every
    64-deep k-tile -- with the pair's sums handed through the LDS before the epilogue. The planner's choice for the qkv-like shapes (plan
    counter 30 asserted); ragged M / N / K (an odd number of k-tiles), every epilogue kind incl. split-K + fused RMSNorm, vs fp32 matmul."""
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.03).bfloat16()
    a = torch.zeros(M, (K + 127) // 128 * 128, dtype=torch.bfloat16, device=dev)      # row pitch = padded K, zero padded
    a[:, :K] = torch.randn(M, K, device=dev, generator=g).bfloat16()
    y = a[:, :K].float() @ w.float().T
    ops.gemm_plan_counts(reset=True)
    if kind == "bias_residual":
        bias = torch.randn(N, device=dev, generator=g) * 0.3
        res = torch.randn(M, N, device=dev, generator=g).bfloat16()
        out = ops.gemm(a, ops.pack_linear(w, bias), residual=res)
        ref = res.float() + y + bias
    elif kind == "f32":
        out = ops.gemm(a, ops.pack_linear(w), out_f32=True)
        ref = y
    elif kind == "norm":
        res = torch.randn(M, N, device=dev, generator=g).bfloat16()
        nw = torch.randn(N, device=dev, generator=g) * 0.2 + 1.0
        out = res.clone()
        h = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm(a, ops.pack_linear(w), residual=out, out=out, norm_w=nw, norm_out=h, norm_style=1, norm_w_offset=0.0, norm_eps=1e-5)
        ref = res.float() + y
    else:
        out = ops.gemm(a, ops.pack_linear(w))
        ref = y
    counts = ops.gemm_plan_counts()
    assert sum(counts) == 1 and (counts[30] == 1 or N < 12000), counts      # the qkv-like shapes must run on the pair kernel
    print("plan", [i for i, v in enumerate(counts) if v])
    assert rel_l2(out, ref) < 6e-3
    d = (out.float() - ref).abs()
    assert (d <= 0.06 + 2e-2 * ref.abs()).all()
    if kind == "norm":
        xf = out.float()
        ref_h = (nw * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).bfloat16().float()).bfloat16()
        assert torch.allclose(h.float(), ref_h.float(), atol=2e-2, rtol=1e-2)


@pytest.mark.parametrize("act", ["silu", "gelu_tanh"])
@pytest.mark.parametrize("glu", [False, True])
def test_gemm_epilogue_fast_activation_on_every_bf16_input(dev, act, glu):
    """The store loops of the staged epilogue evaluate SiLU / tanh-GELU with v_exp_f32 + v_rcp_f32 (common.h act_apply_bf16) on values that are
    rounded to bf16 right after. Every finite bf16 bit pattern goes through an identity GEMM (x * 1 + zeros: exact) into the epilogue; the
    result must sit within one bf16 ulp of torch's fp32 activation rounded to bf16 (2e-6 absolute in tanh-GELU's cancelling tail, where
    0.5 x (1 + tanh u) is quantised to 2^-24 x in the fp32 reference as well)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16)
    x = x[torch.isfinite(x.float())]
    x = torch.cat([x, torch.zeros((-len(x)) % 128, dtype=torch.bfloat16)]).reshape(-1, 128)          # [M, 128], one value per GEMM output
    M = x.shape[0]
    eye = torch.eye(128, dtype=torch.bfloat16)
    if glu:   # gate = x through the identity, up = 1: out = act(x) * 1 (pack_linear(glu=True): rows [gate; up])
        a = torch.cat([x, torch.ones(M, 128, dtype=torch.bfloat16)], 1)
        w = torch.zeros(256, 256, dtype=torch.bfloat16)
        w[:128, :128] = eye
        w[128:, 128] = 1.0
        out = ops.gemm(a.to(dev), ops.pack_linear(w.to(dev), glu=True), act=act)
    else:
        out = ops.gemm(x.to(dev), ops.pack_linear(eye.to(dev)), act=act)
    ref = ACT_REF[act](x.float()).bfloat16().float()
    got = out.float().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    assert bool((err <= ref.abs() * 2.0 ** -7 + 2e-6).all()), (err - ref.abs() * 2.0 ** -7).max()
    assert (got != ref).float().mean().item() < 0.02            # and all but a few rounding-boundary cases are bit-identical


def test_gemm_fp8_loader_wave_and_self_loading_forms_agree(dev, tmp_path):
    """The loader-wave fp8 kernel (gemm_tiled_pc_f8) stays in the library behind COVER_V3_F8=0 (it is the default for the 64 x 128 tile; the
    knob keeps it for the others: A/B runs). The knob is read once per process, so each form runs in a child; the parent compares: same tile,
    same K slices, same k order per accumulator -- BIT-IDENTICAL. (The bf16 loader-wave forms of the long-panel tiles were removed in
    round 6: docs/experiments/r06_pruned_variants.patch.)"""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for tag, env in (("self", {}), ("loader", {"COVER_V3_F8": "0"})):
        path = str(tmp_path / f"{tag}.pt")
        e = dict(os.environ, **env)
        e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "_gemm_forms_child.py"), path], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = torch.load(path)
    ps, pl = res["self"]["plans"], res["loader"]["plans"]
    assert ps[21] == 4 and pl[21] == 4, (ps, pl)                                            # fp8: the same four launches in both
    from tests._gemm_forms_child import CASES
    for i, (M, N, K, glu, f8) in enumerate(CASES):
        a, b = res["self"][i], res["loader"][i]
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (i, M, N, K)


@pytest.mark.parametrize("N,K,kind", [(12288, 4096, "bias_residual"), (22016, 4096, "glu"), (4096, 4096, "norm"), (4096, 11008, "norm")])
def test_gemm_headline_prefill_tiles_m448_bf16(dev, N, K, kind):
    """The headline decision's prefill pass is M = 448 rows (256 patch rows + 8 prompts x 24 text rows) on the Llama-2-7B shapes:
    qkv (448, 12288, 4096), gate_up (448, 22016 GLU + SiLU, 4096), o_proj (448, 4096, 4096) and down (448, 4096, 11008) with the
    residual + fused RMSNorm epilogue through split-K -- in bf16, against an fp32 matmul of the same bf16 operands, with the
    library's plan counters asserting that a 224-row tile (self-loading picks 23..29) is what ran."""
    M = 448
    g = torch.Generator(device=dev).manual_seed(N + K)
    a = torch.randn(M, K, device=dev, generator=g).bfloat16()
    w = (torch.randn(N, K, device=dev, generator=g) * 0.03).bfloat16()
    y = a.float() @ w.float().T
    ops.gemm_plan_counts(reset=True)
    if kind == "glu":
        out = ops.gemm(a, ops.pack_linear(w, glu=True), act="silu")
        ref = torch.nn.functional.silu(y[:, : N // 2]) * y[:, N // 2:]
    elif kind == "bias_residual":
        bias = torch.randn(N, device=dev, generator=g) * 0.3
        res = torch.randn(M, N, device=dev, generator=g).bfloat16()
        out = ops.gemm(a, ops.pack_linear(w, bias), residual=res)
        ref = res.float() + y + bias
    else:   # decoder o_proj / down: x = residual + A W^T in place, h = llama-RMSNorm(x) from the split-K reduction
        res = torch.randn(M, N, device=dev, generator=g).bfloat16()
        nw = torch.randn(N, device=dev, generator=g) * 0.2 + 1.0
        out = res.clone()
        h = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
        ops.gemm(a, ops.pack_linear(w), residual=out, out=out, norm_w=nw, norm_out=h, norm_style=1, norm_w_offset=0.0, norm_eps=1e-5)
        ref = res.float() + y
    counts = ops.gemm_plan_counts()
    assert sum(counts[23:32]) == 1 and sum(counts) == 1, counts   # a 224-row self-loading tile
    assert rel_l2(out, ref) < 6e-3
    d = (out.float() - ref).abs()
    assert (d <= 0.06 + 2e-2 * ref.abs()).all()
    if kind == "norm":
        xf = out.float()   # the norm of what was actually stored
        ref_h = (nw * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).bfloat16().float()).bfloat16()
        assert torch.allclose(h.float(), ref_h.float(), atol=2e-2, rtol=1e-2)


def test_gemm_transpose_detecting(dev):
    # A = I with an asymmetric W: out must equal W^T exactly (bf16 values are exact here)
    K = N = 256
    a = bf(torch.eye(K))
    w = bf(torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 251 - 125)
    lin = ops.pack_linear(w.to(dev))
    for variant in (1, 2):
        out = ops.gemm(a.to(dev), lin, variant=variant)
        assert torch.equal(out.float().cpu(), w.float().T)


@pytest.mark.parametrize("variant", [3, 5])
@pytest.mark.parametrize("M", [1, 5, 16, 32, 40, 64])
@pytest.mark.parametrize("N,K", [(512, 1024), (4096, 512), (264, 128), (1376, 2176), (1024, 4096)])
def test_gemm_skinny(dev, variant, M, N, K):
    g = torch.Generator().manual_seed(M * 131 + N + K)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.05)
    bias = torch.randn(N, generator=g)
    lin = ops.pack_linear(w.to(dev), bias.to(dev))
    out = ops.gemm(a.to(dev), lin, variant=variant)
    ref = a.float() @ w.float().T + bias
    assert rel_l2(out, ref) < 6e-3
    out32 = ops.gemm(a.to(dev), lin, variant=variant, out_f32=True)
    assert torch.allclose(out32.cpu(), bf(ref).float(), atol=0.05, rtol=2e-2)


@pytest.mark.parametrize("M", [1, 16, 27, 32])
@pytest.mark.parametrize("N,K,glu", [(768, 2048, False), (1536, 4096, True), (416, 2176, True), (22016, 4096, True)])
def test_gemm_skinny_full_k_fused_epilogue(dev, M, N, K, glu):
    # third-generation weight streaming (variant 6): no split-K slabs, bias / activation / GLU / residual in the kernel
    g = torch.Generator().manual_seed(M * 13 + N + K)
    w = bf(torch.randn(N, K, generator=g) * 0.05)
    a = bf(torch.randn(M, K, generator=g))
    n_out = N // 2 if glu else N
    bias = torch.randn(N, generator=g) * 0.1
    res = bf(torch.randn(M, n_out, generator=g))
    if glu:
        bias = torch.zeros(N)   # the GLU epilogue has no bias term (Llama / Gemma MLPs)
    lin = ops.pack_linear(w.to(dev), None if glu else bias.to(dev), glu=glu)
    kw = dict(act="silu") if glu else dict(act="gelu_tanh", residual=res.to(dev))
    out = ops.gemm(a.to(dev), lin, variant=6, **kw)
    y = a.float() @ w.float().T + bias
    ref = torch.nn.functional.silu(y[:, :n_out]) * y[:, n_out:] if glu else torch.nn.functional.gelu(y, approximate="tanh") + res.float()
    assert out.shape == (M, n_out)
    assert rel_l2(out, ref) < 6e-3
    # and it agrees with the split-K generation up to the bf16 rounding of differently ordered fp32 sums
    out3 = ops.gemm(a.to(dev), lin, variant=3, **kw)
    assert rel_l2(out, out3.float().cpu()) < 4e-3


@pytest.mark.parametrize("variant,M", [(1, 150), (2, 150), (3, 32)])
@pytest.mark.parametrize("act", ["gelu_tanh", "gelu_erf", "silu", "relu"])
def test_gemm_epilogues(dev, variant, M, act):
    N, K = 384, 256
    g = torch.Generator().manual_seed(11)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.08)
    bias = torch.randn(N, generator=g) * 0.5
    res = bf(torch.randn(M, N, generator=g))
    ls = torch.rand(N, generator=g)
    lin = ops.pack_linear(w.to(dev), bias.to(dev))
    lin0 = ops.pack_linear(w.to(dev))
    y = a.float() @ w.float().T
    # activation
    out = ops.gemm(a.to(dev), lin, act=act, variant=variant)
    assert rel_l2(out, ACT_REF[act](y + bias)) < 8e-3
    # residual + layer scale
    out = ops.gemm(a.to(dev), lin, residual=res.to(dev), layer_scale=ls.to(dev), variant=variant)
    assert rel_l2(out, res.float() + ls * (y + bias)) < 8e-3
    # fp32 residual, fp32 output
    res32 = torch.randn(M, N, generator=g)
    out = ops.gemm(a.to(dev), lin0, residual=res32.to(dev), out_f32=True, variant=variant)
    assert rel_l2(out, res32 + y) < 8e-3
    # in-place residual (out aliases residual), as the decoder uses it
    x = res.clone().to(dev)
    ops.gemm(a.to(dev), lin0, residual=x, out=x, variant=variant)
    assert rel_l2(x, res.float() + y) < 8e-3
    # GLU: W = [gate; up]
    wg = bf(torch.randn(2 * N, K, generator=g) * 0.08)
    ling = ops.pack_linear(wg.to(dev), glu=True)
    out = ops.gemm(a.to(dev), ling, act=act, variant=variant)
    yy = a.float() @ wg.float().T
    assert out.shape == (M, N)
    assert rel_l2(out, ACT_REF[act](yy[:, :N]) * yy[:, N:]) < 1e-2


def test_gemm_random_sweep(dev):
    """300 random problems through cover_gemm_bf16's automatic plan selection (ragged M / N, K up to 11 008, weight streaming / 64..224-row
    tiles / split-K; plain, bias + activation, in-place residual, GLU, residual + fused RMSNorm) against fp32 matmuls of the same bf16
    operands (tools/dbg/fuzz_gemm.py: 6 400 cases over four seeds ran clean when this was added)."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("fuzz_gemm", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dbg", "fuzz_gemm.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    fails, plans = fz.run(300, 7, dev, verbose=False)
    assert not fails, fails[:5]
    assert len(plans) >= 6, plans          # the sweep reached the streaming kernels and several tile families


# ------------------------------------------------------------------------------------------------ attention
def attn_ref(q, segs, scale):
    """q [B,Tq,Hq,D]; segs: list of (k [B,Tk,Hkv,D], v [B,Tk,Hkv,D], vis bool [B,Tq,Tk])."""
    B, Tq, Hq, D = q.shape
    k = torch.cat([s[0] for s in segs], 1).float()
    v = torch.cat([s[1] for s in segs], 1).float()
    vis = torch.cat([s[2] for s in segs], 2)
    G = Hq // k.shape[2]
    k = k.repeat_interleave(G, 2)
    v = v.repeat_interleave(G, 2)
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k) * scale
    s = s.masked_fill(~vis[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.nan_to_num(p, nan=0.0)
    return torch.einsum("bhqk,bkhd->bqhd", p, v)


def make_cache(k, v, dev, tcap=None):
    """k, v [S, T, Hkv, D] -> device K cache [S][T][Hkv][D] and V^T cache [S][Hkv][D][tcap] + strides."""
    S, T, Hkv, D = k.shape
    tcap = tcap or (T + 31) // 32 * 32
    kc = k.contiguous().to(dev)
    vt = torch.zeros(S, Hkv, D, tcap, dtype=torch.bfloat16)
    vt[..., :T] = v.permute(0, 2, 3, 1)
    return kc, vt.to(dev), (T * Hkv * D, Hkv * D, D), (Hkv * D * tcap, D * tcap, tcap)


@pytest.mark.parametrize("D", [64, 96, 128, 256])
@pytest.mark.parametrize("Tq,Tk,Hq,Hkv", [(50, 77, 4, 4), (1, 300, 8, 8), (5, 40, 8, 1), (130, 130, 2, 1)])
def test_attention_len_mask(dev, D, Tq, Tk, Hq, Hkv):
    B = 3
    g = torch.Generator().manual_seed(D + Tq)
    q = bf(torch.randn(B, Tq, Hq, D, generator=g))
    k = bf(torch.randn(B, Tk, Hkv, D, generator=g))
    v = bf(torch.randn(B, Tk, Hkv, D, generator=g))
    lens = torch.tensor([Tk, max(1, Tk // 2), max(1, Tk - 3)], dtype=torch.int32)
    vis = (torch.arange(Tk)[None, None, :] < lens[:, None, None]).expand(B, Tq, Tk)
    ref = attn_ref(q, [(k, v, vis)], D ** -0.5)
    kc, vt, ks, vs = make_cache(k, v, dev)
    out = torch.empty(B, Tq, Hq, D, dtype=torch.bfloat16, device=dev)
    seg = ops.Segment(kc, vt, ks, vs, length=Tk, len_of_batch=lens.to(dev))
    ops.attention(q.to(dev), (Tq * Hq * D, Hq * D, D), out, (Tq * Hq * D, Hq * D, D), B, Tq, Hq, Hkv, D, D ** -0.5, [seg])
    assert rel_l2(out, ref) < 1.2e-2
    assert torch.allclose(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("Tq", [1, 4, 37])
def test_attention_three_segments(dev, Tq):
    # shared prefix (one slot for every batch row) + per-prompt segment via slot map + own causal segment
    B, Hq, Hkv, D = 6, 4, 2, 128
    T0, T1, T2 = 70, 45, Tq + 3
    g = torch.Generator().manual_seed(5 + Tq)
    q = bf(torch.randn(B, Tq, Hq, D, generator=g))
    k0, v0 = bf(torch.randn(1, T0, Hkv, D, generator=g)), bf(torch.randn(1, T0, Hkv, D, generator=g))
    k1, v1 = bf(torch.randn(2, T1, Hkv, D, generator=g)), bf(torch.randn(2, T1, Hkv, D, generator=g))
    k2, v2 = bf(torch.randn(B, T2, Hkv, D, generator=g)), bf(torch.randn(B, T2, Hkv, D, generator=g))
    slot1 = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32)
    len1 = torch.tensor([45, 45, 45, 30, 30, 30], dtype=torch.int32)
    zero = torch.zeros(B, dtype=torch.int32)
    vis0 = torch.ones(B, Tq, T0, dtype=torch.bool)
    vis1 = (torch.arange(T1)[None, None, :] < len1[:, None, None]).expand(B, Tq, T1)
    vis2 = (torch.arange(T2)[None, None, :] <= (torch.arange(Tq)[None, :, None] + 3)).expand(B, Tq, T2)
    ref = attn_ref(q, [(k0.expand(B, -1, -1, -1), v0.expand(B, -1, -1, -1), vis0), (k1[slot1.long()], v1[slot1.long()], vis1),
                       (k2, v2, vis2)], 0.11)
    c0 = make_cache(k0, v0, dev)
    c1 = make_cache(k1, v1, dev)
    c2 = make_cache(k2, v2, dev)
    segs = [ops.Segment(c0[0], c0[1], c0[2], c0[3], length=T0, slot_of_batch=zero.to(dev)),
            ops.Segment(c1[0], c1[1], c1[2], c1[3], length=T1, slot_of_batch=slot1.to(dev), len_of_batch=len1.to(dev)),
            ops.Segment(c2[0], c2[1], c2[2], c2[3], length=T2, mask=ops.MASK_CAUSAL, causal_offset=3)]
    out = torch.empty(B, Tq, Hq, D, dtype=torch.bfloat16, device=dev)
    ops.attention(q.to(dev), (Tq * Hq * D, Hq * D, D), out, (Tq * Hq * D, Hq * D, D), B, Tq, Hq, Hkv, D, 0.11, segs)
    assert rel_l2(out, ref) < 1.2e-2


def test_attention_vislen_pi0_suffix(dev):
    # pi0 denoise step: 5 suffix tokens x 8 q heads over 1 kv head; prefix by length + suffix block mask [1,5,5,5,5]
    B, Tq, Hq, Hkv, D, Tp = 4, 5, 8, 1, 256, 90
    g = torch.Generator().manual_seed(9)
    q = bf(torch.randn(B, Tq, Hq, D, generator=g))
    kp, vp = bf(torch.randn(2, Tp, Hkv, D, generator=g)), bf(torch.randn(2, Tp, Hkv, D, generator=g))
    ks_, vs_ = bf(torch.randn(B, Tq, Hkv, D, generator=g)), bf(torch.randn(B, Tq, Hkv, D, generator=g))
    slot = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    plen = torch.tensor([80, 80, 61, 61], dtype=torch.int32)
    vl = torch.tensor([1, 5, 5, 5, 5], dtype=torch.int32)
    visp = (torch.arange(Tp)[None, None, :] < plen[:, None, None]).expand(B, Tq, Tp)
    viss = (torch.arange(Tq)[None, None, :] < vl[None, :, None]).expand(B, Tq, Tq)
    ref = attn_ref(q, [(kp[slot.long()], vp[slot.long()], visp), (ks_, vs_, viss)], D ** -0.5)
    cp = make_cache(kp, vp, dev)
    cs = make_cache(ks_, vs_, dev)
    segs = [ops.Segment(cp[0], cp[1], cp[2], cp[3], length=Tp, slot_of_batch=slot.to(dev), len_of_batch=plen.to(dev)),
            ops.Segment(cs[0], cs[1], cs[2], cs[3], length=Tq, mask=ops.MASK_VISLEN, vis_len=vl.to(dev))]
    out = torch.empty(B, Tq, Hq, D, dtype=torch.bfloat16, device=dev)
    ops.attention(q.to(dev), (Tq * Hq * D, Hq * D, D), out, (Tq * Hq * D, Hq * D, D), B, Tq, Hq, Hkv, D, D ** -0.5, segs)
    assert rel_l2(out, ref) < 1.2e-2


def test_attention_spike_forces_rescale(dev):
    # one key far above the rest late in the sequence: exercises the online-softmax rescale branch
    B, Tq, H, D, Tk = 1, 16, 1, 64, 200
    g = torch.Generator().manual_seed(3)
    q = bf(torch.randn(B, Tq, H, D, generator=g))
    k = bf(torch.randn(B, Tk, H, D, generator=g) * 0.1)
    v = bf(torch.randn(B, Tk, H, D, generator=g))
    k[0, 170, 0] = q[0, 3, 0] * 4
    vis = torch.ones(B, Tq, Tk, dtype=torch.bool)
    ref = attn_ref(q, [(k, v, vis)], 1.0)
    kc, vt, ks, vs = make_cache(k, v, dev)
    out = torch.empty(B, Tq, H, D, dtype=torch.bfloat16, device=dev)
    ops.attention(q.to(dev), (Tq * H * D, H * D, D), out, (Tq * H * D, H * D, D), B, Tq, H, H, D, 1.0,
                  [ops.Segment(kc, vt, ks, vs, length=Tk)])
    assert torch.allclose(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


def test_attention_random_sweep(dev):
    """300 random problems through cover_attention_bf16 (head dims 64 / 96 / 128 / 256, GQA ratios 1-8, 1-3 key segments with shared slots,
    slot maps, per-row lengths and causal offsets, Tq 1..300, keys 1..900) against an fp32 restatement (tools/dbg/fuzz_attn.py: 1 800 cases
    over three seeds ran clean when this was added)."""
    import importlib.util, os
    spec = importlib.util.spec_from_file_location("fuzz_attn", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dbg", "fuzz_attn.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    fails = fz.run(300, 11, dev, verbose=False)
    assert not fails, fails[:5]


# ------------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("dim", [1024, 1152, 4096])
def test_norms(dev, dim):
    g = torch.Generator().manual_seed(dim)
    x = bf(torch.randn(37, dim, generator=g) * 3 + 0.5)
    w, b = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    ref = torch.nn.functional.layer_norm(x.float(), (dim,), w, b, 1e-6)
    out = ops.layernorm(x.to(dev), w.to(dev), b.to(dev), 1e-6)
    assert torch.allclose(out.float().cpu(), ref, atol=2e-2, rtol=1e-2)
    xf = x.float()
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
    out = ops.rmsnorm(x.to(dev), w.to(dev), 1e-6, w_offset=1.0, style=0)  # Gemma
    assert torch.allclose(out.float().cpu(), bf(xf * rstd * (1 + w)).float(), atol=2e-2, rtol=1e-2)
    out = ops.rmsnorm(x.to(dev), w.to(dev), 1e-6, w_offset=0.0, style=1)  # Llama
    assert torch.allclose(out.float().cpu(), bf(w * bf(xf * rstd).float()).float(), atol=2e-2, rtol=1e-2)
    x32 = torch.randn(5, dim, generator=g)
    rstd = torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + 1e-6)
    out = ops.rmsnorm(x32.to(dev), w.to(dev), 1e-6, w_offset=1.0, style=0)
    assert torch.allclose(out.float().cpu(), bf(x32 * rstd * (1 + w)).float(), atol=2e-2, rtol=1e-2)


@pytest.mark.parametrize("T,D", [(7, 128), (24, 128), (70, 64), (19, 256)])   # T >= 16: vectorised q / k rotation + token-group V placement
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_rope_kv_write(dev, mode, T, D):
    B, Hq, Hkv, tcap, npos = 2, 4, 2, 128, 64
    g = torch.Generator().manual_seed(mode)
    qkv = bf(torch.randn(B * T, (Hq + 2 * Hkv) * D, generator=g))
    pos = torch.randint(0, npos, (B * T,), generator=g, dtype=torch.int32)
    half = D // 2
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(npos).float()[:, None] * inv[None]
    cos, sin = ang.cos(), ang.sin()
    kc = torch.zeros(3, tcap, Hkv, D, dtype=torch.bfloat16, device=dev)
    vt = torch.zeros(3, Hkv, D, tcap, dtype=torch.bfloat16, device=dev)
    slot = torch.tensor([2, 0], dtype=torch.int32)
    toff = torch.tensor([1, 4], dtype=torch.int32)
    d_qkv = qkv.clone().to(dev)
    ops.rope_kv_write(d_qkv, B, T, Hq, Hkv, D, positions=pos.to(dev), cos=cos.to(dev), sin=sin.to(dev), rope_mode=mode,
                      k_cache=kc, k_strides=(tcap * Hkv * D, Hkv * D, D), vt_cache=vt, vt_strides=(Hkv * D * tcap, D * tcap, tcap),
                      slot_of_batch=slot.to(dev), t_offset_of_batch=toff.to(dev), t_offset=2)
    x = qkv.float().reshape(B, T, Hq + 2 * Hkv, D)
    c = cos[pos.long()].reshape(B, T, 1, half)
    s = sin[pos.long()].reshape(B, T, 1, half)

    def rot(x):
        x1, x2 = x[..., :half], x[..., half:]
        if mode == 0:
            return x
        if mode == 1:
            return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
        cb, sb = bf(c).float(), bf(s).float()
        return torch.cat([bf(bf(x1 * cb).float() + bf(-x2 * sb).float()).float(), bf(bf(x2 * cb).float() + bf(x1 * sb).float()).float()], -1)

    got = d_qkv.float().cpu().reshape(B, T, Hq + 2 * Hkv, D)
    assert torch.equal(got[:, :, :Hq], bf(rot(x[:, :, :Hq])).float())
    kref = bf(rot(x[:, :, Hq:Hq + Hkv])).float()
    for b in range(B):
        t0 = 2 + toff[b].item()
        assert torch.equal(kc[slot[b].item(), t0:t0 + T].float().cpu(), kref[b])
        assert torch.equal(vt[slot[b].item(), :, :, t0:t0 + T].float().cpu(), x[b, :, Hq + Hkv:].permute(1, 2, 0))


def test_small_row_kernels(dev):
    g = torch.Generator().manual_seed(0)
    table = bf(torch.randn(100, 256, generator=g))
    ids = torch.randint(0, 100, (17,), generator=g)
    sc = math.sqrt(256)
    out = ops.embed_gather(table.to(dev), ids.to(dev), sc)
    assert torch.equal(out.float().cpu(), bf(table[ids].float() * torch.tensor(sc, dtype=torch.float32)).float())
    # patchify: uint8 HWC and fp32 CHW agree with unfold
    img = torch.randint(0, 256, (2, 28, 42, 3), generator=g, dtype=torch.uint8)
    mul, add = [1 / 255 / 0.5] * 3, [-1.0] * 3
    p = ops.patchify(img.to(dev), 14, mul, add, 640)
    x = img.float().permute(0, 3, 1, 2) * (1 / 255 / 0.5) - 1.0
    ref = torch.nn.functional.unfold(x, 14, stride=14).transpose(1, 2).reshape(-1, 588)
    assert torch.allclose(p[:, :588].float().cpu(), bf(ref).float(), atol=1e-2)
    assert p[:, 588:].abs().max().item() == 0
    p2 = ops.patchify(x.contiguous().to(dev), 14, [1.0] * 3, [0.0] * 3, 640)
    assert torch.equal(p2[:, :588].float().cpu(), bf(ref).float())
    # add_rows / scale / casts / copy_rows
    xx = bf(torch.randn(12, 64, generator=g))
    pe = bf(torch.randn(4, 64, generator=g))
    o = ops.add_rows(xx.clone().to(dev), pe.to(dev))
    assert torch.equal(o.float().cpu(), bf(xx.float() + pe.float().repeat(3, 1)).float())
    o = ops.scale_bf16(xx.clone().to(dev), float(bf(torch.tensor(8.0))), float(bf(torch.tensor(8.0))))
    assert torch.equal(o.float().cpu(), bf(bf(xx.float() / 8).float() * 8).float())
    f = torch.randn(5, 40, generator=g)
    assert torch.equal(ops.cast_f32_to_bf16(f.to(dev)).float().cpu(), bf(f).float())
    assert torch.equal(ops.cast_bf16_to_f32(xx.to(dev)).cpu(), xx.float())
    dst = torch.zeros(12, 64, dtype=torch.bfloat16, device=dev)
    si = torch.tensor([3, 1, 7], dtype=torch.int32)
    di = torch.tensor([0, 5, 11], dtype=torch.int32)
    ops.copy_rows(xx.to(dev), dst, 3, 64, si.to(dev), di.to(dev))
    assert torch.equal(dst[di.long()].float().cpu(), xx[si.long()].float())


# ------------------------------------------------------------------------------------------------ fp32 kernels
@pytest.mark.parametrize("M,N,K", [(64, 576, 1024), (1, 512, 512), (320, 512, 7), (70, 1024, 576), (33, 32, 1024)])
def test_gemm_f32(dev, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    a, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    out = ops.gemm_f32(a.to(dev), w.to(dev), bias=bias.to(dev), act="gelu_erf", alpha=-0.1, residual=res.to(dev))
    ref = res + -0.1 * torch.nn.functional.gelu((a.double() @ w.double().T).float() + bias)
    assert torch.allclose(out.cpu(), ref, atol=2e-5, rtol=2e-5)
    # k-major B operand ("NN"): C = A @ Bkn
    bkn = torch.randn(K, N, generator=g)
    out = ops.gemm_f32(a.to(dev), bkn.to(dev), b_is_kn=True)
    assert torch.allclose(out.cpu(), (a.double() @ bkn.double()).float(), atol=1e-4, rtol=2e-5)


def test_mha_f32_and_rows(dev):
    g = torch.Generator().manual_seed(1)
    B, Tq, Tk, H, Dh = 5, 10, 10, 8, 64
    q, k, v = (torch.randn(B, t, H * Dh, generator=g) for t in (Tq, Tk, Tk))
    pad = torch.zeros(B, Tk, dtype=torch.bool)
    pad[0, :6] = True
    pad[3, :2] = True
    out = ops.mha_f32(q.to(dev), k.to(dev), v.to(dev), B, Tq, Tk, H, Dh, (Tq * H * Dh, H * Dh), (Tk * H * Dh, H * Dh),
                      (Tk * H * Dh, H * Dh), key_pad=pad.to(torch.uint8).to(dev))
    qh, kh, vh = (t.reshape(B, -1, H, Dh).transpose(1, 2) for t in (q, k, v))
    s = (qh * Dh ** -0.5) @ kh.transpose(-1, -2)
    s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    ref = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Tq, H * Dh)
    assert torch.allclose(out.cpu(), ref, atol=2e-5, rtol=2e-5)
    x = torch.randn(9, 576, generator=g)
    assert torch.allclose(ops.softmax_rows_f32(x.clone().to(dev), 1 / 0.07).cpu(), torch.softmax(x / 0.07, -1), atol=1e-6, rtol=1e-4)
    assert torch.allclose(ops.l2norm_rows_f32(x.to(dev)).cpu(), x / x.norm(dim=-1, keepdim=True), atol=1e-6, rtol=1e-5)
    w, b = torch.randn(576, generator=g), torch.randn(576, generator=g)
    assert torch.allclose(ops.layernorm_f32(x.to(dev), w.to(dev), b.to(dev)).cpu(),
                          torch.nn.functional.layer_norm(x, (576,), w, b), atol=1e-5, rtol=1e-5)
    assert torch.allclose(ops.add_f32(x.to(dev), x[:3].contiguous().to(dev)).cpu(), x + x[:3].repeat(3, 1))
    xm = torch.randn(B, Tk, 512, generator=g)
    mm = ops.masked_mean_f32(xm.to(dev), pad.to(torch.uint8).to(dev), B, Tk, 512)
    keep = (~pad).float()[..., None]
    assert torch.allclose(mm.cpu(), (xm * keep).sum(1) / keep.sum(1).clamp(min=1e-9), atol=1e-6, rtol=1e-5)
    t = torch.tensor([1.0, 0.9, 0.5, 0.1])
    emb = ops.sincos_time_embed(t.to(dev), 1024, 4e-3, 4.0)
    fr = torch.linspace(0.0, 1.0, 512, dtype=torch.float64)
    per = 4e-3 * (4.0 / 4e-3) ** fr
    arg = (1.0 / per * 2 * math.pi)[None] * t.double()[:, None]
    ref = torch.cat([arg.sin(), arg.cos()], 1).to(torch.bfloat16)
    assert torch.allclose(emb.float().cpu(), ref.float(), atol=8e-3)
    assert (emb.cpu() != ref).float().mean().item() < 0.01  # bf16 rounding of values computed in float64


# ------------------------------------------------------------------------------------------------ selection
def test_token_select(dev):
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(9, 32064, generator=g)
    logits[4, 100] = logits[4, 31999] = 50.0  # exact tie -> first index
    tok, lg = ops.token_select(logits.to(dev), 0, 32000)
    assert torch.equal(tok.cpu(), logits[:, :32000].argmax(-1))
    assert tok[4].item() == 100
    u = torch.rand(9, generator=g)
    tok, _ = ops.token_select(logits.to(dev), 31744, 32000, uniform=u.to(dev), temperature=0.7)
    sub = logits[:, 31744:32000].numpy()
    for r in range(9):
        p = np.exp(((sub[r] - sub[r].max()) / np.float32(0.7)).astype(np.float32)).astype(np.float32)
        cs = np.cumsum(p, dtype=np.float32)
        pick = int(np.argmax(cs > np.float32(u[r].item()) * cs[-1]))
        assert abs(tok[r].item() - (31744 + pick)) <= 0  # same arithmetic -> same index
    # wide greedy ranges (pi0-FAST: 257 152 logits): the 1024-thread vector path, ragged tail, ties, and the scalar path for an
    # unaligned lower bound -- first maximum wins everywhere
    wide = torch.randn(3, 257152, generator=g)
    wide[1, 7] = wide[1, 200003] = wide[1, 257149] = 60.0
    wide[2, 257149] = 70.0                                       # in the scalar tail of [4, 257150)
    for lo, hi in [(0, 257152), (4, 257150), (3, 257150)]:
        tok, lgv = ops.token_select(wide.to(dev), lo, hi)
        ref = wide[:, lo:hi].argmax(-1) + lo
        assert torch.equal(tok.cpu(), ref), (lo, hi)
        assert torch.equal(lgv.cpu(), wide[torch.arange(3), ref])
    assert ops.token_select(wide.to(dev), 0, 257152)[0][1].item() == 7


@pytest.mark.parametrize("N,gs", [(40, 5), (512, 16), (7, 7), (16, 1)])
def test_score_select(dev, N, gs):
    """score_rows_k (16 candidates per block: N = 40 / 7 leave a ragged last block, 512 = config 5) + group_argmax_k."""
    g = torch.Generator().manual_seed(4)
    M, dim = 3, 512
    it = torch.nn.functional.normalize(torch.randn(M, dim, generator=g), dim=-1)
    act = torch.nn.functional.normalize(torch.randn(M, N, dim, generator=g), dim=-1)
    scores, result, best, fit, fact = ops.score_select(it.to(dev), act.to(dev), gs)
    f_it = it.mean(0)
    f_it = f_it / f_it.norm()
    f_act = act.mean(0)
    f_act = f_act / f_act.norm(dim=-1, keepdim=True)
    ref = f_act @ f_it
    assert torch.allclose(scores.cpu(), ref, atol=1e-6)
    gm = ref.view(N // gs, gs).mean(1)
    bg = gm.argmax().item()
    bi = ref.view(N // gs, gs)[bg].argmax().item()
    assert result.cpu().tolist()[:3] == [bg * gs + bi, bg, bi]
    assert abs(best[0].item() - ref[bg * gs + bi].item()) < 1e-6
    assert torch.allclose(fit.cpu().view(-1), f_it, atol=1e-6) and torch.allclose(fact.cpu().view(N, dim), f_act, atol=1e-6)
    # ties: first maximum wins at both levels
    s = torch.zeros(12)
    r, _ = ops.group_argmax(s.to(dev), 3)
    assert r.cpu().tolist()[:3] == [0, 0, 0]
    s[7] = s[10] = 1.0
    r, _ = ops.group_argmax(s.to(dev), 3)
    assert r.cpu().tolist()[:3] == [7, 2, 1]


def test_attention_shared_keys_form_equals_the_per_tile_form(dev, tmp_path):
    """attn_shared_k (64 query rows of a (batch entry, head) share one LDS-staged copy of every K / V^T tile; the large-N decode pass) against (1) the per-tile
    kernel it replaces there (COVER_ATTN_SHARED=0 in a child process: the knob is read once) -- within 5e-3 rel-L2 (the key-split merge sums in another order; the
    non-split per-tile form is the same arithmetic in the same order) -- and (2) an fp32 softmax over [shared keys | own-entry keys] without the resumed state."""
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    outs = {}
    for knob in ("1", "0"):
        f = str(tmp_path / f"o{knob}.pt")
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_attn_shared_child.py"), f], env=dict(os.environ, COVER_ATTN_SHARED=knob, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        outs[knob] = torch.load(f)
    a, b = outs["1"]["resumed"].float(), outs["0"]["resumed"].float()        # 1 024 query tiles resumed from a state: the per-tile form runs key-split
    assert ((a - b).norm() / b.norm()).item() < 5e-3
    # without a state the per-tile form runs un-split: one wave walks a tile's keys in order, as a wave of the shared form does -- identical bits
    assert torch.equal(outs["1"]["plain"].view(torch.int16), outs["0"]["plain"].view(torch.int16))
    from _attn_shared_child import problem
    P, S, H, D, q, segs, state, (k0, v0, k1, v1, len1, T0) = problem(torch.device("cpu"))
    qq = q.float().view(P, S, 3, H, D)[:, :, 0]                                      # [P, S, H, D]
    ref = torch.empty(P, S, H, D)
    for pi in range(P):
        L1 = int(len1[pi])
        kk = torch.cat([k0[0, :T0].float(), k1[pi, :L1].float()], 0)                 # [T, H, D]
        vv = torch.cat([v0[0, :, :, :T0].float().permute(2, 0, 1), v1[pi, :, :, :L1].float().permute(2, 0, 1)], 0)
        sc = torch.einsum("shd,thd->hst", qq[pi], kk) * D ** -0.5
        pr = torch.softmax(sc, -1).to(torch.bfloat16).float()
        ref[pi] = torch.einsum("hst,thd->shd", pr, vv)
    got = outs["1"]["plain"].float().view(P, S, H, D)
    assert ((got - ref).norm() / ref.norm()).item() < 1.2e-2


def test_attention_state_chaining_decode(dev):
    # decode shape: shared segment attended with the candidates as query rows (phase A), then per-candidate segments
    # seeded with that state (phase B) == one call over all three segments
    N, Hq, Hkv, D = 32, 8, 8, 128
    T0, T1, T2 = 257, 24, 5
    g = torch.Generator().manual_seed(77)
    q = bf(torch.randn(N, 1, Hq, D, generator=g))
    k0, v0 = bf(torch.randn(1, T0, Hkv, D, generator=g)), bf(torch.randn(1, T0, Hkv, D, generator=g))
    k1, v1 = bf(torch.randn(8, T1, Hkv, D, generator=g)), bf(torch.randn(8, T1, Hkv, D, generator=g))
    k2, v2 = bf(torch.randn(N, T2, Hkv, D, generator=g)), bf(torch.randn(N, T2, Hkv, D, generator=g))
    slot1 = (torch.arange(N) // 4).to(torch.int32)
    len1 = (16 + slot1 % 8).to(torch.int32)
    zero = torch.zeros(N, dtype=torch.int32)
    c0, c1, c2 = make_cache(k0, v0, dev), make_cache(k1, v1, dev), make_cache(k2, v2, dev)
    s0 = ops.Segment(c0[0], c0[1], c0[2], c0[3], length=T0, slot_of_batch=zero.to(dev))
    s1 = ops.Segment(c1[0], c1[1], c1[2], c1[3], length=T1, slot_of_batch=slot1.to(dev), len_of_batch=len1.to(dev))
    s2 = ops.Segment(c2[0], c2[1], c2[2], c2[3], length=3)
    qd = q.to(dev)
    st = (Hq * D, Hq * D, D)
    one = torch.empty(N, 1, Hq, D, dtype=torch.bfloat16, device=dev)
    ops.attention(qd, st, one, st, N, 1, Hq, Hkv, D, D ** -0.5, [s0, s1, s2])
    so = torch.empty(N, Hq, D, dtype=torch.float32, device=dev)
    sml = torch.empty(N, Hq, 2, dtype=torch.float32, device=dev)
    ops.attention(qd, (0, Hq * D, D), None, st, 1, N, Hq, Hkv, D, D ** -0.5, [s0], state_out=(so, sml))
    two = torch.empty_like(one)
    ops.attention(qd, st, two, st, N, 1, Hq, Hkv, D, D ** -0.5, [s1, s2], state_in=(so, sml))
    vis0 = torch.ones(N, 1, T0, dtype=torch.bool)
    vis1 = (torch.arange(T1)[None, None, :] < len1[:, None, None])
    vis2 = (torch.arange(T2)[None, None, :] < 3).expand(N, 1, T2)
    ref = attn_ref(q, [(k0.expand(N, -1, -1, -1), v0.expand(N, -1, -1, -1), vis0), (k1[slot1.long()], v1[slot1.long()], vis1),
                       (k2, v2, vis2)], D ** -0.5)
    assert rel_l2(one, ref) < 1.2e-2 and rel_l2(two, ref) < 1.2e-2
    assert torch.allclose(one.float().cpu(), two.float().cpu(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("variant,M", [(3, 32), (3, 5), (1, 150)])
@pytest.mark.parametrize("style", [0, 1])
def test_gemm_fused_rmsnorm(dev, variant, M, style):
    # out = residual + A W^T ; norm_out = rmsnorm(out): fused into the split-K reduction on the streaming path
    N, K = 1024, 512
    g = torch.Generator().manual_seed(M + style)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.05)
    res = bf(torch.randn(M, N, generator=g))
    nw = torch.randn(N, generator=g) * 0.2 + (1.0 if style == 1 else 0.0)
    lin = ops.pack_linear(w.to(dev))
    x = res.clone().to(dev)
    h = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    ops.gemm(a.to(dev), lin, residual=x, out=x, variant=variant, norm_w=nw.to(dev), norm_out=h, norm_style=style,
             norm_w_offset=0.0 if style == 1 else 1.0, norm_eps=1e-6)
    ref_x = bf(res.float() + a.float() @ w.float().T)
    assert rel_l2(x, ref_x) < 6e-3
    xf = x.float().cpu()  # the norm must be the norm of what was actually stored
    rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)
    ref_h = bf(nw * bf(xf * rstd).float()) if style == 1 else bf(xf * rstd * (1 + nw))
    assert torch.allclose(h.float().cpu(), ref_h.float(), atol=2e-2, rtol=1e-2)


@pytest.mark.parametrize("M,N,K", [(257, 1024, 4096), (150, 1152, 1152), (300, 4096, 1024), (32, 1024, 512)])
def test_gemm_fused_layernorm(dev, M, N, K):
    # out = residual + ls * (A W^T + b) ; norm_out = LayerNorm(out) with the arithmetic of cover_layernorm_bf16: folded
    # into the split-K reduction when the GEMM splits K (ViT-sized outputs), a separate launch otherwise -- same values
    g = torch.Generator().manual_seed(M + N)
    a = bf(torch.randn(M, K, generator=g))
    w = bf(torch.randn(N, K, generator=g) * 0.05)
    bias = torch.randn(N, generator=g) * 0.1
    res = bf(torch.randn(M, N, generator=g))
    ls = torch.rand(N, generator=g) + 0.5
    nw, nb = torch.randn(N, generator=g) * 0.2 + 1.0, torch.randn(N, generator=g) * 0.1
    lin = ops.pack_linear(w.to(dev), bias.to(dev))
    x = res.clone().to(dev)
    h = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    ops.gemm(a.to(dev), lin, residual=x, layer_scale=ls.to(dev), out=x, norm_w=nw.to(dev), norm_b=nb.to(dev), norm_out=h,
             norm_style=2, norm_eps=1e-6)
    ref_x = bf(res.float() + ls * (a.float() @ w.float().T + bias))
    assert rel_l2(x, ref_x) < 6e-3
    h2 = ops.layernorm(x, nw.to(dev), nb.to(dev), 1e-6)   # the separate kernel on what was actually stored
    dh = (h.float() - h2.float()).abs().cpu()   # same arithmetic, different reduction tree: at most a rare 1-ulp flip
    assert dh.max() <= 0.04 and (dh > 0).float().mean() < 2e-3
    ref_h = torch.nn.functional.layer_norm(x.float().cpu(), (N,), nw, nb, 1e-6)
    assert torch.allclose(h.float().cpu(), ref_h, atol=3e-2, rtol=1e-2)


def test_tokens_to_histories_matches_host_path(dev):
    # device de-tokeniser + history assembly == the host path (numpy float64 -> fp32, front padding with -5)
    import numpy as np
    g = torch.Generator().manual_seed(12)
    N, vocab, nb = 9, 32000, 256
    tok = torch.randint(vocab - nb - 3, vocab + 2, (N, 7), generator=g)
    bins = np.linspace(-1, 1, nb)
    centers = (bins[:-1] + bins[1:]) / 2.0
    past = (torch.randn(6, 7, generator=g) * 0.02).double().numpy()
    hb, pad = ops.tokens_to_histories(tok.to(dev), vocab, torch.tensor(centers, dtype=torch.float32, device=dev),
                                      torch.tensor(past, dtype=torch.float32, device=dev))
    d = np.clip(vocab - tok.numpy() - 1, 0, centers.shape[0] - 1)
    a = centers[d]
    a[:, 6] = (a[:, 6] >= 0.5)
    ref = np.stack([np.vstack([np.ones((3, 7)) * -5, past, a[n][None]]) for n in range(N)]).astype(np.float32)
    assert np.array_equal(hb.cpu().numpy(), ref)
    assert np.array_equal(pad.cpu().numpy(), (ref[:, :, 0] == -5).astype(np.uint8))


@pytest.mark.parametrize("n_past,n_use", [(0, 2), (6, 2), (6, 4), (0, 4), (3, 3), (0, 10), (2, 8)])
def test_tokens_to_histories_steps_matches_host_path(dev, n_past, n_use):
    """Action-chunk horizon > 1 (BASELINE config 5): the first n_use 7-token actions of a candidate's chunk become its n_use newest
    history rows. Reference = the de-tokeniser arithmetic (policy_wrapper.py:259-266) per step, then host.process_inputs'
    [past | future steps] stacking (eval_utils.py:172-214) with the verifier gripper rule, then the front padding of
    efficient_ensemble_merged.py:378-390. Bit-exact (table look-ups and copies)."""
    import numpy as np
    g = torch.Generator().manual_seed(31 + 16 * n_past + n_use)
    N, vocab, nb = 11, 32000, 256
    width = 7 * n_use + (7 if n_use % 2 else 0)              # the token row may be longer than the steps that are used
    tok = torch.randint(vocab - nb - 3, vocab + 2, (N, width), generator=g)
    bins = np.linspace(-1, 1, nb)
    centers = (bins[:-1] + bins[1:]) / 2.0
    history = [(torch.randn(7, generator=g) * 0.02).double().numpy() for _ in range(n_past)]
    past = torch.tensor(np.stack(history), dtype=torch.float32, device=dev) if n_past else None
    hb, pad = ops.tokens_to_histories(tok.to(dev), vocab, torch.tensor(centers, dtype=torch.float32, device=dev), past, n_use=n_use)
    d = np.clip(vocab - tok.numpy()[:, : 7 * n_use].reshape(N, n_use, 7) - 1, 0, centers.shape[0] - 1)
    a = centers[d]                                            # [N, n_use, 7]
    a[..., 6] = np.where(a[..., 6] < 0.5, 0, 1)               # postprocess_gripper_verifier (simpler.py:222-226)
    ref = np.full((N, 10, 7), -5.0, dtype=np.float32)
    for n in range(N):
        rows = np.vstack(history + [a[n]]) if n_past else a[n]
        ref[n, 10 - rows.shape[0]:] = rows.astype(np.float32)
    assert np.array_equal(hb.cpu().numpy(), ref)
    want_pad = np.zeros((N, 10), dtype=np.uint8)
    want_pad[:, : 10 - n_past - n_use] = 1
    assert np.array_equal(pad.cpu().numpy(), want_pad)


@pytest.mark.parametrize("n_past,n_use,denorm", [(6, 4, True), (0, 4, True), (2, 1, False), (6, 1, True), (0, 10, False)])
def test_actions_to_histories_matches_host_path(dev, n_past, n_use, denorm):
    # device post-processing of flow-matching chunks == host.process_inputs(verifier_action=True) + front padding
    import numpy as np
    from cover_vla_amd import host
    g = torch.Generator().manual_seed(100 + n_past * 16 + n_use)
    N, chunk, width = 13, max(n_use, 4), 32
    x = torch.rand(N, chunk, width, generator=g) * 2.4 - 1.2
    x[0, 0, 6] = 0.5                                     # the gripper threshold itself binarises to 1
    history = [(torch.randn(7, generator=g) * 0.02).double().numpy() for _ in range(n_past)]
    past = torch.tensor(np.stack(history), dtype=torch.float32, device=dev) if n_past else None
    st = host.bridge_statistics()["action"]
    lo_hi = torch.tensor(list(st["p01"][:6]) + list(st["p99"][:6]), dtype=torch.float32, device=dev) if denorm else None
    hb, pad = ops.actions_to_histories(x.to(dev)[:, :, :7] if n_use % 2 else x.to(dev), n_use, past, lo_hi)
    if denorm:
        queue = [x[:, t, :7].numpy() for t in range(n_use)]
        rows = host.process_inputs(queue, True, history, n_use)
    else:
        a = x[:, :n_use, :7].double().numpy().copy()
        a[..., 6] = np.where(a[..., 6] < 0.5, 0, 1)
        rows = [np.vstack(history + [a[n]]) if n_past else a[n] for n in range(N)]
    n_pad = 10 - n_past - n_use
    ref = np.stack([np.vstack([np.full((n_pad, 7), -5.0), r]) for r in rows])
    got = hb.cpu().numpy()
    assert np.array_equal(got[:, :n_pad + n_past], ref[:, :n_pad + n_past].astype(np.float32))
    assert np.array_equal(got[..., 6], ref[..., 6].astype(np.float32))
    assert np.abs(got - ref).max() <= 5e-7               # fp32 arithmetic vs float64 on the host (|values| < 0.5)
    assert np.array_equal(pad.cpu().numpy(), (ref[:, :, 0] == -5).astype(np.uint8))
    with pytest.raises(Exception):
        ops.actions_to_histories(x.to(dev), 7, torch.zeros(6, 7, device=dev), None)


@pytest.mark.parametrize("D,H", [(128, 8), (64, 4)])
@pytest.mark.parametrize("N,write_t,mode,from_partials", [(32, 0, 1, False), (32, 4, 2, True), (21, 3, 1, True), (5, 6, 0, False),
                                                         (64, 5, 1, False), (144, 2, 2, True)])
def test_decode_attention_fused_matches_three_launch_path(dev, D, H, N, write_t, mode, from_partials):
    _decode_attention_case(dev, D, H, N, write_t, mode, from_partials, permute_slots=False)


@pytest.mark.parametrize("D,H", [(128, 8), (64, 4)])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n_splits", [1, 4, 6])
def test_decode_attention_fused_folds_any_number_of_slabs(dev, D, H, mode, n_splits):
    """The QKV GEMM hands over up to 8 split-K slabs: one, exactly the four the kernel holds in registers, and more than four (read in a
    loop). N = 21: a partly filled second candidate tile. Appended K / V^T bit-equal to rope_kv_write folding the same slabs."""
    _decode_attention_case(dev, D, H, 21, 3, mode, True, permute_slots=False, n_splits=n_splits)


def test_decode_attention_fused_at_many_units_with_long_own_segments(dev):
    """The regime where cover_decoder_forward switches from the fused launch to the three-launch path (>= 768 (tile, head) units and
    > 16 own keys, BASELINE config 5): both paths must agree there too. N = 400 candidates x 32 heads, 20 own keys."""
    _decode_attention_case(dev, 128, 32, 400, 19, 2, False, permute_slots=False)


def test_decode_attention_fused_with_an_explicit_own_slot_table(dev):
    # candidates' own-token segments live in permuted cache slots (write_slot_of_batch / seg[2].slot_of_batch)
    _decode_attention_case(dev, 128, 8, 29, 3, 2, True, permute_slots=True)


@pytest.mark.parametrize("N,pattern", [(32, "interleaved"), (29, "interleaved"), (40, "scattered"), (144, "interleaved")])
def test_decode_attention_fused_with_recurring_prompt_slots(dev, N, pattern):
    """a prompt slot that recurs NON-contiguously inside a 16-candidate tile (0,1,0,1,... / a random assignment) must
    enter every candidate's softmax once. Checked against the three-launch path AND directly against fp32 torch."""
    _decode_attention_case(dev, 128, 8, N, 3, 2, True, permute_slots=False, slot_pattern=pattern, check_fp32=True)


def test_decode_attention_fused_random_sweep(dev):
    """60 random shapes of the fused decode attention (head dim, heads, candidates 1..200, own keys 1..21, RoPE mode, qkv from split-K
    slabs or rows, permuted own slots, prompt-slot patterns) against the RoPE launch + generic attention and, for the recurring-slot
    patterns, fp32 torch; appended K / V^T bit-exact."""
    import random
    rnd = random.Random(5)
    for _ in range(60):
        D, H = rnd.choice([(128, 8), (128, 32), (64, 4), (128, 16), (64, 16)])
        N = rnd.choice([rnd.randint(1, 16), rnd.randint(17, 64), rnd.randint(65, 200)])
        if H * ((N + 15) // 16) > 1400:
            N = 64
        write_t = rnd.choice([0, 0, rnd.randint(1, 7), rnd.randint(8, 20)])
        pattern = rnd.choice(["grouped", "interleaved", "scattered"])
        _decode_attention_case(dev, D, H, N, write_t, rnd.randint(0, 2), rnd.random() < 0.5, permute_slots=rnd.random() < 0.3,
                               slot_pattern=pattern, check_fp32=(pattern != "grouped" and N <= 48))


def _rope_ref(x, pos, cos, sin, mode):
    """x fp32 [N, H, D] (bf16 values), the two RoPE arithmetics of rope_kv_write restated in torch (bf16 roundings where the kernel has them)."""
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    c, s = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    r = lambda t: t.bfloat16().float()
    if mode == 0:
        return x
    if mode == 2:
        c, s = r(c), r(s)
        return torch.cat([r(r(x1 * c) + r(-x2 * s)), r(r(x2 * c) + r(x1 * s))], -1)
    return torch.cat([r(x1 * c - x2 * s), r(x2 * c + x1 * s)], -1)


def _fq_rows_e4m3(x):
    """per-row (last dim) power-of-two scale + RNE e4m3, de-quantised: the own-token fp8 cache's quantiser restated"""
    amax = x.abs().amax(-1, keepdim=True)
    s = torch.where(amax > 0, torch.pow(2.0, torch.ceil(torch.log2(amax.double() / 448.0))).float(), torch.ones_like(amax))
    return (x / s).to(torch.float8_e4m3fn).float() * s, s


@pytest.mark.parametrize("D,H,N,S,steps,mode,fp8", [(128, 32, 64, 16, 3, 2, False), (128, 32, 64, 16, 3, 2, True), (128, 8, 96, 24, 9, 2, True),
                                                     (128, 8, 40, 5, 18, 1, False), (64, 4, 30, 6, 7, 2, True), (64, 4, 30, 6, 7, 0, False),
                                                     (128, 8, 48, 12, 56, 2, True), (128, 8, 48, 12, 56, 2, False)])
def test_decode_own_attention_chain_matches_fp32_torch(dev, D, H, N, S, steps, mode, fp8):
    """Large-N candidate decode (BASELINE config 5): own-token VALU pass (RoPE + append into the head-major own cache, bf16 or e4m3 with
    per-row scales, + attention over the own keys, state out) chained into ONE MFMA pass over [shared prefix | prompt text] with the S
    samples of a prompt as the query rows of a batch entry -- run for `steps` consecutive decode steps -- against an fp32 torch
    softmax over [K0 | K1[prompt] | own keys so far]. The reference attends the values the cache holds (bf16 rows, or the e4m3
    quantiser restated in torch): what is checked is the attention arithmetic and the append, with the usual bf16-P tolerance.
    The cache contents themselves are compared exactly (appended rows, scales)."""
    T0, T1, cap, npos = 257, 24, 64, 400
    P = N // S
    g = torch.Generator().manual_seed(7 * N + steps + D)
    ncol = 3 * H * D
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(npos).float()[:, None] * inv[None]
    cos, sin = ang.cos(), ang.sin()
    k0, v0 = bf(torch.randn(1, T0, H, D, generator=g)), bf(torch.randn(1, T0, H, D, generator=g))
    k1, v1 = bf(torch.randn(P, T1, H, D, generator=g)), bf(torch.randn(P, T1, H, D, generator=g))
    len1 = (9 + (torch.arange(P) * 5) % 16).to(torch.int32)
    c0, c1 = make_cache(k0, v0, dev), make_cache(k1, v1, dev)
    s0 = ops.Segment(c0[0], c0[1], c0[2], c0[3], length=T0, slot_of_batch=torch.zeros(N, dtype=torch.int32, device=dev))
    s1 = ops.Segment(c1[0], c1[1], c1[2], c1[3], length=T1, len_of_batch=len1.to(dev))         # slot = batch entry = prompt
    # the caches start POISONED (NaN bit patterns, NaN scales): rows at or beyond write_t are loaded under a mask (clamped index) and
    # must contribute exactly nothing -- the public entry point documents no zero-initialisation requirement
    if fp8:
        k_own = torch.full((N, H, cap, D), 0x7F, dtype=torch.uint8, device=dev)          # e4m3fn NaN
        v_own = k_own.clone()
        ks = torch.full((N, H, cap), float("nan"), dtype=torch.float32, device=dev)
        vs = ks.clone()
    else:
        k_own = torch.full((N, H, cap, D), float("nan"), dtype=torch.bfloat16, device=dev)
        v_own = k_own.clone()
        ks = vs = None
    state = (torch.empty(N, H, D, dtype=torch.float32, device=dev), torch.empty(N, H, 2, dtype=torch.float32, device=dev))
    own_k, own_v = [], []                                   # reference: the values the cache should hold, [N, H, D] per step
    for t in range(steps):
        qkv = bf(torch.randn(N, ncol, generator=g))
        pos = torch.randint(0, npos, (N,), generator=g, dtype=torch.int32)
        x = qkv.float().view(N, 3, H, D)
        q_ref = _rope_ref(x[:, 0], pos, cos, sin, mode)
        k_new, v_new = _rope_ref(x[:, 1], pos, cos, sin, mode), x[:, 2]
        if fp8:
            k_new, ksc = _fq_rows_e4m3(k_new)
            v_new, vsc = _fq_rows_e4m3(v_new)
        own_k.append(k_new)
        own_v.append(v_new)
        qd = qkv.clone().to(dev)
        ops.decode_own_attention(qd, N, H, D, D ** -0.5, k_own, v_own, cap, t, state, positions=pos.to(dev), cos=cos.to(dev), sin=sin.to(dev),
                                 rope_mode=mode, k_scale=ks, v_scale=vs)
        out = torch.full((N, H * D), float("nan"), dtype=torch.bfloat16, device=dev)
        ops.attention(qd, (S * ncol, ncol, D), out, (S * H * D, H * D, D), P, S, H, H, D, D ** -0.5, [s0, s1], state_in=state)
        # q rotated in place, exactly
        assert torch.equal(qd[:, :H * D].float().cpu().view(N, H, D), q_ref)
        # appended cache rows, exactly
        if fp8:
            got_k = k_own[:, :, t].cpu().view(torch.float8_e4m3fn).float() * ks[:, :, t].cpu()[..., None]
            got_v = v_own[:, :, t].cpu().view(torch.float8_e4m3fn).float() * vs[:, :, t].cpu()[..., None]
            assert torch.equal(ks[:, :, t].cpu(), ksc[..., 0]) and torch.equal(vs[:, :, t].cpu(), vsc[..., 0])
        else:
            got_k, got_v = k_own[:, :, t].float().cpu(), v_own[:, :, t].float().cpu()
        assert torch.equal(got_k, k_new) and torch.equal(got_v, v_new)
        if t in (0, 1, steps // 2, steps - 1):
            kk_own, vv_own = torch.stack(own_k, 1), torch.stack(own_v, 1)                       # [N, t+1, H, D]
            exp = torch.empty(N, H, D)
            for n in range(N):
                p, ln = n // S, int(len1[n // S])
                kk = torch.cat([k0[0].float(), k1[p, :ln].float(), kk_own[n]], 0)
                vv = torch.cat([v0[0].float(), v1[p, :ln].float(), vv_own[n]], 0)
                sc = torch.einsum("hd,thd->ht", q_ref[n], kk) * D ** -0.5
                exp[n] = torch.einsum("ht,thd->hd", torch.softmax(sc, -1), vv)
            o, e = out.float().cpu(), exp.view(N, H * D)
            assert torch.isfinite(o).all()
            assert rel_l2(o, e) < 8e-3 and (o - e).abs().max() < 4e-2, (t, rel_l2(o, e), (o - e).abs().max())


def _decode_attention_case(dev, D, H, N, write_t, mode, from_partials, permute_slots, slot_pattern="grouped", check_fp32=False, n_splits=3):
    # one launch (RoPE + KV append + [shared | per-prompt | own] attention) == rope_kv_write + attention over 3 segments
    # (N = 144: more than 128 (candidate tile, head) units for H = 8, i.e. the unsplit VS = 1 variant; fewer: VS = 2)
    T0, T1, cap2, npos = 257, 24, 32, 320
    g = torch.Generator().manual_seed(1000 * N + 10 * write_t + mode)
    ncol = 3 * H * D
    if from_partials:
        part = torch.randn(n_splits, N, ncol, generator=g) * 0.6
        bias = torch.randn(ncol, generator=g) * 0.1
        qkv = bf(part.sum(0) + bias)
    else:
        part = bias = None
        qkv = bf(torch.randn(N, ncol, generator=g))
    pos = torch.randint(0, npos, (N,), generator=g, dtype=torch.int32)
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(npos).float()[:, None] * inv[None]
    cos, sin = ang.cos().to(dev), ang.sin().to(dev)
    k0, v0 = bf(torch.randn(1, T0, H, D, generator=g)), bf(torch.randn(1, T0, H, D, generator=g))
    k1, v1 = bf(torch.randn(8, T1, H, D, generator=g)), bf(torch.randn(8, T1, H, D, generator=g))
    k2, v2 = bf(torch.randn(N, cap2, H, D, generator=g)), bf(torch.randn(N, cap2, H, D, generator=g))
    if slot_pattern == "grouped":
        slot1 = (torch.arange(N) // 3 % 8).to(torch.int32)     # prompt groups straddle the 16-candidate tiles
    elif slot_pattern == "interleaved":
        slot1 = (torch.arange(N) % 3).to(torch.int32)          # 0,1,2,0,1,2,...: every slot recurs inside every tile
    else:
        slot1 = torch.randint(0, 8, (N,), generator=g, dtype=torch.int32)
    len1 = (9 + (slot1 * 5) % 16).to(torch.int32)
    zero = torch.zeros(N, dtype=torch.int32)
    c0, c1 = make_cache(k0, v0, dev), make_cache(k1, v1, dev)
    ca, cb = make_cache(k2, v2, dev, cap2), make_cache(k2, v2, dev, cap2)
    s0 = ops.Segment(c0[0], c0[1], c0[2], c0[3], length=T0, slot_of_batch=zero.to(dev))
    s1 = ops.Segment(c1[0], c1[1], c1[2], c1[3], length=T1, slot_of_batch=slot1.to(dev), len_of_batch=len1.to(dev))
    L2 = write_t + 1
    slot2 = torch.randperm(N, generator=g).to(torch.int32).to(dev) if permute_slots else None
    # reference path
    qa = qkv.clone().to(dev)
    ops.rope_kv_write(qa, N, 1, H, H, D, positions=pos.to(dev), cos=cos, sin=sin, rope_mode=mode, k_cache=ca[0], k_strides=ca[2],
                      vt_cache=ca[1], vt_strides=ca[3], t_offset=write_t, slot_of_batch=slot2)
    ref = torch.empty(N, H * D, dtype=torch.bfloat16, device=dev)
    ops.attention(qa, (ncol, ncol, D), ref, (H * D, H * D, D), N, 1, H, H, D, D ** -0.5,
                  [s0, s1, ops.Segment(ca[0], ca[1], ca[2], ca[3], length=L2, slot_of_batch=slot2)])
    # fused path
    out = torch.full((N, H * D), float("nan"), dtype=torch.bfloat16, device=dev)
    ops.decode_attention_fused(qkv.to(dev), N, H, D, D ** -0.5, [s0, s1, ops.Segment(cb[0], cb[1], cb[2], cb[3], length=L2, slot_of_batch=slot2)],
                               write_t, out, positions=pos.to(dev), cos=cos, sin=sin, rope_mode=mode,
                               partial=None if part is None else part.to(dev), bias=None if bias is None else bias.to(dev))
    assert torch.equal(ca[0].cpu().view(torch.int16), cb[0].cpu().view(torch.int16))       # appended K rows, bit-exact
    assert torch.equal(ca[1].cpu().view(torch.int16), cb[1].cpu().view(torch.int16))       # appended V^T columns
    o, r = out.float().cpu(), ref.float().cpu()
    assert torch.isfinite(o).all()
    assert rel_l2(o, r) < 6e-3 and (o - r).abs().max() < 3e-2
    if check_fp32:
        # direct fp32 restatement from the caches the fused launch left behind: softmax(q . [K0 | K1[slot] | K2[own]]) V
        kc2 = cb[0].float().cpu().view(N, cap2, H, D)
        vt2 = cb[1].float().cpu().view(N, H, D, cap2)
        q = qa[:, :H * D].float().cpu().view(N, H, D)          # rotated in place by the reference path's rope_kv_write
        exp = torch.empty(N, H, D)
        for n in range(N):
            sl, ln = int(slot1[n]), int(len1[n])
            own = int(slot2[n]) if slot2 is not None else n
            kk = torch.cat([k0[0].float(), k1[sl, :ln].float(), kc2[own, :L2]], 0)                       # [T, H, D]
            vv = torch.cat([v0[0].float(), v1[sl, :ln].float(), vt2[own, :, :, :L2].permute(2, 0, 1)], 0)
            sc = torch.einsum("hd,thd->ht", q[n], kk) * D ** -0.5
            exp[n] = torch.einsum("ht,thd->hd", torch.softmax(sc, -1), vv)
        e = exp.view(N, H * D)
        assert rel_l2(o, e) < 8e-3 and (o - e).abs().max() < 4e-2   # bf16 probabilities and output rounding
