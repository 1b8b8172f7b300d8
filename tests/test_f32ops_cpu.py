"""The fp32 GEMM's dispatch table (cover_gemm_f32_plan: no launch, no GPU) one condition at a time, the proof that the shared GEMM case table
of tests/f32_ref.py reaches every kernel with ragged edges, and the evidence that the references and bounds test_f32ops_gpu.py asserts
are sound: plain CPU fp32 restatements sit inside them.

Pointers are fake addresses: the plan query only checks them for null and alignment."""
import numpy as np
import pytest
import torch

from cover_vla_amd import ops
from tests import f32_ref as R

A, B, C = R.FAKE_A, R.FAKE_B, R.FAKE_C


def plan(M, N, K, a_rs=None, a_ks=1, b_rs=None, b_ks=1, a_ptr=A, b_ptr=B, c_ptr=C, **kw):
    name, deep = ops.gemm_f32_plan(a_ptr, K if a_rs is None else a_rs, a_ks, b_ptr, K if b_rs is None else b_rs, b_ks, c_ptr, N, M, N, K, **kw)
    assert not deep      # the COVER_F32_UNR=8 window is an experiment knob, off by default
    return name


# ------------------------------------------------------------------------------------------------ dispatch table
def test_plan_m_16_vs_17_picks_the_fragment_count():
    assert plan(1, 512, 512) == "DIRECT_FM1"
    assert plan(16, 512, 512) == "DIRECT_FM1"
    assert plan(17, 512, 512) == "DIRECT_FM2"
    assert plan(0, 512, 512) is None and plan(16, 0, 512) is None


def test_plan_k_needs_64_and_a_multiple_of_16_for_the_direct_kernel():
    assert plan(16, 64, 48) == "TILE32_K32"        # K % 16 == 0 but K < 64
    assert plan(16, 64, 64) == "DIRECT_FM1"
    assert plan(16, 64, 72) == "TILE32_K32"        # K >= 64 but K % 16 != 0
    assert plan(16, 64, 80) == "DIRECT_FM1"
    assert plan(33, 64, 80) == "DIRECT_FM2"
    assert plan(16, 64, 255) == "TILE32_K32" and plan(16, 64, 264) == "TILE32_K128"   # the tiled pair splits at K = 256
    assert plan(16, 64, 256) == "DIRECT_FM1"


def test_plan_strides_and_alignment_fall_back_to_the_tiled_kernels():
    assert plan(33, 64, 128, a_rs=136) == "DIRECT_FM2"                      # a padded row stride that stays a multiple of 4
    assert plan(33, 64, 128, a_rs=129) == "TILE32_K32"                      # row stride % 4 != 0
    assert plan(33, 64, 128, b_rs=130) == "TILE32_K32"
    assert plan(33, 64, 256, a_rs=258) == "TILE32_K128"
    assert plan(33, 64, 128, a_ptr=A + 4) == "TILE32_K32"                   # base pointer off by one element
    assert plan(33, 64, 128, b_ptr=B + 4) == "TILE32_K32"
    assert plan(33, 64, 128, a_ptr=A + 16, b_ptr=B + 32) == "DIRECT_FM2"
    assert plan(33, 64, 128, c_ptr=C + 4) == "DIRECT_FM2"                   # C is written with scalar stores: no alignment rule
    assert plan(33, 64, 128, a_rs=1, a_ks=33) == "TILE32_K32"               # column-major A
    assert plan(33, 64, 128, b_rs=1, b_ks=64) == "TILE32_K32"               # B as [K, N]
    assert plan(33, 64, 128, batch=2, a_bs=33 * 128, b_bs=64 * 128) == "DIRECT_FM2"
    assert plan(33, 64, 128, batch=2, a_bs=33 * 128 + 2, b_bs=64 * 128) == "TILE32_K32"   # batch strides % 4 != 0
    assert plan(33, 64, 128, batch=2, a_bs=33 * 128, b_bs=64 * 128 + 1) == "TILE32_K32"
    assert plan(33, 64, 128, batch=2, a_bs=0, b_bs=0) == "DIRECT_FM2"       # shared operands


def test_plan_block_counts_on_either_side_of_256_and_of_the_direct_bound():
    assert plan(1024, 1024, 7) == "TILE64"                                  # 16 x 16 = 256 blocks of 64 x 64
    assert plan(1024, 960, 7) == "TILE32_K32"                               # 240
    assert plan(1024, 960, 257) == "TILE32_K128"
    assert plan(1024, 1024, 257) == "TILE64"
    assert plan(512, 512, 33, batch=4, a_bs=512 * 33, b_bs=512 * 33) == "TILE64"       # the batch counts: 8 x 8 x 4
    assert plan(512, 512, 33, batch=3, a_bs=512 * 33, b_bs=512 * 33) == "TILE32_K32"
    assert plan(1000, 1030, 64) == "DIRECT_FM2"                             # k-contiguous: direct whatever the grid, up to the bound
    assert plan(8192, 8128, 64) == "DIRECT_FM2"                             # 128 x 127 = 16256 < 16384
    assert plan(8192, 8192, 64) == "TILE64"                                 # 16384: not below the bound
    assert plan(16, 8192 * 128, 64) == "TILE64"


def test_plan_direct_max_override_is_read_per_call(monkeypatch):
    assert plan(16, 64, 64) == "DIRECT_FM1" and plan(2048, 2048, 64) == "DIRECT_FM2"
    monkeypatch.setenv("COVER_F32_DIRECT_MAX", "0")
    assert plan(16, 64, 64) == "TILE32_K32" and plan(17, 64, 256) == "TILE32_K128" and plan(2048, 2048, 64) == "TILE64"
    monkeypatch.setenv("COVER_F32_DIRECT_MAX", "1024")
    assert plan(2048, 2048, 64) == "TILE64" and plan(2048, 1984, 64) == "DIRECT_FM2"   # 1024 and 992 blocks
    monkeypatch.delenv("COVER_F32_DIRECT_MAX")
    assert plan(2048, 2048, 64) == "DIRECT_FM2"


def test_plan_query_rejects_null_pointers():
    with pytest.raises(ops.L.CoverError):
        ops.gemm_f32_plan(None, 64, 1, B, 64, 1, C, 64, 16, 64, 64)


# ------------------------------------------------------------------------------------------------ the shared GEMM case table
CASES = R.gemm_cases()


def case_plan(cs):
    args, kw = R.gemm_plan_args(cs)
    return ops.gemm_f32_plan(*args, **kw)[0]


def test_case_table_reaches_every_kernel_with_ragged_edges():
    assert 60 <= len(CASES) <= 100
    seen = {p: dict(n=0, ragged_m=0, ragged_n=0) for p in ops.GEMM_F32_PLANS}
    for cs in CASES:
        p = case_plan(cs)
        tm, tn = R.TILE[p]
        seen[p]["n"] += 1
        seen[p]["ragged_m"] += cs["M"] % tm != 0
        seen[p]["ragged_n"] += cs["N"] % tn != 0
    print({p: tuple(v.values()) for p, v in seen.items()})
    for p, v in seen.items():
        assert v["n"] >= 3 and v["ragged_m"] >= 1 and v["ragged_n"] >= 1, (p, v)


def test_case_table_covers_the_arguments_the_callers_use(monkeypatch):
    has = lambda f: any(f(cs) for cs in CASES)   # noqa: E731
    for lay in ("contig", "padded", "colmajor", "offset1", "oddstride"):
        assert has(lambda cs: cs["a"] == lay)
    for lay in ("nk", "kn", "nk_strided"):
        assert has(lambda cs: cs["b"] == lay)
    for res in ("none", "own", "inplace"):
        assert has(lambda cs: cs["res"] == res and cs["batch"] == 1) and has(lambda cs: cs["res"] == res and cs["batch"] > 1)
    for nb in (1, 2, 5):
        assert has(lambda cs: cs["batch"] == nb)
    assert has(lambda cs: cs["a_shared"]) and has(lambda cs: cs["b_shared"]) and has(lambda cs: cs["c_bs_pad"] > 0)
    assert has(lambda cs: cs["bias"] == "batch" and cs["batch"] > 1) and has(lambda cs: cs["bias"] == "shared" and cs["batch"] > 1)
    for act in R.ACTS:
        assert has(lambda cs: cs["act"] == act)
    for alpha in R.ALPHAS:
        assert has(lambda cs: cs["alpha"] == alpha)
    assert {cs["M"] for cs in CASES} >= set(R.MS) and {cs["N"] for cs in CASES} >= set(R.NS) and {cs["K"] for cs in CASES} >= set(R.KS)
    # every directly dispatched case has a tiled twin (the exact check reruns it with the direct kernel off)
    direct = [cs for cs in CASES if case_plan(cs).startswith("DIRECT")]
    monkeypatch.setenv("COVER_F32_DIRECT_MAX", "0")
    assert len(direct) >= 10 and {case_plan(cs) for cs in direct} == {"TILE64", "TILE32_K128", "TILE32_K32"}
    for cs in CASES:
        assert cs["K"] * 16 < 2 ** 24            # exact check: every partial sum of products of integers in [-4, 4] is representable


@pytest.mark.parametrize("cs", CASES, ids=[cs["id"] for cs in CASES])
def test_cpu_fp32_matmul_sits_inside_the_gemm_bound_and_the_exact_check_is_exact(cs):
    """torch's own CPU fp32 matmul + epilogue (another summation order, another libm) against the float64 reference: inside the bound the GPU
    test asserts, on the whole table -- the bound is not too tight; and bit-equal on the integer operands of the exact check."""
    for kind, (act, alpha) in (("bounded", (cs["act"], cs["alpha"])), ("exact", R.exact_epilogue(cs))):
        t = R.gemm_build(cs, kind, "cpu")
        res_before = None if t["res"] is None else t["res"].clone()
        b = t["b"] if cs["b"] == "kn" else t["b"].transpose(-1, -2)
        x = torch.matmul(t["a"], b)
        if t["bias"] is not None:
            x = x + (t["bias"].view(cs["batch"], 1, cs["N"]) if cs["bias"] == "batch" else t["bias"])
        y = R.ACT64[act](x) * torch.tensor(alpha, dtype=torch.float32)
        if res_before is not None:
            y = res_before + y
        assert y.dtype == torch.float32
        t["out"].copy_(y)
        ref = R.gemm_ref64(cs, t, act, alpha, res_before)
        err = (t["out"].double() - ref).abs()
        if kind == "exact":
            assert torch.equal(t["out"].double(), ref)
        else:
            bound = R.gemm_bound(cs, t, act, alpha, res_before)
            assert bool((err <= bound).all()), (err / bound).max().item()
        assert R.outside_untouched(t, cs)


# ------------------------------------------------------------------------------------------------ the other references
def test_mha_ref64_is_scaled_dot_product_attention():
    g = torch.Generator().manual_seed(3)
    for B_, Tq, Tk, H, Dh in R.MHA_SHAPES:
        q, k, v = (torch.randn(B_, t, H * Dh, generator=g) for t in (Tq, Tk, Tk))
        pad = torch.zeros(B_, Tk, dtype=torch.bool)
        pad[0, :Tk - 1] = True
        ref = R.mha_ref64(q, k, v, H, Dh, pad)
        qh, kh, vh = (x.double().reshape(B_, -1, H, Dh).transpose(1, 2) for x in (q, k, v))
        sd = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=~pad[:, None, None, :])
        assert torch.allclose(ref, sd.transpose(1, 2).reshape(B_, Tq, H * Dh), atol=1e-6)   # (the helper scales by the kernel's fp32 Dh^-1/2)
    pad[:] = True
    assert R.mha_ref64(q, k, v, H, Dh, pad).isnan().all()


@pytest.mark.parametrize("dim", R.ROW_WIDTHS)
def test_layernorm_two_pass_restatement_meets_the_tolerances(dim):
    g = torch.Generator().manual_seed(dim)
    x, w, b = torch.randn(9, dim, generator=g), torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    got = torch.from_numpy(R.layernorm_two_pass_f32(x.numpy(), w.numpy(), b.numpy()))
    assert torch.allclose(got.double(), R.layernorm_ref64(x, w, b), atol=2e-5, rtol=2e-5)
    assert torch.allclose(got, torch.nn.functional.layer_norm(x, (dim,), w, b), atol=2e-5, rtol=2e-5)
    if dim > 1:
        xo = x + 100.0
        atol = R.layernorm_offset_atol(xo, w)
        assert 2e-5 < atol < 2e-4
        got = torch.from_numpy(R.layernorm_two_pass_f32(xo.numpy(), w.numpy(), b.numpy()))
        assert torch.allclose(got.double(), R.layernorm_ref64(xo, w, b), atol=atol, rtol=2e-5)
    const = torch.full((2, dim), 3.25)
    assert torch.equal(torch.from_numpy(R.layernorm_two_pass_f32(const.numpy(), w.numpy(), b.numpy())), b.expand(2, dim))


def test_xent_and_masked_mean_references_match_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 9, generator=g) * 80
    x[2, 0] = x[2, 7] = x[2, 2]
    loss, rank = R.xent_diag_ref64(x)
    assert torch.allclose(loss, torch.nn.functional.cross_entropy(x.double(), torch.arange(6), reduction="none"), atol=1e-12)
    order = torch.argsort(x[2], descending=True, stable=True)       # stable: equal logits keep column order
    assert rank[2].item() == order.tolist().index(2) and rank[2].item() == (x[2] > x[2, 2]).sum().item() + 1
    xm = torch.randn(3, 10, 5, generator=g)
    pad = torch.zeros(3, 10, dtype=torch.bool)
    pad[0, 4:] = True
    pad[1] = True
    mm = R.masked_mean_ref64(xm, pad)
    assert torch.allclose(mm[0], xm[0, :4].double().mean(0)) and torch.equal(mm[1], torch.zeros(5, dtype=torch.float64))
    assert torch.allclose(R.masked_mean_ref64(xm, None), xm.double().mean(1))


def test_sincos_float64_restatement_rounds_to_the_reference_bf16():
    """the kernel's formula in numpy float64, rounded to bf16, against the torch float64 reference: zero mismatches, so the 1 % the GPU test
    allows is headroom for the device's sin / cos / pow only"""
    t = torch.tensor([0.0, 1e-3, 0.5, 1.0])
    for dim in (2, 4, 30, 1024):
        ref = R.sincos_ref64(t, dim, 4e-3, 4.0)
        got = R.sincos_numpy_bf16(t.numpy(), dim, 4e-3, 4.0)
        assert got.shape == ref.shape == (4, dim)
        assert int((got != ref).sum()) == 0, dim
