"""tests/rowops_ref.py against torch on the CPU, the binding of the two entry points the row-kernel tests need, and the proof that the
acceptance rule of test_rowops_gpu.py (bf16(ref64) or a neighbour, at most 1e-3 of a case not equal) is met by plain fp32 arithmetic at every
width the GPU tests use. No GPU."""
import ctypes as C
import os

import pytest
import torch

from tests import rowops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ binding and signatures
def test_header_binding_and_struct_agree():
    from cover_vla_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert ("int cover_rmsnorm_bf16_q8(const void* x, int x_f32, int ldx, const float* w, float w_offset, int style, void* y, int ldy,\n"
            "                          int rows, int dim, float eps, void* q8, int ld8, float* q8s, void* stream);") in hdr
    assert "int cover_rope_kv_write_pair(const cover_rope_args* args0, const cover_rope_args* args1, void* stream);" in hdr
    p, i, f = C.c_void_p, C.c_int, C.c_float
    assert L.SYMBOLS["cover_rmsnorm_bf16_q8"] == (i, [p, i, i, p, f, i, p, i, i, i, f, p, i, p, p])
    assert L.SYMBOLS["cover_rmsnorm_bf16_q8"][1][:11] == L.SYMBOLS["cover_rmsnorm_bf16"][1][:11]
    assert L.SYMBOLS["cover_rope_kv_write_pair"] == (i, [C.POINTER(L.RopeArgs), C.POINTER(L.RopeArgs), p])
    assert L._STRUCTS["cover_rope_args"] is L.RopeArgs
    names = [n for n, _ in L.RopeArgs._fields_]
    assert names[-4:] == ["t_offset", "n_splits", "partial", "bias"]
    body = hdr[hdr.index("typedef struct cover_rope_args {"):hdr.index("} cover_rope_args;")]
    marks = {"qkv": "void* qkv;", "B": "int B,", "T": " T,", "Hq": " Hq,", "Hkv": " Hkv,", "D": " D;", "k_slot_stride": "k_slot_stride,",
             "k_t_stride": "k_t_stride,", "vt_slot_stride": "vt_slot_stride,", "vt_h_stride": "vt_h_stride,"}
    pos = [body.index(marks.get(n, n + ";")) for n in names]
    assert pos == sorted(pos)
    assert C.sizeof(L.RopeArgs) == 168
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_rmsnorm_bf16_q8") and hasattr(h, "cover_rope_kv_write_pair")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_rope_args") == C.sizeof(L.RopeArgs)


def test_new_wrappers_have_no_cpu_path():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    with pytest.raises(CoverError):
        ops.rmsnorm(torch.zeros(2, 128, dtype=BF), torch.ones(128), 1e-6, q8=True)
    with pytest.raises(CoverError):
        ops.rope_args(torch.zeros(2, 24, dtype=BF), 1, 2, 1, 1, 8, vt_cache=torch.zeros(64, dtype=BF))


# ------------------------------------------------------------------------------------------------ the rounding helpers
def test_round_bf16_from64_is_one_rounding():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8 - 2.0 ** -40, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -40),
                      0.0, 3.0], dtype=torch.float64)
    want = torch.tensor([1.0, 1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 0.0, 3.0])
    assert torch.equal(R.round_bf16_from64(x).float(), want)
    assert R.round_bf16_from64(x).float()[1] != x.float().to(BF).float()[1]       # the cast through fp32 rounds twice: to the tie, then to even
    g = torch.Generator().manual_seed(1)
    y = torch.randn(20000, generator=g, dtype=torch.float64) * 100
    assert torch.equal(R.round_bf16_from64(y), y.float().to(BF))                   # away from such ties the two agree


def test_neighbour_check_counts_and_rejects():
    ref = torch.tensor([1.0, 2.0, -3.0, 0.0], dtype=torch.float64)
    exact = ref.float().to(BF)
    assert R.neighbour_check(exact, ref) == (True, 0.0)
    up = exact.clone()
    up[1] = 2.0 + 2.0 ** -6                                                       # the next bf16 above 2
    assert R.neighbour_check(up, ref) == (True, 0.25)
    up[1] = 2.0 + 2.0 ** -5
    assert R.neighbour_check(up, ref)[0] is False
    down = exact.clone()
    down[3] = -0.0
    assert R.neighbour_check(down, ref) == (True, 0.0)                            # the two zeros are one value
    down[3] = -9.1835e-41                                                         # the smallest negative bf16: 0's lower neighbour
    assert R.neighbour_check(down, ref) == (True, 0.25)
    down[0] = float("nan")
    assert R.neighbour_check(down, ref)[0] is False


# ------------------------------------------------------------------------------------------------ float64 references against torch
@pytest.mark.parametrize("dim", R.NORM_DIMS)
def test_norm_references_against_torch_double(dim):
    x, w, b = R.norm_inputs(5, dim, "plain")
    xd = x.double()
    for bias in (b, None):
        want = torch.nn.functional.layer_norm(xd, (dim,), w.double(), None if bias is None else bias.double(), 1e-6)
        assert torch.allclose(R.layernorm_ref64(x, w, bias, 1e-6), want, atol=1e-12, rtol=1e-12)
    # RMSNorm is LayerNorm without the centring: on rows made zero-mean by appending their negation the two agree
    sym = torch.cat([xd, -xd], 1)
    want = torch.nn.functional.layer_norm(sym, (2 * dim,), torch.cat([w, w]).double() + 1.0, None, 1e-6)
    got = R.rmsnorm_ref64(sym, torch.cat([w, w]), 1e-6, 1.0, 0)
    assert torch.allclose(got, want, atol=1e-12, rtol=1e-12)
    rstd = torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-6)
    s1 = R.rmsnorm_ref64(x, w, 1e-6, 0.0, 1)
    assert torch.allclose(s1, w.double() * (xd * rstd), atol=0, rtol=2.0 ** -8)   # the inner rounding moves a value by at most half a bf16 ulp
    inner = s1[:, w != 0] / w.double()[w != 0]
    assert torch.allclose(inner.float().to(BF).double(), inner, atol=1e-30, rtol=1e-12)      # ... and is really there
    assert torch.allclose(R.rmsnorm_ref64(x, None, 1e-6, 1.0, 0), xd * rstd, atol=0, rtol=1e-12)      # w = NULL: zeros, so the factor is w_offset
    assert torch.equal(R.rmsnorm_ref64(x, None, 1e-6, 0.0, 1), torch.zeros_like(xd))


@pytest.mark.parametrize("patch,hw", R.PATCH_CASES)
def test_patchify_reference_against_unfold(patch, hw):
    img = R.patch_image("u8", hw)
    x = img.double().permute(0, 3, 1, 2)
    m, a = (torch.tensor(v, dtype=torch.float32).double().view(1, 3, 1, 1) for v in (R.PATCH_MUL, R.PATCH_ADD))
    gh, gw = hw[0] // patch, hw[1] // patch
    kk = 3 * patch * patch
    want = torch.nn.functional.unfold((x * m + a)[:, :, :gh * patch, :gw * patch], patch, stride=patch).transpose(1, 2).reshape(-1, kk)
    got = R.patchify_ref64(img, patch, R.PATCH_MUL, R.PATCH_ADD, kk + 24)
    assert got.shape == (3 * gh * gw, kk + 24) and torch.equal(got[:, :kk], want) and not got[:, kk:].any()
    f32 = R.patch_image("f32", hw)
    assert torch.equal(R.patchify_ref64(f32, patch, (1.0,) * 3, (0.0,) * 3, kk)[:, :kk],
                       torch.nn.functional.unfold(f32.double()[:, :, :gh * patch, :gw * patch], patch, stride=patch).transpose(1, 2).reshape(-1, kk))


# ------------------------------------------------------------------------------------------------ the acceptance rule is satisfiable in fp32
def _within_rule(got, ref64, what, hi64=None):
    ok, share = R.neighbour_check(got, ref64, hi64)
    print(f"{what}: share of elements not equal to bf16(ref64) = {share:.2e}")
    assert ok, what
    return share


@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("dim", R.NORM_DIMS)
def test_fp32_norms_meet_the_acceptance_rule(dim, kind):
    """rows = 37 (the cap is a share per case: a one-row case of 8 elements passes only without any unequal element, which is what fp32 gives)"""
    for rows in R.NORM_ROWS:
        x, w, b = R.norm_inputs(rows, dim, kind)
        xb = x.to(BF)
        for bias in (b, None):
            lo, hi = R.layernorm_bounds64(xb, w, bias, 1e-6)
            assert _within_rule(R.layernorm_f32(xb, w, bias, 1e-6), lo, f"layernorm {rows}x{dim}", hi) <= R.NEIGHBOUR_CAP
        for xin in (xb, x):
            for style, off, ww in ((0, 1.0, w), (1, 0.0, w), (0, 1.0, None)):
                got = R.rmsnorm_f32(xin, ww, 1e-6, off, style)
                lo, hi = R.rmsnorm_bounds64(xin, ww, 1e-6, off, style)
                assert _within_rule(got, lo, f"rmsnorm style {style} {rows}x{dim}", hi) <= R.NEIGHBOUR_CAP


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("patch,hw", R.PATCH_CASES)
def test_fp32_patchify_meets_the_acceptance_rule(patch, hw, kind):
    img = R.patch_image(kind, hw)
    ld = 3 * patch * patch + 8
    ref = R.patchify_ref64(img, patch, R.PATCH_MUL, R.PATCH_ADD, ld)
    for fma in (False, True):                                                     # the compiler may contract pix * mul + add or not
        assert _within_rule(R.patchify_f32(img, patch, R.PATCH_MUL, R.PATCH_ADD, ld, fma), ref, f"patchify fma={fma}") <= R.NEIGHBOUR_CAP


# ------------------------------------------------------------------------------------------------ exact references
def test_quantiser_reference_against_float8_cast():
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(6, 256, generator=g) * torch.logspace(-2, 1, 6)[:, None]).to(BF)
    y[1] = 0
    y[2] = y[2].clamp(-40, 40)
    y[2, 7] = 448.0 * 2 ** -3
    q, s = R.quantize_rows_e4m3_ref(y)
    assert s[1] == 1.0 and s[2] == 2.0 ** -3
    amax = y.float().abs().amax(1)
    live = amax > 0
    assert bool((amax[live] / s[live] <= 448).all()) and bool((amax[live] / s[live] > 224).all())     # the smallest such power of two
    assert bool((torch.log2(s) == torch.log2(s).round()).all())
    nat = torch.empty_like(q)
    nat[:, R.act_perm(256)] = q
    assert torch.equal(nat, (y.float() / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8))
    perm = R.act_perm(128)
    assert sorted(perm.tolist()) == list(range(128))
    assert perm[:24].tolist() == list(range(0, 8)) + list(range(32, 40)) + list(range(8, 16)) and perm[64] == 64
    for dim in R.Q8_DIMS:                                                         # the boundary row of the Q8 RMSNorm inputs lands where it says
        for style in (0, 1):
            x, w, off = R.q8_inputs(dim, style)
            yy = R.rmsnorm_f32(x, w, 1e-6, off, style)
            assert yy[2].float().abs().max() == 14.0 and yy[2, 3] == 14.0 and not yy[1].any()
            assert R.quantize_rows_e4m3_ref(yy)[1][2] == 2.0 ** -5


def test_small_references_at_tiny_shapes():
    table = torch.arange(12, dtype=torch.float32).view(4, 3).to(BF)
    ids = torch.tensor([3, 0, 3])
    assert torch.equal(R.embed_gather_ref(table, ids, 1.0).float(), torch.tensor([[9., 10, 11], [0, 1, 2], [9, 10, 11]]))
    assert torch.equal(R.embed_gather_ref(table, ids, 2.0).float(), torch.tensor([[18., 20, 22], [0, 2, 4], [18, 20, 22]]))
    dst = torch.full((3, 4), 7.0).to(BF)
    out = R.copy_rows_ref(table, dst, 2, 2, sidx=[2, 2], didx=[1, 0])
    assert torch.equal(out.float(), torch.tensor([[6., 7, 7, 7], [6, 7, 7, 7], [7, 7, 7, 7]]))
    x = torch.ones(5, 2).to(BF)
    assert torch.equal(R.add_rows_ref(x, torch.tensor([[1., 2], [3, 4]]).to(BF)).float(), torch.tensor([[2., 3], [4, 5], [2, 3], [4, 5], [2, 3]]))
    v = torch.tensor([[257.0]]).to(BF)                                            # bf16(257) = 256; 256 / 8 * 8
    assert R.scale_ref(v, 8.0, 8.0).float().item() == 256.0
    third = torch.tensor([[1 / 3]]).to(BF)
    assert R.scale_ref(third, 1.0, 3.0).float().item() == (third.float() * 3).to(BF).float().item()
    sp = R.special_f32_row()
    b = R.cast_f32_to_bf16_ref(sp)
    bits = (R.bf_bits(b).to(torch.int32) & 0xFFFF).tolist()
    assert bits[:4] == [0x0000, 0x8000, 0x7F80, 0xFF80] and b[4].isnan()
    assert bits[9:15] == [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80]        # ties to even, just above / below a tie
    assert bits[15:18] == [0x7F80, 0xFF80, 0x7F80] and bits[19] == 0x7F7F         # the largest finite fp32 is past bf16's: it rounds to inf
    assert bits[5:9] == [0x0000, 0x8080, 0x0000, 0x0002]                          # subnormals round like every other value
    back = R.cast_bf16_to_f32_ref(b)
    assert torch.equal(back[~back.isnan()], b.float()[~b.float().isnan()])


ROPE_TINY = [R.rope_case(3, 8, 1, heads=(2, 1), B=2, pos="clamp", cache_pad=True, ld_pad=3, qkv_off=4, k_offset=5, vt_offset=3),
             R.rope_case(3, 8, 2, heads=(1, 1), B=2, pos="none", slot=False, toff=False, cs_off=1),
             R.rope_case(2, 4, 0, heads=(2, 2), B=1, kcache=False),
             R.rope_case(2, 4, 1, heads=(2, 2), B=2, kcache=False, k_odd=True),
             R.rope_case(2, 8, 2, heads=(2, 1), B=2, pos="clamp", S=3, bias=True),
             R.rope_case(2, 8, 0, heads=(2, 1), B=2, S=3, bias=False),
             R.rope_case(2, 8, 0, heads=(2, 1), B=2, S=1, bias=True, kcache=False)]


@pytest.mark.parametrize("cs", ROPE_TINY, ids=[c["id"] for c in ROPE_TINY])
def test_placement_reference_against_a_naive_loop(cs):
    t = R.rope_build(cs)
    fast, slow = R.rope_expected(cs, t), R.rope_expected_naive(cs, t)
    for a, b, start in zip(fast, slow, (t["qkv"], t["k"], t["vt"])):
        assert (a is None) == (b is None) == (start is None)
        if a is not None:
            assert R.same_bits(a, b)
            assert not R.same_bits(a, start) or (start is t["qkv"] and cs["mode"] == 0 and cs["S"] == 0)     # something was placed
    q, k, v = R.rope_values(cs, t)
    after = dict(t, qkv=fast[0], k=fast[1], vt=fast[2])
    ql, kl, vl = R.rope_logical(cs, after)
    if cs["mode"] != 0 or cs["S"] > 0:
        assert R.same_bits(ql, q.reshape(ql.shape)) and R.same_bits(kl, k)
    assert R.same_bits(vl, v)
    n_written = sum(int((R.bf_bits(a) != R.bf_bits(s)).sum()) for a, s in zip(fast, (t["qkv"], t["k"], t["vt"])) if a is not None)
    assert n_written <= q.numel() + k.numel() + v.numel()


def test_fold_reference_is_sequential_and_order_matters():
    p = torch.tensor([1.0, 2.0 ** -25, 2.0 ** -25]).view(3, 1, 1)
    assert R.fold_ref(p, None).item() == 1.0
    assert R.fold_ref(p.flip(0), None).item() == 1.0                              # (bf16 hides the last fp32 bit here ...)
    cs = R.rope_folds()[-1]
    t = R.rope_build(cs)
    assert cs["S"] == 3 and t["bias"] is not None
    fwd, rev = R.fold_ref(t["partial"], t["bias"]), R.fold_ref(t["partial"].flip(0), t["bias"])
    assert 0.05 < float((fwd != rev).float().mean())                              # ... the test partials do not let it
    assert 0.3 < float((fwd != R.fold_ref(t["partial"], None)).float().mean())   # and a dropped bias shows
    v = t["partial"][0] + t["partial"][1] + t["partial"][2] + t["bias"]
    assert torch.equal(fwd, v.to(BF).float())


def test_case_tables_reach_every_path_and_cell():
    cases = R.rope_sweep() + R.rope_named()
    paths = {R.rope_path(c) for c in cases}
    assert paths == {"scalar", "vtok_scalarqk", "vtok_vecqk", "vtok_noqk"}
    assert all(c["id"].startswith(R.rope_path(c)) for c in cases)
    assert len({c["id"] for c in cases}) == len(cases)
    seen = {(c["T"], c["D"], c["mode"]) for c in cases}
    assert all((T, D, m) in seen for T in R.ROPE_T for D in R.ROPE_D for m in (0, 1, 2))
    assert {(c["Hq"], c["Hkv"], c["B"]) for c in cases} >= {(h[0], h[1], B) for h in R.ROPE_HEADS for B in (1, 3)}
    for c in cases:                                                               # what each D is in the table for
        if c["T"] >= 16 and c["ld_pad"] % 8 == 0:
            want = {36: "scalar", 72: "vtok_noqk" if (c["mode"] == 0 and not c["kcache"]) else "vtok_scalarqk"}.get(c["D"])
            assert want is None or R.rope_path(c) == want
        if c["T"] < 16:
            assert R.rope_path(c) == "scalar"
    by_tag = {c["id"].rsplit("-", 1)[-1]: c for c in R.rope_named()}
    for tag, per_wave in (("ragged68of16", 16), ("ragged68of8", 8), ("ragged102of4", 4)):
        c = by_tag[tag]
        assert R.rope_path(c) == "vtok_vecqk" and 64 // (c["D"] // 16) == per_wave and (c["B"] * c["T"] * (c["Hq"] + c["Hkv"])) % per_wave != 0
    for aligned, others in R.rope_fallbacks():
        assert R.rope_path(aligned) == "vtok_vecqk"
        assert [R.rope_path(c) for c in others] == ["scalar", "scalar", "vtok_scalarqk", "vtok_scalarqk"]
    assert all(R.rope_path(c) == "scalar" for c in R.rope_folds()) and len(R.rope_folds()) == 18
    assert sorted({c["S"] for c in R.rope_folds()}) == [1, 3, 6]                  # one slab, the product's three, more than four
    for name, c0, c1 in R.rope_pairs():
        w = [R.rope_waves(c0), R.rope_waves(c1)]
        assert sorted(w) in ([14, 25], [0, 14], [0, 25]) and all(x % 4 for x in w if x)
