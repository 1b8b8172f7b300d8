"""cover_gemm_bf16 against order-independent exact references (tests/gemm_exact_ref.py): every bf16 plan slot and split-K completion, bit for
bit on the exact epilogues, position-coded operands that name the weight element each output read, and per-element bounds on the inexact
epilogues and the fused norms. Every case asserts the plan counter of its pinned slot, runs on a NaN-filled workspace and output (the header
promises nothing about the workspace's initial contents, so nothing may be read before it is written), checks the cells around a strided
output, and runs twice on the same workspace with identical bits."""
import pytest
import torch

from cover_vla_amd import ops
from tests import gemm_exact_ref as R

pytestmark = pytest.mark.gpu

REL = 2.0 ** -8                    # derived: the most ONE bf16 round-to-nearest moves a value, relative (half an ulp at the bottom of a binade)
REL2 = 2 * 2.0 ** -8 + 2.0 ** -16  # derived: two roundings in a row, (1 + 2^-8)^2 - 1
# Bounds, with `a` the absolute error of the kernel's activation arithmetic (the fast v_exp_f32 / v_rcp_f32 forms of SiLU and tanh-GELU, erff):
#   activation:  |out - ref| <= REL |ref| + a                   out = bf16(act(x)), one rounding
#   GLU:         |out - ref| <= REL2 |ref| + a |bf16(up)|       out = bf16(bf16(act(g)) * bf16(up)): two roundings, both stated in epi_store4_glu;
#                                                               an error of act(g) reaches the output multiplied by the up operand
# `a` was measured on the MI355X as the largest excess over the relative term (per unit of |bf16(up)| for GLU) over every inexact case of the
# table (pre-activations of standard deviation ~2, |x| up to ~10); constant = 2 x the measured maximum, rounded up to one significant digit
# (margin for the hardware exp / rcp on other inputs, not for the code under test).          measured maximum -> constant
A_ABS = {
    "gelu_tanh": 6e-7,        # 2.816e-07 -> 6e-7
    "gelu_erf": 2e-7,         # 7.657e-08 -> 2e-7
    "silu": 0.0,              # 0 (no element beyond the relative term) -> 0
    "glu_silu": 0.0,          # 0 -> 0   (per unit of |bf16(up)|)
    "glu_gelu_tanh": 6e-7,     # 2.805e-07 -> 6e-7   (per unit of |bf16(up)|)
}
# norm_out against the float64 norm of the stored bf16 rows, `a` per unit of the weight the kernel multiplies by (|norm_w|, |1 + norm_w| for Gemma):
#   Gemma RMSNorm (style 0), LayerNorm:  REL |ref| + a |w|      one rounding
#   Llama RMSNorm (style 1):             2 REL |ref| + a |w|    norm_out = bf16(w * bf16(x * rstd)): two roundings, as cover_rmsnorm_bf16 states
A_NORM = {
    "rms0": 0.0,    # 0 -> 0
    "rms1": 0.0,    # 0 -> 0
    "ln": 0.0,      # 0 (-2.3e-08) -> 0
}


def _report_excess(name, key, err, rel_term, unit):
    """re-measuring aid (pytest -s): the largest excess over the relative term per unit of `unit`, the quantity the constants above come from"""
    ok = unit > 0
    ex = float(((err - rel_term)[ok] / unit[ok]).max()) if bool(ok.any()) else 0.0
    print(f"{name}: largest excess over the relative term for {key}: {ex:.3e}")


def _run(c, d, dev):
    """one case on the device, twice on the same workspace: returns (out view [M, n_out] on the CPU, norm_out or None)"""
    M, K, kp, no = c.M, c.K, R.kp(c.K), R.n_out(c)
    p = R.parts(c)
    lda = kp + 128 if c.wide else kp
    a = torch.full((M, lda), float("nan"), dtype=torch.bfloat16, device=dev)
    a[:, :kp] = 0
    a[:, :K] = d["a"].to(dev).bfloat16()
    lin = ops.pack_linear(d["w"].to(dev), d["bias"].to(dev) if "bias" in d else None, glu="glu" in c.kind)
    out_dtype = torch.float32 if "f32" in p else torch.bfloat16
    n_ws = ops.L.lib().cover_gemm_workspace_bytes(M, c.N, K) if c.ws == "sized" else 4
    ws = torch.full((n_ws // 4,), float("nan"), dtype=torch.float32, device=dev) if n_ws else None
    kw = dict(act=R.act_of(c), variant=c.variant, out_scale=d["oscale"])
    if "ls" in d:
        kw["layer_scale"] = d["ls"].to(dev)
    h = None
    if "nw" in d:
        ln = "res_ln" in p
        kw.update(norm_w=d["nw"].to(dev), norm_style=2 if ln else 0 if "style0" in c.mods else 1, norm_w_offset=1.0 if "style0" in c.mods else 0.0,
                  norm_eps=1e-6, norm_b=d["nb"].to(dev) if ln else None)
    runs = []
    for rep in range(2):
        buf = torch.full((M, R.ldc_of(c)), R.SENTINEL, dtype=out_dtype, device=dev)
        out = buf[:, 8:8 + no] if c.wide else buf
        out.fill_(float("nan"))
        res = None
        if "res" in d:
            if "inplace" in c.mods:
                out.copy_(d["res"].to(dev))
                res = out
            else:
                res = d["res"].to(dev).to(torch.float32 if "res_f32" in c.mods else torch.bfloat16)
        if "nw" in d:
            h = torch.full((M, no), float("nan"), dtype=torch.bfloat16, device=dev)
            kw["norm_out"] = h
        ops.gemm_plan_counts(reset=True)
        ops.gemm(a[:, :kp], lin, residual=res, out=out, ws=ws, **kw)
        counts = ops.gemm_plan_counts()
        assert sum(counts) == 1 and counts[c.plan[0]] == 1, (c.name, [i for i, v in enumerate(counts) if v])
        torch.cuda.synchronize()
        if c.wide:
            assert bool((buf[:, :8] == R.SENTINEL).all()) and bool((buf[:, 8 + no:] == R.SENTINEL).all()), f"{c.name}: cells outside the output slice were written"
        runs.append((out.cpu().clone(), None if h is None else h.cpu().clone()))
    (o0, h0), (o1, h1) = runs
    assert not bool(torch.isnan(o0).any()), f"{c.name}: output cells left unwritten (or NaN read from unwritten workspace / beyond the padded K)"
    assert torch.equal(o0, o1), f"{c.name}: the second run on the same workspace differs from the first"
    if h0 is not None:
        assert not bool(torch.isnan(h0).any()) and torch.equal(h0, h1), f"{c.name}: norm_out unwritten or not reproducible"
    return o0, h0


def _stored(c, value64):
    """what the kernel stores of the exact value: fp32 as is (representable, asserted), bf16 rounded ONCE, RNE"""
    f = R.f32_exact(value64)
    return f if "f32" in R.parts(c) else f.bfloat16()


def _check_norm(c, d, x, h):
    ref = R.norm_reference(c, d, x)
    key = "ln" if "res_ln" in c.kind else "rms0" if "style0" in c.mods else "rms1"
    nw = d["nw"].to(torch.float64)
    unit = ((1.0 + nw) if key == "rms0" else nw).abs().expand_as(ref)
    rel_term = (2 * REL if key == "rms1" else REL) * ref.abs()
    _report_excess(c.name, key, (h.to(torch.float64) - ref).abs(), rel_term, unit)
    msg = R.first_violation(h, ref, rel_term + A_NORM[key] * unit, f"{c.name} norm_out ({key})")
    assert msg is None, msg


@pytest.mark.parametrize("c", [c for c in R.CASES], ids=lambda c: c.name)
def test_gemm_exact(dev, c):
    d = R.build_inputs(c, "int")
    value = R.reference(c, d)
    want = _stored(c, value)
    out, h = _run(c, d, dev)
    msg = R.first_mismatch(out, want, f"{c.name} (slot {c.plan[0]}, {c.plan[1]} K slices, completion {c.plan[2]})",
                           lambda m, n: f"exact value {float(value[m, n])!r}")
    assert msg is None, msg


@pytest.mark.parametrize("c", R.NORM_CASES, ids=lambda c: c.name)
def test_gemm_fused_norm(dev, c):
    """norm_out (folded into the split-K reduction, or the norm launch behind an unsplit GEMM) against the float64 norm of the kernel's own
    stored residual-stream rows, which test_gemm_exact pins bit for bit"""
    d = R.build_inputs(c, "int")
    out, h = _run(c, d, dev)
    _check_norm(c, d, out, h)


@pytest.mark.parametrize("c", R.position_cases(), ids=lambda c: c.name)
def test_gemm_position_coded(dev, c):
    d = R.build_inputs(c, "pos")
    km = d["k_of_row"]
    want = d["w"][:, km].T.contiguous().bfloat16()      # out[m, n] = W[n, (7 m + 3) mod K]: the code of the one element row m reads
    out, _ = _run(c, d, dev)

    def decode(m, n):
        code = float(out[m, n])
        ks = torch.nonzero(d["w"][n] == code).flatten()[:6].tolist()
        return f"row m reads k = {int(km[m])}; the received code {code!r} is W[{n}, k] at k = {ks} (if any: a sum of codes or another column otherwise)"
    msg = R.first_mismatch(out, want, f"{c.name} (slot {c.plan[0]})", decode)
    assert msg is None, msg


@pytest.mark.parametrize("c", R.INEXACT_CASES, ids=lambda c: c.name)
def test_gemm_inexact_epilogue(dev, c):
    d = R.build_inputs(c, "scaled")
    ref, up = R.reference_inexact(c, d)
    out, _ = _run(c, d, dev)
    key = ("glu_" if up is not None else "") + R.act_of(c)
    unit = torch.ones_like(ref) if up is None else up.abs()
    rel_term = (REL if up is None else REL2) * ref.abs()
    _report_excess(c.name, key, (out.to(torch.float64) - ref).abs(), rel_term, unit)
    msg = R.first_violation(out, ref, rel_term + A_ABS[key] * unit, f"{c.name} ({key})")
    assert msg is None, msg
