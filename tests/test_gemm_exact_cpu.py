"""The exact-GEMM references on their own (no GPU): the float64 reference equals an int64 matmul, an fp32 accumulation of the table's operands
gives the same bits in any k order and across any K split (the order-independence the GPU tests rest on, at the table's largest K), every
case plans onto its pinned slot / K split / completion, and the table reaches every bf16 slot and completion that test_gemm_plan_cpu's
literal tables reach."""
import pytest
import torch

from cover_vla_amd import _lib
from tests import gemm_exact_ref as R
from tests import test_gemm_plan_cpu as P

ALL_CASES = R.CASES + R.INEXACT_CASES + R.position_cases()


def test_case_names_are_unique_and_operands_are_bf16_exact():
    names = [c.name for c in ALL_CASES]
    assert len(set(names)) == len(names)
    small = lambda cs: [c for c in cs if c.M * c.N * c.K <= 200e6]   # noqa: E731  (building operands is cheap; no matmul here)
    seen = set()
    for cases, mode in ((small(R.CASES), "int"), (small(R.INEXACT_CASES), "scaled"), (small(R.position_cases()), "pos")):
        for c in cases:
            d = R.build_inputs(c, mode)
            for k in ("a", "w", "bias", "res", "ls"):
                if k in d:
                    assert bool((d[k].bfloat16().float() == d[k]).all()), (c.name, k)
                    seen.add((mode, k))
            seen.update((mode, m) for m in c.mods)
            seen.update((mode, part) for part in R.parts(c))
    # every branch of the builder went through the check
    assert {("int", k) for k in ("a", "w", "bias", "res", "ls", "res_f32", "inplace", "glu", "res_norm", "res_ln")} <= seen
    assert {("scaled", k) for k in ("a", "w", "bias", "glu", "glu_gelu")} <= seen and ("pos", "w") in seen


@pytest.mark.parametrize("c", [c for c in R.CASES if c.M * c.N * c.K <= 50e6], ids=lambda c: c.name)
def test_float64_reference_equals_int64_matmul(c):
    d = R.build_inputs(c, "int")
    acc = R.accumulators(d)
    a_i, w_i = d["a"].to(torch.int64), (d["w"] * 4).to(torch.int64)      # W = integers / 4
    assert bool(((a_i @ w_i.T).to(torch.float64) / 4 == acc).all())
    assert float(acc.abs().max()) * 4 <= 16 * c.K


def test_fp32_accumulation_is_order_independent_at_the_largest_k():
    K = max(c.K for c in ALL_CASES)
    c = R.Case("order", 24, 40, K, "plain", (), 1, "sized", False, None)
    for mode in ("int", "scaled"):
        d = R.build_inputs(c, mode)
        want = R.f32_exact(R.accumulators(d))
        a, w = d["a"], d["w"]
        prod = a[:, None, :] * w[None, :, :]                      # fp32 products [M, N, K]: exact (|a w| <= 16 times a power of two)
        g = torch.Generator().manual_seed(7)
        for _ in range(3):                                         # three shuffled k orders, summed strictly one element at a time
            perm = torch.randperm(K, generator=g)
            s = torch.zeros(c.M, c.N)
            for k in perm.tolist():
                s = s + prod[:, :, k]
            assert torch.equal(s, want)
        for S in (2, 3, 5):                                        # K slices of whole 64-deep k-tiles, slabs summed in slab order
            per = (K // 64 + S - 1) // S * 64
            s = torch.zeros(c.M, c.N)
            for lo in range(0, K, per):
                s = s + (a[:, lo:lo + per] @ w[:, lo:lo + per].T)
            assert torch.equal(s, want)
    # the bound behind it: |partial sum| <= 16 K units of the weight's power of two, below 2^24 for every K of the table
    assert 16 * K < 2 ** 24


def _ws_bytes(c):
    return _lib.lib().cover_gemm_workspace_bytes(c.M, c.N, c.K) if c.ws == "sized" else 4


def test_every_case_plans_onto_its_pinned_slot(monkeypatch):
    monkeypatch.delenv("COVER_FP8_MFMA", raising=False)
    bad = []
    for c in ALL_CASES:
        p = P.plan(c.M, c.N, c.K, c.kind, c.variant, _ws_bytes(c), ldc=R.ldc_of(c))
        got = None if p is None else (p[0], p[3], p[4], p[5])
        if got != c.plan:
            bad.append(f"{c.name} (M={c.M} N={c.N} K={c.K} {c.kind} v{c.variant} ws={c.ws}): {got} != {c.plan}")
    assert not bad, "\n".join(bad)


def test_split_k_cases_include_a_slice_count_that_does_not_divide_the_k_tiles():
    ragged = [c.name for c in R.CASES if c.plan[0] not in (19, 20, 22) and c.plan[1] > 1 and (R.kp(c.K) // 64) % c.plan[1]]
    assert ragged, "no tiled split-K case with a ragged last slice"


def test_table_reaches_every_bf16_slot_and_completion_of_the_plan_tables():
    """every (slot, completion) a bf16 row of test_gemm_plan_cpu's literal tables reaches (model GEMMs, GPU-test shapes, sweep) is reached by an
    exact case; slot 21 = fp8 operands, out of scope (picks 3..8 and slot 27 are knob-only and appear in no table)"""
    want = set()
    for plans in (P.MODEL_PLANS, P.GPU_TEST_PLANS, P.SWEEP_PLANS):
        for _, p in plans:
            if p is not None and p[0] not in (21, -1):
                want.add((p[0], p[4]))
    have = {(c.plan[0], c.plan[2]) for c in R.CASES}
    assert want - have == set(), sorted(want - have)
    assert {s for s, _ in want} - {c.plan[0] for c in R.position_cases()} == set()
