"""Per-member verifier scores, the part that needs no GPU: the fp32 reference of tests/member_scores_ref.py against float64, the
identities of kappa = 0 and M = 1, the constructed case in which disagreement flips the decision, the struct mirror against the
header, the argument checks of ops.member_scores and host.verify_and_select's forwarding of the two keywords."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import member_scores_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_NEG_ZERO = np.float32(-0.0)


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_reference_is_within_the_fp32_bound_of_float64(case):
    """A member score is a sum of dim products in which every term passes through one product rounding, at most ceil(dim / 64) adds of
    its lane's chain (the first, onto 0.0f, is exact) and the 6 adds of the butterfly: k = ceil(dim / 64) + 7 roundings, so
    |s - s64| <= gamma_k * sum |it * act| =: e_m.
    mean: the M-add chain and the division are M + 1 more roundings of values bounded by sum |s_m|, and the members' own errors pass
    through averaged: |mean - mean64| <= (1 + gamma_{M+1}) * mean(e_m) + gamma_{M+1} * mean |s64_m| =: e_mean.
    spread = ||dv||_2 / sqrt(M) with dv_m = s_m - mean. Each computed dv_m is off by at most d_m = (e_m + e_mean) * (1 + u) + u |dv64_m|,
    and a 2-norm moves by at most the 2-norm of the perturbation; the squares, the M-add chain, the division and the square root
    (which halves a relative error) add a relative gamma_{M+3} at most:
    |spread - spread64| <= ||d||_2 / sqrt(M) + gamma_{M+3} * (spread64 + ||d||_2 / sqrt(M))."""
    M, N, gs, dim = case
    it, act = MR.case_inputs(case)
    r = MR.reference(it, act, MR.fused_scores_f64(it, act), gs, 0.5, "lcb")
    prod = it.astype(np.float64)[:, None, :] * act.astype(np.float64)
    s64, mag = prod.sum(axis=-1), np.abs(prod).sum(axis=-1)
    k = math.ceil(dim / 64) + 7
    e = MR.gamma(k) * mag
    err = np.abs(r["member_scores"].astype(np.float64) - s64)
    print(f"{MR.case_id(case)}: member score error {err.max():.3e}, smallest slack {(e - err).min():.3e}")
    assert (err <= e).all()
    g1 = MR.gamma(M + 1)
    mean64 = s64.mean(axis=0)
    e_mean = (1.0 + g1) * e.mean(axis=0) + g1 * np.abs(s64).mean(axis=0)
    assert (np.abs(r["mean"].astype(np.float64) - mean64) <= e_mean).all()
    dv64 = s64 - mean64
    d = (e + e_mean) * (1.0 + MR.U) + MR.U * np.abs(dv64)
    dn = np.sqrt((d * d).sum(axis=0) / M)
    spread64 = np.sqrt((dv64 * dv64).sum(axis=0) / M)
    e_spread = dn + MR.gamma(M + 3) * (spread64 + dn)
    assert (np.abs(r["spread"].astype(np.float64) - spread64) <= e_spread).all()
    assert np.array_equal(r["min"], r["member_scores"].min(axis=0)) and np.array_equal(r["min_member"], r["member_scores"].argmin(axis=0))
    if M > 1 and dim >= 64:
        assert (r["spread"] > 0).all() and len(np.unique(r["min_member"])) > 1        # the members do disagree on these inputs


@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_kappa_zero_keeps_the_bits_of_scores(case):
    M, N, gs, dim = case
    it, act = MR.case_inputs(case)
    scores = MR.fused_scores_f64(it, act).copy()
    scores[N // 2] = F32_NEG_ZERO
    r = MR.reference(it, act, scores, gs, 0.0, "lcb")
    assert np.array_equal(_bits(r["robust"]), _bits(scores)) and _bits(r["robust"])[N // 2] == np.int32(-2 ** 31)
    res, best = MR.group_argmax(scores, gs)
    assert np.array_equal(r["result"], res) and np.array_equal(_bits(r["best"]), _bits(best))
    moved = MR.reference(it, act, scores, gs, 0.5, "lcb")["robust"]
    assert M == 1 or dim < 64 or not np.array_equal(_bits(moved), _bits(scores))       # ... and a penalty is not a no-op


def test_one_member_has_no_spread():
    case = (1, 16, 1, 512)
    it, act = MR.case_inputs(case)
    scores = MR.fused_scores_f64(it, act)
    for kappa in MR.KAPPAS:
        r = MR.reference(it, act, scores, 1, kappa, "lcb")
        assert np.array_equal(_bits(r["spread"]), np.zeros(16, dtype=np.int32))        # exactly +0.0
        assert np.array_equal(_bits(r["robust"]), _bits(scores)), kappa
        assert np.array_equal(_bits(r["mean"]), _bits(r["member_scores"][0])) and not r["min_member"].any()
    r = MR.reference(it, act, scores, 1, 0.0, "min")
    assert np.array_equal(_bits(r["robust"]), _bits(r["member_scores"][0]))


def test_constructed_flip():
    """One member loves candidate A and the others do not: the fused score prefers A, the penalised score and the worst member B."""
    it, act = MR.flip_inputs()
    scores = MR.fused_scores_f64(it, act)
    assert abs(scores[0] - 0.90370) < 1e-5 and abs(scores[1] - 0.89113) < 1e-5
    r0 = MR.reference(it, act, scores, 2, 0.0, "lcb")
    assert abs(r0["spread"][0] - 0.42426) < 1e-5 and r0["spread"][1] == 0.0 and abs(r0["min"][0] - 0.1) < 1e-6
    assert r0["min_member"].tolist() == [2, 0]
    assert r0["result"].tolist() == [0, 0, 0, 0]
    r1 = MR.reference(it, act, scores, 2, 0.1, "lcb")
    assert abs(r1["robust"][0] - 0.86127) < 1e-5 and abs(r1["robust"][1] - 0.89113) < 1e-5
    assert r1["result"].tolist() == [1, 0, 1, 0]
    rm = MR.reference(it, act, scores, 2, 0.0, "min")
    assert rm["result"].tolist() == [1, 0, 1, 0] and abs(rm["best"][0] - 0.75) < 1e-6
    assert r0["member_result"][:, 0].tolist() == [0, 0, 1]                             # members 0 and 1 pick A, member 2 picks B
    for a, b in ((r0["robust"][0], r0["robust"][1]), (r1["robust"][1], r1["robust"][0]), (rm["robust"][1], rm["robust"][0])):
        assert a - b >= 0.01                                                           # four orders above fp32 rounding


def test_ties_go_to_the_first():
    case, it, act = MR.tie_inputs()
    scores = MR.fused_scores_f64(it, act)
    for mode, kappa in MR.RUNS[:2] + MR.RUNS[3:]:
        r = MR.reference(it, act, scores, case[2], kappa, mode)
        assert r["robust"][0] == r["robust"][1] and np.array_equal(r["robust"][0:4], r["robust"][4:8])
        assert r["result"].tolist() == [0, 0, 0, 0] and r["member_result"].tolist() == [[0, 0, 0, 0]] * 3
    same = np.repeat(act[:1], 3, axis=0)                                               # every member holds member 0's rows
    r = MR.reference(np.repeat(it[:1], 3, axis=0), same, scores, case[2], 0.0, "min")
    assert not r["min_member"].any() and np.array_equal(_bits(r["min"]), _bits(r["member_scores"][0]))


# ------------------------------------------------------------------------------------------------ binding
def test_struct_mirror_and_symbol():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_member_scores_args"] is L.MemberScoresArgs
    assert L.SYMBOLS["cover_member_scores"] == (C.c_int, [C.POINTER(L.MemberScoresArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    body = hdr[hdr.index("typedef struct cover_member_scores_args {") + len("typedef struct cover_member_scores_args {"):
               hdr.index("} cover_member_scores_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", d)[-1] for stmt in body.split(";") if stmt.strip() for d in stmt.split(",")]
    assert declared == [f[0] for f in L.MemberScoresArgs._fields_]
    assert "int cover_member_scores(const cover_member_scores_args* args, void* stream);" in hdr
    assert C.sizeof(L.MemberScoresArgs) == 13 * 8 + 6 * 4                              # no padding: pointers, then 4 ints, float, int
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_member_scores")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_member_scores_args") == C.sizeof(L.MemberScoresArgs)


def test_argument_validation_needs_no_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    it, act, s = torch.zeros(3, 8), torch.zeros(3, 6, 8), torch.zeros(6)
    bad = [
        (it.double(), act, s, 2, {}), (it, act.double(), s, 2, {}), (it, act, s.double(), 2, {}), (it.numpy(), act, s, 2, {}),   # dtype / kind
        (it[0], act, s, 2, {}), (it, act[0], s, 2, {}), (it, act, s.view(2, 3), 2, {}),                                            # rank
        (torch.zeros(2, 8), act, s, 2, {}), (torch.zeros(3, 7), act, s, 2, {}), (it, act, torch.zeros(5), 2, {}),                  # shapes
        (torch.zeros(3, 16)[:, ::2], act, s, 2, {}), (it, torch.zeros(3, 6, 16)[:, :, ::2], s, 2, {}), (it, act, torch.zeros(12)[::2], 2, {}),
        (torch.zeros(17, 8), torch.zeros(17, 6, 8), s, 2, {}), (torch.zeros(0, 8), torch.zeros(0, 6, 8), s, 2, {}),               # M
        (torch.zeros(3, 8), torch.zeros(3, 0, 8), torch.zeros(0), 1, {}),                                                          # N
        (torch.zeros(3, 4097), torch.zeros(3, 6, 4097), s, 2, {}), (torch.zeros(3, 0), torch.zeros(3, 6, 0), s, 2, {}),            # dim
        (it, act, s, 4, {}), (it, act, s, 0, {}), (it, act, s, -2, {}), (it, torch.zeros(3, 8192, 8), torch.zeros(8192), 1, {}),   # groups
        (it, act, s, 2, dict(kappa=-0.1)), (it, act, s, 2, dict(kappa=float("nan"))), (it, act, s, 2, dict(kappa=float("inf"))),
        (it, act, s, 2, dict(kappa=1e39)),
        (it, act, s, 2, dict(mode="max")), (it, act, s, 2, dict(mode=0)), (it, act, s, 2, dict(mode="min", kappa=0.5)),
    ]
    for a, b, c, gs, kw in bad:
        with pytest.raises(CoverError):
            ops.member_scores(a, b, c, gs, **kw)
    for kw in (dict(), dict(kappa=0.5), dict(mode="min")):                             # valid arguments, host tensors: no CPU path
        with pytest.raises(CoverError, match="device"):
            ops.member_scores(it, act, s, 2, **kw)


def test_signatures_default_to_off():
    from cover_vla_amd import host, ops
    from cover_vla_amd.verifier import EfficientEnsembleMerged as E
    p = inspect.signature(ops.member_scores).parameters
    assert list(p) == ["it", "act", "scores", "group_size", "kappa", "mode"] and p["kappa"].default == 0.0 and p["mode"].default == "lcb"
    for fn in (E.score_histories, E.score_features, E.compute_max_similarity_scores_batch, host.verify_and_select):
        p = inspect.signature(fn).parameters
        assert p["member_kappa"].default is None and p["member_mode"].default == "lcb"


# ------------------------------------------------------------------------------------------------ host.verify_and_select
class _StubVerifier:
    """Scripted scores; records the keywords it receives and keeps a scripted last_member_stats when it is given member_kappa."""

    def __init__(self, stage1, scores, member_scores):
        self.stage1, self.scores, self.ms, self.calls = stage1, np.asarray(scores, dtype=np.float32), np.asarray(member_scores, dtype=np.float32), []
        self.last_member_stats = None

    def compute_max_similarity_scores_batch(self, images, instructions, all_action_histories, cfg_repeat_language_instructions=1, **kw):
        n, g = len(all_action_histories), cfg_repeat_language_instructions
        self.calls.append((n, g, dict(kw)))
        if "member_kappa" not in kw:
            if n == 1:
                return self.stage1, instructions[0], all_action_histories[0], torch.tensor(0)
            gi = int(MR.group_argmax(self.scores, g)[0][0])
            return float(self.scores[gi]), instructions[0], all_action_histories[gi], torch.tensor(gi)
        ms = self.ms[:, :n]
        mean = ms.mean(axis=0)
        spread = np.sqrt(((ms - mean) ** 2).mean(axis=0)).astype(np.float32)
        base = np.array([self.stage1], dtype=np.float32) if n == 1 else self.scores
        robust = ms.min(axis=0) if kw["member_mode"] == "min" else (base - np.float32(kw["member_kappa"]) * spread).astype(np.float32)
        res, best = MR.group_argmax(robust, g)
        self.last_member_stats = dict(spread=torch.from_numpy(spread), robust=robust,
                                      member_result=np.stack([MR.group_argmax(ms[m], g)[0] for m in range(len(ms))]))
        return float(best[0]), instructions[0], all_action_histories[int(res[0])], torch.tensor(int(res[0]))


class _OldVerifier:
    """A verifier that does not know the keywords."""

    def __init__(self):
        self.calls = 0

    def compute_max_similarity_scores_batch(self, images, instructions, all_action_histories, cfg_repeat_language_instructions=1):
        self.calls += 1
        return 0.05, instructions[0], all_action_histories[0], torch.tensor(0)


def test_verify_and_select_forwards_the_keywords_to_both_stages():
    from cover_vla_amd import host
    rng = np.random.default_rng(1)
    B, S = 6, 3
    q = [rng.uniform(-1, 1, size=(B, 7)).astype(np.float32) for _ in range(4)]
    tasks = ["a"] * 3 + ["b"] * 3
    hist = [rng.normal(size=7) for _ in range(3)]
    scores = [0.1, 0.1, 0.1, 0.2, 0.9, 0.3]
    ms = [[0.1, 0.1, 0.1, 0.2, 1.0, 0.3],            # member 0 loves candidate 4, the others do not: they pick 5
          [0.1, 0.1, 0.1, 0.2, 0.0, 0.3],
          [0.1, 0.1, 0.1, 0.2, 0.0, 0.3]]
    args = (None, "a", tasks, q, hist, S)
    # the default call: neither stage receives the keywords, the record says so, no member figures
    fv = _StubVerifier(0.05, scores, ms)
    r0 = host.verify_and_select(fv, *args, process_image=False)
    assert fv.calls == [(1, 1, {}), (B, S, {})] and r0["global_action_idx"] == 4
    assert r0["member_kappa"] is None and "spread" not in r0 and "member_agreement" not in r0
    fv = _StubVerifier(0.05, scores, ms)
    host.verify_and_select(fv, *args, process_image=False, member_mode="min")           # a mode without a kappa: still off
    assert [c[2] for c in fv.calls] == [{}, {}]
    # with a value both stages receive both keywords
    fv = _StubVerifier(0.05, scores, ms)
    r = host.verify_and_select(fv, *args, process_image=False, member_kappa=0.5)
    kw = dict(member_kappa=0.5, member_mode="lcb")
    assert fv.calls == [(1, 1, kw), (B, S, kw)]
    # candidate 4's spread is sqrt(2) / 3 = 0.4714: 0.9 - 0.5 * 0.4714 = 0.664 still wins; one member of three agrees with the decision
    assert r["global_action_idx"] == 4 and r["member_kappa"] == 0.5 and r["member_agreement"] == 1
    want_spread = math.sqrt(2.0) / 3.0
    assert abs(r["spread"] - want_spread) < 1e-6 and abs(r["max_score"] - (0.9 - 0.5 * want_spread)) < 1e-6
    # a larger penalty (0.9 - 1.5 * 0.4714 = 0.193 < 0.3) flips the executed action inside group 1, and then two members agree
    fv = _StubVerifier(0.05, scores, ms)
    r = host.verify_and_select(fv, *args, process_image=False, member_kappa=1.5)
    assert r["global_action_idx"] == 5 and r["member_agreement"] == 2 and abs(r["spread"]) < 1e-6 and r["member_kappa"] == 1.5
    assert not np.array_equal(r["execute_action"][:6], r0["execute_action"][:6])
    # mode min reaches both stages as well (the gate sees candidate 0's worst member, 0.1, against a threshold of 0.2)
    fv = _StubVerifier(0.05, scores, ms)
    r = host.verify_and_select(fv, *args, process_image=False, threshold=0.2, member_kappa=0.0, member_mode="min")
    assert [c[2] for c in fv.calls] == [dict(member_kappa=0.0, member_mode="min")] * 2 and r["global_action_idx"] == 5
    # the gate is pessimistic: a confident stage 1 stays one call, with the keywords, and the figures are candidate 0's
    fv = _StubVerifier(0.5, scores, ms)
    r = host.verify_and_select(fv, *args, process_image=False, member_kappa=0.5)
    assert fv.calls == [(1, 1, kw)] and r["global_action_idx"] == 0 and abs(r["spread"]) < 1e-6 and r["member_agreement"] == 3
    # together with a prior: stage 1 gets the member keywords alone, stage 2 all four
    prior = np.zeros(B, dtype=np.float32)
    fv = _StubVerifier(0.05, scores, ms)
    host.verify_and_select(fv, *args, process_image=False, member_kappa=0.5, candidate_prior=prior, prior_beta=0.05)
    assert set(fv.calls[0][2]) == {"member_kappa", "member_mode"}
    assert set(fv.calls[1][2]) == {"member_kappa", "member_mode", "candidate_prior", "prior_beta"}
    # a verifier that does not know the keywords keeps working as long as member_kappa is None
    old = _OldVerifier()
    r = host.verify_and_select(old, *args, process_image=False)
    assert old.calls == 2 and r["member_kappa"] is None and "spread" not in r
    with pytest.raises(TypeError):
        host.verify_and_select(_OldVerifier(), *args, process_image=False, member_kappa=0.0)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            host.verify_and_select(_StubVerifier(0.05, scores, ms), *args, process_image=False, member_kappa=bad)
