"""Prior-weighted selection, the part that needs no GPU: the fp32 reference of tests/prior_ref.py against a float64 restatement and the
oracle's grouped arg-max, the fairness of the GPU tests' inputs, the struct mirror against a compiled probe of the header, the argument
checks of ops.prior_select and host.verify_and_select's use of the prior."""
import ctypes as C
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import prior_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_small_example_by_hand():
    scores = np.array([0.25, 0.125, 0.25, 0.0], dtype=np.float32)
    lps = np.array([[-1.0, -0.5], [-0.25, -0.25], [-0.5, -1.0], [-np.inf, -1.0]], dtype=np.float32)
    r = PR.reference(scores, lps, None, 0, 2, 1.0, False, 2)
    assert r["prior"].tolist() == [-1.5, -0.5, -1.5, -np.inf] and r["combined"].tolist() == [-1.25, -0.375, -1.25, -np.inf]
    assert r["group_mean"].tolist() == [-0.8125, -np.inf] and r["result"].tolist() == [1, 0, 1, 0]
    assert r["best"].tolist() == [-0.375, -0.8125] and r["ranked"].tolist() == [1, 0]
    r = PR.reference(scores, lps, None, 0, 2, 0.0, False, 2)                    # beta 0: the scores, whatever the prior holds
    assert r["combined"].tolist() == scores.tolist() and r["result"].tolist() == [0, 0, 0, 0] and r["ranked"].tolist() == [0, 1]
    tok = np.array([[5, 0], [0, 0], [5, 5], [0, 5]])                            # pad 0: candidate 1 has no counted step
    r = PR.reference(scores, lps, tok, 0, 4, 1.0, True, 4)
    assert r["prior"].tolist() == [-1.0, 0.0, -0.75, -1.0] and r["result"].tolist() == [1, 0, 1, 0]
    assert r["ranked"].tolist() == [1, 2, 0, 3]                                 # combined 0.125, -0.5, -0.75, -1.0
    r = PR.reference(np.zeros(4, dtype=np.float32), np.full((4, 1), -np.inf, dtype=np.float32), None, 0, 2, 0.5, False, 2)
    assert r["result"].tolist() == [0, 0, 0, 0] and r["ranked"].tolist() == [0, 1]          # every group -inf: group 0, member 0


def test_reference_agrees_with_float64_where_the_margin_decides():
    """Same winner wherever the float64 margin between the two best exceeds the fp32 error bound of the chain (steps * 2^-24 * sum |lp|
    plus the two roundings; prior_ref.reference_f64). The quantised variant is made of exact ties and is left to the bit-exact tests."""
    cs = PR.cases(variants=("uniform", "neginf"))
    left_out = 0
    for c in cs:
        scores, lps, tokens = PR.make_inputs(c)
        N, gs, steps, top_m = c["shape"]
        want, decided = PR.reference_f64(scores, lps, tokens, PR.PAD_ID, gs, c["beta"], c["length_normalize"])
        if not decided:
            left_out += 1
            continue
        assert int(PR.case_reference(c)["result"][0]) == want, PR.case_id(c)
    print(f"left out {left_out} of {len(cs)} cases ({100.0 * left_out / len(cs):.1f} %)")
    assert left_out <= 0.10 * len(cs)


def test_beta_zero_is_the_oracles_grouped_argmax():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from cover_ref import verifier as V
    n = 0
    for c in PR.cases():
        if c["beta"] != 0.0:
            continue
        scores, lps, tokens = PR.make_inputs(c)
        N, gs, steps, top_m = c["shape"]
        r = PR.case_reference(c)
        gidx, g, i, mx, gm = V.select(torch.from_numpy(scores), gs)
        assert r["result"].tolist() == [gidx, g, i, 0] and float(r["best"][0]) == mx, PR.case_id(c)
        assert np.array_equal(r["combined"].view(np.int32), scores.view(np.int32))
        n += 1
    assert n == len(PR.cases()) // 3


def test_inputs_are_fair():
    """A condition on the GPU tests' inputs, checked with the reference alone: an implementation that ignored the prior could not pass."""
    moved = total = 0
    for c in PR.cases():
        if c["beta"] == 0.0 or c["shape"][0] == 1:
            continue
        base = int(PR.case_reference(dict(c, beta=0.0))["result"][0])
        moved += int(PR.case_reference(c)["result"][0]) != base
        total += 1
    print(f"the prior moves the winner in {moved} of {total} cases with beta > 0 and more than one candidate")
    assert moved >= 0.25 * total
    tie_max = tie_ranked = n_q = 0
    for c in PR.cases(variants=("quantised",)):
        N, gs, steps, top_m = c["shape"]
        if gs == 1:
            continue
        r = PR.case_reference(c)
        grp = r["combined"][r["result"][1] * gs:(r["result"][1] + 1) * gs]
        tie_max += int((grp == r["best"][0]).sum() > 1)
        tie_ranked += int(len(np.unique(r["combined"][r["ranked"]])) < len(r["ranked"]))
        n_q += 1
    print(f"quantised variant: the maximum is tied in {tie_max} and the ranked list holds a tie in {tie_ranked} of {n_q} cases")
    assert tie_max >= n_q // 4 and tie_ranked >= n_q // 2
    # the -inf variant reaches the decision whenever beta > 0: a whole group at -inf, and finite winners
    for c in PR.cases(variants=("neginf",)):
        r = PR.case_reference(c)
        N, gs, steps, top_m = c["shape"]
        if c["beta"] > 0:
            assert np.isneginf(r["group_mean"]).any() and np.isneginf(r["combined"]).any()
            assert np.isfinite(r["best"]).all() or N // gs == 1
    # a candidate whose every step is a pad has prior 0.0
    for c in PR.cases(variants=("uniform",)):
        if c["with_tokens"]:
            assert PR.case_reference(c)["prior"][c["shape"][0] // 2] == 0.0


# ------------------------------------------------------------------------------------------------ binding
_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cover_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(cover_prior_select_args, f));
int main(void) {
    printf("sizeof %zu\n", sizeof(cover_prior_select_args));
    F(scores) F(logprobs) F(lp_n_stride) F(lp_t_stride) F(tokens) F(tok_n_stride) F(tok_t_stride) F(pad_token_id) F(N) F(steps)
    F(group_size) F(top_m) F(beta) F(length_normalize) F(prior_out) F(combined_out) F(group_mean_out) F(result_out) F(best_out)
    F(ranked_out)
    printf("abi %d\n", COVER_ABI_VERSION);
    return 0;
}
"""


def test_struct_mirror_matches_a_compiled_probe_of_the_header(tmp_path):
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_prior_select_args"] is L.PriorSelectArgs
    assert L.SYMBOLS["cover_prior_select"] == (C.c_int, [C.POINTER(L.PriorSelectArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_prior_select(const cover_prior_select_args* args, void* stream);" in hdr
    assert hdr.index("int cover_group_argmax(") < hdr.index("typedef struct cover_prior_select_args {")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed to probe include/cover_hip.h"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("abi")) == 1
    assert int(out.pop("sizeof")) == C.sizeof(L.PriorSelectArgs)
    assert list(out) == [f[0] for f in L.PriorSelectArgs._fields_]
    for name, _ in L.PriorSelectArgs._fields_:
        assert int(out[name]) == getattr(L.PriorSelectArgs, name).offset, name
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_prior_select")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_prior_select_args") == C.sizeof(L.PriorSelectArgs)
        h.cover_abi_version.restype = C.c_int
        assert h.cover_abi_version() == 1


def test_argument_validation_needs_no_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    s, lp = torch.zeros(8), torch.zeros(8, 3)
    tok = torch.ones(8, 3, dtype=torch.int64)
    bad = [
        (s.double(), lp, 2, 0.1, {}), (s, lp.double(), 2, 0.1, {}), (s.numpy(), lp, 2, 0.1, {}),          # dtype / kind
        (s.view(2, 4), lp, 2, 0.1, {}), (torch.zeros(16)[::2], lp, 2, 0.1, {}), (torch.zeros(0), torch.zeros(0, 3), 1, 0.1, {}),
        (s, torch.zeros(7, 3), 2, 0.1, {}), (s, torch.zeros(3, 8), 2, 0.1, {}), (s, torch.zeros(8, 3, 1), 2, 0.1, {}),    # shape mismatch
        (s, torch.zeros(8, 0), 2, 0.1, {}), (s, torch.zeros(8, 4097), 2, 0.1, {}),
        (s, lp, 3, 0.1, {}), (s, lp, 0, 0.1, {}), (s, lp, -2, 0.1, {}),                                     # N % group_size
        (torch.zeros(8192), torch.zeros(8192), 1, 0.1, {}), (torch.zeros(8192), torch.zeros(8192), 8192, 0.1, {}),
        (s, lp, 2, -0.1, {}), (s, lp, 2, float("nan"), {}), (s, lp, 2, float("inf"), {}), (s, lp, 2, 1e39, {}),   # beta
        (s, lp, 2, 0.1, dict(top_m=3)), (s, lp, 2, 0.1, dict(top_m=-1)),                                   # top_m
        (torch.zeros(256), torch.zeros(256), 128, 0.1, dict(top_m=65)),
        (s, lp, 2, 0.1, dict(tokens=tok)), (s, lp, 2, 0.1, dict(pad_token_id=0)),                           # given together
        (s, lp, 2, 0.1, dict(tokens=tok.int(), pad_token_id=0)), (s, lp, 2, 0.1, dict(tokens=tok[:, :2], pad_token_id=0)),
        (s, lp, 2, 0.1, dict(tokens=tok.numpy(), pad_token_id=0)),
    ]
    for scores, lps, gs, beta, kw in bad:
        with pytest.raises(CoverError):
            ops.prior_select(scores, lps, gs, beta, **kw)
    for kw in (dict(), dict(tokens=tok, pad_token_id=0, length_normalize=True, top_m=2)):          # valid arguments, host tensors: no CPU path
        with pytest.raises(CoverError, match="device"):
            ops.prior_select(s, lp, 2, 0.1, **kw)
        with pytest.raises(CoverError, match="device"):
            ops.prior_select(s, lp.t().contiguous().t(), 2, 0.0, **kw)


def test_signatures_default_to_off():
    from cover_vla_amd import host, ops
    from cover_vla_amd.verifier import EfficientEnsembleMerged as E
    p = inspect.signature(ops.prior_select).parameters
    assert list(p)[:4] == ["scores", "logprobs", "group_size", "beta"]
    assert [(k, p[k].default) for k in list(p)[4:]] == [("tokens", None), ("pad_token_id", None), ("length_normalize", False), ("top_m", 0)]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[4:])
    p = inspect.signature(E.score_histories).parameters
    assert [(k, p[k].default) for k in ("prior", "prior_beta", "length_normalize", "prior_tokens", "pad_token_id", "top_m")] == \
        [("prior", None), ("prior_beta", 0.0), ("length_normalize", False), ("prior_tokens", None), ("pad_token_id", None), ("top_m", 0)]
    for fn in (E.score_features, E.compute_max_similarity_scores_batch, host.verify_and_select):
        p = inspect.signature(fn).parameters
        assert p["candidate_prior"].default is None and p["prior_beta"].default == 0.0


# ------------------------------------------------------------------------------------------------ host.verify_and_select
class _StubVerifier:
    """Scripted scores; knows the two keywords and selects on score + beta * prior with the reference's arithmetic."""

    def __init__(self, stage1, scores):
        self.stage1, self.scores, self.calls = stage1, np.asarray(scores, dtype=np.float32), []

    def compute_max_similarity_scores_batch(self, images, instructions, all_action_histories, cfg_repeat_language_instructions=1, **kw):
        self.calls.append((len(all_action_histories), cfg_repeat_language_instructions, dict(kw)))
        if len(all_action_histories) == 1:
            return self.stage1, instructions[0], all_action_histories[0], torch.tensor(0)
        g = cfg_repeat_language_instructions
        prior = np.asarray(kw.get("candidate_prior", np.zeros(len(self.scores))), dtype=np.float32)
        r = PR.reference(self.scores, prior, None, 0, g, kw.get("prior_beta", 0.0), False, 0)
        gi = int(r["result"][0])
        return float(r["best"][0]), instructions[0], all_action_histories[gi], torch.tensor(gi)


class _OldVerifier:
    """A verifier that does not know the keywords."""

    def __init__(self):
        self.calls = 0

    def compute_max_similarity_scores_batch(self, images, instructions, all_action_histories, cfg_repeat_language_instructions=1):
        self.calls += 1
        return 0.05, instructions[0], all_action_histories[0], torch.tensor(0)


def test_verify_and_select_applies_the_prior_in_stage_two_only():
    from cover_vla_amd import host
    rng = np.random.default_rng(1)
    B, S = 6, 3
    q = [rng.uniform(-1, 1, size=(B, 7)).astype(np.float32) for _ in range(4)]
    tasks = ["a"] * 3 + ["b"] * 3
    hist = [rng.normal(size=7) for _ in range(3)]
    scores = [0.1, 0.1, 0.1, 0.2, 0.9, 0.3]
    prior = np.array([-1.0, -1.0, -1.0, -30.0, -30.0, -30.0], dtype=np.float32)     # the policy finds group 1 very unlikely
    args = (None, "a", tasks, q, hist, S)
    # the default call: no keyword reaches the verifier, the score-only winner, prior_beta 0.0 in the record
    fv = _StubVerifier(0.05, scores)
    r0 = host.verify_and_select(fv, *args, process_image=False)
    assert fv.calls == [(1, 1, {}), (B, S, {})] and r0["global_action_idx"] == 4 and r0["prior_beta"] == 0.0 and "prior" not in r0
    # a prior with beta 0, or a beta without a prior: still nothing forwarded, the same decision
    for kw in (dict(candidate_prior=prior), dict(prior_beta=0.5), dict(candidate_prior=prior, prior_beta=0.0)):
        fv = _StubVerifier(0.05, scores)
        r = host.verify_and_select(fv, *args, process_image=False, **kw)
        assert [c[2] for c in fv.calls] == [{}, {}] and r["global_action_idx"] == 4 and "prior" not in r
        assert np.array_equal(r["execute_action"], r0["execute_action"]) and r["max_score"] == r0["max_score"]
    # beta > 0 flips the executed action: group 0 wins (0.1 - 0.05 * 1 against a mean of 0.4667 - 0.05 * 30)
    fv = _StubVerifier(0.05, scores)
    r = host.verify_and_select(fv, *args, process_image=False, candidate_prior=prior, prior_beta=0.05)
    assert fv.calls[0] == (1, 1, {})                                                # stage 1 scores one candidate: no prior
    assert fv.calls[1][:2] == (B, S) and set(fv.calls[1][2]) == {"candidate_prior", "prior_beta"}
    assert fv.calls[1][2]["prior_beta"] == 0.05 and fv.calls[1][2]["candidate_prior"] is prior
    assert r["global_action_idx"] == 0 and r["max_instruction"] == "a" and r["prior_beta"] == 0.05 and r["prior"] == -1.0
    assert r["max_score"] == float(np.float32(0.1) + np.float32(0.05) * np.float32(-1.0))        # the combined score
    assert not np.array_equal(r["execute_action"][:6], r0["execute_action"][:6])
    assert np.array_equal(r["remaining"][0], q[1][0:1])
    # per-step values: the record carries the winner's sum
    r = host.verify_and_select(_StubVerifier(0.05, scores), *args, process_image=False, prior_beta=0.05,
                               candidate_prior=torch.tensor(np.stack([prior / 2, prior / 2], axis=1)))
    assert r["prior"] == -1.0
    # stage 1 confident: one call, no prior anywhere
    fv = _StubVerifier(0.5, scores)
    r = host.verify_and_select(fv, *args, process_image=False, candidate_prior=prior, prior_beta=0.05)
    assert fv.calls == [(1, 1, {})] and r["global_action_idx"] == 0 and "prior" not in r and r["prior_beta"] == 0.05
    # a verifier that does not know the keywords keeps working as long as beta is 0
    old = _OldVerifier()
    host.verify_and_select(old, *args, process_image=False, candidate_prior=prior)
    assert old.calls == 2
    with pytest.raises(TypeError):
        host.verify_and_select(_OldVerifier(), *args, process_image=False, candidate_prior=prior, prior_beta=0.05)
    for beta in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            host.verify_and_select(_StubVerifier(0.05, scores), *args, process_image=False, candidate_prior=prior, prior_beta=beta)
