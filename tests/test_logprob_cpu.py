"""Per-token log-probabilities, the part that needs no GPU: the float64 reference against torch.log_softmax on the warped scores
(what Hugging Face's warpers followed by compute_transition_scores compute), the fairness of the GPU tests' inputs, the teacher set,
host.sequence_logprob, the struct mirrors and the argument checks of the binding."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_is_log_softmax_of_the_warped_scores():
    l = np.array([0.0, 3.0, 1.0, 3.0, 2.0, -1.0, 3.0], dtype=np.float32)
    r = LR.reference_logprob_row(l, 0.0, 1.0, 2, 1.0)                       # the three tied maxima stay: each has probability 1/3
    assert np.allclose(r["lp"][[1, 3, 6]], -np.log(3.0), atol=1e-15) and np.isneginf(r["lp"][[0, 2, 4, 5]]).all()
    x, u = R.lm_like_rows(77, 12, 4096, 0, 4096)
    for T, k, p in [(1.0, 50, 1.0), (1.0, 0, 0.9), (0.7, 64, 0.95), (1.3, 20, 0.8), (1.5, 8, 1.0), (1.0, 0, 1.0)]:
        refs = LR.reference_logprob_rows(x, 0, 4096, u, T, k, p)
        for r, ref in enumerate(refs):
            s = x[r].double() / float(np.float32(T))
            s[torch.from_numpy(~ref["keep"])] = -float("inf")
            want = torch.log_softmax(s, dim=-1).numpy()
            assert np.array_equal(np.isneginf(want), np.isneginf(ref["lp"]))
            fin = ref["keep"]
            assert np.abs(want[fin] - ref["lp"][fin]).max() < 1e-12, (T, k, p, r)
            assert abs(np.log(np.exp(ref["lp"][fin]).sum())) < 1e-12           # a distribution over the kept set


def test_tolerance_has_the_derived_form():
    assert LR.TOL_A == pytest.approx(5.1e-6, rel=1e-9)
    assert float(LR.tolerance(40.0, 40.0)) == pytest.approx(5.1e-6 + 40 * 2.0 ** -23 + 40 * 2.0 ** -24, rel=1e-12)
    assert 1.1e-5 < float(LR.tolerance(40.0, 40.0)) < 1.3e-5
    assert float(LR.tolerance(0.0, 0.0)) == LR.TOL_A


@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_inputs_are_fair_and_the_teacher_set_mixes(case):
    """The GPU tests' inputs: at most one row of 64 left out, the picks' log-probabilities in [-7.2, -0.14], and the teacher set lands
    outside the kept set in 61-64 of 64 rows of every filtered case (and inside it in every row of an unfiltered one)."""
    x, u, lo, hi, T, k, p, refs = LR.case_data(case)
    left_out = sum(not r["cut_decided"] for r in refs)
    picks = np.array([r["lp"][r["token"]] for r in refs])
    teach = LR.teacher_tokens(refs, lo, hi)
    outside = sum(not r["keep"][t - lo] for r, t in zip(refs, teach))
    print(f"{LR.case_id(case)}: left out {left_out} | lp(pick) in [{picks.min():.3f}, {picks.max():.3f}] | teacher tokens outside the kept set {outside}")
    assert left_out <= 1 and left_out <= R.CAP * len(refs)
    assert np.isfinite(picks).all() and -7.2 <= picks.min() and picks.max() <= -0.14
    assert ((teach >= lo) & (teach < hi)).all()
    filtered = (0 < k < hi - lo) or p < 1.0
    assert (61 <= outside <= 64) if filtered else outside == 0


def test_sequence_logprob():
    from cover_vla_amd.host import sequence_logprob
    lp = torch.tensor([[-1.0, -2.0, -0.5, 0.0], [-0.25, 0.0, 0.0, 0.0], [-1.0, -1.0, -1.0, -1.0]])
    tok = torch.tensor([[5, 6, 1, 0], [1, 0, 0, 0], [7, 8, 9, 3]])
    assert torch.equal(sequence_logprob(lp), torch.tensor([-3.5, -0.25, -4.0]))
    assert torch.equal(sequence_logprob(lp, tok, pad_token_id=0), torch.tensor([-3.5, -0.25, -4.0]))
    assert torch.equal(sequence_logprob(lp, tok, pad_token_id=0, length_normalize=True), torch.tensor([-3.5 / 3, -0.25, -1.0]))
    assert torch.equal(sequence_logprob(lp, length_normalize=True), torch.tensor([-3.5 / 4, -0.25 / 4, -1.0]))
    # values scored elsewhere: a pad scores -inf there and is left out
    lp2 = lp.clone()
    lp2[tok == 0] = -float("inf")
    assert torch.equal(sequence_logprob(lp2, tok, pad_token_id=0), torch.tensor([-3.5, -0.25, -4.0]))
    assert torch.isneginf(sequence_logprob(lp2)[:2]).all()
    # numpy in, numpy out; a row of pads only divides by 1
    out = sequence_logprob(lp.numpy(), tok.numpy(), 0, True)
    assert isinstance(out, np.ndarray) and np.allclose(out, [-3.5 / 3, -0.25, -1.0])
    assert sequence_logprob(np.zeros((1, 3)), np.zeros((1, 3), dtype=np.int64), 0, True).tolist() == [0.0]


def test_struct_mirrors_and_symbols():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_token_sample_scored_args"] is L.TokenSampleScoredArgs
    assert L._STRUCTS["cover_token_logprob_args"] is L.TokenLogprobArgs
    assert "cover_token_sample_scored" in L.SYMBOLS and "cover_token_logprob" in L.SYMBOLS
    scored = [f[0] for f in L.TokenSampleScoredArgs._fields_]
    assert scored == [f[0] for f in L.TokenSampleArgs._fields_] + ["logprob_out"]
    assert C.sizeof(L.TokenSampleArgs) == 80 and C.sizeof(L.TokenSampleScoredArgs) == 88       # the plain struct did not grow
    lpn = [f[0] for f in L.TokenLogprobArgs._fields_]
    assert lpn == ["logits", "ld", "rows", "lo", "hi", "temperature", "top_k", "top_p", "token", "logprob_out", "kept_out"]
    assert C.sizeof(L.TokenLogprobArgs) == 64
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    for name, fields in (("cover_token_sample_scored_args", scored), ("cover_token_logprob_args", lpn)):
        body = hdr[hdr.index("typedef struct %s {" % name):hdr.index("} %s;" % name)]
        marks = {"logits": "logits;", "ld": " ld;", "rows": " rows;", "lo": " lo, hi;", "hi": " hi;"}
        pos = [body.index(marks.get(n, n + ";")) for n in fields]
        assert pos == sorted(pos), name
    assert "int cover_token_sample_scored(const cover_token_sample_scored_args* args, void* stream);" in hdr
    assert "int cover_token_logprob(const cover_token_logprob_args* args, void* stream);" in hdr
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_token_sample_scored") and hasattr(h, "cover_token_logprob")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_token_sample_scored_args") == C.sizeof(L.TokenSampleScoredArgs)
        assert h.cover_sizeof(b"cover_token_logprob_args") == C.sizeof(L.TokenLogprobArgs)
        assert h.cover_sizeof(b"cover_token_sample_args") == 80


def test_argument_validation_needs_no_device():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    lg = torch.zeros(2, 16)
    tok = torch.zeros(2, dtype=torch.int64)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=-0.5), dict(top_k=-1)):
        with pytest.raises(CoverError):
            ops.token_logprob(lg, 0, 16, tok, **kw)
    with pytest.raises(CoverError):
        ops.token_logprob(lg, 8, 8, tok)
    with pytest.raises(CoverError):           # valid arguments, host tensors: there is no CPU path
        ops.token_logprob(lg, 0, 16, tok)
    with pytest.raises(CoverError):
        ops.token_sample(lg, 0, 16, torch.zeros(2), out_logprob=torch.zeros(2))


def test_signatures_default_to_off():
    from cover_vla_amd import ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTTokens
    assert inspect.signature(ops.token_sample).parameters["out_logprob"].default is None
    p = inspect.signature(ops.token_logprob).parameters
    assert list(p)[:4] == ["logits", "lo", "hi", "tokens"]
    assert (p["temperature"].default, p["top_k"].default, p["top_p"].default, p["out"].default, p["out_kept"].default) == (1.0, 0, 1.0, None, None)
    assert inspect.signature(OpenVLA.sample).parameters["return_logprobs"].default is False
    assert inspect.signature(PI0FASTTokens.generate_tokens).parameters["return_logprobs"].default is False
    assert PI0FASTConfig().return_logprobs is False
