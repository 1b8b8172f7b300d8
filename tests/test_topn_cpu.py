"""Top-n alternatives and entropy, the part that needs no GPU: the float64 reference of tests/topn_ref.py against torch.topk /
log_softmax / Categorical.entropy on the warped scores, the derived tolerance, the fairness of the GPU tests' inputs, the struct mirror,
the argument checks of the binding and host.step_entropy_summary."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import sampling_ref as R
from tests import topn_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_is_topk_log_softmax_and_categorical_entropy():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(10, 2048, generator=g) * 3.0                            # continuous: no ties
    for T, k, p in [(1.0, 0, 1.0), (1.0, 50, 1.0), (0.7, 64, 0.95), (1.3, 20, 0.8), (1.0, 0, 0.9)]:
        for r, ref in enumerate(TR.reference_topn_rows(x, 0, 2048, 5, T, k, p)):
            s = x[r].double() / float(np.float32(T))
            s[torch.from_numpy(~ref["keep"])] = -float("inf")
            logp = torch.log_softmax(s, dim=-1)
            val, idx = torch.topk(logp, 5)
            assert np.array_equal(idx.numpy(), ref["top_tok"]), (T, k, p, r)
            assert np.abs(val.numpy() - ref["top_lp"]).max() < 1e-12
            H = float(torch.distributions.Categorical(logits=s).entropy())
            assert abs(H - ref["H"]) < 1e-10, (T, k, p, r, H, ref["H"])
            assert -1e-12 <= ref["H"] <= np.log(ref["kept"]) + 1e-12
    # padding and the tie rule
    r = TR.reference_topn_row(np.array([0.0, 3.0, 1.0, 3.0, -0.0, -1.0, 3.0], dtype=np.float32), 5, 1.0, 2, 1.0)
    assert r["top_tok"].tolist() == [1, 3, 6, -1, -1] and np.isneginf(r["top_lp"][3:]).all()
    assert np.allclose(r["top_lp"][:3], -np.log(3.0), atol=1e-15) and abs(r["H"] - np.log(3.0)) < 1e-15
    r = TR.reference_topn_row(np.array([0.0, 3.0, 1.0, 3.0, -0.0, -1.0, 3.0], dtype=np.float32), 6, 1.0, 0, 1.0)
    assert r["top_tok"].tolist() == [1, 3, 6, 2, 0, 4]                       # +0.0 and -0.0 are equal: by index


def test_entropy_tolerance_has_the_derived_form():
    assert TR.TOL_H_ABS == 5.2e-6 and TR.TOL_H_REL == 1.05e-5 + 2.0 ** -24
    assert LR.TOL_A + 2.0 ** -24 <= TR.TOL_H_ABS                             # log M, and the conversion of S
    assert (4.8e-6 + 2.4e-7) + 3 * 2.0 ** -24 + LR.TOL_A <= 1.05e-5          # a term of S, and M under it
    assert float(TR.tolerance_entropy(0.0)) == 5.2e-6
    assert float(TR.tolerance_entropy(5.0)) == pytest.approx(5.2e-6 + 5 * 1.05e-5 + 5 * 2.0 ** -24, rel=1e-12)


@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_inputs_are_fair(case):
    """The GPU tests' inputs: at most one row of 64 left out, entropies that span an interval, alternatives that differ in probability."""
    refs = TR.case_refs(case)
    left_out = sum(not r["cut_decided"] for r in refs)
    H = np.array([r["H"] for r in refs])
    print(f"{LR.case_id(case)}: left out {left_out} | entropy in [{H.min():.4f}, {H.max():.4f}] | kept in "
          f"[{min(r['kept'] for r in refs)}, {max(r['kept'] for r in refs)}]")
    assert left_out <= 1 and left_out <= R.CAP * len(refs)
    assert H.min() > 0.05 and H.max() - H.min() > 0.25                        # thousands of times the tolerance (top_k = 8: H <= 2.08)
    assert all((np.diff(r["top_lp"][:min(5, r["kept"])]) <= 0).all() for r in refs)


def test_tie_inputs_are_decided():
    for name, (x, lo, hi, n, T, k) in TR.tie_inputs().items():
        refs = TR.reference_topn_rows(x, lo, hi, n, T, k, 1.0)
        assert all(r["cut_decided"] for r in refs), name
        for r in refs:
            m = min(n, r["kept"])
            assert (r["top_tok"][:m] >= 0).all() and (r["top_tok"][m:] == -1).all(), name
    t = TR.tie_inputs()
    x, lo, hi, n, T, k = t["constant row"]
    assert hi - lo == 5000 and TR.reference_topn_row(x[0, lo:hi].numpy(), n, T, k, 1.0)["top_tok"].tolist() == list(range(n))
    x, lo, hi, n, T, k = t["plateau of 100 maxima"]
    r = TR.reference_topn_row(x[0, lo:hi].numpy(), n, T, k, 1.0)
    assert r["top_tok"].tolist() == sorted(np.nonzero(x[0].numpy() == 9.0)[0].tolist())[:64]
    x, lo, hi, n, T, k = t["top_k 3, n 8"]
    assert all(r["kept"] == 3 and r["top_tok"][3:].tolist() == [-1] * 5 for r in TR.reference_topn_rows(x, lo, hi, n, T, k, 1.0))
    x, lo, hi, n, T, k = t["hi - lo < n"]
    assert all(r["kept"] == 5 and (r["top_tok"][5:] == -1).all() for r in TR.reference_topn_rows(x, lo, hi, n, T, k, 1.0))


def test_struct_mirror_and_symbol():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_token_topn_args"] is L.TokenTopnArgs and "cover_token_topn" in L.SYMBOLS
    names = [f[0] for f in L.TokenTopnArgs._fields_]
    assert names == ["logits", "ld", "rows", "lo", "hi", "temperature", "top_k", "top_p", "n", "token_out", "ld_tok", "logprob_out", "ld_lp",
                     "entropy_out", "kept_out"]
    assert C.sizeof(L.TokenTopnArgs) == 96 and C.sizeof(L.TokenLogprobArgs) == 64
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    body = hdr[hdr.index("typedef struct cover_token_topn_args {"):hdr.index("} cover_token_topn_args;")]
    marks = {"logits": "logits;", "ld": " ld;", "rows": " rows;", "lo": " lo, hi;", "hi": " hi;", "n": " n;"}
    pos = [body.index(marks.get(n, n + ";")) for n in names]
    assert pos == sorted(pos)
    assert "int cover_token_topn(const cover_token_topn_args* args, void* stream);" in hdr
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_token_topn")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_token_topn_args") == C.sizeof(L.TokenTopnArgs)
        h.cover_abi_version.restype = C.c_int
        assert h.cover_abi_version() == 1


def test_argument_validation_needs_no_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    lg = torch.zeros(2, 16)
    for kw in (dict(n=0), dict(n=65), dict(n=-1), dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=-0.5),
               dict(top_k=-1), dict(lo=8, hi=8), dict(lo=-1), dict(hi=17)):
        args = dict(lo=0, hi=16, n=4)
        args.update(kw)
        with pytest.raises(CoverError):
            ops.token_topn(lg, **args)
    with pytest.raises(CoverError):
        ops.token_topn(lg.double(), 0, 16, 4)
    with pytest.raises(CoverError):
        ops.token_topn(torch.zeros(2, 32)[:, ::2], 0, 16, 4)
    bad_outs = (dict(out_tok=torch.zeros(2, 4, dtype=torch.int32)), dict(out_tok=torch.zeros(2, 5, dtype=torch.int64)),
                dict(out_tok=torch.zeros(2, 8, dtype=torch.int64)[:, ::2]), dict(out_tok=torch.zeros(4, 2, dtype=torch.int64).t()),
                dict(out_logprob=torch.zeros(2, 4, dtype=torch.float64)), dict(out_logprob=torch.zeros(3, 4)),
                dict(out_entropy=torch.zeros(2, dtype=torch.float64)), dict(out_entropy=torch.zeros(4)[::2]),
                dict(out_kept=torch.zeros(2, dtype=torch.int64)), dict(out_kept=torch.zeros(3, dtype=torch.int32)))
    for kw in bad_outs:
        with pytest.raises(CoverError):
            ops.token_topn(lg, 0, 16, 4, **kw)
    with pytest.raises(CoverError):           # valid arguments, host tensors: there is no CPU path
        ops.token_topn(lg, 0, 16, 4, out_tok=torch.zeros(3, 2, 4, dtype=torch.int64)[1], out_logprob=torch.zeros(2, 8)[:, :4])


def test_signatures_default_to_off():
    from cover_vla_amd import ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTTokens
    p = inspect.signature(ops.token_topn).parameters
    assert list(p)[:4] == ["logits", "lo", "hi", "n"]
    assert [p[k].default for k in ("temperature", "top_k", "top_p", "out_tok", "out_logprob", "out_entropy", "out_kept")] == \
        [1.0, 0, 1.0, None, None, None, None]
    assert inspect.signature(OpenVLA.sample).parameters["top_logprobs"].default == 0
    assert inspect.signature(PI0FASTTokens.generate_tokens).parameters["top_logprobs"].default == 0
    assert PI0FASTConfig().top_logprobs == 0


def test_step_entropy_summary():
    from cover_vla_amd.host import step_entropy_summary
    ent = torch.tensor([[1.0, 3.0, 2.0, 0.0], [0.5, 0.0, 0.0, 0.0], [1.0, 1.0, 4.0, 2.0]])
    tok = torch.tensor([[5, 6, 1, 0], [1, 0, 0, 0], [7, 8, 9, 3]])            # EOS = 1, pad = 0: row 1 finishes at once
    mean, mx = step_entropy_summary(ent, tok, 0)
    assert torch.equal(mean, torch.tensor([2.0, 0.5, 2.0])) and torch.equal(mx, torch.tensor([3.0, 0.5, 4.0]))
    mean, mx = step_entropy_summary(ent)                                       # every step counts
    assert torch.equal(mean, torch.tensor([1.5, 0.125, 2.0])) and torch.equal(mx, torch.tensor([3.0, 0.5, 4.0]))
    # a value at a pad step is left out, whatever it is; a row of pads only gives 0.0
    ent2 = ent.clone()
    ent2[tok == 0] = 9.0
    mean, mx = step_entropy_summary(ent2, tok, 0)
    assert torch.equal(mean, torch.tensor([2.0, 0.5, 2.0])) and torch.equal(mx, torch.tensor([3.0, 0.5, 4.0]))
    mean, mx = step_entropy_summary(ent.numpy(), tok.numpy(), 0)
    assert isinstance(mean, np.ndarray) and np.allclose(mean, [2.0, 0.5, 2.0]) and np.allclose(mx, [3.0, 0.5, 4.0])
    mean, mx = step_entropy_summary(np.ones((1, 3)), np.zeros((1, 3), dtype=np.int64), 0)
    assert mean.tolist() == [0.0] and mx.tolist() == [0.0]
