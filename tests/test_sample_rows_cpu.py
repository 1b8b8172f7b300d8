"""Sampling parameters per row, the part that needs no GPU: the fairness of the GPU tests' inputs (the reference alone), host.sampling_ladder,
the wrappers' host-side validation, the binding's struct mirrors and ops.pick_token's dispatch with row_params."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import sample_rows_ref as RR
from tests import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(RR.CASES))
def test_inputs_are_fair(name):
    """The GPU comparison may leave out undecided rows; the reference alone shows that it cannot quietly skip more than CAP of a case."""
    x, u, lo, hi, (T, k, p), refs = RR.case_data(name)
    und = RR.undecided(refs)
    print(f"{name}: [{lo}, {hi}) rows {len(refs)} | undecided at DELTA {len(und)} | kept {[r['kept'] for r in refs[:8]]}")
    assert len(refs) == RR.CASES[name][3] and len(und) <= R.CAP * len(refs)
    for r, ref in enumerate(refs):
        if T[r] == 0:
            assert ref["greedy"] and ref["kept"] == hi - lo and ref["token"] == int(np.argmax(x[r, lo:hi].numpy()))
        elif k[r] > 0 and p[r] >= 1:
            assert ref["kept"] == k[r]                       # continuous data: no ties at the k-th value


def test_case_table_is_the_issue_s():
    assert RR.LADDER == [(0, 0, 1), (1, 0, 1), (0.7, 64, 0.95), (1, 50, 1), (1, 0, 0.9), (1.5, 8, 1), (1.3, 20, 0.8), (0.5, 1, 1)]
    assert RR.CASES == {"narrow": (32064, 31744, 32000, 32, 7101), "mid": (4200, 3, 4100, 32, 7102), "wide": (257152, 3, 257150, 16, 7103)}
    assert RR.CASES["mid"][2] - RR.CASES["mid"][1] == 4097
    T, k, p = RR.ladder_params(10)
    assert T.dtype == np.float32 and k.dtype == np.int32 and p.dtype == np.float32
    assert T[8] == 0 and (float(T[9]), int(k[9]), float(p[9])) == (1.0, 0, 1.0) and int(k[2]) == 64


def test_sampling_ladder():
    from cover_vla_amd.host import sampling_ladder
    T, k, p = sampling_ladder(2, 4, [0, 0.7, 1.0, 1.3], top_k=[0, 0, 50, 0])
    assert T.dtype == np.float32 and k.dtype == np.int32 and p.dtype == np.float32
    assert T.tolist() == [np.float32(v) for v in (0, 0.7, 1.0, 1.3)] * 2 and k.tolist() == [0, 0, 50, 0] * 2 and p.tolist() == [1.0] * 8
    for i in range(8):                                       # candidate i belongs to prompt i // n_samples and carries entry i % n_samples
        assert T[i] == np.float32([0, 0.7, 1.0, 1.3][i % 4])
    T, k, p = sampling_ladder(3, 2, 0.5, top_k=7, top_p=(0.9, 1.0))
    assert T.tolist() == [0.5] * 6 and k.tolist() == [7] * 6 and p.tolist() == [np.float32(0.9), 1.0] * 3
    assert all(a.shape == (1,) for a in sampling_ladder(1, 1, 0.0))
    for bad in (dict(temperature=[0, 1, 2]), dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=[0, float("inf")]),
                dict(temperature=1.0, top_p=0.0), dict(temperature=1.0, top_p=[0.5, -1]), dict(temperature=1.0, top_k=-1),
                dict(temperature=1.0, top_k=1.5), dict(temperature=1.0, top_k=[1, 2, 3]), dict(temperature=[[0, 1]])):
        with pytest.raises(ValueError):
            sampling_ladder(2, 2, **bad)
    for n_prompts, n_samples in ((0, 2), (2, 0)):
        with pytest.raises(ValueError):
            sampling_ladder(n_prompts, n_samples, 1.0)


def test_struct_mirrors_and_symbols():
    from cover_vla_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    table = {"cover_token_sample_rows": (L.TokenSampleRowsArgs, 96), "cover_token_logprob_rows": (L.TokenLogprobRowsArgs, 80),
             "cover_token_topn_rows": (L.TokenTopnRowsArgs, 112)}
    for sym, (st, size) in table.items():
        assert sym in L.SYMBOLS and L._STRUCTS[sym + "_args"] is st and C.sizeof(st) == size
        body = hdr[hdr.index("typedef struct %s_args {" % sym):hdr.index("} %s_args;" % sym)]
        pos = [re.search(r" lo, hi;" if f == "lo" else r"[ *]%s;" % f, body).start() for f, _ in st._fields_ if f != "hi"]
        assert pos == sorted(pos), sym                       # the header declares the same fields in the same order
        assert "int %s(const %s_args* args, void* stream);" % (sym, sym) in hdr
    assert "#define COVER_ABI_VERSION 1" in hdr
    # the scalar structs are what they were
    assert C.sizeof(L.TokenSampleArgs) == 80 and C.sizeof(L.TokenSampleScoredArgs) == 88 and C.sizeof(L.TokenTopnArgs) == 96
    if os.path.exists(L.LIB_PATH):                           # cover_sizeof is host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        h.cover_sizeof.restype = C.c_size_t
        for sym, (st, size) in table.items():
            assert hasattr(h, sym) and h.cover_sizeof((sym + "_args").encode()) == C.sizeof(st)


def test_host_side_validation_needs_no_device(monkeypatch):
    """Bad Python / CPU parameters and bad shapes raise before any device call (and before the library is even loaded)."""
    from cover_vla_amd import _lib as L, ops

    def touched(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "lib", touched)
    lg, u, tok = torch.zeros(3, 16), torch.zeros(3), torch.zeros(3, dtype=torch.int64)
    calls = {
        "token_sample_rows": lambda T, k=None, p=None, **kw: ops.token_sample_rows(kw.pop("lg", lg), kw.pop("lo", 0), kw.pop("hi", 16), kw.pop("u", u), T, k, p, **kw),
        "token_logprob_rows": lambda T, k=None, p=None, **kw: ops.token_logprob_rows(kw.pop("lg", lg), kw.pop("lo", 0), kw.pop("hi", 16), kw.pop("tok", tok), T, k, p, **kw),
        "token_topn_rows": lambda T, k=None, p=None, **kw: ops.token_topn_rows(kw.pop("lg", lg), kw.pop("lo", 0), kw.pop("hi", 16), kw.pop("n", 4), T, k, p, **kw),
    }
    nan, inf = float("nan"), float("inf")
    for name, call in calls.items():
        for T, k, p in (([1, -1, 1], None, None), ([1, nan, 1], None, None), ([1, inf, 1], None, None), ([1, 1], None, None), (None, None, None),
                        ([1, 1, 1], [0, -1, 0], None), ([1, 1, 1], [0, 1.5, 0], None), ([1, 1, 1], [0, 0], None),
                        ([1, 1, 1], None, [1, 0, 1]), ([1, 1, 1], None, [1, nan, 1]), ([1, 1, 1], None, [1, 1, 1, 1]),
                        (torch.tensor([1.0, -2.0, 1.0]), None, None), (torch.ones(3), torch.tensor([0, -3, 0], dtype=torch.int32), None),
                        (torch.ones(3), None, torch.tensor([1.0, 0.0, 1.0])), (np.ones((3, 1)), None, None), ("abc", None, None)):
            with pytest.raises(L.CoverError):
                call(T, k, p)
        for kw in (dict(lo=8, hi=8), dict(lo=-1), dict(hi=17), dict(lg=torch.zeros(3, 16, dtype=torch.float64)), dict(lg=torch.zeros(3, 16)[:, ::2], hi=8)):
            with pytest.raises(L.CoverError):
                call([1, 0, 1], **kw)
        with pytest.raises(L.CoverError):                    # valid arguments, host tensors: there is no CPU path
            call([1, 0, 0.5], [0, 3, 0], [1, 0.5, 1])
    with pytest.raises(L.CoverError):
        calls["token_sample_rows"]([1, 1, 1], u=None)
    with pytest.raises(L.CoverError):
        calls["token_sample_rows"]([1, 1, 1], u=torch.zeros(2))
    with pytest.raises(L.CoverError):
        calls["token_sample_rows"]([1, 1, 1], out_kept=torch.zeros(3))
    with pytest.raises(L.CoverError):
        calls["token_logprob_rows"]([1, 1, 1], tok=torch.zeros(3, dtype=torch.int32))
    for n in (0, 65):
        with pytest.raises(L.CoverError):
            calls["token_topn_rows"]([1, 1, 1], n=n)
    with pytest.raises(L.CoverError):
        calls["token_topn_rows"]([1, 1, 1], out_tok=torch.zeros(3, 5, dtype=torch.int64))


def test_pick_token_dispatch_with_row_params(monkeypatch):
    """row_params = ONE token_sample_rows call that carries the out_* rows; without it the calls made before (tests/test_sampling_cpu.py
    pins those in full: here one of each kind shows that the new argument's default leaves them alone)."""
    from cover_vla_amd import ops
    calls = []
    tok, lgt, kept, lpv = torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(2)
    rp = (torch.ones(2), torch.zeros(2, dtype=torch.int32), torch.ones(2))

    def rows(logits, lo, hi, uniform, temperature, top_k=None, top_p=None, out_tok=None, out_logit=None, out_kept=None, out_logprob=None):
        calls.append(("token_sample_rows", lo, hi, uniform, temperature, top_k, top_p, out_tok, out_logit, out_kept, out_logprob))
        return tok, lgt, kept

    def select(logits, lo, hi, uniform=None, temperature=1.0, out_tok=None, out_logit=None):
        calls.append(("token_select", lo, hi, uniform is None, temperature))
        return tok, lgt

    def sample(logits, lo, hi, uniform, temperature=1.0, top_k=0, top_p=1.0, **outs):
        calls.append(("token_sample", lo, hi, temperature, top_k, top_p))
        return tok, lgt, kept

    def logprob(logits, lo, hi, tokens, temperature=1.0, top_k=0, top_p=1.0, out=None, out_kept=None):
        calls.append(("token_logprob", lo, hi, temperature, top_k, top_p))
        return out

    fakes = dict(token_sample_rows=rows, token_select=select, token_sample=sample, token_logprob=logprob)
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if fn.__module__ == ops.__name__ and not name.startswith("_") and name != "pick_token":
            monkeypatch.setattr(ops, name, fakes.get(name) or (lambda *a, _n=name, **k: calls.append(_n)))
    lg, u = torch.zeros(2, 16), torch.zeros(2)
    for lo, hi in ((0, 16), (3, 11)):
        for lp in (None, lpv):
            for filt in (None, (5, 0.5)):                    # temperature and filt are unused with row_params
                del calls[:]
                r = ops.pick_token(lg, lo, hi, u, 0.7, filt, out_tok=tok, out_logit=lgt, out_kept=kept, out_logprob=lp, row_params=rp)
                assert r[0] is tok and r[1] is lgt and r[2] is kept
                assert len(calls) == 1 and calls[0][:4] == ("token_sample_rows", lo, hi, u)
                assert all(a is b for a, b in zip(calls[0][4:], rp + (tok, lgt, kept, lp)))
    # no row_params: the calls made before
    del calls[:]
    ops.pick_token(lg, 0, 16, None, 0.7, (5, 0.5), out_logprob=lpv)
    assert calls == [("token_select", 0, 16, True, 1.0), ("token_logprob", 0, 16, 1.0, 0, 1.0)]
    del calls[:]
    ops.pick_token(lg, 0, 16, u, 0.7, None, out_logprob=lpv, row_params=None)
    assert calls == [("token_select", 0, 16, False, 0.7), ("token_logprob", 0, 16, 0.7, 0, 1.0)]
    del calls[:]
    ops.pick_token(lg, 0, 16, u, 0.7, (5, 0.5), out_logprob=lpv)
    assert calls == [("token_sample", 0, 16, 0.7, 5, 0.5)]


def test_models_accept_per_row_parameters_in_their_signatures():
    from cover_vla_amd import ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTTokens
    assert inspect.signature(ops.pick_token).parameters["row_params"].default is None
    for fn in (OpenVLA.sample, PI0FASTTokens.generate_tokens):          # the scalar defaults stay
        p = inspect.signature(fn).parameters
        assert (p["temperature"].default, p["top_k"].default, p["top_p"].default) == (1.0, 0, 1.0)
        assert "length-" in fn.__doc__ and "token_sample_rows" in fn.__doc__
    cfg = PI0FASTConfig(temperature=[0.0, 1.0], top_k=[0, 5], top_p=[1.0, 0.9])
    assert cfg.temperature == [0.0, 1.0]
    assert ops.is_per_row([1.0]) and ops.is_per_row(np.ones(2)) and ops.is_per_row(torch.ones(2))
    assert not ops.is_per_row(1.0) and not ops.is_per_row(np.float32(1)) and not ops.is_per_row(torch.tensor(1.0))


def test_row_param_tensors_validates_every_value_and_casts():
    """What the models hand to pick_token(row_params=): fp32 / int32 / fp32 [rows] from scalars and tensors of any numeric dtype, every
    value checked on the host -- a pick that feeds an embedding gather must never be the -1 of an invalid row."""
    from cover_vla_amd import _lib as L, ops
    T, k, p = ops.row_param_tensors(3, torch.tensor([0.0, 0.7, 1.3], dtype=torch.float64), torch.tensor([0, 50, 0]), 0.9, "cpu")
    assert (T.dtype, k.dtype, p.dtype) == (torch.float32, torch.int32, torch.float32)
    assert T.tolist() == pytest.approx([0.0, 0.7, 1.3]) and k.tolist() == [0, 50, 0] and p.tolist() == pytest.approx([0.9] * 3)
    T, k, p = ops.row_param_tensors(2, torch.tensor(0.5), [1, 2], np.float32(1.0), "cpu")      # a 0-dim tensor is a scalar
    assert T.tolist() == [0.5, 0.5] and k.tolist() == [1, 2] and p.tolist() == [1.0, 1.0]
    for bad in ((torch.tensor([1.0, float("nan")]), 0, 1.0), (torch.tensor([1.0, -1.0]), 0, 1.0), (1.0, torch.tensor([0, -1]), 1.0),
                (1.0, 0, torch.tensor([1.0, 0.0])), (1.0, 0, torch.tensor([1.0, float("nan")])), (torch.ones(3), 0, 1.0),
                (float("inf"), [0, 0], 1.0), (1.0, torch.tensor([0.5, 1.0]), 1.0)):
        with pytest.raises(L.CoverError):
            ops.row_param_tensors(2, *bad, "cpu")

