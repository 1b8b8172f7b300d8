"""Device-side top-k / top-p sampling, the part that needs no GPU: the float64 reference against Hugging Face's warpers, the
fairness of the GPU tests' inputs (share of decided rows, from the same seeds), the binding's struct mirror and argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_semantics_on_constructed_rows():
    l = np.array([0.0, 3.0, 1.0, 3.0, 2.0, -1.0, 3.0], dtype=np.float32)
    # top-k keeps everything tied with the k-th value
    r = R.reference_row(l, 0.0, 1.0, 2, 1.0)
    assert r["kept"] == 3 and r["keep"].tolist() == [False, True, False, True, False, False, True] and r["token"] == 1
    assert R.reference_row(l, np.nextafter(np.float32(1), np.float32(0)), 1.0, 2, 1.0)["token"] == 6
    # top-p: equal weights by ascending index, shortest prefix that reaches the target, at least one token
    e3 = np.exp(3.0)
    total = 3 * e3 + np.exp(2.0) + np.exp(1.0) + 1.0 + np.exp(-1.0)
    r = R.reference_row(l, 0.5, 1.0, 0, 1.5 * e3 / total)
    assert r["keep"].tolist() == [False, True, False, True, False, False, False] and r["kept"] == 2
    assert R.reference_row(l, 0.5, 1.0, 0, 1e-6)["keep"].tolist() == [False, True, False, False, False, False, False]
    assert R.reference_row(l, 0.5, 1.0, 0, 1.0)["kept"] == 7 and R.reference_row(l, 0.5, 1.0, 7, 1.0)["kept"] == 7
    # the pick: first kept index whose running sum exceeds u x mass
    w = np.exp(l.astype(np.float64) - 3.0)
    cs = np.cumsum(w) / w.sum()
    for u in (0.0, 0.1, 0.33, 0.5, 0.77, 0.999):
        assert R.reference_row(l, u, 1.0, 0, 1.0)["token"] == int(np.argmax(cs > np.float32(u)))


def test_reference_kept_set_matches_hf_warpers():
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper on rows without ties: the same kept set."""
    tf = pytest.importorskip("transformers")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x, u = R.lm_like_rows(77, 24, 4096, 0, 4096)
    free = [r for r in range(24) if np.unique(x[r].numpy()).size == 4096]          # rows without ties
    assert len(free) >= 12
    x, u = x[free[:12]], u[free[:12]]
    n_checked = 0
    for T, k, p in [(1.0, 50, 1.0), (1.0, 0, 0.9), (0.7, 64, 0.95), (1.3, 20, 0.8), (1.5, 8, 1.0), (1.0, 0, 1.0)]:
        s = x.double()
        if T != 1.0:
            s = TemperatureLogitsWarper(float(np.float32(T)))(None, s)
        if k > 0:
            s = TopKLogitsWarper(top_k=k)(None, s)
        if p < 1.0:
            s = TopPLogitsWarper(top_p=float(np.float32(p)))(None, s)
        hf_keep = torch.isfinite(s).numpy()
        for r, ref in enumerate(R.reference_rows(x, 0, 4096, u, T, k, p)):
            if ref["cut_decided"]:
                assert np.array_equal(hf_keep[r], ref["keep"]), (T, k, p, r)
                n_checked += 1
    assert n_checked >= 60


def _undecided(kind, ci, ri):
    if kind == "wide":
        T, k, p = R.WIDE_CASES[ci]
        lo, hi = R.WIDE_RANGES[ri]
        x, u = R.lm_like_rows(R.case_seed(kind, ci, ri), R.ROWS, R.WIDE_V, lo, hi)
    else:
        T, k, p = R.NARROW_CASES[ci]
        lo, hi = R.NARROW_LO, R.NARROW_HI
        x, u = R.lm_like_rows(R.case_seed(kind, ci), R.ROWS, R.NARROW_LD, lo, hi)
    refs = R.reference_rows(x, lo, hi, u, T, k, p)
    und = sum(not (r["pick_decided"] and r["cut_decided"]) for r in refs)
    print(f"{kind} (T={T}, top_k={k}, top_p={p}) [{lo}, {hi}): undecided {und} of {len(refs)}, "
          f"median kept {int(np.median([r['kept'] for r in refs]))}")
    return und, refs


@pytest.mark.parametrize("ci", range(len(R.WIDE_CASES)))
@pytest.mark.parametrize("ri", range(len(R.WIDE_RANGES)))
def test_wide_inputs_are_fair(ci, ri):
    """The inputs of the GPU parity test (same seeds) leave at most 10 % of a case's rows undecided at the derived DELTA."""
    und, refs = _undecided("wide", ci, ri)
    assert und <= R.CAP * len(refs)
    T, k, p = R.WIDE_CASES[ci]
    if 0 < k and p >= 1.0:
        assert all(r["kept"] == k for r in refs)                     # continuous data: no ties at the k-th value


@pytest.mark.parametrize("ci", range(len(R.NARROW_CASES)))
def test_narrow_inputs_are_fair(ci):
    und, refs = _undecided("narrow", ci, 0)
    assert und <= R.CAP * len(refs)


def test_delta_is_below_the_issue_ceiling():
    assert R.DELTA <= 1e-4


def test_token_sample_struct_mirror_and_symbol():
    from cover_vla_amd import _lib as L
    assert "cover_token_sample" in L.SYMBOLS and L._STRUCTS["cover_token_sample_args"] is L.TokenSampleArgs
    names = [f[0] for f in L.TokenSampleArgs._fields_]
    assert names == ["logits", "ld", "rows", "lo", "hi", "uniform", "temperature", "top_k", "top_p", "token_out", "logit_out", "kept_out"]
    assert C.sizeof(L.TokenSampleArgs) == 80
    # the header declares the same fields in the same order
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    body = hdr[hdr.index("typedef struct cover_token_sample_args {"):hdr.index("} cover_token_sample_args;")]
    pos = [body.index(n) for n in ["logits;", " ld;", " rows;", " lo, hi;", "uniform;", "temperature;", "top_k;", "top_p;", "token_out;",
                                   "logit_out;", "kept_out;"]]
    assert pos == sorted(pos)
    assert "int cover_token_sample(const cover_token_sample_args* args, void* stream);" in hdr
    # the built library exports the symbol and agrees on the struct's size (no GPU call: cover_sizeof is host code)
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_token_sample")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_token_sample_args") == C.sizeof(L.TokenSampleArgs)
        assert h.cover_sizeof(b"cover_token_select_args") == C.sizeof(L.TokenSelectArgs)


def test_token_sample_argument_validation_needs_no_device():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    lg = torch.zeros(2, 16)
    u = torch.zeros(2)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=-0.5), dict(top_k=-1)):
        with pytest.raises(CoverError):
            ops.token_sample(lg, 0, 16, u, **kw)
    with pytest.raises(CoverError):
        ops.token_sample(lg, 8, 8, u)
    with pytest.raises(CoverError):
        ops.token_sample(lg, 0, 16, None)
    with pytest.raises(CoverError):           # valid arguments, host tensors: there is no CPU path
        ops.token_sample(lg, 0, 16, u)


def test_generate_tokens_and_sample_signatures():
    import inspect
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTTokens
    p = inspect.signature(PI0FASTTokens.generate_tokens).parameters
    assert p["uniforms"].default is None and p["temperature"].default == 1.0 and p["top_k"].default == 0 and p["top_p"].default == 1.0
    p = inspect.signature(OpenVLA.sample).parameters
    assert p["top_k"].default == 0 and p["top_p"].default == 1.0
    cfg = PI0FASTConfig()
    assert (cfg.temperature, cfg.top_k, cfg.top_p, cfg.sample_seed) == (1.0, 0, 1.0, None)


def test_pick_token_dispatch(monkeypatch):
    """ops.pick_token issues the launches its callers issued, with their arguments and nothing else: greedy = token_select, then
    token_logprob at temperature 1 unfiltered whatever temperature was passed; sampled unfiltered = token_select, then token_logprob
    at the same temperature; sampled filtered = ONE token_sample that carries out_kept / out_logprob."""
    import inspect
    from cover_vla_amd import ops
    calls = []
    tok, lgt, kept, lpv = torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(2, dtype=torch.int32), torch.zeros(2)

    def rec(name, uniform, temperature, top_k, top_p, **outs):
        return (name, uniform is None, temperature, top_k, top_p, tuple(sorted(k for k, v in outs.items() if v is not None)))

    def select(logits, lo, hi, uniform=None, temperature=1.0, out_tok=None, out_logit=None):
        calls.append((lo, hi) + rec("token_select", uniform, temperature, None, None, out_tok=out_tok, out_logit=out_logit))
        return tok, lgt

    def sample(logits, lo, hi, uniform, temperature=1.0, top_k=0, top_p=1.0, out_tok=None, out_logit=None, out_kept=None, out_logprob=None):
        calls.append((lo, hi) + rec("token_sample", uniform, temperature, top_k, top_p, out_tok=out_tok, out_logit=out_logit, out_kept=out_kept,
                                    out_logprob=out_logprob))
        return tok, lgt, kept

    def logprob(logits, lo, hi, tokens, temperature=1.0, top_k=0, top_p=1.0, out=None, out_kept=None):
        assert tokens is tok                                      # the pick that was just made
        calls.append((lo, hi) + rec("token_logprob", None, temperature, top_k, top_p, out=out, out_kept=out_kept))
        return out

    fakes = dict(token_select=select, token_sample=sample, token_logprob=logprob)
    for name, fn in inspect.getmembers(ops, inspect.isfunction):
        if fn.__module__ == ops.__name__ and not name.startswith("_") and name != "pick_token":
            monkeypatch.setattr(ops, name, fakes.get(name) or (lambda *a, _n=name, **k: calls.append(_n)))
    lg, u = torch.zeros(2, 16), torch.zeros(2)
    sel = lambda lo, hi, greedy, T, *outs: (lo, hi, "token_select", greedy, T, None, None, outs)
    lpc = lambda lo, hi, T: (lo, hi, "token_logprob", True, T, 0, 1.0, ("out",))
    for lo, hi in ((0, 16), (3, 11)):
        for with_lp in (False, True):
            lp = lpv if with_lp else None
            # greedy: temperature and filt are ignored, the log-probability runs at temperature 1
            for filt in (None, (5, 0.5)):
                del calls[:]
                r = ops.pick_token(lg, lo, hi, None, 0.7, filt, out_tok=tok, out_logit=lgt, out_kept=kept, out_logprob=lp)
                assert r[0] is tok and r[1] is lgt and r[2] is None
                assert calls == [sel(lo, hi, True, 1.0, "out_logit", "out_tok")] + ([lpc(lo, hi, 1.0)] if with_lp else [])
            # sampled unfiltered
            del calls[:]
            r = ops.pick_token(lg, lo, hi, u, 0.7, None, out_logit=lgt, out_kept=kept, out_logprob=lp)
            assert r[0] is tok and r[1] is lgt and r[2] is None
            assert calls == [sel(lo, hi, False, 0.7, "out_logit")] + ([lpc(lo, hi, 0.7)] if with_lp else [])
            # sampled filtered: one call, also with filters that filter nothing
            for k, p in ((5, 0.5), (0, 1.0)):
                del calls[:]
                r = ops.pick_token(lg, lo, hi, u, 0.7, (k, p), out_tok=tok, out_kept=kept, out_logprob=lp)
                assert r[0] is tok and r[1] is lgt and r[2] is kept
                assert calls == [(lo, hi, "token_sample", False, 0.7, k, p, ("out_kept",) + (("out_logprob",) if with_lp else ()) + ("out_tok",))]
    del calls[:]
    assert ops.pick_token(lg, 0, 16)[2] is None and calls == [sel(0, 16, True, 1.0)]      # the defaults: greedy, fresh tensors
