"""The proposal log-density prior without a GPU: the case table of tests/proposal_prior_ref.py really holds the conditions it names,
host.vote_log_shares against a float64 restatement, the margin by which the omitted normalisation term can bias a group (the fitted
rows' mean of acc is the same constant in every group), and the binding, host.ProposalPrior, vote_log_shares and the ops wrappers
reject bad arguments before anything is launched."""
import ctypes as C
import inspect
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from tests import proposal_prior_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _each(variant):
    cs = PR.cases(variants=(variant,))
    assert cs
    return [(c, PR.make_inputs(c), PR.case_reference(c)) for c in cs]


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_the_listed_shapes_and_variants():
    cs = PR.cases()
    assert len({PR.case_id(c) for c in cs}) == len(cs)
    for form in ("tokens", "actions"):
        assert {c["shape"] for c in cs if c["form"] == form} == set(PR.SHAPES)
        for s in PR.SHAPES:
            got = {c["variant"] for c in cs if c["form"] == form and c["shape"] == s}
            assert got == {v for v in PR.VARIANTS if PR.feasible(form, s, v)} and {"spread", "noshare"} <= got
    assert {c["variant"] for c in cs if c["form"] == "tokens"} == set(PR.VARIANTS) - {"nan"}
    assert {c["variant"] for c in cs if c["form"] == "actions"} == set(PR.VARIANTS) - {"outside"}
    shapes = PR.SHAPES
    assert any(n == 1 and S == 1 for G, n, S, h in shapes) and any(n == 1 and S > 1 for G, n, S, h in shapes)
    assert any(n == 2 for G, n, S, h in shapes) and (2, 5, 8, 1) in shapes
    assert any(n == S and n > 1 for G, n, S, h in shapes) and any(S > 256 and G == 3 for G, n, S, h in shapes)
    assert PR.STRIDED in shapes and PR.STRIDED[3] == 4


def test_one_fitted_row_puts_the_floor_on_every_dim():
    seen = 0
    for c, inp, r in _each("spread"):
        G, n, S, h = c["shape"]
        if n == 1:
            assert (r["sd_raw"] == 0).all() and (r["sd"] == np.float32(inp["sd_floor"])).all()
            assert (r["acc"][:, 0] == 0).all()                      # the fitted row sits on its own mean
            seen += 1
    assert seen >= 2


def test_variant_floor_is_active_on_some_dims_only():
    for c, inp, r in _each("floor"):
        active = r["sd_raw"] < np.float32(inp["sd_floor"])
        assert active.any() and not active.all()
        assert (r["sd"][active] == np.float32(inp["sd_floor"])).all() and (r["sd"][~active] == r["sd_raw"][~active]).all()
        assert np.isfinite(r["prior"]).all()


def test_variant_tie_splits_the_votes_evenly():
    for c, inp, r in _each("tie"):
        G, n, S, h = c["shape"]
        assert (r["votes"][..., 0] == r["votes"][..., 1]).all() and (r["votes"].sum(-1) == n).all()
        assert (r["counts"] == n // 2).all()                        # either class of any row has half the votes


def test_variant_zero_has_rows_whose_class_nobody_voted_for():
    for c, inp, r in _each("zero"):
        G, n, S, h = c["shape"]
        assert inp["log_share"][0] == -np.inf and np.isfinite(inp["log_share"][1:]).all()
        none = (r["counts"] == 0).any(axis=-1)                      # [G, S]
        assert none.any() and not none[:, :n].any() and not none.all()
        p = r["prior"].reshape(G, S)
        assert (p[none] == -np.inf).all() and np.isfinite(p[~none]).all()


def test_variant_outside_engages_the_clamp():
    for c, inp, r in _each("outside"):
        b = PR.TOK_VOCAB - inp["tokens"] - 1
        assert (b < 0).any() and (b > AR.N_CENTERS - 1).any()
        x = AR.token_values(inp["tokens"], inp["centers"], PR.TOK_VOCAB)
        assert (x[b < 0] == inp["centers"][0]).all() and (x[b > AR.N_CENTERS - 1] == inp["centers"][-1]).all()
        assert np.isfinite(r["prior"]).all()


def test_variant_nan_reaches_its_own_row_only():
    for c, inp, r in _each("nan"):
        G, n, S, h = c["shape"]
        rows = inp["nan_rows"]
        assert len(rows) >= 1 and (rows % S >= n).all()
        bad = np.isnan(inp["actions"]).any(axis=(1, 2))
        assert np.array_equal(np.flatnonzero(bad), np.sort(rows))
        assert np.array_equal(np.isnan(r["prior"]), bad)
        clean = dict(inp, actions=np.where(np.isnan(inp["actions"]), np.float32(0), inp["actions"]))
        r0 = PR.reference_of(clean, "actions", h)
        assert np.array_equal(r0["prior"][~bad].view(np.int32), r["prior"][~bad].view(np.int32))
        for k in ("mean", "sd", "votes"):
            assert np.array_equal(r0[k], r[k])


def test_variant_noshare_has_no_gripper_term():
    for c, inp, r in _each("noshare"):
        assert inp["log_share"] is None and inp["sigma"] == 1.0
        assert np.array_equal(r["prior"].view(np.int32), (np.float32(-0.5) * r["acc"]).reshape(-1).view(np.int32))


def test_the_gripper_term_is_added_step_by_step():
    for c, inp, r in _each("spread"):
        G, n, S, h = c["shape"]
        ls = inp["log_share"]
        assert ls.shape == (n + 1,) and np.isfinite(ls).all()
        p = (np.float32(-0.5) * r["acc"]).astype(np.float32)
        for t in range(h):
            p = (p + ls[r["counts"][:, :, t]]).astype(np.float32)
        assert np.array_equal(p.reshape(-1).view(np.int32), r["prior"].view(np.int32))
        assert (r["counts"] >= 0).all() and (r["counts"] <= n).all()


# ------------------------------------------------------------------------------------------------ the reference against float64
def test_prior_agrees_with_float64():
    """-0.5 * sum z^2 in float64 from the float64 fit, floor inactive: fp32 holds it to 1e-4 relative (6 h terms of a few roundings each,
    on fits whose own relative error is a few 1e-7 amplified by |x - mean| / sd, a handful here)."""
    checked = 0
    for c, inp, r in _each("noshare"):
        G, n, S, h = c["shape"]
        if n < 2 or (r["sd_raw"] < np.float32(inp["sd_floor"])).any():
            continue
        x = PR.values_of(inp, c["form"], h).reshape(G, S, h, 7)[..., :6].astype(np.float64)
        mean, sd = x[:, :n].mean(axis=1), x[:, :n].std(axis=1, ddof=1)
        want = -0.5 * (((x - mean[:, None]) / sd[:, None]) ** 2).sum(axis=(2, 3))
        assert (np.abs(r["prior"].reshape(G, S) - want) <= 1e-4 * np.abs(want) + 1e-6).all(), PR.case_id(c)
        checked += want.size
    assert checked > 1000


def test_fitted_rows_mean_of_acc_is_the_same_constant_in_every_group():
    """What leaving out -sum log s costs the group stage of cover_prior_select: with the floor inactive the fitted rows' acc average to
    6 h (n - 1) / n (sigma = 1; / sigma^2 otherwise) in every group, whatever its spread, to 1e-5 relative."""
    unit_sigma = 0
    for c in PR.cases():
        inp, r = PR.make_inputs(c), PR.case_reference(c)
        G, n, S, h = c["shape"]
        if n < 2 or (r["sd_raw"] < np.float32(inp["sd_floor"])).any():
            continue
        got = r["acc"][:, :n].astype(np.float64).mean(axis=1)
        want = 6.0 * h * (n - 1) / n / float(np.float32(inp["sigma"])) ** 2
        assert (np.abs(got - want) <= 1e-5 * want).all(), (PR.case_id(c), got, want)
        unit_sigma += inp["sigma"] == 1.0
    assert unit_sigma >= 6


# ------------------------------------------------------------------------------------------------ host
def test_vote_log_shares_match_float64():
    from cover_vla_amd import host
    for n in (1, 2, 5, 64, 4096):
        for alpha in (0.0, 0.5, 1.0, 3):
            got = host.vote_log_shares(n, alpha)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (n + 1,)
            want = [np.float32(math.log((c + alpha) / (n + 2.0 * alpha))) if c + alpha > 0 else np.float32(-np.inf) for c in range(n + 1)]
            assert np.array_equal(got.view(np.int32), np.array(want, dtype=np.float32).view(np.int32)), (n, alpha)
            assert np.array_equal(got.view(np.int32), PR.log_shares(n, alpha).view(np.int32))
            assert (np.diff(got) > 0).all() and got[-1] <= 0
    assert host.vote_log_shares(4, 0.0)[0] == -np.inf and host.vote_log_shares(4, 0.0)[4] == 0.0
    assert host.vote_log_shares(np.int64(3), np.float32(0.5)).shape == (4,)
    for bad in ((0, 1.0), (-1, 1.0), (4097, 1.0), (2.0, 1.0), (True, 1.0), (3, -0.1), (3, float("nan")), (3, float("inf")), (3, "1"), (3, None)):
        with pytest.raises(ValueError):
            host.vote_log_shares(*bad)


def test_host_proposal_prior_checks_its_values():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    ls = torch.from_numpy(host.vote_log_shares(3, 1.0))
    p = host.ProposalPrior(3, 0.8, 1e-3)
    assert tuple(p) == (3, 0.8, 1e-3, None) and p.samples_per_prompt == 3 and p.sigma == 0.8 and p.sd_floor == 1e-3 and p.log_share is None
    assert host.ProposalPrior(3, 1, 0.01, log_share=ls).log_share is ls
    bad = [dict(samples_per_prompt=0), dict(samples_per_prompt=4097), dict(samples_per_prompt=2.0), dict(samples_per_prompt=True),
           dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma="1"), dict(sigma=1e39), dict(sigma=1e-50),
           dict(sd_floor=0.0), dict(sd_floor=-0.1), dict(sd_floor=float("nan")), dict(sd_floor=float("inf")), dict(sd_floor=None),
           dict(sigma=1e-30, sd_floor=1e-30),
           dict(log_share=ls.numpy()), dict(log_share=ls.double()), dict(log_share=ls[:3]), dict(log_share=ls[None]),
           dict(log_share=torch.zeros(5))]
    for over in bad:
        kw = dict(samples_per_prompt=3, sigma=0.8, sd_floor=1e-3)
        kw.update(over)
        with pytest.raises(CoverError):
            host.ProposalPrior(**kw)
    with pytest.raises(TypeError):
        host.ProposalPrior(3)                                       # sigma and sd_floor have no defaults


def test_wrappers_validate_without_a_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    G, n, S, h = 2, 3, 7, 2
    tok = torch.full((G * S, 7 * h), PR.TOK_VOCAB - 100, dtype=torch.int64)
    act = torch.zeros(G * S, h, 7)
    cen = torch.from_numpy(AR.openvla_centers())
    ls = torch.zeros(n + 1)
    T = lambda **kw: ops.proposal_prior_tokens(kw.pop("tokens", tok), kw.pop("S", S), kw.pop("n", n), kw.pop("centers", cen), PR.TOK_VOCAB,
                                               **{"steps": h, "sigma": 0.8, "sd_floor": 1e-3, **kw})
    A = lambda **kw: ops.proposal_prior_actions(kw.pop("actions", act), kw.pop("S", S), kw.pop("n", n), **{"sigma": 0.8, "sd_floor": 1e-3, **kw})
    common = [dict(n=0), dict(n=-1), dict(n=8), dict(S=0), dict(S=4), dict(S=14, n=15), dict(S=4097), dict(n=2.0), dict(S=7.0), dict(n=True),
              dict(sigma=0.0), dict(sigma=-0.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=1e39), dict(sigma=1e-50),
              dict(sigma="1"), dict(sigma=None),
              dict(sd_floor=0.0), dict(sd_floor=-1e-3), dict(sd_floor=float("nan")), dict(sd_floor=float("inf")), dict(sd_floor=None),
              dict(sigma=1e-30, sd_floor=1e-30),
              dict(log_share=ls.numpy()), dict(log_share=ls.double()), dict(log_share=torch.zeros(n)), dict(log_share=torch.zeros(n + 2)),
              dict(log_share=ls[None]), dict(log_share=torch.zeros(2 * n + 2)[::2]),
              dict(out=torch.zeros(G * S, dtype=torch.float64)), dict(out=torch.zeros(G * S + 1)), dict(out=torch.zeros(G * S, 1)),
              dict(out=torch.zeros(2 * G * S)[::2]), dict(out=np.zeros(G * S, dtype=np.float32))]
    for kw in common:
        with pytest.raises(CoverError):
            T(**dict(kw))
        with pytest.raises(CoverError):
            A(**dict(kw))
    for kw in (dict(tokens=tok.int()), dict(tokens=tok.numpy()), dict(tokens=tok[0]), dict(tokens=tok[:, :13]), dict(tokens=tok.t().contiguous().t()),
               dict(steps=0), dict(steps=3), dict(centers=cen.double()), dict(centers=cen[None]), dict(centers=cen[:0]), dict(centers=cen.numpy()),
               dict(tokens=torch.zeros(65 * 7, dtype=torch.int64).expand(G * S, 65 * 7), steps=65),
               dict(tokens=torch.zeros(G * S, 65 * 7, dtype=torch.int64), steps=65)):
        with pytest.raises(CoverError):
            T(**kw)
    for kw in (dict(actions=act.double()), dict(actions=act.numpy()), dict(actions=act[0]), dict(actions=act[..., :6]),
               dict(actions=torch.zeros(G * S, h, 14)[..., ::2]), dict(actions=torch.zeros(G * S, 65, 7))):
        with pytest.raises(CoverError):
            A(**kw)
    with pytest.raises(TypeError):                                  # sigma and sd_floor have no defaults
        ops.proposal_prior_tokens(tok, S, n, cen, PR.TOK_VOCAB, steps=h, sigma=1.0)
    with pytest.raises(TypeError):
        ops.proposal_prior_actions(act, S, n, sd_floor=1.0)
    # valid arguments on host tensors: there is no CPU path
    for call in (T, A):
        with pytest.raises(CoverError, match="device"):
            call()
        with pytest.raises(CoverError, match="device"):             # S == n_fit, every option
            call(S=n, n=n, **({"tokens": tok[:G * n]} if call is T else {"actions": act[:G * n]}), log_share=ls, stats=True, out=torch.zeros(G * n))
    with pytest.raises(CoverError, match="device"):
        ops.proposal_prior_actions(torch.zeros(G * S, h + 6, 32)[:, :h, :7], S, n, sigma=1.0, sd_floor=0.5)   # the strided view is accepted as it is
    with pytest.raises(CoverError, match="device"):
        ops.proposal_prior_tokens(torch.zeros(G * S, 7 * h + 3, dtype=torch.int64)[:, :7 * h], S, n, cen, PR.TOK_VOCAB, steps=h, sigma=1.0, sd_floor=0.5)


def test_signatures_have_no_default_sigma_or_floor():
    from cover_vla_amd import host, ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0 import PI0Policy
    E, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(ops.proposal_prior_tokens).parameters
    assert list(p)[:5] == ["tokens", "group_rows", "n_fit", "centers", "tok_vocab"]
    assert [(k, p[k].default) for k in list(p)[5:]] == [("steps", 1), ("sigma", E), ("sd_floor", E), ("log_share", None), ("out", None), ("stats", False)]
    assert all(p[k].kind is KW for k in list(p)[5:])
    p = inspect.signature(ops.proposal_prior_actions).parameters
    assert list(p)[:3] == ["actions", "group_rows", "n_fit"]
    assert [(k, p[k].default) for k in list(p)[3:]] == [("sigma", E), ("sd_floor", E), ("log_share", None), ("out", None), ("stats", False)]
    assert all(p[k].kind is KW for k in list(p)[3:])
    p = inspect.signature(OpenVLA.proposal_prior).parameters
    assert list(p) == ["self", "tokens", "group_rows", "n_fit", "sigma", "sd_floor", "log_share"]
    assert p["sigma"].default is E and p["sd_floor"].default is E and p["log_share"].default is None and p["sigma"].kind is KW
    p = inspect.signature(PI0Policy.select_action).parameters
    assert list(p) == ["self", "batch", "noise", "noise_std", "augment"]    # the pi0 option is the attribute PI0Policy.proposal_prior, no keyword
    assert "self.proposal_prior" in PI0Policy.select_action.__doc__ and "last_proposal_prior" in PI0Policy.select_action.__doc__
    assert host.ProposalPrior._fields == ("samples_per_prompt", "sigma", "sd_floor", "log_share")
    p = inspect.signature(host.vote_log_shares).parameters
    assert list(p) == ["n_fit", "alpha"] and p["alpha"].default is E
    assert "unnormalised" in ops.proposal_prior_tokens.__doc__.lower() and "NaN" in ops.proposal_prior_actions.__doc__


# ------------------------------------------------------------------------------------------------ binding
_FIELDS = ("src", "n_stride", "t_stride", "centers", "log_share", "n_centers", "tok_vocab", "G", "group_rows", "n_fit", "h", "sigma", "sd_floor",
           "prior_out", "mean_out", "sd_out", "votes_out")
_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cover_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(cover_proposal_prior_args, f));
int main(void) {
    printf("sizeof %zu\n", sizeof(cover_proposal_prior_args));
    """ + " ".join(f"F({f})" for f in _FIELDS) + r"""
    return 0;
}
"""


def test_struct_mirror_matches_a_compiled_probe_of_the_header(tmp_path):
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_proposal_prior_args"] is L.ProposalPriorArgs
    for sym in ("cover_proposal_prior_tokens", "cover_proposal_prior_actions"):
        assert L.SYMBOLS[sym] == (C.c_int, [C.POINTER(L.ProposalPriorArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_proposal_prior_tokens(const cover_proposal_prior_args* args, void* stream);" in hdr
    assert "int cover_proposal_prior_actions(const cover_proposal_prior_args* args, void* stream);" in hdr
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed to probe include/cover_hip.h"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("sizeof")) == C.sizeof(L.ProposalPriorArgs) == 104
    assert list(out) == [f[0] for f in L.ProposalPriorArgs._fields_] == list(_FIELDS)
    for name, _ in L.ProposalPriorArgs._fields_:
        assert int(out[name]) == getattr(L.ProposalPriorArgs, name).offset, name
    assert C.sizeof(L.AugmentArgs) == 112                           # the shared-fit refactor left the augment ABI alone
    if os.path.exists(L.LIB_PATH):                                  # cover_sizeof is host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_proposal_prior_tokens") and hasattr(h, "cover_proposal_prior_actions")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_proposal_prior_args") == C.sizeof(L.ProposalPriorArgs)
        assert h.cover_sizeof(b"cover_augment_args") == 112


def test_the_fit_is_stated_once():
    """augment.hip and proposal_prior.hip take the fit from one header; neither restates it."""
    csrc = os.path.join(ROOT, "cover_vla_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("augment.hip", "proposal_prior.hip", "augment_fit.h")}
    assert "sqrtf(var)" in text["augment_fit.h"] and "#pragma clang fp contract(off)" in text["augment_fit.h"]
    for f in ("augment.hip", "proposal_prior.hip"):
        assert '#include "augment_fit.h"' in text[f] and "augment_group_stats<T>(" in text[f] and "sqrtf" not in text[f]
        assert "#pragma clang fp contract(off)" in text[f] and "tok_vocab -" not in text[f]
    rows = open(os.path.join(csrc, "chunk_rows.h")).read()                 # the rows the fit reads: one token rule, in the row source
    assert '#include "chunk_rows.h"' in text["augment_fit.h"] and "tok_vocab -" not in text["augment_fit.h"]
    assert rows.count("tok_vocab -") == 1 and rows.count("float aug_value(") == 2 and "#pragma clang fp contract(off)" in rows
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "proposal_prior.hip" in make and " chunk_rows.h " in make
