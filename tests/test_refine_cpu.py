"""Verifier-guided refinement without a GPU: the reference of tests/refine_ref.py ranks as it says and is augment_ref on its own elites, the
case table holds the conditions it names and its feasibility rule stays inside its cap, the binding mirrors the header, the ops wrappers
reject bad arguments before anything is launched, and EfficientEnsembleMerged.score_refined is the composition it documents."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import augment_ref as AR
from tests import refine_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(c, inp):
    return inp[c["form"]]


# ------------------------------------------------------------------------------------------------ the case table
def test_feasibility_rule_stays_inside_its_cap():
    g = RR.grid()
    dropped = [x for x in g if not RR.feasible(*x)]
    assert len(g) == (2 * len(RR.SHAPES) + len(RR.FLOAT_ONLY)) * len(RR.VARIANTS)
    assert len(dropped) <= RR.MAX_INFEASIBLE * len(g) and RR.MAX_INFEASIBLE == 0.25, (len(dropped), len(g))
    cs = RR.cases()
    assert len(cs) == len(g) - len(dropped) and len({RR.case_id(c) for c in cs}) == len(cs)
    for form in ("tokens", "actions"):
        assert {c["shape"] for c in cs if c["form"] == form} == set(RR.SHAPES) | (set(RR.FLOAT_ONLY) if form == "actions" else set())
        assert {c["variant"] for c in cs if c["form"] == form} == set(RR.VARIANTS)
    for s in RR.SHAPES + RR.FLOAT_ONLY:                               # every shape from S = 5 on runs every variant
        if s[1] >= 5:
            assert all(RR.feasible(f, s, v) for f in ("tokens", "actions") for v in RR.VARIANTS)
    assert RR.SHAPES == [(1, 1, 1, 1, 1), (1, 2, 1, 3, 1), (2, 5, 2, 32, 1), (3, 37, 4, 65, 2), (2, 64, 8, 56, 4), (1, 300, 5, 7, 2),
                         (1, 4096, 16, 4, 1)]
    assert (2, 5, 5, 3, 50) in RR.FLOAT_ONLY and RR.STRIDED in RR.FLOAT_ONLY
    assert any(RR.token_row_stride(s) > 7 * s[4] for s in RR.SHAPES) and any(RR.token_row_stride(s) == 7 * s[4] for s in RR.SHAPES)


def _each(variant):
    cs = RR.cases(variants=(variant,))
    assert cs
    return [(c, RR.make_inputs(c), RR.case_reference(c)) for c in cs]


def test_distinct_agrees_with_a_stable_argsort():
    for variant in ("distinct", "reverse", "k0"):
        for c, inp, r in _each(variant):
            G, S, m, K, h = c["shape"]
            sc = inp["scores"].reshape(G, S)
            assert all(len(set(row.tolist())) == S for row in sc)
            want = np.stack([np.argsort(-row, kind="stable")[:m] for row in sc])
            assert np.array_equal(r["order"], want), RR.case_id(c)
            assert np.array_equal(r["elite_rows"], want + S * np.arange(G)[:, None]) and r["elite_rows"].dtype == np.int32
            if variant == "reverse":
                assert np.array_equal(r["order"], np.broadcast_to(np.arange(S - 1, S - 1 - m, -1), (G, m)))


def test_rows_behind_the_elites_are_augment_ref_on_the_elites():
    for c in RR.cases():
        inp, r = RR.make_inputs(c), RR.case_reference(c)
        G, S, m, K, h = c["shape"]
        K = inp["K"]
        src = _src(c, inp)
        out = r["out"].reshape((G, m + K) + r["out"].shape[1:])
        elites = out[:, :m].reshape((G * m,) + r["out"].shape[1:])
        assert np.array_equal(elites, src[r["elite_rows"].reshape(-1)]), RR.case_id(c)      # gathered verbatim
        assert np.array_equal(r["elite_scores"].view(np.int32), inp["scores"][r["elite_rows"]].view(np.int32))
        kw = dict(sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"])
        if c["form"] == "tokens":
            a = AR.reference_tokens(elites, m, K, inp["normals"], inp["centers"], RR.TOK_VOCAB, h, **kw)
        else:
            a = AR.reference_actions(elites, m, K, inp["normals"], **kw)
        for k in ("out", "mean", "sd", "votes"):
            assert np.array_equal(np.ascontiguousarray(a[k]).view(np.int32 if a[k].dtype == np.float32 else a[k].dtype),
                                  np.ascontiguousarray(r[k]).view(np.int32 if r[k].dtype == np.float32 else r[k].dtype)), (RR.case_id(c), k)
        assert r["out"].shape[0] == G * (m + K)


def test_variant_all_equal_keeps_the_first_rows():
    for c, inp, r in _each("all_equal"):
        G, S, m, K, h = c["shape"]
        assert np.array_equal(r["order"], np.broadcast_to(np.arange(m), (G, m)))


def test_variant_ties_are_decided_by_the_index():
    some = 0
    for c, inp, r in _each("ties"):
        G, S, m, K, h = c["shape"]
        sc = inp["scores"].reshape(G, S)
        assert len(np.unique(sc)) <= 3
        for g in range(G):
            es = sc[g][r["order"][g]]
            assert (np.diff(es) <= 0).all()
            for v in np.unique(es):                                    # inside one score: ascending rows, and the lowest ones of that score
                idx = r["order"][g][es == v]
                assert (np.diff(idx) > 0).all()
                assert np.array_equal(idx, np.flatnonzero(sc[g] == v)[:len(idx)])
                some += len(idx) > 1
    assert some


def test_variant_signed_zero_counts_as_one_score():
    for c, inp, r in _each("signed_zero"):
        G, S, m, K, h = c["shape"]
        sc = inp["scores"].reshape(G, S)
        for g in range(G):
            zeros = np.flatnonzero(sc[g] == 0)
            assert np.signbit(sc[g][zeros]).any() and not np.signbit(sc[g][zeros]).all() and np.signbit(sc[g][zeros[0]])
            assert (sc[g][sc[g] != 0] < 0).all()
            k = min(m, len(zeros))
            assert np.array_equal(r["order"][g][:k], zeros[:k])        # the zeros lead, by index whatever their sign


def test_variant_neg_inf_rows_are_elites_in_index_order():
    for c, inp, r in _each("neg_inf"):
        G, S, m, K, h = c["shape"]
        sc = inp["scores"].reshape(G, S)
        for g in range(G):
            n_inf = int(np.isneginf(sc[g]).sum())
            assert n_inf > S - m
            n_fin = S - n_inf
            assert np.isfinite(sc[g][r["order"][g][:n_fin]]).all()
            assert np.array_equal(r["order"][g][n_fin:], np.flatnonzero(np.isneginf(sc[g]))[:m - n_fin])


def test_variant_nan_ranks_behind_minus_infinity():
    nan_elites = 0
    for c, inp, r in _each("nan"):
        G, S, m, K, h = c["shape"]
        sc = inp["scores"].reshape(G, S)
        for g in range(G):
            nan = np.isnan(sc[g])
            assert np.isnan(sc[g][0]) and not np.signbit(sc[g][0])     # a positive NaN at row 0: desc_key alone would rank it first
            assert (nan & np.signbit(sc[g])).any() and (nan & ~np.signbit(sc[g])).any() and np.isneginf(sc[g]).any()
            n_num = int((~nan).sum())
            k = min(m, n_num)
            assert not np.isnan(sc[g][r["order"][g][:k]]).any()
            es = sc[g][r["order"][g][:k]]
            assert (es[1:] <= es[:-1]).all()                           # -inf among the numbers, behind the finite ones
            assert np.array_equal(r["order"][g][k:], np.flatnonzero(nan)[:m - k])
            nan_elites += m - k
        assert np.array_equal(r["elite_scores"].view(np.int32), sc.reshape(-1)[r["elite_rows"]].view(np.int32))     # payloads kept
    assert nan_elites


def test_variant_k0_is_a_pure_gather():
    for c, inp, r in _each("k0"):
        G, S, m, K, h = c["shape"]
        assert inp["K"] == 0 and inp["normals"].shape[1] == 0
        assert np.array_equal(r["out"], _src(c, inp)[r["elite_rows"].reshape(-1)])


# ------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_validate_without_a_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    G, S, m, K, h = 2, 6, 3, 4, 2
    N = G * S
    tok = torch.full((N, 7 * h), RR.TOK_VOCAB - 100, dtype=torch.int64)
    act = torch.zeros(N, h, 7)
    sc = torch.zeros(N)
    z = torch.zeros(G, K, h, 6)
    cen = torch.from_numpy(AR.openvla_centers())
    T = lambda **kw: ops.refine_tokens(kw.pop("tokens", tok), kw.pop("scores", sc), kw.pop("S", S), kw.pop("m", m), kw.pop("K", K),
                                       kw.pop("normals", z), kw.pop("centers", cen), RR.TOK_VOCAB, **{"steps": h, **kw})
    A = lambda **kw: ops.refine_actions(kw.pop("actions", act), kw.pop("scores", sc), kw.pop("S", S), kw.pop("m", m), kw.pop("K", K),
                                        kw.pop("normals", z), **kw)
    common = [dict(m=0), dict(m=7), dict(m=-1), dict(m=2.0), dict(m=True), dict(S=5), dict(S=0), dict(S=4097), dict(S=6.0), dict(K=-1),
              dict(K=4097), dict(K=5), dict(K=4.0),
              dict(scores=sc.double()), dict(scores=sc.numpy()), dict(scores=sc[:-1]), dict(scores=torch.zeros(N + 1)), dict(scores=sc[None]),
              dict(scores=torch.zeros(2 * N)[::2]), dict(scores=sc.to("meta")), dict(scores=sc.long()),
              dict(normals=z.double()), dict(normals=z.numpy()), dict(normals=z[:, :, :1]), dict(normals=torch.zeros(G, K, h, 12)[..., ::2]),
              dict(normals=z.reshape(G * K, h, 6)), dict(normals=torch.zeros(G, K + 1, h, 6)), dict(normals=z.to("meta")),
              dict(sigma=-0.5), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=1e39),
              dict(sd_floor=-1e-3), dict(sd_floor=float("nan")), dict(sd_floor=float("inf")), dict(clip=(0.5, -0.5)), dict(clip=(float("nan"), 1.0)),
              dict(clip=0.5), dict(clip=(1.0,))]
    for kw in common:
        with pytest.raises(CoverError):
            T(**dict(kw))
        with pytest.raises(CoverError):
            A(**dict(kw))
    for kw in (dict(tokens=tok.int()), dict(tokens=tok.numpy()), dict(tokens=tok[0]), dict(tokens=tok[:, :13]), dict(tokens=tok.t().contiguous().t()),
               dict(steps=0), dict(steps=3), dict(centers=cen.double()), dict(centers=cen[None]), dict(centers=cen[:0]), dict(centers=cen.numpy()),
               dict(out=torch.zeros(G * (m + K), 7 * h)), dict(out=torch.zeros(N, 7 * h, dtype=torch.int64)),
               dict(tokens=torch.zeros(65 * 7, dtype=torch.int64).expand(N, 65 * 7), steps=65, normals=torch.zeros(G, K, 65, 6))):
        with pytest.raises(CoverError):
            T(**kw)
    for kw in (dict(actions=act.double()), dict(actions=act.numpy()), dict(actions=act[0]), dict(actions=act[..., :6]),
               dict(actions=torch.zeros(N, h, 14)[..., ::2]), dict(out=torch.zeros(G * (m + K), h, 7, dtype=torch.float64)),
               dict(out=torch.zeros(G * (m + K), h, 8)[..., :7]), dict(out=torch.zeros(N, h, 7)),
               dict(actions=torch.zeros(N, 65, 7), normals=torch.zeros(G, K, 65, 6))):
        with pytest.raises(CoverError):
            A(**kw)
    # valid arguments on host tensors: there is no CPU path
    for call in (T, A):
        with pytest.raises(CoverError, match="device"):
            call()
        with pytest.raises(CoverError, match="device"):
            call(K=0, normals=torch.zeros(G, 0, h, 6), stats=True, elites=True, clip=(-float("inf"), float("inf")), m=S)
    with pytest.raises(CoverError, match="device"):
        ops.refine_actions(torch.zeros(N, h + 1, 32)[:, :h, :7], sc, S, m, K, z)              # the strided view is accepted as it is


def test_signatures_default_to_off():
    from cover_vla_amd import ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    p = inspect.signature(ops.refine_tokens).parameters
    assert list(p)[:8] == ["tokens", "scores", "group_rows", "n_elite", "n_new", "normals", "centers", "tok_vocab"]
    assert [(k, p[k].default) for k in list(p)[8:]] == [("steps", 1), ("sigma", 1.0), ("sd_floor", 0.0), ("clip", (-1.0, 1.0)), ("out", None),
                                                         ("stats", False), ("elites", False)]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[8:])
    p = inspect.signature(ops.refine_actions).parameters
    assert list(p)[:6] == ["actions", "scores", "group_rows", "n_elite", "n_new", "normals"]
    assert [k for k in list(p)[6:]] == ["sigma", "sd_floor", "clip", "out", "stats", "elites"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[6:])
    assert ops.RefineElites._fields == ("rows", "scores")
    p = inspect.signature(OpenVLA.refine).parameters
    assert list(p) == ["self", "tokens", "scores", "group_rows", "n_elite", "normals", "sigma", "sd_floor", "elites"]
    assert (p["sigma"].default, p["sd_floor"].default, p["elites"].default) == (1.0, 0.0, False)
    p = inspect.signature(EfficientEnsembleMerged.score_refined).parameters
    assert list(p) == ["self", "its", "candidates", "group_rows", "to_histories", "refine", "normals", "n_elite", "prior_fn", "score_kw"]
    assert p["prior_fn"].default is None and p["score_kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert "NaN" in ops.refine_tokens.__doc__ and "TIE" in ops.refine_tokens.__doc__


# ------------------------------------------------------------------------------------------------ binding
def test_binding_mirrors_the_header():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_refine_args"] is L.RefineArgs
    for sym in ("cover_refine_tokens", "cover_refine_actions"):
        assert L.SYMBOLS[sym] == (C.c_int, [C.POINTER(L.RefineArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_refine_tokens(const cover_refine_args* args, void* stream);" in hdr
    assert "int cover_refine_actions(const cover_refine_args* args, void* stream);" in hdr
    body = hdr[hdr.index("typedef struct cover_refine_args {"):hdr.index("} cover_refine_args;")]
    body = re.sub(r"/\*.*?\*/", "", body)
    pos = [re.search(rf"\b{name}\b", body).start() for name, _ in L.RefineArgs._fields_]   # the header's fields in the header's order
    assert pos == sorted(pos)
    assert C.sizeof(L.RefineArgs) == 144 and C.sizeof(L.AugmentArgs) == 112
    if os.path.exists(L.LIB_PATH):                                    # cover_sizeof and cover_abi_version are host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_refine_tokens") and hasattr(h, "cover_refine_actions")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_refine_args") == C.sizeof(L.RefineArgs)
        assert h.cover_abi_version() == 1


def test_draw_is_shared_not_copied():
    """augment.hip and refine.hip take the draw from one header and the fit from the other; neither restates them."""
    csrc = os.path.join(ROOT, "cover_vla_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("augment.hip", "refine.hip", "augment_draw.h", "Makefile")}
    assert "fminf(fmaxf(v, clip_lo), clip_hi)" in text["augment_draw.h"] and "#pragma clang fp contract(off)" in text["augment_draw.h"]
    for f in ("augment.hip", "refine.hip"):
        assert '#include "augment_draw.h"' in text[f] and "augment_draw_rows<T>(" in text[f] and "augment_group_stats<T>(" in text[f]
        assert "fmaxf" not in text[f] and "sqrtf" not in text[f] and "#pragma clang fp contract(off)" in text[f]
    assert "bitonic_sort_lds(" in text["refine.hip"] and "desc_key(" in text["refine.hip"]
    assert "refine.hip" in text["Makefile"] and "augment_draw.h" in text["Makefile"]


# ------------------------------------------------------------------------------------------------ score_refined
class _StubVerifier:
    """score_histories as a pure row-wise function of the histories; the dict gains robust / combined as the real one does."""

    def __init__(self, log):
        self.log = log

    def score_histories(self, its, hb, group_size, pad=None, **kw):
        self.log.append(("score", tuple(hb.shape), group_size, dict(kw)))
        scores = -(hb ** 2).sum(dim=1)
        out = {"scores": scores}
        base = scores
        if kw.get("member_kappa") is not None:
            out["robust"] = base = scores - 0.5 * hb[:, 0].abs()
        if kw.get("prior") is not None:
            out["combined"] = base = base + kw.get("prior_beta", 0.0) * kw["prior"]
        per = base.reshape(-1, group_size)
        g = int(per.max(dim=1).values.argmax())
        l = int(per[g].argmax())
        out["result"] = torch.tensor([g * group_size + l, g, l, 0], dtype=torch.int32)
        out["best"] = torch.stack([per[g, l], per.mean()])
        out["group_best"] = per.max(dim=1).values
        return out


def _stub_refine(log, with_elites):
    def refine(cands, values, S, m, z):
        log.append(("refine", tuple(cands.shape), S, m, values))
        G = cands.shape[0] // S
        order = torch.stack([torch.argsort(-values[g * S:(g + 1) * S], stable=True)[:m] + g * S for g in range(G)])
        el = cands[order.reshape(-1)].reshape(G, m, -1)
        new = el.mean(dim=1, keepdim=True) + 0.3 * z.reshape(G, z.shape[1], -1)[..., :cands.shape[1]]
        out = torch.cat([el, new], dim=1).reshape(G * (m + z.shape[1]), -1)
        return (out, order.to(torch.int32)) if with_elites else out
    return refine


def _refined(kw, normals, with_elites=True, prior_fn=None):
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    log = []
    ver = object.__new__(EfficientEnsembleMerged)                      # the loop only: no checkpoint, no device
    ver.score_histories = _StubVerifier(log).score_histories
    g = torch.Generator().manual_seed(4)
    cands = torch.randn(3 * 10, 6, generator=g)
    its = torch.zeros(1)
    out = ver.score_refined(its, cands, 10, to_histories=lambda c: (c, None), refine=_stub_refine(log, with_elites), normals=normals, n_elite=3,
                            prior_fn=prior_fn, **kw)
    return cands, log, out


def test_score_refined_is_the_documented_composition():
    g = torch.Generator().manual_seed(5)
    normals = [torch.randn(3, 7, 1, 6, generator=g), torch.randn(3, 5, 1, 6, generator=g)]
    for kw, key in ((dict(), "scores"), (dict(member_kappa=0.5), "robust"),
                    (dict(member_kappa=0.5, prior_beta=0.25), "combined"), (dict(prior_beta=0.25), "combined")):
        prior_fn = None
        seen_fit = []
        if "prior_beta" in kw:
            def prior_fn(c, S, n_fit):
                seen_fit.append((tuple(c.shape), S, n_fit))
                return -c[:, 1].abs()
        cands, log, out = _refined(kw, normals, prior_fn=prior_fn)
        kinds = [e[0] for e in log]
        assert kinds == ["score", "refine", "score", "refine", "score"]
        assert [(e[1], e[2]) for e in log if e[0] == "score"] == [((30, 6), 10), ((30, 6), 10), ((24, 6), 8)]
        assert [(e[1], e[2], e[3]) for e in log if e[0] == "refine"] == [((30, 6), 10, 3), ((30, 6), 10, 3)]
        for e in log:
            if e[0] == "score":
                assert {k: v for k, v in e[3].items() if k != "prior"} == kw and ("prior" in e[3]) == ("prior_beta" in kw)
        if prior_fn is not None:
            assert seen_fit == [((30, 6), 10, None), ((30, 6), 10, 3), ((24, 6), 8, 3)]
        # the value a round refines on is the one the previous decision was made on: recompute the chain by hand
        ver = _StubVerifier([])
        refine = _stub_refine([], True)
        c, S, n_fit, outs = cands, 10, None, []
        for r in range(3):
            if r:
                c, rows = refine(c, outs[-1][key], S, 3, normals[r - 1])
                S, n_fit = 3 + normals[r - 1].shape[1], 3
            k2 = dict(kw)
            if prior_fn is not None:
                k2["prior"] = -c[:, 1].abs()
            outs.append(ver.score_histories(None, c, S, **k2))
        assert key in outs[-1] and all(k2 in outs[-1] for k2 in ("scores",))
        assert torch.equal(log[1][4], outs[0][key]) and torch.equal(log[3][4], outs[1][key])
        assert torch.equal(out["candidates"], c) and tuple(out["candidates"].shape) == (24, 6)
        for k in outs[-1]:
            assert torch.equal(out[k], outs[-1][k]), k
        assert len(out["rounds"]) == 3 and out["rounds"][0]["elite_rows"] is None
        for r in range(3):
            assert torch.equal(out["rounds"][r]["best"], outs[r]["best"]) and torch.equal(out["rounds"][r]["result"], outs[r]["result"])
        assert out["rounds"][1]["elite_rows"].dtype == torch.int32 and tuple(out["rounds"][2]["elite_rows"].shape) == (3, 3)
        # the elites are carried verbatim and the stub scorer is row-wise: no prompt's best value decreases (without a prior that is
        # refitted per round, which re-scores the carried rows)
        if prior_fn is None:
            for a, b in zip(outs[:-1], outs[1:]):
                assert (b["group_best"] >= a["group_best"]).all()
                assert float(b["best"][0]) >= float(a["best"][0])


def test_score_refined_with_no_rounds_is_one_scoring_call():
    cands, log, out = _refined(dict(top_m=0), [])
    assert [e[0] for e in log] == ["score"] and log[0][1:3] == ((30, 6), 10) and log[0][3] == dict(top_m=0)
    assert out["candidates"] is cands and len(out["rounds"]) == 1 and out["rounds"][0]["elite_rows"] is None
    assert torch.equal(out["rounds"][0]["result"], out["result"])
    # a refine that returns the rows alone: elite_rows stays None
    g = torch.Generator().manual_seed(6)
    cands, log, out = _refined(dict(), [torch.randn(3, 2, 1, 6, generator=g)], with_elites=False)
    assert [e[0] for e in log] == ["score", "refine", "score"] and out["rounds"][1]["elite_rows"] is None
    assert tuple(out["candidates"].shape) == (15, 6)


def test_score_refined_rejects_a_fixed_prior_with_rounds():
    from cover_vla_amd._lib import CoverError
    g = torch.Generator().manual_seed(7)
    with pytest.raises(CoverError):
        _refined(dict(prior=torch.zeros(30), prior_beta=0.5), [torch.randn(3, 2, 1, 6, generator=g)])
    with pytest.raises(CoverError):
        _refined(dict(prior=torch.zeros(30), prior_beta=0.5), [], prior_fn=lambda c, S, n: torch.zeros(len(c)))
    cands, log, out = _refined(dict(prior=torch.zeros(30), prior_beta=0.5), [])      # the given candidates' own prior: forwarded
    assert [e[0] for e in log] == ["score"] and "combined" in out
