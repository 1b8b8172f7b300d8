"""Neighbourhood-smoothed scores without a GPU: the reference of tests/smooth_ref.py has the properties the header states, its case table
is not vacuous, the constructed decision flips with the margins it promises, the binding mirrors the header, host.Smooth and the ops
wrappers reject bad arguments before anything is launched, and score_refined refines on `smoothed`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import smooth_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SMALL = [s for s in SR.SHAPES + SR.FLOAT_ONLY if s[1] <= 130]          # the CPU properties need no large shape


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


def _values(c):
    inp = SR.make_inputs(c)
    return inp, SR.values_of(inp, c["form"], c["shape"][2])


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_names_what_it_says():
    assert SR.SHAPES == [(1, 1, 1), (3, 17, 1), (2, 63, 2), (2, 64, 1), (2, 65, 1), (1, 130, 3), (1, 1025, 1)]
    assert SR.LARGE == (1, 4096, 1) and SR.HISTORY == (2, 40, 10) and SR.SHRINKS == (0.0, 0.5) and SR.SPLITS == (0, 1)
    cs = SR.cases()
    assert len({SR.case_id(c) for c in cs}) == len(cs) == 4 * (2 * len(SR.SHAPES) + len(SR.FLOAT_ONLY) + len(SR.TOKEN_EXTRA))
    assert any(SR.token_row_stride(s) > 7 * s[2] for s in SR.SHAPES) and any(SR.token_row_stride(s) == 7 * s[2] for s in SR.SHAPES)
    assert 0.0 in SR.ZERO_SCALE and all(v > 0 for v in SR.DIM_SCALE)


@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_neighbourhoods_of_the_table_are_partial(form):
    """Not vacuous: at every shape with a cluster some rows have neighbours and no row has its whole group; splitting by gripper class
    removes pairs; the history layout's pads and shared past contribute nothing."""
    for shape in (s for s in SR.shapes_of(form) if 17 <= s[1] <= 130):
        ref = {p: SR.case_reference(dict(form=form, shape=shape, shrink=0.5, split=p)) for p in SR.SPLITS}
        nb0, nb1 = ref[0]["neighbours"], ref[1]["neighbours"]
        assert nb0.max() > 1 and nb0.max() < shape[1] and (nb0 == 1).sum() < len(nb0), (shape, nb0)
        assert (nb1 <= nb0).all() and (nb1 < nb0).any() and nb1.max() > 1, shape
        assert not np.array_equal(_bits(ref[1]["smoothed"]), _bits(SR.make_inputs(dict(form=form, shape=shape, shrink=0.5, split=1))["scores"]))
    inp, x = _values(dict(form="actions", shape=SR.HISTORY, shrink=0.0, split=1))
    own = SR.reference(x[:, 6:], inp["scores"], inp["S"], inp["dim_scale"], inp["radius"])
    for k, v in SR.case_reference(dict(form="actions", shape=SR.HISTORY, shrink=0.0, split=1)).items():
        assert np.array_equal(v.view(np.int32), own[k].view(np.int32)), k     # exact zeros: the distance is that of the own steps


def test_zero_scale_hides_the_planted_nan():
    c = dict(form="actions", shape=SR.ZERO_DIM, shrink=0.5, split=1)
    inp, x = _values(c)
    assert np.isnan(x[..., 1]).any() and np.isnan(x[..., 4]).any() and not np.isnan(np.delete(x, (1, 4), axis=2)).any()
    clean = np.where(np.isnan(x), F32(0.25), x)
    a, b = SR.case_reference(c), SR.reference(clean, inp["scores"], inp["S"], inp["dim_scale"], inp["radius"], 0.5, 1)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert a["neighbours"].max() > 1 and not np.isnan(a["smoothed"]).any()


# ------------------------------------------------------------------------------------------------ reference properties
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_radius_below_every_distance_returns_the_scores(form):
    for shape in (s for s in SR.shapes_of(form) if s in SMALL and s != SR.ZERO_DIM):
        inp, x = _values(dict(form=form, shape=shape, shrink=0.0, split=0))
        x = x.copy()
        x[:, 0, 0] += np.arange(len(x), dtype=F32) * F32(0.01)         # every pair differs by >= 0.01 in dim 0 (scale 1)
        r = SR.reference(x, inp["scores"], inp["S"], inp["dim_scale"], 0.005, 0.0, 0)
        assert np.array_equal(_bits(r["smoothed"]), _bits(inp["scores"])) and (r["neighbours"] == 1).all()
        assert np.array_equal(_bits(r["density"]), _bits(np.full(len(x), F32(1.0) / F32(shape[1]))))


@pytest.mark.parametrize("S", (1, 2, 17, 63, 64))
def test_identical_rows_give_the_chain_mean(S):
    """All rows identical, shrink 0, S <= 64: every weight is 1, every lane holds exactly one score and den is exactly S, so smoothed is
    the butterfly's sum of the scores over (float)S. That sum is a tree, the single chain ((0.0f + s_0) + s_1) + ... is not: the two are
    the same bits for every S only where no addition rounds, so the chain is asserted on scores that are multiples of 2^-10 (their
    sums are exact in either order) and the tree on arbitrary ones."""
    rng = np.random.default_rng(S)
    x = np.broadcast_to(rng.uniform(-1, 1, (1, 2, 7)).astype(F32), (S, 2, 7))
    s = (rng.integers(-2000, 2000, S).astype(F32) / F32(1024.0)).astype(F32)
    chain = F32(0.0)
    for v in s:
        chain = chain + v
    r = SR.reference(x, s, S, SR.DIM_SCALE, 0.3, 0.0, 1)
    assert np.array_equal(_bits(r["smoothed"]), _bits(np.full(S, chain / F32(S))))
    assert (r["neighbours"] == S).all() and np.array_equal(_bits(r["density"]), _bits(np.ones(S, dtype=F32)))
    assert _bits(r["group_mean"])[0] == _bits(chain / F32(S))[0]
    s = rng.normal(size=S).astype(F32)
    lanes = np.zeros((1, 64), dtype=F32)
    lanes[0, :S] = s
    o = 32
    while o:
        lanes = lanes + lanes[:, np.arange(64) ^ o]
        o //= 2
    r = SR.reference(x, s, S, SR.DIM_SCALE, 0.3, 0.0, 1)
    assert np.array_equal(_bits(r["smoothed"]), _bits(np.full(S, lanes[0, 0] / F32(S))))
    assert _bits(r["group_mean"])[0] == _bits(lanes[0, 0] / F32(S))[0]


@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_float64_evaluation_agrees(form):
    for c in SR.cases(forms=(form,), shapes=SMALL):
        inp, x = _values(c)
        want = SR.reference_f64(x, inp["scores"], inp["S"], inp["dim_scale"], inp["radius"], inp["shrink"], inp["split"])
        got = SR.case_reference(c)["smoothed"].astype(np.float64)
        assert (inp["scores"] > 0.1).all()                             # the table's scores are positive: no mean of them cancels
        assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (SR.case_id(c), np.max(np.abs(got - want) / np.abs(want)))


def test_large_shrink_approaches_the_group_mean():
    c = dict(form="actions", shape=(3, 17, 1), shrink=0.0, split=1)
    inp, x = _values(c)
    err = []
    for shrink in (1e2, 1e4, 1e6):
        r = SR.reference(x, inp["scores"], inp["S"], inp["dim_scale"], inp["radius"], shrink, 1)
        m0 = np.repeat(r["group_mean"], inp["S"])
        err.append(float(np.max(np.abs(r["smoothed"] - m0))))
    assert err[0] > err[1] > err[2] and err[2] <= 1e-6, err


def test_special_scores_pass_through_and_are_no_evidence():
    c = dict(form="actions", shape=(2, 65, 1), shrink=0.5, split=0)
    inp, x = _values(c)
    s = inp["scores"].copy()
    s.view(np.uint32)[[3, 70]] = 0x7FC00ABC, 0xFFC12345
    s[[10, 80]], s[[20, 90]] = np.inf, -np.inf
    special = [3, 70, 10, 80, 20, 90]
    r = SR.reference(x, s, inp["S"], inp["dim_scale"], inp["radius"], 0.5, 0)
    assert np.array_equal(_bits(r["smoothed"])[special], _bits(s)[special])
    far = x.copy()
    far[special, 0, 0] += F32(50.0) + np.arange(6, dtype=F32)          # the same rows moved out of every radius
    r2 = SR.reference(far, s, inp["S"], inp["dim_scale"], inp["radius"], 0.5, 0)
    rest = np.setdiff1d(np.arange(len(s)), special)
    assert np.array_equal(_bits(r["smoothed"])[rest], _bits(r2["smoothed"])[rest]) and np.isfinite(r["smoothed"][rest]).all()
    assert np.array_equal(_bits(r["group_mean"]), _bits(r2["group_mean"]))
    none = SR.reference(x, np.full(len(s), np.nan, dtype=F32), inp["S"], inp["dim_scale"], inp["radius"], 0.5, 0)
    assert np.isnan(none["smoothed"]).all() and np.array_equal(_bits(none["group_mean"]), _bits(np.zeros(2)))


# ------------------------------------------------------------------------------------------------ the constructed decision
def test_constructed_decision_flips_with_a_margin():
    d = SR.constructed_decision()
    s = d["scores"]
    assert int(np.argmax(s)) == 8 and s[8] - np.delete(s, 8).max() >= 1e-3
    r = SR.reference(d["actions"], s, d["S"], d["dim_scale"], d["radius"], d["shrink"], d["split"])
    sm = r["smoothed"]
    assert int(np.argmax(sm)) < 8 and sm[:8].max() - sm[8:].max() >= 1e-3, sm
    assert (r["neighbours"][:8] == 8).all() and (r["neighbours"][8:] == 1).all()
    assert r["group_mean"][0] < s[:8].min()                            # the low rows pull the mean below the cluster


# ------------------------------------------------------------------------------------------------ binding
def test_binding_mirrors_the_header():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_smooth_args"] is L.SmoothArgs
    for sym in ("cover_smooth_scores_tokens", "cover_smooth_scores_actions"):
        assert L.SYMBOLS[sym] == (C.c_int, [C.POINTER(L.SmoothArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_smooth_scores_tokens(const cover_smooth_args* args, void* stream);" in hdr
    assert "int cover_smooth_scores_actions(const cover_smooth_args* args, void* stream);" in hdr
    body = hdr[hdr.index("typedef struct cover_smooth_args {"):hdr.index("} cover_smooth_args;")]
    body = re.sub(r"/\*.*?\*/", "", body)
    pos = [re.search(rf"\b{name}\b", body).start() for name, _ in L.SmoothArgs._fields_]   # the header's fields in the header's order
    assert pos == sorted(pos)
    assert C.sizeof(L.SmoothArgs) == 112
    if os.path.exists(L.LIB_PATH):                                     # cover_sizeof and cover_abi_version are host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_smooth_scores_tokens") and hasattr(h, "cover_smooth_scores_actions")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_smooth_args") == C.sizeof(L.SmoothArgs)
        assert h.cover_abi_version() == 1


def test_kernel_file_shares_the_token_rule():
    csrc = os.path.join(ROOT, "cover_vla_amd", "csrc")
    text = open(os.path.join(csrc, "smooth.hip")).read()
    rows = open(os.path.join(csrc, "chunk_rows.h")).read()                 # the row source holds the token rule, once
    assert '#include "chunk_rows.h"' in text and "chunk_stage_rows(" in text and "tok_vocab -" not in text and "centers[" not in text
    assert rows.count("tok_vocab -") == 1 and "s.value(" in rows[rows.index("void chunk_stage_rows("):]
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.lower().replace("no atomics", "")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert "smooth.hip" in make and " chunk_rows.h " in make


# ------------------------------------------------------------------------------------------------ host validation
def test_host_smooth_validates():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    ok = host.Smooth(0.1, [1, 1, 1, 0.5, 0.5, 0], shrink=2, split_gripper=0)
    assert ok == (0.1, (1.0, 1.0, 1.0, 0.5, 0.5, 0.0), 2.0, False) and ok.shrink == 2.0 and ok.split_gripper is False
    assert host.Smooth(0.1, np.ones(6)).shrink == 0.0 and host.Smooth(0.1, np.ones(6)).split_gripper is True
    with pytest.raises(AttributeError):
        ok.radius = 1.0
    nan, inf = float("nan"), float("inf")
    for scale in ([1, 1, 1, 1, 1, -0.5], [1, nan, 1, 1, 1, 1], [1, 1, inf, 1, 1, 1], [1, 1, 1, 1, 1], [1] * 7, 1.0, "abcdef", [1e39] + [1] * 5):
        with pytest.raises(CoverError):
            host.Smooth(0.1, scale)
    for radius in (0, -0.1, nan, inf, 1e-30, 1e30, "1", True):
        with pytest.raises(CoverError):
            host.Smooth(radius, np.ones(6))
    for shrink in (-0.5, nan, inf, "0", True):
        with pytest.raises(CoverError):
            host.Smooth(0.1, np.ones(6), shrink=shrink)
    with pytest.raises(TypeError):
        host.Smooth(dim_scale=np.ones(6))                              # no default radius


def test_ops_wrappers_reject_bad_arguments_before_any_launch():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    tok, act, s = torch.zeros(6, 7, dtype=torch.int64), torch.zeros(6, 1, 7), torch.zeros(6)
    cen = torch.zeros(255)
    kw = dict(radius=0.1, dim_scale=[1.0] * 6)
    with pytest.raises(CoverError, match="no CPU path"):
        ops.smooth_scores_actions(act, s, 3, **kw)
    with pytest.raises(CoverError, match="no CPU path"):
        ops.smooth_scores_tokens(tok, s, 3, cen, 32000, **kw)
    for bad in (dict(kw, radius=0.0), dict(kw, radius=float("nan")), dict(kw, shrink=-1.0), dict(kw, shrink=float("inf")),
                dict(kw, dim_scale=[1.0] * 5), dict(kw, dim_scale=[1, 1, 1, 1, 1, -1.0]), dict(kw, dim_scale=[1, 1, 1, 1, 1, float("nan")])):
        with pytest.raises(CoverError, match="radius|shrink|dim_scale"):
            ops.smooth_scores_actions(act, s, 3, **bad)
    for S in (0, 4, 4097, 2.0, True):
        with pytest.raises(CoverError, match="group_rows"):
            ops.smooth_scores_actions(act, s, S, **kw)
    with pytest.raises(CoverError, match="scores"):
        ops.smooth_scores_actions(act, s[:5], 3, **kw)
    with pytest.raises(CoverError, match="actions must be"):
        ops.smooth_scores_actions(act[..., :6], s, 3, **kw)
    with pytest.raises(CoverError, match="tokens must be"):
        ops.smooth_scores_tokens(tok.to(torch.int32), s, 3, cen, 32000, **kw)
    with pytest.raises(TypeError):
        ops.smooth_scores_actions(act, s, 3, dim_scale=[1.0] * 6)      # no default radius


# ------------------------------------------------------------------------------------------------ score_refined
def test_score_refined_refines_on_smoothed():
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    seen = []

    class Stub:
        def score_histories(self, its, hb, group_size, pad=None, **kw):
            n = len(hb)
            out = {"scores": torch.arange(n, dtype=torch.float32), "robust": torch.arange(n, dtype=torch.float32) + 100,
                   "result": torch.zeros(4, dtype=torch.int32), "best": torch.zeros(2)}
            if kw.get("smooth") is not None:
                out["smoothed"] = torch.arange(n, dtype=torch.float32) + 200
            if kw.get("top_m"):
                out["combined"] = torch.arange(n, dtype=torch.float32) + 300
            return out

    def refine(c, values, S, m, z):
        seen.append(float(values[0]))
        return c

    run = lambda **kw: EfficientEnsembleMerged.score_refined(Stub(), None, torch.zeros(4, 7), 2, to_histories=lambda c: (c, None), refine=refine,
                                                             normals=[torch.zeros(2, 0, 1, 6)], n_elite=2, **kw)
    run()
    run(smooth="a record")
    run(smooth="a record", top_m=1)
    assert seen == [100.0, 200.0, 300.0]


# ------------------------------------------------------------------------------------------------ host.verify_and_select
class _StubVerifier:
    """Scripted stage results; records the keywords it is given and keeps last_smooth_stats as the real verifier does."""

    def __init__(self, stage1):
        self.stage1, self.calls, self.last_smooth_stats = stage1, [], None

    def compute_max_similarity_scores_batch(self, images, instructions, all_action_histories, cfg_repeat_language_instructions=1, **kw):
        self.calls.append((len(all_action_histories), dict(kw)))
        if len(all_action_histories) == 1:
            return self.stage1, instructions[0], all_action_histories[0], torch.tensor(0)
        if kw.get("smooth") is not None:
            self.last_smooth_stats = {"neighbours": np.arange(10, 10 + len(all_action_histories), dtype=np.int32)}
        return 0.9, instructions[0], all_action_histories[4], torch.tensor(4)


def test_verify_and_select_forwards_smooth_to_stage_two_only():
    from cover_vla_amd import host
    rng = np.random.default_rng(1)
    B, S = 6, 3
    q = [rng.uniform(-1, 1, size=(B, 7)).astype(np.float32) for _ in range(4)]
    args = (None, "a", ["a"] * 3 + ["b"] * 3, q, [rng.normal(size=7) for _ in range(3)], S)
    smooth = host.Smooth(0.1, [1.0] * 6, shrink=1.0)
    fv = _StubVerifier(0.05)
    r = host.verify_and_select(fv, *args, process_image=False)
    assert fv.calls == [(1, {}), (B, {})] and "neighbours" not in r       # smooth=None: nothing reaches the verifier
    fv = _StubVerifier(0.05)
    r = host.verify_and_select(fv, *args, process_image=False, smooth=smooth)
    assert fv.calls == [(1, {}), (B, {"smooth": smooth})] and r["global_action_idx"] == 4 and r["neighbours"] == 14
    fv = _StubVerifier(0.5)                                               # stage 1 passes: stage 2 does not run, nothing is forwarded or recorded
    r = host.verify_and_select(fv, *args, process_image=False, smooth=smooth)
    assert fv.calls == [(1, {})] and "neighbours" not in r
    with pytest.raises(ValueError, match="host.Smooth"):
        host.verify_and_select(fv, *args, process_image=False, smooth=dict(radius=0.1))
