"""The chunk-coherence prior without a GPU: the reference of tests/coherence_ref.py has the properties the header states, its case table is
not vacuous, host.coherence_step_weights and host.Coherence check their values, the binding mirrors the header and the ops wrappers
reject bad arguments before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import coherence_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ONES = (1.0,) * 6


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32)).view(np.uint32)


def _rows(n, h, seed=0):
    x = np.random.default_rng(seed).uniform(-1, 1, (n, h, 7)).astype(F32)
    x[..., 6] = (x[..., 6] > 0).astype(F32)
    return x


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_names_what_it_says():
    assert CR.SHAPES == [(1, 1, 1, 1, 1, 0), (3, 17, 1, 4, 6, 2), (2, 33, 63, 3, 3, 0), (2, 16, 64, 8, 8, 0), (1, 15, 65, 8, 9, 8),
                         (2, 5, 130, 64, 64, 0), (1, 3, 1025, 1, 1, 0)]
    assert CR.PENALTIES == (0.0, 0.25) and CR.GROUPINGS == (0, 1) and CR.DIM_SCALE.count(0.0) == 1
    cs = CR.cases()
    assert len({CR.case_id(c) for c in cs}) == len(cs) == 4 * (2 * len(CR.SHAPES) + len(CR.FLOAT_ONLY))
    assert any(CR.token_row_stride(s) > 7 * s[3] for s in CR.SHAPES) and any(CR.token_row_stride(s) == 7 * s[3] for s in CR.SHAPES)
    assert CR.overlap(8, 9, 8) == 1 and CR.overlap(4, 6, 2) == 4 and CR.overlap(3, 5, 1) == 3
    text = open(os.path.join(ROOT, "cover_vla_amd", "csrc", "coherence.hip")).read()
    assert f"#define COHERENCE_MAX_TILE {CR.LARGEST_TILE}" in text          # the table's R_big is one more than the kernel's largest tile


@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_cases_of_the_table_are_not_vacuous(form):
    for shape in CR.shapes_of(form):
        G, S, R, h, hr, shift = shape
        for p in CR.GROUPINGS:
            c0, c1 = (dict(form=form, shape=shape, per_group=p, penalty=k) for k in CR.PENALTIES)
            inp = CR.make_inputs(c0)
            r0, r1 = CR.case_reference(c0), CR.case_reference(c1)
            w = inp["weight"].reshape(-1, R)
            assert (w[:, 0] != 0).all() and (w[:, R - 1] != 0).all()
            if R >= 63:
                assert (w == 0).any() and (w > 0).any() and (w < 0).any(), shape
            assert np.isfinite(r0["prior"]).all() and np.isfinite(r0["min_dist"]).all() and (r0["nearest"] >= 0).all(), CR.case_id(c0)
            firsts = np.arange(G if p else 1) * S                          # the rows that equal reference 0: D = 0, the tie goes to r = 0
            assert (r0["min_dist"][firsts] == 0).all() and (r0["nearest"][firsts] == 0).all()
            if S > 1:                                                      # (S = 1: the one row is its reference, the prior is -0.0)
                assert len(np.unique(_bits(r0["prior"]))) > 1
                assert not np.array_equal(_bits(r0["prior"]), _bits(r1["prior"])), CR.case_id(c1)    # the penalty acts
            x = CR.values_of(inp, form, h)
            f64 = CR.reference_f64(x, inp["ref"], inp["weight"], S, shift, inp["step_weight"], inp["dim_scale"], 0.0)
            assert np.allclose(r0["prior"], f64, rtol=1e-4, atol=1e-5), CR.case_id(c0)
        if form == "actions":
            assert np.isnan(CR.make_inputs(c0)["actions"][..., CR.DIM_SCALE.index(0.0)]).any() or S * h < 8
        assert np.isnan(CR.make_inputs(c0)["ref"][..., CR.DIM_SCALE.index(0.0)]).any() or R * hr < 8


# ------------------------------------------------------------------------------------------------ the properties the header states
def test_candidate_equal_to_its_only_reference_stores_minus_zero():
    x = _rows(3, 4)
    sw = CR.step_weights(4)
    for pen in (0.0, 0.25):
        r = CR.reference(x[:1], x[:1], np.ones(1, F32), 1, 0, sw, ONES, pen)
        assert _bits(r["prior"])[0] == 0x80000000 and r["min_dist"][0] == 0 and r["nearest"][0] == 0
    r = CR.reference(x, x[:1], np.ones(1, F32), 3, 0, sw, ONES)
    assert _bits(r["prior"])[0] == 0x80000000 and (r["prior"][1:] < 0).all()
    # a shift: candidate step t meets reference step t + 2; the overlap of h = 4 and hr = 3 is one step
    ref = np.full((1, 3, 7), np.nan, dtype=F32)
    ref[0, 2] = x[0, 0]
    r = CR.reference(x[:1], ref, np.ones(1, F32), 1, 2, sw, ONES)
    assert _bits(r["prior"])[0] == 0x80000000


def test_moving_away_lowers_the_prior_and_later_steps_count_less():
    x = _rows(1, 4)
    sw = CR.step_weights(4, 0.5)
    prev = F32(0.0)
    for k in range(1, 5):
        y = x.copy()
        y[0, 1, 3] += F32(0.1 * k)
        p = CR.reference(y, x, np.ones(1, F32), 1, 0, sw, ONES)["prior"][0]
        assert p < prev
        prev = p
    early, late = x.copy(), x.copy()
    early[0, 0, 0] += F32(0.25)
    late[0, 3, 0] += F32(0.25)
    pe, pl = (CR.reference(v, x, np.ones(1, F32), 1, 0, sw, ONES)["prior"][0] for v in (early, late))
    assert pe < pl < 0
    # a dim of scale 0 is not read; the gripper counts only with a penalty
    z = x.copy()
    z[0, :, 2] = np.nan
    z[0, 0, 6] = 1 - z[0, 0, 6]
    sc = (1.0, 1.0, 0.0, 1.0, 1.0, 1.0)
    assert _bits(CR.reference(z, x, np.ones(1, F32), 1, 0, sw, sc)["prior"])[0] == 0x80000000
    assert CR.reference(z, x, np.ones(1, F32), 1, 0, sw, sc, 0.25)["prior"][0] == F32(-0.25)


def test_zero_weight_reference_is_invisible_and_the_sign_follows_the_weight():
    x, ref = _rows(5, 2, 1), _rows(70, 2, 2)
    sw = CR.step_weights(2)
    w = np.random.default_rng(3).normal(size=70).astype(F32)
    w[[4, 64, 69]] = 0
    a = CR.reference(x, ref, w, 5, 0, sw, ONES)
    bad = ref.copy()
    bad[[4, 64, 69]] = np.nan
    b = CR.reference(x, bad, w, 5, 0, sw, ONES)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    assert not np.isin(a["nearest"], [4, 64, 69]).any()
    # one reference: the term's sign is the weight's
    pos = CR.reference(x, ref[:1], np.array([0.75], F32), 5, 0, sw, ONES)["prior"]
    neg = CR.reference(x, ref[:1], np.array([-0.75], F32), 5, 0, sw, ONES)["prior"]
    assert (pos < 0).all() and np.array_equal(_bits(pos) ^ np.uint32(0x80000000), _bits(neg))
    # a weighted NaN reference: every row's prior is the one NaN, and nearest skips it
    bad = ref.copy()
    bad[7, 0, 1] = np.nan
    c = CR.reference(x, bad, w, 5, 0, sw, ONES)
    assert (_bits(c["prior"]) == 0x7FC00000).all() and (c["nearest"] != 7).all() and np.isfinite(c["min_dist"]).all()
    # a NaN candidate element: its own row only
    y = x.copy()
    y[2, 1, 0] = np.nan
    d = CR.reference(y, ref, w, 5, 0, sw, ONES)
    assert _bits(d["prior"])[2] == 0x7FC00000 and d["nearest"][2] == -1 and np.isposinf(d["min_dist"][2])
    rest = [0, 1, 3, 4]
    assert np.array_equal(_bits(d["prior"])[rest], _bits(a["prior"])[rest]) and np.array_equal(d["nearest"][rest], a["nearest"][rest])


def test_nearest_is_the_lexicographic_minimum():
    x = _rows(2, 1, 4)
    ref = _rows(130, 1, 5)
    ref[[3, 67, 129]] = x[0]                                               # three exact ties at D = 0: lanes 3, 3 and 1
    sw, w = CR.step_weights(1), np.ones(130, F32)
    r = CR.reference(x, ref, w, 2, 0, sw, ONES)
    assert r["nearest"][0] == 3 and r["min_dist"][0] == 0
    w[3] = 0                                                               # weight 0 does not qualify
    assert CR.reference(x, ref, w, 2, 0, sw, ONES)["nearest"][0] == 67
    w[67] = -2.0                                                           # a negative weight does
    assert CR.reference(x, ref, w, 2, 0, sw, ONES)["nearest"][0] == 67
    none = CR.reference(x, ref, np.zeros(130, F32), 2, 0, sw, ONES)
    assert (none["nearest"] == -1).all() and np.isposinf(none["min_dist"]).all() and (_bits(none["prior"]) == 0x80000000).all()
    # a distance of +inf is a distance: the only qualifying reference is the nearest
    far = np.full((1, 1, 7), 3e38, dtype=F32)
    r = CR.reference(-far, far, np.ones(1, F32), 1, 0, sw, ONES)
    assert r["nearest"][0] == 0 and np.isposinf(r["min_dist"][0]) and np.isneginf(r["prior"][0])
    # an unusable scale: every prior NaN, nothing qualifies
    for v in (-1.0, np.nan, np.inf):
        r = CR.reference(x, ref, np.ones(130, F32), 2, 0, sw, (1.0, v, 1.0, 1.0, 1.0, 1.0))
        assert (_bits(r["prior"]) == 0x7FC00000).all() and (r["nearest"] == -1).all() and np.isposinf(r["min_dist"]).all()


# ------------------------------------------------------------------------------------------------ host records
def test_step_weights_against_float64():
    from cover_vla_amd import host
    for h, decay in ((1, 0.5), (4, 0.8), (64, 0.9), (10, 1.0), (64, 1e-3), (7, 1)):
        got = host.coherence_step_weights(h, decay)
        want = np.array([np.float32(float(decay) ** t) for t in range(h)], dtype=F32)
        assert got.dtype == F32 and got.shape == (h,) and np.array_equal(_bits(got), _bits(want)), (h, decay)
        assert got[0] == 1 and (np.diff(got.astype(np.float64)) <= 0).all()
        assert np.array_equal(_bits(got), _bits(CR.step_weights(h, decay)))
    for bad in (0, 0.0, -0.5, 1.5, float("nan"), float("inf"), True, "0.5", None):
        with pytest.raises(ValueError):
            host.coherence_step_weights(4, bad)
    for bad in (0, 65, -1, 2.0, True):
        with pytest.raises(ValueError):
            host.coherence_step_weights(bad, 0.5)


def test_coherence_record_checks_its_values():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    c = host.Coherence([1, 1, 0.5, 0, 0, 0.25], 0.8, gripper_penalty=0.25)
    assert c == ((1.0, 1.0, 0.5, 0.0, 0.0, 0.25), 0.8, 0.25) and c.dim_scale[3] == 0.0 and c.decay == 0.8 and c.gripper_penalty == 0.25
    assert host.Coherence(ONES, 1).gripper_penalty == 0.0
    for scale in ([1] * 5, [1] * 7, [1, 1, 1, 1, 1, -1], [1, 1, 1, 1, 1, float("nan")], [1, 1, 1, 1, 1, float("inf")], "abc", None, 1.0,
                  [1, 1, 1, 1, 1, 1e39]):
        with pytest.raises(CoverError, match="dim_scale"):
            host.Coherence(scale, 0.8)
    for decay in (0, -0.1, 1.0001, float("nan"), float("inf"), True, "1", None):
        with pytest.raises(CoverError, match="decay"):
            host.Coherence(ONES, decay)
    for pen in (-0.1, float("nan"), float("inf"), 1e39, True, "0", None):
        with pytest.raises(CoverError, match="gripper_penalty"):
            host.Coherence(ONES, 0.8, pen)
    with pytest.raises(TypeError):
        host.Coherence(ONES)                                               # no default decay
    kw = c.kwargs("cpu", 4)                                                # the uploads, here to the host
    assert set(kw) == {"step_weight", "dim_scale", "gripper_penalty"} and kw["gripper_penalty"] == 0.25
    assert np.array_equal(_bits(kw["step_weight"].numpy()), _bits(host.coherence_step_weights(4, 0.8)))
    assert kw["dim_scale"].dtype == torch.float32 and kw["dim_scale"].tolist() == [1.0, 1.0, 0.5, 0.0, 0.0, 0.25]
    assert c.kwargs("cpu", 4)["step_weight"] is kw["step_weight"] and c.scale_on("cpu") is kw["dim_scale"]   # one upload per device
    assert c.steps_on("cpu", 5) is not kw["step_weight"] and tuple(c.steps_on("cpu", 5).shape) == (5,)
    for text in (host.Coherence.__doc__, host.coherence_step_weights.__doc__):
        assert "recommended" in text


# ------------------------------------------------------------------------------------------------ binding
def test_binding_mirrors_the_header():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_coherence_args"] is L.CoherenceArgs
    for sym in ("cover_coherence_prior_tokens", "cover_coherence_prior_actions"):
        assert L.SYMBOLS[sym] == (C.c_int, [C.POINTER(L.CoherenceArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_coherence_prior_tokens(const cover_coherence_args* args, void* stream);" in hdr
    assert "int cover_coherence_prior_actions(const cover_coherence_args* args, void* stream);" in hdr
    body = hdr[hdr.index("typedef struct cover_coherence_args {"):hdr.index("} cover_coherence_args;")]
    body = re.sub(r"/\*.*?\*/", "", body)
    pos = [re.search(rf"\b{name}\b", body).start() for name, _ in L.CoherenceArgs._fields_]   # the header's fields in the header's order
    assert pos == sorted(pos)
    assert C.sizeof(L.CoherenceArgs) == 152
    if os.path.exists(L.LIB_PATH):                                         # cover_sizeof and cover_abi_version are host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_coherence_prior_tokens") and hasattr(h, "cover_coherence_prior_actions")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_coherence_args") == C.sizeof(L.CoherenceArgs)
        assert h.cover_sizeof(b"cover_smooth_args") == 112                 # no existing struct changes size
        assert h.cover_abi_version() == 1


def test_kernel_file_shares_the_token_rule():
    csrc = os.path.join(ROOT, "cover_vla_amd", "csrc")
    text = open(os.path.join(csrc, "coherence.hip")).read()
    rows = open(os.path.join(csrc, "chunk_rows.h")).read()                 # the row source holds the token rule, once
    assert '#include "chunk_rows.h"' in text and "chunk_stage_rows(" in text and "tok_vocab -" not in text and "centers[" not in text
    assert rows.count("tok_vocab -") == 1 and "s.value(" in rows[rows.index("void chunk_stage_rows("):]
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.lower().replace("no atomics", "")
    assert "powf" not in text and "fmaf" not in text
    assert " coherence.hip " in open(os.path.join(csrc, "Makefile")).read()
    capi = open(os.path.join(csrc, "capi.hip")).read()
    assert "COHERENCE_LIMITS" in capi and "SZ(cover_coherence_args)" in capi


# ------------------------------------------------------------------------------------------------ the wrappers' checks
def test_ops_wrappers_reject_bad_arguments_before_any_launch():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    x = torch.zeros(6, 2, 7)
    tok = torch.zeros(6, 14, dtype=torch.int64)
    cen = torch.zeros(255)
    ref, w, sw = torch.zeros(3, 4, 7), torch.ones(3), torch.ones(2)
    ok = dict(step_weight=sw, dim_scale=ONES)
    bad = [
        (dict(group_rows=4), "group_rows"), (dict(group_rows=0), "group_rows"), (dict(group_rows=2.0), "integers"),
        (dict(ref=torch.zeros(3, 4, 6)), "ref must"), (dict(ref=torch.zeros(3, 4, 7, dtype=torch.float64)), "ref must"),
        (dict(ref=torch.zeros(4, 3, 4, 7)), "per-prompt"), (dict(ref=torch.zeros(3, 65, 7)), "hr"), (dict(ref=ref.numpy()), "ref must"),
        (dict(ref=torch.zeros(3, 8, 7)[:, ::2]), "ref must"),
        (dict(shift=4), "shift"), (dict(shift=-1), "shift"), (dict(shift=True), "integers"),
        (dict(ref_weight=torch.ones(4)), "ref_weight"), (dict(ref_weight=torch.ones(3, dtype=torch.float64)), "ref_weight"),
        (dict(ref_weight=torch.ones(3, 3)), "ref_weight"),
        (dict(step_weight=torch.ones(3)), "step_weight"), (dict(step_weight=[1.0, 1.0]), "step_weight"),
        (dict(dim_scale=[1] * 5), "dim_scale"), (dict(dim_scale=[1, 1, 1, 1, 1, -1]), "dim_scale"),
        (dict(gripper_penalty=-1.0), "gripper_penalty"), (dict(gripper_penalty=float("nan")), "gripper_penalty"),
        (dict(gripper_penalty=True), "gripper_penalty"),
    ]
    for over, msg in bad:
        kw = dict(dict(group_rows=3, ref=ref, ref_weight=w, shift=0, **ok), **over)
        S, r, rw = kw.pop("group_rows"), kw.pop("ref"), kw.pop("ref_weight")
        with pytest.raises(CoverError, match=msg):
            ops.coherence_prior_actions(x, S, r, rw, **kw)
        with pytest.raises(CoverError, match=msg):
            ops.coherence_prior_tokens(tok, S, r, rw, cen, 32000, steps=2, **kw)
    with pytest.raises(CoverError, match="device tensors"):                # everything else is in order: there is no CPU path
        ops.coherence_prior_actions(x, 3, ref, w, **ok)
    with pytest.raises(CoverError, match="actions must"):
        ops.coherence_prior_actions(torch.zeros(6, 2, 6), 3, ref, w, **ok)
    with pytest.raises(CoverError, match="steps"):
        ops.coherence_prior_tokens(tok, 3, ref, w, cen, 32000, steps=3, **ok)
    with pytest.raises(TypeError):
        ops.coherence_prior_actions(x, 3, ref, w, dim_scale=ONES)          # no default step weights
    with pytest.raises(TypeError):
        ops.coherence_prior_actions(x, 3, ref, w, step_weight=sw)          # no default scale


def test_policy_entry_points_exist_and_check_their_record():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0 import PI0Policy
    assert callable(OpenVLA.coherence_prior) and callable(PI0Policy.commit)
    with pytest.raises(CoverError, match="host.Coherence"):
        OpenVLA.coherence_prior(None, torch.zeros(2, 7, dtype=torch.int64), 2, dict(decay=0.5))
    c = host.Coherence(ONES, 0.5)
    with pytest.raises(CoverError, match="exactly one"):
        OpenVLA.coherence_prior(None, torch.zeros(2, 7, dtype=torch.int64), 2, c)
    with pytest.raises(CoverError, match="exactly one"):
        OpenVLA.coherence_prior(None, torch.zeros(2, 7, dtype=torch.int64), 2, c, ref_tokens=torch.zeros(1, 7, dtype=torch.int64),
                                ref_actions=torch.zeros(1, 1, 7))
