"""Diverse candidate subsets without a GPU: the reference of tests/diverse_ref.py against an independent float64 brute-force greedy on
inputs where fp32 is exact, hand-checked cases, special values, the case table, the binding, and the checks of the host layer
(host.Diversity, host.spread_scores, the ops wrappers, OpenVLA.diverse_subset and PI0Policy.diverse) that need no device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import coherence_ref as CR
from tests import diverse_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ONES = (1.0,) * 6
KEYS = ("picked", "count", "value", "dist", "assign", "row_dist")


def _bits(x):
    x = np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _ref(x, S, m, quality=None, weight=0.0, cover=-1.0, decay=1.0, dim_scale=ONES, penalty=0.0):
    x = np.asarray(x, dtype=F32)
    return DR.reference(x, S, m, None if quality is None else np.asarray(quality, dtype=F32), weight, cover,
                        DR.step_weights(x.shape[1], decay), dim_scale, penalty)


# ------------------------------------------------------------------------------------------------ 1. against a float64 brute force
def _brute_force(x, S, m, quality, weight, cover, decay, dim_scale, penalty):
    """An independent float64 greedy: the whole pair matrix first (ordinary sums), eligibility stated as "every element the distance
    reads is finite", the pick as a Python max over (value, -index) tuples."""
    x = np.asarray(x, dtype=np.float64)
    N, h = x.shape[:2]
    G = N // S
    sc = np.asarray(dim_scale, dtype=np.float64)
    sw = np.float64(decay) ** np.arange(h)
    out = dict(picked=np.full((G, m), -1, np.int32), count=np.zeros(G, np.int32), value=np.full((G, m), np.nan), dist=np.full((G, m), np.inf),
               assign=np.full(N, -1, np.int32), row_dist=np.full(N, np.inf))
    for g in range(G):
        xs = x[g * S:(g + 1) * S]
        q = np.zeros(S) if quality is None else np.asarray(quality[g * S:(g + 1) * S], dtype=np.float64)
        read = np.where(sc != 0, xs[..., :6], 0.0)
        e = (((read[:, None] - read[None]) * sc) ** 2).sum(axis=3)
        e = e + penalty * ((xs[:, None, :, 6] >= 0.5) != (xs[None, :, :, 6] >= 0.5))
        D = (e * sw).sum(axis=2)
        eligible = [bool(np.isfinite(read[i]).all() and not np.isnan(q[i])) for i in range(S)]
        mind, picks = [np.inf] * S, []
        for k in range(m):
            cands = []
            for i in range(S):
                if eligible[i] and i not in picks and mind[i] > cover:
                    v = q[i] if (k == 0 or weight == 0) else q[i] + weight * mind[i]
                    if not np.isnan(v):
                        cands.append((v, -i))
            if not cands:
                break
            v, neg = max(cands)
            p = -neg
            out["picked"][g, k], out["value"][g, k], out["dist"][g, k] = g * S + p, v, mind[p]
            picks.append(p)
            for i in range(S):
                if D[i, p] < mind[i]:
                    mind[i] = D[i, p]
                    out["assign"][g * S + i] = k
        out["count"][g] = len(picks)
        out["row_dist"][g * S:(g + 1) * S] = mind
    return out


# (G, S, m, h, decay, scale, weight, penalty, cover, quality given): fp32 is exact on all of them (see the test)
EXACT = [(1, 1, 1, 1, 1.0, 1.0, 1.0, 0.0, -1.0, 0), (3, 4, 4, 1, 1.0, 2.0, 0.5, 0.25, -1.0, 1), (2, 9, 9, 2, 0.5, 1.0, 0.0, 0.0, -1.0, 1),
         (2, 17, 6, 3, 1.0, 0.5, 2.0, 0.5, 0.0, 1), (1, 33, 12, 8, 0.5, 1.0, 0.5, 0.25, -1.0, 1), (2, 12, 12, 4, 0.5, 2.0, 1.0, 0.0, 0.0, 0),
         (1, 40, 40, 2, 1.0, 1.0, 0.25, 1.0, 1.0, 1), (2, 20, 5, 50, 1.0, 1.0, 1.0, 0.25, -1.0, 0), (1, 16, 16, 8, 0.5, 0.5, 4.0, 0.0, 0.5, 1)]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "-".join(map(str, c)))
def test_reference_matches_a_float64_brute_force_where_fp32_is_exact(case):
    """Values on a grid of 1/64 in [-1, 1], one power of two as the scale of the dims that count, weight and penalty powers of two, decay
    1 or 0.5 (h <= 8), integer qualities: every product and sum of the specification is then exact in fp32, so the fp32 reference and
    the float64 greedy must agree on every output, ties included."""
    G, S, m, h, decay, scale, weight, penalty, cover, with_q = case
    assert decay == 1.0 or h <= 8
    rng = np.random.default_rng(hash(case[:4]) % 1000)
    x = (rng.integers(-64, 65, (G * S, h, 7)) / 64.0).astype(F32)
    x[..., 6] = rng.integers(0, 2, (G * S, h))
    for i in np.flatnonzero(rng.random(G * S) < 0.3):                      # duplicates inside the groups
        x[i] = x[(i // S) * S + rng.integers(0, S)]
    if S > 4:
        x[1, 0, 2] = np.nan                                                # a dim of scale 0: invisible
        x[2, h - 1, 6] = np.nan                                            # dim 6: invisible (class 0)
        x[3, 0, 0] = np.nan                                                # a dim that counts: never picked
    dim_scale = (scale, scale, 0.0, scale, scale, scale)
    quality = rng.integers(-3, 4, G * S).astype(F32) if with_q else None
    if with_q and S > 4:
        quality[4] = np.nan
    got = _ref(x, S, m, quality, weight, cover, decay, dim_scale, penalty)
    want = _brute_force(x, S, m, quality, weight, cover, decay, dim_scale, penalty)
    for k in KEYS:
        g, w = got[k], want[k]
        assert g.shape == w.shape, k
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if g.dtype == F32 else g == w   # float64 holds every fp32 value exactly
        assert same.all(), (k, g, w)
    if S > 4:
        assert 3 not in got["picked"] and (not with_q or 4 not in got["picked"])
        assert got["assign"][3] == -1 and np.isposinf(got["row_dist"][3])


# ------------------------------------------------------------------------------------------------ 2. hand-checked cases
def test_one_row_groups():
    x = np.arange(3 * 2 * 7, dtype=F32).reshape(3, 2, 7) / 64
    r = _ref(x, 1, 1, weight=1.0)
    assert r["picked"].tolist() == [[0], [1], [2]] and r["count"].tolist() == [1, 1, 1] and r["assign"].tolist() == [0, 0, 0]
    assert _bits(r["value"]).tolist() == [[0], [0], [0]] and np.isposinf(r["dist"]).all() and (r["row_dist"] == 0).all()


def test_all_rows_equal_with_cover_zero_gives_one_pick():
    x = np.tile(np.linspace(-0.5, 0.5, 14, dtype=F32).reshape(1, 2, 7), (6, 1, 1))
    r = _ref(x, 6, 4, weight=1.0, cover=0.0)
    assert r["count"].tolist() == [1] and r["picked"].tolist() == [[0, -1, -1, -1]]
    assert (_bits(r["value"])[0, 1:] == 0x7FC00000).all() and np.isposinf(r["dist"]).all()
    assert r["assign"].tolist() == [0] * 6 and (r["row_dist"] == 0).all()
    assert np.array_equal(DR.gathered(x, r["picked"], 6), x[[0, 0, 0, 0]])
    off = _ref(x, 6, 4, weight=1.0)                                        # the covering rule off: duplicates are picked, by index
    assert off["count"].tolist() == [4] and off["picked"].tolist() == [[0, 1, 2, 3]] and off["assign"].tolist() == [0] * 6
    assert off["dist"][0, 1:].tolist() == [0.0, 0.0, 0.0]


def test_weight_zero_picks_in_refines_rank_order():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (2 * 9, 2, 7)).astype(F32)
    q = np.array([0.5, -0.0, 2.0, 0.0, 2.0, -np.inf, np.inf, 0.25, -1.0] + [1.0] * 9, dtype=F32)
    r = _ref(x, 9, 9, quality=q, weight=0.0)
    # higher first, equal scores (-0 == +0) by ascending index
    assert r["picked"][0].tolist() == [6, 2, 4, 0, 7, 1, 3, 8, 5] and r["picked"][1].tolist() == list(range(9, 18))
    assert np.array_equal(_bits(r["value"][0]), _bits(q[[6, 2, 4, 0, 7, 1, 3, 8, 5]]))
    assert r["count"].tolist() == [9, 9] and r["assign"][:9].tolist() == [3, 5, 1, 6, 2, 8, 0, 4, 7]


def test_no_quality_and_weight_one_is_the_farthest_point_traversal_from_row_zero():
    # one dim, one step: positions 0, 1, 10, 4, 5, 10.5, 4 (x 1/16). From 0: the farthest is 10.5 (row 5); then the row farthest from
    # {0, 10.5}: 4 and 5 are min(4, 6.5) = 4 and min(5, 5.5) = 5 away -> row 4 (position 5); then {0, 5, 10.5}: position 1 is 1 away,
    # 10 is 0.5, both 4s are 1 -> a tie at squared distance (1/16)^2 between rows 1, 3 and 6: the lowest index, row 1; then row 3
    # (1/16 from position 5; row 6 equals it), and with cover_dist = 0 row 6 stays pickable only while its distance is > 0
    pos = np.array([0, 1, 10, 4, 5, 10.5, 4], dtype=F32) / 16
    x = np.zeros((7, 1, 7), dtype=F32)
    x[:, 0, 0] = pos
    r = _ref(x, 7, 7, weight=1.0)
    assert r["picked"][0].tolist() == [0, 5, 4, 1, 3, 2, 6]
    sq = lambda a: float(F32(a / 16) * F32(a / 16))
    assert r["dist"][0].tolist() == [np.inf, sq(10.5), sq(5), sq(1), sq(1), sq(0.5), 0.0]
    assert r["value"][0].tolist() == [0.0] + r["dist"][0].tolist()[1:]     # quality 0, weight 1
    assert r["assign"].tolist() == [0, 3, 5, 4, 2, 1, 4] and (r["row_dist"] == 0).all()   # row 6 is covered by slot 4 (row 3), strictly first
    c0 = _ref(x, 7, 7, weight=1.0, cover=0.0)
    assert c0["picked"][0].tolist() == [0, 5, 4, 1, 3, 2, -1] and c0["count"].tolist() == [6] and c0["assign"].tolist() == r["assign"].tolist()
    ball = _ref(x, 7, 7, weight=1.0, cover=sq(1))                          # every row within 1/16 of a pick: three picks cover the group
    assert ball["picked"][0].tolist() == [0, 5, 4, -1, -1, -1, -1] and ball["assign"].tolist() == [0, 0, 1, 2, 2, 1, 2]


def test_self_distance_and_pair_distance_are_coherences():
    c = dict(form="actions", shape=(2, 65, 9, 3), quality=1, weight=0.5, cover=-1.0)
    inp = DR.make_inputs(c)
    x = inp["actions"][:65]
    want = CR.pair_dists(x, x[7:8], inp["dim_scale"], inp["step_weight"], inp["penalty"])[:, 0]
    got = DR.dists(x, x[7], inp["dim_scale"], inp["step_weight"], inp["penalty"])
    assert np.array_equal(_bits(got), _bits(want))


# ------------------------------------------------------------------------------------------------ 3. special values
def test_nan_quality_or_nan_element_is_never_picked_and_invisible_nans_are_invisible():
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (8, 2, 7)).astype(F32)
    scale = (1.0, 1.0, 0.0, 0.5, 0.5, 0.25)
    clean = _ref(x, 8, 8, quality=np.arange(8, dtype=F32), weight=0.5, dim_scale=scale, penalty=0.25)
    assert clean["count"].tolist() == [8]
    q = np.arange(8, dtype=F32)
    q[7] = np.nan                                                          # the best row by quality
    r = _ref(x, 8, 8, quality=q, weight=0.5, dim_scale=scale, penalty=0.25)
    assert r["count"].tolist() == [7] and 7 not in r["picked"] and r["picked"][0, 7] == -1
    assert r["assign"][7] >= 0 and np.isfinite(r["row_dist"][7])           # its elements are finite: it has a nearest pick
    bad = x.copy()
    bad[6, 1, 4] = np.inf                                                  # inf - inf: the self-distance is NaN
    bad[5, 0, 0] = np.nan
    r = _ref(bad, 8, 8, quality=np.arange(8, dtype=F32), weight=0.5, dim_scale=scale, penalty=0.25)
    assert r["count"].tolist() == [6] and not {5, 6} & set(r["picked"][0].tolist())
    assert r["assign"][[5, 6]].tolist() == [-1, -1] and np.isposinf(r["row_dist"][[5, 6]]).all()
    hidden = x.copy()
    hidden[:, :, 2] = np.nan                                               # a dim of scale 0
    hidden[3, :, 6] = np.nan                                               # dim 6: class 0, as row 3's were
    hidden_ref = x.copy()
    hidden_ref[3, :, 6] = 0.0
    a = _ref(hidden, 8, 8, quality=np.arange(8, dtype=F32), weight=0.5, dim_scale=scale, penalty=0.25)
    b = _ref(hidden_ref, 8, 8, quality=np.arange(8, dtype=F32), weight=0.5, dim_scale=scale, penalty=0.25)
    for k in KEYS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert a["count"].tolist() == [8]


def test_invalid_dim_scale_gives_count_zero():
    x = np.random.default_rng(6).uniform(-1, 1, (6, 1, 7)).astype(F32)
    for v in (-1.0, np.nan, np.inf):
        r = _ref(x, 3, 2, weight=1.0, dim_scale=(1.0, 1.0, 1.0, v, 1.0, 1.0))
        assert r["count"].tolist() == [0, 0] and (r["picked"] == -1).all() and (r["assign"] == -1).all()
        assert np.isposinf(r["row_dist"]).all() and np.isposinf(r["dist"]).all() and (_bits(r["value"]) == 0x7FC00000).all()
        assert np.array_equal(DR.gathered(x, r["picked"], 3), x[[0, 0, 3, 3]])   # a group with no pick stores its row 0


def test_minus_inf_quality_meets_plus_inf_distance():
    x = np.zeros((3, 1, 7), dtype=F32)
    x[:, 0, 0] = [0.0, 0.5, 1.0]
    r = _ref(x, 3, 3, quality=[-np.inf, -np.inf, -np.inf], weight=1.0)     # pick 0: the quality alone, row 0; then -inf + finite = -inf
    assert r["picked"][0].tolist() == [0, 1, 2] and np.isneginf(r["value"]).all()


# ------------------------------------------------------------------------------------------------ 4. the case table
def test_case_table_names_what_it_says():
    for s in ((1, 1, 1, 1), (3, 4, 4, 1), (2, 63, 7, 2), (2, 64, 64, 1), (2, 65, 9, 3), (1, 1023, 5, 1), (1, 1025, 1025, 1), (1, 4096, 256, 1),
              (2, 37, 8, 50), (1, 8, 3, 64)):
        assert s in DR.SHAPES
    lo, hi = DR.boundary_shapes()
    assert lo in DR.SHAPES and hi in DR.SHAPES and hi[1] == lo[1] + 1 and lo[2:] == hi[2:]
    assert DR.lds_resident(*lo[1:]) and not DR.lds_resident(*hi[1:])
    assert DR.lds_resident(4096, 256, 1) and not DR.lds_resident(1030, 5, 6) and not DR.lds_resident(4096, 256, 8)
    src = open(os.path.join(ROOT, "cover_vla_amd", "csrc", "diverse.hip")).read()
    assert "#define DIVERSE_LDS_BUDGET (160 * 1024 - 256)" in src and DR.LDS_BUDGET == 160 * 1024 - 256
    assert "((size_t)stride + a->h + a->m) * sizeof(float)" in src and "(size_t)S * stride * sizeof(float)" in src
    assert any(DR.token_row_stride(s) > 7 * s[3] for s in DR.SHAPES)
    assert len(DR.cases(forms=("tokens",), shapes=(DR.SHAPES[0],))) == 8   # quality given / None x weight {0, 0.5} x cover_dist {-1, 0}
    assert DR.STRIDED in DR.shapes_of("actions") and DR.STRIDED not in DR.shapes_of("tokens")


@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_cases_of_the_table_are_not_vacuous(form):
    short = False
    for shape in ((2, 65, 9, 3), (2, 64, 64, 1), (3, 4, 4, 1)):
        for c in DR.cases(forms=(form,), shapes=(shape,)):
            r = DR.case_reference(c)
            assert (r["count"] >= 1).all()
            if c["cover"] == 0.0 and shape[2] == shape[1]:
                short = short or bool((r["count"] < shape[2]).any())       # the planted duplicates: count < m occurs
            if c["cover"] < 0 and form == "tokens" and not c["quality"]:
                assert (r["count"] == shape[2]).all()                      # no NaN anywhere: every slot is filled
    assert short
    full = DR.case_reference(dict(form="tokens", shape=(1, 1025, 1025, 1), quality=0, weight=0.5, cover=-1.0))
    assert sorted(full["picked"][0].tolist()) == list(range(1025))         # every row picked


# ------------------------------------------------------------------------------------------------ 5. the host layer
def test_diversity_record_checks_its_values():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    d = host.Diversity(8, 0.5, [1, 1, 0.5, 0, 0, 0.25], 0.8, 0.25)
    assert d == (8, 0.5, (1.0, 1.0, 0.5, 0.0, 0.0, 0.25), 0.8, 0.25, -1.0) and d.keep == 8 and d.cover_dist == -1.0
    assert host.Diversity(1, 0, ONES, 1, 0, cover_dist=0).cover_dist == 0.0 and host.Diversity(1, 0, ONES, 1, 0, -float("inf")).cover_dist < 0
    for keep in (0, -1, 4097, 2.0, True, "3", None):
        with pytest.raises(CoverError, match="keep"):
            host.Diversity(keep, 0.5, ONES, 0.8, 0.0)
    for w in (-0.5, float("nan"), float("inf"), 1e39, True, "1", None):
        with pytest.raises(CoverError, match="weight"):
            host.Diversity(4, w, ONES, 0.8, 0.0)
    for scale in ([1] * 5, [1, 1, 1, 1, 1, -1], [1, 1, 1, 1, 1, float("nan")], "abc", None):
        with pytest.raises(CoverError, match="dim_scale"):
            host.Diversity(4, 0.5, scale, 0.8, 0.0)
    for decay in (0, -0.1, 1.0001, float("nan"), float("inf"), True, None):
        with pytest.raises(CoverError, match="decay"):
            host.Diversity(4, 0.5, ONES, decay, 0.0)
    for pen in (-0.1, float("nan"), float("inf"), 1e39, True, None):
        with pytest.raises(CoverError, match="gripper_penalty"):
            host.Diversity(4, 0.5, ONES, 0.8, pen)
    for cd in (float("nan"), float("inf"), 1e39, True, "0", None):
        with pytest.raises(CoverError, match="cover_dist"):
            host.Diversity(4, 0.5, ONES, 0.8, 0.0, cd)
    with pytest.raises(TypeError):
        host.Diversity(4, 0.5, ONES, 0.8)                                  # no default penalty, decay, scale, weight or keep
    kw = d.kwargs("cpu", 4)
    assert set(kw) == {"weight", "cover_dist", "step_weight", "dim_scale", "gripper_penalty"}
    assert (kw["weight"], kw["cover_dist"], kw["gripper_penalty"]) == (0.5, -1.0, 0.25)
    assert np.array_equal(_bits(kw["step_weight"].numpy()), _bits(host.coherence_step_weights(4, 0.8)))
    coh = host.Coherence(d.dim_scale, 0.8, 0.25)                           # the uploads are Coherence's: one per device
    assert kw["step_weight"] is coh.steps_on("cpu", 4) and kw["dim_scale"] is coh.scale_on("cpu") and d.kwargs("cpu", 4)["dim_scale"] is kw["dim_scale"]
    assert "recommended" in host.Diversity.__doc__


def _subset(x, S, m, **kw):
    from cover_vla_amd import ops
    r = _ref(x, S, m, **kw)
    t = lambda k: torch.from_numpy(r[k])
    return ops.DiverseSubset(torch.from_numpy(DR.gathered(x, r["picked"], S)), t("picked"), t("count"), t("value"), t("dist"), t("assign"),
                             t("row_dist")), r


def test_spread_scores_on_cpu_tensors():
    from cover_vla_amd import host, ops
    assert ops.DiverseSubset._fields == ("rows", "picked", "count", "value", "dist", "assign", "row_dist")
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, (2 * 7, 1, 7)).astype(F32)
    x[3] = x[0]
    x[9, 0, 1] = np.nan                                                    # never picked, no nearest pick
    sub, r = _subset(x, 7, 3, weight=1.0, cover=0.0)
    assert sub.valid.dtype == torch.bool and torch.equal(sub.valid, sub.picked >= 0) and bool(sub.valid.all())
    kept = torch.tensor([1.0, 2.0, 3.0, 10.0, 20.0, 30.0])
    full = host.spread_scores(kept, sub, 7)
    assert tuple(full.shape) == (14,) and full.dtype == torch.float32
    for i in range(14):
        a = int(r["assign"][i])
        assert float(full[i]) == (-np.inf if a < 0 else float(kept[(i // 7) * 3 + a])), i
    assert float(full[9]) == -np.inf and float(full[3]) == float(full[0])  # a duplicate carries its original's score
    for g in range(2):                                                     # a picked row carries its own slot's score
        for k in range(3):
            assert float(full[int(r["picked"][g, k])]) == float(kept[g * 3 + k])
    # the grouped arg-max of the spread scores names a row assigned to the winning slot
    win = full.view(2, 7).argmax(dim=1)
    assert [int(r["assign"][g * 7 + int(win[g])]) for g in range(2)] == [2, 2]
    none, _ = _subset(x, 7, 3, weight=1.0, dim_scale=(1.0, -1.0, 1.0, 1.0, 1.0, 1.0))   # no pick at all
    assert not bool(none.valid.any()) and bool(torch.isneginf(host.spread_scores(kept, none, 7)).all())
    for bad in (kept[:5], kept.double(), kept.numpy()):
        with pytest.raises(ValueError, match="scores_kept"):
            host.spread_scores(bad, sub, 7)
    with pytest.raises(ValueError, match="group_rows"):
        host.spread_scores(kept, sub, 6)
    with pytest.raises(ValueError, match="group_rows"):
        host.spread_scores(kept, sub, 0)


def test_binding_mirrors_the_header():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_diverse_args"] is L.DiverseArgs
    for sym in ("cover_diverse_subset_tokens", "cover_diverse_subset_actions"):
        assert L.SYMBOLS[sym] == (C.c_int, [C.POINTER(L.DiverseArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_diverse_subset_tokens(const cover_diverse_args* args, void* stream);" in hdr
    assert "int cover_diverse_subset_actions(const cover_diverse_args* args, void* stream);" in hdr
    body = hdr[hdr.index("typedef struct cover_diverse_args {"):hdr.index("} cover_diverse_args;")]
    body = re.sub(r"/\*.*?\*/", "", body)
    pos = [re.search(rf"\b{name}\b", body).start() for name, _ in L.DiverseArgs._fields_]   # the header's fields in the header's order
    assert pos == sorted(pos)
    assert C.sizeof(L.DiverseArgs) == 152
    if os.path.exists(L.LIB_PATH):                                         # cover_sizeof is host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_diverse_subset_tokens") and hasattr(h, "cover_diverse_subset_actions")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_diverse_args") == C.sizeof(L.DiverseArgs)
        assert h.cover_sizeof(b"cover_coherence_args") == 152              # no existing struct changes size


def test_kernel_files_share_one_distance():
    csrc = os.path.join(ROOT, "cover_vla_amd", "csrc")
    shared = open(os.path.join(csrc, "chunk_dist.h")).read()
    assert "chunk_pair_dist_of(" in shared and "#pragma clang fp contract(off)" in shared
    for name in ("coherence.hip", "diverse.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "chunk_dist.h"' in text and "chunk_pair_dist" in text and "diff * sc" not in text, name
        assert "#pragma clang fp contract(off)" in text and "powf" not in text and "fmaf" not in text
    text = open(os.path.join(csrc, "diverse.hip")).read()
    rows = open(os.path.join(csrc, "chunk_rows.h")).read()                 # the row source holds the token rule, once
    assert '#include "chunk_rows.h"' in text and "aug_value(f, " in text and "chunk_src<T> f = {" in text and "centers[" not in text
    assert rows.count("tok_vocab -") == 1 and "aug_value(*this" in rows and shared.count("diff * sc") == 1
    assert "desc_key(" in text and "tok_vocab -" not in text and "atomic" not in text.lower()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert " diverse.hip " in make and " chunk_dist.h " in make and " chunk_rows.h " in make
    capi = open(os.path.join(csrc, "capi.hip")).read()
    assert "DIVERSE_LIMITS" in capi and "SZ(cover_diverse_args)" in capi


def test_ops_wrappers_reject_bad_arguments_before_any_launch():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    x = torch.zeros(6, 2, 7)
    tok = torch.zeros(6, 14, dtype=torch.int64)
    cen = torch.zeros(255)
    ok = dict(weight=0.5, step_weight=torch.ones(2), dim_scale=ONES)
    bad = [
        (dict(group_rows=4), "group_rows"), (dict(group_rows=0), "group_rows"), (dict(group_rows=2.0), "integers"),
        (dict(keep=0), "keep"), (dict(keep=4), "keep"), (dict(keep=True), "integers"),
        (dict(quality=torch.zeros(5)), "quality"), (dict(quality=torch.zeros(6, dtype=torch.float64)), "quality"), (dict(quality=[0.0] * 6), "quality"),
        (dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"), (dict(weight=True), "weight"),
        (dict(cover_dist=float("nan")), "cover_dist"), (dict(cover_dist=float("inf")), "cover_dist"), (dict(cover_dist=1e39), "cover_dist"),
        (dict(step_weight=torch.ones(3)), "step_weight"), (dict(step_weight=[1.0, 1.0]), "step_weight"),
        (dict(dim_scale=[1] * 5), "dim_scale"), (dict(dim_scale=[1, 1, 1, 1, 1, -1]), "dim_scale"),
        (dict(gripper_penalty=-1.0), "gripper_penalty"), (dict(gripper_penalty=float("inf")), "gripper_penalty"),
    ]
    for over, msg in bad:
        kw = dict(dict(group_rows=3, keep=2, **ok), **over)
        S, m = kw.pop("group_rows"), kw.pop("keep")
        with pytest.raises(CoverError, match=msg):
            ops.diverse_subset_actions(x, S, m, **kw)
        with pytest.raises(CoverError, match=msg):
            ops.diverse_subset_tokens(tok, S, m, cen, 32000, steps=2, **kw)
    with pytest.raises(CoverError, match="device tensors"):                # everything else is in order: there is no CPU path
        ops.diverse_subset_actions(x, 3, 2, **ok)
    with pytest.raises(CoverError, match="device tensors"):
        ops.diverse_subset_tokens(tok, 3, 2, cen, 32000, steps=2, cover_dist=-float("inf"), **ok)
    with pytest.raises(CoverError, match="actions must"):
        ops.diverse_subset_actions(torch.zeros(6, 2, 6), 3, 2, **ok)
    with pytest.raises(CoverError, match="steps"):
        ops.diverse_subset_tokens(tok, 3, 2, cen, 32000, steps=3, **ok)
    with pytest.raises(TypeError):
        ops.diverse_subset_actions(x, 3, 2, step_weight=torch.ones(2), dim_scale=ONES)   # no default weight


def test_policy_entry_points_check_their_record_before_anything_runs():
    from cover_vla_amd import host
    from cover_vla_amd._lib import CoverError
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0 import PI0Config, PI0Policy
    with pytest.raises(CoverError, match="host.Diversity"):
        OpenVLA.diverse_subset(None, torch.zeros(4, 7, dtype=torch.int64), 2, dict(keep=2))
    pol = PI0Policy(PI0Config(n_action_steps=2, chunk_size=4, tokenizer_max_length=8, resize_imgs_with_padding=None),
                    SimpleNamespace(dev="cpu"), None)
    assert pol.diverse is None and pol.last_diverse is None
    batch = {"observation.state": torch.zeros(6, 8)}
    pol.diverse = dict(keep=2)
    with pytest.raises(CoverError, match="host.Diversity"):
        pol.select_action(batch)
    pol.diverse = host.Diversity(7, 0.5, ONES, 0.8, 0.0)
    with pytest.raises(CoverError, match="keep = 7 exceeds the 6 rows"):   # no augment, no proposal prior: the batch is one prompt
        pol.select_action(batch)
    pol.proposal_prior = host.ProposalPrior(3, 1.0, 0.01)
    pol.diverse = host.Diversity(4, 0.5, ONES, 0.8, 0.0)
    with pytest.raises(CoverError, match="keep = 4 exceeds the 3 rows"):
        pol.select_action(batch)
    aug = host.Augment(3, 2, torch.zeros(2, 2, 2, 6))
    pol.diverse = host.Diversity(6, 0.5, ONES, 0.8, 0.0)
    with pytest.raises(CoverError, match="keep = 6 exceeds the 5 rows"):
        pol.select_action(batch, augment=aug)
    pol.last_diverse = object()
    pol.reset()
    assert pol.last_diverse is None and pol.diverse is not None            # reset() clears the result, not the setting
