"""Beam search, the part that needs no GPU: the references of tests/beam_ref.py against exhaustive enumeration and step-wise arg-max, the
tie and padding rules of the merge on constructed inputs, the backtrack and gather references, and the binding of the three entry points."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from tests import beam_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float("-inf")


def _tables(V, S, seed):
    """Random logits for every prefix: tables[i] has shape [V] * (i + 1)."""
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 2.0, size=(V,) * (i + 1)).astype(np.float32) for i in range(S)]


def _step_logits(tables_of_group, B):
    def f(prefixes):
        i = prefixes.shape[1]
        return np.stack([tables_of_group[r // B][i][tuple(np.clip(prefixes[r], 0, None))] for r in range(prefixes.shape[0])])
    return f


def test_beam_covering_every_prefix_is_the_exhaustive_top_b():
    V, S = 5, 3
    B = V * V
    tabs = [_tables(V, S, 11), _tables(V, S, 12)]
    tokens, logprobs, scores, _ = BR.search(_step_logits(tabs, B), 2, B, S, 0, V)
    for g in range(2):
        every = []
        for seq in itertools.product(range(V), repeat=S):
            s, lps = np.float32(0.0), []
            for i in range(S):
                order, lp = BR.topn_lists(tabs[g][i][seq[:i]][None], 0, V, V)        # the row's full sorted list
                lps.append(lp[0][list(order[0]).index(seq[i])])
                s = np.float32(s + lps[-1])
            every.append((s, seq, lps))
        every.sort(key=lambda e: -float(e[0]))
        top = every[:B + 1]
        assert len({float(e[0]) for e in top}) == B + 1, "the case must have no exact score tie at the cut"
        for r in range(B):
            o = g * B + r
            assert tuple(tokens[o]) == top[r][1], (g, r)
            assert scores[o].tobytes() == top[r][0].tobytes() and logprobs[o].tobytes() == np.array(top[r][2], np.float32).tobytes()


def test_one_beam_is_stepwise_argmax():
    V, S, G = 11, 4, 3
    tabs = [_tables(V, S, 20 + g) for g in range(G)]
    tokens, logprobs, scores, parents = BR.search(_step_logits(tabs, 1), G, 1, S, 0, V)
    assert (parents == 0).all()
    for g in range(G):
        seq = []
        for i in range(S):
            seq.append(int(np.argmax(tabs[g][i][tuple(seq)])))
        assert tokens[g].tolist() == seq
        s = np.float32(0.0)
        for lp in logprobs[g]:
            s = np.float32(s + lp)
        assert s.tobytes() == scores[g].tobytes()


def test_search_output_is_the_prefixes_it_grew():
    V, S, B, G = 7, 4, 3, 2
    tabs = [_tables(V, S, 30 + g) for g in range(G)]
    tokens, logprobs, scores, parents = BR.search(_step_logits(tabs, B), G, B, S, 0, V)
    assert any((p != np.arange(G * B) % B).any() for p in parents[1:]), "a step with a non-identity parent is what the backtrack is for"
    for g in range(G):
        rows = tokens[g * B:(g + 1) * B]
        assert len({tuple(r) for r in rows}) == B and (np.diff(scores[g * B:(g + 1) * B]) <= 0).all()
        for r in rows:                                                   # each step's log-probability is that of its own prefix's row
            o = g * B + rows.tolist().index(r.tolist())
            for i in range(S):
                tok, lp = BR.topn_lists(tabs[g][i][tuple(r[:i])][None], 0, V, V)
                assert logprobs[o, i] == lp[0][tok[0].tolist().index(r[i])]


def test_merge_tie_rule():
    tok = np.array([[10, 11], [20, 21]], np.int64)
    # equal scores across beams (equal cum, equal lp): the lower beam first
    p, t, f, c, l = BR.merge([0.0, 0.0], tok, np.array([[-1.0, -2.0], [-1.0, -2.0]], np.float32), 2, 5)
    assert p.tolist() == [0, 1] and t.tolist() == [10, 20] and f.tolist() == [10, 20] and c.tolist() == [-1.0, -1.0] and l.tolist() == [-1.0, -1.0]
    # equal scores inside a row: the lower rank first, and the row beats an equal later row
    p, t, _, c, _ = BR.merge([0.0, 0.0], tok, np.array([[-1.0, -1.0], [-1.0, -3.0]], np.float32), 2, 5)
    assert p.tolist() == [0, 0] and t.tolist() == [10, 11] and c.tolist() == [-1.0, -1.0]
    # equal scores from different (cum, lp) pairs, and -0.0 == +0.0
    p, t, _, c, _ = BR.merge([-1.0, -2.0], tok, np.array([[-2.0, -4.0], [-1.0, -1.5]], np.float32), 2, 5)
    assert p.tolist() == [0, 1] and t.tolist() == [10, 20] and c.tolist() == [-3.0, -3.0]
    p, t, _, _, _ = BR.merge([-0.0, 0.0], tok, np.array([[-0.0, -9.0], [0.0, -9.0]], np.float32), 2, 5)
    assert p.tolist() == [0, 1] and t.tolist() == [10, 20]
    # a higher score wins whatever the beam
    p, t, _, c, _ = BR.merge([-5.0, 0.0], tok, np.array([[-0.5, -1.0], [-0.25, -8.0]], np.float32), 2, 5)
    assert p.tolist() == [1, 0] and t.tolist() == [20, 10] and c.tolist() == [-0.25, -5.5]


def test_merge_dead_beams_and_padding():
    tok = np.array([[4, 5, -1], [6, 7, 8], [9, 1, 2]], np.int64)
    lp = np.array([[-1.0, -2.0, NINF], [-0.1, -0.2, -0.3], [-0.1, -0.2, -0.3]], np.float32)
    p, t, f, c, l = BR.merge(np.array([0.0, NINF, np.nan], np.float32), tok, lp, 3, 99)
    assert p.tolist() == [0, 0, -1] and t.tolist() == [4, 5, -1] and f.tolist() == [4, 5, 99]
    assert c.tolist() == [-1.0, -2.0, NINF] and l.tolist() == [-1.0, -2.0, NINF]
    # the step-0 state: one live beam fills the group from its own list
    p, t, _, c, _ = BR.merge(np.array([0.0, NINF, NINF], np.float32), np.array([[6, 7, 8]] * 3, np.int64), np.array([[-0.1, -0.2, -0.3]] * 3, np.float32), 3, 0)
    assert p.tolist() == [0, 0, 0] and t.tolist() == [6, 7, 8] and c.tolist() == [np.float32(-0.1), np.float32(-0.2), np.float32(-0.3)]
    # nothing live
    p, t, f, c, _ = BR.merge(np.array([NINF, NINF], np.float32), tok[:2, :2], lp[:2, :2], 2, 3)
    assert p.tolist() == [-1, -1] and t.tolist() == [-1, -1] and f.tolist() == [3, 3] and c.tolist() == [NINF, NINF]


def test_backtrack_reference():
    parent = np.array([[0, 0], [1, 0], [1, 1]], np.int32)          # S = 3, one group of B = 2
    token = np.array([[10, 11], [20, 21], [30, 31]], np.int64)
    lp = -np.arange(6, dtype=np.float32).reshape(3, 2)
    t, l = BR.backtrack(parent, token, lp, 2)
    assert t.tolist() == [[10, 21, 30], [10, 21, 31]] and l.tolist() == [[-0.0, -3.0, -4.0], [-0.0, -3.0, -5.0]]
    parent[1, 1] = -1                                              # the chain of both final beams breaks at step 1: step 0 stays -1 / -inf
    t, l = BR.backtrack(parent, token, lp, 2)
    assert t.tolist() == [[-1, 21, 30], [-1, 21, 31]] and l[:, 0].tolist() == [NINF, NINF]


def test_gather_reference():
    k = [np.arange(4 * 8 * 2 * 8, dtype=np.float32).reshape(4, 8, 2, 8)]
    vt = [np.arange(4 * 2 * 8 * 8, dtype=np.float32).reshape(4, 2, 8, 8) + 1000]
    ko, vo = BR.gather(k, vt, [0, 0, -1, 4], [2, 3, 1, 1], 3, 4)
    assert (ko[0][2, :3] == k[0][0, :3]).all() and (ko[0][3, :3] == k[0][0, :3]).all() and (ko[0][2, 3:] == k[0][2, 3:]).all()
    assert (vo[0][3, :, :, :3] == vt[0][0, :, :, :3]).all() and (vo[0][3, :, :, 3:] == vt[0][3, :, :, 3:]).all()
    assert (ko[0][:2] == k[0][:2]).all() and (vo[0][:2] == vt[0][:2]).all()


def test_binding_mirrors_the_header():
    from cover_vla_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    for sym, st in (("cover_beam_merge", L.BeamMergeArgs), ("cover_kv_gather_slots", L.KvGatherSlotsArgs), ("cover_beam_backtrack", L.BeamBacktrackArgs)):
        assert L._STRUCTS[sym + "_args"] is st and L.SYMBOLS[sym] == (C.c_int, [C.POINTER(st), C.c_void_p])
        assert f"int {sym}(const {sym}_args* args, void* stream);" in hdr
    assert C.sizeof(L.BeamMergeArgs) == 96 and C.sizeof(L.KvGatherSlotsArgs) == 96 and C.sizeof(L.BeamBacktrackArgs) == 56
    if os.path.exists(L.LIB_PATH):                                 # cover_sizeof is host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        h.cover_sizeof.restype = C.c_size_t
        for sym, st in (("cover_beam_merge", L.BeamMergeArgs), ("cover_kv_gather_slots", L.KvGatherSlotsArgs), ("cover_beam_backtrack", L.BeamBacktrackArgs)):
            assert hasattr(h, sym) and h.cover_sizeof((sym + "_args").encode()) == C.sizeof(st)


def test_wrappers_reject_bad_arguments_before_any_launch():
    from cover_vla_amd import _lib as L, ops
    cum, tok, lp = torch.zeros(4), torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 2)
    for bad in (lambda: ops.beam_merge(cum, tok, lp, 2, 0),                                  # host tensors: there is no CPU path
                lambda: ops.beam_merge(cum, tok, lp, 0, 0), lambda: ops.beam_merge(cum, tok, lp, 65, 0),
                lambda: ops.beam_merge(cum, tok, lp, 3, 0), lambda: ops.beam_merge(cum, tok, lp, 2, -1),
                lambda: ops.beam_merge(cum.double(), tok, lp, 2, 0), lambda: ops.beam_merge(cum, tok.int(), lp, 2, 0),
                lambda: ops.beam_merge(cum, tok, lp, 2, 0, out_cum=cum),
                lambda: ops.beam_backtrack(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 4), 2),
                lambda: ops.beam_backtrack(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 4), 3),
                lambda: ops.beam_backtrack(torch.zeros(3, 4, dtype=torch.int32), torch.zeros(4, 3, dtype=torch.int64), torch.zeros(3, 4), 2),
                lambda: ops.kv_gather_slots(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                                            torch.zeros(3, dtype=torch.int32), 1, k_offset=0, vt_offset=0, k_slot_stride=1024, vt_slot_stride=1024,
                                            n_slots=4, cap=32, Hkv=2, D=16),
                lambda: ops.kv_gather_slots(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32),
                                            torch.zeros(3, dtype=torch.int32), 1, k_offset=0, vt_offset=0, k_slot_stride=1024, vt_slot_stride=1024,
                                            n_slots=4, cap=32, Hkv=2, D=16)):
        with pytest.raises(L.CoverError):
            bad()
