"""Shared prefill of pi0-FAST candidates, host side: the grouping rule (pi0fast.prefix_groups), the feedback rule of
tests/feedback_ref.py (the numpy reference of cover_decode_feedback), the binding of the new entry point and the defaults of the new
arguments. Nothing here needs a GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from tests import feedback_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ prefix_groups
def _rows(*rows):
    L = max(len(r) for r in rows)
    tok = np.zeros((len(rows), L), dtype=np.int64)
    pad = np.zeros((len(rows), L), dtype=np.int64)
    for i, r in enumerate(rows):
        tok[i, :len(r)] = r
        pad[i, :len(r)] = 1
    return tok, pad


def test_prefix_groups_first_occurrence_order():
    from cover_vla_amd.pi0fast import prefix_groups
    a, b, c = [9, 8, 7], [1, 2], [5, 5, 5, 5]
    tok, pad = _rows(a, b, a, c, b, a, c)                       # interleaved duplicates; `a` sorts last but occurs first
    first, slot = prefix_groups(tok, pad)
    assert first.tolist() == [0, 1, 3] and slot.tolist() == [0, 1, 0, 2, 1, 0, 2]
    assert first.dtype == np.int64 and slot.dtype == np.int64
    assert np.array_equal(slot[first], np.arange(3))            # the representatives are their own groups, in order
    assert np.array_equal(tok[first][slot], tok) and np.array_equal(pad[first][slot], pad)
    # tensors in, the same answer
    f2, s2 = prefix_groups(torch.from_numpy(tok), torch.from_numpy(pad))
    assert np.array_equal(f2, first) and np.array_equal(s2, slot)
    f3, s3 = prefix_groups(torch.from_numpy(tok), torch.from_numpy(pad).to(torch.bool))
    assert np.array_equal(f3, first) and np.array_equal(s3, slot)


def test_prefix_groups_pad_mask_distinguishes_rows():
    from cover_vla_amd.pi0fast import prefix_groups
    tok = np.array([[4, 5, 0], [4, 5, 0], [4, 5, 0]], dtype=np.int64)
    pad = np.array([[1, 1, 0], [1, 1, 1], [1, 1, 0]], dtype=np.int64)     # row 1: the trailing 0 is a real token
    first, slot = prefix_groups(tok, pad)
    assert first.tolist() == [0, 1] and slot.tolist() == [0, 1, 0]


def test_prefix_groups_identity_and_single_group():
    from cover_vla_amd.pi0fast import prefix_groups
    g = np.random.default_rng(3)
    tok = g.permutation(40 * 6).reshape(40, 6).astype(np.int64)          # all entries distinct: all rows distinct
    first, slot = prefix_groups(tok, np.ones_like(tok))
    assert np.array_equal(first, np.arange(40)) and np.array_equal(slot, np.arange(40))
    one = np.tile(tok[:1], (7, 1))
    first, slot = prefix_groups(one, np.ones_like(one))
    assert first.tolist() == [0] and slot.tolist() == [0] * 7
    first, slot = prefix_groups(tok[:1], np.ones_like(tok[:1]))
    assert first.tolist() == [0] and slot.tolist() == [0]
    with pytest.raises(ValueError):
        prefix_groups(tok, np.ones((40, 5), dtype=np.int64))


def test_prefix_groups_is_the_greedy_ordering_rule():
    """The expressions of the greedy de-duplication in generate_tokens, on random rows with many repeats."""
    from cover_vla_amd.pi0fast import prefix_groups
    g = np.random.default_rng(11)
    base = g.integers(0, 50, size=(5, 4))
    tok = base[g.integers(0, 5, size=33)]
    pad = np.ones_like(tok)
    key = np.concatenate([tok, pad], axis=1)
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    f, s = prefix_groups(tok, pad)
    assert np.array_equal(f, first[order]) and np.array_equal(s, rank[inv.reshape(-1)])
    assert np.array_equal(f, np.sort(f)) and all(int(f[p]) == int(np.nonzero(s == p)[0][0]) for p in range(len(f)))


# ------------------------------------------------------------------------------------------------ the feedback rule
def test_feedback_pad_after_eos_and_live():
    EOS, PAD = 1, 0
    picks = np.array([[5, 1, 7, 8],          # EOS at step 1: pad from step 2
                      [6, 6, 6, 6],          # never finishes
                      [1, 9, 9, 9],          # EOS at once
                      [3, 4, 5, 1]])         # EOS at the last step
    out, done, _, live = F.run(picks, EOS, PAD)
    assert out.tolist() == [[5, 1, 0, 0], [6, 6, 6, 6], [1, 0, 0, 0], [3, 4, 5, 1]]
    assert done.tolist() == [True, False, True, True]
    assert live.tolist() == [3, 2, 2, 1] and live.dtype == np.int32
    # eos = -1: nothing finishes, every pick is emitted
    out, done, _, live = F.run(picks, -1, PAD)
    assert np.array_equal(out, picks) and not done.any() and live.tolist() == [4, 4, 4, 4]


def test_feedback_force_overrides_pick_not_pad():
    EOS, PAD = 1, 0
    picks = np.array([[5, 5, 5, 5], [1, 1, 1, 1]])
    force = np.array([[7, 1, 8, 9], [2, 3, 1, 4]])
    out, done, _, live = F.run(picks, EOS, PAD, force=force)
    assert out.tolist() == [[7, 1, 0, 0], [2, 3, 1, 0]]          # the forced token decides, the picked EOS of row 1 does not
    assert done.all() and live.tolist() == [2, 1, 0, 0]


def test_feedback_finished_rows_score_zero():
    EOS, PAD = 1, 0
    picks = np.array([[5, 1, 7], [6, 6, 6]])
    lps = np.array([[-1.5, -0.25, -3.0], [-2.0, -np.inf, -0.5]], dtype=np.float32)
    out, _, lp_out, _ = F.run(picks, EOS, PAD, lps=lps)
    assert lp_out.dtype == np.float32
    assert lp_out[0].tolist() == [-1.5, -0.25, 0.0]              # the EOS itself is a choice, the pad after it is not
    assert lp_out[1, 0] == -2.0 and np.isneginf(lp_out[1, 1]) and lp_out[1, 2] == -0.5
    # one step in place: the state carries over
    done = np.array([True, False])
    tok = np.full((2, 2), -7, dtype=np.int64)
    lpo = np.full((2, 2), 9.0, dtype=np.float32)
    live = np.zeros(2, dtype=np.int32)
    t = F.feedback_step([4, 1], done, tok, 1, EOS, PAD, lp=np.array([-1.0, -2.0], dtype=np.float32), lp_out=lpo, live=live)
    assert t.tolist() == [0, 1] and tok.tolist() == [[-7, 0], [-7, 1]] and lpo.tolist() == [[9.0, 0.0], [9.0, -2.0]]
    assert done.tolist() == [True, True] and live.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ binding and signatures
def test_struct_mirror_and_symbol():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_decode_feedback_args"] is L.DecodeFeedbackArgs and "cover_decode_feedback" in L.SYMBOLS
    names = [f[0] for f in L.DecodeFeedbackArgs._fields_]
    assert names == ["pick", "force", "force_stride", "lp", "lp_out", "ld_lp", "done", "tok_out", "ld_tok", "eos", "pad", "table",
                     "vocab", "dim", "scale", "x_out", "ldo", "live", "rows"]
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    body = hdr[hdr.index("typedef struct cover_decode_feedback_args {"):hdr.index("} cover_decode_feedback_args;")]
    marks = {"lp": " lp;", "eos": " eos, pad;", "pad": " pad;", "vocab": " vocab, dim;", "dim": " dim;", "done": " done;", "rows": "int rows;"}
    pos = [body.index(marks.get(n, n + ";")) for n in names]
    assert pos == sorted(pos)
    assert "int cover_decode_feedback(const cover_decode_feedback_args* args, void* stream);" in hdr
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_decode_feedback")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_decode_feedback_args") == C.sizeof(L.DecodeFeedbackArgs)


def test_decode_feedback_has_no_cpu_path():
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError
    pick = torch.zeros(2, dtype=torch.int64)
    done = torch.zeros(2, dtype=torch.bool)
    out = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(CoverError):
        ops.decode_feedback(pick, done, out, 0, 1, 0)
    assert not out.any()


def test_signatures_default_to_off():
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTTokens
    assert inspect.signature(PI0FASTTokens.generate_tokens).parameters["share_prefix"].default is False
    assert PI0FASTConfig().share_prefix is False
    assert inspect.signature(PI0FASTTokens.__init__).parameters["max_prompts"].default is None
    from cover_vla_amd import ops
    p = inspect.signature(ops.decode_feedback).parameters
    assert list(p)[:6] == ["pick", "done", "tok_out", "step", "eos", "pad"]
    assert all(p[n].default is None for n in ("force", "lp", "lp_out", "table", "x_out", "live"))
