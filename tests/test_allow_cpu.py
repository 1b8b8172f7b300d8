"""Allowed-token sets without a GPU: the host builder (ops.token_allow_sets), the FAST band helper, the struct mirror, and the float64
reference of tests/allow_ref.py itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import ops
from cover_vla_amd.pi0fast import fast_action_token_range, fast_tokens_to_paligemma_tokens
from tests import allow_ref as AR
from tests import sample_rows_ref as SR
from tests import sampling_ref as R


def _words(t):
    return t.view(torch.int32).numpy().view(np.uint32)


def test_builder_round_trip():
    vocab = 100
    sets = [[0, 31, 32, (60, 70)], [99], [(0, 100)], [(5, 5)]]
    b = ops.token_allow_sets(vocab, sets)
    assert b.dtype == torch.uint32 and tuple(b.shape) == (4, 4) and b.is_contiguous()
    w = _words(b)
    assert w[0].tolist() == [0x80000001, 0xF0000001, 0x0000003F, 0] and w[1].tolist() == [0, 0, 0, 1 << 3]
    assert w[2].tolist() == [0xFFFFFFFF] * 3 + [0xF] and not w[3].any()              # bits at or above vocab stay clear; an empty range
    for i, entries in enumerate(sets):                                             # bit (c & 31) of word (c >> 5), every column
        want = np.zeros(vocab, dtype=bool)
        for e in entries:
            if isinstance(e, tuple):
                want[e[0]:e[1]] = True
            else:
                want[e] = True
        got = np.array([(int(w[i, c >> 5]) >> (c & 31)) & 1 for c in range(vocab)], dtype=bool)
        assert np.array_equal(got, want), i
    rng = np.random.default_rng(3)
    on = rng.random((2, 257152)) < 0.5                                             # the wide vocabulary against the test-side packer
    big = ops.token_allow_sets(257152, [np.nonzero(on[0])[0].tolist(), np.nonzero(on[1])[0]])
    assert tuple(big.shape) == (2, 8036) and np.array_equal(_words(big), AR.pack_bits(on))
    for bad in ([-1], [100], [(0, 101)], [(-1, 4)], [(7, 3)], [(1, 2, 3)]):
        with pytest.raises(ValueError):
            ops.token_allow_sets(vocab, [[1], bad])
    with pytest.raises(ValueError):
        ops.token_allow_sets(vocab, [])
    h = ops.TokenAllow(b)
    assert h.n_sets == 4 and h.set_of_row is None
    for bits, sor in ((b.view(torch.int32).float(), None), (b[0], None), (b, torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(L.CoverError):
            ops.TokenAllow(bits, sor)


def test_fast_action_token_range():
    for vocab, fast, skip in ((257152, 2048, 128), (512, 64, 128), (300, 172, 128)):
        a, b = fast_action_token_range(vocab, fast, skip)
        ids = fast_tokens_to_paligemma_tokens(np.arange(fast), vocab, skip)
        assert b - a == fast and sorted(ids.tolist()) == list(range(a, b))
        assert a - 1 not in ids and b not in ids
    assert fast_action_token_range(257152, 2048) == (257152 - 128 - 2048, 257152 - 128)
    with pytest.raises(ValueError):
        fast_action_token_range(300, 173, 128)


def test_struct_mirror_and_symbols():
    assert C.sizeof(L.TokenAllow) == 32
    assert [f[0] for f in L.TokenAllow._fields_] == ["bits", "ld_words", "n_sets", "_pad", "set_of_row"]
    for name in ("cover_token_sample_rows_allowed", "cover_token_logprob_rows_allowed", "cover_token_topn_rows_allowed"):
        assert name in L.SYMBOLS and len(L.SYMBOLS[name][1]) == 3
    import os
    if os.path.exists(L.LIB_PATH):                                                 # the built library agrees (lib() checks every struct)
        assert L.lib().cover_sizeof(b"cover_token_allow") == C.sizeof(L.TokenAllow)


@pytest.mark.parametrize("name", list(SR.CASES))
def test_reference_is_decided_and_restricted(name):
    x, u, lo, hi, (T, k, p), on, sor, refs = AR.case_data(name)
    und = SR.undecided(refs)
    print(f"{name}: rows {len(refs)} | undecided {len(und)}")
    assert len(und) <= R.CAP * len(refs)
    for r, ref in enumerate(refs):
        allowed = on[sor[r], lo:hi]
        assert ref["allowed"] is not None and np.array_equal(ref["allowed"], allowed)
        assert not (ref["keep"] & ~allowed).any() and ref["kept"] == int(ref["keep"].sum()) >= 1 and allowed[ref["token"]]
        top = ref["top_tok"][ref["top_tok"] >= 0]
        assert allowed[top].all() and top.size == min(64, ref["kept"])
        assert np.isneginf(ref["lp"][~allowed]).all()
        if sor[r] == 2:                                                            # three allowed columns
            assert int(allowed.sum()) == 3
            if int(k[r]) == 8:                                                     # top_k = 8 >= |allowed|: all three stay
                assert ref["kept"] == 3 and float(p[r]) == 1.0
        if T[r] == 0:
            xr = x.numpy()[r, lo:hi]
            first = int(np.nonzero(allowed & (xr == xr[allowed].max()))[0][0])
            assert ref["greedy"] and ref["token"] == first and ref["kept"] == int(allowed.sum())
    assert any(sor[r] == 2 and int(k[r]) == 8 for r in range(len(refs)))
    w = AR.pack_bits(on)
    assert w.shape == (3, (x.shape[1] + 31) // 32)
    c = lo + (hi - lo) // 2
    assert (int(w[2, c >> 5]) >> (c & 31)) & 1 and int(sum(bin(int(v)).count("1") for v in w[2])) == 3
