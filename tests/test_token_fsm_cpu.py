"""Token grammars without a GPU: host.length_grammar against the independent tables of tests/fsm_ref.py, ops.TokenFsm's host
validation, ops.token_fsm_check, the struct mirror and the binding, and a random-walk property of the reference itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import host, ops
from tests import fsm_ref as FR

VOCAB, BODY, END, EOS_IDS = 300, (40, 200), [210], [1]
CASES = [(0, 1), (1, 1), (2, 5), (3, 3)]


def _membership(allow):
    w = np.ascontiguousarray(allow.bits.view(torch.int32).numpy()).view(np.uint32)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)


@pytest.mark.parametrize("min_len,max_len", CASES)
def test_length_grammar_tables(min_len, max_len):
    allow, fsm = host.length_grammar(VOCAB, BODY, END, EOS_IDS, min_len, max_len)
    cls, trans, allowed = FR.length_tables(VOCAB, BODY, END, EOS_IDS, min_len, max_len)
    assert fsm.n_states == max_len + 3 and fsm.n_classes == 4 and fsm.start_state == 0 and fsm.vocab == VOCAB
    assert np.array_equal(fsm.class_of_token_np, cls) and fsm.class_of_token_np.dtype == np.uint8
    assert np.array_equal(fsm.trans_np, trans) and fsm.trans_np.dtype == np.int32
    on = _membership(allow)
    assert on.shape[1] >= VOCAB and not on[:, VOCAB:].any()
    for s in range(fsm.n_states):                                  # the set a state names holds exactly the ids the table allows
        assert np.array_equal(on[fsm.set_of_state_np[s], :VOCAB], allowed[s]), s
    # the states share their sets: as many bit sets as the table has distinct rows, however many states there are
    assert allow.n_sets == FR.n_distinct_sets(min_len, max_len) == len({r.tobytes() for r in allowed})
    assert len({r.tobytes() for r in on}) == allow.n_sets          # and no two of them are equal
    assert allow.n_sets == (4 if (min_len, max_len) == (2, 5) else 3)
    assert ops.token_fsm_check(fsm, allow, 0, VOCAB) == list(range(fsm.n_states))
    assert ops.token_fsm_check(fsm, allow, 1, 211) == list(range(fsm.n_states))        # the tightest range that holds eos and end


def test_length_grammar_set_count_does_not_grow():
    allow, fsm = host.length_grammar(VOCAB, BODY, END, EOS_IDS, 7, 120)
    assert allow.n_sets == 4 and fsm.n_states == 123
    allow, fsm = host.length_grammar(VOCAB, BODY, END, EOS_IDS, 2, 5, extra_sets=[[3, (250, 260)]])
    on = _membership(allow)
    assert allow.n_sets == 5 and int(fsm.set_of_state_np.max()) == 3 and on[4, 3] and on[4, 250:260].all() and on[4].sum() == 11
    for bad in (dict(min_len=3, max_len=2), dict(min_len=-1, max_len=2), dict(body=(40, 211)), dict(eos=[210]), dict(end=[300]), dict(body=(9, 9))):
        kw = dict(vocab=VOCAB, body=BODY, end=END, eos=EOS_IDS, min_len=1, max_len=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            host.length_grammar(**kw)


def test_fsm_check_names_the_dead_state():
    allow, fsm = host.length_grammar(VOCAB, BODY, END, EOS_IDS, 2, 2)
    # the end id (210) lies outside [lo, hi) = [0, 205): state 2 (two body tokens emitted, end only) has nothing to draw
    with pytest.raises(L.CoverError, match=r"state 2 "):
        ops.token_fsm_check(fsm, allow, 0, 205)
    # with (2, 4) the first state that allows end only is 4; states 2 and 3 still have the body
    allow, fsm = host.length_grammar(VOCAB, BODY, END, EOS_IDS, 2, 4)
    with pytest.raises(L.CoverError, match=r"state 4 "):
        ops.token_fsm_check(fsm, allow, 0, 205)
    # eos (1) outside the range: ENDED (state 5) is dead, and is reached only through the end class
    with pytest.raises(L.CoverError, match=r"state 5 "):
        ops.token_fsm_check(fsm, allow, 3, 297)
    # a state that no allowed class leads to is not visited: an unreachable state with an empty set is fine
    cls = np.zeros(10, dtype=np.uint8)
    cls[5:] = 1
    bits = ops.token_allow_sets(10, [[(0, 5)], [(5, 5)]])
    f = ops.TokenFsm(cls, [[0, 1], [1, 1]], [0, 1])
    assert ops.token_fsm_check(f, ops.TokenAllow(bits), 0, 10) == [0]         # class 1 has no allowed token in state 0's set
    f2 = ops.TokenFsm(cls, [[1, 1], [1, 1]], [0, 1])
    with pytest.raises(L.CoverError, match=r"state 1 "):
        ops.token_fsm_check(f2, ops.TokenAllow(bits), 0, 10)
    for lo, hi in ((0, 11), (-1, 5), (4, 4)):
        with pytest.raises(L.CoverError):
            ops.token_fsm_check(f, ops.TokenAllow(bits), lo, hi)


def test_token_fsm_validation():
    cls = np.array([0, 1, 2, 1], dtype=np.uint8)
    trans = np.array([[0, 1, 1], [1, 0, 1]], dtype=np.int32)
    f = ops.TokenFsm(cls, trans, [0, 1], start_state=1)
    assert (f.n_states, f.n_classes, f.vocab, f.start_state) == (2, 3, 4, 1)
    f = ops.TokenFsm(torch.from_numpy(cls), torch.from_numpy(trans), torch.tensor([0, 1]))
    bad_trans = trans.copy()
    bad_trans[1, 2] = 2
    neg_trans = trans.copy()
    neg_trans[0, 0] = -1
    for args in ((cls, bad_trans, [0, 1]), (cls, neg_trans, [0, 1]), (cls, trans, [0, -1]), (cls, trans, [0, 1, 0]), (cls, trans[0], [0, 1]),
                 (np.array([0, 3]), trans, [0, 1]), (cls.astype(np.float32), trans, [0, 1]), (cls, np.zeros((2, 257), dtype=np.int32), [0, 1]),
                 (cls[:0], trans, [0, 1])):
        with pytest.raises(L.CoverError):
            ops.TokenFsm(*args)
    for start in (-1, 2):
        with pytest.raises(L.CoverError):
            ops.TokenFsm(cls, trans, [0, 1], start_state=start)
    # a set index beyond the TokenAllow's n_sets is refused when the two are paired
    one = ops.TokenAllow(ops.token_allow_sets(4, [[(0, 4)]]))
    two = ops.TokenAllow(ops.token_allow_sets(4, [[(0, 4)], [1]]))
    ops.TokenFsm(cls, trans, [0, 1]).check_sets(two)
    with pytest.raises(L.CoverError):
        ops.TokenFsm(cls, trans, [0, 1]).check_sets(one)
    with pytest.raises(L.CoverError):
        ops.token_fsm_check(ops.TokenFsm(cls, trans, [0, 1]), one, 0, 4)
    state, sor = ops.TokenFsm(cls, trans, [5, 7], start_state=1).rows(3, "cpu")
    assert state.dtype == torch.int32 and state.tolist() == [1, 1, 1] and sor.dtype == torch.int32 and sor.tolist() == [7, 7, 7]


def test_struct_mirror_and_symbol():
    assert "cover_decode_feedback_fsm" in L.SYMBOLS and L._STRUCTS["cover_token_fsm"] is L.TokenFsm
    assert [n for n, _ in L.TokenFsm._fields_] == ["class_of_token", "trans", "set_of_state", "n_states", "n_classes", "state", "set_of_row"]
    assert C.sizeof(L.TokenFsm) == 48
    assert L.lib().cover_sizeof(b"cover_token_fsm") == C.sizeof(L.TokenFsm)
    assert L.lib().cover_decode_feedback_fsm(None, None, None, None, 0, None) == -1          # COVER_EINVAL before anything touches a device


def test_step_torch_equals_reference():
    """TokenFsm.step_torch (the models' unfused path) against the reference on CPU tensors: random tables, finished rows, ids outside the
    vocabulary and states outside the table."""
    rng = np.random.default_rng(11)
    V, S, K, B = 70, 6, 4, 64
    cls = rng.integers(0, K, V).astype(np.uint8)
    trans = rng.integers(0, S, (S, K)).astype(np.int32)
    sos = rng.integers(0, 9, S).astype(np.int32)
    f = ops.TokenFsm(cls, trans, sos).to("cpu")
    state = rng.integers(-1, S + 2, B).astype(np.int32)
    for _ in range(6):
        tok = rng.integers(-2, V + 2, B).astype(np.int64)
        was = rng.random(B) < 0.3
        want_state = state.copy()
        want_sor = FR.fsm_step(want_state, tok, was, cls, trans, sos)
        st, sor = torch.from_numpy(state.copy()), torch.full((B,), 99, dtype=torch.int32)
        f.step_torch(st, sor, torch.from_numpy(tok), torch.from_numpy(~was))
        assert np.array_equal(st.numpy(), want_state) and np.array_equal(sor.numpy(), want_sor)
        state = want_state


@pytest.mark.parametrize("min_len,max_len", CASES)
def test_random_walks_obey_the_grammar(min_len, max_len):
    """Under the reference, any token string that respects the current set at every step is min_len..max_len body ids, one end id, eos."""
    cls, trans, allowed = FR.length_tables(VOCAB, BODY, END, EOS_IDS, min_len, max_len)
    set_of_state = np.arange(max_len + 3, dtype=np.int32)         # one set per state: the walk only needs the membership
    rng = np.random.default_rng(100 * min_len + max_len)
    PAD, steps = 0, max_len + 4
    lengths = set()
    for _ in range(200):
        state = np.zeros(1, dtype=np.int32)
        done, row = False, []
        for _ in range(steps):
            if done:
                row.append(PAD)
                continue
            ids = np.nonzero(allowed[state[0]])[0]
            k = rng.choice(np.unique(cls[ids]))                    # a class first, so the single end id is as likely as the body band
            t = int(rng.choice(ids[cls[ids] == k]))
            row.append(t)
            sor = FR.fsm_step(state, [t], [False], cls, trans, set_of_state)
            assert sor[0] == state[0]
            done = t == EOS_IDS[0]
        assert done and FR.obeys_length_grammar(row, BODY, END, EOS_IDS, PAD, min_len, max_len, VOCAB), row
        n_body = row.index(END[0])
        assert min_len <= n_body <= max_len and row[n_body + 1] == EOS_IDS[0] and all(t == PAD for t in row[n_body + 2:])
        lengths.add(n_body)
    assert lengths == set(range(min_len, max_len + 1))             # every permitted length comes up


def test_obeys_length_grammar_rejects():
    ok = lambda row: FR.obeys_length_grammar(row, BODY, END, EOS_IDS, 0, 2, 4, VOCAB)
    assert ok([50, 60, 210, 1, 0, 0]) and ok([50, 60, 70, 80, 210, 1]) and ok([50, 60, 70]) and ok([50, 60, 210])
    assert not ok([50, 210, 1, 0]) and not ok([1, 0, 0]) and not ok([50, 60, 70, 80, 90, 210]) and not ok([50, 60, 5, 210, 1])
    assert not ok([50, 60, 210, 210]) and not ok([50, 60, 210, 1, 50]) and not ok([50, 60, 1])
