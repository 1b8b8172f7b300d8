"""Numpy reference of the per-row token automaton of cover_decode_feedback_fsm (include/cover_hip.h) and of the tables
host.length_grammar is expected to build, written from the specification alone (nothing of cover_vla_amd is imported).

The automaton step, per row b, with t the token the feedback step emitted and was_done the done flag before the step:

    if 0 <= state[b] < n_states:
        if not was_done[b] and 0 <= t[b] < vocab:  state[b] = trans[state[b], class_of_token[t[b]]]
        set_of_row[b] = set_of_state[state[b]]
    else:
        state[b] unchanged, set_of_row[b] = -1

Integers only: the GPU tests compare exactly.

The length grammar "min_len..max_len body tokens, one end token, eos": states 0..max_len count body tokens, ENDED = max_len + 1,
FINISHED = max_len + 2; classes body 0, end 1, eos 2, other 3. A state allows body while n < max_len, end once n >= min_len, eos in
ENDED / FINISHED only. A token of an allowed class moves (body n + 1, end ENDED, eos FINISHED), any other token stays."""
import numpy as np

BODY, END, EOS, OTHER = 0, 1, 2, 3


def fsm_step(state, tokens, was_done, class_of_token, trans, set_of_state):
    """One step, in place on state (int32 [B]); returns set_of_row int32 [B]."""
    n_states = trans.shape[0]
    vocab = class_of_token.shape[0]
    set_of_row = np.full(state.shape[0], -1, dtype=np.int32)
    for b in range(state.shape[0]):
        s = int(state[b])
        if not 0 <= s < n_states:
            continue
        t = int(tokens[b])
        if not was_done[b] and 0 <= t < vocab:
            s = int(trans[s, int(class_of_token[t])])
            state[b] = s
        set_of_row[b] = set_of_state[s]
    return set_of_row


def _members(vocab, ids):
    on = np.zeros(vocab, dtype=bool)
    if isinstance(ids, tuple):
        on[ids[0]:ids[1]] = True
    else:
        on[list(ids)] = True
    return on


def length_tables(vocab, body, end, eos, min_len, max_len):
    """(class_of_token uint8 [vocab], trans int32 [max_len + 3, 4], allowed bool [max_len + 3, vocab]): allowed[s] is the membership
    of the set a row in state s draws from."""
    body, end, eos = _members(vocab, body), _members(vocab, end), _members(vocab, eos)
    cls = np.full(vocab, OTHER, dtype=np.uint8)
    cls[body], cls[end], cls[eos] = BODY, END, EOS
    ended, finished = max_len + 1, max_len + 2
    n_states = max_len + 3
    trans = np.zeros((n_states, 4), dtype=np.int32)
    allowed = np.zeros((n_states, vocab), dtype=bool)
    for s in range(n_states):
        trans[s, :] = s
        if s <= max_len:
            if s < max_len:
                allowed[s] |= body
                trans[s, BODY] = s + 1
            if s >= min_len:
                allowed[s] |= end
                trans[s, END] = ended
        else:
            allowed[s] |= eos
            trans[s, EOS] = finished
    return cls, trans, allowed


def n_distinct_sets(min_len, max_len):
    """How many different sets the table of the length grammar holds: eos-only always; body-only if some n < min_len (and n < max_len);
    body-or-end if some min_len <= n < max_len; end-only always (state max_len). Independent of how large max_len is: at most four."""
    return 2 + (1 if min_len > 0 else 0) + (1 if min_len < max_len else 0)


def obeys_length_grammar(row, body, end, eos, pad, min_len, max_len, vocab):
    """True when row (a sequence of ids) is min_len..max_len body ids, one end id, one eos id, then pad only (possibly cut off by the
    end of the row before the end / eos id: a prefix of a valid string whose next token could still complete it)."""
    body, end, eos = _members(vocab, body), _members(vocab, end), _members(vocab, eos)
    row = [int(t) for t in row]
    n = 0
    while n < len(row) and body[row[n]]:
        n += 1
    if n > max_len:
        return False
    if n == len(row):
        return True                                   # still in the body when the row ran out
    if n < min_len or not end[row[n]]:
        return False
    if n + 1 == len(row):
        return True
    if not eos[row[n + 1]]:
        return False
    return all(t == pad for t in row[n + 2:])
