"""Numpy reference of cover_decode_feedback (include/cover_hip.h): the bookkeeping between two decode steps of pi0-FAST's
generate_tokens, statement for statement what its per-row path does with torch ops after every pick.

    t           = force[b] if forced else pick[b]
    lp_out[b,i] = 0.0 if done[b] else lp[b]
    t           = pad if done[b] else t
    tok_out[b,i]= t
    done[b]    |= t == eos
    live[i]    += not done[b]

Integers only, except that the log-probability is copied or replaced by 0.0: every result is exact, the GPU tests compare bit for
bit. The embedding row of the emitted id is checked against ops.embed_gather there."""
import numpy as np


def feedback_step(pick, done, tok_out, i, eos, pad, force=None, lp=None, lp_out=None, live=None):
    """One step, in place on done (bool [B]), tok_out (int64 [B, >= i + 1]), lp_out (float32 [B, >= i + 1]), live (int32 [>= i + 1]).
    Returns the emitted ids int64 [B]."""
    pick = np.asarray(pick, dtype=np.int64)
    t = np.asarray(force, dtype=np.int64).copy() if force is not None else pick.copy()
    was = done.copy()
    if lp_out is not None:
        lp_out[:, i] = np.where(was, np.float32(0.0), np.asarray(lp, dtype=np.float32))
    t[was] = pad
    tok_out[:, i] = t
    done |= (t == eos)
    if live is not None:
        live[i] += int((~done).sum())
    return t


def run(picks, eos, pad, force=None, lps=None):
    """All steps of a [B, n] pick matrix from a fresh state: (tokens int64 [B, n], done bool [B], lp_out float32 [B, n] or None,
    live int32 [n])."""
    picks = np.asarray(picks, dtype=np.int64)
    B, n = picks.shape
    out = np.full((B, n), pad, dtype=np.int64)
    done = np.zeros(B, dtype=bool)
    live = np.zeros(n, dtype=np.int32)
    lp_out = np.zeros((B, n), dtype=np.float32) if lps is not None else None
    for i in range(n):
        feedback_step(picks[:, i], done, out, i, eos, pad, force=None if force is None else force[:, i],
                      lp=None if lps is None else lps[:, i], lp_out=lp_out, live=live)
    return out, done, lp_out, live
