"""What the per-row sampling tests share (cover_token_sample_rows / _logprob_rows / _topn_rows, include/cover_hip.h): the case table, the
parameter ladder and the float64 references. Nothing is derived here: a sampled row's reference is tests/logprob_ref.reference_logprob_row
(which is tests/sampling_ref.reference_row plus the log-probabilities) called with THAT ROW's parameters, its top-n tests/topn_ref.topn_of;
a greedy row (temperature 0) is np.argmax over the input floats -- the first maximum -- with the log-probabilities of the temperature 1,
unfiltered distribution (the same function with (1, 0, 1): every column kept). Margins and tolerances are those modules' own
(sampling_ref.DELTA / CAP, logprob_ref.tolerance, topn_ref.tolerance_entropy).

Row r of every case takes LADDER[r % 8]; logits and uniforms come from sampling_ref.lm_like_rows. `mid` has 4097 columns behind an
unaligned lo: one past the 4096-column boundary of the scalar calls' host dispatch and of the kernel's LDS candidate list."""
import functools

import numpy as np

from tests import logprob_ref as LR
from tests import sampling_ref as R
from tests import topn_ref as TR

LADDER = [(0, 0, 1), (1, 0, 1), (0.7, 64, 0.95), (1, 50, 1), (1, 0, 0.9), (1.5, 8, 1), (1.3, 20, 0.8), (0.5, 1, 1)]   # (T, top_k, top_p)
CASES = {              # name -> (ld, lo, hi, rows, seed)
    "narrow": (32064, 31744, 32000, 32, 7101),
    "mid": (4200, 3, 4100, 32, 7102),
    "wide": (257152, 3, 257150, 16, 7103),
}


def ladder_params(rows):
    """(temperature float32, top_k int32, top_p float32) numpy [rows]: row r carries LADDER[r % 8]."""
    T, k, p = zip(*(LADDER[r % len(LADDER)] for r in range(rows)))
    return np.array(T, dtype=np.float32), np.array(k, dtype=np.int32), np.array(p, dtype=np.float32)


def reference_row(l32, u, T, k, p, n_top=64):
    """One row with its own parameters: logprob_ref's dict (token relative to lo, kept, keep, pick_decided, cut_decided, x, lp) plus
    topn_ref's top_tok / top_lp / top_x / H and `greedy`. T == 0: the first arg-max, kept = n, scored and ranked at (1, 0, 1)."""
    l32 = np.asarray(l32, dtype=np.float32)
    if T == 0:
        ref = LR.reference_logprob_row(l32, 0.0, 1.0, 0, 1.0)
        assert ref["keep"].all() and ref["cut_decided"]
        ref.update(token=int(np.argmax(l32)), kept=int(l32.size), pick_decided=True, greedy=True)
    else:
        ref = LR.reference_logprob_row(l32, u, T, k, p)
        ref["greedy"] = False
    return TR.topn_of(ref, l32, n_top)


def reference_rows(x, lo, hi, u, T, k, p):
    x, u = np.asarray(x), np.asarray(u)
    return [reference_row(x[r, lo:hi], u[r], float(T[r]), int(k[r]), float(p[r])) for r in range(x.shape[0])]


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(x fp32 [rows, ld], u fp32 [rows], lo, hi, (T, k, p) numpy [rows], refs) of one case; computed once per process, never modified."""
    ld, lo, hi, rows, seed = CASES[name]
    x, u = R.lm_like_rows(seed, rows, ld, lo, hi)
    params = ladder_params(rows)
    return x, u, lo, hi, params, reference_rows(x.numpy(), lo, hi, u.numpy(), *params)


def undecided(refs):
    return [i for i, r in enumerate(refs) if not (r["pick_decided"] and r["cut_decided"])]


def check_rows(tok, kept, lp, refs, lo, hi, what=""):
    """tok / kept / lp from the device (lp None: not checked). Every greedy row: the arg-max exactly, kept = hi - lo. Every sampled row that
    is decided: the reference's token and kept count (the count wherever the cut is decided). Log-probabilities of the device's own picks
    within logprob_ref.tolerance wherever the cut is decided (logprob_ref.check_logprobs). At most sampling_ref.CAP of the rows undecided.
    Prints the figures before it asserts."""
    tok, kept = np.asarray(tok), np.asarray(kept)
    und = undecided(refs)
    bad = []
    for i, r in enumerate(refs):
        if r["greedy"]:
            if int(tok[i]) != lo + r["token"] or int(kept[i]) != hi - lo:
                bad.append((i, "greedy", int(tok[i]), lo + r["token"], int(kept[i])))
            continue
        if r["cut_decided"] and int(kept[i]) != r["kept"]:
            bad.append((i, "kept", int(kept[i]), r["kept"]))
        if r["cut_decided"] and r["pick_decided"] and int(tok[i]) != lo + r["token"]:
            bad.append((i, "token", int(tok[i]), lo + r["token"]))
    print(f"{what}: rows {len(refs)} | greedy {sum(r['greedy'] for r in refs)} | undecided {len(und)} | mismatches {len(bad)}")
    assert len(und) <= R.CAP * len(refs), (what, und)
    assert not bad, (what, bad[:8])
    if lp is not None:
        LR.check_logprobs(lp, tok, refs, lo, hi, what=what + " logprob")
