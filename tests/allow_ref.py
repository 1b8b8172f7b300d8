"""What the allowed-token-set tests share (cover_token_{sample,logprob,topn}_rows_allowed, include/cover_hip.h): the sets, the bit layout
and the float64 references. Nothing is derived here. Geometry, logits, uniforms and the parameter ladder are tests/sample_rows_ref's
(CASES, LADDER, sampling_ref.lm_like_rows through case_data); the reference of a row is sample_rows_ref.reference_row -- the float64
functions of the unmasked calls -- on a copy of the row with -inf in the disallowed columns, after which keep &= allowed, kept =
keep.sum() and topn_ref.topn_of is taken on that kept set (an -inf column weighs 0, so it changes no mass, no cut and no pick; it is only
counted, and the intersection takes it out again). A greedy row: np.argmax of that copy, the first allowed maximum, kept = |allowed|.

Three sets per case, row r uses set r % 3 and parameters LADDER[r % 8]:
  0  the band [lo + n/3, lo + 2n/3 + 5) plus every 7th ABSOLUTE column (of the whole row, so bits outside [lo, hi) are set too)
  1  a seeded random half of all columns
  2  exactly three columns: lo + 1, lo + n/2, hi - 1
Margins and tolerances are the imported modules' own (sampling_ref.DELTA / CAP, logprob_ref.tolerance, topn_ref.tolerance_entropy)."""
import functools

import numpy as np

from tests import logprob_ref as LR
from tests import sample_rows_ref as SR
from tests import sampling_ref as R
from tests import topn_ref as TR

N_SETS = 3


def pack_bits(on):
    """bool [n_sets, cols] -> uint32 [n_sets, ceil(cols / 32)]: bit (c & 31) of word (c >> 5) is column c. The layout of the header, written
    out with shifts (not with the builder under test)."""
    on = np.asarray(on, dtype=bool)
    words = (on.shape[1] + 31) // 32
    out = np.zeros((on.shape[0], words), dtype=np.uint32)
    for s, c in zip(*np.nonzero(on)):
        out[s, c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return out


def case_sets(name):
    """bool [3, ld]: the three sets of a case over ABSOLUTE columns."""
    ld, lo, hi, rows, seed = SR.CASES[name]
    n = hi - lo
    on = np.zeros((N_SETS, ld), dtype=bool)
    on[0, lo + n // 3: lo + 2 * n // 3 + 5] = True
    on[0, ::7] = True
    on[1] = np.random.default_rng(seed + 50).random(ld) < 0.5
    on[2, [lo + 1, lo + n // 2, hi - 1]] = True
    return on


def reference_row(l32, allowed, u, T, k, p, n_top=64):
    """l32 fp32 [n] and allowed bool [n] over columns [lo, hi): sample_rows_ref.reference_row of the row with -inf in the disallowed columns,
    restricted afterwards (keep &= allowed, kept, top-n and entropy on that)."""
    allowed = np.asarray(allowed, dtype=bool)
    assert allowed.any()
    masked = np.where(allowed, np.asarray(l32, dtype=np.float32), np.float32(-np.inf)).astype(np.float32)
    ref = SR.reference_row(masked, u, T, k, p, n_top)
    ref["keep"] = ref["keep"] & allowed
    ref["kept"] = int(ref["keep"].sum())
    ref = TR.topn_of(ref, masked, n_top)
    ref["allowed"] = allowed
    assert allowed[ref["token"]]
    return ref


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(x fp32 [rows, ld], u, lo, hi, (T, k, p), on bool [3, ld], set_of_row int32 [rows], refs) of one case; computed once per process,
    never modified."""
    x, u, lo, hi, params, _ = SR.case_data(name)
    on = case_sets(name)
    rows = x.shape[0]
    sor = (np.arange(rows) % N_SETS).astype(np.int32)
    xn, un = x.numpy(), u.numpy()
    refs = [reference_row(xn[r, lo:hi], on[sor[r], lo:hi], un[r], float(params[0][r]), int(params[1][r]), float(params[2][r])) for r in range(rows)]
    return x, u, lo, hi, params, on, sor, refs


def masked_copy(x, on_rows, lo, hi):
    """numpy fp32 copy of x [rows, ld] with -inf in the columns of [lo, hi) that on_rows bool [rows, ld] disallows: the second oracle's input."""
    x = np.array(x, dtype=np.float32, copy=True)
    x[:, lo:hi] = np.where(on_rows[:, lo:hi], x[:, lo:hi], np.float32(-np.inf))
    return x


def check_rows(tok, kept, lp, refs, lo, hi, what=""):
    """sample_rows_ref.check_rows for restricted rows: every pick is allowed; a greedy row is the first allowed arg-max with kept = |allowed|;
    a decided sampled row has the reference's token and kept count; log-probabilities of the device's picks within logprob_ref.tolerance
    (logprob_ref.check_logprobs); at most sampling_ref.CAP of the rows undecided. Prints the figures before it asserts."""
    tok, kept = np.asarray(tok), np.asarray(kept)
    und = SR.undecided(refs)
    bad = []
    for i, r in enumerate(refs):
        t = int(tok[i])
        if not (lo <= t < hi and r["allowed"][t - lo]):
            bad.append((i, "not allowed", t))
            continue
        if r["greedy"]:
            if t != lo + r["token"] or int(kept[i]) != int(r["allowed"].sum()):
                bad.append((i, "greedy", t, lo + r["token"], int(kept[i]), int(r["allowed"].sum())))
            continue
        if r["cut_decided"] and int(kept[i]) != r["kept"]:
            bad.append((i, "kept", int(kept[i]), r["kept"]))
        if r["cut_decided"] and r["pick_decided"] and t != lo + r["token"]:
            bad.append((i, "token", t, lo + r["token"]))
    print(f"{what}: rows {len(refs)} | greedy {sum(r['greedy'] for r in refs)} | undecided {len(und)} | mismatches {len(bad)}")
    assert len(und) <= R.CAP * len(refs), (what, und)
    assert not bad, (what, bad[:8])
    if lp is not None:
        LR.check_logprobs(lp, tok, refs, lo, hi, what=what + " logprob")
