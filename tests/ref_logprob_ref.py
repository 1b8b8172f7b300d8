"""Float64 reference of the reference score of cover_token_sample_rows_ref (include/cover_hip.h): the log-probability of a GIVEN column
under temperature T_ref with both filters off, over the columns of [lo, hi) (over the allowed ones when a set is given). Nothing is derived
here: it is tests/logprob_ref.reference_logprob_row at (T_ref, top_k 0, top_p 1) -- every column kept -- read at the token; with a set, on a
copy of the row with -inf in the disallowed columns (an -inf column weighs 0), as tests/allow_ref does. The tolerance is
logprob_ref.tolerance, derived there for exactly this arithmetic (fp32 exponent, exact Q43 integer mass, one double logarithm, one rounding)."""
import numpy as np

from tests import logprob_ref as LR


def reference_ref_logprob(l32, token_rel, t_ref, allowed=None):
    """l32 fp32 [n]: the logits of columns [lo, hi); token_rel: the scored column relative to lo; allowed bool [n] or None.
    Returns (lp, x_t) in float64: the log-probability of the token at (t_ref, 0, 1) and its exponent (what the tolerance scales with)."""
    l32 = np.asarray(l32, dtype=np.float32)
    if allowed is not None:
        allowed = np.asarray(allowed, dtype=bool)
        assert allowed[token_rel]
        l32 = np.where(allowed, l32, np.float32(-np.inf)).astype(np.float32)
    ref = LR.reference_logprob_row(l32, 0.0, float(t_ref), 0, 1.0)
    assert ref["keep"].all() and ref["cut_decided"]                          # unfiltered: nothing to decide
    return float(ref["lp"][token_rel]), float(ref["x"][token_rel])


def check_ref_logprobs(got, tokens, x, lo, hi, t_ref, allowed_rows=None, what=""):
    """got fp32 [rows] from the device for the absolute ids `tokens` on logits x [rows, ld]. Every row: the reference is finite (asserted
    first) and the device value lies within logprob_ref.tolerance of it. No row is left out. Prints the largest error next to its bound
    before it asserts; returns (largest error, its bound)."""
    got, tokens, x = np.asarray(got, dtype=np.float64), np.asarray(tokens), np.asarray(x)
    want = [reference_ref_logprob(x[r, lo:hi], int(tokens[r]) - lo, t_ref, None if allowed_rows is None else allowed_rows[r][lo:hi])
            for r in range(x.shape[0])]
    assert all(np.isfinite(lp) for lp, _ in want), (what, "the reference is not finite on a pick")
    worst, worst_tol, bad = 0.0, 0.0, []
    for r, (lp, xt) in enumerate(want):
        tol = float(LR.tolerance(xt, lp))
        err = abs(got[r] - lp) if np.isfinite(got[r]) else np.inf
        if err > worst:
            worst, worst_tol = err, tol
        if not err <= tol:
            bad.append((r, int(tokens[r]), got[r], lp, err, tol))
    print(f"{what}: rows {len(want)} | T_ref {t_ref} | largest |error| {worst:.3e} (bound there {worst_tol:.3e}) | violations {len(bad)}")
    assert not bad, (what, bad[:8])
    return worst, worst_tol
