"""Float64 numpy reference of cover_token_sample_scored / cover_token_logprob (include/cover_hip.h) and what the log-probability
tests share. The kept mask is tests/sampling_ref.reference_row's (imported, not copied); on it

    x_i = (l_i - max l) / T,    lp(t) = x_t - log(sum_{i kept} exp(x_i))  for a kept t,    -inf otherwise,

which is Hugging Face's warpers (filtered logits -> -inf) followed by compute_transition_scores (a log-softmax of what is left).

TOLERANCE, derived from the arithmetic csrc/sample.hip documents, not tuned. The kernel returns
fp32( double(x_t) - log(double(M) / 2^43) ) with x_t the fp32 exponent of the pick and M the exact integer Q43 mass of the kept set:
  * x_t = (l - max) / T is two fp32 roundings: |dx_t| <= 2 * 2^-24 * |x_t|;
  * the kept mass, relative: the exponents of the weights that matter (|x| <= 40; the rest weighs at most 2^20 * e^-40 = 4.5e-12 of
    a mass that is >= 1) are off by at most 40 * 2^-23 = 4.8e-6, expf by 2 ulp = 2.4e-7, the integer sum of weights rounded to 2^-43
    by at most 2^-24 = 6e-8 for 2^20 terms -- the single-sum terms of sampling_ref.DELTA without its factor 4. A relative error e of
    the mass is an absolute error e (to first order) of its logarithm: 4.8e-6 + 2.4e-7 + 6e-8 = 5.1e-6;
  * the logarithm and the subtraction are double (1e-16, ignored); the result is rounded to fp32 once: 2^-24 * |lp|.
  tol(x_t, lp) = 5.1e-6 + 2^-23 * |x_t| + 2^-24 * |lp|        (1.2e-5 at |x_t| = |lp| = 40; 5.5e-6 to 7e-6 on the test inputs).
There is no floating-point sum over columns in the kernel, so nothing here depends on a summation order.

Rows that count: a row whose top-p cut the reference cannot decide at sampling_ref.DELTA (cut_decided false) has an ambiguous kept
mass and is left out; at most sampling_ref.CAP of a case's rows may be. On a row that counts membership is exact: finite where the
reference is finite, -inf where it is -inf.
"""
import functools

import numpy as np
import torch

from tests import sampling_ref as R

TOL_A = 4.8e-6 + 2.4e-7 + 6e-8


def tolerance(x_t, lp):
    return TOL_A + 2.0 ** -23 * np.abs(x_t) + 2.0 ** -24 * np.abs(lp)


def reference_logprob_row(l32, u, temperature, top_k, top_p):
    """l32: fp32 logits of columns [lo, hi). Returns sampling_ref.reference_row's dict plus x (float64 [n]) and lp (float64 [n]:
    the log-probability of every column, -inf outside the kept set)."""
    l32 = np.asarray(l32, dtype=np.float32)
    ref = R.reference_row(l32, u, temperature, top_k, top_p)
    l = l32.astype(np.float64)
    x = (l - l.max()) / float(np.float32(temperature))
    keep = ref["keep"]
    lse = np.log(np.sum(np.exp(x[keep])))
    ref["x"] = x
    ref["lp"] = np.where(keep, x - lse, -np.inf)
    return ref


def reference_logprob_rows(logits, lo, hi, u, temperature, top_k, top_p):
    lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    uu = u.detach().cpu().numpy() if isinstance(u, torch.Tensor) else np.asarray(u)
    return [reference_logprob_row(lg[r, lo:hi], uu[r], temperature, top_k, top_p) for r in range(lg.shape[0])]


# the input sets of the sampling tests: (kind, case index, range index)
CASES = [("wide", ci, ri) for ci in range(len(R.WIDE_CASES)) for ri in range(len(R.WIDE_RANGES))] + \
        [("narrow", ci, 0) for ci in range(len(R.NARROW_CASES))]


def case_id(case):
    kind, ci, ri = case
    T, k, p = (R.WIDE_CASES if kind == "wide" else R.NARROW_CASES)[ci]
    lo, hi = R.WIDE_RANGES[ri] if kind == "wide" else (R.NARROW_LO, R.NARROW_HI)
    return f"{kind}-T{T}-k{k}-p{p}-lo{lo}"


@functools.lru_cache(maxsize=None)
def case_data(case):
    """(x fp32 [64, ld], u fp32 [64], lo, hi, T, k, p, refs) of one input set; computed once per process."""
    kind, ci, ri = case
    if kind == "wide":
        T, k, p = R.WIDE_CASES[ci]
        lo, hi = R.WIDE_RANGES[ri]
        x, u = R.lm_like_rows(R.case_seed(kind, ci, ri), R.ROWS, R.WIDE_V, lo, hi)
    else:
        T, k, p = R.NARROW_CASES[ci]
        lo, hi = R.NARROW_LO, R.NARROW_HI
        x, u = R.lm_like_rows(R.case_seed(kind, ci), R.ROWS, R.NARROW_LD, lo, hi)
    return x, u, lo, hi, T, k, p, reference_logprob_rows(x, lo, hi, u, T, k, p)


def teacher_tokens(refs, lo, hi):
    """A teacher set that mixes kept and non-kept tokens: (7919 * pick + 13) mod (hi - lo), absolute ids."""
    return np.array([lo + (7919 * r["token"] + 13) % (hi - lo) for r in refs], dtype=np.int64)


def check_logprobs(got, tokens, refs, lo, hi, what="", cap=R.CAP):
    """got: fp32 [rows] from the device for absolute token ids `tokens`. On every row whose cut is decided: -inf exactly where the reference
    is -inf (tokens outside [lo, hi) included), finite and within tolerance() where it is finite. At most `cap` of the rows may be left
    out (sampling_ref.CAP for a case of the kernel tests; a caller that checks many small batches passes 1.0 and caps their total).
    Prints the largest observed error next to its bound before it asserts. Returns (largest error, its bound)."""
    got = np.asarray(got, dtype=np.float64)
    tokens = np.asarray(tokens)
    n = len(refs)
    left_out = [i for i, r in enumerate(refs) if not r["cut_decided"]]
    worst, worst_tol, bad = 0.0, 0.0, []
    for i, r in enumerate(refs):
        t = int(tokens[i])
        inside = lo <= t < hi
        if not inside:
            if got[i] != -np.inf:
                bad.append((i, t, got[i], "outside the range"))
            continue
        if not r["cut_decided"]:
            continue
        want = r["lp"][t - lo]
        if np.isinf(want):
            if got[i] != -np.inf:
                bad.append((i, t, got[i], want))
            continue
        tol = float(tolerance(r["x"][t - lo], want))
        err = abs(got[i] - want) if np.isfinite(got[i]) else np.inf
        if err > worst:
            worst, worst_tol = err, tol
        if not err <= tol:
            bad.append((i, t, got[i], want, err, tol))
    print(f"{what}: rows {n} | left out (cut undecided) {len(left_out)} | largest |error| {worst:.3e} (bound there {worst_tol:.3e}) | "
          f"violations {len(bad)}")
    assert len(left_out) <= cap * n, (what, left_out)
    assert not bad, (what, bad[:8])
    return worst, worst_tol
