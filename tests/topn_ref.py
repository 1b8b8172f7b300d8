"""Float64 numpy reference of cover_token_topn (include/cover_hip.h) and what the top-n tests share. Built on
tests/logprob_ref.reference_logprob_row (imported, not copied): on its kept mask `keep` over columns [lo, hi)

    rank   the kept columns by descending input float, equal floats (-0 == +0) by ascending index: np.lexsort((idx, -l32[idx]))
    lp     logprob_ref's lp of the ranked columns
    H      -sum_{i in keep} p_i log p_i,  p_i = exp(lp_i)   (a column of probability 0, an -inf logit, contributes 0)

Ranks and padding (-1 / -inf beyond the kept set) are exact, no tolerance. Log-probabilities: logprob_ref.tolerance.

ENTROPY TOLERANCE, derived from the arithmetic csrc/sample.hip documents, not tuned. With x_i = (l_i - max) / T <= 0 and w_i = expf(x_i) the
kernel returns fp32( log(M / 2^43) + S / M ) in double, M = sum rint(w_i 2^43) and S = sum rint(w_i (-x_i) 2^43) exact integer sums
over the kept set; exactly, H = log W + (sum w_i (-x_i)) / W.
  * M is off by at most logprob_ref.TOL_A = 5.1e-6 relative (derived there): log M by 5.1e-6 absolute, S / M by 5.1e-6 of itself;
  * a term of S: w_i off by 4.8e-6 + 2.4e-7 = 5.04e-6 relative (the exponent's two roundings for |x| <= 40, expf), -x_i by two fp32
    roundings, the product by one: 5.04e-6 + 3 * 2^-24 relative; the conversion to 2^-43 at most 2^-44 per term, 2^-24 absolute for
    2^20 terms; terms with |x| > 40 weigh at most 2^20 * 40 e^-40 = 1.8e-10 and are ignored;
  * S / M <= H (log W >= 0 because M >= 2^43: the row maximum weighs 1), so the relative errors of S and of M scale with at most H:
    (5.04e-6 + 3 * 2^-24 + 5.1e-6) H = 1.032e-5 H <= 1.05e-5 H, and the absolute ones add to 5.1e-6 + 2^-24 = 5.16e-6 <= 5.2e-6;
  * one rounding to fp32: 2^-24 H.
  tol_H(H) = 5.2e-6 + 1.05e-5 H + 2^-24 H                    (6e-6 at H = 0.1, 5.8e-5 at H = 5)

Rows that count: as in logprob_ref, a row whose top-p cut the reference cannot decide (cut_decided false) is left out; at most
sampling_ref.CAP of a case's rows may be.
"""
import functools

import numpy as np
import torch

from tests import logprob_ref as LR
from tests import sampling_ref as R

TOL_H_ABS = 5.2e-6
TOL_H_REL = 1.05e-5 + 2.0 ** -24


def tolerance_entropy(H):
    return TOL_H_ABS + TOL_H_REL * np.abs(H)


def topn_of(ref, l32, n):
    """ref: logprob_ref.reference_logprob_row's dict for the fp32 logits l32 of columns [lo, hi). Returns a copy plus top_tok (int64 [n],
    relative ids of the min(n, kept) best in rank order, -1 padded), top_lp / top_x (float64 [n], -inf / 0 padded) and H."""
    l32 = np.asarray(l32, dtype=np.float32)
    ref = dict(ref)
    idx = np.nonzero(ref["keep"])[0]
    order = idx[np.lexsort((idx, -(l32[idx] + np.float32(0.0))))][:n]          # + 0.0: -0 -> +0, the two compare equal anyway
    lp = ref["lp"][idx]
    p = np.exp(lp)
    with np.errstate(invalid="ignore"):
        ref["H"] = float(-np.sum(np.where(p > 0, p * lp, 0.0)))
    ref["top_tok"] = np.concatenate([order, np.full(n - order.size, -1)]).astype(np.int64)
    ref["top_lp"] = np.concatenate([ref["lp"][order], np.full(n - order.size, -np.inf)])
    ref["top_x"] = np.concatenate([ref["x"][order], np.zeros(n - order.size)])
    return ref


def reference_topn_row(l32, n, temperature, top_k, top_p):
    return topn_of(LR.reference_logprob_row(l32, 0.0, temperature, top_k, top_p), l32, n)


def reference_topn_rows(logits, lo, hi, n, temperature, top_k, top_p):
    lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    return [reference_topn_row(lg[r, lo:hi], n, temperature, top_k, top_p) for r in range(lg.shape[0])]


@functools.lru_cache(maxsize=None)
def case_refs(case):
    """The 64 best of every row of logprob_ref.case_data(case), on that module's own references (nothing is computed twice); a test with
    a smaller n passes it to check_topn, which looks at the first n slots."""
    x, u, lo, hi, T, k, p, refs = LR.case_data(case)
    lg = x.numpy()
    return [topn_of(r, lg[i, lo:hi], 64) for i, r in enumerate(refs)]


def check_topn(tok, lp, ent, kept, refs, lo, what="", cap=R.CAP, n=None):
    """refs computed for at least n slots (n None: as many as they hold).
    tok int64 [rows, n] (absolute ids), lp fp32 [rows, n], ent fp32 [rows], kept int32 [rows] or None from the device. On every row
    whose cut is decided: ids and padding exact, log-probabilities within logprob_ref.tolerance, entropy within tolerance_entropy, the
    kept count exact. Prints the largest errors next to their bounds before it asserts. Returns the number of rows left out."""
    tok, lp, ent = np.asarray(tok), np.asarray(lp, dtype=np.float64), np.asarray(ent, dtype=np.float64)
    rows = len(refs)
    left_out = [i for i, r in enumerate(refs) if not r["cut_decided"]]
    w_lp = w_lp_tol = w_h = w_h_tol = 0.0
    bad = []
    for i, r in enumerate(refs):
        if not r["cut_decided"]:
            continue
        r = dict(r, top_tok=r["top_tok"][:n], top_lp=r["top_lp"][:n], top_x=r["top_x"][:n])
        want_tok = np.where(r["top_tok"] >= 0, r["top_tok"] + lo, -1)
        if not np.array_equal(tok[i], want_tok):
            bad.append((i, "ids", tok[i].tolist()[:8], want_tok.tolist()[:8]))
            continue
        if kept is not None and int(kept[i]) != r["kept"]:
            bad.append((i, "kept", int(kept[i]), r["kept"]))
        inf = np.isneginf(r["top_lp"])
        if not np.array_equal(np.isneginf(lp[i]), inf):
            bad.append((i, "-inf slots", lp[i].tolist()[:8], r["top_lp"].tolist()[:8]))
            continue
        fin = ~inf
        if fin.any():
            err = np.abs(lp[i][fin] - r["top_lp"][fin])
            tol = LR.tolerance(r["top_x"][fin], r["top_lp"][fin])
            j = int(np.argmax(err - tol))
            if err.max() > w_lp:
                w_lp, w_lp_tol = float(err.max()), float(tol[int(np.argmax(err))])
            if not (err <= tol).all():
                bad.append((i, "logprob", float(err[j]), float(tol[j])))
        e, t = abs(ent[i] - r["H"]), float(tolerance_entropy(r["H"]))
        if e > w_h:
            w_h, w_h_tol = e, t
        if not e <= t:
            bad.append((i, "entropy", ent[i], r["H"], e, t))
    print(f"{what}: rows {rows} | left out (cut undecided) {len(left_out)} | largest |logprob error| {w_lp:.3e} (bound there {w_lp_tol:.3e}) | "
          f"largest |entropy error| {w_h:.3e} (bound there {w_h_tol:.3e}) | violations {len(bad)}")
    assert len(left_out) <= cap * rows, (what, left_out)
    assert not bad, (what, bad[:8])
    return len(left_out)


# ------------------------------------------------------------------------------------------------ tie and padding inputs (top_p = 1.0)
def tie_inputs():
    """name -> (logits fp32 [rows, ld], lo, hi, n, temperature, top_k): a few rows each, every cut decided because top_p is 1.0."""
    g = torch.Generator().manual_seed(31)
    out = {}
    out["constant row"] = (torch.full((3, 5003), 0.25), 2, 5002, 7, 1.0, 0)                 # 5000 columns: stays on the row path
    x = torch.randn(3, 3000, generator=g)
    cols = torch.randperm(3000, generator=g)[:100]
    x[:, cols] = 9.0
    out["plateau of 100 maxima"] = (x, 0, 3000, 64, 0.8, 0)
    for n in (5, 64):
        x = torch.randn(4, 6000, generator=g)
        for r in range(4):
            cols = torch.randperm(6000, generator=g)[:n + 4]
            x[r, cols[:n - 2]] = 20.0 - torch.arange(n - 2, dtype=torch.float32) * 0.125       # ranks 0 .. n-3, distinct
            x[r, cols[n - 2:]] = 8.0                                                          # ranks n-2 .. n+3 equal
        out[f"tie straddling rank {n}"] = (x, 1, 5999, n, 1.0, 0)
    x = torch.full((3, 700), -3.0)
    z = torch.randperm(700, generator=g)[:40]
    x[:, z[:20]] = 0.0
    x[:, z[20:]] = -0.0
    x[2, 5] = 1.0
    out["+0.0 and -0.0"] = (x, 0, 700, 16, 1.0, 0)
    out["top_k 3, n 8"] = (torch.randn(4, 4500, generator=g), 7, 4400, 8, 1.2, 3)
    x = torch.randn(3, 900, generator=g)
    x[:, torch.randperm(900, generator=g)[:600]] = -float("inf")
    x[2, :] = -float("inf")
    x[2, [3, 500, 501]] = torch.tensor([1.0, 2.0, 2.0])
    out["-inf columns"] = (x, 0, 900, 8, 1.0, 0)
    out["hi - lo < n"] = (torch.randn(3, 40, generator=g), 30, 35, 8, 0.7, 0)
    return out
