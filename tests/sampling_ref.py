"""Float64 numpy reference of cover_token_sample's semantics (include/cover_hip.h) and the inputs / margins the sampling tests share.
Not derived from the kernel: an exact sort with the index tie rule and np.cumsum in float64.

DELTA, the margin below which a comparison is not demanded (relative to the mass of the set summed). Derived from what
csrc/sample.hip documents, not tuned:
  * the exponent x = (l - max) / T is two fp32 roundings: |dx| <= 2 * 2^-24 * |x|. Terms with |x| > 40 weigh at most 2^20 * e^-40 =
    4.5e-12 of the mass (the row maximum alone weighs 1) and are ignored, so the weights that matter are off by at most
    40 * 2^-23 = 4.8e-6 relative;
  * expf: 2 ulp = 2.4e-7 relative;
  * the sums: exact integer sums of weights rounded to 2^-43 -- at most 2^-44 per term, 2^-24 = 6e-8 of the mass for 2^20 terms
    (no dependence on an order: there is no floating-point sum in the kernel);
  * the factor 4 for the two sums that enter one comparison.
  4 * (4.8e-6 + 2.4e-7 + 6e-8) = 2.04e-5.
"""
import numpy as np
import torch

DELTA = 2.1e-5
CAP = 0.10            # at most this share of a case's rows may be undecided

WIDE_V = 257152
WIDE_CASES = [(1.0, 0, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.9), (0.7, 64, 0.95), (1.5, 8, 1.0)]      # (temperature, top_k, top_p)
WIDE_RANGES = [(0, 257152), (3, 257150)]
NARROW_LD, NARROW_LO, NARROW_HI = 32064, 31744, 32000
NARROW_CASES = [(1.0, 0, 1.0), (1.0, 50, 0.9), (1.3, 20, 0.8)]
ROWS = 64


def lm_like_rows(seed, rows, ld, lo, hi, n_boost=40):
    """Logits shaped like a language model's: randn in fp32 plus, on n_boost distinct random columns of [lo, hi), a boost drawn from
    U(10, 18); the uniforms come from the same generator. Returns (logits fp32 [rows, ld], u fp32 [rows])."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, ld, generator=g, dtype=torch.float32)
    for r in range(rows):
        cols = lo + torch.randperm(hi - lo, generator=g)[:n_boost]
        x[r, cols] += 10.0 + 8.0 * torch.rand(n_boost, generator=g, dtype=torch.float32)
    u = torch.rand(rows, generator=g, dtype=torch.float32)
    return x, u


def case_seed(kind, ci, ri=0):
    return 1000 + 100 * (0 if kind == "wide" else 1) + 10 * ci + ri


def reference_row(l32, u, temperature, top_k, top_p, delta=DELTA):
    """l32: fp32 logits of columns [lo, hi). Returns dict(token (relative index), kept, keep (bool mask), pick_decided, cut_decided)."""
    l32 = np.asarray(l32, dtype=np.float32)
    n = l32.size
    l = l32.astype(np.float64)
    T, P, U = float(np.float32(temperature)), float(np.float32(top_p)), float(np.float32(u))
    w = np.exp((l - l.max()) / T)
    keep = np.ones(n, dtype=bool)
    if 0 < top_k < n:
        kth = np.partition(l32, n - top_k)[n - top_k]              # k-th largest input float
        keep = l32 >= kth
    cut_decided = True
    if P < 1.0:
        idx = np.nonzero(keep)[0]
        order = idx[np.lexsort((idx, -w[idx]))]                     # descending weight, equal weights by ascending index
        cs = np.cumsum(w[order])
        mass_k = cs[-1]
        tgt = P * mass_k
        j = min(int(np.searchsorted(cs, tgt, side="left")), order.size - 1)   # shortest prefix whose mass reaches the target
        keep = np.zeros(n, dtype=bool)
        keep[order[:j + 1]] = True
        below = cs[j - 1] if j > 0 else 0.0
        cut_decided = bool(tgt - below >= delta * mass_k and cs[j] - tgt >= delta * mass_k)
    kidx = np.nonzero(keep)[0]
    cs = np.cumsum(w[kidx])
    mass = cs[-1]
    t = U * mass
    j = min(int(np.searchsorted(cs, t, side="right")), kidx.size - 1)          # first kept index whose running sum exceeds t
    lo_edge = cs[j - 1] if j > 0 else 0.0
    pick_decided = bool(t - lo_edge >= delta * mass and cs[j] - t >= delta * mass)
    return dict(token=int(kidx[j]), kept=int(kidx.size), keep=keep, pick_decided=pick_decided, cut_decided=cut_decided)


def reference_rows(logits, lo, hi, u, temperature, top_k, top_p, delta=DELTA):
    lg = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    uu = u.detach().cpu().numpy() if isinstance(u, torch.Tensor) else np.asarray(u)
    return [reference_row(lg[r, lo:hi], uu[r], temperature, top_k, top_p, delta) for r in range(lg.shape[0])]


def check_against_reference(tok, kept, refs, lo, top_k, top_p, what=""):
    """Every decided row equals the reference exactly (token; the kept count whenever the cut is decided -- always under top-k alone);
    at most CAP of the rows may be undecided. Prints the figures before it asserts. Returns the number of undecided rows."""
    tok = [int(t) for t in tok]
    kept = [int(k) for k in kept]
    n = len(refs)
    und_pick = sum(not r["pick_decided"] for r in refs)
    und_cut = sum(not r["cut_decided"] for r in refs)
    und = sum(not (r["pick_decided"] and r["cut_decided"]) for r in refs)
    bad_tok = [i for i, r in enumerate(refs) if r["pick_decided"] and r["cut_decided"] and tok[i] != lo + r["token"]]
    bad_kept = [i for i, r in enumerate(refs) if r["cut_decided"] and kept[i] != r["kept"]]
    print(f"{what}: rows {n} | pick undecided {und_pick} | cut undecided {und_cut} | undecided {und} | token mismatches on decided rows "
          f"{len(bad_tok)} | kept mismatches {len(bad_kept)} | median kept {int(np.median([r['kept'] for r in refs]))}")
    assert und <= CAP * n, (what, und, n)
    assert not bad_tok, (what, [(i, tok[i], lo + refs[i]["token"]) for i in bad_tok[:8]])
    assert not bad_kept, (what, [(i, kept[i], refs[i]["kept"]) for i in bad_kept[:8]])
    return und
