"""CPU references of stochastic beam search (cover_gumbel_topn, cover_beam_merge_gumbel; include/cover_hip.h) and what its tests share:
tests/test_gumbel_beam_cpu.py and tests/test_gumbel_beam_gpu.py.

row_step is float64 numpy on the fp32 inputs: nothing of it is derived from the kernel. merge_gumbel has no tolerance (the key is a stored
float, the one sum is ONE fp32 add), like beam_ref.merge. restate_f32 is the same formula in np.float32 arithmetic: what the distance
between ANY fp32 evaluation and the float64 one looks like, which is where the device tolerance comes from (check_lists).

Why g~ needs a measured tolerance and not a constant: v = G - g + log1p(-exp(g - Z)) amplifies the rounding of g - Z (a few 1e-6 at
|g| ~ 20) by 1 / |g - Z| when a column lies close to the row maximum, so the error depends on the closest runner-up of the case."""
import functools

import numpy as np

NINF = np.float32(-np.inf)
U_LO, U_HI = np.float32(2.0 ** -24), np.float32(1.0 - 2.0 ** -24)
MARGIN = 4          # device tolerance = MARGIN * e32 (see check_lists)


def clamp_u(u32):
    """fminf(fmaxf(u, 2^-24), 1 - 2^-24) in fp32; fmax drops a NaN."""
    return np.fmin(np.fmax(np.asarray(u32, dtype=np.float32), U_LO), U_HI)


def _logprobs64(l32, T):
    """float64 log softmax(l / T) of fp32 rows [rows, n]; -inf logits get -inf, NaN logits NaN, a row without a finite maximum all NaN."""
    l = np.asarray(l32, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        m = np.nanmax(np.where(np.isnan(l), -np.inf, l), axis=1, keepdims=True)
        x = (l - m) / float(np.float32(T))
        lse = np.log(np.nansum(np.exp(x), axis=1, keepdims=True))
        return x - lse


def perturbed64(l32, T, phi, G, u32):
    """float64 (lp, g~) [rows, n] of the formula on fp32 inputs; dead children (lp or g not finite) and dead rows (phi or G not finite)
    carry -inf in g~."""
    lp = _logprobs64(l32, T)
    phi, G = (np.asarray(a, dtype=np.float32).astype(np.float64)[:, None] for a in (phi, G))
    u = clamp_u(u32).astype(np.float64)
    with np.errstate(all="ignore"):
        g = phi + lp - np.log(-np.log(u))
        live = np.isfinite(lp) & np.isfinite(g) & np.isfinite(phi) & np.isfinite(G)
        g = np.where(live, g, -np.inf)
        Z = g.max(axis=1, keepdims=True)
        v = G - g + np.log1p(-np.exp(g - Z))
        gt = G - np.maximum(0.0, v) - np.log1p(np.exp(-np.abs(v)))
        gt = np.where(g == Z, G, gt)
    return lp, np.where(live, gt, -np.inf)


def restate_f32(l32, T, phi, G, u32):
    """The formula in np.float32 arithmetic -> g~ fp32 [rows, n] (-inf for the dead). lp as the library documents it: the fp32 exponent
    x = (l - max) / T, the logarithm of the mass and the difference in double, rounded to fp32 once."""
    f = np.float32
    l = np.asarray(l32, dtype=f)
    with np.errstate(all="ignore"):
        m = np.nanmax(np.where(np.isnan(l), NINF, l), axis=1, keepdims=True)
        x = ((l - m) / f(T)).astype(f)
        lp = (x.astype(np.float64) - np.log(np.nansum(np.exp(x.astype(np.float64)), axis=1, keepdims=True))).astype(f)
        phi, G = (np.asarray(a, dtype=f)[:, None] for a in (phi, G))
        u = clamp_u(u32)
        g = ((phi + lp).astype(f) - np.log(-np.log(u)).astype(f)).astype(f)
        live = np.isfinite(lp) & np.isfinite(g) & np.isfinite(phi) & np.isfinite(G)
        g = np.where(live, g, NINF)
        Z = g.max(axis=1, keepdims=True)
        v = ((G - g).astype(f) + np.log1p(-np.exp((g - Z).astype(f)))).astype(f)
        gt = ((G - np.maximum(f(0), v)).astype(f) - np.log1p(np.exp(-np.abs(v)))).astype(f)
    assert gt.dtype == f
    return np.where(live, gt, NINF)


def lists_from(lp, gt, lo, n):
    """(tok int64, lp fp32, g~ fp32) [rows, n]: the live columns by (g~ descending, column ascending), padded with -1 / -inf / -inf. The
    order is taken on the values ROUNDED TO fp32, as a launch takes it on its own fp32 values."""
    g32 = np.asarray(gt).astype(np.float32)
    rows, cols = g32.shape
    order = np.argsort(-g32, axis=1, kind="stable")[:, :n]              # dead columns (-inf) sort last; -0 == +0; ties by column
    if order.shape[1] < n:
        order = np.concatenate([order, np.zeros((rows, n - order.shape[1]), np.int64)], 1)
    g_o = np.take_along_axis(g32, order, 1)
    g_o[:, cols:] = NINF
    live = g_o > NINF
    tok = np.where(live, order + lo, -1).astype(np.int64)
    lp_o = np.where(live, np.take_along_axis(np.asarray(lp), order, 1), -np.inf).astype(np.float32)
    return tok, lp_o, np.where(live, g_o, NINF)


def row_step(logits, lo, hi, n, T, phi, G, u32):
    """The float64 reference of cover_gumbel_topn, its results rounded to fp32 once: (tok, lp, g~) [rows, n]."""
    lp, gt = perturbed64(np.asarray(logits)[:, lo:hi], T, phi, G, u32)
    return lists_from(lp, gt, lo, n)


def merge_gumbel(cum, cand_tok, cand_lp, cand_g, B, feed_pad):
    """cum fp32 [G * B], cand_tok int64 / cand_lp fp32 / cand_g fp32 [G * B, >= B] -> (parent int32, token int64, feed int64, cum_out fp32,
    step_lp fp32, g fp32, each [G * B]; kappa fp32 [G]). The order is (cand_g descending as floats, lower beam, lower rank)."""
    cum = np.asarray(cum, dtype=np.float32)
    tok, lp, cg = np.asarray(cand_tok, dtype=np.int64)[:, :B], np.asarray(cand_lp, dtype=np.float32)[:, :B], np.asarray(cand_g, dtype=np.float32)[:, :B]
    rows = cum.shape[0]
    assert rows % B == 0
    n_g = rows // B
    live = np.isfinite(cum)[:, None] & (tok >= 0) & np.isfinite(lp) & np.isfinite(cg)
    key = np.where(live, cg, NINF).reshape(n_g, B * B)
    key = np.concatenate([key, np.full((n_g, 1), NINF, np.float32)], 1)          # B = 1: rank B exists and is dead
    order = np.argsort(-key, axis=1, kind="stable")[:, :B + 1]                   # stable: equal floats (-0 == +0) by lower b * B + j
    k_o = np.take_along_axis(key, order, 1)
    ok = (k_o[:, :B] > NINF).reshape(rows)
    c = np.minimum(order[:, :B], B * B - 1).reshape(rows)
    b, j = c // B, c % B
    src = (np.arange(rows) // B) * B + b
    with np.errstate(all="ignore"):
        s = (cum[src] + lp[src, j]).astype(np.float32)                           # one fp32 add
    parent = np.where(ok, b, -1).astype(np.int32)
    token = np.where(ok, tok[src, j], -1).astype(np.int64)
    feed = np.where(ok, tok[src, j], feed_pad).astype(np.int64)
    return (parent, token, feed, np.where(ok, s, NINF).astype(np.float32), np.where(ok, lp[src, j], NINF).astype(np.float32),
            np.where(ok, cg[src, j], NINF).astype(np.float32), k_o[:, B].astype(np.float32))


def search(step_logits, n_groups, B, S, lo, hi, uniforms, T=1.0, feed_pad=0):
    """Whole stochastic beam search. step_logits(prefixes) -> fp32 logits [G * B, V] for the int64 prefixes [G * B, i] (a dead beam's
    prefix holds -1); uniforms fp32 [S, G * B, hi - lo]. Returns (tokens [G * B, S], logprobs [G * B, S], scores, perturbed [G * B],
    kappa [G], parents [S, G * B])."""
    from tests import beam_ref as BR
    rows = n_groups * B
    cum, pert = np.full(rows, NINF, np.float32), np.full(rows, NINF, np.float32)
    cum[::B] = 0.0
    pert[::B] = 0.0
    prefixes = np.zeros((rows, 0), np.int64)
    parents, toks, lps = [], [], []
    kappa = None
    for i in range(S):
        ct, cl, cg = row_step(step_logits(prefixes), lo, hi, B, T, cum, pert, uniforms[i])
        parent, token, _, cum, step_lp, pert, kappa = merge_gumbel(cum, ct, cl, cg, B, feed_pad)
        src = (np.arange(rows) // B) * B + np.maximum(parent, 0)
        prefixes = np.concatenate([np.where((parent >= 0)[:, None], prefixes[src], -1), token[:, None]], 1)
        parents.append(parent), toks.append(token), lps.append(step_lp)
    tokens, logprobs = BR.backtrack(np.stack(parents), np.stack(toks), np.stack(lps), B)
    return tokens, logprobs, cum, pert, kappa, np.stack(parents)


def toy_tree(V, S, seed):
    """A V-token, S-step tree: (tables, p) with tables[i][prefix] the fp32 logits after that prefix (shape [V] * (i + 1)) and p[seq] the
    exact float64 probability of every sequence at temperature 1."""
    import itertools
    rng = np.random.default_rng(seed)
    tables = [rng.normal(0, 1.5, size=(V,) * (i + 1)).astype(np.float32) for i in range(S)]
    p = np.zeros((V,) * S)
    for seq in itertools.product(range(V), repeat=S):
        lp = 0.0
        for i in range(S):
            row = tables[i][seq[:i]].astype(np.float64)
            lp += row[seq[i]] - np.log(np.exp(row).sum())
        p[seq] = np.exp(lp)
    assert abs(p.sum() - 1.0) < 1e-12
    return tables, p


def rank0_frequencies_ok(tokens, p, what):
    """tokens int [runs, S] (relative ids): the rank-0 sequences of `runs` independent searches. Their frequencies must lie within 4 sigma
    (binomial) of the exact probabilities p. Prints the worst deviation before it asserts."""
    V, S = p.shape[0], p.ndim
    runs = tokens.shape[0]
    idx = (np.asarray(tokens) * (V ** np.arange(S - 1, -1, -1))).sum(1)
    freq = np.bincount(idx, minlength=V ** S) / runs
    sigma = np.sqrt(p.ravel() * (1 - p.ravel()) / runs)
    dev = np.abs(freq - p.ravel())
    print(f"{what}: rank-0 frequencies over {runs} runs: worst deviation {dev.max():.4f}, worst in sigmas {(dev / sigma).max():.2f}")
    assert (dev <= 4 * sigma).all(), (what, dev.max(), (dev / sigma).max())


# ------------------------------------------------------------------------------------------------ the kernel test cases
# (name, hi - lo, n, lo, extra columns behind hi, T): every (width, n) pair and both temperatures; the first two share a width so that one
# of them runs at lo = 0 on a dense row and the other inside a wider one.
CASES = [("w256-n1", 256, 1, 0, 0, 1.0), ("w256-n5", 256, 5, 37, 11, 0.7), ("w256-n64", 256, 64, 100, 3, 1.0),
         ("w4096-n64", 4096, 64, 5, 2, 0.7), ("w5-n8", 5, 8, 3, 4, 1.0)]
ROWS = 12


@functools.lru_cache(maxsize=None)
def case_data(name):
    """dict(logits fp32 [ROWS, ld], lo, hi, n, T, phi, G, u) of one case. N(0, 3) logits, phi in [-20, 0], G = phi + Gumbel. Special rows:
    0 dead (phi = -inf), 1 dead (G = NaN), 2 -inf columns, 3 all -inf inside the range, 4 uniforms of 0 / 1 / NaN, 5 two equal maxima
    (equal logits AND equal uniforms on two columns, the largest g of the row)."""
    _, w, n, lo, extra, T = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(500 + [c[0] for c in CASES].index(name))
    hi, ld = lo + w, lo + w + extra
    logits = rng.normal(0, 3.0, size=(ROWS, ld)).astype(np.float32)
    phi = -rng.uniform(0, 20, size=ROWS).astype(np.float32)
    G = (phi + rng.gumbel(size=ROWS)).astype(np.float32)
    u = rng.random(size=(ROWS, w), dtype=np.float32)
    phi[0], G[1] = -np.inf, np.nan
    logits[2, lo:hi:2] = -np.inf
    logits[3, lo:hi] = -np.inf
    u[4, 0], u[4, 1 % w], u[4, 2 % w] = 0.0, 1.0, np.nan
    a, b = lo + 1, lo + w - 1
    logits[5, a] = logits[5, b] = 40.0
    u[5, a - lo] = u[5, b - lo] = 0.75
    return dict(logits=logits, lo=lo, hi=hi, n=n, T=T, phi=phi, G=G, u=u)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(lp64, gt64, e32) of a case: the float64 per-column values and the worst |g~ error| of restate_f32 against them over the live columns."""
    c = case_data(name)
    lp, gt = perturbed64(c["logits"][:, c["lo"]:c["hi"]], c["T"], c["phi"], c["G"], c["u"])
    g32 = restate_f32(c["logits"][:, c["lo"]:c["hi"]], c["T"], c["phi"], c["G"], c["u"])
    live = gt > -np.inf
    assert np.array_equal(live, g32 > NINF)
    return lp, gt, float(np.abs(g32.astype(np.float64)[live] - gt[live]).max())


def check_lists(tok, g, lo, n, gt64, e32, what, cap):
    """A launch's lists (tok int64, g fp32, [rows, n]) against the float64 per-column g~ [rows, cols].
    Tolerance: tol = MARGIN * e32, e32 the worst error of the fp32 restatement on the same inputs; the factor 4 is the margin for device
    expf / logf / log1pf being a few ulp where numpy's are at most one and for the log-probability's own logprob_ref.tolerance.
    Exact: the number of live slots of a row and the padding behind them. Value: every live slot's g within tol of the float64 g~ OF ITS OWN
    COLUMN. Ids, per slot: rank j holds the reference's id, unless the reference's g~ at rank j lies within 2 * tol of a neighbouring
    rank's (j - 1 or j + 1; rank n counts) -- an undecided slot, which must hold one of the reference ids within that distance of rank j.
    Ranks whose float64 values are EQUAL (the arg-max children of a row, all exactly G) are not undecided: the column rule decides them.
    At most `cap` of the case's live slots may be undecided. Prints the figures before it asserts; returns (worst error, tol, share)."""
    tok, g = np.asarray(tok), np.asarray(g, dtype=np.float32)
    tol = MARGIN * e32
    worst, und, slots, bad = 0.0, 0, 0, []
    for r in range(tok.shape[0]):
        ref = gt64[r]
        order = np.argsort(-ref, kind="stable")
        n_live = int((ref > -np.inf).sum())
        k = min(n, n_live)
        if not ((tok[r, k:] == -1).all() and (g[r, k:] == NINF).all() and (tok[r, :k] >= lo).all()):
            bad.append((r, "padding / live count", k))
            continue
        sv = ref[order]                                                           # the reference's values by rank
        for j in range(k):
            slots += 1
            c = int(tok[r, j]) - lo
            err = abs(float(g[r, j]) - ref[c]) if 0 <= c < ref.size and ref[c] > -np.inf else np.inf
            worst = max(worst, err)
            if not err <= tol:
                bad.append((r, j, "value", float(g[r, j]), c, err))
            near = (j > 0 and 0 < sv[j - 1] - sv[j] <= 2 * tol) or (j + 1 < n_live and 0 < sv[j] - sv[j + 1] <= 2 * tol)
            if near:
                und += 1
                if c not in set(np.nonzero(np.abs(ref - sv[j]) <= 2 * tol)[0].tolist()):
                    bad.append((r, j, "id of an undecided slot", c))
            elif c != order[j]:
                bad.append((r, j, "id", c, int(order[j])))
    share = und / max(slots, 1)
    print(f"{what}: live slots {slots} | worst |g~ error| {worst:.3e} (bound {tol:.3e} = {MARGIN} * e32 {e32:.3e}) | undecided slots {und} "
          f"({share:.4f} of them, cap {cap}) | violations {len(bad)}")
    assert not bad, (what, bad[:8])
    assert share <= cap, (what, und, slots)
    return worst, tol, share
