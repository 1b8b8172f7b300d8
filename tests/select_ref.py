"""References, error bounds and case tables of tests/test_select_{cpu,gpu}.py: the older half of csrc/select.hip (cover_token_select,
cover_score_select, cover_group_argmax, cover_tokens_to_histories_steps, cover_actions_to_histories). numpy only, no GPU code.

Notation: u = 2^-24 is the unit roundoff of fp32, gamma(k) = k u / (1 - k u) bounds the relative error of k successive roundings.
fp32 division and square root are correctly rounded (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt; the Makefile does
not turn it off), so each costs one u like an add or a product. An fma replaces two roundings by one, so every bound below, which
counts the product and the add, holds with or without contraction.

NaN rule (include/cover_hip.h, cover_token_select): a NaN never wins a comparison, and if nothing wins the pick is the first index of
the range. greedy() and group_argmax() state it with explicit loops (np.argmax treats a NaN as the maximum).

---------------------------------------------------------------------------------------------------------------------------------
1. Sampling path of cover_token_select: the bound B(n, T, row) of sampling_bound().

The kernel picks the first c with csum[c] > tgt, tgt = fl(uni * total), i.e. the first c with q_c > uni where
q_c = csum[c] / (tgt / uni). The float64 reference picks the first c with F_c > uni, F the exact CDF of the weights
w_i = exp((l_i - max) / T). B bounds |q_c - F_c| for every c:

 (a) exponent. The kernel forms x^ = fl(fl(l - max) * fl(1 / T)): three roundings (the difference, the reciprocal, the product; max is
     an input float and exact), so x^ = x (1 + d), |d| <= gamma(3), x = (l - max) / T <= 0: the rounding is amplified by |x|,
     exp(x^) = exp(x) exp(x d), a relative error of expm1(gamma(3) |x|).
 (b) expf. ROCm documents a maximum error of 1 ulp for expf (HIP documentation, "HIP math API", table of single-precision
     mathematical functions: expf, 1 ULP); 1 ulp <= 2 u relative for a normal result. A result below the smallest normal
     2^-126 may be flushed or rounded on the denormal grid: an ABSOLUTE error of at most 2^-126. So the fp32 weight w^_i obeys
         |w^_i - w_i| <= e_i := w_i (expm1(gamma(3) |x_i|) (1 + 2 u) + 2 u) + 2^-126.
     Let E = sum_i e_i, W = sum_i w_i (>= 1: the maximum has weight exp(0)), r = E / W.
 (c) the two chains. total and csum[c] are sequential chains of at most n fp32 adds of non-negative terms, so each is its exact sum
     of the w^ times (1 + theta), |theta| <= gamma(n) (no cancellation: the error is relative to the sum itself):
         csum[c] = (C_c + E_c) (1 + theta_c),  total = (W + E_W) (1 + theta_W),  C_c = sum_{i <= c} w_i,  |E_c|, |E_W| <= E.
 (d) the product tgt = uni * total (1 + d'), |d'| <= u (W >= 1, so no underflow).
 Together q_c = (C_c + E_c) / (W + E_W) * (1 + theta_c) / ((1 + theta_W) (1 + d')). The first factor differs from F_c = C_c / W by
 (E_c W - C_c E_W) / (W (W + E_W)), at most 2 r / (1 - r) in magnitude; the second factor differs from 1 by at most
 g = (2 gamma(n) + u) / (1 - gamma(n) - u)^2. Hence
         B = 2 r / (1 - r) + g (1 + 2 r / (1 - r)).
 gamma(n) dominates: B ~ 2 n u, 4.9e-4 at n = 4096 and 3e-5 at n = 256. The float64 CDF itself (np.cumsum in float64, error
 ~ n 2^-53) is exact on this scale.

 Consequences used by the tests. (i) Every c with F_c <= uni - B has q_c <= uni, and the first c with F_c > uni + B has q_c > uni,
 so the kernel's pick lies in pick_bracket() = [pick(uni - B), pick(uni + B)] for EVERY uniform; (ii) if uni is farther than B from
 every boundary F_0 .. F_{n-2} the bracket is one index and the pick is decided: token == reference, exactly (F_{n-1} = 1 is no
 boundary: when rounding lets no running sum exceed the target, the fallback picks n - 1, which is the reference's pick too).
 A row whose steps are all narrower than 2 B has no decidable uniform under this bound -- the flat rows at n >= 1000. Those are
 decided exactly by another argument: (iii) all weights are expf(0) = 1.0f, sums of ones up to 4096 are exact in fp32, so
 csum[c] = c + 1, tgt = fl(uni * n) and the pick is min(floor(fl(uni * n)), n - 1): flat_pick(). (iv) uni = 0: tgt = 0 and the pick
 is the first c with a non-zero fp32 weight. x >= -87 gives exp(x) > 2^-126, a non-zero result under (b); x <= -105 gives
 exp(x) < 2^-151, below half the smallest denormal, which expf returns as 0 (OCML clamps below -103.972); zero_pick() decides a
 row when no weight in front of the first certainly non-zero one lies between the two.
 The sampled rows of the case table scale with max(T, 1) so that they keep steps wider than 2 B at every temperature.

---------------------------------------------------------------------------------------------------------------------------------
2. cover_score_select's fused cosine: score_bounds(it, act).

Per candidate (and once for the image-text side) the kernel forms, for every d, a^_d = fl(chain over members) / M; then
q = sum_d a^_d^2, nrm = sqrt(q), f^_d = a^_d / nrm, and score = sum_d fit^_d fact^_d.
 (a) member mean: M - 1 adds and a division (0 + x and x / 1 are exact, so M = 1 costs nothing): |a^_d - a_d| <= gamma(M) abar_d,
     abar_d = mean_m |x_{m,d}|. Members may cancel, so this is NOT relative to a_d: t = gamma(M) ||abar|| / ||a|| bounds
     ||a^ - a|| / ||a||, the sine of the angle between them, and the unit vectors differ by at most t / sqrt(1 - t^2) (the chord is at
     most the tangent).
 (b) squared norm: a sum of non-negative terms -- one product, a lane-strided chain of K = ceil(dim / stride) terms (K - 1 adds),
     the xor butterfly (6 adds, of which only ceil(log2(lanes in use)) add a non-zero partner), and for the 1024-thread
     image-text side the chain over the waves in use: R roundings, relative error gamma(R). The square root halves it and adds u, the
     division adds u: f^ = (a^ / ||a^||) (1 + e), |e| <= nu = (gamma(R) / 2 + 2 u) / (1 - gamma(R) - 2 u).
     So ||f^ - f|| <= eta = t / sqrt(1 - t^2) + nu, and | ||f^|| - 1 | <= eta.
 (c) the dot product: exact value f^it . f^act differs from fit . fact by at most eta_it + eta_act + eta_it eta_act (unit vectors);
     its fp32 evaluation (product, K - 1 chain adds over 64 lanes, butterfly: R_dot roundings) adds at most
     gamma(R_dot) sum_d |f^it_d f^act_d| <= gamma(R_dot) (S + eta_it + eta_act + eta_it eta_act), S = sum_d |fit_d fact_d| <= 1.
         bound = (eta_it + eta_act + eta_it eta_act) (1 + gamma(R_dot)) + gamma(R_dot) S.
 1.2e-6 at dim = 7 and 7.0e-6 at dim = 4096 for the two-member cases of the table, 7.8e-6 with 16 members at dim = 128 (their means
 nearly cancel: ||abar|| / ||a|| is large). A worst case over every rounding; the kernel's observed error stays below 1e-7.

---------------------------------------------------------------------------------------------------------------------------------
3. cover_actions_to_histories: out = (v + 1) / 2 * (hi - lo) + lo in fp32. (v + 1) and (hi - lo) are one rounding each, the halving is
exact, the product and the final add one each (or one fma): with t = (v + 1) / 2 and s = hi - lo
         |out^ - out| <= gamma(4) (|t| |s| + |lo|)   (<= 2 gamma(4) max(1, |t|) max(|lo|, |hi|, |hi - lo|)).
Without lo_hi the value passes through, and the gripper column, the past rows and the pad rows are copies or constants: exact.
cover_tokens_to_histories is a table look-up: exact."""
import math

import numpy as np

from tests import member_scores_ref as MR

F32 = np.float32
U = MR.U
gamma = MR.gamma
NAN = F32(np.nan)


def bits(x):
    """fp32 -> its int32 bit patterns (other dtypes pass through), so that NaNs and signed zeros compare."""
    x = np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


# ------------------------------------------------------------------------------------------------ the arg-max rule
def _first_max(v):
    """Index of the first maximum among the non-NaN values, None if there is none (-inf counts: it equals the start value)."""
    best, bi = -math.inf, None
    for i, x in enumerate(v):
        x = float(x)
        if x > best or (bi is None and x == best):
            best, bi = x, i
    return bi


def greedy(row, lo, hi):
    """cover_token_select's greedy rule on one row -> (token, fp32 logit at the token: compare its bits)."""
    row = np.asarray(row, dtype=F32)
    i = _first_max(row[lo:hi])
    pick = lo if i is None else lo + i
    return pick, row[pick]


def group_argmax(scores, gs):
    """cover_group_argmax: the fp32 index-order chain of member_scores_ref.group_argmax with the NaN rule at both levels.
    -> (result int32 [4], best fp32 [2] = {scores[result[0]], gmean[result[1]]}, own bits)."""
    rs = np.asarray(scores, dtype=F32).reshape(-1, gs)
    gsum = np.zeros(rs.shape[0], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(gs):
            gsum = (gsum + rs[:, j]).astype(F32)
        gmean = (gsum / F32(gs)).astype(F32)
    bg = _first_max(gmean) or 0
    bi = _first_max(rs[bg]) or 0
    return np.array([bg * gs + bi, bg, bi, 0], dtype=np.int32), np.array([rs[bg, bi], gmean[bg]], dtype=F32)


# ------------------------------------------------------------------------------------------------ sampling
def _exponents(row, lo, hi, T):
    l = np.asarray(row, dtype=F32)[lo:hi]
    return (l.astype(np.float64) - float(l.max())) / float(F32(T))


def inverse_cdf(row, lo, hi, u, T):
    """-> (token, F float64 [n]): the exact CDF of exp((l - max) / T) over [lo, hi) and the first index whose CDF exceeds u
    (the last index if none does)."""
    w = np.exp(_exponents(row, lo, hi, T))
    F = np.cumsum(w) / w.sum()
    F[-1] = 1.0
    return lo + _pick(F, float(u)), F


def _pick(F, u):
    hit = np.nonzero(F > u)[0]
    return int(hit[0]) if hit.size else F.size - 1


def sampling_bound(row, lo, hi, T):
    """B(n, T, row) of section 1."""
    x = _exponents(row, lo, hi, T)
    n = x.size
    w = np.exp(x)
    e = w * (np.expm1(gamma(3) * np.abs(x)) * (1 + 2 * U) + 2 * U) + 2.0 ** -126
    r = e.sum() / w.sum()
    g = (2 * gamma(n) + U) / (1 - gamma(n) - U) ** 2
    first = 2 * r / (1 - r)
    return first + g * (1 + first)


def pick_bracket(F, u, B):
    """[first, last] relative index the kernel may pick under the bound; one index when u is decided."""
    return _pick(F, float(u) - B), _pick(F, float(u) + B)


def decided(F, u, B):
    """The issue's condition: u is farther than B from every boundary F_0 .. F_{n-2}."""
    return F.size == 1 or bool(np.abs(F[:-1] - float(u)).min() > B)


def flat_pick(n, u):
    """A row of equal logits: csum[c] = c + 1 exactly, tgt = fl(u * n)."""
    return min(int(math.floor(float(F32(u) * F32(n)))), n - 1)


def zero_pick(row, lo, hi, T):
    """u = 0: the first index with a non-zero fp32 weight, or None when an exponent in front of it is in (-105, -87)."""
    x = _exponents(row, lo, hi, T)
    k = int(np.nonzero(x >= -87.0)[0][0])                           # exists: the maximum has x = 0
    return lo + k if bool((x[:k] <= -105.0).all()) else None


WIDTHS = (1, 2, 255, 256, 257, 1000, 4095, 4096)
TEMPERATURES = (0.05, 0.7, 1.0, 20.0)
DISTS = ("peaked", "flat", "normal")
FIXED_U = (F32(0.0), F32(2.0 ** -24), np.nextafter(F32(1), F32(0)))
N_DRAWN, OVERSAMPLE = 16, 4
CELLS = [(n, T, d) for n in WIDTHS for T in TEMPERATURES for d in DISTS]


def cell_id(c):
    return "n%d-T%g-%s" % c


def _cell_seed(cell):
    return 7000 + CELLS.index(cell)


def _build_cell(cell):
    n, T, dist = cell
    rng = np.random.default_rng(_cell_seed(cell))
    scale = max(T, 1.0)                                  # keeps steps wider than 2 B at T = 20 (see the docstring)
    if dist == "flat":
        row = np.full(n, rng.normal(), dtype=F32)
    elif dist == "peaked":                               # one dominant logit over a low ripple, not at either end when n > 2
        row = (0.25 * scale * rng.normal(size=n)).astype(F32)
        row[n // 3] = F32(14.0 * scale)
    else:                                                # wide enough that the mass sits on steps wider than 2 B at n = 4096 too
        row = ((1.0 if n <= 1000 else 4.0) * scale * rng.normal(size=n)).astype(F32)
    _, F = inverse_cdf(row, 0, n, 0.0, T)
    B = sampling_bound(row, 0, n, T)
    drawn = rng.random(N_DRAWN * OVERSAMPLE, dtype=F32)
    if dist == "flat":
        kept = drawn[:N_DRAWN]
        picks = [flat_pick(n, u) for u in kept]
    else:
        kept = np.array([u for u in drawn if decided(F, u, B)][:N_DRAWN], dtype=F32)
        picks = [_pick(F, float(u)) for u in kept]
    return dict(row=row, F=F, B=B, drawn=drawn, kept=kept, picks=np.array(picks, dtype=np.int64))


_CELLS = {}


def sampling_cell(cell):
    """dict(row fp32 [n], F, B, drawn fp32 [64], kept fp32 [<= 16] decided uniforms, picks = their reference picks, relative to lo).
    Computed once per cell: read-only."""
    if cell not in _CELLS:
        _CELLS[cell] = _build_cell(cell)
    return _CELLS[cell]


def fixed_expectation(cell, u):
    """For one of FIXED_U -> (first, last) relative picks allowed: one index wherever the case is decided."""
    n, T, dist = cell
    c = sampling_cell(cell)
    if dist == "flat":
        k = flat_pick(n, u)
        return k, k
    if float(u) == 0.0:
        k = zero_pick(c["row"], 0, n, T)
        if k is not None:
            return k, k
    return pick_bracket(c["F"], u, c["B"])


def emulate_sampler(row, lo, hi, u, T, scan="sequential"):
    """The kernel's fp32 arithmetic in numpy (np.exp on float32 in place of expf) -> (token, q float64 [n] = csum / (tgt / u) for
    u > 0, else csum / total). scan = "pairwise": the running sums by recursive halving; "exclusive": a scan that leaves out the
    element itself -- the stand-ins of the CPU tests."""
    l = np.asarray(row, dtype=F32)[lo:hi]
    inv_t = F32(1.0) / F32(T)
    p = np.exp(((l - l.max()).astype(F32) * inv_t).astype(F32)).astype(F32)
    total = F32(0.0)
    for v in p:
        total = F32(total + v)
    if scan == "sequential":
        cs = np.cumsum(p, dtype=F32)                     # ufunc.accumulate: one chain in index order
    elif scan == "exclusive":
        cs = (np.cumsum(p, dtype=F32) - p).astype(F32)
    else:
        def scan_pw(v):
            if v.size == 1:
                return v.copy()
            h = v.size // 2
            a, b = scan_pw(v[:h]), scan_pw(v[h:])
            return np.concatenate([a, (b + a[-1]).astype(F32)])
        cs = scan_pw(p)
    tgt = F32(F32(u) * total)
    hit = np.nonzero(cs > tgt)[0]
    pick = int(hit[0]) if hit.size else l.size - 1
    den = float(tgt) / float(u) if float(u) > 0 else float(total)
    return lo + pick, cs.astype(np.float64) / den


# ------------------------------------------------------------------------------------------------ greedy rows
WIDE_MIN = 8192                                           # the wide kernel's width threshold
W3 = 4 * 4096 + 4 * 1024 + 3                              # four-in-flight loop + single-load remainder + a 3-element scalar tail
# id -> (lo, width, ld % 4, base offset in floats, kernel the host picks)
GREEDY_LAYOUTS = {
    "w8191-scalar": (0, WIDE_MIN - 1, 0, 0, "scalar"),
    "w8192-wide-no-4x-loop": (0, WIDE_MIN, 0, 0, "wide"),
    "w20483-lo4-wide-all-regimes": (4, W3, 0, 0, "wide"),
    "w20483-lo3-scalar": (3, W3, 0, 0, "scalar"),
    "w20483-ld-odd-scalar": (4, W3, 1, 0, "scalar"),
    "w20483-base-plus-one-float-scalar": (4, W3, 0, 1, "scalar"),
    "w300-narrow": (5, 300, 3, 0, "scalar"),
}
GREEDY_ROWS = ("max-at-lo", "max-at-hi-1", "max-in-tail", "tie-x3-first-wins", "outside-larger", "all-neg-inf", "signed-zero-tie",
               "nan-scattered", "all-nan", "random")
GREEDY_NAN_ROWS = ("nan-scattered", "all-nan")
NAN_PAYLOAD = 0x7FC12345                                  # the all-NaN row's NaN at lo carries a payload: logit_out must return it


def is_wide(lo, width, ld, base_off):
    """launch_token_select's predicate for a greedy call (the buffer itself is 16-byte aligned)."""
    return width >= WIDE_MIN and lo % 4 == 0 and ld % 4 == 0 and base_off % 4 == 0


def greedy_matrix(layout, names, seed=11):
    """-> (flat fp32 buffer, base offset, ld, lo, hi): rows `names` of a [len(names), ld] matrix that starts `base offset` floats into
    the buffer. Everything outside [lo, hi) -- the columns in front, behind and the ld padding -- is +inf and must never win."""
    lo, width, ld_mod, base_off, _ = GREEDY_LAYOUTS[layout]
    hi = lo + width
    ld = hi + 5
    while ld % 4 != ld_mod:
        ld += 1
    rng = np.random.default_rng(seed)
    m = np.full((len(names), ld), np.inf, dtype=F32)
    n4 = width // 4
    for r, name in enumerate(names):
        v = rng.normal(size=width).astype(F32)
        if name == "max-at-lo":
            v[0] = 9.0
        elif name == "max-at-hi-1":
            v[-1] = 9.0
        elif name == "max-in-tail":                      # the scalar tail of the wide kernel when width % 4 != 0, else the last float4
            v[4 * n4 if width % 4 else width - 2] = 9.0
        elif name == "tie-x3-first-wins":                # three threads, waves and (at 20483) loop regimes; one more in the tail
            for c in (min(4 * 700 + 1, width - 2), min(4 * (4096 + 70) + 2, width - 2), width - 1):
                v[c] = 9.0
        elif name == "all-neg-inf":
            v[:] = -np.inf
        elif name == "signed-zero-tie":                  # -0.0 first: the pick is the first zero and logit_out keeps its sign
            v = -np.abs(v) - F32(1.0)
            v[width // 2] = -0.0
            v[width // 2 + 130] = 0.0
            v[width - 1] = 0.0
        elif name == "nan-scattered":
            v[rng.random(width) < 0.3] = np.nan
            v[0] = v[-1] = np.nan
            v[width // 2 + 1] = 9.0
        elif name == "all-nan":
            v[:] = np.nan
            v[0:1] = np.array([NAN_PAYLOAD], dtype=np.int32).view(F32)
        m[r, lo:hi] = v
    buf = np.full(base_off + m.size + 3, np.inf, dtype=F32)
    buf[base_off:base_off + m.size] = m.reshape(-1)
    return buf, base_off, ld, lo, hi


# ------------------------------------------------------------------------------------------------ fused scores
# (M, N, group_size, dim)
SCORE_CASES = [(1, 1, 1, 64),                             # one of everything
               (2, 15, 5, 7),                             # 57 idle lanes, one partial block
               (3, 16, 4, 70),                            # lanes with one or two terms, exactly one block
               (3, 17, 17, 512),                          # one candidate in a second block, one group
               (2, 40, 5, 4096),                          # the largest dim, ragged last block
               (16, 33, 3, 128)]                          # many members
POSITIONS_CASE = (3, 40, 5, 512)                          # the moving candidate sits at n = 3, 19 and N - 1 = 39


def score_inputs(case):
    """member_scores_ref.make_inputs' leaning rows (scores spread over (-0.2, 0.9)), seeded per case; read-only."""
    if case not in _SCORE_INPUTS:
        _SCORE_INPUTS[case] = MR.make_inputs(case, seed=5000 + sum(p * q for p, q in zip(case, (1, 3, 5, 7))))
    return _SCORE_INPUTS[case]


_SCORE_INPUTS = {}


def fused_f64(it, act):
    """-> (fit [dim], fact [N, dim], scores [N]) in float64, nothing rounded. (member_scores_ref.fused_scores_f64 is this score
    rounded to fp32.)"""
    fit = np.asarray(it, dtype=np.float64).mean(axis=0)
    fit = fit / np.linalg.norm(fit)
    fact = np.asarray(act, dtype=np.float64).mean(axis=0)
    fact = fact / np.linalg.norm(fact, axis=-1, keepdims=True)
    return fit, fact, fact @ fit


def _butterfly_adds(lanes):
    return 6 if lanes >= 64 else (0 if lanes <= 1 else math.ceil(math.log2(lanes)))


def score_bounds(it, act):
    """Section 2 -> (eta_it, eta_act [N], score bound [N])."""
    it, act = np.asarray(it, dtype=np.float64), np.asarray(act, dtype=np.float64)
    M, N, dim = act.shape
    gm = gamma(M) if M > 1 else 0.0

    def eta(x, R):                                        # x [M, ..., dim]
        t = gm * np.linalg.norm(np.abs(x).mean(axis=0), axis=-1) / np.linalg.norm(x.mean(axis=0), axis=-1)
        nu = (gamma(R) / 2 + 2 * U) / (1 - gamma(R) - 2 * U)
        return t / np.sqrt(1 - t * t) + nu
    K = -(-dim // 64)
    R_wave = 1 + (K - 1) + _butterfly_adds(min(dim, 64))
    waves = -(-min(dim, 1024) // 64)
    R_block = 1 + (-(-dim // 1024) - 1) + _butterfly_adds(min(dim, 64)) + (waves - 1)
    eta_it, eta_act = eta(it, R_block), eta(act, R_wave)
    fit, fact, _ = fused_f64(it, act)
    S = np.abs(fact * fit).sum(axis=-1)
    both = eta_it + eta_act + eta_it * eta_act
    return float(eta_it), eta_act, both * (1 + gamma(R_wave)) + gamma(R_wave) * S


def decision_f64(scores64, gs):
    """The float64 decision and its two margins -> (result [3], best group mean - second, winner - runner-up in its group); a margin
    without a rival is +inf."""
    rs = np.asarray(scores64, dtype=np.float64).reshape(-1, gs)
    gmean = rs.mean(axis=1)
    bg = int(np.argmax(gmean))
    bi = int(np.argmax(rs[bg]))
    m_g = gmean[bg] - np.delete(gmean, bg).max() if gmean.size > 1 else math.inf
    m_i = rs[bg, bi] - np.delete(rs[bg], bi).max() if gs > 1 else math.inf
    return [bg * gs + bi, bg, bi], float(m_g), float(m_i)


def emulate_score(it, act, drop_lane=None):
    """score_rows_k's arithmetic in numpy fp32 without fma -> scores fp32 [N]. drop_lane: the dot product's butterfly loses that
    lane's partial -- the stand-in of the CPU tests."""
    it, act = np.asarray(it, dtype=F32), np.asarray(act, dtype=F32)
    M, N, dim = act.shape

    def mean(x):
        s = np.zeros(x.shape[1:], dtype=F32)
        for m in range(M):
            s = (s + x[m]).astype(F32)
        return (s / F32(M)).astype(F32)

    def lanes(terms, drop=None):                          # terms [..., dim] -> lane-strided chains + butterfly
        p = np.zeros(terms.shape[:-1] + (64,), dtype=F32)
        for d0 in range(0, dim, 64):
            w = min(64, dim - d0)
            p[..., :w] = (p[..., :w] + terms[..., d0:d0 + w]).astype(F32)
        if drop is not None:
            p[..., drop] = 0
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            p = (p + p[..., lane ^ o]).astype(F32)
        return p[..., 0]
    a_it, a_act = mean(it), mean(act)
    f_it = (a_it / np.sqrt(lanes((a_it * a_it).astype(F32)))).astype(F32)     # the block's own order differs: inside gamma(R_block)
    f_act = (a_act / np.sqrt(lanes((a_act * a_act).astype(F32)))[:, None]).astype(F32)
    return lanes((f_it[None, :] * f_act).astype(F32), drop_lane)


# ------------------------------------------------------------------------------------------------ group_argmax cases
def _rand_scores(N, seed):
    return np.random.default_rng(seed).normal(size=N).astype(F32)


def _ga_tie_groups():
    s = _rand_scores(4096 * 2, 61).reshape(4096, 2)
    s[5] = s[261] = (F32(7.0), F32(6.0))                  # groups 5 and 261 meet in one thread of the 256-thread stride
    return s.reshape(-1), 2


def _ga_tie_candidates():
    s = _rand_scores(1000, 62)
    s[1] = s[257] = F32(7.0)                              # candidates 1 and 257 of one 1000-wide group: the same thread again
    return s, 1000


def _ga_tie_after_rounding():
    # group 1 = (1, 0, 0) sums to 1; group 2 = (1, 2^-25, 2^-25) is larger exactly, but its index-order fp32 chain rounds to 1 twice
    s = np.zeros(12, dtype=F32)
    s[3:6] = (1.0, 0.0, 0.0)
    s[6:9] = (1.0, 2.0 ** -25, 2.0 ** -25)
    return s, 3


def _ga_nan_in_best_group():
    s = _rand_scores(12, 63)
    s[3:6] = (50.0, np.nan, 60.0)                         # would win by far: its mean is a NaN
    return s, 3


def _ga_all_nan():
    return np.full(1000, np.nan, dtype=F32), 4


def _ga_all_nan_wide_group():
    return np.full(1000, np.nan, dtype=F32), 1000


def _ga_all_groups_nan_but_one():
    s = _rand_scores(4096 * 3, 64).reshape(4096, 3)
    s[:, 1] = np.nan
    s[2900] = (-3.0, -2.0, -4.0)
    return s.reshape(-1), 3


def _ga_every_mean_nan_numbers_in_group0():
    s = _rand_scores(15, 65).reshape(5, 3)                # no group wins: group 0, and inside it the first maximum among the numbers
    s[:, 0] = np.nan
    s[0] = (np.nan, 1.0, 2.0)
    return s.reshape(-1), 3


GROUP_ARGMAX_SHAPES = [(1, 1), (12, 3), (1000, 1000), (4096, 1), (8192, 2), (4096 * 3, 3)]
GROUP_ARGMAX_TIES = {"groups-5-and-261": _ga_tie_groups, "candidates-1-and-257": _ga_tie_candidates,
                     "tie-after-fp32-rounding": _ga_tie_after_rounding}
GROUP_ARGMAX_NAN = {"nan-in-best-group": _ga_nan_in_best_group, "all-nan": _ga_all_nan, "all-nan-one-wide-group": _ga_all_nan_wide_group,
                    "all-groups-nan-but-one": _ga_all_groups_nan_but_one,
                    "every-mean-nan-numbers-in-group-0": _ga_every_mean_nan_numbers_in_group0}


def group_argmax_shape_scores(N, gs):
    return _rand_scores(N, 60000 + N + gs)


# ------------------------------------------------------------------------------------------------ histories
HIST_STEPS = [(0, 1), (9, 1), (0, 10), (3, 3), (2, 8)]   # (n_past, n_use)
HIST_N = (1, 25, 26, 77)                                  # 26 x 10 = 260 threads: four into a second block
TOK_VOCAB, N_CENTERS = 32000, 255
PAD_VALUE = -5.0


def hist_centers():
    """The 255 bin centres of the 256-bin de-tokeniser, with three gripper-relevant entries replaced: exactly 0.5, the float below
    it, and a NaN (0.5 and NaN binarise to 1, the float below to 0)."""
    edges = np.linspace(-1, 1, N_CENTERS + 1)
    c = ((edges[:-1] + edges[1:]) / 2.0).astype(F32)
    c[100], c[101], c[102] = F32(0.5), np.nextafter(F32(0.5), F32(0)), NAN
    return c


def hist_past(n_past, seed=70):
    return (0.02 * np.random.default_rng(seed).normal(size=(n_past, 7))).astype(F32) if n_past else None


def hist_tokens(N, n_use, seed=71):
    """int64 [N, ld] with ld = 7 n_use + 5 columns of padding (token for bin 7, which no used entry of row 0 decodes to). Row 0 holds
    the edge ids: both end bins, one beyond each, -1 and 2^31 - 1, and the three special gripper bins."""
    rng = np.random.default_rng(seed + 100 * N + n_use)
    ld = 7 * n_use + 5
    t = np.full((N, ld), TOK_VOCAB - 1 - 7, dtype=np.int64)
    t[:, :7 * n_use] = rng.integers(TOK_VOCAB - N_CENTERS - 3, TOK_VOCAB + 2, size=(N, 7 * n_use))
    edge = [TOK_VOCAB - 1, TOK_VOCAB - N_CENTERS, TOK_VOCAB, TOK_VOCAB - N_CENTERS - 1, -1, 2 ** 31 - 1]
    t[0, :6] = edge
    t[0, 6] = TOK_VOCAB - 1 - 100                         # gripper bin 100: exactly 0.5
    if N > 1:
        t[1, 6] = TOK_VOCAB - 1 - 101
        t[N - 1, 7 * n_use - 1] = TOK_VOCAB - 1 - 102     # the last used entry of the last candidate: the NaN centre
        t[N - 1, :6] = edge[::-1]
    return t


def _frame(N, n_past, n_use, past, dtype):
    n_pad = 10 - n_past - n_use
    hist = np.empty((N, 10, 7), dtype=dtype)
    hist[:, :n_pad] = PAD_VALUE
    if n_past:
        hist[:, n_pad:n_pad + n_past] = past
    pad = np.zeros((N, 10), dtype=np.uint8)
    pad[:, :n_pad] = 1
    return hist, pad, n_pad + n_past


def histories_tokens(tokens, tok_vocab, centers, past, n_use):
    """Exact -> (hist fp32 [N, 10, 7], pad uint8 [N, 10])."""
    N = tokens.shape[0]
    n_past = 0 if past is None else past.shape[0]
    hist, pad, first = _frame(N, n_past, n_use, past, F32)
    b = np.clip(tok_vocab - tokens[:, :7 * n_use].astype(object) - 1, 0, centers.size - 1).astype(np.int64)   # Python ints: no wrap
    a = centers[b].reshape(N, n_use, 7).copy()
    a[..., 6] = np.where(a[..., 6] < F32(0.5), F32(0), F32(1))       # a NaN is not below 0.5
    hist[:, first:] = a
    return hist, pad


def histories_actions(actions, n_use, lo_hi, past):
    """float64 -> (hist float64 [N, 10, 7], pad, bound float64 [N, 10, 7]: 0 wherever the value is a copy or a constant)."""
    a = np.asarray(actions, dtype=F32)[:, :n_use, :7]
    N = a.shape[0]
    n_past = 0 if past is None else past.shape[0]
    hist, pad, first = _frame(N, n_past, n_use, None if past is None else past.astype(np.float64), np.float64)
    bound = np.zeros_like(hist)
    out = a.astype(np.float64)
    if lo_hi is not None:
        lo, hi = np.asarray(lo_hi[:6], dtype=np.float64), np.asarray(lo_hi[6:], dtype=np.float64)
        t = (out[..., :6] + 1.0) / 2.0
        out[..., :6] = t * (hi - lo) + lo
        bound[:, first:, :6] = gamma(4) * (np.abs(t) * np.abs(hi - lo) + np.abs(lo))
    out[..., 6] = np.where(a[..., 6] < F32(0.5), 0.0, 1.0)
    hist[:, first:] = out
    return hist, pad, bound


def hist_actions(N, n_use, seed=72):
    """fp32 [N, chunk, 32]: columns 0-6 are the action, the rest NaN. Values beyond [-1, 1], exactly -1 and +1, and the three gripper
    inputs 0.5, the float below it and NaN."""
    rng = np.random.default_rng(seed + 100 * N + n_use)
    chunk = n_use + 2
    x = np.full((N, chunk, 32), np.nan, dtype=F32)
    x[:, :, :7] = rng.uniform(-1.3, 1.3, size=(N, chunk, 7)).astype(F32)
    x[0, 0, :7] = (-1.0, 1.0, -1.5, 2.0, 0.0, -0.0, 0.5)
    x[N - 1, n_use - 1, 6] = np.nextafter(F32(0.5), F32(0))
    if N > 1:
        x[1, 0, 6] = np.nan
    return x


def hist_lo_hi():
    """p01 | p99 of the kind the dataset statistics hold (|values| below 1, lo < hi), fixed here."""
    lo = np.array([-0.029, -0.042, -0.026, -0.081, -0.093, -0.21], dtype=F32)
    hi = np.array([0.028, 0.041, 0.040, 0.082, 0.078, 0.19], dtype=F32)
    return np.concatenate([lo, hi])
