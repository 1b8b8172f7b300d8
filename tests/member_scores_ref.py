"""Reference of cover_member_scores (include/cover_hip.h) and the case table of tests/test_member_scores_{cpu,gpu}.py.

The kernel's arithmetic is specified rounding by rounding, so the reference restates it in numpy with every intermediate held as
np.float32: the 64 lane-strided chains of a wave as a [..., 64] array that takes one rounded product and one rounded add per 64-wide
slice of the row, the xor butterfly as six array adds over those 64 partials, the member-order chains of the mean and of the sum of
squares as explicit loops (never np.sum, which is pairwise), np.sqrt on float32 and the two-rounding penalty. The GPU results are
compared with it as integer bit patterns."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32
MODES = ("lcb", "min")

# (M, N, group_size, dim)
CASES = [(3, 40, 5, 512),           # ragged last block (40 = 2 x 16 + 8)
         (1, 16, 1, 512),           # M = 1
         (16, 7, 7, 512),           # the largest M, one group, one partial block
         (3, 512, 16, 512),         # config 5's size
         (2, 33, 3, 70),            # dim not a multiple of 64: lanes with one or two terms
         (2, 5, 5, 1),              # 63 idle lanes
         (3, 16, 4, 4096),          # the largest dim
         (2, 4096, 1, 64)]          # 4096 groups, the limit of group_argmax_dev
KAPPAS = (0.0, 0.5, 1000.0)
RUNS = [("lcb", k) for k in KAPPAS] + [("min", 0.0)]
KEYS = ("member_scores", "mean", "spread", "min", "min_member", "robust", "result", "best", "member_result", "member_best")


def case_id(c):
    return "x".join(map(str, c))


def gamma(k):
    return k * U / (1.0 - k * U)


def _unit(x):
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(F32)


def make_inputs(case, seed=None):
    """-> it fp32 [M, dim], act fp32 [M, N, dim]: seeded unit rows (to fp32 rounding). Member m's candidate rows lean towards its
    image-text row by a cosine drawn per (member, candidate), so the members disagree by candidate and the scores spread over
    (-0.2, 0.9) instead of crowding around 0 as independent directions in a high dimension would."""
    M, N, gs, dim = case
    rng = np.random.default_rng(4000 + CASES.index(case) if seed is None else seed)
    it = _unit(rng.normal(size=(M, dim)))
    c = rng.uniform(-0.2, 0.9, size=(M, N, 1))
    noise = rng.normal(size=(M, N, dim))
    noise /= np.linalg.norm(noise, axis=-1, keepdims=True)
    act = _unit(c * it[:, None, :].astype(np.float64) + np.sqrt(1.0 - c * c) * noise)
    if dim == 1:            # a unit row is +1 or -1: members of opposite sign average to the zero vector, whose fused score is 0 / 0.
        it = np.ones_like(it)                                   # So the sign is the candidate's, the same under every member
        act = np.repeat(act[:1], M, axis=0)
    return it, act


def flip_inputs():
    """The constructed flip: M = 3, dim = 512, one group of two. Every it[m] = e_0, act[m] = c_m e_0 + sqrt(1 - c_m^2) e_{1 + m}.
    Candidate A, c = (1, 1, 0.1): fused score 0.90370, spread 0.42426, min 0.1. Candidate B, c = (0.75, 0.75, 0.75): fused score
    0.89113, spread 0."""
    M, dim = 3, 512
    it = np.zeros((M, dim), dtype=F32)
    it[:, 0] = 1.0
    act = np.zeros((M, 2, dim), dtype=F32)
    for n, cs in enumerate(((1.0, 1.0, 0.1), (0.75, 0.75, 0.75))):
        for m, c in enumerate(cs):
            act[m, n, 0] = c
            act[m, n, 1 + m] = np.sqrt(1.0 - c * c)
    return it, act


def tie_inputs():
    """M = 3, N = 16 in groups of 4, dim = 512: candidates 0 and 1 are one row, ahead of every other under every member (cosine 0.95;
    candidates 2 and 3 follow at 0.85, which puts their group ahead too), and group 1 is a copy of group 0 -- the first candidate and
    the first group have to win."""
    case = (3, 16, 4, 512)
    it, act = make_inputs(case, seed=99)
    M, N, gs, dim = case
    rng = np.random.default_rng(98)

    def leaning(c):
        noise = rng.normal(size=(M, dim))
        noise /= np.linalg.norm(noise, axis=-1, keepdims=True)
        return _unit(c * it.astype(np.float64) + np.sqrt(1.0 - c * c) * noise)
    act = act.copy()
    act[:, 0] = act[:, 1] = leaning(0.95)
    act[:, 2], act[:, 3] = leaning(0.85), leaning(0.85)
    act[:, 4:8] = act[:, 0:4]
    return case, it, act


def fused_scores_f64(it, act):
    """cover_score_select's fused score -- the cosine of the member-averaged, renormalised embeddings -- in float64, rounded once to
    fp32. The CPU tests' stand-in for the `scores` input (any fp32 [N] would do: the kernel only reads it); the GPU tests take the
    device's own bits from ops.score_select instead."""
    fit = it.astype(np.float64).mean(axis=0)
    fit /= np.linalg.norm(fit)
    fact = act.astype(np.float64).mean(axis=0)
    fact /= np.linalg.norm(fact, axis=-1, keepdims=True)
    return (fact @ fit).astype(F32)


def member_rows(it, act):
    """s [M, N]: lane l's chain p = p + it[d] * act[d] over d = l, l + 64, ..., then the butterfly over the 64 partials."""
    it, act = np.asarray(it, dtype=F32), np.asarray(act, dtype=F32)
    M, N, dim = act.shape
    p = np.zeros((M, N, 64), dtype=F32)
    for d0 in range(0, dim, 64):
        w = min(64, dim - d0)                                    # lanes >= w have no term in this slice (or none at all)
        prod = (it[:, None, d0:d0 + w] * act[:, :, d0:d0 + w]).astype(F32)
        p[:, :, :w] = (p[:, :, :w] + prod).astype(F32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = (p + p[:, :, lane ^ o]).astype(F32)
    assert (p == p[:, :, :1]).all() or np.isnan(p).any()         # a + b == b + a: every lane ends with the same bits
    return np.ascontiguousarray(p[:, :, 0])


def group_argmax(scores, gs):
    """cover_group_argmax: index-order fp32 group sums / group_size, first maximum wins at both levels."""
    rs = np.asarray(scores, dtype=F32).reshape(-1, gs)
    gsum = np.zeros(rs.shape[0], dtype=F32)
    for j in range(gs):
        gsum = (gsum + rs[:, j]).astype(F32)
    gmean = (gsum / F32(gs)).astype(F32)
    bg = int(np.argmax(gmean))
    bi = int(np.argmax(rs[bg]))
    return np.array([bg * gs + bi, bg, bi, 0], dtype=np.int32), np.array([rs[bg, bi], gmean[bg]], dtype=F32)


def reference(it, act, scores, group_size, kappa, mode):
    """The specified arithmetic -> dict of numpy arrays under KEYS."""
    scores = np.asarray(scores, dtype=F32)
    s = member_rows(it, act)
    M, N = s.shape
    t = np.zeros(N, dtype=F32)
    for m in range(M):
        t = (t + s[m]).astype(F32)
    mean = (t / F32(M)).astype(F32)
    ss = np.zeros(N, dtype=F32)
    for m in range(M):
        dv = (s[m] - mean).astype(F32)
        sq = (dv * dv).astype(F32)
        ss = (ss + sq).astype(F32)
    var = (ss / F32(M)).astype(F32)
    spread = np.sqrt(var)
    assert spread.dtype == F32
    mn, arg = s[0].copy(), np.zeros(N, dtype=np.int32)
    for m in range(1, M):
        rep = s[m] < mn                                          # first minimum wins, a NaN never replaces
        mn = np.where(rep, s[m], mn).astype(F32)
        arg = np.where(rep, m, arg).astype(np.int32)
    k = F32(kappa)
    if mode == "min":
        robust = mn.copy()
    elif k == 0:
        robust = scores.copy()
    else:
        pen = (k * spread).astype(F32)
        robust = (scores - pen).astype(F32)                      # two roundings
    result, best = group_argmax(robust, group_size)
    mres = [group_argmax(s[m], group_size) for m in range(M)]
    return dict(member_scores=s, mean=mean, spread=spread, min=mn, min_member=arg, robust=robust, result=result, best=best,
                member_result=np.stack([r for r, _ in mres]), member_best=np.stack([b for _, b in mres]))


_INPUTS = {}


def case_inputs(case):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    if case not in _INPUTS:
        _INPUTS[case] = make_inputs(case)
    return _INPUTS[case]
