"""Reference of cover_prior_select (include/cover_hip.h) and the case table of tests/test_prior_select_{cpu,gpu}.py.

The kernel's arithmetic is specified rounding by rounding, so the reference restates it in numpy fp32 with explicit sequential loops
(over steps for the prior, over the members for a group mean: one np.float32 add per step, vectorised over the candidates only) --
never np.sum, which is pairwise -- and the GPU results are compared with it as integer bit patterns.

A case is one combination of shape, memory layout, pad masking, length normalisation, beta and input variant."""
import itertools

import numpy as np

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of fp32

# (N, group_size, steps, top_m): the smallest shapes at which the kernel can still go wrong
SHAPES = [(1, 1, 1, 1), (7, 7, 3, 7), (40, 5, 7, 5), (48, 3, 256, 2),
          (300, 1, 2, 1),           # more groups than a 256-thread block
          (4096, 1, 1, 0),          # 4096 groups (the LDS array's size), ranked_out NULL
          (4096, 4096, 2, 64),      # one group of 4096 (the ranking's LDS array), top_m at its limit
          (512, 64, 7, 64)]
LAYOUTS = ("candidate-major", "step-major")
BETAS = (0.0, 0.05, 1.0)
VARIANTS = ("uniform", "quantised", "neginf")
PAD_ID = 0


def cases(variants=VARIANTS, shapes=SHAPES):
    return [dict(shape=s, layout=l, with_tokens=w, length_normalize=ln, beta=b, variant=v)
            for s, v, l, w, ln, b in itertools.product(shapes, variants, LAYOUTS, (False, True), (False, True), BETAS)]


def case_id(c):
    return (f"{'x'.join(map(str, c['shape']))}-{c['variant']}-{c['layout']}-{'tok' if c['with_tokens'] else 'notok'}-"
            f"{'norm' if c['length_normalize'] else 'sum'}-b{c['beta']}")


def make_inputs(c):
    """-> scores fp32 [N], logprobs fp32 [N, steps], tokens int64 [N, steps] or None (all in candidate-major order; the layout is the
    caller's to apply). The inputs depend on the shape, the variant and with_tokens only, so that the beta = 0 run of a case is the
    baseline of its beta > 0 runs."""
    N, gs, steps, top_m = c["shape"]
    seed = 1000 * SHAPES.index(c["shape"]) + 10 * VARIANTS.index(c["variant"]) + int(c["with_tokens"]) + 77
    rng = np.random.default_rng(seed)
    scores = rng.uniform(0.0, 0.3, N).astype(F32)
    lps = (-rng.uniform(0.1, 2.0, (N, steps))).astype(F32)
    if c["variant"] == "quantised":                    # exact ties are common: multiples of 1/8 and of 1/4
        scores = (np.floor(scores * 8.0 + 0.5) / 8.0).astype(F32)
        lps = (-np.ceil(-lps * 4.0) / 4.0).astype(F32)
    tokens = None
    forced = np.zeros((N, steps), dtype=bool)          # steps that stay counted: they carry this variant's -inf entries
    if c["variant"] == "neginf":
        G = N // gs
        g = G // 2
        forced[g * gs:(g + 1) * gs, 0] = True          # one whole group
        for n in rng.choice(N, size=min(3, N), replace=False):
            forced[n, rng.integers(steps)] = True
        lps[forced] = -np.inf
    if c["with_tokens"]:
        tokens = rng.integers(1, 500, (N, steps)).astype(np.int64)
        pad = (rng.uniform(size=(N, steps)) < 0.25) & ~forced
        if N > 1 or c["variant"] != "neginf":
            pad[N // 2] = ~forced[N // 2]              # one candidate whose every (unforced) step is a pad
        tokens[pad] = PAD_ID
        junk = pad & (rng.uniform(size=(N, steps)) < 0.5)
        lps[junk] = -np.inf                            # a pad scored elsewhere scores -inf: it must not be read into the sum
    return scores, lps, tokens


def reference(scores, lps, tokens, pad_id, group_size, beta, length_normalize, top_m):
    """The specified arithmetic. scores fp32 [N]; lps fp32 [N, steps]; tokens int64 [N, steps] or None."""
    scores = np.asarray(scores, dtype=F32)
    lps = np.asarray(lps, dtype=F32).reshape(len(scores), -1)
    N, steps = lps.shape
    counted = np.ones((N, steps), dtype=bool) if tokens is None else (np.asarray(tokens).reshape(N, steps) != pad_id)
    with np.errstate(invalid="ignore", over="ignore"):
        prior = np.zeros(N, dtype=F32)
        for t in range(steps):                                                   # one chain of fp32 adds in step order
            prior = np.where(counted[:, t], (prior + lps[:, t]).astype(F32), prior).astype(F32)
        if length_normalize:
            prior = (prior / np.maximum(counted.sum(axis=1), 1).astype(F32)).astype(F32)
        b = F32(beta)
        combined = scores.copy() if b == 0 else (scores + (b * prior).astype(F32)).astype(F32)   # two roundings
        G = N // group_size
        rs = combined.reshape(G, group_size)
        gsum = np.zeros(G, dtype=F32)
        for j in range(group_size):                                              # index-order fp32 sum
            gsum = (gsum + rs[:, j]).astype(F32)
        gmean = (gsum / F32(group_size)).astype(F32)
    bg = int(np.argmax(gmean))                                                   # first maximum; all -inf: 0
    bi = int(np.argmax(rs[bg]))
    order = np.argsort(-rs[bg], kind="stable")                                   # descending value, equal values by ascending index
    ranked = (bg * group_size + order[:top_m]).astype(np.int32)
    return dict(prior=prior, combined=combined, group_mean=gmean, result=np.array([bg * group_size + bi, bg, bi, 0], dtype=np.int32),
                best=np.array([rs[bg, bi], gmean[bg]], dtype=F32), ranked=ranked)


_REFS = {}


def case_reference(c):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    key = case_id(dict(c, layout=""))                     # the layout is how the inputs lie in memory, not what they are
    if key not in _REFS:
        scores, lps, tokens = make_inputs(c)
        N, gs, steps, top_m = c["shape"]
        _REFS[key] = reference(scores, lps, tokens, PAD_ID, gs, c["beta"], c["length_normalize"], top_m)
    return _REFS[key]


def reference_f64(scores, lps, tokens, pad_id, group_size, beta, length_normalize):
    """The same decision in float64, with the margins that decide whether fp32 can be held to it: -> (winner, decided). The winner is
    decided when the float64 gap between the two best group means and the gap between the two best members of the winning group both
    exceed the fp32 error of the values compared. Per candidate that error is the chain's, steps * 2^-24 * sum |lp| (times beta, and
    divided by the count when normalised), plus the two roundings of the product and the sum; a group mean adds its own chain,
    group_size * 2^-24 * sum |combined| / group_size, and the rounding of the division."""
    s = np.asarray(scores, dtype=np.float64)
    lp = np.asarray(lps, dtype=np.float64).reshape(len(s), -1)
    N, steps = lp.shape
    counted = np.ones((N, steps), dtype=bool) if tokens is None else (np.asarray(tokens).reshape(N, steps) != pad_id)
    with np.errstate(invalid="ignore"):
        x = np.where(counted, lp, 0.0)
        prior = x.sum(axis=1)
        mag = np.abs(x).sum(axis=1)
        div = np.maximum(counted.sum(axis=1), 1) if length_normalize else 1.0
        prior, mag = prior / div, mag / div
        b = float(F32(beta))
        combined = s if b == 0 else s + b * prior
        err = np.zeros(N) if b == 0 else b * (steps * U * mag + U * np.abs(prior)) + U * (np.abs(b * prior) + np.abs(combined))
        err = np.where(np.isfinite(combined), err, 0.0)
        rs, re = combined.reshape(-1, group_size), err.reshape(-1, group_size)
        gmean = rs.mean(axis=1)
        gerr = re.mean(axis=1) + group_size * U * np.abs(rs).sum(axis=1) / group_size + U * np.abs(gmean)
        gerr = np.where(np.isfinite(gmean), gerr, 0.0)

        def top2(v, e):
            o = np.argsort(-v, kind="stable")
            if len(o) == 1:
                return int(o[0]), True
            gap = v[o[0]] - v[o[1]]                  # -inf against -inf: nan, undecided
            return int(o[0]), bool(gap > e[o[0]] + e[o[1]])
        bg, ok_g = top2(gmean, gerr)
        bi, ok_i = top2(rs[bg], re[bg])
    return bg * group_size + bi, ok_g and ok_i
