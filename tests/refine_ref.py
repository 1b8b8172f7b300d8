"""Reference of cover_refine_tokens / cover_refine_actions (include/cover_hip.h) and the case table of tests/test_refine_{cpu,gpu}.py.

The ranking is restated as a stable sort on (NaN flag, -score with -0 and +0 merged, index); the n_elite best rows of every group are
gathered in that order and tests/augment_ref.py's reference_tokens / reference_actions run on the gathered rows -- the fit is imported,
not restated -- so rows n_elite.. of the output are the augmentation of its own first n_elite rows. The GPU results are compared with it
as integer bit patterns.

A case is one combination of form ("tokens" / "actions"), shape (G, S, m, K, h), memory layout and score variant."""
import numpy as np

from tests import augment_ref as AR

F32 = np.float32
TOK_VOCAB = AR.TOK_VOCAB

# (G, S, m, K, h): groups (prompts), scored rows per group, elites, new rows per group, steps
SHAPES = [(1, 1, 1, 1, 1),        # smallest case
          (1, 2, 1, 3, 1),        # one elite, sd 0
          (2, 5, 2, 32, 1),
          (3, 37, 4, 65, 2),      # S not a power of two: dead keys are in play
          (2, 64, 8, 56, 4),
          (1, 300, 5, 7, 2),      # more than one key per thread, n2 = 512
          (1, 4096, 16, 4, 1)]    # the LDS limit
FLOAT_ONLY = [(2, 5, 5, 3, 50),   # 350 statistics items: more than one pass of the 256-thread block; m == S
              (2, 9, 3, 6, 3)]    # read through the strides (chunk * 32, 32) of a [N, chunk, 32] buffer
STRIDED = (2, 9, 3, 6, 3)
VARIANTS = ("distinct", "ties", "all_equal", "signed_zero", "neg_inf", "nan", "reverse", "k0")
MAX_INFEASIBLE = 0.25             # the share of the (form, shape, variant) grid the feasibility rule may drop


def token_row_stride(shape):
    """The row stride, in elements, the token form of a shape is read through: beyond 7 h at every other shape of the table."""
    return 7 * shape[4] + (3 if SHAPES.index(shape) % 2 else 0)


def feasible(form, shape, variant):
    S = shape[1]
    if variant in ("all_equal", "neg_inf", "reverse"):
        return S >= 2                           # one row has nothing to be ordered against
    if variant in ("signed_zero", "nan"):
        return S >= 3                           # a -0, a +0 and a negative; a +NaN, a -NaN and a number
    if variant == "ties":
        return S >= 4                           # three values among four rows: at least one tie
    return True


def grid(forms=("tokens", "actions")):
    return [(f, s, v) for f in forms for s in SHAPES + (FLOAT_ONLY if f == "actions" else []) for v in VARIANTS]


def cases(forms=("tokens", "actions"), shapes=None, variants=VARIANTS):
    return [dict(form=f, shape=s, variant=v) for f, s, v in grid(forms)
            if (shapes is None or s in shapes) and v in variants and feasible(f, s, v)]


def case_id(c):
    return f"{c['form']}-{'x'.join(map(str, c['shape']))}-{c['variant']}"


def make_scores(variant, G, S, m, rng):
    """-> fp32 [G, S]."""
    if variant in ("distinct", "k0"):
        s = np.stack([rng.permutation(S) for _ in range(G)]).astype(F32) * F32(0.37) - F32(3.0)
    elif variant == "reverse":
        s = np.broadcast_to(np.arange(S, dtype=F32) * F32(0.01) - F32(1.0), (G, S)).copy()
    elif variant == "ties":
        s = rng.choice(np.array([-0.5, 0.25, 1.0], dtype=F32), (G, S))
    elif variant == "all_equal":
        s = np.full((G, S), 0.7, dtype=F32)
    elif variant == "signed_zero":              # zeros of both signs, -0.0 at the lowest index, among negatives: the zeros are the best rows
        s = -rng.uniform(0.1, 1.0, (G, S)).astype(F32)
        for g in range(G):
            idx = np.sort(rng.choice(S, size=max(2, min(S - 1, S // 3)), replace=False))
            s[g, idx] = np.where(np.arange(len(idx)) % 2 == 0, F32(-0.0), F32(0.0))
    elif variant == "neg_inf":                  # fewer finite rows than elites: the last elites are the first -inf rows by index
        s = np.full((G, S), -np.inf, dtype=F32)
        for g in range(G):
            idx = rng.choice(S, size=m // 2, replace=False)
            s[g, idx] = rng.uniform(-1.0, 1.0, len(idx)).astype(F32)
    elif variant == "nan":                      # NaNs of both signs (+NaN at the lowest index) around a few numbers, -inf among them
        s = np.empty((G, S), dtype=F32)
        for g in range(G):
            idx = rng.choice(np.arange(1, S), size=min(S - 2, max(2, m - 1)), replace=False)   # the numbers; row 0 stays a NaN
            rest = np.setdiff1d(np.arange(S), idx)                                              # the NaN rows: +NaN, -NaN, +NaN, ... by index
            s[g, rest] = np.where(np.arange(len(rest)) % 2 == 0, 0x7FC00000, 0xFFC00000).astype(np.uint32).view(F32)
            s[g, idx] = rng.uniform(-1.0, 1.0, len(idx)).astype(F32)
            s[g, idx[::2]] = -np.inf
    else:
        raise ValueError(variant)
    return np.ascontiguousarray(s, dtype=F32)


def make_inputs(c):
    """-> dict: tokens int64 [G*S, 7h] or actions fp32 [G*S, h, 7] (contiguous; the layout is the caller's to apply), scores fp32 [G*S],
    normals fp32 [G, K, h, 6], centers fp32 [255], sigma, sd_floor, clip, and S / m / K as the case runs them (K = 0 for k0)."""
    form, (G, S, m, K, h), variant = c["form"], c["shape"], c["variant"]
    seed = 1000 * (SHAPES + FLOAT_ONLY).index(c["shape"]) + 10 * VARIANTS.index(variant) + (5 if form == "actions" else 0) + 77
    rng = np.random.default_rng(seed)
    if variant == "k0":
        K = 0
    N = G * S
    centers = AR.openvla_centers()
    b = rng.integers(20, 235, (N, h, 7))
    cls = rng.integers(0, 2, (N, h))            # gripper class: bins 192.. are >= 0.5
    b[..., 6] = np.where(cls == 1, rng.integers(195, 250, (N, h)), rng.integers(5, 185, (N, h)))
    z = rng.standard_normal((G, K, h, 6)).astype(F32)
    out = dict(S=S, m=m, K=K, normals=z, centers=centers, sigma=1.25, sd_floor=0.004, clip=(-1.0, 1.0),
               scores=make_scores(variant, G, S, m, rng).reshape(N))
    if form == "tokens":
        out["tokens"] = (TOK_VOCAB - 1 - b).astype(np.int64).reshape(N, 7 * h)
    else:
        out["actions"] = (centers[b].astype(np.float64) + rng.uniform(-0.003, 0.003, b.shape)).astype(F32)
    return out


# ------------------------------------------------------------------------------------------------ the specified order
def rank_order(scores):
    """scores fp32 [S] -> the row indices by rank: a stable sort on (NaN flag, -score with -0 and +0 merged, index)."""
    s = np.asarray(scores, dtype=F32)
    nan = np.isnan(s)
    with np.errstate(invalid="ignore"):
        neg = np.where(nan, F32(0.0), -(s + F32(0.0)))                 # -0.0 + 0.0 == +0.0: one score
    return np.lexsort((np.arange(len(s)), neg, nan))                   # the last key is the primary one


def reference(src, scores, S, m, K, z, form, centers=None, steps=None, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0), tok_vocab=TOK_VOCAB):
    """src: int64 [G*S, >= 7 steps] tokens or fp32 [G*S, h, >= 7] actions -> dict(out, elite_rows int32 [G, m], elite_scores fp32 [G, m],
    mean, sd, votes): augment_ref's reference on the gathered elites."""
    scores = np.asarray(scores, dtype=F32)
    G = len(scores) // S
    order = np.stack([rank_order(scores[g * S:(g + 1) * S])[:m] for g in range(G)])          # [G, m]
    rows = (order + S * np.arange(G)[:, None]).astype(np.int32)
    gathered = np.asarray(src)[rows.reshape(-1)]
    if form == "tokens":
        r = AR.reference_tokens(gathered, m, K, z, centers, tok_vocab, steps, sigma, sd_floor, clip)
    else:
        r = AR.reference_actions(gathered, m, K, z, sigma, sd_floor, clip)
    return dict(out=r["out"], elite_rows=rows, elite_scores=scores[rows], mean=r["mean"], sd=r["sd"], votes=r["votes"], order=order)


def reference_of(inp, form):
    h = inp["normals"].shape[2]
    return reference(inp[form], inp["scores"], inp["S"], inp["m"], inp["K"], inp["normals"], form, inp["centers"], h, inp["sigma"],
                     inp["sd_floor"], inp["clip"])


_REFS = {}


def case_reference(c):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    key = case_id(c)
    if key not in _REFS:
        _REFS[key] = reference_of(make_inputs(c), c["form"])
    return _REFS[key]
