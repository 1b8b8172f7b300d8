"""Reference of cover_smooth_scores_tokens / cover_smooth_scores_actions (include/cover_hip.h) and the case table of
tests/test_smooth_{cpu,gpu}.py.

Every operation is an explicit np.float32 operation in the order the header states: the squared distance is one chain over (step, dim),
the row sums are 64 lane-strided chains per row (arrays [rows, 64]) that meet in the xor butterfly p = p + p[:, idx ^ o], the group mean
is the same over the finite scores. Never np.sum, which sums pairwise. The GPU results are compared with it as integer bit patterns.

A case is one combination of form ("tokens" / "actions"), shape (G, S, h), layout, shrink and split_gripper."""
import numpy as np

from tests import augment_ref as AR

F32 = np.float32
TOK_VOCAB = AR.TOK_VOCAB
LANES = 64
_IDX = np.arange(LANES)

# (G, S, h): the lane-stride edges (63 / 64 / 65), a ragged last stride, row tiles of 16 that do not divide S, more than one j-tile (1025)
SHAPES = [(1, 1, 1), (3, 17, 1), (2, 63, 2), (2, 64, 1), (2, 65, 1), (1, 130, 3), (1, 1025, 1)]
STRIDED = (2, 40, 3)              # actions read through the strides (chunk * 32, 32, 1) of a [N, chunk, 32] buffer
LARGE = (1, 4096, 1)              # the row limit: 256 blocks of one group, four j-tiles
HISTORY = (2, 40, 10)             # the padded history layout [N, 10, 7]: pad rows, shared past rows, the candidate's own steps
ZERO_DIM = (2, 33, 2)             # dim_scale has a zero, and NaN is planted in that dim: it must be invisible
WIDE = (1, 65, 64)                # the step limit: one j-tile is 64 rows of 449 floats
FLOAT_ONLY = [STRIDED, LARGE, HISTORY, ZERO_DIM, WIDE]
TOKEN_EXTRA = [LARGE]
SHRINKS = (0.0, 0.5)
SPLITS = (0, 1)
DIM_SCALE = (1.0, 1.0, 0.75, 0.5, 0.5, 0.25)
ZERO_SCALE = (1.0, 0.0, 0.75, 0.5, 0.0, 0.25)


def token_row_stride(shape):
    """The row stride, in elements, the token form of a shape is read through: beyond 7 h at every other shape of the table."""
    return 7 * shape[2] + (3 if SHAPES.index(shape) % 2 else 0) if shape in SHAPES else 7 * shape[2]


def shapes_of(form):
    return SHAPES + (FLOAT_ONLY if form == "actions" else TOKEN_EXTRA)


def cases(forms=("tokens", "actions"), shapes=None):
    return [dict(form=f, shape=s, shrink=k, split=p) for f in forms for s in shapes_of(f) if shapes is None or s in shapes
            for k in SHRINKS for p in SPLITS]


def case_id(c):
    return f"{c['form']}-{'x'.join(map(str, c['shape']))}-shrink{c['shrink']}-split{c['split']}"


def case_radius(shape):
    """Sized to the jitter inside a cluster (below), so that a row's neighbourhood is a part of its cluster: some cluster mates in, some
    out. The history layout's own steps are the last four."""
    steps = 4 if shape == HISTORY else shape[2]
    return 0.039 * float(np.sqrt(steps))


def make_inputs(c):
    """-> dict: tokens int64 [G*S, 7h] or actions fp32 [G*S, h, 7] (contiguous; the layout is the caller's to apply), scores fp32 [G*S],
    centers fp32 [255], dim_scale (6 floats), radius, shrink, split, S. Rows are cluster centres plus a jitter of a few bins; the scores
    are a cluster effect plus noise around 0.3, all finite and positive (a mean of them does not cancel)."""
    form, (G, S, h) = c["form"], c["shape"]
    seed = 1000 * (SHAPES + FLOAT_ONLY).index(c["shape"]) + (5 if form == "actions" else 0) + 31
    rng = np.random.default_rng(seed)
    N = G * S
    centers = AR.openvla_centers()
    n_cl = max(1, S // 8)
    cl = rng.integers(0, n_cl, N)
    cl_of_group = cl + n_cl * (np.arange(N) // S)
    mid = rng.integers(30, 225, (G * n_cl, h, 7))
    b = mid[cl_of_group] + rng.integers(-3, 4, (N, h, 7))
    cls = rng.integers(0, 2, (G * n_cl, h))[cl_of_group]                 # the gripper class goes with the cluster ...
    flip = np.zeros((N, h), dtype=bool)                                  # ... but for one step of a seventh of the rows
    flip[np.arange(N), rng.integers(0, h, N)] = rng.random(N) < 0.15
    cls = np.where(flip, 1 - cls, cls)
    b[..., 6] = np.where(cls == 1, rng.integers(195, 250, (N, h)), rng.integers(5, 185, (N, h)))   # bins 192.. are >= 0.5
    scores = (0.3 + np.clip(rng.normal(size=G * n_cl), -3, 3)[cl_of_group] * 0.05 + np.clip(rng.normal(size=N), -3, 3) * 0.01).astype(F32)
    out = dict(S=S, scores=scores, centers=centers, dim_scale=ZERO_SCALE if c["shape"] == ZERO_DIM else DIM_SCALE,
               radius=case_radius(c["shape"]), shrink=c["shrink"], split=c["split"])
    if form == "tokens":
        out["tokens"] = (TOK_VOCAB - 1 - b).astype(np.int64).reshape(N, 7 * h)
        return out
    x = (centers[b].astype(np.float64) + rng.uniform(-0.003, 0.003, b.shape)).astype(F32)
    if c["shape"] == HISTORY:                                            # steps 0..2 pads, 3..5 the group's past, 6..9 the candidate's own
        x[:, :3] = F32(-5.0)
        x[:, 3:6] = x.reshape(G, S, h, 7)[:, :1, 3:6].repeat(S, axis=1).reshape(N, 3, 7)
    if c["shape"] == ZERO_DIM:
        x[rng.integers(0, N, N // 3), rng.integers(0, h, N // 3), 1] = np.nan
        x[rng.integers(0, N, N // 3), rng.integers(0, h, N // 3), 4] = np.nan
    out["actions"] = x
    return out


# ------------------------------------------------------------------------------------------------ the specified arithmetic
def detokenise(tokens, centers, steps, tok_vocab=TOK_VOCAB):
    """int64 [N, >= 7 steps] -> fp32 [N, steps, 7]: centers[clamp(tok_vocab - token - 1)]."""
    t = np.asarray(tokens)[:, :7 * steps].astype(np.int64)
    return np.asarray(centers, dtype=F32)[np.clip(tok_vocab - t - 1, 0, len(centers) - 1)].reshape(len(t), steps, 7)


def is_finite(s):
    return (np.asarray(s, dtype=F32).view(np.uint32) & np.uint32(0x7F800000)) != np.uint32(0x7F800000)


def pair_weights(x, dim_scale, radius2, split):
    """x fp32 [S, h, >= 7] of ONE group -> fp32 [S, S], w[n, j]; the diagonal is 1 by definition."""
    S, h = x.shape[:2]
    sc = np.asarray(dim_scale, dtype=F32)
    d2 = np.zeros((S, S), dtype=F32)
    same = np.ones((S, S), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(h):
            if split:
                cls = x[:, t, 6] >= F32(0.5)
                same &= cls[:, None] == cls[None, :]
            for d in range(6):
                if sc[d] != 0:
                    diff = x[:, None, t, d] - x[None, :, t, d]
                    s = diff * sc[d]
                    sq = s * s
                    d2 = d2 + sq
        w = np.where(d2 < radius2, F32(1.0) - d2 / radius2, F32(0.0)).astype(F32)
    w[~same] = 0
    if not all(v >= 0 and np.isfinite(v) for v in sc):                 # the kernel's rule for a scale the wrapper would have refused
        w[:] = 0
    w[np.arange(S), np.arange(S)] = 1
    return w


def butterfly(p):
    """p fp32 (or int) [rows, 64] -> [rows]: v = v + v[lane ^ o], o = 32 .. 1."""
    o = LANES // 2
    while o:
        p = p + p[:, _IDX ^ o]
        o //= 2
    return p[:, 0]


def lane_chains(w, scores):
    """w fp32 [R, S], scores fp32 [S] -> (num, den, dsum fp32 [R], cnt int32 [R])."""
    R, S = w.shape
    fin = is_finite(scores)
    num, den, dsum = (np.zeros((R, LANES), dtype=F32) for _ in range(3))
    cnt = np.zeros((R, LANES), dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, S, LANES):
            k = min(LANES, S - j0)
            wj, sj = w[:, j0:j0 + k], scores[None, j0:j0 + k]
            pos = wj > 0
            ev = pos & fin[None, j0:j0 + k]
            dsum[:, :k] = np.where(pos, dsum[:, :k] + wj, dsum[:, :k])
            cnt[:, :k] += pos
            den[:, :k] = np.where(ev, den[:, :k] + wj, den[:, :k])
            prod = np.where(ev, wj * np.where(ev, sj, F32(0)), F32(0)).astype(F32)
            num[:, :k] = np.where(ev, num[:, :k] + prod, num[:, :k])
        return butterfly(num), butterfly(den), butterfly(dsum), butterfly(cnt)


def group_mean(scores):
    """fp32 [S] -> (m0, count): the lane-strided chain over the finite scores, the butterfly, one divide; 0.0 with no finite score."""
    s = np.asarray(scores, dtype=F32)
    fin = is_finite(s)
    acc, cnt = np.zeros((1, LANES), dtype=F32), 0
    for j0 in range(0, len(s), LANES):
        k = min(LANES, len(s) - j0)
        f = fin[j0:j0 + k]
        acc[0, :k] = np.where(f, acc[0, :k] + np.where(f, s[j0:j0 + k], F32(0)), acc[0, :k])
        cnt += int(f.sum())
    total = butterfly(acc)[0]
    return (total / F32(cnt) if cnt else F32(0.0)), cnt


def row_sums(x, scores, S, dim_scale, radius, split=1):
    """What does not depend on shrink: x fp32 [G*S, h, >= 7], scores fp32 [G*S] -> dict(num, den, dsum fp32 [N], cnt int32 [N], m0 fp32 [G])."""
    x, scores = np.asarray(x, dtype=F32), np.asarray(scores, dtype=F32)
    N = len(scores)
    G = N // S
    r = F32(radius)
    radius2 = r * r                                                        # squared once, in fp32
    out = dict(num=np.empty(N, dtype=F32), den=np.empty(N, dtype=F32), dsum=np.empty(N, dtype=F32), cnt=np.empty(N, dtype=np.int32),
               m0=np.empty(G, dtype=F32))
    for g in range(G):
        sl = slice(g * S, (g + 1) * S)
        w = pair_weights(x[sl], dim_scale, radius2, split)
        out["num"][sl], out["den"][sl], out["dsum"][sl], out["cnt"][sl] = lane_chains(w, scores[sl])
        out["m0"][g] = group_mean(scores[sl])[0]
    return out


def finish(sums, scores, S, shrink):
    """row_sums' dict -> dict(smoothed fp32 [N], density fp32 [N], neighbours int32 [N], group_mean fp32 [G])."""
    scores, shrink = np.asarray(scores, dtype=F32), F32(shrink)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if shrink == 0:
            sm = sums["num"] / sums["den"]
        else:
            tm = shrink * np.repeat(sums["m0"], S)
            nn = sums["num"] + tm
            dd = sums["den"] + shrink
            sm = nn / dd
    smoothed = np.where(is_finite(scores), sm.astype(F32).view(np.uint32), scores.view(np.uint32)).view(F32)
    return dict(smoothed=smoothed, density=sums["dsum"] / F32(S), neighbours=sums["cnt"], group_mean=sums["m0"])


def reference(x, scores, S, dim_scale, radius, shrink=0.0, split=1):
    """x fp32 [G*S, h, >= 7], scores fp32 [G*S] -> dict(smoothed fp32 [N], density fp32 [N], neighbours int32 [N], group_mean fp32 [G])."""
    return finish(row_sums(x, scores, S, dim_scale, radius, split), scores, S, shrink)


def reference_f64(x, scores, S, dim_scale, radius, shrink=0.0, split=1):
    """The same formula in float64 with ordinary sums (finite scores only) -> smoothed float64 [N]."""
    x, s64 = np.asarray(x, dtype=np.float64), np.asarray(scores, dtype=np.float64)
    sc = np.asarray(dim_scale, dtype=np.float64)
    r2 = float(F32(radius)) ** 2
    out = np.empty(len(s64))
    for g in range(len(s64) // S):
        sl = slice(g * S, (g + 1) * S)
        xs = np.where(sc != 0, x[sl, :, :6], 0.0)                          # a dim of scale 0 is not read
        diff = (xs[:, None] - xs[None]) * sc
        d2 = (diff * diff).sum(axis=(2, 3))
        w = np.where(d2 < r2, 1.0 - d2 / r2, 0.0)
        if split:
            cls = x[sl, :, 6] >= 0.5
            w[(cls[:, None] != cls[None]).any(axis=2)] = 0.0
        np.fill_diagonal(w, 1.0)
        out[sl] = (w @ s64[sl] + shrink * s64[sl].mean()) / (w.sum(axis=1) + shrink)
    return out


def values_of(inp, form, h):
    return detokenise(inp["tokens"], inp["centers"], h) if form == "tokens" else inp["actions"]


def reference_of(inp, form, h):
    return reference(values_of(inp, form, h), inp["scores"], inp["S"], inp["dim_scale"], inp["radius"], inp["shrink"], inp["split"])


_REFS, _SUMS = {}, {}


def case_reference(c):
    """Computed once per case and shared by the tests (the row sums once per form, shape and split): treat the arrays as read-only."""
    key = case_id(c)
    if key not in _REFS:
        inp = make_inputs(c)
        sk = (c["form"], c["shape"], c["split"])
        if sk not in _SUMS:
            _SUMS[sk] = row_sums(values_of(inp, c["form"], c["shape"][2]), inp["scores"], inp["S"], inp["dim_scale"], inp["radius"], c["split"])
        _REFS[key] = finish(_SUMS[sk], inp["scores"], inp["S"], c["shrink"])
    return _REFS[key]
# ------------------------------------------------------------------------------------------------ the constructed decision
def constructed_decision():
    """One group of S = 12, h = 1: rows 0..7 a tight cluster with steady scores, row 8 isolated with the highest raw score, rows 9..11
    isolated with low scores that pull the group mean down. -> dict(actions fp32 [12, 1, 7], scores fp32 [12], S, dim_scale, radius,
    shrink, split). The raw arg-max is row 8; smoothing with shrink = 1 halves the lone row's lead towards the low group mean while a
    cluster row keeps its local mean nearly whole (its eight-fold evidence outweighs the shrink)."""
    x = np.zeros((12, 1, 7), dtype=F32)
    x[:8, 0, :6] = np.array([0.10, -0.20, 0.05, 0.0, 0.30, -0.10], dtype=F32) + (np.arange(8, dtype=F32)[:, None] - F32(3.5)) * F32(0.002)
    x[8, 0, :6] = F32(0.8)
    x[9, 0, :6], x[10, 0, :6], x[11, 0, :6] = F32(-0.8), F32(-0.4), F32(0.5)
    scores = np.array([0.100, 0.102, 0.098, 0.101, 0.099, 0.103, 0.097, 0.100, 0.120, -0.20, -0.25, -0.30], dtype=F32)
    return dict(actions=x, scores=scores, S=12, dim_scale=(1.0,) * 6, radius=0.1, shrink=1.0, split=1)
