"""Reference of cover_diverse_subset_tokens / cover_diverse_subset_actions (include/cover_hip.h) and the case table of
tests/test_diverse_cpu.py and tests/test_zz_diverse_gpu.py.

Every operation is an explicit np.float32 operation in the order the header states: a pair's distance D is one chain over the steps of
step_weight[t] * e, e one chain over the dims of non-zero scale plus the gripper penalty (never np.sum, which sums pairwise); a row's
value is quality + (weight * mind), two operations, or the quality alone at weight 0 and at pick 0. The greedy loop is the header's:
eligibility from the quality and the self-distance, the lexicographic (value descending with -0 == +0, index ascending) pick among the
unpicked eligible rows with mind > cover_dist, the strict `d < mind` update of every row after every pick. The GPU results are compared
with it as integer bit patterns.

A case is one combination of form ("tokens" / "actions"), shape (G, S, m, h), quality given or None, weight and cover_dist."""
import numpy as np

from tests import augment_ref as AR
from tests import coherence_ref as CR

F32 = np.float32
TOK_VOCAB = AR.TOK_VOCAB
NAN_BITS = np.uint32(0x7FC00000)
INF = F32(np.inf)
THREADS = 1024                    # csrc/diverse.hip: one block per group, thread tid owns rows tid + 1024 q
LDS_BUDGET = 160 * 1024 - 256     # csrc/diverse.hip DIVERSE_LDS_BUDGET: the dynamic LDS bytes of one block


def lds_resident(S, m, h):
    """Whether the launch keeps the group's values in LDS (diverse_launch in csrc/diverse.hip, stated in include/cover_hip.h): the pick's
    row [7 h | 1], the step weights [h], the picked indices [m] and the S rows of 7 h | 1 floats fit LDS_BUDGET bytes."""
    stride = (7 * h) | 1
    return 4 * ((S + 1) * stride + h + m) <= LDS_BUDGET


def boundary_shapes(m=6, h=8):
    """-> the two shapes (1, S, m, h) and (1, S + 1, m, h) on either side of the LDS-resident / global dispatch boundary."""
    S = m
    while lds_resident(S + 1, m, h):
        S += 1
    assert lds_resident(S, m, h) and not lds_resident(S + 1, m, h) and S + 1 <= 4096
    return (1, S, m, h), (1, S + 1, m, h)


# (G, S, m, h): one row; every row of a tiny group; the wave edge (63 / 64 / 65 rows); a second row per thread (1023 / 1025 rows, every row
# picked); four rows per thread; pi0's shape; the widest row (449 floats); either side of the LDS boundary; the global path with a second
# row per thread
SHAPES = [(1, 1, 1, 1), (3, 4, 4, 1), (2, 63, 7, 2), (2, 64, 64, 1), (2, 65, 9, 3), (1, 1023, 5, 1), (1, 1025, 1025, 1), (1, 4096, 256, 1),
          (2, 37, 8, 50), (1, 8, 3, 64), *boundary_shapes(), (1, 1030, 5, 6)]
STRIDED = (2, 20, 6, 3)           # actions read through the strides (chunk * 32, 32, 1) of a [N, chunk, 32] buffer
FLOAT_ONLY = [STRIDED]
QUALITIES = (1, 0)                # quality given / None
WEIGHTS = (0.0, 0.5)
COVERS = (-1.0, 0.0)
DIM_SCALE = (1.0, 1.0, 0.0, 0.5, 0.5, 0.25)   # one zero entry: NaN is planted in that dim of some action rows
DECAY = 0.8
PENALTY = 0.25


def token_row_stride(shape):
    """The row stride, in elements, the token form of a shape is read through: beyond 7 h at every other shape of the table."""
    return 7 * shape[3] + (3 if SHAPES.index(shape) % 2 else 0)


def shapes_of(form):
    return SHAPES + (FLOAT_ONLY if form == "actions" else [])


def cases(forms=("tokens", "actions"), shapes=None):
    return [dict(form=f, shape=s, quality=q, weight=w, cover=c) for f in forms for s in shapes_of(f) if shapes is None or s in shapes
            for q in QUALITIES for w in WEIGHTS for c in COVERS]


def case_id(c):
    return f"{c['form']}-{'x'.join(map(str, c['shape']))}-{'q' if c['quality'] else 'noq'}-w{c['weight']}-c{c['cover']}"


step_weights = CR.step_weights
detokenise = CR.detokenise


def make_inputs(c):
    """-> dict: tokens int64 [G*S, 7h] or actions fp32 [G*S, h, 7] (contiguous; the layout is the caller's to apply), quality fp32 [G*S] or
    None, step_weight fp32 [h], dim_scale, centers fp32 [255], S, m, weight, cover, penalty. The inputs depend on (form, shape) alone, the
    quality included, so the option combinations of a shape see the same rows. About a quarter of the rows of a group are exact copies of
    another row of it (with cover_dist = 0 the count stays below m at the shapes that pick every row). The qualities lie on a grid of
    quarters (ties go by index) with one NaN per group of more than two rows. Actions: some rows carry a NaN in the dim of scale 0
    (invisible) or in dim 6 (invisible), and at groups of more than four rows one row has a NaN in a dim that counts (never picked)."""
    form, (G, S, m, h) = c["form"], c["shape"]
    seed = 1000 * (SHAPES + FLOAT_ONLY).index(c["shape"]) + (5 if form == "actions" else 0) + 91
    rng = np.random.default_rng(seed)
    N = G * S
    centers = AR.openvla_centers()
    mid = rng.integers(40, 215, (G, 1, h, 7))
    b = (mid + rng.integers(-12, 13, (G, S, h, 7)))
    b[..., 6] = np.where(rng.random((G, S, h)) < 0.5, rng.integers(195, 250, (G, S, h)), rng.integers(5, 185, (G, S, h)))   # bins 192.. are >= 0.5
    noise = rng.uniform(-0.003, 0.003, b.shape)
    for g in range(G):
        for i in np.flatnonzero(rng.random(S) < 0.25):
            j = int(rng.integers(0, S))
            b[g, i], noise[g, i] = b[g, j], noise[g, j]
    b = b.reshape(N, h, 7)
    quality = (rng.integers(-6, 7, N) / 4.0).astype(F32)
    if S > 2:
        quality[np.arange(G) * S + rng.integers(0, S, G)] = np.nan
    out = dict(S=S, m=m, weight=c["weight"], cover=c["cover"], penalty=PENALTY, centers=centers, dim_scale=DIM_SCALE,
               step_weight=step_weights(h, DECAY), quality=quality if c["quality"] else None)
    if form == "tokens":
        out["tokens"] = (TOK_VOCAB - 1 - b).astype(np.int64).reshape(N, 7 * h)
        return out
    x = (centers[b].astype(np.float64) + noise.reshape(N, h, 7)).astype(F32)
    nan_dim = DIM_SCALE.index(0.0)
    x[..., nan_dim] = np.where(rng.random((N, h)) < 0.25, F32(np.nan), x[..., nan_dim])
    x[..., 6] = np.where(rng.random((N, h)) < 0.1, F32(np.nan), x[..., 6])
    if S > 4:
        rows = np.arange(G) * S + rng.integers(0, S, G)
        x[rows, rng.integers(0, h, G), 1] = np.nan
    out["actions"] = x
    return out


# ------------------------------------------------------------------------------------------------ the specified arithmetic
def dists(x, y, dim_scale, step_weight, penalty):
    """x fp32 [S, h, >= 7], y fp32 [h, >= 7] (one row) or [S, h, >= 7] (row by row) -> D fp32 [S]."""
    S, h = x.shape[:2]
    y = np.broadcast_to(y, x.shape) if y.ndim == 2 else y
    sc, sw, pen = np.asarray(dim_scale, dtype=F32), np.asarray(step_weight, dtype=F32), F32(penalty)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.zeros((S, h), dtype=F32)                                    # the chains over d of all steps at once: they are independent
        for d in range(6):
            if sc[d] != 0:
                diff = x[:, :, d] - y[:, :, d]
                s = diff * sc[d]
                sq = s * s
                e = e + sq
        if pen != 0:
            differ = (x[:, :, 6] >= F32(0.5)) != (y[:, :, 6] >= F32(0.5))
            e = np.where(differ, e + pen, e)
        D = np.zeros(S, dtype=F32)
        for t in range(h):                                                 # the chain over t, in order
            p = sw[t] * e[:, t]
            D = D + p
    return D


def group_reference(x, m, quality, weight, cover, step_weight, dim_scale, penalty):
    """One group: x fp32 [S, h, >= 7], quality fp32 [S] or None -> (picked int32 [m] (indices in the group, -1 unfilled), count,
    value fp32 [m], dist fp32 [m], assign int32 [S], row_dist fp32 [S])."""
    S = len(x)
    q = np.zeros(S, dtype=F32) if quality is None else np.asarray(quality, dtype=F32)
    weight, cover = F32(weight), F32(cover)
    picked = np.full(m, -1, dtype=np.int32)
    value = np.full(m, NAN_BITS, dtype=np.uint32).view(F32)
    dist = np.full(m, INF, dtype=F32)
    mind, assign = np.full(S, INF, dtype=F32), np.full(S, -1, dtype=np.int32)
    if not CR.scale_usable(dim_scale):
        return picked, 0, value, dist, assign, mind
    eligible = ~np.isnan(q) & ~np.isnan(dists(x, x, dim_scale, step_weight, penalty))
    taken = np.zeros(S, dtype=bool)
    count = 0
    for k in range(m):
        with np.errstate(invalid="ignore", over="ignore"):
            if k > 0 and weight != 0:
                prod = weight * mind
                v = q + prod
            else:
                v = q
            cand = eligible & ~taken & (mind > cover) & ~np.isnan(v)
        if not cand.any():
            break
        best = np.max(v[cand])
        p = int(np.argmax(cand & (v == best)))                             # the lowest index among the largest; -0 == +0
        picked[k], value[k], dist[k] = p, v[p], mind[p]
        taken[p] = True
        d = dists(x, x[p], dim_scale, step_weight, penalty)
        with np.errstate(invalid="ignore"):
            closer = d < mind                                              # strict; a NaN d never enters
        mind = np.where(closer, d, mind)
        assign = np.where(closer, np.int32(k), assign).astype(np.int32)
        count = k + 1
    return picked, count, value, dist, assign, mind


def reference(x, S, m, quality, weight, cover, step_weight, dim_scale, penalty=0.0):
    """x fp32 [G*S, h, >= 7] -> dict(picked int32 [G, m] (global rows g * S + j, -1 unfilled), count int32 [G], value fp32 [G, m],
    dist fp32 [G, m], assign int32 [G*S], row_dist fp32 [G*S])."""
    x = np.asarray(x, dtype=F32)
    N = len(x)
    G = N // S
    out = dict(picked=np.empty((G, m), np.int32), count=np.empty(G, np.int32), value=np.empty((G, m), F32), dist=np.empty((G, m), F32),
               assign=np.empty(N, np.int32), row_dist=np.empty(N, F32))
    for g in range(G):
        sl = slice(g * S, (g + 1) * S)
        p, n, v, d, a, r = group_reference(x[sl], m, None if quality is None else quality[sl], weight, cover, step_weight, dim_scale, penalty)
        out["picked"][g] = np.where(p >= 0, p + g * S, -1)
        out["count"][g], out["value"][g], out["dist"][g], out["assign"][sl], out["row_dist"][sl] = n, v, d, a, r
    return out


def gathered(rows, picked, S):
    """The `out` of the launch: rows [G*S, ...] (tokens [N, 7h] or actions [N, h, 7]) gathered through picked [G, m]; an unfilled slot
    repeats the group's slot 0, a group with no pick its row 0."""
    G, m = picked.shape
    src = np.where(picked >= 0, picked, np.where(picked[:, :1] >= 0, picked[:, :1], np.arange(G)[:, None] * S))
    return rows[src.reshape(-1)]


def values_of(inp, form, h):
    return detokenise(inp["tokens"], inp["centers"], h) if form == "tokens" else inp["actions"]


def reference_of(inp, form, h):
    return reference(values_of(inp, form, h), inp["S"], inp["m"], inp["quality"], inp["weight"], inp["cover"], inp["step_weight"],
                     inp["dim_scale"], inp["penalty"])


_REFS = {}


def case_reference(c):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    key = case_id(c)
    if key not in _REFS:
        _REFS[key] = reference_of(make_inputs(c), c["form"], c["shape"][3])
    return _REFS[key]
