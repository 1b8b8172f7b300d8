"""Reference of cover_coherence_prior_tokens / cover_coherence_prior_actions (include/cover_hip.h) and the case table of
tests/test_coherence_{cpu,gpu}.py.

Every operation is an explicit np.float32 operation in the order the header states: a pair's distance D is one chain over the overlapping
steps of step_weight[t] * e, e one chain over the dims of non-zero scale plus the gripper penalty; a row's sum is 64 lane-strided chains
over the references of non-zero weight (arrays [rows, 64]) that meet in the xor butterfly p = p + p[:, idx ^ o]. Never np.sum, which sums
pairwise. The prior is the sum with its sign bit flipped, a NaN sum the one NaN 0x7FC00000. The GPU results are compared with it as
integer bit patterns.

A case is one combination of form ("tokens" / "actions"), shape (G, S, R, h, hr, shift), shared or per-group references and
gripper_penalty."""
import numpy as np

from tests import augment_ref as AR

F32 = np.float32
TOK_VOCAB = AR.TOK_VOCAB
LANES = 64
_IDX = np.arange(LANES)
NAN_BITS = np.uint32(0x7FC00000)
LARGEST_TILE = 1024               # csrc/coherence.hip: the references of one LDS tile at the narrowest row (an overlap of one step)

# (G, S, R, h, hr, shift): one row and one reference; a shift inside a longer reference; the lane-stride edges of R (63 / 64 / 65); an
# overlap of one step out of eight; three LDS tiles at the widest row (449 floats); one reference more than the largest tile
SHAPES = [(1, 1, 1, 1, 1, 0), (3, 17, 1, 4, 6, 2), (2, 33, 63, 3, 3, 0), (2, 16, 64, 8, 8, 0), (1, 15, 65, 8, 9, 8),
          (2, 5, 130, 64, 64, 0), (1, 3, LARGEST_TILE + 1, 1, 1, 0)]
STRIDED = (2, 20, 5, 3, 5, 1)     # actions read through the strides (chunk * 32, 32, 1) of a [N, chunk, 32] buffer
FLOAT_ONLY = [STRIDED]
GROUPINGS = (0, 1)                # 0: one reference set shared by all groups; 1: a set per group
PENALTIES = (0.0, 0.25)
DIM_SCALE = (1.0, 1.0, 0.0, 0.5, 0.5, 0.25)   # one zero entry: NaN is planted in that dim of some references and (actions) candidates
DECAY = 0.8


def token_row_stride(shape):
    """The row stride, in elements, the token form of a shape is read through: beyond 7 h at every other shape of the table."""
    return 7 * shape[3] + (3 if SHAPES.index(shape) % 2 else 0)


def shapes_of(form):
    return SHAPES + (FLOAT_ONLY if form == "actions" else [])


def cases(forms=("tokens", "actions"), shapes=None):
    return [dict(form=f, shape=s, per_group=p, penalty=k) for f in forms for s in shapes_of(f) if shapes is None or s in shapes
            for p in GROUPINGS for k in PENALTIES]


def case_id(c):
    return f"{c['form']}-{'x'.join(map(str, c['shape']))}-{'pergroup' if c['per_group'] else 'shared'}-pen{c['penalty']}"


def overlap(h, hr, shift):
    return min(h, hr - shift)


def step_weights(h, decay=DECAY):
    """host.coherence_step_weights' formula: float32(decay ** t) computed in float64."""
    return (np.float64(decay) ** np.arange(h, dtype=np.float64)).astype(F32)


def make_inputs(c):
    """-> dict: tokens int64 [G*S, 7h] or actions fp32 [G*S, h, 7] (contiguous; the layout is the caller's to apply), ref fp32 [R, hr, 7]
    or [G, R, hr, 7], weight fp32 [R] or [G, R] (signed, about a fifth exact zeros), step_weight fp32 [h], dim_scale, centers fp32 [255],
    S, shift, penalty. Row 0 of every group equals reference 0 over the overlap (of group 0 when the set is shared), and the last
    reference is a copy of reference 0, both with weight != 0: a tie for `nearest` at D = 0. The reference steps outside the overlap and
    (actions) the candidate steps beyond it are NaN: they are never read. Some references carry a NaN in the dim of scale 0."""
    form, (G, S, R, h, hr, shift) = c["form"], c["shape"]
    T = overlap(h, hr, shift)
    seed = 1000 * (SHAPES + FLOAT_ONLY).index(c["shape"]) + (5 if form == "actions" else 0) + 47
    rng = np.random.default_rng(seed)
    N = G * S
    centers = AR.openvla_centers()
    mid = rng.integers(40, 215, (G, 1, h, 7))
    b = (mid + rng.integers(-12, 13, (G, S, h, 7))).reshape(N, h, 7)
    b[..., 6] = np.where(rng.random((N, h)) < 0.5, rng.integers(195, 250, (N, h)), rng.integers(5, 185, (N, h)))   # bins 192.. are >= 0.5
    if form == "tokens":
        x = centers[b]
    else:
        x = (centers[b].astype(np.float64) + rng.uniform(-0.003, 0.003, b.shape)).astype(F32)
    Gr = G if c["per_group"] else 1
    rb = np.clip(np.broadcast_to(mid[:Gr, :, :1], (Gr, R, 1, 7)) + rng.integers(-12, 13, (Gr, R, hr, 7)), 0, 254)
    rb[..., 6] = np.where(rng.random((Gr, R, hr)) < 0.5, rng.integers(195, 250, (Gr, R, hr)), rng.integers(5, 185, (Gr, R, hr)))
    ref = (centers[rb].astype(np.float64) + rng.uniform(-0.003, 0.003, rb.shape)).astype(F32)
    for g in range(Gr):
        ref[g, 0, shift:shift + T] = x[g * S, :T]
    ref[:, R - 1] = ref[:, 0]
    nan_dim = DIM_SCALE.index(0.0)
    ref[..., nan_dim] = np.where(rng.random((Gr, R, hr)) < 0.25, F32(np.nan), ref[..., nan_dim])
    ref[:, :, :shift] = np.nan
    ref[:, :, shift + T:] = np.nan
    w = np.clip(rng.normal(size=(Gr, R)), -3, 3).astype(F32)
    w[np.abs(w) < 0.05] = F32(0.05)
    zero = rng.random((Gr, R)) < 0.2
    zero[:, 0] = zero[:, R - 1] = False
    w[zero] = 0
    out = dict(S=S, shift=shift, penalty=c["penalty"], centers=centers, dim_scale=DIM_SCALE, step_weight=step_weights(h),
               ref=ref if c["per_group"] else ref[0], weight=w if c["per_group"] else w[0])
    if form == "tokens":
        out["tokens"] = (TOK_VOCAB - 1 - b).astype(np.int64).reshape(N, 7 * h)
        return out
    x = x.copy()
    x[..., nan_dim] = np.where(rng.random((N, h)) < 0.25, F32(np.nan), x[..., nan_dim])
    x[:, T:] = np.nan
    out["actions"] = x
    return out


# ------------------------------------------------------------------------------------------------ the specified arithmetic
def detokenise(tokens, centers, steps, tok_vocab=TOK_VOCAB):
    """int64 [N, >= 7 steps] -> fp32 [N, steps, 7]: centers[clamp(tok_vocab - token - 1)]."""
    t = np.asarray(tokens)[:, :7 * steps].astype(np.int64)
    return np.asarray(centers, dtype=F32)[np.clip(tok_vocab - t - 1, 0, len(centers) - 1)].reshape(len(t), steps, 7)


def scale_usable(dim_scale):
    sc = np.asarray(dim_scale, dtype=F32)
    return bool(np.isfinite(sc).all() and (sc >= 0).all())


def pair_dists(x, y, dim_scale, step_weight, penalty):
    """x fp32 [S, T, >= 7] (candidates), y fp32 [R, T, 7] (references, already shifted) -> D fp32 [S, R]."""
    S, T = x.shape[:2]
    sc, sw, pen = np.asarray(dim_scale, dtype=F32), np.asarray(step_weight, dtype=F32), F32(penalty)
    D = np.zeros((S, len(y)), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            e = np.zeros_like(D)
            for d in range(6):
                if sc[d] != 0:
                    diff = x[:, None, t, d] - y[None, :, t, d]
                    s = diff * sc[d]
                    sq = s * s
                    e = e + sq
            if pen != 0:
                differ = (x[:, None, t, 6] >= F32(0.5)) != (y[None, :, t, 6] >= F32(0.5))
                e = np.where(differ, e + pen, e)
            p = sw[t] * e
            D = D + p
    return D


def butterfly(p):
    """p fp32 [rows, 64] -> [rows]: v = v + v[lane ^ o], o = 32 .. 1."""
    o = LANES // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while o:
            p = p + p[:, _IDX ^ o]
            o //= 2
    return p[:, 0]


def row_results(D, w):
    """D fp32 [S, R], w fp32 [R] -> (prior fp32 [S], min_dist fp32 [S], nearest int32 [S])."""
    S, R = D.shape
    acc = np.zeros((S, LANES), dtype=F32)
    nz = w != 0                                                            # a NaN weight is not zero
    with np.errstate(invalid="ignore", over="ignore"):
        for r0 in range(0, R, LANES):
            k = min(LANES, R - r0)
            use = np.broadcast_to(nz[None, r0:r0 + k], (S, k))
            prod = w[None, r0:r0 + k] * np.where(use, D[:, r0:r0 + k], F32(0))
            acc[:, :k] = np.where(use, acc[:, :k] + prod, acc[:, :k])
        total = butterfly(acc)
    bits = total.view(np.uint32) ^ np.uint32(0x80000000)                   # -acc: 0.0 becomes 0x80000000
    prior = np.where(np.isnan(total), NAN_BITS, bits).astype(np.uint32).view(F32)
    ok = nz[None, :] & ~np.isnan(D)                                        # the lexicographic (D, r) minimum over these
    Dm = np.where(ok, D, F32(np.inf))
    m = Dm.min(axis=1)
    nearest = np.where(ok.any(axis=1), np.argmax(ok & (Dm == m[:, None]), axis=1), -1).astype(np.int32)
    return prior, m.astype(F32), nearest


def reference(x, ref, weight, S, shift, step_weight, dim_scale, penalty=0.0):
    """x fp32 [G*S, h, >= 7], ref fp32 [R, hr, 7] or [G, R, hr, 7], weight fp32 [R] or [G, R] -> dict(prior fp32 [N], min_dist fp32 [N],
    nearest int32 [N])."""
    x, ref, weight = np.asarray(x, dtype=F32), np.asarray(ref, dtype=F32), np.asarray(weight, dtype=F32)
    N, h = x.shape[:2]
    G, hr = N // S, ref.shape[-2]
    T = overlap(h, hr, shift)
    out = dict(prior=np.empty(N, dtype=F32), min_dist=np.empty(N, dtype=F32), nearest=np.empty(N, dtype=np.int32))
    if not scale_usable(dim_scale):                                        # the kernel's rule for a scale the wrapper would have refused
        out["prior"].view(np.uint32)[:] = NAN_BITS
        out["min_dist"][:], out["nearest"][:] = np.inf, -1
        return out
    for g in range(G):
        sl = slice(g * S, (g + 1) * S)
        y = (ref[g] if ref.ndim == 4 else ref)[:, shift:shift + T]
        D = pair_dists(x[sl, :T], y, dim_scale, step_weight, penalty)
        out["prior"][sl], out["min_dist"][sl], out["nearest"][sl] = row_results(D, weight[g] if weight.ndim == 2 else weight)
    return out


def reference_f64(x, ref, weight, S, shift, step_weight, dim_scale, penalty=0.0):
    """The same formula in float64 with ordinary sums (no NaN handling beyond the dims of scale 0 and the unread steps) -> prior float64 [N]."""
    x, ref, w = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    sc, sw = np.asarray(dim_scale, dtype=np.float64), np.asarray(step_weight, dtype=np.float64)
    N, h = x.shape[:2]
    T = overlap(h, ref.shape[-2], shift)
    out = np.empty(N)
    for g in range(N // S):
        sl = slice(g * S, (g + 1) * S)
        y = (ref[g] if ref.ndim == 4 else ref)[:, shift:shift + T]
        xs, ys = np.where(sc != 0, x[sl, :T, :6], 0.0), np.where(sc != 0, y[..., :6], 0.0)
        e = (((xs[:, None] - ys[None]) * sc) ** 2).sum(axis=3)
        e = e + float(penalty) * ((x[sl, None, :T, 6] >= 0.5) != (y[None, :, :, 6] >= 0.5))
        D = (e * sw[:T]).sum(axis=2)
        wg = w[g] if w.ndim == 2 else w
        out[sl] = -(np.where(wg != 0, D, 0.0) * wg).sum(axis=1)
    return out


def values_of(inp, form, h):
    return detokenise(inp["tokens"], inp["centers"], h) if form == "tokens" else inp["actions"]


def reference_of(inp, form, h):
    return reference(values_of(inp, form, h), inp["ref"], inp["weight"], inp["S"], inp["shift"], inp["step_weight"], inp["dim_scale"],
                     inp["penalty"])


_REFS = {}


def case_reference(c):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    key = case_id(c)
    if key not in _REFS:
        _REFS[key] = reference_of(make_inputs(c), c["form"], c["shape"][3])
    return _REFS[key]
