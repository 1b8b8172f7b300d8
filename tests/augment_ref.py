"""Reference of cover_augment_tokens / cover_augment_actions (include/cover_hip.h) and the case table of tests/test_augment_{cpu,gpu}.py.

The kernels' arithmetic is specified rounding by rounding, so the reference restates it in numpy fp32: the sums over the samples are
explicit Python loops over j (one np.float32 add per sample, vectorised over groups, steps and dims only) -- never np.mean / np.std /
np.sum, which are pairwise -- and every other operation is one np.float32 operation. The GPU results are compared with it as integer
bit patterns.

A case is one combination of form ("tokens" / "actions"), shape (G, n, K, h), memory layout and input variant."""
import numpy as np

F32 = np.float32
TOK_VOCAB = 32000
N_CENTERS = 255

# (G, n, K, h): groups (prompts), policy samples per group, augmented rows per group, steps
SHAPES = [(1, 1, 1, 1), (1, 2, 3, 1), (2, 5, 32, 1), (3, 4, 65, 2), (8, 4, 60, 4), (2, 5, 123, 8)]
FLOAT_ONLY = [(8, 5, 59, 4),      # read through the strides (chunk * 32, 32) of a [N, chunk, 32] buffer
              (1, 3, 7, 50)]      # 350 statistics items: more than one pass of the 256-thread block
STRIDED = (8, 5, 59, 4)
VARIANTS = ("spread", "equal", "floor", "clip", "tie0", "tie1", "midway", "sigma0", "k0", "outside")


def openvla_centers():
    """The de-tokeniser's table (OpenVLA.tokens_to_actions, float64) cast to fp32."""
    bins = np.linspace(-1, 1, N_CENTERS + 1)
    return ((bins[:-1] + bins[1:]) / 2.0).astype(F32)


def dyadic_centers():
    """255 centres (b - 127) / 128: every centre, every sum of up to 8 of them and every midpoint between neighbours is exact in fp32."""
    return ((np.arange(N_CENTERS) - 127) / 128.0).astype(F32)


def feasible(form, shape, variant):
    G, n, K, h = shape
    if variant in ("tie0", "tie1"):
        return n % 2 == 0                       # a tie needs an even number of voters
    if variant == "floor":
        return n >= 2                           # one sample has sd 0 everywhere: the floor would be active on all dims
    if variant in ("midway", "outside"):
        return form == "tokens"                 # both are about the centre table
    return True


def cases(forms=("tokens", "actions"), shapes=None, variants=VARIANTS):
    out = []
    for form in forms:
        for s in (shapes if shapes is not None else SHAPES + (FLOAT_ONLY if form == "actions" else [])):
            if form == "tokens" and s in FLOAT_ONLY:
                continue
            out += [dict(form=form, shape=s, variant=v) for v in variants if feasible(form, s, v)]
    return out


def case_id(c):
    return f"{c['form']}-{'x'.join(map(str, c['shape']))}-{c['variant']}"


def _all_shapes():
    return SHAPES + FLOAT_ONLY


def make_inputs(c):
    """-> dict: bins int64 [G*n, h, 7] (the centre index of every sample value; the value itself for the float form is centers[bins] plus
    a sub-bin offset), tokens int64 [G*n, 7h] or actions fp32 [G*n, h, 7] (contiguous; the layout is the caller's to apply), normals fp32
    [G, K, h, 6], centers fp32 [255], sigma, sd_floor, clip, and n / K as the case runs them (K = 0 for the k0 variant)."""
    form, (G, n, K, h), variant = c["form"], c["shape"], c["variant"]
    seed = 100 * _all_shapes().index(c["shape"]) + VARIANTS.index(variant) + (50 if form == "actions" else 0) + 5
    rng = np.random.default_rng(seed)
    N = G * n
    # exact sums for the two variants that need them: n equal values then average to exactly that value, so d = 0 and sd = 0
    centers = dyadic_centers() if variant in ("midway", "equal") else openvla_centers()
    sigma, sd_floor, clip = 1.0, 0.0, (-1.0, 1.0)
    b = rng.integers(20, 235, (G, n, h, 7))                        # spread samples
    cls = rng.integers(0, 2, (G, n, h))                            # gripper class: bins 192.. are >= 0.5 in both tables
    b[..., 6] = np.where(cls == 1, rng.integers(195, 250, (G, n, h)), rng.integers(5, 185, (G, n, h)))
    if K > 0:
        z = rng.standard_normal((G, K, h, 6)).astype(F32)
    else:
        z = np.zeros((G, 0, h, 6), dtype=F32)
    if variant == "spread" and K > 0:
        z[0, 0, 0, 0] = np.nan                                     # lands on clip lo
    if variant == "equal":
        b[:] = b[:, :1]                                            # every sample of a group is sample 0
    if variant == "floor":
        b[..., :3] = b[:, :1, :, :3]                               # dims 0-2: sd 0, below the floor
        b[:, 0, :, 3:6], b[:, 1, :, 3:6] = 30, 220                 # dims 3-5: two samples 190 bins apart, sd far above it
        sd_floor = 0.02
    if variant == "clip":
        clip = (-0.3, 0.3)
        b[0, :, 0, 0] = 240                                        # mean 0.886, sd 0: clipped
        b[0, :, 0, 1] = 127                                        # mean 0, sd 0: not clipped
    if variant in ("tie0", "tie1"):
        first = 0 if variant == "tie0" else 1
        cls = np.broadcast_to((np.arange(n) < n // 2)[None, :, None], (G, n, h)) ^ (first == 0)   # sample 0's class = `first`
        b[..., 6] = np.where(cls, rng.integers(195, 250, (G, n, h)), rng.integers(5, 185, (G, n, h)))
    if variant == "midway":
        b[..., :6] = rng.integers(1, 254, (G, 1, h, 6))            # all samples equal: mean = the centre exactly, sd 0
        sd_floor = 1.0 / 256.0                                     # half the centre spacing
        z = np.where(np.arange(K)[None, :, None, None] % 2 == 0, 1.0, -1.0).astype(F32) * np.ones((G, K, h, 6), dtype=F32)
    if variant == "sigma0":
        sigma = 0.0
    if variant == "k0":
        K = 0
        z = np.zeros((G, 0, h, 6), dtype=F32)
    out = dict(n=n, K=K, normals=z, centers=centers, sigma=sigma, sd_floor=sd_floor, clip=clip, bins=b.reshape(N, h, 7))
    if form == "tokens":
        tokens = (TOK_VOCAB - 1 - b).astype(np.int64).reshape(N, 7 * h)
        if variant == "outside":                                   # below the action range (-> last centre) and past the vocabulary (-> first)
            flat = tokens.reshape(-1)
            idx = rng.choice(flat.size, size=max(2, flat.size // 5), replace=False)
            flat[idx[0::2]] = rng.integers(0, TOK_VOCAB - 256, len(idx[0::2]))
            flat[idx[1::2]] = TOK_VOCAB + rng.integers(0, 1000, len(idx[1::2]))
        out["tokens"] = tokens
    else:
        off = rng.uniform(-0.003, 0.003, b.shape) if variant not in ("equal",) else np.zeros(b.shape)
        x = (centers[b].astype(np.float64) + off).astype(F32)
        if variant == "equal":
            x[:] = x[:, :1]
        if variant == "floor":
            x[..., :3] = x[:, :1, :, :3]
        if variant == "clip":
            x[0, :, 0, 0], x[0, :, 0, 1] = F32(0.886), F32(0.0)
        out["actions"] = x.reshape(N, h, 7)
    return out


# ------------------------------------------------------------------------------------------------ the specified arithmetic
def token_values(tokens, centers, tok_vocab):
    b = np.clip(tok_vocab - np.asarray(tokens, dtype=np.int64) - 1, 0, len(centers) - 1)
    return np.asarray(centers, dtype=F32)[b]


def reference_stats(x, n, sd_floor):
    """x fp32 [G*n, h, 7] sample values -> dict(mean, sd_raw, sd fp32 [G, h, 6], votes int32 [G, h, 2], jwin [G, h])."""
    x = np.asarray(x, dtype=F32)
    N, h, _ = x.shape
    G = N // n
    x = x.reshape(G, n, h, 7)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((G, h, 6), dtype=F32)
        for j in range(n):                                         # one chain of fp32 adds in sample order
            s = (s + x[:, j, :, :6]).astype(F32)
        mean = (s / F32(n)).astype(F32)
        ss = np.zeros((G, h, 6), dtype=F32)
        for j in range(n):
            d = (x[:, j, :, :6] - mean).astype(F32)
            ss = (ss + (d * d).astype(F32)).astype(F32)
        var = (ss / F32(n - 1)).astype(F32) if n > 1 else np.zeros((G, h, 6), dtype=F32)
        sd_raw = np.sqrt(var).astype(F32)
        sd = np.fmax(sd_raw, F32(sd_floor)).astype(F32)
    cls = x[..., 6] >= F32(0.5)                                    # [G, n, h]
    ones = cls.sum(axis=1).astype(np.int32)
    zeros = (n - ones).astype(np.int32)
    win1 = (ones > zeros) | ((ones == zeros) & cls[:, 0])          # a tie goes to the class of sample 0
    jwin = np.argmax(cls == win1[:, None, :], axis=1)              # the lowest-index sample in the winning class
    return dict(mean=mean, sd_raw=sd_raw, sd=sd, votes=np.stack([zeros, ones], axis=-1).astype(np.int32), jwin=jwin)


def reference_values(st, z, sigma, clip):
    """-> v fp32 [G, K, h, 6]: s = sigma * sd; p = s * z; v = mean + p; clip (three roundings, fmax then fmin: a NaN lands on lo)."""
    z = np.asarray(z, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (F32(sigma) * st["sd"]).astype(F32)
        p = (s[:, None] * z).astype(F32)
        v = (st["mean"][:, None] + p).astype(F32)
        unclipped = v
        v = np.fmin(np.fmax(v, F32(clip[0])), F32(clip[1])).astype(F32)
    return v, unclipped


def nearest_center(v, centers):
    """First index that minimises |v - centers[b]| in fp32."""
    with np.errstate(invalid="ignore"):
        return np.argmin(np.abs((v[..., None] - np.asarray(centers, dtype=F32)).astype(F32)), axis=-1)


def reference_actions(actions, n, K, z, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0)):
    """actions fp32 [G*n, h, >= 7] -> dict(out fp32 [G*S, h, 7], mean, sd, votes, v, unclipped)."""
    x = np.ascontiguousarray(np.asarray(actions, dtype=F32)[:, :, :7])
    N, h, _ = x.shape
    G, S = N // n, n + K
    st = reference_stats(x, n, sd_floor)
    v, unclipped = reference_values(st, np.asarray(z, dtype=F32).reshape(G, K, h, 6), sigma, clip)
    out = np.empty((G, S, h, 7), dtype=F32)
    out[:, :n] = x.reshape(G, n, h, 7)
    out[:, n:, :, :6] = v
    grip = np.take_along_axis(x.reshape(G, n, h, 7)[..., 6], st["jwin"][:, None, :], axis=1)     # [G, 1, h]
    out[:, n:, :, 6] = grip
    return dict(st, out=out.reshape(G * S, h, 7), v=v, unclipped=unclipped)


def reference_tokens(tokens, n, K, z, centers, tok_vocab, steps, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0)):
    """tokens int64 [G*n, >= 7 steps] -> dict(out int64 [G*S, 7 steps], mean, sd, votes, v, unclipped, bstar)."""
    tok = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64)[:, :7 * steps])
    N, h = tok.shape[0], steps
    G, S = N // n, n + K
    x = token_values(tok, centers, tok_vocab).reshape(N, h, 7)
    st = reference_stats(x, n, sd_floor)
    v, unclipped = reference_values(st, np.asarray(z, dtype=F32).reshape(G, K, h, 6), sigma, clip)
    bstar = nearest_center(v, centers)
    out = np.empty((G, S, h, 7), dtype=np.int64)
    out[:, :n] = tok.reshape(G, n, h, 7)
    out[:, n:, :, :6] = tok_vocab - 1 - bstar
    out[:, n:, :, 6] = np.take_along_axis(tok.reshape(G, n, h, 7)[..., 6], st["jwin"][:, None, :], axis=1)
    return dict(st, out=out.reshape(G * S, 7 * h), v=v, unclipped=unclipped, bstar=bstar)


def reference_of(inp, form):
    G_h = inp["normals"].shape[2]
    if form == "tokens":
        return reference_tokens(inp["tokens"], inp["n"], inp["K"], inp["normals"], inp["centers"], TOK_VOCAB, G_h, inp["sigma"], inp["sd_floor"],
                                inp["clip"])
    return reference_actions(inp["actions"], inp["n"], inp["K"], inp["normals"], inp["sigma"], inp["sd_floor"], inp["clip"])


_REFS = {}


def case_reference(c):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    key = case_id(c)
    if key not in _REFS:
        _REFS[key] = reference_of(make_inputs(c), c["form"])
    return _REFS[key]
