"""Reference of cover_proposal_prior_tokens / cover_proposal_prior_actions (include/cover_hip.h) and the case table of
tests/test_proposal_prior_{cpu,gpu}.py.

The kernels' arithmetic is specified rounding by rounding, so the reference restates it in numpy fp32: the fit is augment_ref's
(imported, so the two references cannot drift apart, as the two kernels share one device function), and the row chain is an explicit
Python loop over (step, dim) with one np.float32 operation per rounding, vectorised over groups and rows only -- never np.sum, which is
pairwise. The GPU results are compared with it as integer bit patterns.

A case is one combination of form ("tokens" / "actions"), shape (G, n_fit, S, h) and input variant."""
import numpy as np

from tests import augment_ref as AR

F32 = np.float32
TOK_VOCAB = AR.TOK_VOCAB

# (G, n_fit, S, h): groups (prompts), rows the Gaussian is fitted to, rows per group, steps
SHAPES = [(1, 1, 1, 1),          # one row: variance 0, the floor on every dim, the row sits on its own mean
          (2, 1, 4, 2),          # n_fit = 1 with rows behind it
          (2, 2, 6, 1),          # n_fit = 2
          (2, 5, 8, 1),
          (2, 4, 4, 3),          # S == n_fit: policy samples scored among their siblings, no augmentation
          (8, 5, 12, 4),         # the float form reads it through the strides (10 * 32, 32) of a [B, 10, 32] buffer
          (3, 4, 300, 2)]        # S > 256: two passes of the row loop
STRIDED = (8, 5, 12, 4)
VARIANTS = ("spread", "noshare", "floor", "tie", "zero", "outside", "nan")
SIGMA, SD_FLOOR = 0.8, 1e-3      # sigma is no power of two: the rounding of sigma * sd is part of what is compared


def log_shares(n_fit, alpha):
    """host.vote_log_shares restated: float32(log((c + alpha) / (n_fit + 2 alpha))) in float64, c = 0..n_fit."""
    c = np.arange(n_fit + 1, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log((c + np.float64(alpha)) / (np.float64(n_fit) + 2.0 * np.float64(alpha))).astype(F32)


def feasible(form, shape, variant):
    G, n, S, h = shape
    if variant == "floor":
        return n >= 2                           # one fitted row has sd 0 everywhere: the floor is then active on all dims ("spread" shows it)
    if variant == "tie":
        return n % 2 == 0                       # a tie needs an even number of voters
    if variant == "zero":
        return S > n                            # a row whose class nobody voted for is not among the voters
    if variant == "outside":
        return form == "tokens"                 # about the centre table
    if variant == "nan":
        return form == "actions" and S > n      # tokens cannot carry one; in a fitted row it would reach every row through the mean
    return True


def cases(forms=("tokens", "actions"), shapes=None, variants=VARIANTS):
    return [dict(form=f, shape=s, variant=v) for f in forms for s in (shapes if shapes is not None else SHAPES) for v in variants
            if feasible(f, s, v)]


def case_id(c):
    return f"{c['form']}-{'x'.join(map(str, c['shape']))}-{c['variant']}"


def make_inputs(c):
    """-> dict: tokens int64 [G*S, 7h] or actions fp32 [G*S, h, 7] (contiguous; the layout is the caller's to apply), centers fp32 [255],
    sigma, sd_floor, log_share fp32 [n_fit + 1] or None, n_fit, S, and for the nan variant nan_rows (global row indices)."""
    form, (G, n, S, h), variant = c["form"], c["shape"], c["variant"]
    seed = 100 * SHAPES.index(c["shape"]) + VARIANTS.index(variant) + (50 if form == "actions" else 0) + 9
    rng = np.random.default_rng(seed)
    centers = AR.openvla_centers()
    sigma, sd_floor = (1.0 if variant == "noshare" else SIGMA), SD_FLOOR           # noshare: the plain fit, sigma 1 and no gripper term
    log_share = None if variant == "noshare" else log_shares(n, 0.0 if variant == "zero" else 1.0)
    mid = rng.integers(60, 195, (G, 1, h, 7))
    b = np.clip(mid + rng.integers(-40, 41, (G, S, h, 7)), 0, AR.N_CENTERS - 1)        # rows scattered about a per-(group, step, dim) centre
    cls = rng.integers(0, 2, (G, S, h))                                             # gripper class: bins 192.. are >= 0.5
    if variant == "tie":
        cls[:, :n] = (np.arange(n) < n // 2)[None, :, None]
    if variant == "zero":
        cls[:, :n] = 1                                                              # every voter is class 1 ...
        cls[:, n:, 0] = np.arange(S - n)[None, :] % 2                               # ... and every other row behind them class 0 at step 0
    b[..., 6] = np.where(cls == 1, rng.integers(195, 250, (G, S, h)), rng.integers(5, 185, (G, S, h)))
    if variant == "floor":
        b[:, :n, :, :3] = b[:, :1, :, :3]                                           # dims 0-2: the fitted rows agree, sd 0, below the floor
        b[:, 0, :, 3:6], b[:, 1, :, 3:6] = 30, 220                                  # dims 3-5: two fitted rows 190 bins apart
        sd_floor = 0.02
    out = dict(n_fit=n, S=S, centers=centers, sigma=sigma, sd_floor=sd_floor, log_share=log_share)
    if form == "tokens":
        tokens = (TOK_VOCAB - 1 - b).astype(np.int64).reshape(G * S, 7 * h)
        if variant == "outside":                                   # below the action range (-> last centre) and past the vocabulary (-> first)
            flat = tokens.reshape(-1)
            idx = rng.choice(flat.size, size=max(2, flat.size // 5), replace=False)
            flat[idx[0::2]] = rng.integers(0, TOK_VOCAB - 256, len(idx[0::2]))
            flat[idx[1::2]] = TOK_VOCAB + rng.integers(0, 1000, len(idx[1::2]))
        out["tokens"] = tokens
    else:
        x = (centers[b].astype(np.float64) + rng.uniform(-0.003, 0.003, b.shape)).astype(F32)
        if variant == "floor":
            x[:, :n, :, :3] = x[:, :1, :, :3]
        if variant == "nan":
            rows = [(g, n + (g % (S - n))) for g in range(0, G, 2)]                 # one row behind the voters in every other group
            for g, r in rows:
                x[g, r, h - 1, (g + 2) % 6] = np.nan
            out["nan_rows"] = np.array([g * S + r for g, r in rows])
        out["actions"] = x.reshape(G * S, h, 7)
    return out


# ------------------------------------------------------------------------------------------------ the specified arithmetic
def reference_prior(x, S, n_fit, sigma, sd_floor, log_share=None):
    """x fp32 [G*S, h, >= 7] row values -> dict(prior fp32 [G*S], acc fp32 [G, S], counts int [G, S, h] (the votes of each row's own
    class), mean, sd_raw, sd fp32 [G, h, 6], votes int32 [G, h, 2]) -- the fit is augment_ref.reference_stats over the first n_fit rows
    of every group."""
    x = np.ascontiguousarray(np.asarray(x, dtype=F32)[:, :, :7])
    N, h, _ = x.shape
    G = N // S
    xg = x.reshape(G, S, h, 7)
    st = AR.reference_stats(np.ascontiguousarray(xg[:, :n_fit]).reshape(G * n_fit, h, 7), n_fit, sd_floor)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = (F32(sigma) * st["sd"]).astype(F32)
        acc = np.zeros((G, S), dtype=F32)
        for t in range(h):                                         # one chain per row, in (step, dim) order
            for d in range(6):
                dev = (xg[:, :, t, d] - st["mean"][:, None, t, d]).astype(F32)
                z = (dev / s[:, None, t, d]).astype(F32)
                sq = (z * z).astype(F32)
                acc = (acc + sq).astype(F32)
        p = (F32(-0.5) * acc).astype(F32)
        cls = xg[..., 6] >= F32(0.5)                               # [G, S, h]
        counts = np.where(cls, st["votes"][:, None, :, 1], st["votes"][:, None, :, 0])
        if log_share is not None:
            ls = np.asarray(log_share, dtype=F32)
            for t in range(h):
                p = (p + ls[counts[:, :, t]]).astype(F32)
    return dict(st, prior=p.reshape(G * S), acc=acc, counts=counts)


def reference_tokens(tokens, S, n_fit, centers, tok_vocab, steps, sigma, sd_floor, log_share=None):
    tok = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64)[:, :7 * steps])
    return reference_prior(AR.token_values(tok, centers, tok_vocab).reshape(tok.shape[0], steps, 7), S, n_fit, sigma, sd_floor, log_share)


def values_of(inp, form, h):
    """The fp32 values the fit and the chains see: [G*S, h, 7]."""
    if form == "tokens":
        return AR.token_values(inp["tokens"], inp["centers"], TOK_VOCAB).reshape(-1, h, 7)
    return inp["actions"]


def reference_of(inp, form, h):
    return reference_prior(values_of(inp, form, h), inp["S"], inp["n_fit"], inp["sigma"], inp["sd_floor"], inp["log_share"])


_REFS = {}


def case_reference(c):
    """Computed once per case and shared by the tests: treat the arrays as read-only."""
    key = case_id(c)
    if key not in _REFS:
        _REFS[key] = reference_of(make_inputs(c), c["form"], c["shape"][3])
    return _REFS[key]
