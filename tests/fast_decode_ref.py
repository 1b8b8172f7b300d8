"""Reference of cover_fast_decode (include/cover_hip.h) and the inputs of tests/test_fast_decode_{cpu,gpu}.py.

The expansion (terminator, classification, concatenation, truncation / padding, status bits) is Python integers; the IDCT is explicit
np.float32 operations, one at a time, in the order the header states: c = float32(q) / float32(scale), then per output one chain over
k = 0 .. H-1 of prod = basis[t][k] * c[k][d]; acc = acc + prod. Never a matmul or np.sum, which choose their own order. The GPU results
are compared with it as integer bit patterns."""
import numpy as np

F32 = np.float32
TRUNCATED, PADDED, MISMATCH, STRAY, UNDECODABLE, NO_TERMINATOR = 1, 2, 4, 8, 16, 32
FATAL = MISMATCH | STRAY | UNDECODABLE


def decode_row(tokens, pieces, band, stop_ids, skip_ids, min_token, H, D, relaxed):
    """One row's tokens (a sequence of ints) -> (q: list of H * D ints, n, status). pieces: a list over the FAST ids of code-point
    lists, None = undecodable."""
    lo, hi = band
    HD = H * D
    tokens = [int(t) for t in tokens]
    stop = next((p for p, t in enumerate(tokens) if t in stop_ids), len(tokens))
    status = NO_TERMINATOR if stop == len(tokens) else 0
    symbols = []
    for t in tokens[:stop]:
        f = hi - 1 - t
        if lo <= t < hi and f < len(pieces):
            if pieces[f] is None:
                status |= UNDECODABLE
            else:
                symbols.extend(int(s) for s in pieces[f])
        elif t not in skip_ids:
            status |= STRAY
    n = len(symbols)
    if relaxed:
        status |= TRUNCATED if n > HD else PADDED if n < HD else 0
    elif n != HD:
        status |= MISMATCH
    q = [s + min_token for s in symbols[:HD]] + [0] * max(HD - n, 0)
    if status & FATAL:
        q = [0] * HD
    return q, n, status


def idct(coeff, basis, scale, H, D):
    """coeff int [B, H * D] (frequency-major), basis fp32 [H, H] -> fp32 [B, H, D], every operation one fp32 rounding."""
    assert basis.dtype == F32 and basis.shape == (H, H)
    q = np.asarray(coeff, dtype=np.int64).reshape(-1, H, D)
    c = q.astype(F32) / F32(scale)                                         # [B, k, d]
    acc = np.zeros((q.shape[0], H, D), dtype=F32)
    for k in range(H):
        prod = basis[None, :, k, None] * c[:, k, None, :]                  # [B, t, d]
        acc = acc + prod
    assert acc.dtype == F32
    return acc


def reference(tokens, pieces, basis, *, band, stop_ids, skip_ids=(), min_token, scale, horizon, action_dim, relaxed=True):
    """tokens int [B, L] -> dict(actions fp32 [B, H, D], coeff int32 [B, H * D], n_symbols int32 [B], status int32 [B])."""
    rows = [decode_row(r, pieces, band, tuple(stop_ids), tuple(skip_ids), min_token, horizon, action_dim, relaxed) for r in np.asarray(tokens)]
    coeff = np.array([r[0] for r in rows], dtype=np.int64).reshape(len(rows), horizon * action_dim)
    return dict(actions=idct(coeff, basis, scale, horizon, action_dim), coeff=coeff.astype(np.int32),
                n_symbols=np.array([r[1] for r in rows], dtype=np.int32), status=np.array([r[2] for r in rows], dtype=np.int32))


def basis64(H):
    """The orthonormal inverse DCT-II matrix in float64: what host.fast_idct_basis rounds to fp32."""
    t, k = np.arange(H, dtype=np.float64)[:, None], np.arange(H, dtype=np.float64)[None, :]
    b = np.sqrt(2.0 / H) * np.cos(np.pi * (2.0 * t + 1.0) * k / (2.0 * H))
    b[:, 0] = np.sqrt(1.0 / H)
    return b


def error_bound(coeff, scale, H, D):
    """The derived per-element bound of |fp32 chain - float64 IDCT|: (H + 3) * 2^-24 * sum_k |B64[t][k]| * |q[k][d] / scale| -- one
    rounding each for the basis entry, the quotient and the product, plus H adds. -> float64 [B, H, D]."""
    c = np.abs(np.asarray(coeff, dtype=np.float64).reshape(-1, H, D) / float(scale))
    return (H + 3) * 2.0 ** -24 * np.einsum("tk,bkd->btd", np.abs(basis64(H)), c)


# ------------------------------------------------------------------------------------------------ the constructed status rows
# A vocabulary of 200 ids: FAST ids mirrored below 200 (band 190 .. 199: ten FAST ids, of which the table decodes six), "|" = 50,
# EOS = 1, pad = 0, the format tokens 60 ("Action"), 61 (":") and BOS = 2. H * D = 6 coefficients.
BAND, END, EOS, PAD, BOS = (190, 200), 50, 1, 0, 2
STOP_IDS, SKIP_IDS = (END, EOS, PAD), (60, 61, BOS)
STATUS_H, STATUS_D, STATUS_MIN_TOKEN, STATUS_SCALE = 2, 3, -12, 4.0
STATUS_PIECES = [[], [10], [11, 12], [13, 14, 15], None, [20, 21, 22, 23, 24, 25, 26]]   # a zero-length piece, an undecodable one, one beyond H * D


def tok(f):
    """The vocabulary id of FAST id f in BAND."""
    return BAND[1] - 1 - f


def status_rows():
    """-> (names, tokens int64 [rows, 8], the status expected with relaxed, the status expected without, the coefficients expected with
    relaxed before min_token (None = a zeroed row))."""
    t = tok
    table = [
        ("terminator at position 0", [END, t(3), t(3), t(2)], PADDED, MISMATCH, []),
        ("no terminator", [t(3), t(3), 60, 61, BOS, 60, 60, 60], NO_TERMINATOR, NO_TERMINATOR, [13, 14, 15, 13, 14, 15]),
        ("EOS before the terminator", [t(3), EOS, t(3), END], PADDED, MISMATCH, [13, 14, 15]),
        ("a stray id", [t(3), 70, t(3), END], STRAY, STRAY, None),
        ("the sampler's -1", [t(3), -1, t(3), END], STRAY, STRAY, None),
        ("a FAST id beyond the table", [t(3), t(8), t(3), END], STRAY, STRAY, None),
        ("an undecodable piece", [t(3), t(4), t(3), END], UNDECODABLE, UNDECODABLE, None),
        ("exact fit", [60, 61, t(3), t(2), t(1), END], 0, 0, [13, 14, 15, 11, 12, 10]),
        ("truncation inside a piece", [t(3), t(2), t(3), END], TRUNCATED, MISMATCH, [13, 14, 15, 11, 12, 13]),
        ("zero-length pieces", [t(0), t(3), t(0), t(3), t(0), END], 0, 0, [13, 14, 15, 13, 14, 15]),
        ("one piece longer than H * D", [t(5), END], TRUNCATED, MISMATCH, [20, 21, 22, 23, 24, 25]),
        ("stray and short", [70, t(1), END], STRAY | PADDED, STRAY | MISMATCH, None),
    ]
    tokens = np.full((len(table), 8), PAD, dtype=np.int64)
    for i, row in enumerate(table):
        tokens[i, :len(row[1])] = row[1]
    return [r[0] for r in table], tokens, [r[2] for r in table], [r[3] for r in table], [r[4] for r in table]


def status_kwargs(relaxed):
    return dict(band=BAND, stop_ids=STOP_IDS, skip_ids=SKIP_IDS, min_token=STATUS_MIN_TOKEN, scale=STATUS_SCALE, horizon=STATUS_H,
                action_dim=STATUS_D, relaxed=relaxed)


# ------------------------------------------------------------------------------------------------ random cases
SHAPES = ((1, 1), (4, 7), (50, 32), (128, 32))       # (H, D): one cell, the golden's, pi0-FAST's, the limits (the basis leaves LDS)
LENGTHS = (1, 63, 64, 65, 257, 300)                  # the wave boundary, the block boundary (256) and the scan carry
N_SHORT = 40                                         # FAST ids 0 .. 39: pieces of 0 .. 9 symbols; 40: undecodable; 41: longer than H * D
CASE_MIN_TOKEN, CASE_SCALE = -300, 10.0


def case_pieces(H, D, seed=0):
    rng = np.random.default_rng(seed)
    pieces = [list(map(int, rng.integers(0, 600, size=f % 10))) for f in range(N_SHORT)]
    return pieces + [None, list(map(int, rng.integers(0, 600, size=H * D + 3)))]


def case_band(n_pieces):
    """A band that holds exactly the table's FAST ids below a vocabulary of 1000 ids (the stop and format ids stay outside it)."""
    return (1000 - n_pieces, 1000)


def case_kwargs(H, D, relaxed=True):
    return dict(band=case_band(N_SHORT + 2), stop_ids=STOP_IDS, skip_ids=SKIP_IDS, min_token=CASE_MIN_TOKEN, scale=CASE_SCALE, horizon=H,
                action_dim=D, relaxed=relaxed)


def case_tokens(B, L, H, D, seed=0):
    """int64 [B, L]: row b is of kind b % 5 -- 0 clean with a terminator, 1 clean without, 2 the long piece early (truncation), 3 a stray id,
    4 an undecodable piece; format tokens are sprinkled in, and what follows the terminator is junk that must not be read into a result."""
    rng = np.random.default_rng(seed + 1000 * L + B)
    lo, hi = case_band(N_SHORT + 2)
    out = np.empty((B, L), dtype=np.int64)
    for b in range(B):
        kind = b % 5
        row = hi - 1 - rng.integers(0, N_SHORT, size=L)
        fmt = rng.random(L) < 0.1
        row[fmt] = rng.choice(SKIP_IDS, size=int(fmt.sum()))
        if kind == 2:
            row[rng.integers(0, min(L, 3))] = hi - 1 - (N_SHORT + 1)
        if kind == 3:
            row[rng.integers(0, max(L // 2, 1))] = rng.choice([-1, 70, lo - 1, hi, 1 << 40])
        if kind == 4:
            row[rng.integers(0, max(L // 2, 1))] = hi - 1 - N_SHORT
        if kind != 1 and L > 1:
            p = int(rng.integers(L // 2, L))
            row[p] = rng.choice(STOP_IDS)
            row[p + 1:] = rng.integers(-5, 1100, size=L - p - 1)
        out[b] = row
    return out
