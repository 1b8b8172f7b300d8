"""float64 references, error bounds and the shared case tables for the fp32 kernels of csrc/f32ops.hip (tests/test_f32ops_cpu.py and
tests/test_f32ops_gpu.py). Plain torch / numpy on the CPU: nothing here needs a GPU.

GEMM cases are described by layouts, not tensors: `gemm_layout` turns a case into element strides / offsets / buffer sizes (what the fake-pointer
plan query needs) and `gemm_build` materialises the same layout on any device as views of flat storages."""
import math
import random

import numpy as np
import torch

U = 2.0 ** -24             # unit roundoff of fp32 (round to nearest)
NAN_BITS = 0x7FC0DEAD      # quiet-NaN pattern the output buffers are pre-filled with: any write shows, any read of it poisons a result
TILE = {"DIRECT_FM1": (16, 32), "DIRECT_FM2": (32, 32), "TILE64": (64, 64), "TILE32_K128": (32, 32), "TILE32_K32": (32, 32)}
FAKE_A, FAKE_B, FAKE_C = 0x10000000, 0x20000000, 0x30000000   # aligned fake device addresses for the plan query (never dereferenced)

ACT64 = {
    "none": lambda x: x,
    "gelu_tanh": lambda x: torch.nn.functional.gelu(x, approximate="tanh"),
    "gelu_erf": lambda x: torch.nn.functional.gelu(x),
    "silu": torch.nn.functional.silu,
    "relu": torch.relu,
}
# sup |act'|: gelu (both forms) peaks at 1.129 near x = 1.41, silu at 1.0998 near x = 2.4
ACT_LIPSCHITZ = {"none": 1.0, "relu": 1.0, "gelu_tanh": 1.13, "gelu_erf": 1.13, "silu": 1.1}


def nan_filled(numel, device):
    return torch.full((numel,), NAN_BITS, dtype=torch.int32).view(torch.float32).to(device)


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ GEMM case table
def _case(M, N, K, a="contig", b="nk", c="slice", res="none", batch=1, a_shared=False, b_shared=False, bias="shared", act="none",
          alpha=1.0, c_bs_pad=0, a_bs_pad=0):
    """a: contig | padded (row stride K + 8) | colmajor ([K, M].T) | offset1 (storage offset of one element) | oddstride (row stride % 4 != 0)
    b: nk ([N, K]) | kn ([K, N], b_is_kn) | nk_strided (row stride K + 8)
    c: slice (columns 2 .. N + 2 of a buffer N + 5 wide) | tight (row stride N)       -- both with two guard rows after M
    res: none | own (its own row stride N + 1 != C's) | inplace (residual is out)
    bias: none | shared | batch (bias_batch_stride = N)
    c_bs_pad / a_bs_pad: extra elements between the batches of C / A (a_bs_pad % 4 != 0 takes the batch off the direct kernel)"""
    return dict(M=M, N=N, K=K, a=a, b=b, c=c, res=res, batch=batch, a_shared=a_shared, b_shared=b_shared, bias=bias, act=act, alpha=alpha,
                c_bs_pad=c_bs_pad, a_bs_pad=a_bs_pad)


MS = (1, 15, 16, 17, 31, 33, 64, 65, 100)
NS = (1, 31, 32, 33, 63, 65, 130)
KS = (1, 7, 31, 33, 64, 80, 127, 128, 144, 256, 272, 1040, 2048)
ACTS = ("none", "gelu_tanh", "gelu_erf", "silu", "relu")
ALPHAS = (1.0, -0.1, 0.5)


def gemm_cases(seed=20261017, n_random=56):
    """The shared GEMM case table: hand-placed cases for each dispatch path, layout and argument the production callers use (verifier.py,
    pi0.py), then a seeded draw from the dimension sets crossed with layouts, batch forms and epilogues. test_f32ops_cpu.py proves that the
    table reaches all five kernels with ragged M and N edges in each; test_f32ops_gpu.py runs it."""
    c = [
        # the direct kernel, both fragment counts, ragged and full edges (nn.Linear form: every verifier head GEMM)
        _case(1, 130, 2048, bias="shared", act="gelu_erf"),
        _case(15, 33, 64, res="own", act="relu", alpha=0.5),
        _case(16, 32, 80, c="tight"),
        _case(17, 31, 64, res="inplace", act="silu", alpha=-0.1),
        _case(33, 65, 1040, a="padded", b="nk_strided", res="own", act="gelu_tanh"),
        _case(100, 130, 272, res="inplace"),
        _case(64, 63, 144, c="tight", bias="none"),
        # batched as the ensemble stacks issue them: shared A, shared B, per-member bias, residual with batch, padded C slabs
        _case(1, 65, 256, batch=5, bias="batch", res="own", act="gelu_erf", c_bs_pad=3),
        _case(17, 33, 128, batch=2, a_shared=True, bias="batch", act="relu"),
        _case(31, 130, 64, batch=5, a_shared=True, b_shared=True, bias="none", c_bs_pad=5),
        _case(33, 32, 80, batch=2, b_shared=True, bias="shared", res="inplace", alpha=0.5),
        _case(100, 65, 144, batch=2, bias="batch", res="own", c="tight", act="silu", alpha=-0.1),
        # off the direct kernel: base pointer, row stride, batch stride, K % 16, K < 64, k stride
        _case(16, 33, 128, a="offset1"),
        _case(33, 63, 2048, a="oddstride", res="own", act="gelu_tanh"),
        _case(17, 65, 256, batch=2, a_bs_pad=2, bias="batch"),
        _case(15, 31, 72 + 8, a="colmajor"),
        _case(65, 130, 1040, a="colmajor", b="kn", res="own", alpha=0.5),
        _case(31, 33, 127, res="inplace", act="relu"),
        _case(64, 64, 33, c="tight"),
        _case(100, 1, 7, b="kn", bias="batch", batch=5, c_bs_pad=1),
        _case(1, 1, 1, bias="none"),
        _case(65, 33, 272, b="kn", act="gelu_erf", alpha=-0.1),
        # large grids: the 64x64 tile (>= 256 blocks), exact and ragged, batched, every operand layout
        _case(1024, 1024, 7, b="kn", c="tight", bias="none"),
        _case(1000, 1030, 33, b="kn", res="own", act="relu"),
        _case(512, 512, 31, batch=4, bias="batch", c="tight"),
        _case(500, 450, 80, batch=5, a="colmajor", b_shared=True, res="inplace", alpha=0.5, c_bs_pad=7),
        _case(1000, 1030, 127, a="oddstride", b="nk_strided", act="silu", alpha=-0.1),
        # large grid that stays on the direct kernel (below the direct bound)
        _case(1000, 1030, 64, res="own", act="gelu_tanh"),
    ]
    rnd = random.Random(seed)
    for _ in range(n_random):
        batch = rnd.choice((1, 1, 1, 2, 5))
        c.append(_case(rnd.choice(MS), rnd.choice(NS), rnd.choice(KS),
                       a=rnd.choice(("contig", "contig", "padded", "colmajor", "offset1", "oddstride")),
                       b=rnd.choice(("nk", "nk", "kn", "nk_strided")),
                       c=rnd.choice(("slice", "slice", "tight")),
                       res=rnd.choice(("none", "own", "inplace")),
                       batch=batch, a_shared=batch > 1 and rnd.random() < 0.4, b_shared=batch > 1 and rnd.random() < 0.3,
                       bias=rnd.choice(("none", "shared", "batch")) if batch > 1 else rnd.choice(("none", "shared")),
                       act=rnd.choice(ACTS), alpha=rnd.choice(ALPHAS), c_bs_pad=rnd.choice((0, 0, 3)) if batch > 1 else 0))
    for i, cs in enumerate(c):
        cs["id"] = "{:02d}-M{M}-N{N}-K{K}-{a}-{b}-{c}-res_{res}-b{batch}{sa}{sb}-bias_{bias}-{act}".format(
            i, sa="A0" if cs["a_shared"] else "", sb="B0" if cs["b_shared"] else "", **{k: v for k, v in cs.items() if k != "id"})
    return c


def gemm_layout(cs):
    """Element strides, storage offsets and storage sizes of a case. Operand storages carry a tail of 128 k-steps beyond their last element, so
    a kernel that drops a k guard reads (and the exact check sees) live values, never memory outside the tensor."""
    M, N, K, nb = cs["M"], cs["N"], cs["K"], cs["batch"]
    L = {}
    a = cs["a"]
    if a == "colmajor":
        rs, ks, off = 1, M, 0
        span = K * M
    else:
        rs = {"contig": K, "offset1": K, "padded": K + 8, "oddstride": K + 1 if (K + 1) % 4 else K + 2}[a]
        ks, off = 1, 1 if a == "offset1" else 0
        span = M * rs
    L["a_rs"], L["a_ks"], L["a_off"] = rs, ks, off
    L["a_bs"] = 0 if (cs["a_shared"] or nb == 1) else span + cs["a_bs_pad"]
    L["a_numel"] = off + (span + cs["a_bs_pad"]) * (1 if cs["a_shared"] else nb) + 128 * ks + 128
    b = cs["b"]
    if b == "kn":
        rs, ks, span = 1, N, K * N
    else:
        rs = K + 8 if b == "nk_strided" else K
        ks, span = 1, N * rs
    L["b_rs"], L["b_ks"] = rs, ks
    L["b_bs"] = 0 if (cs["b_shared"] or nb == 1) else span
    L["b_numel"] = span * (1 if cs["b_shared"] else nb) + 128 * ks + 128
    ldc, col0 = (N + 5, 2) if cs["c"] == "slice" else (N, 0)
    L["ldc"], L["c_off"] = ldc, col0
    L["c_bs"] = (M + 2) * ldc + cs["c_bs_pad"]
    L["c_numel"] = nb * L["c_bs"]
    L["ld_res"] = {"none": 0, "own": N + 1, "inplace": ldc}[cs["res"]]     # own: batch z starts at z * c_bs (the kernel's contract); read only
    L["res_numel"] = nb * L["c_bs"] + M * (N + 1) if cs["res"] == "own" else 0   # (room for C's row stride too: a kernel that mixes the two up
                                                                                    #  reads wrong values, not memory outside the tensor)
    L["bias_bs"] = N if cs["bias"] == "batch" else 0
    L["bias_numel"] = 0 if cs["bias"] == "none" else (N * nb if cs["bias"] == "batch" else N)
    return L


def gemm_plan_args(cs, ptrs=None):
    """positional and keyword arguments of ops.gemm_f32_plan for a case: with the real data pointers (a, b, out) of materialised views, or
    with fake aligned storage addresses plus the views' storage offsets"""
    L = gemm_layout(cs)
    a_ptr, b_ptr, c_ptr = ptrs if ptrs is not None else (FAKE_A + 4 * L["a_off"], FAKE_B, FAKE_C + 4 * L["c_off"])
    return ((a_ptr, L["a_rs"], L["a_ks"], b_ptr, L["b_rs"], L["b_ks"], c_ptr, L["ldc"], cs["M"], cs["N"], cs["K"]),
            dict(batch=cs["batch"], a_bs=L["a_bs"], b_bs=L["b_bs"], c_bs=L["c_bs"]))


def exact_epilogue(cs):
    """(act, alpha) of a case's exact run: relu or none, and a power of two"""
    return ("relu" if cs["act"] in ("relu", "silu", "gelu_tanh") else "none"), {1.0: 1.0, -0.1: 2.0, 0.5: 0.5}[cs["alpha"]]


def gemm_build(cs, kind, device, seed=0):
    """Materialise a case on `device`. kind = "exact": operands, bias and residual are integers in [-4, 4] (every product and partial sum is an
    integer below K * 16 < 2^24, exactly representable: the fp32 result does not depend on the summation order); "bounded": standard normal
    A, bias and residual, B scaled by K^-1/2 so the pre-activation stays where the activations bend.
    Returns a dict with the views (a [nb?, M, K], b, out [nb?, M, N], res) and the flat storages."""
    M, N, K, nb = cs["M"], cs["N"], cs["K"], cs["batch"]
    L = gemm_layout(cs)
    g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 104729 + K)

    def fill(n, scale=1.0):
        if kind == "exact":
            return torch.randint(-4, 5, (n,), generator=g).float()
        return torch.randn(n, generator=g) * scale

    sa, sb = fill(L["a_numel"]).to(device), fill(L["b_numel"], K ** -0.5).to(device)
    bias = fill(L["bias_numel"]).to(device) if L["bias_numel"] else None
    sc = nan_filled(L["c_numel"], device)
    lead = (nb,) if nb > 1 else ()
    bsz = lambda s: (s,) if nb > 1 else ()   # noqa: E731
    av = sa.as_strided(lead + (M, K), bsz(L["a_bs"]) + (L["a_rs"], L["a_ks"]), L["a_off"])
    if cs["b"] == "kn":
        bv = sb.as_strided(lead + (K, N), bsz(L["b_bs"]) + (L["b_ks"], L["b_rs"]), 0)
    else:
        bv = sb.as_strided(lead + (N, K), bsz(L["b_bs"]) + (L["b_rs"], L["b_ks"]), 0)
    out = sc.as_strided(lead + (M, N), bsz(L["c_bs"]) + (L["ldc"], 1), L["c_off"])
    res = sres = None
    if cs["res"] == "own":
        sres = fill(L["res_numel"]).to(device)
        res = sres.as_strided(lead + (M, N), bsz(L["c_bs"]) + (L["ld_res"], 1), 0)
    elif cs["res"] == "inplace":
        out.copy_(fill(nb * M * N).view(lead + (M, N)).to(device))
        res = out
    return dict(a=av, b=bv, out=out, res=res, bias=bias, c_store=sc, L=L)


def gemm_call_kwargs(cs, t, act, alpha):
    """keyword arguments of ops.gemm_f32(t["a"], t["b"], **kw)"""
    L = t["L"]
    return dict(bias=t["bias"], act=act, alpha=alpha, residual=t["res"], out=t["out"], b_is_kn=cs["b"] == "kn", batch=cs["batch"],
                a_bs=L["a_bs"], b_bs=L["b_bs"], c_bs=L["c_bs"], M=cs["M"], N=cs["N"], K=cs["K"], bias_bs=L["bias_bs"])


def _operands64(cs, t, res_before):
    nb = cs["batch"]
    a = t["a"].detach().cpu().double().expand((nb,) + tuple(t["a"].shape[-2:])) if nb > 1 else t["a"].detach().cpu().double()
    b = t["b"].detach().cpu().double()
    if cs["b"] != "kn":
        b = b.transpose(-1, -2)
    bias = None
    if t["bias"] is not None:
        bias = t["bias"].detach().cpu().double()
        bias = bias.view(nb, 1, cs["N"]) if cs["bias"] == "batch" and nb > 1 else bias.view(-1)[:cs["N"]]
    res = None if res_before is None else res_before.detach().cpu().double()
    return a, b, bias, res


def gemm_ref64(cs, t, act, alpha, res_before):
    """float64 residual + alpha * act(A B^T + bias); `res_before` = the residual's values before the launch (a clone when residual is out).
    alpha is the fp32 value the kernel multiplies by."""
    a, b, bias, res = _operands64(cs, t, res_before)
    x = a @ b
    if bias is not None:
        x = x + bias
    y = float(np.float32(alpha)) * ACT64[act](x)
    return y if res is None else res + y


# The fp32 kernels accumulate with v_mfma_f32_16x16x4_f32: per output element a chain of fused multiply-adds, one rounding per k term in
# whatever order the kernel's k <-> lane map gives. The classical forward bound for a length-K dot product in ANY order with at most n
# roundings on the path of a term is gamma_n * sum_k |a_k b_k|, gamma_n = n u / (1 - n u). Roundings on a term's path:
#   K        the k chain itself (gemm_f32_k: one chain of K; gemm_f32_direct_k: four chains of K / 4 -- fewer)
#   + 3      gemm_f32_direct_k adds its four waves' partial tiles in LDS order: ((w0 + w1) + w2) + w3
#   + 1      the bias add (its rounding is relative to |x| <= |A||B|^T + |bias|)
#   + 1      covers 1 / (1 - n u) for every K of the table (n u < 1.3e-4 at K = 2048: less than 0.3 of a rounding)
# => c = 5. Evaluating the activation in fp32 adds, relative to |x| (again <= |A||B|^T + |bias|):
#   none / relu  0
#   gelu_*       10: 0.5 x (1 + t(x)) with t = tanhf / erff: the OpenCL accuracy bounds (5 ulp tanh; erf is given 16 ulp there, ocml's erff is
#                documented at 2) put <= 8 u |x| on 0.5 x (1 + t), the cubic argument and the two multiplies the rest
#   silu         6 + 1.5 |x|: x / (1 + e^-x); the fast exponential's argument scaling costs |x| log2(e) u relative in e^-x, the add, the
#                division and the exponential itself at most 6 more
# These enter as extra `c` (they scale the same |A||B|^T + |bias| term). Then |alpha| and the Lipschitz constant of the activation, and one
# ulp (2^-23 relative) of the value for the multiplication by alpha and one ulp of the result for the residual add.
GEMM_C_SUM = 5


def gemm_bound(cs, t, act, alpha, res_before):
    """Per-element bound on |fp32 kernel - float64 reference| of a case:
        |alpha| * Lip(act) * (K + c) * 2^-24 * (|A| |B|^T + |bias|)  +  2^-23 * (|alpha act(x)| [if alpha != 1] + |result| [if residual])
    with c = GEMM_C_SUM + the activation's evaluation term (see the derivation above this function). Nothing here was tuned on device output."""
    a, b, bias, res = _operands64(cs, t, res_before)
    x = a @ b
    s = a.abs() @ b.abs()
    if bias is not None:
        x, s = x + bias, s + bias.abs()
    c_act = {"none": 0.0, "relu": 0.0, "gelu_tanh": 10.0, "gelu_erf": 10.0}.get(act)
    if c_act is None:
        c_act = 6.0 + 1.5 * x.abs()
    al = abs(float(np.float32(alpha)))
    y = al * ACT64[act](x).abs()
    bound = al * ACT_LIPSCHITZ[act] * (cs["K"] + GEMM_C_SUM + c_act) * U * s
    if al != 1.0:
        bound = bound + 2 * U * y
    if res is not None:
        bound = bound + 2 * U * (res + float(np.float32(alpha)) * ACT64[act](x)).abs()
    return bound + 1e-37   # (an exact zero on both sides still compares <=)


def outside_untouched(t, cs):
    """the bytes of C's storage outside [batch][M, N] still hold the pre-fill pattern: pad columns, rows after M, slabs between batches"""
    L, nb = t["L"], cs["batch"]
    store = bits(t["c_store"].detach().cpu())
    mask = torch.zeros(store.numel(), dtype=torch.bool)
    lead = (nb,) if nb > 1 else ()
    bsz = (L["c_bs"],) if nb > 1 else ()
    mask.as_strided(lead + (cs["M"], cs["N"]), bsz + (L["ldc"], 1), L["c_off"]).fill_(True)
    return bool((store[~mask] == torch.tensor(NAN_BITS, dtype=torch.int32)).all())


# ------------------------------------------------------------------------------------------------ attention
MHA_SHAPES = [(2, 10, 10, 8, 64), (3, 1, 130, 4, 32), (1, 64, 128, 1, 128), (2, 90, 91, 2, 16), (2, 5, 7, 3, 6), (2, 5, 8, 3, 20), (1, 9, 9, 2, 4)]


def mha_ref64(q, k, v, H, Dh, pad=None):
    """q [B, Tq, H*Dh], k / v [B, Tk, H*Dh] (any dtype) -> float64 [B, Tq, H*Dh]; pad bool [B, Tk], True = ignore the key. A batch whose keys
    are all padded gives NaN rows (softmax over -inf only), as nn.MultiheadAttention does."""
    B, Tq = q.shape[:2]
    qh, kh, vh = (x.double().reshape(B, -1, H, Dh).transpose(1, 2) for x in (q, k, v))
    s = (qh * float(np.float32(Dh ** -0.5))) @ kh.transpose(-1, -2)
    if pad is not None:
        s = s.masked_fill(pad.bool()[:, None, None, :], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Tq, H * Dh)


# ------------------------------------------------------------------------------------------------ row kernels
ROW_WIDTHS = (1, 3, 255, 256, 257, 576, 1000, 5000)
ROW_COUNTS = (1, 9)


def layernorm_ref64(x, w, b, eps=1e-5):
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    y = (x - mu) / torch.sqrt(var + float(np.float32(eps)))
    if w is not None:
        y = y * w.double()
    return y if b is None else y + b.double()


def _block_sum_f32(v):
    """layernorm_f32_k's block_sum in numpy fp32: 256 threads stride the row, each wave of 64 adds in a butterfly (xor 32, 16, ... 1), the four
    wave totals are added in order"""
    acc = np.zeros(256, np.float32)
    for c0 in range(0, v.shape[0], 256):
        seg = v[c0:c0 + 256]
        acc[:seg.shape[0]] += seg
    idx = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[idx ^ o]).astype(np.float32)
    t = np.float32(0)
    for w in range(4):
        t = np.float32(t + acc[w * 64])
    return t


def layernorm_two_pass_f32(x, w, b, eps=1e-5):
    """numpy fp32 restatement of layernorm_f32_k (two passes: mean, then the deviations' mean square), x [rows, dim] float32"""
    x = np.asarray(x, np.float32)
    out = np.empty_like(x)
    dim = x.shape[1]
    for r in range(x.shape[0]):
        mean = np.float32(_block_sum_f32(x[r]) / np.float32(dim))
        d = (x[r] - mean).astype(np.float32)
        rstd = np.float32(1.0) / np.sqrt(np.float32(_block_sum_f32((d * d).astype(np.float32)) / np.float32(dim) + np.float32(eps)))
        y = (d * rstd).astype(np.float32)
        if w is not None:
            y = (y * np.asarray(w, np.float32)).astype(np.float32)
        if b is not None:
            y = (y + np.asarray(b, np.float32)).astype(np.float32)
        out[r] = y
    return out


def layernorm_offset_atol(x, w):
    """Absolute tolerance for rows with a large common offset. The two-pass scheme subtracts an fp32 mean: its error dm (the tree sum of `dim`
    values near max|x| rounds at every level; ~ 2 * 2^-24 * max|x| for the block's 256-lane / butterfly / 4-wave order) shifts every deviation
    by the same dm, i.e. the normalised output by dm / sigma, times |w|. Added to the file's 2e-5."""
    x = x.double()
    sigma = x.std(-1, unbiased=False).min().item()
    wmax = 1.0 if w is None else w.abs().max().item()
    return 2e-5 + 2 * U * x.abs().max().item() / sigma * wmax


def xent_diag_ref64(x):
    """x [rows, cols] -> (loss float64 [rows] = logsumexp(row) - row[r], rank int64 [rows] = entries strictly above row[r], plus equal ones at a
    lower column)"""
    rows, cols = x.shape
    xd = x.double()
    d = xd[torch.arange(rows), torch.arange(rows)]
    loss = torch.logsumexp(xd, -1) - d
    col = torch.arange(cols)[None]
    ahead = (x > x[torch.arange(rows), torch.arange(rows)][:, None]) | ((x == x[torch.arange(rows), torch.arange(rows)][:, None]) &
                                                                        (col < torch.arange(rows)[:, None]))
    return loss, ahead.sum(-1)


def masked_mean_ref64(x, pad):
    """x [B, T, D], pad bool [B, T] or None: sum_t x (1 - pad) / clamp(sum(1 - pad), min=1e-9)"""
    keep = torch.ones(x.shape[:2], dtype=torch.float64) if pad is None else (~pad.bool()).double()
    return (x.double() * keep[..., None]).sum(1) / keep.sum(1, keepdim=True).clamp(min=1e-9)


def sincos_ref64(t, dim, min_period, max_period):
    """create_sinusoidal_pos_embedding in torch float64 -> bf16 (the reference of test_kernels_gpu.py's test, any dim)"""
    half = dim // 2
    fr = torch.linspace(0.0, 1.0, half, dtype=torch.float64)
    per = min_period * (max_period / min_period) ** fr
    arg = (1.0 / per * 2 * math.pi)[None] * t.double()[:, None]
    return torch.cat([arg.sin(), arg.cos()], 1).to(torch.bfloat16)


def sincos_numpy_bf16(t, dim, min_period, max_period):
    """the kernel's own formula (fraction = i / (half - 1), period = min * (max / min)^fraction, arg = 1 / period * 2 pi * t) in numpy float64,
    rounded float64 -> float32 -> bf16 as the kernel rounds"""
    half = dim // 2
    i = np.arange(half, dtype=np.float64)
    fraction = i / (half - 1) if half > 1 else np.zeros(half)
    period = min_period * np.power(max_period / min_period, fraction)
    arg = (1.0 / period * 2.0 * 3.141592653589793)[None] * np.asarray(t, np.float32).astype(np.float64)[:, None]
    v = np.concatenate([np.sin(arg), np.cos(arg)], 1).astype(np.float32)
    return torch.from_numpy(v).to(torch.bfloat16)
