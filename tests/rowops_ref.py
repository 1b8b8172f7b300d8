"""References, the acceptance rule and the shared case tables for the bf16 row kernels of csrc/rowops.hip (tests/test_rowops_cpu.py and
tests/test_rowops_gpu.py). Plain torch / numpy on the CPU, no project code: nothing here needs a GPU.

Two kinds of reference:
  * exact restatements in fp32 torch, same operation order and the same bf16 roundings as include/cover_hip.h documents (RoPE, the split-K
    fold, K / V^T placement, gathers, copies, casts, the e4m3 row quantiser): the kernels must match them bit for bit;
  * float64 references (LayerNorm, RMSNorm, patchify) with the acceptance rule `neighbour_check`: every element equals bf16(ref64) or one of
    its two bf16 neighbours, and at most NEIGHBOUR_CAP of a case's elements are not equal.

rope_kv_write cases are dicts (`rope_case`); `rope_build` materialises one as flat CPU storages pre-filled with sentinels, `rope_views` turns
storages (on any device) into the call's arguments, `rope_expected` returns the three whole storages the call must leave behind and `rope_path`
names the device path the case takes from the kernel's own dispatch conditions."""
import itertools
import math

import numpy as np
import torch

BF = torch.bfloat16
NEIGHBOUR_CAP = 1e-3
SENT_QKV, SENT_K, SENT_VT, SENT_OUT = 0x7FC1, 0x4A5B, 0x3C2D, 0x7FC3      # bf16 bit patterns the buffers are pre-filled with (all non-zero)
SENT_Q8 = 0xA5


def bfr(t):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    return t.to(BF).float()


def bf_bits(t):
    return t.contiguous().view(torch.int16)


def sentinel_bf16(numel, pattern, device="cpu"):
    return torch.full((numel,), pattern, dtype=torch.int16).view(BF).to(device)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bf_bits(a.cpu()), bf_bits(b.cpu()))


# ------------------------------------------------------------------------------------------------ acceptance rule of the rounded kernels
def _ordered(b16):
    """bf16 bit patterns -> integers ordered like the values (+0 and -0 both 0): neighbours differ by one"""
    k = bf_bits(b16).to(torch.int32) & 0xFFFF
    return torch.where(k < 0x8000, k, -(k & 0x7FFF))


def _from_ordered(o):
    k = torch.where(o >= 0, o, 0x8000 | (-o))
    return torch.where(k >= 0x8000, k - 0x10000, k).to(torch.int16).view(BF)


def round_bf16_from64(ref64):
    """RNE of float64 to bf16 without the double rounding of a cast through fp32: the float cast's candidate unless a neighbour is strictly closer
    (an exact midpoint in float64 is exact in fp32 too, where the cast's own tie rule is already the right one)"""
    b = ref64.float().to(BF)
    o = _ordered(b)
    best, dist = b, (b.double() - ref64).abs()
    for step in (-1, 1):
        cand = _from_ordered(o + step)
        d = (cand.double() - ref64).abs()
        closer = d < dist
        best, dist = torch.where(closer, cand, best), torch.where(closer, d, dist)
    return best


def neighbour_check(got, ref64, hi64=None):
    """(every element is bf16(ref64) or one of its two bf16 neighbours, share of elements that are not equal).
    With hi64 the reference is the interval [ref64, hi64] of float64 values that fp32 arithmetic cannot tell apart (layernorm_bounds64,
    rmsnorm_bounds64): `equal` is then anything from bf16(ref64) to bf16(hi64), a neighbour one step outside. The interval is narrower than
    a bf16 step by orders of magnitude, so for all but the elements whose reference sits on a rounding boundary it is the plain rule."""
    assert got.dtype == BF and got.shape == ref64.shape
    g = _ordered(got.cpu())
    lo = _ordered(round_bf16_from64(ref64))
    hi = lo if hi64 is None else _ordered(round_bf16_from64(hi64))
    d = (lo - g).clamp(min=0) + (g - hi).clamp(min=0)
    ok = bool((d <= 1).all()) and not bool(got.float().isnan().any())
    return ok, float((d != 0).double().mean()) if d.numel() else 0.0


# ------------------------------------------------------------------------------------------------ float64 references
def layernorm_ref64(x, w, b, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + float(np.float32(eps))) * w.double()
    return y if b is None else y + b.double()


def rmsnorm_ref64(x, w, eps, w_offset, style):
    """style 0: x * rstd * (w_offset + w); style 1: w * bf16(x * rstd) with the inner bf16 rounding kept. w None counts as zeros."""
    x = x.double()
    rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + float(np.float32(eps)))
    ww = torch.zeros(x.shape[-1], dtype=torch.float64) if w is None else w.double()
    if style == 1:
        return ww * round_bf16_from64(x * rstd).double()
    return x * rstd * (float(np.float32(w_offset)) + ww)


U32 = 2.0 ** -24


def layernorm_bounds64(x, w, b, eps):
    """[lo, hi] around layernorm_ref64 that fp32 arithmetic cannot resolve. The kernel's mean is a sum of at most 8 + 8 + 4 fp32 additions deep
    (a thread's chunk, the wave shuffles, the block's waves) and a division: |mean error| <= 24 u max|x|, plus u max|x| for x - mean; that
    error passes through rstd * w. The products and the bias add round at 2 u (|product| + |b|), which matters only where they cancel.
    For a well-conditioned element this is ~1e-6 of a bf16 step; it is the whole value where x - mean or product + b cancels to nothing,
    and it decides the rounding where the reference sits within it of a bf16 tie (rows with a large common offset: ~1e-3 of all elements)."""
    ref = layernorm_ref64(x, w, b, eps)
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + float(np.float32(eps)))
    prod = ((xd - mean) * rstd * w.double()).abs()
    slack = 25 * U32 * xd.abs().amax(-1, keepdim=True) * rstd * w.double().abs() + 2 * U32 * (prod + (0 if b is None else b.double().abs()))
    return ref - slack, ref + slack


def rmsnorm_bounds64(x, w, eps, w_offset, style):
    """style 0: the reference itself. Style 1 rounds x * rstd to bf16 INSIDE the formula: where the float64 product lies within fp32's error of
    a bf16 tie (rsqrt 1 ulp, the sum of squares, the product: 8 u relative), fp32 arithmetic may round it the other way, which moves the
    output by a whole inner step (up to two output steps). Both roundings are then the reference."""
    ref = rmsnorm_ref64(x, w, eps, w_offset, style)
    if style != 1:
        return ref, ref
    xd = x.double()
    inner = xd / torch.sqrt((xd * xd).mean(-1, keepdim=True) + float(np.float32(eps)))
    ww = torch.zeros(x.shape[-1], dtype=torch.float64) if w is None else w.double()
    a, b = ww * round_bf16_from64(inner * (1 - 8 * U32)).double(), ww * round_bf16_from64(inner * (1 + 8 * U32)).double()
    return torch.minimum(a, b), torch.maximum(a, b)


def layernorm_f32(x, w, b, eps):
    """the two-pass fp32 arithmetic restated in torch fp32 (not the kernel's summation order)"""
    x = x.float()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    y = d * rstd * w
    return (y if b is None else y + b).to(BF)


def rmsnorm_f32(x, w, eps, w_offset, style):
    x = x.float()
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    ww = torch.zeros(x.shape[-1]) if w is None else w
    if style == 1:
        return (ww * bfr(x * rstd)).to(BF)
    return (x * rstd * (w_offset + ww)).to(BF)


def _patch_rows(x, patch):
    """[n, 3, H, W] -> [n * nP, 3 * p * p] rows, k = c * p * p + py * p + px, trailing pixels dropped"""
    n, C, H, W = x.shape
    gh, gw = H // patch, W // patch
    x = x[:, :, :gh * patch, :gw * patch].reshape(n, C, gh, patch, gw, patch)
    return x.permute(0, 2, 4, 1, 3, 5).reshape(n * gh * gw, C * patch * patch)


def _as_chw(img):
    return img.permute(0, 3, 1, 2) if img.dtype == torch.uint8 else img


def patchify_ref64(img, patch, mul, add, ld_out):
    """img uint8 [n, H, W, 3] or fp32 [n, 3, H, W] -> float64 [n * nP, ld_out]: pix * mul[c] + add[c] (mul / add as fp32 values), zero padded"""
    m = torch.tensor(mul, dtype=torch.float32).double().view(1, 3, 1, 1)
    a = torch.tensor(add, dtype=torch.float32).double().view(1, 3, 1, 1)
    rows = _patch_rows(_as_chw(img).double() * m + a, patch)
    out = torch.zeros(rows.shape[0], ld_out, dtype=torch.float64)
    out[:, :rows.shape[1]] = rows
    return out


def patchify_f32(img, patch, mul, add, ld_out, fma):
    """fp32 restatement: product and sum rounded separately, or (fma) rounded once"""
    m, a = torch.tensor(mul, dtype=torch.float32).view(1, 3, 1, 1), torch.tensor(add, dtype=torch.float32).view(1, 3, 1, 1)
    x = _as_chw(img)
    v = (x.double() * m.double() + a.double()).float() if fma else x.float() * m + a
    rows = _patch_rows(v, patch)
    out = torch.zeros(rows.shape[0], ld_out)
    out[:, :rows.shape[1]] = rows
    return out.to(BF)


NORM_DIMS = (8, 264, 2048, 2056, 4104, 8192)     # one chunk | a partial wave | exactly 256 chunks | one thread with two chunks | | the maximum
NORM_ROWS = (1, 37)
Q8_DIMS = (128, 2176, 4096, 8192)
PATCH_CASES = [(p, hw) for p in (14, 16) for hw in ((30, 45), (28, 42))] + [(16, (32, 48))]     # (patch 16 divides neither of the first two)
PATCH_MUL = (1 / 255 / 0.229, 1 / 255 / 0.224, 1 / 255 / 0.225)
PATCH_ADD = (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225)


def norm_inputs(rows, dim, kind, salt=0):
    """kind: plain (randn * 3 + 0.5, row 0 of a multi-row case zeroed) | offset (mean 64, spread 1). Returns fp32 x, w, b."""
    g = torch.Generator().manual_seed(rows * 100003 + dim * 17 + salt)
    x = torch.randn(rows, dim, generator=g)
    x = x + 64.0 if kind == "offset" else x * 3 + 0.5
    if kind == "plain" and rows > 1:
        x[0] = 0.0
    return x, torch.randn(dim, generator=g), torch.randn(dim, generator=g)


def patch_image(kind, hw, n_img=3, seed=5):
    g = torch.Generator().manual_seed(seed + hw[0])
    img = torch.randint(0, 256, (n_img, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    return img if kind == "u8" else (img.float().permute(0, 3, 1, 2) / 255 + torch.rand(n_img, 3, hw[0], hw[1], generator=g) / 512).contiguous()


# ------------------------------------------------------------------------------------------------ exact references: small row kernels
def embed_gather_ref(table, ids, scale):
    rows = table[ids.long()]
    return rows.clone() if scale == 1.0 else (rows.float() * torch.tensor(scale, dtype=torch.float32)).to(BF)


def copy_rows_ref(src, dst, rows, cols, sidx=None, didx=None):
    out = dst.clone()
    for i in range(rows):
        out[i if didx is None else int(didx[i]), :cols] = src[i if sidx is None else int(sidx[i]), :cols]
    return out


def add_rows_ref(x, add):
    return (x.float() + add[torch.arange(x.shape[0]) % add.shape[0]].float()).to(BF)


def scale_ref(x, pre_div, post_mul):
    v = x.float()
    if pre_div != 1.0:
        v = bfr(v / torch.tensor(pre_div, dtype=torch.float32))
    return (v * torch.tensor(post_mul, dtype=torch.float32)).to(BF)


def cast_f32_to_bf16_ref(x):
    return x.to(BF)


def cast_bf16_to_f32_ref(x):
    return (bf_bits(x).to(torch.int32) << 16).view(torch.float32)


def special_f32_row():
    """+-0, +-inf, NaN, fp32 subnormals, round-to-nearest-even ties under an even and an odd upper half, the largest finite fp32"""
    words = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000,
             0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x00408000, 0x7F7F7FFF]
    return torch.tensor(np.array(words, dtype=np.uint32).view(np.int32)).view(torch.float32)


# ------------------------------------------------------------------------------------------------ exact reference: e4m3 row quantiser
def act_perm(kp):
    """byte position -> k inside a quantised row: in every 64-block, byte 16 g + 8 h + e holds k = 32 h + 8 g + e"""
    p = np.arange(kp)
    c, r = p // 64, p % 64
    g, h, e = r // 16, (r // 8) % 2, r % 8
    return torch.from_numpy(c * 64 + 32 * h + 8 * g + e)


def quantize_rows_e4m3_ref(y):
    """bf16 [M, K] (K % 64 == 0) -> (uint8 [M, K] e4m3 bytes in operand order, fp32 [M] scales): the smallest power of two s with amax / s <= 448
    (1 for a zero row), RNE e4m3 of y / s"""
    yf = y.float()
    amax = yf.abs().amax(1)
    s = torch.where(amax > 0, torch.pow(2.0, torch.ceil(torch.log2(amax.double() / 448.0))).float(), torch.ones_like(amax))
    nat = (yf / s[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return nat[:, act_perm(y.shape[1])], s


def q8_inputs(dim, style, seed=0):
    """5 rows; row 1 zero; row 2 built so that its largest output is 448 * 2^-5 = 14 up to a few fp32 ulps before the bf16 rounding (every
    other output of the row stays below 8). Returns fp32 x (bf16-representable), w, w_offset."""
    g = torch.Generator().manual_seed(dim * 7 + style + seed)
    x = bfr(torch.randn(5, dim, generator=g))
    x[1] = 0.0
    x[2] = x[2].clamp(-2.5, 2.5)
    x[2, 3] = 2.0
    w = 1.0 + 0.1 * torch.randn(dim, generator=g).clamp(-3, 3)
    w_offset = 0.0 if style == 1 else 1.0
    if style == 0:
        w = w - 1.0
    rstd = torch.rsqrt((x[2].double() ** 2).mean() + 1e-6)
    u = x[2, 3].double() * rstd
    if style == 1:
        u = round_bf16_from64(u).double()
    w[3] = float(14.0 / u) - w_offset
    return x, w, w_offset


# ------------------------------------------------------------------------------------------------ exact references: RoPE, fold, placement
N_POS = 48


def rope_tables(D, n_pos=N_POS):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    ang = torch.arange(n_pos).float()[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def rope_rotate(x, pos, cos, sin, mode):
    """x fp32 [rows, heads, D] of bf16 values, pos [rows] already clamped. Mode 1: fp32 products rounded one by one (no FMA), one bf16 rounding;
    mode 2: bf16 cos / sin and a bf16 rounding after every operation (HF rotate_half in bf16); mode 0: x."""
    if mode == 0:
        return bfr(x)
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    c, s = cos[pos.long()][:, None, :], sin[pos.long()][:, None, :]
    if mode == 2:
        c, s = bfr(c), bfr(s)
        return torch.cat([bfr(bfr(x1 * c) + bfr(-x2 * s)), bfr(bfr(x2 * c) + bfr(x1 * s))], -1)
    return torch.cat([bfr(x1 * c - x2 * s), bfr(x2 * c + x1 * s)], -1)


def fold_ref(partial, bias):
    """fp32 [S, rows, N] -> bf16(((p0 + p1) + ...) + bias) as fp32"""
    v = torch.zeros_like(partial[0])
    for s in range(partial.shape[0]):
        v = v + partial[s]
    if bias is not None:
        v = v + bias
    return bfr(v)


def rope_case(T, D, mode, heads=(4, 2), B=1, pos="rand", kcache=True, slot=True, toff=True, ld_pad=0, qkv_off=0, cache_pad=False, k_odd=False,
              cs_off=0, k_offset=0, vt_offset=0, t_offset=2, S=0, bias=False, tag=""):
    """pos: rand | none (pos = t) | clamp (holds -3 and n_pos + 5). ld_pad: extra columns in a qkv row. qkv_off: the view starts this many elements
    into its storage. cache_pad: cache strides with padding (multiples of 8 for K). k_odd: a K head stride that is no multiple of 8. cs_off: the
    cos / sin views start this many floats into their storages. S > 0: values come from S split-K partials (+ bias)."""
    cs = dict(T=T, D=D, mode=mode, Hq=heads[0], Hkv=heads[1], B=B, pos=pos, kcache=kcache, slot=slot, toff=toff, ld_pad=ld_pad, qkv_off=qkv_off,
              cache_pad=cache_pad, k_odd=k_odd, cs_off=cs_off, k_offset=k_offset, vt_offset=vt_offset, t_offset=t_offset, S=S, bias=bias)
    cs["id"] = f"{rope_path(cs)}-T{T}-D{D}-m{mode}-h{heads[0]}x{heads[1]}-B{B}-pos_{pos}" + ("" if kcache else "-nokc") + (f"-{tag}" if tag else "")
    return cs


def rope_geometry(cs):
    """element strides, offsets and storage sizes of a case"""
    Hq, Hkv, D, B, T = cs["Hq"], cs["Hkv"], cs["D"], cs["B"], cs["T"]
    ncols = (Hq + 2 * Hkv) * D
    toffs = [(3 * b + 1) % 5 for b in range(B)] if cs["toff"] else [0] * B
    slots = [B - b for b in range(B)] if cs["slot"] else list(range(B))          # slot 0 of the B + 1 stays unused under a slot table
    tcap = cs["t_offset"] + max(toffs + [0]) + T + 3
    kh = D + (3 if cs["k_odd"] else 8 if cs["cache_pad"] else 0)
    kt = Hkv * kh + (8 if cs["cache_pad"] else 0)
    ks = tcap * kt + (16 if cs["cache_pad"] else 0)
    vd = tcap + (5 if cs["cache_pad"] else 0)
    vh = D * vd + (3 if cs["cache_pad"] else 0)
    vs = Hkv * vh + (7 if cs["cache_pad"] else 0)
    return dict(ncols=ncols, ld=ncols + cs["ld_pad"], rows=B * T, toffs=toffs, slots=slots, tcap=tcap, k_strides=(ks, kt, kh), vt_strides=(vs, vh, vd),
                k_numel=cs["k_offset"] + (B + 1) * ks + 8, vt_numel=cs["vt_offset"] + (B + 1) * vs + 8)


def rope_path(cs):
    """the device path, from the conditions of rope_v_tokens / rope_qk_vec (csrc/rowops.hip); storages are 16-byte aligned, so a pointer's alignment
    is its element offset's"""
    ld = (cs["Hq"] + 2 * cs["Hkv"]) * cs["D"] + cs["ld_pad"]
    multi = cs["T"] >= 16 and cs["S"] <= 0 and ld % 8 == 0 and cs["qkv_off"] % 8 == 0
    if not (multi and cs["D"] % 8 == 0):
        return "scalar"
    if cs["mode"] == 0 and not cs["kcache"]:
        return "vtok_noqk"
    kh = cs["D"] + (3 if cs["k_odd"] else 8 if cs["cache_pad"] else 0)
    k_ok = not cs["kcache"] or (cs["k_offset"] % 8 == 0 and kh % 8 == 0)          # (the other two K strides are multiples of 8 whenever kh is)
    vec = cs["D"] in (64, 128, 256) and cs["mode"] != 0 and cs["cs_off"] % 4 == 0 and k_ok
    return "vtok_vecqk" if vec else "vtok_scalarqk"


def rope_build(cs, seed=0):
    """flat CPU storages of a case, every output buffer pre-filled with its sentinel"""
    g = torch.Generator().manual_seed(seed + cs["T"] * 1009 + cs["D"] * 31 + cs["mode"] * 7 + cs["B"])
    geo = rope_geometry(cs)
    rows, ncols, ld, half = geo["rows"], geo["ncols"], geo["ld"], cs["D"] // 2
    t = dict(geo=geo)
    t["qkv"] = sentinel_bf16(cs["qkv_off"] + rows * ld + 8, SENT_QKV)
    t["partial"] = t["bias"] = None
    if cs["S"] > 0:
        # sums that depend on their order. Odd columns: magnitudes 1, 2^-20, 1. Even columns: p0 = a, p1 = -a + c 2^-18, p2 = t 2^-20, so that
        # (p0 + p1) + p2 keeps t while (p2 + p1) + p0 or p0 + (p1 + p2) round it away at a's 2^-24: a difference of 2^-7 of the 2^-18 result
        p = torch.randn(cs["S"], rows, ncols, generator=g)
        even = (torch.arange(ncols) % 2 == 0)
        if cs["S"] > 1:
            p[1] = torch.where(even, -p[0] + torch.randn(rows, ncols, generator=g) * 2.0 ** -18, p[1] * 2.0 ** -20)
        if cs["S"] > 2:
            p[2] = torch.where(even, p[2] * 2.0 ** -20, p[2])
        t["partial"] = p.contiguous()
        if cs["bias"]:
            t["bias"] = torch.randn(ncols, generator=g) * torch.where(even, 2.0 ** -20, 1.0)
    else:
        rope_views(cs, t)[0].copy_(torch.randn(rows, ncols, generator=g).to(BF))
    if cs["pos"] == "none":
        t["pos"] = None
    else:
        t["pos"] = torch.randint(0, N_POS, (rows,), generator=g, dtype=torch.int32)
        if cs["pos"] == "clamp" and rows:
            t["pos"][0], t["pos"][rows - 1], t["pos"][rows // 2] = -3, N_POS + 5, N_POS - 1
    cos, sin = rope_tables(cs["D"])
    t["cos"], t["sin"] = torch.full((cs["cs_off"] + N_POS * half,), 7.0), torch.full((cs["cs_off"] + N_POS * half,), 7.0)
    t["cos"][cs["cs_off"]:] = cos.reshape(-1)
    t["sin"][cs["cs_off"]:] = sin.reshape(-1)
    t["k"] = sentinel_bf16(geo["k_numel"], SENT_K) if cs["kcache"] else None
    t["vt"] = sentinel_bf16(geo["vt_numel"], SENT_VT)
    t["slot"] = torch.tensor(geo["slots"], dtype=torch.int32) if cs["slot"] else None
    t["toff"] = torch.tensor(geo["toffs"], dtype=torch.int32) if cs["toff"] else None
    return t


def rope_to(t, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in t.items()}


def rope_views(cs, t):
    """(the qkv view, keyword arguments of ops.rope_kv_write / ops.rope_args) over the storages of `t`, on whatever device they live"""
    geo, half = t["geo"], cs["D"] // 2
    qkv = t["qkv"][cs["qkv_off"]:cs["qkv_off"] + geo["rows"] * geo["ld"]].view(geo["rows"], geo["ld"])[:, :geo["ncols"]]
    if cs.get("mode") is None or "cos" not in t:
        return qkv, {}
    kw = dict(positions=t["pos"], rope_mode=cs["mode"], k_cache=t["k"], k_strides=geo["k_strides"] if cs["kcache"] else (0, 0, 0),
              k_offset=cs["k_offset"] if cs["kcache"] else 0, vt_cache=t["vt"], vt_strides=geo["vt_strides"], vt_offset=cs["vt_offset"],
              slot_of_batch=t["slot"], t_offset_of_batch=t["toff"], t_offset=cs["t_offset"])
    kw["cos"] = t["cos"][cs["cs_off"]:].view(N_POS, half)
    kw["sin"] = t["sin"][cs["cs_off"]:].view(N_POS, half)
    if t["partial"] is not None:
        kw["partial"], kw["bias"] = t["partial"], t["bias"]
    return qkv, kw


def rope_values(cs, t):
    """what the call must compute, by logical index: q [rows, Hq, D], k [B, T, Hkv, D] (rotated), v [B, T, Hkv, D], all bf16"""
    geo = t["geo"]
    Hq, Hkv, D, B, T = cs["Hq"], cs["Hkv"], cs["D"], cs["B"], cs["T"]
    if t["partial"] is not None:
        x = fold_ref(t["partial"], t["bias"])
    else:
        x = rope_views(cs, t)[0].float()
    x = x.reshape(geo["rows"], Hq + 2 * Hkv, D)
    pos = torch.arange(T, dtype=torch.int32).repeat(B) if t["pos"] is None else t["pos"]
    pos = pos.clamp(0, N_POS - 1)
    cos, sin = rope_tables(D)
    qk = rope_rotate(x[:, :Hq + Hkv], pos, cos, sin, cs["mode"])
    return (qk[:, :Hq].to(BF), qk[:, Hq:].reshape(B, T, Hkv, D).to(BF), x[:, Hq + Hkv:].reshape(B, T, Hkv, D).to(BF))


def _cache_index(geo, cs, strides_bthd, base):
    """flat element index of cell (b, t, h, d) -> long [B, T, Hkv, D]"""
    B, T, Hkv, D = cs["B"], cs["T"], cs["Hkv"], cs["D"]
    sb, st, sh, sd = strides_bthd
    slot = torch.tensor(geo["slots"], dtype=torch.long).view(B, 1, 1, 1)
    tt = (cs["t_offset"] + torch.tensor(geo["toffs"], dtype=torch.long).view(B, 1, 1, 1)) + torch.arange(T).view(1, T, 1, 1)
    return base + slot * sb + tt * st + torch.arange(Hkv).view(1, 1, Hkv, 1) * sh + torch.arange(D).view(1, 1, 1, D) * sd


def rope_expected(cs, t):
    """the whole qkv, K and V^T storages after the call (K None without a cache), starting from the pre-filled ones of `t`"""
    geo = t["geo"]
    Hq, Hkv, D = cs["Hq"], cs["Hkv"], cs["D"]
    q, k, v = rope_values(cs, t)
    qkv, kc, vt = t["qkv"].clone(), None if t["k"] is None else t["k"].clone(), t["vt"].clone()
    folded = cs["S"] > 0
    if geo["rows"]:
        view = qkv[cs["qkv_off"]:cs["qkv_off"] + geo["rows"] * geo["ld"]].view(geo["rows"], geo["ld"])
        if cs["mode"] != 0 or folded:                                             # q rotated (or folded) in place; mode 0 leaves the stored q alone
            view[:, :Hq * D] = q.reshape(geo["rows"], Hq * D)
        if kc is None:
            if cs["mode"] != 0 or folded:                                         # K stays in the qkv buffer, rotated in place
                view[:, Hq * D:(Hq + Hkv) * D] = k.reshape(geo["rows"], Hkv * D)
        else:
            ks, kt, kh = geo["k_strides"]
            kc[_cache_index(geo, cs, (ks, kt, kh, 1), cs["k_offset"]).reshape(-1)] = k.reshape(-1)
        vs, vh, vd = geo["vt_strides"]
        vt[_cache_index(geo, cs, (vs, 1, vh, vd), cs["vt_offset"]).reshape(-1)] = v.reshape(-1)
    return qkv, kc, vt


def rope_expected_naive(cs, t):
    """rope_expected as a loop over cells with scalar arithmetic (numpy fp32): the tiny-shape cross-check of the indexed version"""
    geo = t["geo"]
    Hq, Hkv, D, B, T = cs["Hq"], cs["Hkv"], cs["D"], cs["B"], cs["T"]
    half, ld = D // 2, geo["ld"]
    f32 = np.float32

    def r(v):
        return f32(torch.tensor(float(v), dtype=torch.float32).to(BF).float().item())

    cos, sin = (a.numpy() for a in rope_tables(D))
    qkv, kc, vt = t["qkv"].clone(), None if t["k"] is None else t["k"].clone(), t["vt"].clone()
    src = t["qkv"].float().numpy()
    for b, tk in itertools.product(range(B), range(T)):
        row = b * T + tk
        pos = tk if t["pos"] is None else int(t["pos"][row])
        pos = min(max(pos, 0), N_POS - 1)
        slot, tt = geo["slots"][b], cs["t_offset"] + geo["toffs"][b] + tk
        for hh in range(Hq + 2 * Hkv):
            def val(d):
                col = hh * D + d
                if cs["S"] <= 0:
                    return f32(src[cs["qkv_off"] + row * ld + col])
                acc = f32(0)
                for s in range(cs["S"]):
                    acc = f32(acc + f32(t["partial"][s, row, col].item()))
                if t["bias"] is not None:
                    acc = f32(acc + f32(t["bias"][col].item()))
                return r(acc)
            if hh >= Hq + Hkv:
                vs, vh, vd = geo["vt_strides"]
                for d in range(D):
                    vt[cs["vt_offset"] + slot * vs + (hh - Hq - Hkv) * vh + d * vd + tt] = float(val(d))
                continue
            out = np.zeros(D, dtype=np.float32)
            for i in range(half):
                x1, x2 = val(i), val(i + half)
                c, s = f32(cos[pos, i]), f32(sin[pos, i])
                if cs["mode"] == 0:
                    out[i], out[i + half] = x1, x2
                elif cs["mode"] == 2:
                    c, s = r(c), r(s)
                    out[i] = r(f32(r(f32(x1 * c)) + r(f32(-x2 * s))))
                    out[i + half] = r(f32(r(f32(x2 * c)) + r(f32(x1 * s))))
                else:
                    out[i] = r(f32(f32(x1 * c) - f32(x2 * s)))
                    out[i + half] = r(f32(f32(x2 * c) + f32(x1 * s)))
            if hh >= Hq and kc is not None:
                ks, kt, kh = geo["k_strides"]
                base = cs["k_offset"] + slot * ks + tt * kt + (hh - Hq) * kh
                kc[base:base + D] = torch.from_numpy(out).to(BF)
            elif cs["mode"] != 0 or cs["S"] > 0:
                base = cs["qkv_off"] + row * ld + hh * D
                qkv[base:base + D] = torch.from_numpy(out).to(BF)
    return qkv, kc, vt


def rope_logical(cs, t):
    """(q, K, V) read back by logical index from the storages of `t` (after a call): equal between two layouts of the same data"""
    geo = t["geo"]
    Hq, D = cs["Hq"], cs["D"]
    q = rope_views(cs, t)[0][:, :Hq * D].cpu()
    vs, vh, vd = geo["vt_strides"]
    v = t["vt"].cpu()[_cache_index(geo, cs, (vs, 1, vh, vd), cs["vt_offset"])]
    if t["k"] is None:
        k = rope_views(cs, t)[0][:, Hq * D:(Hq + cs["Hkv"]) * D].cpu().reshape(cs["B"], cs["T"], cs["Hkv"], D)
    else:
        ks, kt, kh = geo["k_strides"]
        k = t["k"].cpu()[_cache_index(geo, cs, (ks, kt, kh, 1), cs["k_offset"])]
    return q, k, v


ROPE_T = (1, 15, 16, 17, 63, 64, 65, 129)       # the path switch at 16; one / two / three token groups; a last group of one lane
ROPE_D = (36, 72, 64, 128, 256)                 # 36: not a multiple of 8 (scalar at any T); 72: token-group V + scalar q / k
ROPE_HEADS = ((3, 1), (4, 2), (2, 2))


def rope_sweep():
    """T x D x mode with the head geometry, batch, position form, optional arguments and layouts cycling through the cells"""
    out = []
    for i, (T, D, mode) in enumerate(itertools.product(ROPE_T, ROPE_D, (0, 1, 2))):
        out.append(rope_case(T, D, mode, heads=ROPE_HEADS[i % 3], B=(1, 3)[(i // 3) % 2], pos=("rand", "none", "clamp")[(i // 2) % 3],
                             kcache=(i % 4 != 3), slot=(i % 5 != 0), toff=(i % 7 != 0), ld_pad=(0, 16)[i % 2], cache_pad=bool((i // 2) % 2),
                             k_offset=(0, 24)[(i // 4) % 2], vt_offset=(0, 5)[(i // 3) % 2]))
    return out


def rope_named():
    """the cells the sweep's cycling could miss, each by name"""
    c = [
        rope_case(17, 64, 2, heads=(3, 1), B=1, tag="ragged68of16"),              # 68 q / k items, 16 per wave
        rope_case(17, 128, 1, heads=(3, 1), B=1, tag="ragged68of8"),              # 8 per wave
        rope_case(17, 256, 2, heads=(4, 2), B=1, tag="ragged102of4"),             # 4 per wave
        rope_case(24, 64, 1, kcache=False, B=3, tag="k_in_place"),
        rope_case(7, 64, 1, kcache=False, B=3, tag="k_in_place"),
        rope_case(24, 128, 0, kcache=False, B=3, ld_pad=16, tag="vit"),           # no q / k waves: q and k untouched
        rope_case(24, 64, 2, B=3, pos="none", slot=False, toff=False, tag="no_optionals"),
        rope_case(24, 64, 2, B=3, pos="clamp", slot=False, tag="no_slot"),
        rope_case(24, 64, 1, B=3, pos="clamp", toff=False, tag="no_toff"),
        rope_case(5, 64, 2, B=3, pos="none", slot=False, toff=False, tag="no_optionals"),
        rope_case(24, 64, 2, B=3, ld_pad=24, cache_pad=True, k_offset=40, vt_offset=11, tag="padded"),
        rope_case(5, 128, 1, B=3, ld_pad=3, cache_pad=True, k_offset=3, vt_offset=11, tag="padded"),
    ]
    return c


def rope_fallbacks():
    """(aligned case, [cases that differ only in one alignment]) at T = 24: same logical results, on the 2-byte paths by the kernel's own guards"""
    out = []
    for mode, D in ((1, 64), (2, 128)):
        base = dict(heads=(4, 2), B=3, pos="rand")
        out.append((rope_case(24, D, mode, tag="aligned", **base),
                    [rope_case(24, D, mode, qkv_off=4, tag="qkv_off4", **base), rope_case(24, D, mode, ld_pad=4, tag="ld_mod8", **base),
                     rope_case(24, D, mode, k_odd=True, tag="k_stride_mod8", **base), rope_case(24, D, mode, cs_off=1, tag="cossin_off1", **base)]))
    return out


def rope_folds():
    """S = 6: more slabs than the four that the fused decode launch holds in registers (its fold is compared with rope_kv_write's)"""
    many = [rope_case(1, 64, mode, heads=(4, 2), B=5, pos="clamp", S=6, bias=True, cache_pad=True, tag="fold_S6_bias") for mode in (0, 2)]
    return many + [rope_case(T, 64, mode, heads=(4, 2), B=B, pos="clamp", S=S, bias=bias, cache_pad=True, tag=f"fold_S{S}" + ("_bias" if bias else ""))
            for (T, B) in ((1, 5), (24, 2)) for mode in (0, 2) for S in (1, 3) for bias in (False, True)]


def rope_pairs():
    """(name, case 0, case 1): a T = 1 scalar group (25 waves) + a T = 24 vectorised group (6 + 8 = 14 waves), neither a multiple of the 4 waves of
    a block; both orders; and one group without rows"""
    dec = rope_case(1, 64, 2, heads=(3, 1), B=5, pos="rand", tag="decode_rows")
    pre = rope_case(24, 64, 2, heads=(3, 1), B=1, pos="none", tag="prefill_rows")
    empty = rope_case(24, 64, 2, heads=(3, 1), B=0, pos="none", slot=False, toff=False, tag="no_rows")
    return [("scalar+vec", dec, pre), ("vec+scalar", pre, dec), ("vec+empty", pre, empty), ("empty+scalar", empty, dec)]


def rope_waves(cs):
    """waves a case launches (rope_waves_host)"""
    B, T, Hq, Hkv, D = cs["B"], cs["T"], cs["Hq"], cs["Hkv"], cs["D"]
    path = rope_path(cs)
    if path == "scalar":
        return B * T * (Hq + 2 * Hkv)
    ipw = 64 // (D // 16) if path == "vtok_vecqk" else 1
    qk = 0 if path == "vtok_noqk" else -(-B * T * (Hq + Hkv) // ipw)
    return qk + B * Hkv * (D // 8) * ((T + 63) // 64)
