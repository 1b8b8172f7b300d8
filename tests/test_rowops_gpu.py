"""The bf16 row kernels of csrc/rowops.hip against tests/rowops_ref.py, at every dispatch path of rope_kv_write and the layouts and optional
arguments the models use.

Bit-exact kernels (RoPE + KV placement with its split-K fold and pair launch, gathers, copies, adds, casts, the Q8 twin of RMSNorm): every
output buffer is pre-filled with a non-zero sentinel and the WHOLE buffer is compared with the reference's whole buffer, so a store outside
the intended cells and a missing store both fail. A rope case's id starts with the device path it takes (rowops_ref.rope_path):
scalar | vtok_scalarqk | vtok_vecqk | vtok_noqk.

Rounded kernels (LayerNorm, RMSNorm, patchify) against float64: every element is bf16(ref64) or one of its two bf16 neighbours, and at most
1e-3 of a case's elements are not equal (rowops_ref.neighbour_check; test_rowops_cpu.py shows plain fp32 arithmetic meets it at every width
used here). Each case prints its share.
Largest share measured on an MI355X: 4.88e-04 (one element of a 1 x 2048 RMSNorm row); at 37 rows at most 2.6e-04 (LayerNorm and RMSNorm, every
width); patchify 0."""
import math

import pytest
import torch

from cover_vla_amd import ops
from cover_vla_amd._lib import CoverError
from tests import rowops_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _ids(cases):
    return [c["id"] for c in cases]


# ------------------------------------------------------------------------------------------------ rope_kv_write
def _rope_run(cs, dev, launch=True):
    """build, check the alignment rope_path assumed, launch; returns (cpu storages before, device storages)"""
    t = R.rope_build(cs)
    d = R.rope_to(t, dev)
    qkv, kw = R.rope_views(cs, d)
    assert d["qkv"].data_ptr() % 16 == 0 and d["cos"].data_ptr() % 16 == 0 and d["sin"].data_ptr() % 16 == 0
    assert d["k"] is None or d["k"].data_ptr() % 16 == 0
    assert kw["cos"].data_ptr() % 16 == (4 * cs["cs_off"]) % 16 and (qkv.numel() == 0 or qkv.data_ptr() % 16 == (2 * cs["qkv_off"]) % 16)
    if launch:
        ops.rope_kv_write(qkv, cs["B"], cs["T"], cs["Hq"], cs["Hkv"], cs["D"], **kw)
        torch.cuda.synchronize()
    return t, d


def _rope_assert(cs, t, d):
    want = R.rope_expected(cs, t)
    for name, w, got in zip(("qkv", "k_cache", "vt_cache"), want, (d["qkv"], d["k"], d["vt"])):
        if w is not None:
            assert R.same_bits(got, w), f"{cs['id']}: {name} differs from the reference ({int((R.bf_bits(got.cpu()) != R.bf_bits(w)).sum())} cells)"


ROPE_CASES = R.rope_sweep() + R.rope_named()


@pytest.mark.parametrize("cs", ROPE_CASES, ids=_ids(ROPE_CASES))
def test_rope_kv_write(dev, cs):
    t, d = _rope_run(cs, dev)
    _rope_assert(cs, t, d)


@pytest.mark.parametrize("aligned,others", R.rope_fallbacks(), ids=[a["id"] for a, _ in R.rope_fallbacks()])
def test_rope_kv_write_guarded_fallbacks_give_the_aligned_bits(dev, aligned, others):
    t0, d0 = _rope_run(aligned, dev)
    _rope_assert(aligned, t0, d0)
    base = R.rope_logical(aligned, d0)
    for cs in others:
        t, d = _rope_run(cs, dev)
        _rope_assert(cs, t, d)
        for a, b in zip(base, R.rope_logical(cs, d)):
            assert R.same_bits(a, b), cs["id"]


@pytest.mark.parametrize("cs", R.rope_folds(), ids=_ids(R.rope_folds()))
def test_rope_kv_write_split_fold(dev, cs):
    """values = bf16(((p0 + p1) + p2) + bias); q lands in the sentinel-filled qkv rotated (mode 0: as folded), K and V in the caches, and the k / v
    columns of qkv keep the sentinel"""
    assert R.rope_path(cs) == "scalar"
    t, d = _rope_run(cs, dev)
    _rope_assert(cs, t, d)
    q = R.rope_views(cs, d)[0][:, :cs["Hq"] * cs["D"]].cpu()
    assert not bool((R.bf_bits(q) == R.SENT_QKV).any())


@pytest.mark.parametrize("name,c0,c1", R.rope_pairs(), ids=[p[0] for p in R.rope_pairs()])
def test_rope_kv_write_pair(dev, name, c0, c1):
    singles = [_rope_run(c, dev) for c in (c0, c1)]
    pairs = [_rope_run(c, dev, launch=False) for c in (c0, c1)]
    args = []
    for c, (_, d) in zip((c0, c1), pairs):
        qkv, kw = R.rope_views(c, d)
        args.append(ops.rope_args(qkv, c["B"], c["T"], c["Hq"], c["Hkv"], c["D"], **kw))
    ops.rope_kv_write_pair(args[0], args[1])
    torch.cuda.synchronize()
    for c, (t, d), (_, ds) in zip((c0, c1), pairs, singles):
        _rope_assert(c, t, d)
        for key in ("qkv", "k", "vt"):
            assert R.same_bits(d[key], ds[key]), f"{name}: {key} of {c['id']} differs from the single launch"


# ------------------------------------------------------------------------------------------------ other bit-exact kernels
def _padded(rows, cols, ld, dev, values=None, off=0, pattern=R.SENT_OUT):
    """(storage, [rows, cols] view with row stride ld starting `off` elements in); one guard row more"""
    store = R.sentinel_bf16(off + (rows + 1) * ld, pattern)
    view = store[off:off + rows * ld].view(rows, ld)[:, :cols]
    if values is not None:
        view.copy_(values)
    store = store.to(dev)
    return store, store[off:off + rows * ld].view(rows, ld)[:, :cols]


def _expect(store_before, rows, cols, ld, values, off=0):
    want = store_before.clone()
    want[off:off + rows * ld].view(rows, ld)[:, :cols] = values
    return want


@pytest.mark.parametrize("pad", [0, 24])
@pytest.mark.parametrize("scale", ["one", "sqrt_dim"])
@pytest.mark.parametrize("dim", [8, 136, 2048, 4104])
def test_embed_gather(dev, dim, scale, pad):
    g = torch.Generator().manual_seed(dim)
    table = torch.randn(50, dim, generator=g).to(BF)
    ids = torch.tensor([0, 49, 7, 7, 49, 0, 23, 7, 1])
    sc = 1.0 if scale == "one" else math.sqrt(dim)
    store, out = _padded(len(ids), dim, dim + pad, dev)
    before = store.cpu()
    ops.embed_gather(table.to(dev), ids.to(dev), sc, out=out)
    assert R.same_bits(store, _expect(before, len(ids), dim, dim + pad, R.embed_gather_ref(table, ids, sc)))


@pytest.mark.parametrize("idx", ["none", "src", "dst", "both"])
@pytest.mark.parametrize("cols,off", [(64, 0), (60, 0), (64, 4)], ids=["vec16", "cols60", "src_off4"])
def test_copy_rows(dev, cols, off, idx):
    g = torch.Generator().manual_seed(cols + off)
    n_src, n_dst, rows = 9, 8, 5
    src = torch.randn(n_src, cols, generator=g).to(BF)
    s_store, s_view = _padded(n_src, cols, cols + 8, dev, src, off=off, pattern=R.SENT_QKV)
    d_store, d_view = _padded(n_dst, cols, cols + 16, dev)
    assert s_view.data_ptr() % 16 == (2 * off) % 16 and d_view.data_ptr() % 16 == 0
    si = [3, 1, 3, 8, 0] if idx in ("src", "both") else None
    di = [7, 0, 2, 5, 3] if idx in ("dst", "both") else None
    before = d_store.cpu()
    ops.copy_rows(s_view, d_view, rows, cols, None if si is None else torch.tensor(si, dtype=torch.int32, device=dev),
                  None if di is None else torch.tensor(di, dtype=torch.int32, device=dev))
    dst0 = before[:n_dst * (cols + 16)].view(n_dst, cols + 16)[:, :cols]
    assert R.same_bits(d_store, _expect(before, n_dst, cols, cols + 16, R.copy_rows_ref(src, dst0, rows, cols, si, di)))


@pytest.mark.parametrize("add_rows", [1, 3, 7])
@pytest.mark.parametrize("cols", [1, 255, 257, 1152])
def test_add_rows(dev, cols, add_rows):
    g = torch.Generator().manual_seed(cols + add_rows)
    x, add = torch.randn(7, cols, generator=g).to(BF), torch.randn(add_rows, cols, generator=g).to(BF)
    x_store, x_view = _padded(7, cols, cols + 3, dev, x)
    a_store, a_view = _padded(add_rows, cols, cols + 5, dev, add, pattern=R.SENT_QKV)
    before = x_store.cpu()
    ops.add_rows(x_view, a_view)
    assert R.same_bits(x_store, _expect(before, 7, cols, cols + 3, R.add_rows_ref(x, add)))


@pytest.mark.parametrize("pre_div", [1.0, 8.0])
def test_scale_bf16(dev, pre_div):
    x = torch.randn(5, 257, generator=torch.Generator().manual_seed(2)).to(BF)
    store, view = _padded(5, 257, 260, dev, x)
    before = store.cpu()
    ops.scale_bf16(view, pre_div, 3.0)
    assert R.same_bits(store, _expect(before, 5, 257, 260, R.scale_ref(x, pre_div, 3.0)))


@pytest.mark.parametrize("cols", [1, 255, 257])
def test_casts(dev, cols):
    g = torch.Generator().manual_seed(cols)
    sp = R.special_f32_row()
    reps = -(-cols // sp.numel())
    f = torch.randn(4, cols, generator=g)
    f[1] = sp.repeat(reps)[:cols]
    if cols == 1:
        f = torch.cat([f, sp[:, None]])
    rows = f.shape[0]
    fin = torch.full((rows + 1, cols + 3), 5.0)
    fin[:rows, :cols] = f
    fin = fin.to(dev)
    store, out = _padded(rows, cols, cols + 5, dev)
    before = store.cpu()
    ops.cast_f32_to_bf16(fin[:rows, :cols], out=out)
    want = R.cast_f32_to_bf16_ref(f)
    got = out.cpu()
    nan = want.float().isnan()
    assert torch.equal(got.float().isnan(), nan) and int(nan.sum()) >= 1
    assert R.same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))
    keep = store.cpu().clone()
    keep[:rows * (cols + 5)].view(rows, cols + 5)[:, :cols] = before[0]
    assert R.same_bits(keep, before), "bytes outside the output changed"
    # and back: every bf16 pattern of the row above, specials included, widens exactly
    b_store, b_view = _padded(rows, cols, cols + 5, dev, want, pattern=R.SENT_QKV)
    fout = torch.full((rows + 1, cols + 3), 5.0, device=dev)
    ops.cast_bf16_to_f32(b_view, out=fout[:rows, :cols])
    wantf = torch.full((rows + 1, cols + 3), 5.0)
    wantf[:rows, :cols] = R.cast_bf16_to_f32_ref(want)
    gotf = fout.cpu()
    assert torch.equal(gotf.isnan(), wantf.isnan())
    assert torch.equal(gotf.nan_to_num(0.0).view(torch.int32), wantf.nan_to_num(0.0).view(torch.int32))


# ------------------------------------------------------------------------------------------------ Q8 RMSNorm
@pytest.mark.parametrize("ld8_pad", [0, 128])
@pytest.mark.parametrize("style", [0, 1])
@pytest.mark.parametrize("in_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("dim", R.Q8_DIMS)
def test_rmsnorm_q8(dev, dim, in_f32, style, ld8_pad):
    x, w, off = R.q8_inputs(dim, style)
    xd = (x if in_f32 else x.to(BF)).to(dev)
    rows, ld8 = x.shape[0], dim + ld8_pad
    plain = ops.rmsnorm(xd, w.to(dev), 1e-6, w_offset=off, style=style)
    q = torch.full((rows + 1, ld8), R.SENT_Q8, dtype=torch.uint8, device=dev)
    qs = torch.full((rows + 1,), -7.0, device=dev)
    y, q_out, qs_out = ops.rmsnorm(xd, w.to(dev), 1e-6, w_offset=off, style=style, q8=(q[:rows], qs[:rows]))
    assert R.same_bits(y, plain)
    yc = y.cpu()
    assert yc[2].float().abs().max() == 14.0 and not yc[1].any()                  # the boundary row and the zero row are what they claim
    want_q, want_s = R.quantize_rows_e4m3_ref(yc)
    assert torch.equal(qs.cpu()[:rows], want_s) and qs.cpu()[rows] == -7.0 and want_s[2] == 2.0 ** -5 and want_s[1] == 1.0
    got = q.cpu()
    assert bool((got[rows] == R.SENT_Q8).all()) and bool((got[:rows, dim:] == R.SENT_Q8).all()), "bytes beyond dim changed"
    lib_q, lib_s = ops.quantize_act_fp8(y)
    for other in (want_q, lib_q.cpu()[:, :dim]):
        assert torch.equal(got[:rows, :dim].view(torch.float8_e4m3fn).float(), other.view(torch.float8_e4m3fn).float())
        nz = (other & 0x7F) != 0                                                  # +0 / -0 may differ in sign only
        assert torch.equal(got[:rows, :dim][nz], other[nz])
    assert torch.equal(lib_s.cpu(), want_s)


def test_rmsnorm_q8_refuses_bad_geometry(dev):
    def call(dim, ld8):
        x = torch.zeros(2, dim, dtype=BF, device=dev)
        q = torch.full((2, max(ld8, 16)), R.SENT_Q8, dtype=torch.uint8, device=dev)
        out = R.sentinel_bf16(2 * dim, R.SENT_OUT, dev).view(2, dim)
        with pytest.raises(CoverError):
            ops.rmsnorm(x, None, 1e-6, out=out, q8=(q.as_strided((2, min(ld8, dim)), (ld8, 1)), torch.zeros(2, device=dev)))
        torch.cuda.synchronize()
        assert bool((R.bf_bits(out.cpu()) == R.SENT_OUT).all()) and bool((q.cpu() == R.SENT_Q8).all())
    call(192, 256)          # dim % 128
    call(256, 128)          # ld8 < dim
    call(256, 264)          # ld8 % 16


# ------------------------------------------------------------------------------------------------ rounded kernels
def _rule(got, lo, hi, what):
    ok, share = R.neighbour_check(got, lo, hi)
    print(f"{what}: share of elements not equal to bf16(ref64) = {share:.2e}")
    assert ok, f"{what}: an element is further than one bf16 step from the reference"
    assert share <= R.NEIGHBOUR_CAP, f"{what}: share {share:.2e}"


def _norm_io(x, dim, rows, dev, layout, dtype):
    """x on the device as `layout` says: dense | a column slice (8 elements in, ld = dim + 64); the output padded by 24 columns of sentinel"""
    xs = x.to(dtype)
    if layout == "slice":
        buf = torch.full((rows + 1, dim + 64), 9.0, dtype=dtype)
        buf[:rows, 8:8 + dim] = xs
        xin = buf.to(dev)[:rows, 8:8 + dim]
    else:
        xin = xs.to(dev)
    store, out = _padded(rows, dim, dim + 24, dev)
    return xs, xin, store, out


@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("rows", R.NORM_ROWS)
@pytest.mark.parametrize("dim", R.NORM_DIMS)
def test_layernorm(dev, dim, rows, kind, layout):
    x, w, b = R.norm_inputs(rows, dim, kind)
    for bias in (b, None):
        xs, xin, store, out = _norm_io(x, dim, rows, dev, layout, BF)
        before = store.cpu()
        ops.layernorm(xin, w.to(dev), None if bias is None else bias.to(dev), 1e-6, out=out)
        got = out.cpu()
        assert R.same_bits(store, _expect(before, rows, dim, dim + 24, got)), "bytes outside the output changed"
        _rule(got, *R.layernorm_bounds64(xs, w, bias, 1e-6), f"layernorm {rows}x{dim} {kind} {layout} b={bias is not None}")
        if kind == "plain" and rows > 1:                                          # the zero row: exactly b
            assert torch.equal(got[0].float(), (torch.zeros(dim) if bias is None else bias).to(BF).float())
        inplace = xs.clone().to(dev)
        ops.layernorm(inplace, w.to(dev), None if bias is None else bias.to(dev), 1e-6, out=inplace)
        assert R.same_bits(inplace, got)


@pytest.mark.parametrize("layout", ["dense", "slice"])
@pytest.mark.parametrize("kind", ["plain", "offset"])
@pytest.mark.parametrize("rows", R.NORM_ROWS)
@pytest.mark.parametrize("dim", R.NORM_DIMS)
def test_rmsnorm(dev, dim, rows, kind, layout):
    x, w, _ = R.norm_inputs(rows, dim, kind)
    for dtype in (BF, torch.float32):
        for style, off, ww in ((0, 1.0, w), (1, 0.0, w), (0, 1.0, None)):
            xs, xin, store, out = _norm_io(x, dim, rows, dev, layout, dtype)
            before = store.cpu()
            ops.rmsnorm(xin, None if ww is None else ww.to(dev), 1e-6, w_offset=off, style=style, out=out)
            got = out.cpu()
            assert R.same_bits(store, _expect(before, rows, dim, dim + 24, got)), "bytes outside the output changed"
            _rule(got, *R.rmsnorm_bounds64(xs, ww, 1e-6, off, style), f"rmsnorm style {style} {rows}x{dim} {kind} {layout} {dtype} w={ww is not None}")
            if kind == "plain" and rows > 1:
                assert not got[0].any()
            if dtype == BF:                                                       # the decoder's final norm runs in place
                inplace = xs.clone().to(dev)
                ops.rmsnorm(inplace, None if ww is None else ww.to(dev), 1e-6, w_offset=off, style=style, out=inplace)
                assert R.same_bits(inplace, got)


def test_norms_and_gather_refuse_what_they_cannot_run(dev):
    """widths outside the register-cached row, and bases / strides that would put a 16-byte access off alignment: invalid value, nothing written"""
    w = torch.ones(8200, device=dev)

    def refused(fn):
        with pytest.raises(CoverError):
            fn()
        torch.cuda.synchronize()

    for dim in (12, 8200):
        x = torch.zeros(2, dim, dtype=BF, device=dev)
        out = R.sentinel_bf16(2 * dim, R.SENT_OUT, dev).view(2, dim)
        refused(lambda: ops.layernorm(x, w, None, 1e-6, out=out))
        refused(lambda: ops.rmsnorm(x, w, 1e-6, out=out))
        refused(lambda: ops.rmsnorm(x.float(), w, 1e-6, out=out))
        assert bool((R.bf_bits(out.cpu()) == R.SENT_OUT).all())
    dim = 64
    flat = torch.zeros(4 * (dim + 16), dtype=BF, device=dev)
    flat32 = torch.zeros(4 * (dim + 16), device=dev)
    good = flat[:2 * dim].view(2, dim)
    off4 = flat[4:4 + 2 * dim].view(2, dim)                                       # 8 bytes off
    ld_odd = flat[:2 * (dim + 4)].view(2, dim + 4)[:, :dim]                       # rows 8 bytes apart from 16-byte alignment
    f32_off2 = flat32[2:2 + 2 * dim].view(2, dim)
    f32_ld_odd = flat32[:2 * (dim + 2)].view(2, dim + 2)[:, :dim]
    store = R.sentinel_bf16(4 * (dim + 16), R.SENT_OUT, dev)
    out = store[:2 * dim].view(2, dim)
    out_off4, out_ld_odd = store[4:4 + 2 * dim].view(2, dim), store[:2 * (dim + 4)].view(2, dim + 4)[:, :dim]
    for bad in (off4, ld_odd):
        refused(lambda: ops.layernorm(bad, w, None, 1e-6, out=out))
        refused(lambda: ops.rmsnorm(bad, w, 1e-6, out=out))
    for bad in (f32_off2, f32_ld_odd):
        refused(lambda: ops.rmsnorm(bad, w, 1e-6, out=out))
    for bad_out in (out_off4, out_ld_odd):
        refused(lambda: ops.layernorm(good, w, None, 1e-6, out=bad_out))
        refused(lambda: ops.rmsnorm(good, w, 1e-6, out=bad_out))
        refused(lambda: ops.embed_gather(good, torch.zeros(2, dtype=torch.int64, device=dev), 1.0, out=bad_out))
    refused(lambda: ops.embed_gather(flat[4:4 + 2 * dim].view(2, dim), torch.zeros(2, dtype=torch.int64, device=dev), 1.0, out=out))
    refused(lambda: ops.embed_gather(flat[:24].view(2, 12), torch.zeros(2, dtype=torch.int64, device=dev), 1.0, out=out))
    assert bool((R.bf_bits(store.cpu()) == R.SENT_OUT).all())
    ops.rmsnorm(flat32[4:4 + 2 * dim].view(2, dim), w, 1e-6, out=out)              # fp32 rows need 16 bytes too: 4 floats in is fine
    assert not bool((R.bf_bits(out.cpu()) == R.SENT_OUT).any())


@pytest.mark.parametrize("pad", [0, 40])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("patch,hw", R.PATCH_CASES)
def test_patchify(dev, patch, hw, kind, pad):
    img = R.patch_image(kind, hw)
    kk = 3 * patch * patch
    rows = 3 * (hw[0] // patch) * (hw[1] // patch)
    if hw[0] % patch or hw[1] % patch:                                            # the C entry refuses sizes that are no multiple of the patch
        with pytest.raises(CoverError):
            ops.patchify(img.to(dev), patch, R.PATCH_MUL, R.PATCH_ADD, kk + pad)
        return
    store = R.sentinel_bf16((rows + 1) * (kk + pad), R.SENT_OUT, dev)
    out = store[:rows * (kk + pad)].view(rows, kk + pad)
    ops.patchify(img.to(dev), patch, R.PATCH_MUL, R.PATCH_ADD, kk + pad, out=out)
    got = out.cpu()
    assert bool((R.bf_bits(store.cpu()[rows * (kk + pad):]) == R.SENT_OUT).all())
    assert not got[:, kk:].any()
    ref = R.patchify_ref64(img, patch, R.PATCH_MUL, R.PATCH_ADD, kk + pad)
    _rule(got, ref, None, f"patchify p{patch} {hw[0]}x{hw[1]} {kind} ld+{pad}")
