"""The fp32 kernels of csrc/f32ops.hip against float64 references (tests/f32_ref.py), at every dispatch path of the GEMM, with the operand
layouts and batch / residual / bias arguments the verifier and pi0 callers use, and the row kernels at ragged widths with padded strides.
Unless a test says otherwise the rule is test_kernels_gpu.py's for fp32 kernels: atol and rtol 2e-5 against float64. Output buffers are
pre-filled with a NaN bit pattern and every byte outside the result must still hold it afterwards.

test_f32ops_cpu.py shows, without a GPU, which kernel each GEMM case runs on and that the bounds asserted here hold for plain CPU fp32."""
import pytest
import torch

from cover_vla_amd import ops
from cover_vla_amd._lib import CoverError
from tests import f32_ref as R

pytestmark = pytest.mark.gpu
TOL = dict(atol=2e-5, rtol=2e-5)
CASES = R.gemm_cases()


def close64(got, ref, **tol):
    return torch.allclose(got.detach().cpu().double(), ref, **(tol or TOL), equal_nan=True)


# ------------------------------------------------------------------------------------------------ GEMM
def _run_gemm(cs, kind, act, alpha, dev, expect_plan=None):
    t = R.gemm_build(cs, kind, dev)
    res_before = None if t["res"] is None else t["res"].clone()
    args, kw = R.gemm_plan_args(cs, (t["a"].data_ptr(), t["b"].data_ptr(), t["out"].data_ptr()))
    ran_on = ops.gemm_f32_plan(*args, **kw)[0]
    if expect_plan is not None:
        assert ran_on == expect_plan      # the kernel the CPU table says this case covers is the one the real pointers dispatch to
    ops.gemm_f32(t["a"], t["b"], **R.gemm_call_kwargs(cs, t, act, alpha))
    torch.cuda.synchronize()
    assert R.outside_untouched(t, cs), "bytes outside [M, N] changed"
    return t, R.gemm_ref64(cs, t, act, alpha, res_before), res_before, ran_on


@pytest.mark.parametrize("cs", CASES, ids=[cs["id"] for cs in CASES])
def test_gemm_f32_exact(dev, cs, monkeypatch):
    """Integer operands: every product and partial sum is exactly representable, so the result equals the float64 reference bit for bit
    whatever the summation order or k-to-lane map: a dropped, doubled or misplaced k term, row, column, bias or residual is an integer
    difference. Directly dispatched cases run again on the tiled kernel (COVER_F32_DIRECT_MAX=0): same bits."""
    act, alpha = R.exact_epilogue(cs)
    args, kw = R.gemm_plan_args(cs)
    table_plan = ops.gemm_f32_plan(*args, **kw)[0]
    t, ref, _, _ = _run_gemm(cs, "exact", act, alpha, dev, expect_plan=table_plan)
    first = t["out"].cpu()
    assert torch.equal(first.double(), ref)
    if table_plan.startswith("DIRECT"):
        monkeypatch.setenv("COVER_F32_DIRECT_MAX", "0")
        t2, ref2, _, ran_on = _run_gemm(cs, "exact", act, alpha, dev)
        assert ran_on.startswith("TILE")
        assert torch.equal(t2["out"].cpu(), first) and torch.equal(ref2, ref)


@pytest.mark.parametrize("cs", CASES, ids=[cs["id"] for cs in CASES])
def test_gemm_f32_bounded(dev, cs):
    """Normal operands, the case's activation and alpha, per element inside the forward-error bound of a length-K fp32 dot product in any
    order (f32_ref.gemm_bound: derived from the kernels, not from their output)."""
    t, ref, res_before, _ = _run_gemm(cs, "bounded", cs["act"], cs["alpha"], dev)
    err = (t["out"].cpu().double() - ref).abs()
    bound = R.gemm_bound(cs, t, cs["act"], cs["alpha"], res_before)
    worst = (err / bound).max().item()
    print(f"{cs['id']}: max err / bound = {worst:.3f}, max err = {err.max().item():.3e}")
    assert bool((err <= bound).all()), worst


def test_gemm_f32_raw_forwards_the_bias_batch_stride(dev):
    g = torch.Generator().manual_seed(11)
    nb, M, N, K = 3, 5, 33, 64
    a, w, bias = (torch.randint(-4, 5, s, generator=g).float().to(dev) for s in ((nb, M, K), (nb, N, K), (nb, N)))
    out = R.nan_filled(nb * M * N, dev).view(nb, M, N)
    ops.gemm_f32_raw(a.data_ptr(), K, 1, w.data_ptr(), K, 1, out.data_ptr(), N, M, N, K, bias=bias, batch=nb, a_bs=M * K, b_bs=N * K,
                     c_bs=M * N, bias_bs=N)
    assert torch.equal(out.cpu().double(), a.cpu().double() @ w.cpu().double().transpose(1, 2) + bias.cpu().double()[:, None])


# ------------------------------------------------------------------------------------------------ mha_f32
def _pad_pattern(name, B, Tk):
    if name == "none":
        return None
    pad = torch.zeros(B, Tk, dtype=torch.bool)
    if name == "prefix":
        pad[0, :Tk // 2] = True
        pad[-1, :max(Tk - 2, 0)] = True
    elif name == "all_but_one":
        pad[:, :Tk - 1] = True
    elif name == "one_batch_masked":
        pad[B - 1] = True
        pad[0, :Tk // 3] = True
    return pad


def _mha(dev, shape, layout, pad_name, q_scale=1.0, grid=None):
    B, Tq, Tk, H, Dh = shape
    E = H * Dh
    g = torch.Generator().manual_seed(sum(shape))
    rnd = (lambda *s: torch.randn(*s, generator=g)) if grid is None else (lambda *s: torch.round(torch.randn(*s, generator=g) * grid) / grid)
    if layout == "packed" and Tq == Tk:           # self-attention over one [B*T, 3E] projection (verifier.py, the trajectory encoder)
        qkv = rnd(B * Tq, 3 * E)
        qkv[:, :E] *= q_scale
        d = qkv.to(dev)
        q, k, v = d, d[:, E:], d[:, 2 * E:]
        qs = ks = vs = (Tq * 3 * E, 3 * E)
        qc, kc, vc = (qkv[:, i * E:(i + 1) * E].reshape(B, Tq, E) for i in range(3))
    elif layout == "packed":                      # cross-attention: k / v are column slices of one [B, Tk, 2E] projection (the pooling heads)
        qc, kv = rnd(B, Tq, E) * q_scale, rnd(B, Tk, 2 * E)
        d = kv.to(dev)
        q, k, v = qc.to(dev), d, d[:, :, E:]
        qs, ks, vs = (Tq * E, E), (Tk * 2 * E, 2 * E), (Tk * 2 * E, 2 * E)
        kc, vc = kv[:, :, :E], kv[:, :, E:]
    else:
        qc, kc, vc = rnd(B, Tq, E) * q_scale, rnd(B, Tk, E), rnd(B, Tk, E)
        q, k, v = qc.to(dev), kc.to(dev), vc.to(dev)
        qs, ks, vs = (Tq * E, E), (Tk * E, E), (Tk * E, E)
        if layout == "q_offset1":                 # a base one element off 16-byte alignment: the scalar score loop
            store = torch.zeros(B * Tq * E + 1)
            store[1:] = qc.reshape(-1)
            q = store.to(dev)[1:]
            assert q.data_ptr() % 16 == 4
    pad = _pad_pattern(pad_name, B, Tk)
    ldo, rows = E + 3, Tq + 1                     # padded output strides with guard columns and a guard row per batch
    store = R.nan_filled(B * rows * ldo, dev)
    out = store.view(B, rows, ldo)[:, :Tq, :E]
    ops.mha_f32(q, k, v, B, Tq, Tk, H, Dh, qs, ks, vs, key_pad=None if pad is None else pad.to(torch.uint8).to(dev), out=out,
                o_strides=(rows * ldo, ldo))
    torch.cuda.synchronize()
    mask = torch.zeros(B, rows, ldo, dtype=torch.bool)
    mask[:, :Tq, :E] = True
    assert bool((R.bits(store.cpu())[~mask.view(-1)] == R.NAN_BITS).all()), "bytes outside the output changed"
    return out.cpu(), R.mha_ref64(qc, kc, vc, H, Dh, pad), pad


@pytest.mark.parametrize("pad_name", ["none", "prefix", "all_but_one", "one_batch_masked"])
@pytest.mark.parametrize("layout", ["separate", "packed", "q_offset1"])
@pytest.mark.parametrize("shape", R.MHA_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mha_f32(dev, shape, layout, pad_name):
    got, ref, pad = _mha(dev, shape, layout, pad_name)
    if pad_name == "one_batch_masked":            # NaN exactly on the fully masked batch's rows; every other row is still right
        assert got[-1].isnan().all() and ref[-1].isnan().all()
        assert not got[:-1].isnan().any()
    else:
        assert not got.isnan().any()
    assert close64(got, ref)


def test_mha_f32_large_scores_need_the_stabilised_softmax(dev):
    """q scaled by 30 on a 1/8 grid with Dh = 16 (scale 1/4): every score is exactly representable and reaches far beyond +-88, where an
    unstabilised fp32 exp overflows; the probabilities then follow the float64 softmax at the usual tolerance."""
    got, ref, _ = _mha(dev, (2, 90, 91, 2, 16), "separate", "prefix", q_scale=30.0, grid=8.0)
    assert not got.isnan().any() and close64(got, ref)


def test_mha_f32_refuses_more_than_8192_scores(dev):
    B, Tq, Tk, H, Dh = 1, 1, 8193, 2, 8
    q, k = torch.randn(B, Tq, H * Dh).to(dev), torch.randn(B, Tk, H * Dh).to(dev)
    out = R.nan_filled(B * Tq * H * Dh, dev).view(B, Tq, H * Dh)
    with pytest.raises(CoverError):
        ops.mha_f32(q, k, k, B, Tq, Tk, H, Dh, (Tq * H * Dh, H * Dh), (Tk * H * Dh, H * Dh), (Tk * H * Dh, H * Dh), out=out,
                    o_strides=(Tq * H * Dh, H * Dh))
    torch.cuda.synchronize()
    assert bool((R.bits(out.cpu()) == R.NAN_BITS).all())
    ops.mha_f32(q, k[:, :8192], k[:, :8192], B, Tq, 8192, H, Dh, (Tq * H * Dh, H * Dh), (Tk * H * Dh, H * Dh), (Tk * H * Dh, H * Dh), out=out,
                o_strides=(Tq * H * Dh, H * Dh))
    assert close64(out, R.mha_ref64(q.cpu(), k[:, :8192].cpu(), k[:, :8192].cpu(), H, Dh))


# ------------------------------------------------------------------------------------------------ row kernels
ROWS_COLS = [(r, c) for r in R.ROW_COUNTS for c in R.ROW_WIDTHS]


class Padded:
    """a [rows, cols] view with row stride cols + 3 inside a NaN-patterned storage that carries one more row: reading outside a row poisons
    the result, writing outside it shows in `guards_ok`"""

    def __init__(self, rows, cols, dev, values=None, dtype=torch.float32):
        self.rows, self.cols, self.ld = rows, cols, cols + 3
        if dtype == torch.float32:
            self.store = R.nan_filled((rows + 1) * self.ld, dev)
        else:
            self.store = torch.full(((rows + 1) * self.ld,), 0x7FC1, dtype=torch.int16).view(dtype).to(dev)
        self.pattern = self.store[:1].clone()
        self.view = self.store.view(rows + 1, self.ld)[:rows, :cols]
        if values is not None:
            self.view.copy_(values.to(dev))

    def guards_ok(self):
        as_int = lambda t: t.cpu().view(torch.int32 if t.dtype == torch.float32 else torch.int16)   # noqa: E731
        mask = torch.zeros(self.rows + 1, self.ld, dtype=torch.bool)
        mask[:self.rows, :self.cols] = True
        return bool((as_int(self.store)[~mask.view(-1)] == as_int(self.pattern)).all())


def _gen(rows, cols, salt=0):
    return torch.Generator().manual_seed(rows * 100003 + cols * 17 + salt)


@pytest.mark.parametrize("affine", ["wb", "w_only", "b_only", "neither"])
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_layernorm_f32(dev, rows, cols, affine):
    g = _gen(rows, cols)
    x, w, b = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    w = w if affine in ("wb", "w_only") else None
    b = b if affine in ("wb", "b_only") else None
    xin, out = Padded(rows, cols, dev, x), Padded(rows, cols, dev)
    ops.layernorm_f32(xin.view, None if w is None else w.to(dev), None if b is None else b.to(dev), out=out.view)
    assert out.guards_ok() and xin.guards_ok()
    assert close64(out.view, R.layernorm_ref64(x, w, b))
    # a constant row has zero deviations: the output is exactly b
    const = Padded(rows, cols, dev, torch.full((rows, cols), 3.25))
    ops.layernorm_f32(const.view, None if w is None else w.to(dev), None if b is None else b.to(dev), out=out.view)
    assert torch.equal(out.view.cpu(), (torch.zeros(cols) if b is None else b).expand(rows, cols)) and out.guards_ok()


def test_layernorm_f32_rows_with_a_large_common_offset(dev):
    """rows = N(0, 1) + 100: the two-pass scheme's fp32 mean is off by ~2 * 2^-24 * max|x|, which moves every output by that over sigma;
    tolerance = 2e-5 + 2 * 2^-24 * max|x| / sigma * max|w| (f32_ref.layernorm_offset_atol; the CPU test holds a numpy fp32 restatement of
    the kernel's summation order to the same figure)"""
    rows, cols = 9, 1000
    g = _gen(rows, cols, 1)
    x, w, b = torch.randn(rows, cols, generator=g) + 100.0, torch.randn(cols, generator=g), torch.randn(cols, generator=g)
    xin, out = Padded(rows, cols, dev, x), Padded(rows, cols, dev)
    ops.layernorm_f32(xin.view, w.to(dev), b.to(dev), out=out.view)
    atol = R.layernorm_offset_atol(x, w)
    ref = R.layernorm_ref64(x, w, b)
    print(f"offset rows: max err {(out.view.cpu().double() - ref).abs().max().item():.3e}, atol {atol:.3e}")
    assert out.guards_ok() and close64(out.view, ref, atol=atol, rtol=2e-5)


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("rpg", [1, 7])
@pytest.mark.parametrize("cols", R.ROW_WIDTHS)
def test_layernorm_f32_grouped(dev, cols, rpg, with_b):
    G = 3
    g = _gen(rpg, cols, 2)
    x, w, b = torch.randn(G * rpg, cols, generator=g), torch.randn(G, cols, generator=g), torch.randn(G, cols, generator=g)
    xin, out = Padded(G * rpg, cols, dev, x), Padded(G * rpg, cols, dev)
    wp, bp = Padded(G, cols, dev, w), Padded(G, cols, dev, b)         # parameter stride > dim (w and b share it)
    ops.layernorm_f32_grouped(xin.view, wp.view, bp.view if with_b else None, rpg, out=out.view)
    ref = torch.cat([R.layernorm_ref64(x[i * rpg:(i + 1) * rpg], w[i], b[i] if with_b else None) for i in range(G)])
    assert out.guards_ok() and close64(out.view, ref)


@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_softmax_rows_f32(dev, rows, cols):
    g = _gen(rows, cols, 3)
    x = (torch.rand(rows, cols, generator=g) * 2 - 1) * 30 * 0.07     # x / 0.07 reaches +-30
    x[0, 0] = 30 * 0.07
    if cols > 1:
        x[rows - 1, cols // 2] = float("-inf")
    p = Padded(rows, cols, dev, x)
    scale = 1 / 0.07
    ops.softmax_rows_f32(p.view, scale)
    ref = torch.softmax(x.double() * torch.tensor(scale, dtype=torch.float32).double(), -1)
    got = p.view.cpu()
    assert p.guards_ok() and close64(got, ref)
    assert bool(((got.double().sum(-1) - 1).abs() < 1e-6).all())
    if cols > 1:
        assert got[rows - 1, cols // 2].item() == 0.0


@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_l2norm_rows_f32(dev, rows, cols):
    x = torch.randn(rows, cols, generator=_gen(rows, cols, 4))
    if rows > 1:
        x[rows // 2] = 0.0                                           # a zero row: 0 / 0 = NaN, as x / x.norm() gives
    xin, out = Padded(rows, cols, dev, x), Padded(rows, cols, dev)
    ops.l2norm_rows_f32(xin.view, out=out.view)
    ref = x.double() / x.double().norm(dim=-1, keepdim=True)
    got = out.view.cpu()
    assert torch.equal(got.isnan(), ref.isnan()) and int(got.isnan().sum()) == (cols if rows > 1 else 0)
    assert out.guards_ok() and close64(got, ref)


@pytest.mark.parametrize("b_rows", [1, 3, "rows"])
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_add_f32(dev, rows, cols, b_rows):
    b_rows = rows if b_rows == "rows" else b_rows
    g = _gen(rows, cols, 5)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(b_rows, cols, generator=g)
    ap, bp, out = Padded(rows, cols, dev, a), Padded(b_rows, cols, dev, b), Padded(rows, cols, dev)
    ops.add_f32(ap.view, bp.view, out=out.view)
    assert out.guards_ok() and torch.equal(out.view.cpu(), a + b[torch.arange(rows) % b_rows])


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("rows,cols", ROWS_COLS)
def test_act_f32(dev, rows, cols, act):
    x = torch.randn(rows, cols, generator=_gen(rows, cols, 6)) * 3
    special = torch.tensor([0.0, -0.0, 20.0, -20.0, 1e4, -1e4])
    n = min(cols, 6)
    x[0, :n] = special[:n]
    if cols == 1 and rows > 6:
        x[:6, 0] = special
    xin, out = Padded(rows, cols, dev, x), Padded(rows, cols, dev)
    ops.act_f32(xin.view, act, out=out.view)
    assert out.guards_ok() and close64(out.view, R.ACT64[act](x.double()))
    if act in ("none", "relu"):
        assert torch.equal(out.view.cpu(), R.ACT64[act](x))


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 3), (3, 3), (9, 255), (9, 257), (256, 256), (257, 257), (9, 5000), (300, 1000), (576, 576)])
def test_xent_diag_f32(dev, rows, cols):
    g = _gen(rows, cols, 7)
    x = torch.randn(rows, cols, generator=g) * 40
    x[0, 0] = 80.0
    if cols > 1:
        x[0, cols - 1] = -80.0
    for r in range(0, rows, 2):                                      # ties equal to the diagonal on both sides of it
        d = x[r, r].item()
        if r > 0:
            x[r, r - 1] = d
            x[r, 0] = d
        if r + 1 < cols:
            x[r, r + 1] = d
            x[r, cols - 1] = d
    p = Padded(rows, cols, dev, x)
    loss, rank = ops.xent_diag_f32(p.view)
    ref_loss, ref_rank = R.xent_diag_ref64(x)
    assert p.guards_ok()
    assert torch.equal(rank.cpu().long(), ref_rank)
    assert torch.allclose(loss.cpu().double(), ref_loss, atol=1e-5)  # (the rule of test_models_gpu.py's check of the same kernel)
    with pytest.raises(CoverError):
        ops.xent_diag_f32(torch.zeros(cols + 1, cols, device=dev))   # row r is labelled r: rows <= cols


@pytest.mark.parametrize("pad_name", ["none", "some", "one_batch_padded"])
@pytest.mark.parametrize("D", [1, 255, 257, 512])
@pytest.mark.parametrize("T", [1, 10])
def test_masked_mean_f32(dev, T, D, pad_name):
    B = 3
    x = torch.randn(B, T, D, generator=_gen(T, D, 8))
    pad = None
    if pad_name != "none":
        pad = torch.zeros(B, T, dtype=torch.bool)
        pad[0, T // 2:] = T > 1
        if pad_name == "one_batch_padded":
            pad[1] = True
    got = ops.masked_mean_f32(x.to(dev), None if pad is None else pad.to(torch.uint8).to(dev), B, T, D)
    ref = R.masked_mean_ref64(x, pad)
    assert close64(got, ref)
    if pad_name == "one_batch_padded":
        assert torch.equal(got[1].cpu(), torch.zeros(D))             # 0 / clamp(0, min=1e-9)


def test_sincos_time_embed(dev):
    """every dim and time against the float64 reference: atol 8e-3 per case, and bf16 mismatches under 1 % of ALL elements (pooled: a
    four-element row is not its own population). The CPU test shows a float64 restatement has none, so the cap is libm headroom."""
    t = torch.tensor([0.0, 1e-3, 0.5, 1.0])
    wrong = total = 0
    for dim in (2, 4, 30, 1024):
        p = Padded(t.shape[0], dim, dev, dtype=torch.bfloat16)
        ops.sincos_time_embed(t.to(dev), dim, 4e-3, 4.0, out=p.view)
        ref = R.sincos_ref64(t, dim, 4e-3, 4.0)
        got = p.view.cpu()
        assert p.guards_ok()
        assert torch.allclose(got.float(), ref.float(), atol=8e-3), dim
        wrong += int((got != ref).sum())
        total += ref.numel()
    print(f"sincos: {wrong} of {total} bf16 values differ")
    assert wrong / total < 0.01
