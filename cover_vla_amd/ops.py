"""Tensor-level wrappers over the C ABI (include/cover_hip.h).

PyTorch-ROCm is plumbing here: it owns device memory and the stream; every arithmetic call below goes through
libcover_hip.so. Nothing in this module computes on the CPU or through torch kernels.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib as L
from .graphs import Graph, PooledGraph, Timer, _stream  # noqa: F401  (ops.Graph / ops.PooledGraph / ops.Timer: their home is graphs.py)

ACT = {"none": 0, "gelu_tanh": 1, "gelu_erf": 2, "silu": 3, "relu": 4}
MASK_LEN, MASK_CAUSAL, MASK_VISLEN = 0, 1, 2


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.CoverError("cover_vla_amd ops need device tensors: there is no CPU path")


# ------------------------------------------------------------------------------------------------ GEMM
@dataclass
class PackedLinear:
    """nn.Linear weight in the MFMA fragment-major layout (+ fp32 bias)."""
    wp: torch.Tensor            # packed bf16 storage
    N: int                      # rows of the packed matrix (2*mlp for GLU)
    K: int
    bias: Optional[torch.Tensor] = None   # fp32 [N]
    glu: bool = False
    w8: Optional[torch.Tensor] = None     # e4m3 twin of the same quantised weight (uint8 storage), cover_pack_weight_fp8
    w8s: Optional[torch.Tensor] = None    # fp32 per-channel power-of-two scales in packed channel order
    use_w8: bool = True                   # tests: False reads the bf16 image in the weight-streaming kernels too
    klinear: bool = False                 # w8 is the k-linear image (cover_pack_weight_fp8_klinear): the operand order of MX block-scaled activations

    @property
    def n_out(self) -> int:
        return self.N // 2 if self.glu else self.N

    @property
    def kp(self) -> int:
        return (self.K + 127) // 128 * 128


def pack_linear(weight: torch.Tensor, bias: Optional[torch.Tensor] = None, glu: bool = False, fp8: bool = False,
                klinear: bool = False) -> PackedLinear:
    """weight: [N, K] (nn.Linear layout) on the device; for glu=True weight = cat([gate, up], 0).
    fp8=True: the weight is QUANTISED to e4m3 with per-output-channel power-of-two scales (cover_quantize_rows_fp8) and kept
    twice -- as the e4m3 image the HBM-bound weight-streaming kernels read (half the bytes) and as the bf16 image of the same
    de-quantised values for the MFMA-bound tiled kernels; both give bit-identical results. klinear=True (fp8, not glu): the e4m3 image in
    the k-linear operand order, which the MX block-scaled activations of quantize_act_fp8_mx / a GLU GEMM's out8 pair with (config 5's down_proj)."""
    assert not (klinear and (glu or not fp8))
    _chk_dev(weight)
    w = weight.to(torch.bfloat16).contiguous()
    N, K = w.shape
    h = L.lib()
    w8 = w8s = None
    if fp8:
        scales = torch.empty(N, dtype=torch.float32, device=w.device)
        wdq = torch.empty_like(w)
        L.check(h.cover_quantize_rows_fp8(w.data_ptr(), K, N, K, scales.data_ptr(), wdq.data_ptr(), _stream()), "quantize_rows_fp8")
        w8 = torch.empty(h.cover_packed_weight_fp8_bytes(N, K), dtype=torch.uint8, device=w.device)
        w8s = torch.empty((N + 15) // 16 * 16, dtype=torch.float32, device=w.device)
        if klinear:
            L.check(h.cover_pack_weight_fp8_klinear(wdq.data_ptr(), K, scales.data_ptr(), N, K, w8.data_ptr(), w8s.data_ptr(), _stream()),
                    "pack_weight_fp8_klinear")
        else:
            L.check(h.cover_pack_weight_fp8(wdq.data_ptr(), K, scales.data_ptr(), N, K, w8.data_ptr(), w8s.data_ptr(), 1 if glu else 0,
                                            _stream()), "pack_weight_fp8")
        w = wdq
    nbytes = h.cover_packed_weight_bytes(N, K)
    wp = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w.device)
    L.check(h.cover_pack_weight_bf16(w.data_ptr(), K, N, K, wp.data_ptr(), 1 if glu else 0, _stream()), "pack_weight")
    # the bias of a bf16 nn.Linear is a bf16 parameter in the reference (paligemma.to(bf16), HF bf16 checkpoints): round it
    # ONCE at load; the epilogue then adds exactly that value in fp32
    b = None if bias is None else bias.detach().to(torch.bfloat16).to(torch.float32).contiguous().to(w.device)
    return PackedLinear(wp, N, K, b, glu, w8, w8s, klinear=klinear)


def quantize_act_fp8(x: torch.Tensor, K: Optional[int] = None):
    """bf16 [M, >= K] rows -> (e4m3 rows uint8 [M, padded K] in the MX MFMA operand's k order, fp32 [M] power-of-two row scales)."""
    _chk_dev(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    M = x.shape[0]
    K = x.shape[1] if K is None else K
    kp = (K + 127) // 128 * 128
    q = torch.empty(M, kp, dtype=torch.uint8, device=x.device)
    sc = torch.empty(M, dtype=torch.float32, device=x.device)
    L.check(L.lib().cover_quantize_act_fp8(x.data_ptr(), x.stride(0), M, K, q.data_ptr(), kp, sc.data_ptr(), _stream()), "quantize_act_fp8")
    return q, sc


def quantize_act_fp8_mx(x: torch.Tensor, K: Optional[int] = None):
    """bf16 [M, >= K] rows -> (e4m3 rows uint8 [M, padded K], PLAIN row-major; E8M0 block scales uint8 [padded K / 128, M, 4]: one power-of-two
    scale per 32 consecutive k of a row) -- cover_quantize_act_fp8_mx, the operand form of a k-linear fp8 weight."""
    _chk_dev(x)
    assert x.dtype == torch.bfloat16 and x.dim() == 2 and x.stride(1) == 1
    M = x.shape[0]
    K = x.shape[1] if K is None else K
    kp = (K + 127) // 128 * 128
    q = torch.empty(M, kp, dtype=torch.uint8, device=x.device)
    mx = torch.empty(kp // 128, M, 4, dtype=torch.uint8, device=x.device)
    L.check(L.lib().cover_quantize_act_fp8_mx(x.data_ptr(), x.stride(0), M, K, q.data_ptr(), kp, mx.data_ptr(), _stream()), "quantize_act_fp8_mx")
    return q, mx


def gemm_workspace(M: int, N: int, K: int, device) -> Optional[torch.Tensor]:
    n = L.lib().cover_gemm_workspace_bytes(M, N, K)
    return torch.empty(max(n, 4) // 4, dtype=torch.float32, device=device) if n else None


def gemm(a: torch.Tensor, lin: PackedLinear, *, act: str = "none", residual: Optional[torch.Tensor] = None,
         layer_scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, out_f32: bool = False,
         out_scale: float = 1.0, variant: int = 0, ws: Optional[torch.Tensor] = None, norm_w: Optional[torch.Tensor] = None,
         norm_out: Optional[torch.Tensor] = None, norm_style: int = 0, norm_w_offset: float = 0.0, norm_eps: float = 1e-6,
         norm_b: Optional[torch.Tensor] = None, a8: Optional[tuple] = None, out8: Optional[tuple] = None) -> torch.Tensor:
    """out[M, n_out] = epi(a[M, K] @ W^T). `a` is bf16 with row stride >= padded K (zero padded).
    a8 = (q uint8 [M, >= padded K], scales fp32 [M]) from quantize_act_fp8: with an fp8 weight twin and M > 64 the GEMM runs on the
    MX-scaled fp8 matrix instruction (config 5) on those operands. With a k-linear weight twin a8 = (q, mx uint8 [kp / 128, M, 4]) from
    quantize_act_fp8_mx (or another GEMM's out8). out8 = (q uint8 [M, >= n_out], mx uint8 [ceil(n_out / 128), M, 4]): a GLU GEMM on the fp8
    tiles writes its output rows block-quantised into them INSTEAD of `out` (which is returned untouched)."""
    _chk_dev(a, residual, out)
    assert a.dtype == torch.bfloat16 and a.dim() == 2 and a.stride(1) == 1
    M = a.shape[0]
    h = L.lib()
    if out is None:
        out = torch.empty(M, lin.n_out, dtype=torch.float32 if out_f32 else torch.bfloat16, device=a.device)
    e = L.GemmEpi()
    e.bias = _ptr(lin.bias)
    e.residual = _ptr(residual)
    e.ld_residual = residual.stride(0) if residual is not None else 0
    e.residual_f32 = 1 if (residual is not None and residual.dtype == torch.float32) else 0
    e.layer_scale = _ptr(layer_scale)
    e.act = ACT[act]
    e.glu = 1 if lin.glu else 0
    e.out_f32 = 1 if out.dtype == torch.float32 else 0
    e.out_scale = out_scale
    if lin.w8 is not None and lin.use_w8:
        e.w8, e.w8_scale = lin.w8.data_ptr(), lin.w8s.data_ptr()
        e.w8_klinear = 1 if lin.klinear else 0
        if a8 is not None:
            q, qs = a8
            _chk_dev(q, qs)
            assert q.dtype == torch.uint8 and q.shape[0] == M and q.stride(1) == 1
            if lin.klinear:
                assert qs.dtype == torch.uint8 and qs.is_contiguous() and tuple(qs.shape) == (lin.kp // 128, M, 4)
                e.a8, e.a8_mx, e.ld_a8 = q.data_ptr(), qs.data_ptr(), q.stride(0)
            else:
                assert qs.dtype == torch.float32
                e.a8, e.a8_scale, e.ld_a8 = q.data_ptr(), qs.data_ptr(), q.stride(0)
    if out8 is not None:
        q, qs = out8
        _chk_dev(q, qs)
        assert q.dtype == torch.uint8 and q.shape[0] == M and q.stride(1) == 1 and qs.dtype == torch.uint8 and qs.is_contiguous()
        assert tuple(qs.shape) == ((lin.n_out + 127) // 128, M, 4)
        e.out8, e.out8_mx, e.ld_out8 = q.data_ptr(), qs.data_ptr(), q.stride(0)
    if norm_w is not None:
        e.norm_w, e.norm_out, e.ld_norm_out = norm_w.data_ptr(), norm_out.data_ptr(), norm_out.stride(0)
        e.norm_style, e.norm_w_offset, e.norm_eps = norm_style, norm_w_offset, norm_eps
        e.norm_b = _ptr(norm_b)
    if ws is None:
        ws = gemm_workspace(M, lin.N, lin.K, a.device)   # None when this shape needs no split-K scratch
    L.check(h.cover_gemm_bf16(a.data_ptr(), a.stride(0), lin.wp.data_ptr(), out.data_ptr(), out.stride(0), M, lin.N,
                              lin.K, C.byref(e), _ptr(ws), ws.numel() * 4 if ws is not None else 0, variant,
                              _stream()), "gemm_bf16")
    return out


def gemm_probe() -> dict:
    """In-kernel probe of the most recent self-loading tiled GEMM launch (cover_gemm_probe): microseconds of prologue / k-loop / epilogue of
    its first workgroup, k-tiles, shader cycles per k-tile and the clock (GHz) the loop ran at. Synchronises the device."""
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * 16)()
    L.check(L.lib().cover_gemm_probe(buf), "gemm_probe")
    w0, w1, w2, w3, c0, c1, nk = (int(buf[i]) for i in range(7))
    e4, e5, e6 = (int(buf[i]) for i in (12, 13, 14))
    loop_us = (w2 - w1) * 0.01
    staged = w2 <= e4 <= e5 <= e6 <= w3          # (the direct epilogue of a ragged tile leaves older stamps there)
    return dict(prologue_us=(w1 - w0) * 0.01, loop_us=loop_us, epilogue_us=(w3 - w2) * 0.01, k_tiles=nk,
                cycles_per_k_tile=(c1 - c0) / max(nk, 1), clock_ghz=(c1 - c0) / max(loop_us, 1e-9) / 1e3,
                epilogue_split_us=[(e4 - w2) * 0.01, (e5 - e4) * 0.01, (e6 - e5) * 0.01, (w3 - e6) * 0.01] if staged else None)


def gemm_plan_counts(reset: bool = False) -> list:
    """Launch counters per GEMM kernel plan since the last reset (cover_gemm_plan_counts; the map is in include/cover_hip.h): [0..8] gemm_tiled
    picks, [10] the 64x128 loader-wave tile, [19] / [20] / [22] weight-streaming generations 2 / 3 / 1, [21] fp8 MFMA tiles, self-loading tiles
    (gemm_v3.hip) 8 waves [23] 224x192, [24] 224x128, [25] 256x128, [26] 128x256, 4 waves [27] 224x96, k-split
    wave pairs [30] 224x96."""
    n = 32
    buf = (C.c_longlong * n)()
    L.lib().cover_gemm_plan_counts(buf, n, 1 if reset else 0)
    return list(buf)


# ------------------------------------------------------------------------------------------------ attention
@dataclass
class Segment:
    k: torch.Tensor                 # any bf16 tensor; strides given explicitly (elements)
    vt: torch.Tensor
    k_strides: Sequence[int]        # (slot, t, h)
    vt_strides: Sequence[int]       # (slot, h, d)
    length: int = 0
    len_of_batch: Optional[torch.Tensor] = None   # int32 [B]
    slot_of_batch: Optional[torch.Tensor] = None  # int32 [B]
    mask: int = MASK_LEN
    causal_offset: int = 0
    vis_len: Optional[torch.Tensor] = None        # int32 [Tq]
    k_offset: int = 0               # element offsets added to the base pointers
    vt_offset: int = 0


def fill_segment(s: L.KvSegment, seg: Segment) -> None:
    s.k = seg.k.data_ptr() + 2 * seg.k_offset
    s.vt = seg.vt.data_ptr() + 2 * seg.vt_offset
    s.k_slot_stride, s.k_t_stride, s.k_h_stride = seg.k_strides
    s.vt_slot_stride, s.vt_h_stride, s.vt_d_stride = seg.vt_strides
    s.slot_of_batch = _ptr(seg.slot_of_batch)
    s.len_of_batch = _ptr(seg.len_of_batch)
    s.vis_len = _ptr(seg.vis_len)
    s.len = seg.length
    s.mask_mode = seg.mask
    s.causal_offset = seg.causal_offset


def attention_args(q: torch.Tensor, q_strides: Sequence[int], out: Optional[torch.Tensor], o_strides: Sequence[int], B: int, Tq: int,
                   Hq: int, Hkv: int, D: int, scale: float, segments: Sequence[Segment], state_in=None, state_out=None, out8=None) -> "L.AttnArgs":
    """cover_attn_args of one problem (the struct holds raw addresses: it keeps its tensors alive).
    state_in / state_out: optional (o fp32 [B,Tq,Hq,D], ml fp32 [B,Tq,Hq,2]) pairs chaining calls over KV segments.
    out8 = (q uint8 [rows, Hq * D], mx uint8 [Hq * D / 128, rows, 4]): the output rows block-quantised (quantize_act_fp8_mx's form) INSTEAD of `out`
    (MHA, D = 128, few query tiles: cover_attn_args.out8)."""
    _chk_dev(q, out)
    a = L.AttnArgs()
    a._keep = (q, out, out8, state_in, state_out, list(segments))
    a.q, a.out = q.data_ptr(), _ptr(out)
    if out8 is not None:
        _chk_dev(out8[0], out8[1])
        assert out8[0].dtype == torch.uint8 and out8[1].dtype == torch.uint8 and out8[1].is_contiguous() and out8[0].is_contiguous()
        a.out8, a.out8_mx, a.out8_rows = out8[0].data_ptr(), out8[1].data_ptr(), out8[0].shape[0]
    if state_in is not None:
        a.state_in_o, a.state_in_ml = state_in[0].data_ptr(), state_in[1].data_ptr()
    if state_out is not None:
        a.state_out_o, a.state_out_ml = state_out[0].data_ptr(), state_out[1].data_ptr()
    a.q_b_stride, a.q_t_stride, a.q_h_stride = q_strides
    a.o_b_stride, a.o_t_stride, a.o_h_stride = o_strides
    a.B, a.Tq, a.Hq, a.Hkv, a.D, a.scale = B, Tq, Hq, Hkv, D, scale
    a.n_seg = len(segments)
    for i, sg in enumerate(segments[:3]):    # (the struct has three slots; n_seg above keeps the true count, which the library refuses when it is not 1..3)
        fill_segment(a.seg[i], sg)
    return a


def attention(q: torch.Tensor, q_strides: Sequence[int], out: Optional[torch.Tensor], o_strides: Sequence[int], B: int, Tq: int,
              Hq: int, Hkv: int, D: int, scale: float, segments: Sequence[Segment], state_in=None, state_out=None, out8=None):
    """cover_attention_bf16; arguments as in attention_args."""
    a = attention_args(q, q_strides, out, o_strides, B, Tq, Hq, Hkv, D, scale, segments, state_in, state_out, out8)
    L.check(L.lib().cover_attention_bf16(C.byref(a), _stream()), "attention_bf16")
    return out


ATTN_FORMS = {-1: None, 0: "PER_TILE", 1: "KSPLIT4", 2: "KSPLIT8", 3: "SHARED"}


def attention_plan_of(a: "L.AttnArgs"):
    """(form name or None when nothing would be launched, block-scaled output, workgroups, waves per workgroup) of an attention_args result:
    cover_attention_plan, nothing launched. Raises CoverError exactly when attention would."""
    plan = (C.c_int * 4)()
    L.check(L.lib().cover_attention_plan(C.byref(a), plan), "attention_plan")
    return ATTN_FORMS[plan[0]], bool(plan[1]), int(plan[2]), int(plan[3])


def attention_plan(*args, **kw):
    """attention_plan_of for the arguments of ops.attention"""
    return attention_plan_of(attention_args(*args, **kw))


def attention_pair(a0: "L.AttnArgs", a1: "L.AttnArgs") -> None:
    """two problems (two attention_args results), in one launch when both run key-split: cover_attention_bf16_pair"""
    L.check(L.lib().cover_attention_bf16_pair(C.byref(a0), C.byref(a1), _stream()), "attention_bf16_pair")


def attention_pair_plan(a0: "L.AttnArgs", a1: "L.AttnArgs") -> bool:
    """True: attention_pair runs one dual launch; False: two launches (cover_attention_pair_plan, nothing launched)"""
    dual = C.c_int(0)
    L.check(L.lib().cover_attention_pair_plan(C.byref(a0), C.byref(a1), C.byref(dual)), "attention_pair_plan")
    return bool(dual.value)


def _fill_rope(a, positions, cos, sin, rope_mode) -> None:
    """the position / table fields that the rope, fused-decode and own-token argument structs share"""
    a.positions, a.cos_table, a.sin_table = _ptr(positions), _ptr(cos), _ptr(sin)
    a.n_pos = cos.shape[0] if cos is not None else 0
    a.rope_mode = rope_mode


def decode_attention_fused(qkv, N, H, D, scale, segments, write_t, out, *, positions=None, cos=None, sin=None, rope_mode=0,
                           partial=None, bias=None):
    """RoPE + KV append + [shared | per-prompt | own] attention for one new token per candidate, one launch."""
    _chk_dev(qkv, out)
    a = L.DecodeAttnArgs()
    a.qkv, a.ld_qkv = qkv.data_ptr(), qkv.stride(0)
    if partial is not None:
        a.n_splits, a.partial, a.bias = partial.shape[0], partial.data_ptr(), _ptr(bias)
    a.N, a.H, a.D, a.scale = N, H, D, scale
    _fill_rope(a, positions, cos, sin, rope_mode)
    for i, sg in enumerate(segments):
        fill_segment(a.seg[i], sg)
    a.write_t = write_t
    a.out, a.out_row_stride = out.data_ptr(), out.stride(0)
    L.check(L.lib().cover_decode_attention_fused(C.byref(a), _stream()), "decode_attention_fused")
    return out


def decode_own_attention(qkv, N, H, D, scale, k_own, v_own, t_cap, write_t, state, *, positions=None, cos=None, sin=None, rope_mode=0,
                         k_scale=None, v_scale=None, slot_of_batch=None):
    """Large-N candidate decode, own-token pass (cover_decode_own_attention): RoPE + append into the head-major own cache
    (k_own / v_own [slots][H][t_cap][D], bf16 or uint8 e4m3 + fp32 row scales [slots][H][t_cap]) + attention over keys 0..write_t;
    state = (o fp32 [N,H,D], ml fp32 [N,H,2]) for ops.attention(..., state_in=state)."""
    _chk_dev(qkv, k_own, v_own, state[0], state[1])
    a = L.OwnAttnArgs()
    a.qkv, a.ld_qkv = qkv.data_ptr(), qkv.stride(0)
    a.N, a.H, a.D, a.scale = N, H, D, scale
    _fill_rope(a, positions, cos, sin, rope_mode)
    a.k, a.v = k_own.data_ptr(), v_own.data_ptr()
    a.fp8 = 1 if k_own.dtype == torch.uint8 else 0
    a.k_scale, a.v_scale = _ptr(k_scale), _ptr(v_scale)
    a.t_cap, a.slot_stride = t_cap, H * t_cap * D
    a.slot_of_batch = _ptr(slot_of_batch)
    a.write_t = write_t
    a.state_o, a.state_ml = state[0].data_ptr(), state[1].data_ptr()
    L.check(L.lib().cover_decode_own_attention(C.byref(a), _stream()), "decode_own_attention")
    return state


# ------------------------------------------------------------------------------------------------ row kernels
def layernorm(x, w, b, eps, out=None):
    _chk_dev(x, w)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().cover_layernorm_bf16(x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(b), out.data_ptr(), out.stride(0),
                                         x.shape[0], x.shape[1], eps, _stream()), "layernorm_bf16")
    return out


def rmsnorm(x, w, eps, w_offset=0.0, style=0, out=None, q8=False):
    """q8: also return the e4m3 twin of the output rows and its row scales (cover_rmsnorm_bf16_q8; quantize_act_fp8's form). True allocates
    them, a (q uint8 [rows, ld8], scales fp32 [rows]) pair is written in place."""
    _chk_dev(x, w)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if q8 is not False and q8 is not None:
        if q8 is True:
            q8 = (torch.empty(x.shape[0], (x.shape[1] + 127) // 128 * 128, dtype=torch.uint8, device=x.device),
                  torch.empty(x.shape[0], dtype=torch.float32, device=x.device))
        q, qs = q8
        _chk_dev(q, qs)
        L.check(L.lib().cover_rmsnorm_bf16_q8(x.data_ptr(), 1 if x.dtype == torch.float32 else 0, x.stride(0), _ptr(w), w_offset,
                                              style, out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], eps, q.data_ptr(), q.stride(0),
                                              qs.data_ptr(), _stream()), "rmsnorm_bf16_q8")
        return out, q, qs
    L.check(L.lib().cover_rmsnorm_bf16(x.data_ptr(), 1 if x.dtype == torch.float32 else 0, x.stride(0), _ptr(w), w_offset,
                                       style, out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], eps, _stream()),
            "rmsnorm_bf16")
    return out


def rope_args(qkv, B, T, Hq, Hkv, D, *, positions=None, cos=None, sin=None, rope_mode=0, k_cache=None,
              k_strides=(0, 0, 0), k_offset=0, vt_cache=None, vt_strides=(0, 0, 0), vt_offset=0, slot_of_batch=None,
              t_offset_of_batch=None, t_offset=0, partial=None, bias=None) -> "L.RopeArgs":
    """cover_rope_args of one row group. partial fp32 [n_splits, B * T, (Hq + 2 Hkv) * D] (+ bias fp32 [(Hq + 2 Hkv) * D]): the values are
    bf16(sum_s partial[s] + bias) instead of what qkv holds (the split-K fold); q is still written to qkv."""
    _chk_dev(qkv, vt_cache, partial, bias)
    a = L.RopeArgs()
    a._keep = (qkv, positions, cos, sin, k_cache, vt_cache, slot_of_batch, t_offset_of_batch, partial, bias)   # the struct holds raw addresses
    if partial is not None:
        assert partial.dtype == torch.float32 and partial.is_contiguous() and partial.shape[1:] == (B * T, (Hq + 2 * Hkv) * D)
        assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == (Hq + 2 * Hkv) * D)
        a.n_splits, a.partial, a.bias = partial.shape[0], partial.data_ptr(), _ptr(bias)
    else:
        assert bias is None, "bias is part of the split-K fold: it needs partial"
    a.qkv, a.ld_qkv = qkv.data_ptr(), qkv.stride(0)
    a.B, a.T, a.Hq, a.Hkv, a.D = B, T, Hq, Hkv, D
    _fill_rope(a, positions, cos, sin, rope_mode)
    a.k_cache = None if k_cache is None else k_cache.data_ptr() + 2 * k_offset
    a.k_slot_stride, a.k_t_stride, a.k_h_stride = k_strides
    a.vt_cache = vt_cache.data_ptr() + 2 * vt_offset
    a.vt_slot_stride, a.vt_h_stride, a.vt_d_stride = vt_strides
    a.slot_of_batch = _ptr(slot_of_batch)
    a.t_offset_of_batch = _ptr(t_offset_of_batch)
    a.t_offset = t_offset
    return a


def rope_kv_write(qkv, B, T, Hq, Hkv, D, **kw):
    """RoPE + K / V^T placement of one row group; keywords as in rope_args."""
    a = rope_args(qkv, B, T, Hq, Hkv, D, **kw)
    L.check(L.lib().cover_rope_kv_write(C.byref(a), _stream()), "rope_kv_write")


def rope_kv_write_pair(a0, a1):
    """two row groups (two rope_args results) in one launch: cover_rope_kv_write_pair"""
    L.check(L.lib().cover_rope_kv_write_pair(C.byref(a0), C.byref(a1), _stream()), "rope_kv_write_pair")


def embed_gather(table, ids, scale=1.0, out=None):
    _chk_dev(table, ids)
    n, dim = ids.numel(), table.shape[1]
    if out is None:
        out = torch.empty(n, dim, dtype=torch.bfloat16, device=table.device)
    L.check(L.lib().cover_embed_gather(table.data_ptr(), dim, ids.data_ptr(), n, scale, out.data_ptr(), out.stride(0),
                                       _stream()), "embed_gather")
    return out


def patchify(img, patch, mul, add, ld_out, out=None):
    """img: uint8 [n,H,W,3] or fp32 [n,3,H,W] -> bf16 [n*nP, ld_out] rows (k = c*p*p + py*p + px)."""
    _chk_dev(img)
    a = L.PatchifyArgs()
    if img.dtype == torch.uint8:
        n, H, W, _ = img.shape
        a.in_u8_hwc = 1
    else:
        assert img.dtype == torch.float32
        n, _, H, W = img.shape
        a.in_u8_hwc = 0
    img = img.contiguous()
    a.img, a.H, a.W, a.patch, a.n_img, a.img_stride = img.data_ptr(), H, W, patch, n, 3 * H * W
    for i in range(3):
        a.mul[i], a.add[i] = float(mul[i]), float(add[i])
    rows = n * (H // patch) * (W // patch)
    if out is None:
        out = torch.empty(rows, ld_out, dtype=torch.bfloat16, device=img.device)
    a.out, a.ld_out = out.data_ptr(), out.stride(0)
    L.check(L.lib().cover_patchify(C.byref(a), _stream()), "patchify")
    return out


def copy_rows(src, dst, rows, cols, src_idx=None, dst_idx=None):
    _chk_dev(src, dst)
    L.check(L.lib().cover_copy_rows_bf16(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), rows, cols,
                                         _ptr(src_idx), _ptr(dst_idx), _stream()), "copy_rows")


def add_rows(x, add):
    _chk_dev(x, add)
    L.check(L.lib().cover_add_rows_bf16(x.data_ptr(), x.stride(0), add.data_ptr(), add.stride(0), x.shape[0], x.shape[1],
                                        add.shape[0], _stream()), "add_rows")
    return x


def scale_bf16(x, pre_div, post_mul):
    _chk_dev(x)
    L.check(L.lib().cover_scale_bf16(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], pre_div, post_mul, _stream()),
            "scale_bf16")
    return x


def cast_f32_to_bf16(x, out=None):
    _chk_dev(x)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    L.check(L.lib().cover_cast_f32_to_bf16(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0],
                                           x.shape[1], _stream()), "cast")
    return out


def cast_bf16_to_f32(x, out=None):
    _chk_dev(x)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    L.check(L.lib().cover_cast_bf16_to_f32(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0],
                                           x.shape[1], _stream()), "cast")
    return out


# ------------------------------------------------------------------------------------------------ fp32 kernels
def gemm_f32(a, b, *, bias=None, act="none", alpha=1.0, residual=None, out=None, b_is_kn=False, batch=1,
             a_bs=0, b_bs=0, c_bs=0, M=None, N=None, K=None, bias_bs=0):
    """C[m,n] = residual + alpha*act(sum_k a[m,k] b[n,k] + bias[n]). b_is_kn: b given as [K, N] (k-major)."""
    _chk_dev(a, b)
    g = L.GemmF32Args()
    M = a.shape[-2] if M is None else M
    K = a.shape[-1] if K is None else K
    if N is None:
        N = b.shape[-1] if b_is_kn else b.shape[-2]
    g.A, g.a_row_stride, g.a_k_stride = a.data_ptr(), a.stride(-2), a.stride(-1)
    g.B = b.data_ptr()
    if b_is_kn:
        g.b_row_stride, g.b_k_stride = b.stride(-1), b.stride(-2)
    else:
        g.b_row_stride, g.b_k_stride = b.stride(-2), b.stride(-1)
    if out is None:
        shape = (batch, M, N) if batch > 1 else (M, N)
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    g.C, g.c_row_stride = out.data_ptr(), out.stride(-2)
    g.bias, g.residual = _ptr(bias), _ptr(residual)
    g.ld_residual = residual.stride(-2) if residual is not None else 0
    g.M, g.N, g.K, g.act, g.alpha = M, N, K, ACT[act], alpha
    g.batch, g.a_batch_stride, g.b_batch_stride, g.c_batch_stride = batch, a_bs, b_bs, c_bs
    g.bias_batch_stride = bias_bs
    L.check(L.lib().cover_gemm_f32(C.byref(g), _stream()), "gemm_f32")
    return out


def gemm_f32_raw(a_ptr, a_rs, a_ks, b_ptr, b_rs, b_ks, c_ptr, c_rs, M, N, K, *, bias=None, residual_ptr=None, ld_res=0,
                 act="none", alpha=1.0, batch=1, a_bs=0, b_bs=0, c_bs=0, bias_bs=0):
    """Pointer-level form of gemm_f32 (element strides) for strided / batched views that torch cannot express."""
    g = L.GemmF32Args()
    g.A, g.a_row_stride, g.a_k_stride = a_ptr, a_rs, a_ks
    g.B, g.b_row_stride, g.b_k_stride = b_ptr, b_rs, b_ks
    g.C, g.c_row_stride = c_ptr, c_rs
    g.bias, g.residual, g.ld_residual = _ptr(bias), residual_ptr, ld_res
    g.M, g.N, g.K, g.act, g.alpha = M, N, K, ACT[act], alpha
    g.batch, g.a_batch_stride, g.b_batch_stride, g.c_batch_stride = batch, a_bs, b_bs, c_bs
    g.bias_batch_stride = bias_bs
    L.check(L.lib().cover_gemm_f32(C.byref(g), _stream()), "gemm_f32")


GEMM_F32_PLANS = ("DIRECT_FM1", "DIRECT_FM2", "TILE64", "TILE32_K128", "TILE32_K32")   # COVER_GEMM_F32_* (include/cover_hip.h)


def gemm_f32_plan(a_ptr, a_rs, a_ks, b_ptr, b_rs, b_ks, c_ptr, c_rs, M, N, K, *, batch=1, a_bs=0, b_bs=0, c_bs=0):
    """(plan name, deep) cover_gemm_f32 would take for these pointers (only null / alignment matter) and element strides: no launch,
    no GPU. plan name is one of GEMM_F32_PLANS (None: nothing to launch), deep = the COVER_F32_UNR=8 window."""
    g = L.GemmF32Args()
    g.A, g.a_row_stride, g.a_k_stride = a_ptr, a_rs, a_ks
    g.B, g.b_row_stride, g.b_k_stride = b_ptr, b_rs, b_ks
    g.C, g.c_row_stride = c_ptr, c_rs
    g.M, g.N, g.K, g.alpha = M, N, K, 1.0
    g.batch, g.a_batch_stride, g.b_batch_stride, g.c_batch_stride = batch, a_bs, b_bs, c_bs
    out = (C.c_int * 2)()
    L.check(L.lib().cover_gemm_f32_plan(C.byref(g), out), "gemm_f32_plan")
    return (GEMM_F32_PLANS[out[0]] if out[0] >= 0 else None), bool(out[1])


def layernorm_f32(x, w, b, eps=1e-5, out=None):
    _chk_dev(x)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().cover_layernorm_f32(x.data_ptr(), x.stride(0), _ptr(w), _ptr(b), out.data_ptr(), out.stride(0),
                                        x.shape[0], x.shape[1], eps, _stream()), "layernorm_f32")
    return out


def layernorm_f32_grouped(x, w, b, rows_per_group, eps=1e-5, out=None):
    """x fp32 [G * rows_per_group, dim]; w, b fp32 [G, dim]: group g's rows use w[g], b[g] (ensemble members in one launch)."""
    _chk_dev(x, w)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().cover_layernorm_f32_grouped(x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(b), out.data_ptr(), out.stride(0),
                                                x.shape[0], x.shape[1], eps, rows_per_group, w.stride(0), _stream()),
            "layernorm_f32_grouped")
    return out


def softmax_rows_f32(x, scale=1.0):
    _chk_dev(x)
    L.check(L.lib().cover_softmax_rows_f32(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], scale, _stream()), "softmax")
    return x


def l2norm_rows_f32(x, out=None):
    _chk_dev(x)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().cover_l2norm_rows_f32(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0],
                                          x.shape[1], _stream()), "l2norm")
    return out


def add_f32(a, b, out=None):
    _chk_dev(a, b)
    out = torch.empty_like(a) if out is None else out
    L.check(L.lib().cover_add_f32(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0),
                                  a.shape[0], a.shape[1], b.shape[0], _stream()), "add_f32")
    return out


def xent_diag_f32(logits):
    """logits fp32 [B, C] (B <= C) -> (loss fp32 [B] = logsumexp(row) - row[r], rank int32 [B] = entries ranked ahead of row[r])."""
    _chk_dev(logits)
    B, Cn = logits.shape
    loss = torch.empty(B, dtype=torch.float32, device=logits.device)
    rank = torch.empty(B, dtype=torch.int32, device=logits.device)
    L.check(L.lib().cover_xent_diag_f32(logits.data_ptr(), logits.stride(0), B, Cn, loss.data_ptr(), rank.data_ptr(), _stream()),
            "xent_diag_f32")
    return loss, rank


def act_f32(x, act, out=None):
    _chk_dev(x)
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().cover_act_f32(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], ACT[act], _stream()),
            "act_f32")
    return out


def mha_f32(q, k, v, B, Tq, Tk, H, Dh, q_strides, k_strides, v_strides, key_pad=None, out=None, o_strides=None):
    """strides = (batch, token) in elements; heads are contiguous blocks of Dh inside a token row."""
    _chk_dev(q, k, v)
    if out is None:
        out = torch.empty(B, Tq, H * Dh, dtype=torch.float32, device=q.device)
        o_strides = (Tq * H * Dh, H * Dh)
    a = L.MhaF32Args()
    a.q, a.q_b_stride, a.q_t_stride = q.data_ptr(), q_strides[0], q_strides[1]
    a.k, a.k_b_stride, a.k_t_stride = k.data_ptr(), k_strides[0], k_strides[1]
    a.v, a.v_b_stride, a.v_t_stride = v.data_ptr(), v_strides[0], v_strides[1]
    a.out, a.o_b_stride, a.o_t_stride = out.data_ptr(), o_strides[0], o_strides[1]
    a.key_pad = _ptr(key_pad)
    a.B, a.Tq, a.Tk, a.H, a.Dh, a.scale = B, Tq, Tk, H, Dh, Dh ** -0.5
    L.check(L.lib().cover_mha_f32(C.byref(a), _stream()), "mha_f32")
    return out


def masked_mean_f32(x, pad, B, T, D):
    _chk_dev(x)
    out = torch.empty(B, D, dtype=torch.float32, device=x.device)
    L.check(L.lib().cover_masked_mean_f32(x.data_ptr(), _ptr(pad), out.data_ptr(), B, T, D, _stream()), "masked_mean")
    return out


def sincos_time_embed(time, dim, min_period, max_period, out=None):
    _chk_dev(time)
    B = time.shape[0]
    if out is None:
        out = torch.empty(B, dim, dtype=torch.bfloat16, device=time.device)
    L.check(L.lib().cover_sincos_time_embed(time.data_ptr(), B, dim, min_period, max_period, out.data_ptr(), out.stride(0),
                                            _stream()), "sincos_time_embed")
    return out


# ------------------------------------------------------------------------------------------------ selection
def token_select(logits, lo, hi, uniform=None, temperature=1.0, out_tok=None, out_logit=None):
    """cover_token_select over columns [lo, hi) of fp32 logits [rows, >= hi]: uniform None = greedy (the first maximum), else the inverse-CDF
    pick at `temperature` with uniform fp32 [rows] (hi - lo <= 4096, temperature > 0). Returns (token int64 [rows], its logit fp32 [rows]).
    out_tok int64 [rows] / out_logit fp32 [rows] (contiguous, e.g. a row of a [steps, rows] buffer): written in place of fresh tensors.
    A NaN never wins the greedy comparison; a row of NaNs gives token lo and the NaN at lo, so the id is always inside [lo, hi). A sampled
    row that contains a NaN gives some id inside [lo, hi) and leaves the other rows as they would be without it."""
    _chk_dev(logits, uniform, out_tok, out_logit)
    rows = logits.shape[0]
    tok = torch.empty(rows, dtype=torch.int64, device=logits.device) if out_tok is None else out_tok
    lg = torch.empty(rows, dtype=torch.float32, device=logits.device) if out_logit is None else out_logit
    assert tok.dtype == torch.int64 and lg.dtype == torch.float32 and tok.is_contiguous() and lg.is_contiguous() and tok.numel() == rows == lg.numel()
    assert uniform is None or (uniform.is_contiguous() and uniform.dtype == torch.float32 and uniform.numel() == rows)
    a = L.TokenSelectArgs()
    a.logits, a.ld, a.rows, a.lo, a.hi = logits.data_ptr(), logits.stride(0), rows, lo, hi
    a.uniform, a.temperature = _ptr(uniform), temperature
    a.token_out, a.logit_out = tok.data_ptr(), lg.data_ptr()
    L.check(L.lib().cover_token_select(C.byref(a), _stream()), "token_select")
    return tok, lg


def token_sample(logits, lo, hi, uniform, temperature=1.0, top_k=0, top_p=1.0, out_tok=None, out_logit=None, out_kept=None,
                 out_logprob=None):
    """Filtered inverse-CDF sampling over columns [lo, hi) of fp32 logits [rows, >= hi] (cover_token_sample: temperature, then top-k
    with ties kept, then top-p, then the pick with the host-supplied uniform fp32 [rows] in [0, 1)); hi - lo up to 2^20.
    Returns (token int64 [rows], its raw logit fp32 [rows], size of the kept set int32 [rows]); out_tok / out_logit / out_kept
    (contiguous, [rows]) are written in place of fresh tensors, as in token_select. Deterministic, one launch, recordable.
    out_logprob fp32 [rows] (contiguous): also filled with the log-probability of each pick under the distribution it was drawn from
    (cover_token_sample_scored; the pick, its logit and the kept count are the plain call's, bit for bit)."""
    if uniform is None:
        raise L.CoverError("token_sample needs uniforms (greedy selection is token_select)")
    if not temperature > 0 or not top_p > 0 or top_k < 0 or hi <= lo or lo < 0:
        raise L.CoverError(f"token_sample: temperature > 0, top_p > 0, top_k >= 0 and 0 <= lo < hi are required "
                           f"(got temperature={temperature}, top_k={top_k}, top_p={top_p}, lo={lo}, hi={hi})")
    _chk_dev(logits, uniform, out_tok, out_logit, out_kept, out_logprob)
    rows = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and hi <= logits.shape[1]
    tok = torch.empty(rows, dtype=torch.int64, device=logits.device) if out_tok is None else out_tok
    lg = torch.empty(rows, dtype=torch.float32, device=logits.device) if out_logit is None else out_logit
    kept = torch.empty(rows, dtype=torch.int32, device=logits.device) if out_kept is None else out_kept
    assert tok.dtype == torch.int64 and lg.dtype == torch.float32 and kept.dtype == torch.int32
    assert tok.is_contiguous() and lg.is_contiguous() and kept.is_contiguous() and tok.numel() == rows == lg.numel() == kept.numel()
    assert uniform.is_contiguous() and uniform.dtype == torch.float32 and uniform.numel() == rows
    a = L.TokenSampleArgs() if out_logprob is None else L.TokenSampleScoredArgs()
    a.logits, a.ld, a.rows, a.lo, a.hi = logits.data_ptr(), logits.stride(0), rows, lo, hi
    a.uniform, a.temperature, a.top_k, a.top_p = uniform.data_ptr(), temperature, int(top_k), top_p
    a.token_out, a.logit_out, a.kept_out = tok.data_ptr(), lg.data_ptr(), kept.data_ptr()
    if out_logprob is None:
        L.check(L.lib().cover_token_sample(C.byref(a), _stream()), "token_sample")
    else:
        assert out_logprob.dtype == torch.float32 and out_logprob.is_contiguous() and out_logprob.numel() == rows
        a.logprob_out = out_logprob.data_ptr()
        L.check(L.lib().cover_token_sample_scored(C.byref(a), _stream()), "token_sample_scored")
    return tok, lg, kept


def token_logprob(logits, lo, hi, tokens, temperature=1.0, top_k=0, top_p=1.0, out=None, out_kept=None):
    """Log-probability fp32 [rows] of tokens int64 [rows] under the distribution token_sample draws from with the same parameters
    over columns [lo, hi) (cover_token_logprob: softmax of logits / temperature over the set top-k and top-p keep): -inf for a token
    that is filtered out or lies outside [lo, hi) (a pad id). out fp32 [rows] / out_kept int32 [rows] (contiguous) are written in
    place. Deterministic, one launch, recordable; on token_sample's own picks it equals that call's out_logprob bit for bit."""
    if not temperature > 0 or not top_p > 0 or top_k < 0 or hi <= lo or lo < 0:
        raise L.CoverError(f"token_logprob: temperature > 0, top_p > 0, top_k >= 0 and 0 <= lo < hi are required "
                           f"(got temperature={temperature}, top_k={top_k}, top_p={top_p}, lo={lo}, hi={hi})")
    _chk_dev(logits, tokens, out, out_kept)
    rows = logits.shape[0]
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1 and hi <= logits.shape[1]
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() == rows
    lp = torch.empty(rows, dtype=torch.float32, device=logits.device) if out is None else out
    assert lp.dtype == torch.float32 and lp.is_contiguous() and lp.numel() == rows
    assert out_kept is None or (out_kept.dtype == torch.int32 and out_kept.is_contiguous() and out_kept.numel() == rows)
    a = L.TokenLogprobArgs()
    a.logits, a.ld, a.rows, a.lo, a.hi = logits.data_ptr(), logits.stride(0), rows, lo, hi
    a.temperature, a.top_k, a.top_p = temperature, int(top_k), top_p
    a.token, a.logprob_out, a.kept_out = tokens.data_ptr(), lp.data_ptr(), _ptr(out_kept)
    L.check(L.lib().cover_token_logprob(C.byref(a), _stream()), "token_logprob")
    return lp


# ---- checks and struct fields the CoverError-raising token wrappers share (what = the wrapper's name in the message) ----
def _chk_range(what, lo, hi):
    if hi <= lo or lo < 0:
        raise L.CoverError(f"{what}: 0 <= lo < hi is required (got lo={lo}, hi={hi})")


def _chk_logits(what, logits, hi) -> int:
    """logits fp32 [rows, >= hi] with unit column stride; returns rows."""
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or hi > logits.shape[1]:
        raise L.CoverError(f"{what}: logits must be fp32 [rows, >= hi] with unit column stride")
    return logits.shape[0]


def _chk_topn_n(what, n) -> int:
    if not 1 <= int(n) <= 64:
        raise L.CoverError(f"{what}: 1 <= n <= 64 is required (got n={n})")
    return int(n)


def _chk_rows_out(what, rows, *outs):
    """Each (name, tensor or None, dtype): contiguous [rows]."""
    for name, t, dt in outs:
        if t is not None and (t.dtype != dt or t.numel() != rows or not t.is_contiguous()):
            raise L.CoverError(f"{what}: {name} must be contiguous {dt} [rows]")


def _chk_rows_n_out(what, rows, n, *outs):
    """Each (name, tensor or None, dtype): [rows, n], unit column stride, any row stride >= n."""
    for name, t, dt in outs:
        if t is not None and (t.dtype != dt or tuple(t.shape) != (rows, n) or (n > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < n)):
            raise L.CoverError(f"{what}: {name} must be {dt} [rows, n] with unit column stride and a row stride >= n")


def _fill_rows(a, logits, rows, lo, hi):
    a.logits, a.ld, a.rows, a.lo, a.hi = logits.data_ptr(), logits.stride(0), rows, lo, hi


def _topn_outputs(a, what, logits, rows, n, out_tok, out_logprob, out_entropy, out_kept):
    """Checks the four outputs of a top-n call, allocates the missing ones and fills a's output fields; returns (tok, lp, ent)."""
    _chk_rows_n_out(what, rows, n, ("out_tok", out_tok, torch.int64), ("out_logprob", out_logprob, torch.float32))
    _chk_rows_out(what, rows, ("out_entropy", out_entropy, torch.float32), ("out_kept", out_kept, torch.int32))
    _chk_dev(logits, out_tok, out_logprob, out_entropy, out_kept)
    tok = torch.empty(rows, n, dtype=torch.int64, device=logits.device) if out_tok is None else out_tok
    lp = torch.empty(rows, n, dtype=torch.float32, device=logits.device) if out_logprob is None else out_logprob
    ent = torch.empty(rows, dtype=torch.float32, device=logits.device) if out_entropy is None else out_entropy
    a.n = n
    a.token_out, a.ld_tok = tok.data_ptr(), max(tok.stride(0), n)
    a.logprob_out, a.ld_lp = lp.data_ptr(), max(lp.stride(0), n)
    a.entropy_out, a.kept_out = ent.data_ptr(), _ptr(out_kept)
    return tok, lp, ent


def token_topn(logits, lo, hi, n, temperature=1.0, top_k=0, top_p=1.0, out_tok=None, out_logprob=None, out_entropy=None, out_kept=None):
    """The n (1..64) most probable tokens of every row under the distribution token_sample draws from with the same parameters over
    columns [lo, hi), their log-probabilities and the entropy of that distribution (cover_token_topn). Returns (tokens int64 [rows, n],
    logprobs fp32 [rows, n], entropy fp32 [rows]): ranks by descending logit, equal logits by ascending index; a row whose kept set
    has fewer than n members is padded with token -1 / log-probability -inf; entropy in nats over the kept set. A log-probability is
    token_logprob's for that token, bit for bit. out_tok / out_logprob ([rows, n], unit column stride, any row stride >= n: a step's
    slab of a [steps, rows, n] buffer), out_entropy fp32 / out_kept int32 ([rows], contiguous) are written in place.
    Deterministic, one launch, recordable."""
    if not temperature > 0 or not top_p > 0 or top_k < 0 or hi <= lo or lo < 0:
        raise L.CoverError(f"token_topn: temperature > 0, top_p > 0, top_k >= 0 and 0 <= lo < hi are required "
                           f"(got temperature={temperature}, top_k={top_k}, top_p={top_p}, lo={lo}, hi={hi})")
    n = _chk_topn_n("token_topn", n)
    rows = _chk_logits("token_topn", logits, hi)
    a = L.TokenTopnArgs()
    tok, lp, ent = _topn_outputs(a, "token_topn", logits, rows, n, out_tok, out_logprob, out_entropy, out_kept)
    _fill_rows(a, logits, rows, lo, hi)
    a.temperature, a.top_k, a.top_p = temperature, int(top_k), top_p
    L.check(L.lib().cover_token_topn(C.byref(a), _stream()), "token_topn")
    return tok, lp, ent


def _row_params(what, rows, temperature, top_k, top_p):
    """The per-row parameter arguments of the *_rows wrappers, checked on the host: (temperature, top_k, top_p, upload). A device tensor
    must be contiguous fp32 / int32 / fp32 [rows] and passes as it is (its values are the kernel's to judge: an invalid row reports
    itself). A Python sequence, numpy array or CPU tensor is validated here -- every temperature >= 0, top_p > 0, top_k >= 0, all
    finite -- and comes back as a CPU tensor of the right dtype for the caller to upload once the other arguments have passed."""
    out = []
    for name, v, dt, ok, rule in (("temperature", temperature, torch.float32, lambda a: a >= 0, ">= 0 (0 marks a greedy row)"),
                                  ("top_k", top_k, torch.int32, lambda a: a >= 0, ">= 0"), ("top_p", top_p, torch.float32, lambda a: a > 0, "> 0")):
        if v is None:
            if name == "temperature":
                raise L.CoverError(f"{what}: temperature [rows] is required")
            out.append(None)
        elif isinstance(v, torch.Tensor) and v.is_cuda:
            if v.dtype != dt or v.dim() != 1 or v.numel() != rows or not v.is_contiguous():
                raise L.CoverError(f"{what}: {name} must be a contiguous {dt} device tensor [rows = {rows}]")
            out.append(v)
        else:
            try:
                a = np.asarray(v.numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise L.CoverError(f"{what}: {name} must be numeric [rows]") from e
            if a.shape != (rows,):
                raise L.CoverError(f"{what}: {name} must have one entry per row ({rows}), got shape {a.shape}")
            if not np.all(np.isfinite(a)) or not np.all(ok(a)) or (dt == torch.int32 and (np.any(a != np.rint(a)) or np.any(a > 2 ** 31 - 1))):
                raise L.CoverError(f"{what}: every {name} must be finite and {rule}")
            out.append(torch.from_numpy(a).to(dt))
    return out


# a sampling parameter of the models: one scalar, or one entry per row (sequence, numpy array, CPU or device tensor of any numeric dtype)
RowParam = Union[float, int, Sequence[float], np.ndarray, torch.Tensor]


def is_per_row(v) -> bool:
    """Is a sampling parameter given per row (a sequence, an array or a tensor with a dimension) and not as one scalar?"""
    if isinstance(v, (torch.Tensor, np.ndarray)):
        return v.ndim > 0
    return isinstance(v, (list, tuple))


def row_param_tensors(rows, temperature, top_k, top_p, device):
    """(temperature fp32, top_k int32, top_p fp32) device tensors [rows] from arguments that are each a scalar or one entry per row:
    what the models hand to pick_token(row_params=). Every value is validated on the host as in token_sample_rows -- a device tensor (of any
    numeric dtype) is read back once for it -- so a call that returns never leads to an invalid row: the models feed each pick to an
    embedding gather, which the -1 of an invalid row must not reach."""
    def wide(v):
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu()
        return np.full(rows, float(v)) if not is_per_row(v) else v
    params = _row_params("row_param_tensors", rows, wide(temperature), wide(top_k), wide(top_p))
    return tuple(_upload_row_params(params, device))


def _upload_row_params(params, device):
    return [p if p is None or p.is_cuda else p.to(device) for p in params]


class TokenAllow:
    """Allowed-token sets for the *_rows calls (cover_token_allow): bits uint32 (or int32) device tensor [n_sets, words] with unit column
    stride, bit (c & 31) of word (c >> 5) of a set = column c may be drawn (token_allow_sets builds it); set_of_row int32 device tensor
    [rows] naming each row's set, None = set 0 for every row. A holder of the caller's tensors: the kernels read their current contents,
    so both may be rewritten between launches and graph replays."""

    def __init__(self, bits, set_of_row=None):
        if not isinstance(bits, torch.Tensor) or bits.dtype not in (torch.uint32, torch.int32) or bits.dim() != 2 or bits.shape[0] < 1 \
                or (bits.shape[1] > 1 and bits.stride(1) != 1):
            raise L.CoverError("TokenAllow: bits must be a uint32 tensor [n_sets >= 1, words] with unit column stride")
        if set_of_row is not None and (not isinstance(set_of_row, torch.Tensor) or set_of_row.dtype != torch.int32 or set_of_row.dim() != 1
                                       or not set_of_row.is_contiguous()):
            raise L.CoverError("TokenAllow: set_of_row must be a contiguous int32 tensor [rows]")
        self.bits = bits
        self.set_of_row = set_of_row

    @property
    def n_sets(self):
        return self.bits.shape[0]


def token_allow_sets(vocab, sets, device=None):
    """Build the bit masks of TokenAllow on the host: sets is a sequence of sets, each a sequence of ids and / or half-open (a, b) ranges
    of ids. Returns a uint32 tensor [n_sets, ceil(vocab / 32)] (on device if given). ValueError on an id outside [0, vocab)."""
    vocab = int(vocab)
    if vocab < 1 or len(sets) < 1:
        raise ValueError("token_allow_sets: vocab >= 1 and at least one set are required")
    words = (vocab + 31) // 32
    on = np.zeros((len(sets), words * 32), dtype=bool)
    for i, entries in enumerate(sets):
        for e in entries:
            if isinstance(e, (tuple, list)):
                if len(e) != 2:
                    raise ValueError(f"token_allow_sets: a range is (a, b), got {e!r}")
                a, b = int(e[0]), int(e[1])
                if not 0 <= a <= b <= vocab:
                    raise ValueError(f"token_allow_sets: range ({a}, {b}) leaves [0, {vocab})")
                on[i, a:b] = True
            else:
                t = int(e)
                if not 0 <= t < vocab:
                    raise ValueError(f"token_allow_sets: id {t} is outside [0, {vocab})")
                on[i, t] = True
    bits = np.packbits(on.reshape(len(sets), words, 32), axis=2, bitorder="little").view("<u4").reshape(len(sets), words)
    out = torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).view(torch.uint32)
    return out if device is None else out.to(device)


def _allow_arg(what, allow, rows, hi, logits):
    """The cover_token_allow of a launch from a TokenAllow, shapes checked on the host (the contents are the kernel's to judge)."""
    if not isinstance(allow, TokenAllow):
        raise L.CoverError(f"{what}: allow must be an ops.TokenAllow")
    if allow.bits.shape[1] * 32 < hi:
        raise L.CoverError(f"{what}: allow.bits has {allow.bits.shape[1]} words per set, columns below hi = {hi} need {(hi + 31) // 32}")
    if allow.set_of_row is not None and allow.set_of_row.numel() != rows:
        raise L.CoverError(f"{what}: allow.set_of_row must have one entry per row ({rows})")
    _chk_dev(logits, allow.bits, allow.set_of_row)
    al = L.TokenAllow()
    al.bits, al.ld_words, al.n_sets = allow.bits.data_ptr(), max(allow.bits.stride(0), allow.bits.shape[1]), allow.bits.shape[0]
    al.set_of_row = _ptr(allow.set_of_row)
    return al


def ref_temperature_value(what, v) -> float:
    """A reference temperature (token_sample_rows' ref_temperature, the models' prior_temperature) as a float: one finite number > 0, else CoverError."""
    try:
        v = float(v)
    except (TypeError, ValueError) as e:
        raise L.CoverError(f"{what} must be one number") from e
    if not (v > 0.0 and math.isfinite(v)):
        raise L.CoverError(f"{what} must be finite and > 0 (got {v})")
    return v


def token_sample_rows(logits, lo, hi, uniform, temperature, top_k=None, top_p=None, out_tok=None, out_logit=None, out_kept=None,
                      out_logprob=None, allow=None, ref_temperature=None, out_ref_logprob=None):
    """token_sample with the parameters of every row its own (cover_token_sample_rows): temperature fp32 / top_k int32 / top_p fp32 device
    tensors [rows] (top_k None = 0, top_p None = 1 for every row); a Python sequence or CPU tensor is validated on the host
    (temperature >= 0, top_p > 0, top_k >= 0, all finite) and uploaded. temperature[r] > 0: row r is token_sample's row with its
    parameters, always on the integer masses (no token_select detour for a narrow unfiltered range). temperature[r] == 0: a greedy row,
    token = the first arg-max over [lo, hi), kept = hi - lo, log-probability at temperature 1 unfiltered; its top_k / top_p / uniform
    entries are not read. A row whose device-side parameters are invalid writes token -1, logit / log-probability NaN, kept 0.
    Returns (token int64 [rows], its raw logit fp32 [rows], kept int32 [rows]); out_* as in token_sample. One launch, recordable,
    deterministic: a row's result does not depend on the other rows of the launch.
    allow = TokenAllow: cover_token_sample_rows_allowed, the same on each row restricted to the columns of its set (max, top-k, top-p, pick,
    kept and log-probability over the allowed columns only; disallowed columns are never looked at); a row whose set index is out of
    range or whose set has no column in [lo, hi) is an invalid row. None issues exactly the unmasked call.
    ref_temperature = T_ref with out_ref_logprob fp32 [rows] (given together): cover_token_sample_rows_ref, the same launch also writes the
    log-probability of each pick under ONE reference distribution shared by every row -- temperature T_ref, both filters off, over the same
    range and the same allowed set -- which is token_logprob_rows(logits, lo, hi, token, T_ref, None, None, allow=) bit for bit (NaN on an
    invalid row). The common yardstick of a ladder: out_logprob is taken under each row's own distribution and does not compare across
    rungs. Both None issues exactly the call made without them."""
    if uniform is None:
        raise L.CoverError("token_sample_rows needs uniforms [rows] (a greedy row ignores its entry)")
    if (ref_temperature is None) != (out_ref_logprob is None):
        raise L.CoverError("token_sample_rows: ref_temperature and out_ref_logprob are given together")
    if ref_temperature is not None:
        ref_temperature = ref_temperature_value("token_sample_rows: ref_temperature", ref_temperature)
    _chk_range("token_sample_rows", lo, hi)
    rows = _chk_logits("token_sample_rows", logits, hi)
    params = _row_params("token_sample_rows", rows, temperature, top_k, top_p)
    if uniform.dtype != torch.float32 or uniform.numel() != rows or not uniform.is_contiguous():
        raise L.CoverError("token_sample_rows: uniform must be contiguous fp32 [rows]")
    _chk_rows_out("token_sample_rows", rows, ("out_tok", out_tok, torch.int64), ("out_logit", out_logit, torch.float32),
                  ("out_kept", out_kept, torch.int32), ("out_logprob", out_logprob, torch.float32))
    if out_ref_logprob is not None and (not isinstance(out_ref_logprob, torch.Tensor) or out_ref_logprob.dtype != torch.float32
                                        or out_ref_logprob.dim() != 1 or out_ref_logprob.numel() != rows or not out_ref_logprob.is_contiguous()):
        raise L.CoverError("token_sample_rows: out_ref_logprob must be contiguous torch.float32 [rows]")
    _chk_dev(logits, uniform, out_tok, out_logit, out_kept, out_logprob, out_ref_logprob)
    T, k, p = _upload_row_params(params, logits.device)
    tok = torch.empty(rows, dtype=torch.int64, device=logits.device) if out_tok is None else out_tok
    lg = torch.empty(rows, dtype=torch.float32, device=logits.device) if out_logit is None else out_logit
    kept = torch.empty(rows, dtype=torch.int32, device=logits.device) if out_kept is None else out_kept
    a = L.TokenSampleRowsArgs()
    _fill_rows(a, logits, rows, lo, hi)
    a.uniform, a.temperature, a.top_k, a.top_p = uniform.data_ptr(), T.data_ptr(), _ptr(k), _ptr(p)
    a.token_out, a.logit_out, a.kept_out, a.logprob_out = tok.data_ptr(), lg.data_ptr(), kept.data_ptr(), _ptr(out_logprob)
    if out_ref_logprob is not None:
        al = None if allow is None else C.byref(_allow_arg("token_sample_rows", allow, rows, hi, logits))
        ref = L.TokenRef()
        ref.temperature, ref.logprob_out = ref_temperature, out_ref_logprob.data_ptr()
        L.check(L.lib().cover_token_sample_rows_ref(C.byref(a), al, C.byref(ref), _stream()), "token_sample_rows_ref")
        return tok, lg, kept
    if allow is not None:
        al = _allow_arg("token_sample_rows", allow, rows, hi, logits)
        L.check(L.lib().cover_token_sample_rows_allowed(C.byref(a), C.byref(al), _stream()), "token_sample_rows_allowed")
        return tok, lg, kept
    L.check(L.lib().cover_token_sample_rows(C.byref(a), _stream()), "token_sample_rows")
    return tok, lg, kept


def token_logprob_rows(logits, lo, hi, tokens, temperature, top_k=None, top_p=None, out=None, out_kept=None, allow=None):
    """token_logprob with the parameters of every row its own (cover_token_logprob_rows; the parameter arguments as in
    token_sample_rows). A greedy row (temperature 0) is scored at temperature 1, unfiltered; a row with invalid device-side parameters
    gives NaN and kept 0. On token_sample_rows' own picks it equals that call's out_logprob bit for bit. allow = TokenAllow:
    cover_token_logprob_rows_allowed, scored under the row restricted to its set; a token that is not allowed gets -inf."""
    _chk_range("token_logprob_rows", lo, hi)
    rows = _chk_logits("token_logprob_rows", logits, hi)
    params = _row_params("token_logprob_rows", rows, temperature, top_k, top_p)
    if tokens.dtype != torch.int64 or tokens.numel() != rows or not tokens.is_contiguous():
        raise L.CoverError("token_logprob_rows: tokens must be contiguous int64 [rows]")
    _chk_rows_out("token_logprob_rows", rows, ("out", out, torch.float32), ("out_kept", out_kept, torch.int32))
    _chk_dev(logits, tokens, out, out_kept)
    T, k, p = _upload_row_params(params, logits.device)
    lp = torch.empty(rows, dtype=torch.float32, device=logits.device) if out is None else out
    a = L.TokenLogprobRowsArgs()
    _fill_rows(a, logits, rows, lo, hi)
    a.temperature, a.top_k, a.top_p = T.data_ptr(), _ptr(k), _ptr(p)
    a.token, a.logprob_out, a.kept_out = tokens.data_ptr(), lp.data_ptr(), _ptr(out_kept)
    if allow is not None:
        al = _allow_arg("token_logprob_rows", allow, rows, hi, logits)
        L.check(L.lib().cover_token_logprob_rows_allowed(C.byref(a), C.byref(al), _stream()), "token_logprob_rows_allowed")
        return lp
    L.check(L.lib().cover_token_logprob_rows(C.byref(a), _stream()), "token_logprob_rows")
    return lp


def token_topn_rows(logits, lo, hi, n, temperature, top_k=None, top_p=None, out_tok=None, out_logprob=None, out_entropy=None, out_kept=None,
                    allow=None):
    """token_topn with the parameters of every row its own (cover_token_topn_rows; the parameter arguments as in token_sample_rows).
    A greedy row (temperature 0) is ranked at temperature 1, unfiltered; a row with invalid device-side parameters gives -1 / -inf in
    every slot, entropy NaN and kept 0. Returns (tokens int64 [rows, n], logprobs fp32 [rows, n], entropy fp32 [rows]). allow = TokenAllow:
    cover_token_topn_rows_allowed, only the allowed columns of each row's set are ranked and the entropy is that of the restricted kept set."""
    _chk_range("token_topn_rows", lo, hi)
    n = _chk_topn_n("token_topn_rows", n)
    rows = _chk_logits("token_topn_rows", logits, hi)
    params = _row_params("token_topn_rows", rows, temperature, top_k, top_p)
    a = L.TokenTopnRowsArgs()
    tok, lp, ent = _topn_outputs(a, "token_topn_rows", logits, rows, n, out_tok, out_logprob, out_entropy, out_kept)
    T, k, p = _upload_row_params(params, logits.device)
    _fill_rows(a, logits, rows, lo, hi)
    a.temperature, a.top_k, a.top_p = T.data_ptr(), _ptr(k), _ptr(p)
    if allow is not None:
        al = _allow_arg("token_topn_rows", allow, rows, hi, logits)
        L.check(L.lib().cover_token_topn_rows_allowed(C.byref(a), C.byref(al), _stream()), "token_topn_rows_allowed")
        return tok, lp, ent
    L.check(L.lib().cover_token_topn_rows(C.byref(a), _stream()), "token_topn_rows")
    return tok, lp, ent


def pick_token(logits, lo, hi, uniform=None, temperature=1.0, filt=None, out_tok=None, out_logit=None, out_kept=None, out_logprob=None,
               row_params=None, allow=None, ref=None):
    """One decode step's pick over columns [lo, hi), the three-way choice of every token head. Returns (token, its logit, kept or None).
    uniform None: greedy token_select (temperature and filt are unused); uniform with filt None: token_select's unfiltered inverse-CDF
    sample; uniform with filt = (top_k, top_p): ONE token_sample call, whose kept count is returned. out_logprob fp32 [rows]: filled with
    the log-probability of each pick under the distribution it came from (greedy: temperature 1, unfiltered), by token_sample itself or
    by one token_logprob launch behind token_select. The out_* rows are the wrappers' own; no arithmetic or allocation of its own.
    row_params = (temperature, top_k, top_p) device tensors [rows]: ONE token_sample_rows call with the parameters of every row its own
    (uniform is required, temperature and filt are unused; a row with temperature 0 is greedy); its kept count is returned.
    allow = TokenAllow (with row_params only): that call restricted to each row's allowed-token set.
    ref = (T_ref, out fp32 [rows]) (with row_params only): that call also scores each pick at the reference temperature T_ref, unfiltered,
    into out (token_sample_rows' ref_temperature / out_ref_logprob)."""
    if allow is not None and row_params is None:
        raise L.CoverError("pick_token: allow needs row_params (the allowed-token sets belong to the per-row call)")
    if ref is not None and row_params is None:
        raise L.CoverError("pick_token: ref needs row_params (the reference score belongs to the per-row call)")
    if row_params is not None:
        extra = {} if allow is None else dict(allow=allow)      # None: exactly the call made before the argument existed
        if ref is not None:
            extra.update(ref_temperature=ref[0], out_ref_logprob=ref[1])
        return token_sample_rows(logits, lo, hi, uniform, row_params[0], row_params[1], row_params[2], out_tok=out_tok, out_logit=out_logit,
                                 out_kept=out_kept, out_logprob=out_logprob, **extra)
    if uniform is not None and filt is not None:
        return token_sample(logits, lo, hi, uniform, temperature=temperature, top_k=filt[0], top_p=filt[1], out_tok=out_tok,
                            out_logit=out_logit, out_kept=out_kept, out_logprob=out_logprob)
    if uniform is None:
        temperature = 1.0
    tok, lg = token_select(logits, lo, hi, uniform=uniform, temperature=temperature, out_tok=out_tok, out_logit=out_logit)
    if out_logprob is not None:
        token_logprob(logits, lo, hi, tok, temperature=temperature, out=out_logprob)
    return tok, lg, None


class TokenFsm:
    """A token-class automaton per row (cover_token_fsm), validated once on the host: class_of_token [vocab] integers in [0, n_classes),
    trans [n_states, n_classes] integers in [0, n_states), set_of_state [n_states] integers >= 0 (the allowed-set index a row in that
    state draws from; checked against a TokenAllow's n_sets by check_sets / token_fsm_check), start_state in [0, n_states). n_classes
    <= 256. Arrays, sequences or tensors; the host copies are kept as numpy (class_of_token_np, trans_np, set_of_state_np), the device
    copies are made by to(device) once. Regular grammars only: no stack, nothing across rows."""

    def __init__(self, class_of_token, trans, set_of_state, start_state=0):
        def host(v, what):
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            if v.dtype.kind not in "iub" or v.size == 0:
                raise L.CoverError(f"TokenFsm: {what} must be a non-empty integer array")
            return v.astype(np.int64)
        cls, tr, sos = host(class_of_token, "class_of_token"), host(trans, "trans"), host(set_of_state, "set_of_state")
        if cls.ndim != 1 or tr.ndim != 2 or sos.ndim != 1 or sos.shape[0] != tr.shape[0]:
            raise L.CoverError("TokenFsm: class_of_token is [vocab], trans [n_states, n_classes] and set_of_state [n_states]")
        n_states, n_classes = tr.shape
        if not 1 <= n_classes <= 256:
            raise L.CoverError(f"TokenFsm: 1 <= n_classes <= 256 is required (got {n_classes})")
        if cls.min() < 0 or cls.max() >= n_classes:
            raise L.CoverError(f"TokenFsm: every class_of_token entry must lie in [0, {n_classes})")
        if tr.min() < 0 or tr.max() >= n_states:
            raise L.CoverError(f"TokenFsm: every trans entry must lie in [0, {n_states})")
        if sos.min() < 0:
            raise L.CoverError("TokenFsm: every set_of_state entry must be >= 0")
        if not 0 <= int(start_state) < n_states:
            raise L.CoverError(f"TokenFsm: start_state must lie in [0, {n_states})")
        self.class_of_token_np, self.trans_np, self.set_of_state_np = cls.astype(np.uint8), tr.astype(np.int32), sos.astype(np.int32)
        self.n_states, self.n_classes, self.vocab, self.start_state = int(n_states), int(n_classes), int(cls.shape[0]), int(start_state)
        self.class_of_token = self.trans = self.set_of_state = None      # device tensors, made by to()

    def to(self, device):
        """Upload the three tables to device (once per device); returns self."""
        device = torch.device(device)
        if self.trans is None or self.trans.device != device:
            self.class_of_token = torch.from_numpy(self.class_of_token_np).to(device)
            self.trans = torch.from_numpy(self.trans_np).to(device)
            self.set_of_state = torch.from_numpy(self.set_of_state_np).to(device)
        return self

    def check_sets(self, allow):
        """Every set_of_state entry names a set of allow (a TokenAllow): CoverError otherwise."""
        if not isinstance(allow, TokenAllow):
            raise L.CoverError("TokenFsm: allow must be an ops.TokenAllow")
        if int(self.set_of_state_np.max()) >= allow.n_sets:
            raise L.CoverError(f"TokenFsm: every set_of_state entry must lie in [0, {allow.n_sets}) (the TokenAllow's n_sets)")

    def rows(self, n, device):
        """(state int32 [n] = start_state, set_of_row int32 [n] = set_of_state[start_state]) on device: the two per-row tensors of a decode.
        set_of_row is what the TokenAllow of the picks takes; decode_feedback(fsm=) rewrites both every step."""
        self.to(device)
        state = torch.full((int(n),), self.start_state, dtype=torch.int32, device=device)
        return state, torch.full((int(n),), int(self.set_of_state_np[self.start_state]), dtype=torch.int32, device=device)

    def step_torch(self, state, set_of_row, tokens, live):
        """The update of cover_decode_feedback_fsm in device tensors, in place (the models' unfused path and the fused kernel's in-repo
        reference): state = where(live & valid, trans[state, class_of_token[t]], state); set_of_row = set_of_state[state] (-1 for a state
        outside [0, n_states)). tokens int64 [rows] the emitted ids, live bool [rows] = not done before the step. No host round trip."""
        ok_s = (state >= 0) & (state < self.n_states)
        move = live & ok_s & (tokens >= 0) & (tokens < self.vocab)
        cls = self.class_of_token[tokens.clamp(0, self.vocab - 1)].to(torch.int64)
        s64 = state.clamp(0, self.n_states - 1).to(torch.int64)
        state.copy_(torch.where(move, self.trans[s64, cls], state))
        ok_s = (state >= 0) & (state < self.n_states)
        set_of_row.copy_(torch.where(ok_s, self.set_of_state[state.clamp(0, self.n_states - 1).to(torch.int64)], torch.full_like(set_of_row, -1)))


def token_fsm_check(fsm, allow, lo, hi):
    """Host check of a grammar before it drives a decode: every state reachable from fsm.start_state must have at least one allowed
    column in [lo, hi) in its set, walking only along classes that have an allowed token (in [lo, hi)) in the state's set. CoverError
    naming the dead state otherwise: a row that reached it would be the invalid row (-1 / NaN) of the _allowed kernels. One read-back
    of allow.bits; returns the sorted list of reachable states."""
    if not isinstance(fsm, TokenFsm):
        raise L.CoverError("token_fsm_check: fsm must be an ops.TokenFsm")
    fsm.check_sets(allow)
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi or hi > fsm.vocab or hi > allow.bits.shape[1] * 32:
        raise L.CoverError(f"token_fsm_check: 0 <= lo < hi <= vocab ({fsm.vocab}) within the words of allow.bits is required (got lo={lo}, hi={hi})")
    words = np.ascontiguousarray(allow.bits.detach().cpu().view(torch.int32).numpy()).view(np.uint32)
    on = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, lo:hi].astype(bool)       # [n_sets, hi - lo]
    cls = fsm.class_of_token_np[lo:hi]
    seen, todo = {fsm.start_state}, [fsm.start_state]
    while todo:
        s = todo.pop()
        live = np.unique(cls[on[fsm.set_of_state_np[s]]])
        if live.size == 0:
            raise L.CoverError(f"token_fsm_check: state {s} is reachable from state {fsm.start_state} and its set "
                               f"{int(fsm.set_of_state_np[s])} allows no column in [{lo}, {hi})")
        for n in fsm.trans_np[s, live]:
            if int(n) not in seen:
                seen.add(int(n))
                todo.append(int(n))
    return sorted(seen)


def decode_feedback(pick, done, tok_out, step, eos, pad, force=None, lp=None, lp_out=None, table=None, scale=1.0, x_out=None,
                    live=None, lp2=None, lp2_out=None, fsm=None, fsm_state=None, fsm_set_of_row=None):
    """The bookkeeping between two decode steps in one launch (cover_decode_feedback). Per row b: t = force[b] if given else pick[b];
    lp_out[b, step] = 0.0 if done[b] else lp[b]; t = pad if done[b]; tok_out[b, step] = t; done[b] |= t == eos;
    x_out[b] = bf16(table[t] * scale) (embed_gather on the emitted ids; an id outside the table gives a zero row); live[step] += not done[b].
    pick int64 [rows] contiguous; done torch.bool [rows], in place; tok_out int64 / lp_out fp32 [rows, >= step + 1] with unit column
    stride (any row stride); force int64 [rows] with any stride (a column view); live int32 [>= step + 1], zeroed by the caller.
    x_out bf16 [rows, dim] or None (no embedding: the last step). Recordable, no workspace. Returns x_out.
    lp2 / lp2_out (together; shapes as lp / lp_out): a second log-probability column settled the same way in the same launch
    (cover_decode_feedback_lp2), lp2_out[b, step] = 0.0 if done[b] else lp2[b]; both None issues exactly cover_decode_feedback.
    fsm = TokenFsm with fsm_state / fsm_set_of_row int32 [rows] (all three together; TokenFsm.rows makes the two tensors): the launch is
    cover_decode_feedback_fsm, which also advances each live row's automaton on its emitted token (fsm_state, in place) and writes
    fsm_set_of_row[b] = set_of_state[state[b]] -- the set_of_row of the next pick's TokenAllow. A table, if given, has fsm.vocab rows.
    Without the three it launches exactly what it launched before."""
    if (lp2 is None) != (lp2_out is None):
        raise L.CoverError("decode_feedback: lp2 and lp2_out are given together")
    if (fsm is None) != (fsm_state is None) or (fsm is None) != (fsm_set_of_row is None):
        raise L.CoverError("decode_feedback: fsm, fsm_state and fsm_set_of_row are given together")
    _chk_dev(pick, done, tok_out, force, lp, lp_out, table, x_out, live, lp2, lp2_out, fsm_state, fsm_set_of_row)
    rows = pick.numel()
    assert pick.dtype == torch.int64 and pick.is_contiguous() and done.dtype == torch.bool and done.is_contiguous() and done.numel() == rows
    assert tok_out.dtype == torch.int64 and tok_out.dim() == 2 and tok_out.shape[0] == rows and 0 <= step < tok_out.shape[1]
    assert tok_out.stride(1) == 1 or tok_out.shape[1] == 1
    if (lp is None) != (lp_out is None):
        raise L.CoverError("decode_feedback: lp and lp_out are given together")
    a = L.DecodeFeedbackArgs()
    a.pick, a.done, a.rows = pick.data_ptr(), done.data_ptr(), rows
    a.tok_out, a.ld_tok = tok_out.data_ptr() + 8 * step, tok_out.stride(0)
    a.eos, a.pad = int(eos), int(pad)
    if force is not None:
        assert force.dtype == torch.int64 and force.dim() == 1 and force.numel() == rows
        a.force, a.force_stride = force.data_ptr(), force.stride(0)
    if lp is not None:
        assert lp.dtype == torch.float32 and lp.is_contiguous() and lp.numel() == rows
        assert lp_out.dtype == torch.float32 and lp_out.dim() == 2 and lp_out.shape[0] == rows and step < lp_out.shape[1]
        assert lp_out.stride(1) == 1 or lp_out.shape[1] == 1
        a.lp, a.lp_out, a.ld_lp = lp.data_ptr(), lp_out.data_ptr() + 4 * step, lp_out.stride(0)
    if x_out is not None:
        if table is None:
            raise L.CoverError("decode_feedback: x_out needs the embedding table")
        assert table.dtype == torch.bfloat16 and table.dim() == 2 and table.is_contiguous()
        assert x_out.dtype == torch.bfloat16 and x_out.dim() == 2 and x_out.shape == (rows, table.shape[1]) and x_out.stride(1) == 1
        a.table, a.vocab, a.dim, a.scale = table.data_ptr(), table.shape[0], table.shape[1], scale
        a.x_out, a.ldo = x_out.data_ptr(), x_out.stride(0)
    if live is not None:
        assert live.dtype == torch.int32 and live.dim() == 1 and live.is_contiguous() and step < live.numel()
        a.live = live.data_ptr() + 4 * step
    if lp2 is not None:
        assert lp2.dtype == torch.float32 and lp2.is_contiguous() and lp2.numel() == rows
        assert lp2_out.dtype == torch.float32 and lp2_out.dim() == 2 and lp2_out.shape[0] == rows and step < lp2_out.shape[1]
        assert lp2_out.stride(1) == 1 or lp2_out.shape[1] == 1
    if fsm is not None:
        if not isinstance(fsm, TokenFsm):
            raise L.CoverError("decode_feedback: fsm must be an ops.TokenFsm")
        for name, t in (("fsm_state", fsm_state), ("fsm_set_of_row", fsm_set_of_row)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != rows or not t.is_contiguous():
                raise L.CoverError(f"decode_feedback: {name} must be a contiguous int32 tensor [rows]")
        if table is not None and x_out is not None and table.shape[0] != fsm.vocab:
            raise L.CoverError(f"decode_feedback: the table has {table.shape[0]} rows, fsm.class_of_token {fsm.vocab} entries")
        fsm.to(pick.device)
        a.vocab = fsm.vocab
        f = L.TokenFsm()
        f.class_of_token, f.trans, f.set_of_state = fsm.class_of_token.data_ptr(), fsm.trans.data_ptr(), fsm.set_of_state.data_ptr()
        f.n_states, f.n_classes, f.state, f.set_of_row = fsm.n_states, fsm.n_classes, fsm_state.data_ptr(), fsm_set_of_row.data_ptr()
        l2 = (None, None, 0) if lp2 is None else (lp2.data_ptr(), lp2_out.data_ptr() + 4 * step, lp2_out.stride(0))
        L.check(L.lib().cover_decode_feedback_fsm(C.byref(a), C.byref(f), l2[0], l2[1], l2[2], _stream()), "decode_feedback_fsm")
        return x_out
    if lp2 is not None:
        L.check(L.lib().cover_decode_feedback_lp2(C.byref(a), lp2.data_ptr(), lp2_out.data_ptr() + 4 * step, lp2_out.stride(0), _stream()),
                "decode_feedback_lp2")
        return x_out
    L.check(L.lib().cover_decode_feedback(C.byref(a), _stream()), "decode_feedback")
    return x_out


def score_select(it, act, group_size):
    """it [members, dim], act [members, N, dim] fp32 -> (scores [N], result int32[4], best f32[2], fused_it, fused_act). result / best are
    group_argmax's on scores, NaN rule included (members that cancel average to a zero vector, whose score is 0 / 0)."""
    _chk_dev(it, act)
    m, N, dim = act.shape
    dev = it.device
    scores = torch.empty(N, dtype=torch.float32, device=dev)
    result = torch.empty(4, dtype=torch.int32, device=dev)
    best = torch.empty(2, dtype=torch.float32, device=dev)
    fit = torch.empty(dim, dtype=torch.float32, device=dev)
    fact = torch.empty(N, dim, dtype=torch.float32, device=dev)
    a = L.ScoreSelectArgs()
    a.it, a.act = it.contiguous().data_ptr(), act.contiguous().data_ptr()
    a.n_members, a.N, a.dim, a.group_size = m, N, dim, group_size
    a.scores_out, a.result_out, a.best_out = scores.data_ptr(), result.data_ptr(), best.data_ptr()
    a.fused_it_out, a.fused_act_out = fit.data_ptr(), fact.data_ptr()
    L.check(L.lib().cover_score_select(C.byref(a), _stream()), "score_select")
    return scores, result, best, fit, fact


def tokens_to_histories(tokens, tok_vocab, centers, past, pad_value=-5.0, n_use=1):
    """tokens int64 [N, >= 7 n_use] (device), centers fp32 [n_centers], past fp32 [n_past, 7] -> (hist fp32 [N,10,7], pad uint8
    [N,10]); n_use = how many 7-token actions of a candidate's chunk become history rows (action-chunk horizon > 1)."""
    _chk_dev(tokens, centers)
    N = tokens.shape[0]
    hist = torch.empty(N, 10, 7, dtype=torch.float32, device=tokens.device)
    pad = torch.empty(N, 10, dtype=torch.uint8, device=tokens.device)
    n_past = 0 if past is None else past.shape[0]
    L.check(L.lib().cover_tokens_to_histories_steps(tokens.data_ptr(), tokens.stride(0), N, tok_vocab, centers.data_ptr(),
                                                    centers.numel(), _ptr(past), n_past, n_use, pad_value, hist.data_ptr(),
                                                    pad.data_ptr(), _stream()), "tokens_to_histories")
    return hist, pad


def actions_to_histories(actions, n_use, past, lo_hi=None, pad_value=-5.0):
    """actions fp32 [N, chunk, >=7] (device, normalised policy output), past fp32 [n_past, 7], lo_hi fp32 [12] (p01[:6] | p99[:6])
    or None -> (hist fp32 [N,10,7], pad uint8 [N,10]): the verifier histories of a flow-matching policy's chunks."""
    _chk_dev(actions)
    assert actions.dtype == torch.float32 and actions.stride(2) == 1
    N = actions.shape[0]
    hist = torch.empty(N, 10, 7, dtype=torch.float32, device=actions.device)
    pad = torch.empty(N, 10, dtype=torch.uint8, device=actions.device)
    n_past = 0 if past is None else past.shape[0]
    L.check(L.lib().cover_actions_to_histories(actions.data_ptr(), actions.stride(0), actions.stride(1), N, n_use, _ptr(lo_hi),
                                               _ptr(past), n_past, pad_value, hist.data_ptr(), pad.data_ptr(), _stream()),
            "actions_to_histories")
    return hist, pad


def group_argmax(scores, group_size):
    """scores fp32 [N] -> (result int32 [4] = {global index, group, index in group, 0}, best fp32 [2] = {that score, its group's mean}):
    cover_group_argmax, first maximum wins at both levels. A NaN never wins; where nothing wins (every group mean a NaN, or the taken
    group all NaN) the pick is index 0, so result is always in range and best carries the picked values' own bits."""
    _chk_dev(scores)
    result = torch.empty(4, dtype=torch.int32, device=scores.device)
    best = torch.empty(2, dtype=torch.float32, device=scores.device)
    L.check(L.lib().cover_group_argmax(scores.data_ptr(), scores.numel(), group_size, result.data_ptr(), best.data_ptr(),
                                       _stream()), "group_argmax")
    return result, best


def prior_select(scores, logprobs, group_size, beta, *, tokens=None, pad_token_id=None, length_normalize=False, top_m=0):
    """Grouped arg-max of scores + beta * sequence log-probability, with the best top_m of the winning group (cover_prior_select).
    scores fp32 [N] contiguous; logprobs fp32 [N] (a prior that is summed already) or [N, steps] with ANY strides -- the candidate-major
    tensor OpenVLA.sample / generate_tokens return, or the transposed view of a step-major [steps, N] buffer: strides are passed, nothing
    is copied. tokens int64 of logprobs' shape (any strides) with pad_token_id: steps whose token is the pad are not counted;
    length_normalize divides the sum by the number of counted steps (at least 1). Returns a dict of device tensors: prior [N], combined
    [N], group_mean [N / group_size], result int32 [4] and best fp32 [2] as group_argmax gives them (on combined), ranked int32 [top_m]
    global indices by descending combined score, equal values by ascending index. The prior is one fp32 chain of adds in step order and
    combined = scores exactly when beta == 0, else round(scores + round(beta * prior)): the results are fixed bit patterns.
    One launch, no workspace, recordable."""
    import math
    if not (torch.is_tensor(scores) and torch.is_tensor(logprobs)) or scores.dtype != torch.float32 or logprobs.dtype != torch.float32:
        raise L.CoverError("prior_select: scores and logprobs must be fp32 tensors")
    if scores.dim() != 1 or scores.numel() < 1 or not scores.is_contiguous():
        raise L.CoverError("prior_select: scores must be contiguous fp32 [N], N >= 1")
    N = scores.numel()
    if logprobs.dim() not in (1, 2) or logprobs.shape[0] != N or (logprobs.dim() == 2 and not 1 <= logprobs.shape[1] <= 4096):
        raise L.CoverError(f"prior_select: logprobs must be [N] or [N, 1..4096 steps] with N = {N} (got {tuple(logprobs.shape)})")
    steps = 1 if logprobs.dim() == 1 else logprobs.shape[1]
    if (tokens is None) != (pad_token_id is None):
        raise L.CoverError("prior_select: tokens and pad_token_id are given together")
    if tokens is not None and (not torch.is_tensor(tokens) or tokens.dtype != torch.int64 or tokens.shape != logprobs.shape):
        raise L.CoverError("prior_select: tokens must be int64 of logprobs' shape")
    group_size, top_m = int(group_size), int(top_m)
    if group_size < 1 or N % group_size != 0 or N // group_size > 4096 or group_size > 4096:
        raise L.CoverError(f"prior_select: N % group_size == 0, N / group_size <= 4096 and group_size <= 4096 are required "
                           f"(got N={N}, group_size={group_size})")
    if not 0 <= top_m <= min(group_size, 64):
        raise L.CoverError(f"prior_select: 0 <= top_m <= min(group_size, 64) is required (got top_m={top_m}, group_size={group_size})")
    beta = float(beta)
    if not (math.isfinite(beta) and beta >= 0.0 and math.isfinite(C.c_float(beta).value)):
        raise L.CoverError(f"prior_select: beta must be finite and >= 0 (got {beta})")
    _chk_dev(scores, logprobs, tokens)
    if logprobs.device != scores.device or (tokens is not None and tokens.device != scores.device):
        raise L.CoverError("prior_select: scores, logprobs and tokens must be on one device")
    dev = scores.device
    out = {"prior": torch.empty(N, dtype=torch.float32, device=dev), "combined": torch.empty(N, dtype=torch.float32, device=dev),
           "group_mean": torch.empty(N // group_size, dtype=torch.float32, device=dev),
           "result": torch.empty(4, dtype=torch.int32, device=dev), "best": torch.empty(2, dtype=torch.float32, device=dev),
           "ranked": torch.empty(top_m, dtype=torch.int32, device=dev)}
    a = L.PriorSelectArgs()
    a.scores, a.logprobs = scores.data_ptr(), logprobs.data_ptr()
    a.lp_n_stride, a.lp_t_stride = logprobs.stride(0), (logprobs.stride(1) if logprobs.dim() == 2 else 0)
    if tokens is not None:
        a.tokens, a.pad_token_id = tokens.data_ptr(), int(pad_token_id)
        a.tok_n_stride, a.tok_t_stride = tokens.stride(0), (tokens.stride(1) if tokens.dim() == 2 else 0)
    a.N, a.steps, a.group_size, a.top_m, a.beta, a.length_normalize = N, steps, group_size, top_m, beta, int(bool(length_normalize))
    a.prior_out, a.combined_out, a.group_mean_out = out["prior"].data_ptr(), out["combined"].data_ptr(), out["group_mean"].data_ptr()
    a.result_out, a.best_out, a.ranked_out = out["result"].data_ptr(), out["best"].data_ptr(), (out["ranked"].data_ptr() if top_m else None)
    L.check(L.lib().cover_prior_select(C.byref(a), _stream()), "prior_select")
    return out


MEMBER_MODES = {"lcb": 0, "min": 1}


def member_scores(it, act, scores, group_size, kappa=0.0, mode="lcb"):
    """Per-member scores of the verifier ensemble and a disagreement-aware score (cover_member_scores). it fp32 [M, dim] and act fp32
    [M, N, dim] are the per-member unit rows score_select takes, scores fp32 [N] the fused scores it returned (read, never written); all
    contiguous, on one device, 1 <= M <= 16, 1 <= dim <= 4096. Returns a dict of device tensors: member_scores [M, N] (member m's own
    cosine for every candidate), mean [N], spread [N] (the population standard deviation over the members; exactly 0 for M = 1), min [N]
    and min_member int32 [N] (the first member that attains it), robust [N], result int32 [4] / best fp32 [2] as group_argmax gives
    them on robust, member_result int32 [M, 4] / member_best fp32 [M, 2] as group_argmax gives them on each member's row.
    mode "lcb": robust = scores exactly when kappa == 0, else round(scores - round(kappa * spread)); mode "min": robust = min, and kappa
    must be 0. kappa is finite and >= 0; no default penalty is recommended. Every sum is one fixed fp32 chain (include/cover_hip.h), so
    the results are fixed bit patterns. Two launches, no workspace, recordable."""
    import math
    if not all(torch.is_tensor(t) and t.dtype == torch.float32 for t in (it, act, scores)):
        raise L.CoverError("member_scores: it, act and scores must be fp32 tensors")
    if it.dim() != 2 or act.dim() != 3 or scores.dim() != 1:
        raise L.CoverError(f"member_scores: it [M, dim], act [M, N, dim] and scores [N] are required (got {tuple(it.shape)}, "
                           f"{tuple(act.shape)}, {tuple(scores.shape)})")
    M, N, dim = act.shape
    if tuple(it.shape) != (M, dim) or scores.numel() != N:
        raise L.CoverError(f"member_scores: it {tuple(it.shape)} and scores {tuple(scores.shape)} do not match act {tuple(act.shape)}")
    if not (it.is_contiguous() and act.is_contiguous() and scores.is_contiguous()):
        raise L.CoverError("member_scores: it, act and scores must be contiguous")
    if not 1 <= M <= 16 or N < 1 or not 1 <= dim <= 4096:
        raise L.CoverError(f"member_scores: 1 <= M <= 16, N >= 1 and 1 <= dim <= 4096 are required (got M={M}, N={N}, dim={dim})")
    group_size = int(group_size)
    if group_size < 1 or N % group_size != 0 or N // group_size > 4096:
        raise L.CoverError(f"member_scores: N % group_size == 0 and N / group_size <= 4096 are required (got N={N}, group_size={group_size})")
    if mode not in MEMBER_MODES:
        raise L.CoverError(f"member_scores: mode must be 'lcb' or 'min' (got {mode!r})")
    kappa = float(kappa)
    if not (math.isfinite(kappa) and kappa >= 0.0 and math.isfinite(C.c_float(kappa).value)):
        raise L.CoverError(f"member_scores: kappa must be finite and >= 0 (got {kappa})")
    if mode == "min" and kappa != 0.0:
        raise L.CoverError(f"member_scores: mode 'min' takes no penalty, kappa must be 0 (got {kappa})")
    _chk_dev(it, act, scores)
    if act.device != it.device or scores.device != it.device:
        raise L.CoverError("member_scores: it, act and scores must be on one device")
    dev = it.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"member_scores": torch.empty(M, N, **f32), "mean": torch.empty(N, **f32), "spread": torch.empty(N, **f32),
           "min": torch.empty(N, **f32), "min_member": torch.empty(N, **i32), "robust": torch.empty(N, **f32),
           "result": torch.empty(4, **i32), "best": torch.empty(2, **f32),
           "member_result": torch.empty(M, 4, **i32), "member_best": torch.empty(M, 2, **f32)}
    a = L.MemberScoresArgs()
    a.it, a.act, a.scores = it.data_ptr(), act.data_ptr(), scores.data_ptr()
    a.n_members, a.N, a.dim, a.group_size, a.kappa, a.mode = M, N, dim, group_size, kappa, MEMBER_MODES[mode]
    for k, t in out.items():
        setattr(a, k + "_out", t.data_ptr())
    L.check(L.lib().cover_member_scores(C.byref(a), _stream()), "member_scores")
    return out


# ------------------------------------------------------------------------------------------------ proposal augmentation
class AugmentStats(NamedTuple):
    """What augment_tokens / augment_actions return beside the output with stats=True."""
    mean: torch.Tensor     # fp32 [G, steps, 6]
    sd: torch.Tensor       # fp32 [G, steps, 6], after the floor
    votes: torch.Tensor    # int32 [G, steps, 2]: (class-0 count, class-1 count) of the gripper vote


def _augment_stats(G, steps, dev):
    return AugmentStats(torch.empty(G, steps, 6, dtype=torch.float32, device=dev), torch.empty(G, steps, 6, dtype=torch.float32, device=dev),
                        torch.empty(G, steps, 2, dtype=torch.int32, device=dev))


class _Rows(NamedTuple):
    """The candidate rows of one call, as _token_rows / _action_rows found them: what every kernel over candidate rows is told of them."""
    what: str                           # the public function's name, for the messages
    src: torch.Tensor
    elem: torch.dtype                   # int64 (tokens) or fp32 (actions)
    n_stride: int                       # row stride, in elements
    t_stride: int                       # step stride, in elements
    N: int
    steps: int
    centers: Optional[torch.Tensor]     # tokens: fp32 [n_centers]
    tok_vocab: int

    def out_shape(self, R):
        """The shape of a gathered output of R rows."""
        return (R, 7 * self.steps) if self.elem == torch.int64 else (R, self.steps, 7)

    def fill(self, a):
        """The row fields of any of the six argument structs."""
        a.src, a.n_stride, a.t_stride = self.src.data_ptr(), self.n_stride, self.t_stride
        if self.centers is not None:
            a.centers, a.n_centers, a.tok_vocab = self.centers.data_ptr(), self.centers.numel(), int(self.tok_vocab)


def _token_rows(what, tokens, steps, centers, tok_vocab):
    """The input checks of the token forms -> their _Rows."""
    if not torch.is_tensor(tokens) or tokens.dtype != torch.int64 or tokens.dim() != 2 or (tokens.shape[1] > 1 and tokens.stride(1) != 1):
        raise L.CoverError(f"{what}: tokens must be int64 [rows, >= 7 steps] with unit column stride")
    steps = int(steps)
    if steps < 1 or tokens.shape[1] < 7 * steps or (tokens.shape[0] > 1 and tokens.stride(0) < 7 * steps):
        raise L.CoverError(f"{what}: steps >= 1 and 7 * steps <= columns are required (got steps={steps}, tokens {tuple(tokens.shape)})")
    if not torch.is_tensor(centers) or centers.dtype != torch.float32 or centers.dim() != 1 or centers.numel() < 1 or not centers.is_contiguous():
        raise L.CoverError(f"{what}: centers must be contiguous fp32 [n_centers >= 1]")
    return _Rows(what, tokens, torch.int64, max(tokens.stride(0), 7 * steps), 7, tokens.shape[0], steps, centers, tok_vocab)


def _action_rows(what, actions):
    """The input check of the float forms -> their _Rows."""
    if not torch.is_tensor(actions) or actions.dtype != torch.float32 or actions.dim() != 3 or actions.shape[2] < 7 or actions.stride(2) != 1:
        raise L.CoverError(f"{what}: actions must be fp32 [rows, steps, >= 7] with unit last stride")
    return _Rows(what, actions, torch.float32, actions.stride(0), actions.stride(1), actions.shape[0], actions.shape[1], None, 0)


# The checks the families share, each stated once. A family's own conditions (n_fit <= group_rows, radius > 0, ...) stay in its helper.
def _chk_ints(what, **named):
    """Integers, bools rejected -> the ints, in the order given."""
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in named.values()):
        raise L.CoverError(f"{what}: {', '.join(named)} must be integers (got {', '.join(repr(v) for v in named.values())})")
    return tuple(int(v) for v in named.values())


def _chk_groups(rows, group_rows):
    """rows in prompt groups of group_rows -> (G, S)."""
    what, N = rows.what, rows.N
    S, = _chk_ints(what, group_rows=group_rows)
    if not 1 <= S <= 4096 or N < 1 or N % S != 0:
        raise L.CoverError(f"{what}: 1 <= group_rows <= 4096 and rows % group_rows == 0 are required (got rows={N}, group_rows={S})")
    if not 1 <= rows.steps <= 64 or N > 1 << 20:
        raise L.CoverError(f"{what}: 1 <= steps <= 64 and rows <= 2^20 are required (got steps={rows.steps}, rows={N})")
    return N // S, S


def _chk_f32(what, name, t, *shapes, hint=""):
    """t: a contiguous fp32 tensor of one of the shapes."""
    if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) not in shapes or not t.is_contiguous():
        raise L.CoverError(f"{what}: {name} must be contiguous fp32 {' or '.join(str(list(s)) for s in shapes)}{hint} "
                           f"(got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__})")


def _f32_number(what, name, v, finite=True):
    """A Python or numpy number, bools rejected, finite (finite=False: anything but a NaN) -> the fp32 value the launch receives, which
    may be +-inf or 0 where v is not: the range conditions are the caller's."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or (not math.isfinite(v) if finite else math.isnan(v)):
        raise L.CoverError(f"{what}: {name} must be a {'finite ' if finite else ''}number (got {v!r})")
    return C.c_float(float(v)).value


def _dim_scale_for(what, dim_scale, src):
    """dim_scale as the fp32 [6] tensor the launch reads, on src's device: a device tensor (host.Smooth's, host.Coherence's,
    host.Diversity's upload: validated there, once) as it is, anything else through smooth_dim_scale."""
    if torch.is_tensor(dim_scale) and dim_scale.is_cuda:
        if dim_scale.dtype != torch.float32 or tuple(dim_scale.shape) != (6,) or not dim_scale.is_contiguous():
            raise L.CoverError(f"{what}: a device dim_scale must be contiguous fp32 [6]")
    else:
        dim_scale = torch.from_numpy(smooth_dim_scale(dim_scale.detach().numpy() if torch.is_tensor(dim_scale) else dim_scale, what))
    return dim_scale.to(src.device)


def _out_or_new(what, out, shape, dtype, src):
    """out, checked, or a new tensor of that shape beside src."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=src.device)
    if not torch.is_tensor(out) or out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise L.CoverError(f"{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)}")
    return out


def _one_device(what, src, *others):
    """Every tensor of the call (None = not given) is on src's device, which is a GPU -> that device."""
    _chk_dev(src, *others)
    if any(t is not None and t.device != src.device for t in others):
        raise L.CoverError(f"{what}: every tensor must be on one device")
    return src.device


def _launch(rows, fn, a):
    rows.fill(a)
    L.check(getattr(L.lib(), fn)(C.byref(a), _stream()), rows.what)


def _draw_checks(what, normals, G, K, steps, sigma, sd_floor, clip):
    """The checks of what a draw takes (augment_*, refine_*): the normals' layout and the values -> (sigma, sd_floor, clip lo, clip hi)."""
    _chk_f32(what, "normals", normals, (G, K, steps, 6), hint=" = [prompts, n_augmented, steps, 6]")
    sigma, sd_floor = float(sigma), float(sd_floor)
    for name, v in (("sigma", sigma), ("sd_floor", sd_floor)):
        if not (math.isfinite(v) and v >= 0.0 and math.isfinite(C.c_float(v).value)):
            raise L.CoverError(f"{what}: {name} must be finite and >= 0 (got {v})")
    try:
        lo, hi = (float(v) for v in clip)
    except (TypeError, ValueError):
        raise L.CoverError(f"{what}: clip must be a (lo, hi) pair") from None
    if not lo <= hi:
        raise L.CoverError(f"{what}: clip lo <= hi is required, +-inf = no clip (got {clip})")
    return sigma, sd_floor, lo, hi


def _augment(rows, fn, n_samples, n_augmented, normals, sigma, sd_floor, clip, out, stats):
    """The checks and the launch both augment wrappers share."""
    what, N, steps = rows.what, rows.N, rows.steps
    n, K = int(n_samples), int(n_augmented)
    if not 1 <= n <= 4096 or not 0 <= K <= 4096 or N < 1 or N % n != 0:
        raise L.CoverError(f"{what}: 1 <= n_samples <= 4096, 0 <= n_augmented <= 4096 and rows % n_samples == 0 are required "
                           f"(got rows={N}, n_samples={n}, n_augmented={K})")
    G, S = N // n, n + K
    if not 1 <= steps <= 64 or G * S > 1 << 20:
        raise L.CoverError(f"{what}: 1 <= steps <= 64 and prompts * (n_samples + n_augmented) <= 2^20 are required (got steps={steps}, "
                           f"prompts={G})")
    sigma, sd_floor, lo, hi = _draw_checks(what, normals, G, K, steps, sigma, sd_floor, clip)
    out = _out_or_new(what, out, rows.out_shape(G * S), rows.elem, rows.src)
    dev = _one_device(what, rows.src, normals, rows.centers, out)
    st = _augment_stats(G, steps, dev) if stats else None
    a = L.AugmentArgs()
    a.normals = normals.data_ptr() if K else None
    a.G, a.n, a.K, a.h = G, n, K, steps
    a.sigma, a.sd_floor, a.clip_lo, a.clip_hi = sigma, sd_floor, lo, hi
    a.out = out.data_ptr()
    if st is not None:
        a.mean_out, a.sd_out, a.votes_out = st.mean.data_ptr(), st.sd.data_ptr(), st.votes.data_ptr()
    _launch(rows, fn, a)
    return (out, st) if stats else out


def augment_tokens(tokens, n_samples, n_augmented, normals, centers, tok_vocab, *, steps=1, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0),
                   out=None, stats=False):
    """Gaussian proposal augmentation of action tokens (cover_augment_tokens): tokens int64 [G * n_samples, >= 7 steps] (unit column
    stride, any row stride; candidate i belongs to prompt i // n_samples) -> int64 [G * S, 7 steps], S = n_samples + n_augmented. Per
    prompt, rows 0..n_samples-1 are the input rows verbatim; the n_augmented rows behind them are drawn per (step, dim < 6) from the
    Gaussian fitted to the samples' de-tokenised values centers[clamp(tok_vocab - token - 1)] -- fp32 chain mean, sd with ddof 1 (0 for
    one sample) floored at sd_floor, v = mean + (sigma * sd) * normals[g, k, t, d] clipped to clip = (lo, hi) -- and stored as the token
    of the nearest centre (first minimum). A NaN normal lands on clip lo. The gripper token of every augmented row is that of the
    lowest-index sample in the majority class (value >= 0.5, the verifier's rule); ON A TIE THE CLASS OF SAMPLE 0 WINS. normals fp32
    [G, n_augmented, steps, 6] (host.augmentation_normals): the same normals give the same tokens. centers fp32 [n_centers].
    Downstream code takes the result as it takes sampled tokens, with group_size = S. stats=True -> (out, AugmentStats).
    One launch, no workspace, recordable."""
    rows = _token_rows("augment_tokens", tokens, steps, centers, tok_vocab)
    return _augment(rows, "cover_augment_tokens", n_samples, n_augmented, normals, sigma, sd_floor, clip, out, stats)


def augment_actions(actions, n_samples, n_augmented, normals, *, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0), out=None, stats=False):
    """The same for a flow-matching policy's chunks (cover_augment_actions): actions fp32 [G * n_samples, steps, >= 7] with unit last
    stride and any other strides -- a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place -> contiguous fp32 [G * S, steps, 7].
    The first n_samples rows per prompt are the input's first 7 dims bit for bit; augmented values are stored as they are (clipped to
    clip; +-inf = no clip), the gripper float is that of the lowest-index sample in the majority class (>= 0.5), a tie going to the class
    of sample 0. See augment_tokens for the arithmetic."""
    rows = _action_rows("augment_actions", actions)
    return _augment(rows, "cover_augment_actions", n_samples, n_augmented, normals, sigma, sd_floor, clip, out, stats)


# ------------------------------------------------------------------------------------------------ proposal log-density prior
def _proposal_prior(rows, fn, group_rows, n_fit, sigma, sd_floor, log_share, out, stats):
    """The checks and the launch both proposal-prior wrappers share."""
    what, N, steps = rows.what, rows.N, rows.steps
    n, = _chk_ints(what, n_fit=n_fit)
    G, S = _chk_groups(rows, group_rows)
    if not 1 <= n <= S:
        raise L.CoverError(f"{what}: 1 <= n_fit <= group_rows is required (got group_rows={S}, n_fit={n})")
    sigma, sd_floor = _f32_number(what, "sigma", sigma), _f32_number(what, "sd_floor", sd_floor)
    for name, v in (("sigma", sigma), ("sd_floor", sd_floor)):
        if not (math.isfinite(v) and v > 0.0):
            raise L.CoverError(f"{what}: {name} must be finite and > 0 in fp32 (got {v})")
    if not C.c_float(sigma * sd_floor).value > 0.0:
        raise L.CoverError(f"{what}: the fp32 product sigma * sd_floor must be > 0 (got {sigma} * {sd_floor})")
    if log_share is not None:
        _chk_f32(what, "log_share", log_share, (n + 1,), hint=" = [n_fit + 1] (host.vote_log_shares)")
    out = _out_or_new(what, out, (N,), torch.float32, rows.src)
    dev = _one_device(what, rows.src, rows.centers, log_share, out)
    st = _augment_stats(G, steps, dev) if stats else None
    a = L.ProposalPriorArgs()
    if log_share is not None:
        a.log_share = log_share.data_ptr()
    a.G, a.group_rows, a.n_fit, a.h = G, S, n, steps
    a.sigma, a.sd_floor = sigma, sd_floor
    a.prior_out = out.data_ptr()
    if st is not None:
        a.mean_out, a.sd_out, a.votes_out = st.mean.data_ptr(), st.sd.data_ptr(), st.votes.data_ptr()
    _launch(rows, fn, a)
    return (out, st) if stats else out


def proposal_prior_tokens(tokens, group_rows, n_fit, centers, tok_vocab, *, steps=1, sigma, sd_floor, log_share=None, out=None, stats=False):
    """Proposal log-density prior of action tokens (cover_proposal_prior_tokens): tokens int64 [G * group_rows, >= 7 steps] (unit column
    stride, any row stride; row i belongs to prompt i // group_rows) -> fp32 [G * group_rows]. Per prompt the diagonal Gaussian of
    augment_tokens is fitted to the first n_fit rows' de-tokenised values centers[clamp(tok_vocab - token - 1)] (the same device
    function: chain mean, sd with ddof 1, 0 for one row, floored at sd_floor) and every row r of the group gets
    p = -0.5 * sum_{t, d < 6} ((x - mean) / (sigma * sd))^2, one fp32 chain in (step, dim) order, five roundings per term. That is the
    UNNORMALISED log-density: the -sum log(sigma * sd) term is left out (no logarithm on the device; it is the same for every row of a
    prompt). log_share fp32 [n_fit + 1] (host.vote_log_shares) adds, per step, log_share[c], c = how many of the n_fit rows share the
    row's gripper class (value >= 0.5) at that step; None = the gripper contributes nothing; an entry may be -inf. The result is the
    [N] prior prior_select / compute_max_similarity_scores_batch(candidate_prior=) take, with group_size = group_rows -- after
    augment_tokens group_rows = n_samples + n_augmented and n_fit = n_samples; group_rows == n_fit scores plain policy samples among
    their siblings. sigma and sd_floor must be > 0 (no default is chosen). A NaN appears only in the float form. stats=True ->
    (prior, AugmentStats) of the fit. One launch, no workspace, recordable."""
    rows = _token_rows("proposal_prior_tokens", tokens, steps, centers, tok_vocab)
    return _proposal_prior(rows, "cover_proposal_prior_tokens", group_rows, n_fit, sigma, sd_floor, log_share, out, stats)


def proposal_prior_actions(actions, group_rows, n_fit, *, sigma, sd_floor, log_share=None, out=None, stats=False):
    """The same for a flow-matching policy's chunks (cover_proposal_prior_actions): actions fp32 [G * group_rows, steps, >= 7] with unit
    last stride and any other strides -- a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place -> fp32 [G * group_rows]. A
    NaN element of a row that is not among the n_fit fitted ones gives a NaN prior for that row only. See proposal_prior_tokens."""
    rows = _action_rows("proposal_prior_actions", actions)
    return _proposal_prior(rows, "cover_proposal_prior_actions", group_rows, n_fit, sigma, sd_floor, log_share, out, stats)


# ------------------------------------------------------------------------------------------------ verifier-guided refinement
class RefineElites(NamedTuple):
    """What refine_tokens / refine_actions return beside the output with elites=True."""
    rows: torch.Tensor     # int32 [G, n_elite]: the index in the input of the row gathered to output row r of group g
    scores: torch.Tensor   # fp32 [G, n_elite]: its score, bit for bit


def _refine(rows, fn, scores, group_rows, n_elite, n_new, normals, sigma, sd_floor, clip, out, stats, elites):
    """The checks and the launch both refine wrappers share."""
    what, N, steps = rows.what, rows.N, rows.steps
    m, K = _chk_ints(what, n_elite=n_elite, n_new=n_new)
    G, S = _chk_groups(rows, group_rows)
    if not 1 <= m <= S or not 0 <= K <= 4096 or G * (m + K) > 1 << 20:
        raise L.CoverError(f"{what}: 1 <= n_elite <= group_rows, 0 <= n_new <= 4096 and prompts * (n_elite + n_new) <= 2^20 are required "
                           f"(got group_rows={S}, n_elite={m}, n_new={K}, prompts={G})")
    _chk_f32(what, "scores", scores, (N,), hint=" = [rows]")
    sigma, sd_floor, lo, hi = _draw_checks(what, normals, G, K, steps, sigma, sd_floor, clip)
    out = _out_or_new(what, out, rows.out_shape(G * (m + K)), rows.elem, rows.src)
    dev = _one_device(what, rows.src, scores, normals, rows.centers, out)
    st = _augment_stats(G, steps, dev) if stats else None
    el = RefineElites(torch.empty(G, m, dtype=torch.int32, device=dev), torch.empty(G, m, dtype=torch.float32, device=dev)) if elites else None
    a = L.RefineArgs()
    a.scores, a.normals = scores.data_ptr(), (normals.data_ptr() if K else None)
    a.G, a.group_rows, a.n_elite, a.K, a.h = G, S, m, K, steps
    a.sigma, a.sd_floor, a.clip_lo, a.clip_hi = sigma, sd_floor, lo, hi
    a.out = out.data_ptr()
    if el is not None:
        a.elite_rows_out, a.elite_scores_out = el.rows.data_ptr(), el.scores.data_ptr()
    if st is not None:
        a.mean_out, a.sd_out, a.votes_out = st.mean.data_ptr(), st.sd.data_ptr(), st.votes.data_ptr()
    _launch(rows, fn, a)
    res = (out,) + ((st,) if stats else ()) + ((el,) if elites else ())
    return res if len(res) > 1 else out


def refine_tokens(tokens, scores, group_rows, n_elite, n_new, normals, centers, tok_vocab, *, steps=1, sigma=1.0, sd_floor=0.0,
                  clip=(-1.0, 1.0), out=None, stats=False, elites=False):
    """Verifier-guided refinement of action tokens, one round of the cross-entropy method per prompt (cover_refine_tokens): tokens int64
    [G * group_rows, >= 7 steps] (unit column stride, any row stride; row i belongs to prompt i // group_rows) with scores fp32 [rows],
    contiguous, one per row -- whatever the decision was made on (score_histories' scores, robust or combined) -> int64
    [G * (n_elite + n_new), 7 steps]. Per prompt, output rows 0..n_elite-1 are the n_elite best-scored input rows verbatim, best first;
    the n_new rows behind them are EXACTLY the rows augment_tokens draws from those n_elite rows with the same normals (fp32
    [G, n_new, steps, 6], host.augmentation_normals), sigma, sd_floor and clip: the Gaussian is refitted on the elites, its chains run in
    rank order. RANKING: higher score first, equal scores (-0.0 == +0.0) by ascending row index; a NaN score ranks behind every number,
    -inf included, NaNs among themselves by ascending index. On a gripper TIE the new rows take the class of the best elite. n_new == 0 is
    a pure top-n_elite gather. Downstream code takes the result as it takes augment_tokens' output, with group_size = n_elite + n_new and
    n_fit = n_elite. stats=True adds the AugmentStats of the fit, elites=True adds RefineElites (the gathered rows' input indices and
    scores): -> out, (out, stats), (out, elites) or (out, stats, elites). One launch, no workspace, recordable."""
    rows = _token_rows("refine_tokens", tokens, steps, centers, tok_vocab)
    return _refine(rows, "cover_refine_tokens", scores, group_rows, n_elite, n_new, normals, sigma, sd_floor, clip, out, stats, elites)


def refine_actions(actions, scores, group_rows, n_elite, n_new, normals, *, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0), out=None,
                   stats=False, elites=False):
    """The same for a flow-matching policy's chunks (cover_refine_actions): actions fp32 [G * group_rows, steps, >= 7] with unit last
    stride and any other strides -- a [B, steps, 7] view of a [B, chunk, 32] buffer is read in place -> contiguous fp32
    [G * (n_elite + n_new), steps, 7]. The elites are the input's first 7 dims bit for bit; the new rows are augment_actions' on them
    (a gripper tie goes to the class of the best elite). See refine_tokens for the ranking and the returns."""
    rows = _action_rows("refine_actions", actions)
    return _refine(rows, "cover_refine_actions", scores, group_rows, n_elite, n_new, normals, sigma, sd_floor, clip, out, stats, elites)


# ------------------------------------------------------------------------------------------------ neighbourhood-smoothed scores
class SmoothStats(NamedTuple):
    """What smooth_scores_tokens / smooth_scores_actions return beside the smoothed scores with stats=True."""
    density: torch.Tensor      # fp32 [rows]: the row's summed pair weights (self included) / group_rows
    neighbours: torch.Tensor   # int32 [rows]: the rows of its group with a weight > 0, self included
    group_mean: torch.Tensor   # fp32 [G]: the mean of the group's finite scores (0.0 when it has none)


def smooth_dim_scale(dim_scale, what="smooth_dim_scale") -> np.ndarray:
    """The host check of a smoothing scale: a 6-sequence of finite numbers >= 0 (in fp32 as well) -> fp32 numpy [6]."""
    try:
        v = np.asarray(dim_scale, dtype=np.float64)
    except (TypeError, ValueError):
        raise L.CoverError(f"{what}: dim_scale must be 6 numbers (got {dim_scale!r})") from None
    if v.shape != (6,):
        raise L.CoverError(f"{what}: dim_scale must have 6 entries, one per translation / rotation dim (got shape {v.shape})")
    with np.errstate(over="ignore"):
        f = v.astype(np.float32)
    if not (np.isfinite(v).all() and np.isfinite(f).all() and (v >= 0).all()):
        raise L.CoverError(f"{what}: every dim_scale entry must be finite and >= 0 (got {dim_scale!r})")
    return f


def _smooth(rows, fn, scores, group_rows, radius, dim_scale, shrink, split_gripper, out, stats):
    """The checks and the launch both smoothing wrappers share."""
    what, N = rows.what, rows.N
    G, S = _chk_groups(rows, group_rows)
    _chk_f32(what, "scores", scores, (N,), hint=" = [rows]")
    r, shrink = _f32_number(what, "radius", radius), _f32_number(what, "shrink", shrink)
    radius2 = C.c_float(r * r).value            # squared once, in fp32 (the product of two fp32 values is exact in float64)
    if not (r > 0.0 and math.isfinite(radius2) and radius2 > 0.0):
        raise L.CoverError(f"{what}: radius must be > 0 with a finite fp32 square > 0 (got {radius!r})")
    if not (math.isfinite(shrink) and shrink >= 0.0):
        raise L.CoverError(f"{what}: shrink must be finite and >= 0 (got {shrink!r})")
    dim_scale = _dim_scale_for(what, dim_scale, rows.src)
    out = _out_or_new(what, out, (N,), torch.float32, rows.src)
    dev = _one_device(what, rows.src, scores, dim_scale, rows.centers, out)
    st = SmoothStats(torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev),
                     torch.empty(G, dtype=torch.float32, device=dev)) if stats else None
    a = L.SmoothArgs()
    a.scores, a.dim_scale = scores.data_ptr(), dim_scale.data_ptr()
    a.G, a.group_rows, a.h, a.split_gripper = G, S, rows.steps, 1 if split_gripper else 0
    a.radius2, a.shrink = radius2, shrink
    a.smoothed_out = out.data_ptr()
    if st is not None:
        a.density_out, a.neighbours_out, a.group_mean_out = st.density.data_ptr(), st.neighbours.data_ptr(), st.group_mean.data_ptr()
    _launch(rows, fn, a)
    return (out, st) if stats else out


def smooth_scores_tokens(tokens, scores, group_rows, centers, tok_vocab, *, steps=1, radius, dim_scale, shrink=0.0, split_gripper=True,
                         out=None, stats=False):
    """Neighbourhood-smoothed scores of action tokens (cover_smooth_scores_tokens): tokens int64 [G * group_rows, >= 7 steps] (unit column
    stride, any row stride; row i belongs to prompt i // group_rows) with scores fp32 [rows], contiguous -- score_histories' scores or
    robust -> fp32 [rows], which goes where those go (group_argmax, prior_select, refine_tokens). Every row's score is replaced by the
    kernel-weighted mean of its group's scores, w = max(0, 1 - d2 / radius^2) with d2 = sum over (step, dim < 6) of
    ((x_n - x_j) * dim_scale[dim])^2 on the de-tokenised values centers[clamp(tok_vocab - token - 1)], shrunk towards the mean m0 of the
    group's finite scores: (sum w s + shrink * m0) / (sum w + shrink); shrink == 0 is the plain local mean. The row itself has weight 1.
    split_gripper: rows whose gripper class (value >= 0.5) differs at any step have weight 0. A dim of scale 0 is left out, a NaN there
    included. A row whose own score is not finite keeps it bit for bit and is no evidence for the others. radius is squared once in fp32;
    dim_scale is a 6-sequence of finite numbers >= 0, validated here and uploaded, or an fp32 [6] tensor already on the device
    (host.Smooth's, validated there; on the device a negative or non-finite entry makes every pair weight 0). No radius, scale or shrink
    is chosen or recommended: there is no task-success data to choose them on. stats=True -> (smoothed, SmoothStats). Every rounding is
    specified in include/cover_hip.h. One launch, no workspace, recordable."""
    rows = _token_rows("smooth_scores_tokens", tokens, steps, centers, tok_vocab)
    return _smooth(rows, "cover_smooth_scores_tokens", scores, group_rows, radius, dim_scale, shrink, split_gripper, out, stats)


def smooth_scores_actions(actions, scores, group_rows, *, radius, dim_scale, shrink=0.0, split_gripper=True, out=None, stats=False):
    """The same for float rows (cover_smooth_scores_actions): actions fp32 [G * group_rows, steps, >= 7] with unit last stride and any
    other strides, read in place -- a [B, steps, 7] view of a [B, chunk, 32] buffer, or the padded history tensor [N, 10, 7]
    score_histories holds (rows and pads that are equal within a group contribute exact zeros to the distance). A NaN element in a dim
    of non-zero scale isolates its row: every pair weight with it is 0. See smooth_scores_tokens."""
    rows = _action_rows("smooth_scores_actions", actions)
    return _smooth(rows, "cover_smooth_scores_actions", scores, group_rows, radius, dim_scale, shrink, split_gripper, out, stats)


# ------------------------------------------------------------------------------------------------ chunk-coherence prior
class CoherenceStats(NamedTuple):
    """What coherence_prior_tokens / coherence_prior_actions return beside the prior with stats=True."""
    min_dist: torch.Tensor     # fp32 [rows]: the smallest distance D to a reference of non-zero weight (+inf when there is none)
    nearest: torch.Tensor      # int32 [rows]: that reference's index, the lowest on a tie (-1 when there is none)


def _coherence(rows, fn, group_rows, ref, ref_weight, shift, step_weight, dim_scale, gripper_penalty, out, stats):
    """The checks and the launch both coherence wrappers share."""
    what, N, steps = rows.what, rows.N, rows.steps
    shift, = _chk_ints(what, shift=shift)
    G, S = _chk_groups(rows, group_rows)
    if not torch.is_tensor(ref) or ref.dtype != torch.float32 or ref.dim() not in (3, 4) or ref.shape[-1] != 7 or not ref.is_contiguous():
        raise L.CoverError(f"{what}: ref must be contiguous fp32 [R, hr, 7] (shared) or [prompts, R, hr, 7] "
                           f"(got {tuple(ref.shape) if torch.is_tensor(ref) else type(ref).__name__})")
    R, hr = int(ref.shape[-3]), int(ref.shape[-2])
    if ref.dim() == 4 and ref.shape[0] != G:
        raise L.CoverError(f"{what}: a per-prompt ref must have one set per prompt: [{G}, R, hr, 7] (got {tuple(ref.shape)})")
    if not 1 <= R <= 4096 or not 1 <= hr <= 64 or not 0 <= shift < hr:
        raise L.CoverError(f"{what}: 1 <= R <= 4096, 1 <= hr <= 64 and 0 <= shift < hr are required (got R={R}, hr={hr}, shift={shift})")
    _chk_f32(what, "ref_weight", ref_weight, (R,), (G, R), hint=" = [R] (shared) or [prompts, R]")
    _chk_f32(what, "step_weight", step_weight, (steps,), hint=" = [steps] (host.coherence_step_weights makes it)")
    penalty = _f32_number(what, "gripper_penalty", gripper_penalty)
    if not (math.isfinite(penalty) and penalty >= 0.0):
        raise L.CoverError(f"{what}: gripper_penalty must be finite and >= 0 (got {gripper_penalty!r})")
    dim_scale = _dim_scale_for(what, dim_scale, rows.src)
    out = _out_or_new(what, out, (N,), torch.float32, rows.src)
    dev = _one_device(what, rows.src, ref, ref_weight, step_weight, dim_scale, rows.centers, out)
    st = CoherenceStats(torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)) if stats else None
    a = L.CoherenceArgs()
    a.ref, a.ref_g_stride, a.ref_r_stride = ref.data_ptr(), (R * hr * 7 if ref.dim() == 4 else 0), hr * 7
    a.ref_weight, a.w_g_stride = ref_weight.data_ptr(), (R if ref_weight.dim() == 2 else 0)
    a.step_weight, a.dim_scale = step_weight.data_ptr(), dim_scale.data_ptr()
    a.G, a.group_rows, a.h, a.R, a.hr, a.shift, a.gripper_penalty = G, S, steps, R, hr, shift, penalty
    a.prior_out = out.data_ptr()
    if st is not None:
        a.min_dist_out, a.nearest_out = st.min_dist.data_ptr(), st.nearest.data_ptr()
    _launch(rows, fn, a)
    return (out, st) if stats else out


def coherence_prior_tokens(tokens, group_rows, ref, ref_weight, centers, tok_vocab, *, steps=1, shift=0, step_weight, dim_scale,
                           gripper_penalty=0.0, out=None, stats=False):
    """The chunk-coherence prior of action tokens (cover_coherence_prior_tokens): tokens int64 [G * group_rows, >= 7 steps] (unit column
    stride, any row stride; row i belongs to prompt i // group_rows) -> fp32 [rows], per row minus the weighted sum over the reference
    chunks r of ref_weight[r] * D(row, r), D = sum over the overlapping steps t of step_weight[t] * (sum over dim < 6 of
    ((x - y) * dim_scale[dim])^2 + gripper_penalty where the gripper classes (value >= 0.5) differ), x the de-tokenised value
    centers[clamp(tok_vocab - token - 1)] at candidate step t and y the reference value at step t + shift; the overlap is
    min(steps, hr - shift) steps. ref: fp32 [R, hr, 7] shared by all prompts, or [G, R, hr, 7]; ref_weight: fp32 [R] or [G, R], signed
    (a positive weight pulls towards a reference, a negative one pushes away; a reference of weight 0 is not read into a sum, a NaN there
    included). One reference of weight 1 holding the unexecuted tail of the last committed chunk is the backward coherence of
    Bidirectional Decoding; the group's own rows at +1/S with a weak policy's rows at -1/S' is its forward contrast. The result is a
    prior (higher = more coherent): prior_select's prior, score_histories(prior=), verify_and_select(candidate_prior=), added to other
    priors with plain torch. step_weight: fp32 [steps] on the device (host.coherence_step_weights); dim_scale: a 6-sequence of finite
    numbers >= 0 (0 leaves a dim out), validated here and uploaded, or an fp32 [6] tensor already on the device (host.Coherence's,
    validated there; on the device a negative or non-finite entry makes every prior NaN). A NaN candidate element gives its own row a NaN
    prior. No decay, scale, penalty or mixing weight is chosen or recommended: there is no task-success data to choose them on.
    stats=True -> (prior, CoherenceStats). Every rounding is specified in include/cover_hip.h. One launch, no workspace, recordable."""
    rows = _token_rows("coherence_prior_tokens", tokens, steps, centers, tok_vocab)
    return _coherence(rows, "cover_coherence_prior_tokens", group_rows, ref, ref_weight, shift, step_weight, dim_scale, gripper_penalty, out, stats)


def coherence_prior_actions(actions, group_rows, ref, ref_weight, *, shift=0, step_weight, dim_scale, gripper_penalty=0.0, out=None,
                            stats=False):
    """The same for float rows (cover_coherence_prior_actions): actions fp32 [G * group_rows, steps, >= 7] with unit last stride and any
    other strides, read in place -- a [B, steps, 7] view of a [B, chunk, 32] buffer. See coherence_prior_tokens."""
    rows = _action_rows("coherence_prior_actions", actions)
    return _coherence(rows, "cover_coherence_prior_actions", group_rows, ref, ref_weight, shift, step_weight, dim_scale, gripper_penalty, out, stats)


# ------------------------------------------------------------------------------------------------ diverse candidate subsets
class DiverseSubset(NamedTuple):
    """What diverse_subset_tokens / diverse_subset_actions return (G prompt groups of group_rows rows, keep slots per group)."""
    rows: torch.Tensor         # int64 [G * keep, 7 steps] or fp32 [G * keep, steps, 7]: the picked rows verbatim; an unfilled slot repeats
                               # the group's slot 0 (a group with no pick: its input row 0), so the shape is fixed
    picked: torch.Tensor       # int32 [G, keep]: the input row g * group_rows + j of each slot, -1 = unfilled
    count: torch.Tensor        # int32 [G]: the picks made
    value: torch.Tensor        # fp32 [G, keep]: quality + weight * dist at pick time (slot 0: the quality); NaN (0x7FC00000) = unfilled
    dist: torch.Tensor         # fp32 [G, keep]: the distance to the nearest earlier pick at pick time; +inf for slot 0 and unfilled slots
    assign: torch.Tensor       # int32 [G * group_rows]: the slot of the nearest pick of every input row, -1 where there is none
    row_dist: torch.Tensor     # fp32 [G * group_rows]: the distance to it (+inf where there is none)

    @property
    def valid(self) -> torch.Tensor:
        """bool [G, keep]: the slots that hold a pick."""
        return self.picked >= 0


def _diverse(rows, fn, group_rows, keep, quality, weight, cover_dist, step_weight, dim_scale, gripper_penalty):
    """The checks and the launch both diverse-subset wrappers share."""
    what, N, steps = rows.what, rows.N, rows.steps
    m, = _chk_ints(what, keep=keep)
    G, S = _chk_groups(rows, group_rows)
    if not 1 <= m <= S:
        raise L.CoverError(f"{what}: 1 <= keep <= group_rows is required (got group_rows={S}, keep={m})")
    if quality is not None:
        _chk_f32(what, "quality", quality, (N,), hint=" = [rows], or None")
    _chk_f32(what, "step_weight", step_weight, (steps,), hint=" = [steps] (host.coherence_step_weights makes it)")
    weight, penalty = _f32_number(what, "weight", weight), _f32_number(what, "gripper_penalty", gripper_penalty)
    cover = _f32_number(what, "cover_dist", cover_dist, finite=False)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise L.CoverError(f"{what}: weight must be finite and >= 0 (got {weight!r})")
    if not cover < math.inf:
        raise L.CoverError(f"{what}: cover_dist must be < +inf in fp32; a negative value switches the covering rule off (got {cover_dist!r})")
    if not (math.isfinite(penalty) and penalty >= 0.0):
        raise L.CoverError(f"{what}: gripper_penalty must be finite and >= 0 (got {gripper_penalty!r})")
    dim_scale = _dim_scale_for(what, dim_scale, rows.src)
    dev = _one_device(what, rows.src, quality, step_weight, dim_scale, rows.centers)
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    res = DiverseSubset(torch.empty(rows.out_shape(G * m), dtype=rows.elem, device=dev), torch.empty(G, m, **i32), torch.empty(G, **i32),
                        torch.empty(G, m, **f32), torch.empty(G, m, **f32), torch.empty(N, **i32), torch.empty(N, **f32))
    a = L.DiverseArgs()
    a.quality = quality.data_ptr() if quality is not None else None
    a.step_weight, a.dim_scale = step_weight.data_ptr(), dim_scale.data_ptr()
    a.G, a.group_rows, a.m, a.h = G, S, m, steps
    a.weight, a.cover_dist, a.gripper_penalty = weight, cover, penalty
    a.out, a.picked_rows_out, a.count_out = res.rows.data_ptr(), res.picked.data_ptr(), res.count.data_ptr()
    a.pick_value_out, a.pick_dist_out = res.value.data_ptr(), res.dist.data_ptr()
    a.assign_out, a.row_dist_out = res.assign.data_ptr(), res.row_dist.data_ptr()
    _launch(rows, fn, a)
    return res


def diverse_subset_tokens(tokens, group_rows, keep, centers, tok_vocab, *, steps=1, quality=None, weight, cover_dist=-1.0, step_weight,
                          dim_scale, gripper_penalty=0.0):
    """A diverse subset of action-token chunks (cover_diverse_subset_tokens): tokens int64 [G * group_rows, >= 7 steps] (unit column
    stride, any row stride; row i belongs to prompt i // group_rows) -> DiverseSubset with at most keep rows per prompt, chosen greedily:
    pick 0 is the row of the largest quality (lowest index on a tie), every later pick the row that maximises quality + weight * (its
    distance to the nearest row already picked) among the rows not picked yet whose distance to the nearest pick exceeds cover_dist.
    The distance is coherence_prior_tokens' D between two rows of the group: the sum over the steps t of step_weight[t] * (sum over
    dim < 6 of ((x - y) * dim_scale[dim])^2 + gripper_penalty where the gripper classes (value >= 0.5) differ) on the de-tokenised
    values centers[clamp(tok_vocab - token - 1)]. quality: fp32 [rows] or None (all 0): whatever is known -- a policy log-probability,
    the proposal or coherence prior before the verifier, the verifier's scores after it. weight == 0 picks in refine_tokens' rank order;
    quality None with weight > 0 is the farthest-point traversal from row 0. cover_dist < 0: off; 0: a row equal to a pick (in the dims
    that count) is never picked, so duplicates cost no verifier row; r > 0: the selection ends once every row lies within r of a pick,
    count adapts. A row with a NaN quality or a non-finite element the distance reads is never picked (a NaN in a dim of scale 0 or in
    dim 6 is invisible); rows tie-break by ascending index, so the result is a fixed function of the inputs. The unfilled slots of
    .rows repeat slot 0, so .rows goes to tokens_to_histories / score_histories with group_size = keep as it is; host.spread_scores
    takes the scores back to the input rows through .assign. step_weight: fp32 [steps] on the device (host.coherence_step_weights);
    dim_scale: a 6-sequence of finite numbers >= 0, validated here and uploaded, or an fp32 [6] tensor already on the device
    (host.Diversity's, validated there; on the device a negative or non-finite entry makes count 0). No keep, weight, scale or covering
    distance is chosen or recommended: there is no task-success data to choose them on. Every rounding is specified in
    include/cover_hip.h. One launch, no workspace, recordable."""
    rows = _token_rows("diverse_subset_tokens", tokens, steps, centers, tok_vocab)
    return _diverse(rows, "cover_diverse_subset_tokens", group_rows, keep, quality, weight, cover_dist, step_weight, dim_scale, gripper_penalty)


def diverse_subset_actions(actions, group_rows, keep, *, quality=None, weight, cover_dist=-1.0, step_weight, dim_scale, gripper_penalty=0.0):
    """The same for float rows (cover_diverse_subset_actions): actions fp32 [G * group_rows, steps, >= 7] with unit last stride and any
    other strides, read in place -- a [B, steps, 7] view of a [B, chunk, 32] buffer -> DiverseSubset whose .rows is contiguous fp32
    [G * keep, steps, 7], the picked rows' first 7 dims bit for bit. See diverse_subset_tokens."""
    rows = _action_rows("diverse_subset_actions", actions)
    return _diverse(rows, "cover_diverse_subset_actions", group_rows, keep, quality, weight, cover_dist, step_weight, dim_scale, gripper_penalty)


# ------------------------------------------------------------------------------------------------ pi0-FAST de-tokeniser
FAST_TRUNCATED, FAST_PADDED, FAST_MISMATCH, FAST_STRAY, FAST_UNDECODABLE, FAST_NO_TERMINATOR = 1, 2, 4, 8, 16, 32
FAST_MAX_SYMBOLS = 1 << 18          # of a whole piece table: 4096 positions of the longest piece stay below 2^31


class FastPieces:
    """The piece table of fast_decode (cover_fast_decode): piece_off int32 [n_pieces + 1], non-decreasing from 0, and piece_sym int32, the
    code points FAST id f decodes to at piece_sym[piece_off[f] : piece_off[f + 1]]; a piece whose first symbol is negative marks an id
    the BPE could not decode. Both contiguous and on one device (fast_piece_table builds them). The contents are validated here, once
    (one read-back when the tensors are on the device): the kernel indexes piece_sym with them."""

    def __init__(self, piece_off, piece_sym):
        for name, t in (("piece_off", piece_off), ("piece_sym", piece_sym)):
            if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise L.CoverError(f"FastPieces: {name} must be a contiguous int32 tensor of one dim")
        if piece_off.numel() < 2:
            raise L.CoverError("FastPieces: an empty piece table (piece_off must have n_pieces + 1 >= 2 entries)")
        if piece_off.device != piece_sym.device:
            raise L.CoverError("FastPieces: piece_off and piece_sym must be on one device")
        off, sym = piece_off.detach().cpu().numpy().astype(np.int64), piece_sym.detach().cpu().numpy()
        if off[0] != 0 or np.any(np.diff(off) < 0):
            raise L.CoverError("FastPieces: piece_off must start at 0 and never decrease")
        if off[-1] > min(FAST_MAX_SYMBOLS, sym.shape[0]) or sym.shape[0] < 1:
            raise L.CoverError(f"FastPieces: piece_off ends at {off[-1]}: beyond piece_sym's {sym.shape[0]} entries or the limit of "
                               f"{FAST_MAX_SYMBOLS} symbols (piece_sym must hold at least one entry)")
        used = sym[:off[-1]]
        starts = off[:-1][np.diff(off) > 0]                        # where a non-empty piece begins: the one place a marker may stand
        inner = np.ones(used.shape[0], dtype=bool)
        inner[starts] = False
        if np.any(used > 0x10FFFF) or np.any(used[inner] < 0):
            raise L.CoverError("FastPieces: symbols are code points in [0, 0x10FFFF]; a negative one only as a piece's first (undecodable)")
        self.piece_off, self.piece_sym = piece_off, piece_sym

    @property
    def n_pieces(self):
        return self.piece_off.numel() - 1


def fast_piece_table(pieces, device=None):
    """Build a FastPieces on the host: pieces is a sequence over the FAST ids 0 .. n_pieces - 1, each entry the sequence of code points
    the id decodes to (possibly empty) or None for an id that cannot be decoded (host.fast_pieces_from_decoder makes it from a BPE
    decoder). Returns the FastPieces, on device if given. CoverError on an empty table, a code point outside [0, 0x10FFFF] or more than
    2^18 symbols in all."""
    if isinstance(pieces, (str, bytes)) or not hasattr(pieces, "__len__") or len(pieces) < 1:
        raise L.CoverError("fast_piece_table: pieces must be a non-empty sequence of code-point sequences (None = undecodable)")
    off, sym = [0], []
    for f, p in enumerate(pieces):
        if p is None:
            sym.append(-1)
        else:
            vals = [ord(v) if isinstance(v, str) else v for v in p]
            if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 0x10FFFF for v in vals):
                raise L.CoverError(f"fast_piece_table: piece {f} must hold code points in [0, 0x10FFFF] (got {list(p)!r})")
            sym.extend(int(v) for v in vals)
        off.append(len(sym))
        if len(sym) > FAST_MAX_SYMBOLS:
            raise L.CoverError(f"fast_piece_table: more than {FAST_MAX_SYMBOLS} symbols in all")
    sym = sym or [0]                                               # a table of empty pieces still hands the kernel a pointer
    t_off, t_sym = torch.tensor(off, dtype=torch.int32), torch.tensor(sym, dtype=torch.int32)
    return FastPieces(t_off, t_sym) if device is None else FastPieces(t_off.to(device), t_sym.to(device))


class FastDecoded(NamedTuple):
    """What fast_decode returns with stats=True."""
    actions: torch.Tensor      # fp32 [B, horizon, action_dim] (or the caller's out)
    coeff: torch.Tensor        # int32 [B, horizon * action_dim]: the quantised DCT coefficients, frequency-major; zeros on a fatal status
    n_symbols: torch.Tensor    # int32 [B]: the symbols the row's tokens decode to, before truncation
    status: torch.Tensor       # int32 [B]: FAST_* bits


def _chk_id_list(what, name, ids, limit):
    if isinstance(ids, (str, bytes)) or not hasattr(ids, "__len__") or len(ids) > limit:
        raise L.CoverError(f"{what}: {name} must be a sequence of at most {limit} token ids (got {ids!r})")
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -(1 << 62) <= v < (1 << 62) for v in ids):
        raise L.CoverError(f"{what}: {name} must hold integers (got {ids!r})")
    return [int(v) for v in ids]


def fast_decode(tokens, pieces, basis, *, band, stop_ids, skip_ids=(), min_token, scale, horizon, action_dim, relaxed=True, out=None,
                stats=False):
    """The pi0-FAST de-tokeniser on the device (cover_fast_decode): tokens int64 [B, L <= 4096] with ANY non-negative strides -- the
    candidate-major tensor generate_tokens returns, or the transposed view of a step-major [L, B] buffer: strides are passed, nothing is
    copied -> the fp32 action chunks [B, horizon, action_dim], the layout the *_actions calls read in place. Per row: the tokens before
    the first of stop_ids (the terminator "|", EOS, pad; at most 4) are walked in order; a token t of the half-open band = (lo, hi)
    (pi0fast.fast_action_token_range) is the FAST id hi - 1 - t and contributes the code points of its piece (pieces: a FastPieces); a
    token of skip_ids (format tokens such as "Action", ":" and BOS; at most 8) contributes nothing; the symbols + min_token are the
    quantised DCT coefficients, [horizon, action_dim] frequency-major; relaxed truncates or zero-pads to horizon * action_dim, otherwise
    another count is an error; the chunk is the orthonormal inverse DCT of coefficients / scale along the horizon, with basis = fp32
    [horizon, horizon] on the device (host.fast_idct_basis). A stray id, an undecodable piece or (not relaxed) a wrong count zeroes the
    row, as the reference's decoder does on any exception. The semantics are defined on IDS: PI0FASTPolicy.extract_actions decodes to
    text and encodes again, which prepends BOS and lets the tokenizer re-segment; those artefacts are deliberately not reproduced.
    out: an fp32 [B, horizon, action_dim] tensor or VIEW with unit last stride whose rows do not overlap -- the first action_dim
    columns of a [B, chunk, 32] buffer; only those cells are written. stats=True -> FastDecoded(actions, coeff, n_symbols, status), status
    holding the FAST_* bits (1 truncated, 2 padded, 4 count mismatch, 8 stray id, 16 undecodable piece, 32 no terminator; 4 / 8 / 16 zero
    the row). Every rounding is specified in include/cover_hip.h: the result is a fixed bit pattern. One launch, no workspace,
    recordable."""
    what = "fast_decode"
    if not torch.is_tensor(tokens) or tokens.dtype != torch.int64 or tokens.dim() != 2:
        raise L.CoverError(f"{what}: tokens must be an int64 tensor [B, L]")
    B, Lt = tokens.shape
    if B < 1 or B > 1 << 20 or not 1 <= Lt <= 4096 or min(tokens.stride()) < 0:
        raise L.CoverError(f"{what}: 1 <= B <= 2^20, 1 <= L <= 4096 and non-negative strides are required (got tokens {tuple(tokens.shape)})")
    if not isinstance(pieces, FastPieces):
        raise L.CoverError(f"{what}: pieces must be an ops.FastPieces (ops.fast_piece_table builds one)")
    H, D, min_token = _chk_ints(what, horizon=horizon, action_dim=action_dim, min_token=min_token)
    if not 1 <= H <= 128 or not 1 <= D <= 32:
        raise L.CoverError(f"{what}: 1 <= horizon <= 128 and 1 <= action_dim <= 32 are required (got horizon={H}, action_dim={D})")
    if abs(min_token) > 1 << 30:
        raise L.CoverError(f"{what}: |min_token| <= 2^30 is required (got {min_token})")
    _chk_f32(what, "basis", basis, (H, H), hint=" = [horizon, horizon] (host.fast_idct_basis makes it)")
    if not isinstance(band, (tuple, list)) or len(band) != 2:
        raise L.CoverError(f"{what}: band must be the half-open (lo, hi) of pi0fast.fast_action_token_range (got {band!r})")
    lo, hi = _chk_ints(what, band_lo=band[0], band_hi=band[1])
    if not 0 <= lo <= hi < 1 << 62:
        raise L.CoverError(f"{what}: 0 <= band_lo <= band_hi is required (got {lo}, {hi})")
    stop_ids, skip_ids = _chk_id_list(what, "stop_ids", stop_ids, 4), _chk_id_list(what, "skip_ids", skip_ids, 8)
    s = _f32_number(what, "scale", scale)
    if not math.isfinite(s) or s == 0.0:
        raise L.CoverError(f"{what}: scale must be finite and non-zero as fp32 (got {scale!r})")
    if not isinstance(relaxed, (bool, np.bool_)):
        raise L.CoverError(f"{what}: relaxed must be a bool (got {relaxed!r})")
    if out is None:
        out = torch.empty(B, H, D, dtype=torch.float32, device=tokens.device)
    elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (B, H, D) or (D > 1 and out.stride(2) != 1):
        raise L.CoverError(f"{what}: out must be an fp32 tensor or view of shape {(B, H, D)} with unit last stride")
    t_stride = out.stride(1) if H > 1 else D
    n_stride = out.stride(0) if B > 1 else (H - 1) * t_stride + D
    if t_stride < D or n_stride < (H - 1) * t_stride + D:
        raise L.CoverError(f"{what}: out's steps and rows must not overlap (strides {tuple(out.stride())} for shape {(B, H, D)})")
    dev = _one_device(what, tokens, pieces.piece_off, pieces.piece_sym, basis, out)
    st = None
    if stats:
        st = (torch.empty(B, H * D, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
              torch.empty(B, dtype=torch.int32, device=dev))
    a = L.FastDecodeArgs()
    a.tokens, a.tok_row_stride, a.tok_step_stride = tokens.data_ptr(), tokens.stride(0), tokens.stride(1)
    a.band_lo, a.band_hi, a.n_stop, a.n_skip = lo, hi, len(stop_ids), len(skip_ids)
    for i, v in enumerate(stop_ids):
        a.stop_ids[i] = v
    for i, v in enumerate(skip_ids):
        a.skip_ids[i] = v
    a.piece_off, a.piece_sym, a.basis = pieces.piece_off.data_ptr(), pieces.piece_sym.data_ptr(), basis.data_ptr()
    a.B, a.L, a.n_pieces, a.min_token, a.H, a.D, a.relaxed, a.scale = B, Lt, pieces.n_pieces, min_token, H, D, int(bool(relaxed)), s
    a.out, a.out_n_stride, a.out_t_stride = out.data_ptr(), n_stride, t_stride
    if st is not None:
        a.coeff_out, a.n_symbols, a.status = (t.data_ptr() for t in st)
    L.check(L.lib().cover_fast_decode(C.byref(a), _stream()), what)
    return FastDecoded(out, *st) if stats else out


# ------------------------------------------------------------------------------------------------ beam search
def beam_merge(cum, cand_tok, cand_lp, n_beams, feed_pad, out_parent=None, out_token=None, out_feed=None, out_cum=None, out_step_lp=None):
    """One beam-search step over G = rows / n_beams prompt groups (cover_beam_merge; row g * n_beams + b is beam b of group g).
    cum fp32 [rows] contiguous: the beams' scores so far, -inf / NaN = dead; cand_tok int64 / cand_lp fp32 [rows, n_beams] (unit column
    stride, any row stride >= n_beams): each row's top-n_beams list as token_topn writes it. Candidate (b, j) scores cum[b] +
    cand_lp[b][j] (one fp32 add) and is live iff cum[b] is finite, cand_tok[b][j] >= 0 and cand_lp[b][j] is finite; output beam r is
    the r-th live candidate by higher score, then lower b, then lower j. Returns (parent int32, token int64, feed int64, cum fp32,
    step_lp fp32), each [rows]: parent is the row index inside the group, feed is token or, for a dead output, feed_pad (a valid
    token id for the next embed_gather); dead outputs are -1 / -1 / feed_pad / -inf / -inf. out_cum must not be cum.
    Deterministic, one launch, recordable."""
    B = _chk_topn_n("beam_merge", n_beams)
    if cum.dtype != torch.float32 or cum.dim() != 1 or not cum.is_contiguous() or cum.numel() % B != 0:
        raise L.CoverError("beam_merge: cum must be contiguous fp32 [rows], rows a multiple of n_beams")
    rows = cum.numel()
    if int(feed_pad) < 0:
        raise L.CoverError(f"beam_merge: feed_pad must be a valid token id (got {feed_pad})")
    _chk_rows_n_out("beam_merge", rows, B, ("cand_tok", cand_tok, torch.int64), ("cand_lp", cand_lp, torch.float32))
    outs = (("out_parent", out_parent, torch.int32), ("out_token", out_token, torch.int64), ("out_feed", out_feed, torch.int64),
            ("out_cum", out_cum, torch.float32), ("out_step_lp", out_step_lp, torch.float32))
    _chk_rows_out("beam_merge", rows, *outs)
    _chk_dev(cum, cand_tok, cand_lp, out_parent, out_token, out_feed, out_cum, out_step_lp)
    if out_cum is not None and out_cum.data_ptr() == cum.data_ptr():
        raise L.CoverError("beam_merge: out_cum must not alias cum")
    parent, token, feed, cum_o, step_lp = (torch.empty(rows, dtype=dt, device=cum.device) if t is None else t for _, t, dt in outs)
    a = L.BeamMergeArgs()
    a.cum, a.feed_pad, a.groups, a.B = cum.data_ptr(), int(feed_pad), rows // B, B
    a.cand_tok, a.ld_tok = cand_tok.data_ptr(), max(cand_tok.stride(0), B)
    a.cand_lp, a.ld_lp = cand_lp.data_ptr(), max(cand_lp.stride(0), B)
    a.parent_out, a.token_out, a.feed_out = parent.data_ptr(), token.data_ptr(), feed.data_ptr()
    a.cum_out, a.step_lp_out = cum_o.data_ptr(), step_lp.data_ptr()
    L.check(L.lib().cover_beam_merge(C.byref(a), _stream()), "beam_merge")
    return parent, token, feed, cum_o, step_lp


def kv_gather_slots(k_base, vt_base, src_slot, dst_slot, n_t, *, k_offset, vt_offset, k_slot_stride, vt_slot_stride, n_slots, cap, Hkv, D):
    """Slot-to-slot copies inside one region of the per-layer bf16 K / V^T caches, every layer in one launch (cover_kv_gather_slots).
    k_base / vt_base: int64 device tensors [n_layers] of the layers' cache data_ptr() (models.Decoder.kv_tables()); the keyword
    arguments describe the region (models.Decoder.kv_region(r)): K [slot][t][Hkv][D], V^T [slot][Hkv][D][cap], offsets and slot strides
    in elements. src_slot / dst_slot int32 [rows] on the device: K rows and V^T columns t < n_t of slot dst_slot[i] become those of slot
    src_slot[i]; a row with either slot outside [0, n_slots) is skipped; several rows may share a source. THE CALLER GUARANTEES that no
    destination is also a source and that destinations are distinct. V^T is copied in 16-byte runs: up to 7 columns past n_t of a
    destination slot may be overwritten. n_t == 0 is a no-op. One launch, recordable."""
    for name, t in (("k_base", k_base), ("vt_base", vt_base)):
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise L.CoverError(f"kv_gather_slots: {name} must be a contiguous int64 [n_layers] tensor of device pointers")
    if vt_base.numel() != k_base.numel() or k_base.numel() < 1:
        raise L.CoverError("kv_gather_slots: k_base and vt_base must have one entry per layer")
    if src_slot.dtype != torch.int32 or src_slot.dim() != 1 or not src_slot.is_contiguous():
        raise L.CoverError("kv_gather_slots: src_slot must be contiguous int32 [rows]")
    _chk_rows_out("kv_gather_slots", src_slot.numel(), ("dst_slot", dst_slot, torch.int32))
    _chk_dev(k_base, vt_base, src_slot, dst_slot)
    if not 0 <= int(n_t) <= int(cap):
        raise L.CoverError(f"kv_gather_slots: 0 <= n_t <= cap is required (got n_t={n_t}, cap={cap})")
    a = L.KvGatherSlotsArgs()
    a.k_base, a.vt_base, a.src_slot, a.dst_slot = k_base.data_ptr(), vt_base.data_ptr(), src_slot.data_ptr(), dst_slot.data_ptr()
    a.k_offset, a.vt_offset, a.k_slot_stride, a.vt_slot_stride = int(k_offset), int(vt_offset), int(k_slot_stride), int(vt_slot_stride)
    a.n_layers, a.rows, a.n_slots, a.cap, a.Hkv, a.D, a.n_t = k_base.numel(), src_slot.numel(), int(n_slots), int(cap), int(Hkv), int(D), int(n_t)
    L.check(L.lib().cover_kv_gather_slots(C.byref(a), _stream()), "kv_gather_slots")


def beam_backtrack(parent, token, step_lp, n_beams, out_tokens=None, out_logprobs=None):
    """The sequences that end in each final beam (cover_beam_backtrack). parent int32, token int64, step_lp fp32, all contiguous
    step-major [steps, rows] as beam_merge wrote them step by step; rows a multiple of n_beams. Returns candidate-major (tokens int64
    [rows, steps], logprobs fp32 [rows, steps]): final beam r's last-step entries are its own, parent then names the beam of the step
    before inside the group; a parent outside [0, n_beams) leaves the remaining earlier steps -1 / -inf. One launch, recordable."""
    if parent.dtype != torch.int32 or parent.dim() != 2 or not parent.is_contiguous() or parent.shape[0] < 1 or int(n_beams) < 1 or \
            parent.shape[1] % int(n_beams) != 0:
        raise L.CoverError("beam_backtrack: parent must be contiguous int32 [steps >= 1, rows], rows a multiple of n_beams >= 1")
    steps, rows = parent.shape
    for name, t, dt in (("token", token, torch.int64), ("step_lp", step_lp, torch.float32)):
        if t.dtype != dt or t.shape != parent.shape or not t.is_contiguous():
            raise L.CoverError(f"beam_backtrack: {name} must be contiguous {dt} of parent's shape")
    for name, t, dt in (("out_tokens", out_tokens, torch.int64), ("out_logprobs", out_logprobs, torch.float32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (rows, steps) or not t.is_contiguous()):
            raise L.CoverError(f"beam_backtrack: {name} must be contiguous {dt} [rows, steps]")
    _chk_dev(parent, token, step_lp, out_tokens, out_logprobs)
    tokens = torch.empty(rows, steps, dtype=torch.int64, device=parent.device) if out_tokens is None else out_tokens
    lps = torch.empty(rows, steps, dtype=torch.float32, device=parent.device) if out_logprobs is None else out_logprobs
    a = L.BeamBacktrackArgs()
    a.parent, a.token, a.step_lp, a.steps, a.rows, a.B = parent.data_ptr(), token.data_ptr(), step_lp.data_ptr(), steps, rows, int(n_beams)
    a.tokens_out, a.logprobs_out = tokens.data_ptr(), lps.data_ptr()
    L.check(L.lib().cover_beam_backtrack(C.byref(a), _stream()), "beam_backtrack")
    return tokens, lps


def gumbel_topn(logits, lo, hi, n, phi, g_parent, uniform, temperature=1.0, out_tok=None, out_logprob=None, out_perturbed=None):
    """One stochastic-beam-search step of every row (cover_gumbel_topn; a row is one beam): its n (1..64) children with the largest
    perturbed score over columns [lo, hi), hi - lo <= 4096. phi / g_parent fp32 [rows] contiguous: the beam's cumulative log-probability
    and its own perturbed score (a row where either is not finite is a dead beam: all padding, nothing of it is read); uniform fp32
    [rows, hi - lo] (unit column stride, any row stride): one number per column, clamped to [2^-24, 1 - 2^-24], NaN counting as 2^-24.
    Child v has lp = log softmax(logits / temperature) over [lo, hi) (token_logprob's value at (temperature, 0, 1.0), bit for bit),
    g = (phi + lp) - log(-log(u)) and the perturbed score g~ = G - max(0, v) - log1p(exp(-|v|)), v = G - g + log1p(-exp(g - max g)):
    the row's Gumbels conditioned on their maximum being g_parent, which the arg-max child inherits exactly. Returns (tokens int64
    [rows, n] absolute ids, logprobs fp32 [rows, n], perturbed fp32 [rows, n]) ordered by descending g~, equal g~ by ascending column;
    children whose lp is not finite are left out and the remaining slots are -1 / -inf / -inf. The three out_* ([rows, n], unit column
    stride, any row stride >= n) are written in place. Deterministic, one launch, recordable."""
    if not temperature > 0:
        raise L.CoverError(f"gumbel_topn: temperature > 0 is required (got {temperature})")
    _chk_range("gumbel_topn", lo, hi)
    if hi - lo > 4096:
        raise L.CoverError(f"gumbel_topn: hi - lo <= 4096 is required (got lo={lo}, hi={hi})")
    n = _chk_topn_n("gumbel_topn", n)
    rows = _chk_logits("gumbel_topn", logits, hi)
    if phi is None or g_parent is None or uniform is None:
        raise L.CoverError("gumbel_topn: phi, g_parent and uniform are required")
    _chk_rows_out("gumbel_topn", rows, ("phi", phi, torch.float32), ("g_parent", g_parent, torch.float32))
    if uniform.dtype != torch.float32 or tuple(uniform.shape) != (rows, hi - lo) or (hi - lo > 1 and uniform.stride(1) != 1) or \
            (rows > 1 and uniform.stride(0) < hi - lo):
        raise L.CoverError("gumbel_topn: uniform must be fp32 [rows, hi - lo] with unit column stride and a row stride >= hi - lo")
    outs = (("out_tok", out_tok, torch.int64), ("out_logprob", out_logprob, torch.float32), ("out_perturbed", out_perturbed, torch.float32))
    _chk_rows_n_out("gumbel_topn", rows, n, *outs)
    _chk_dev(logits, phi, g_parent, uniform, out_tok, out_logprob, out_perturbed)
    tok, lp, g = (torch.empty(rows, n, dtype=dt, device=logits.device) if t is None else t for _, t, dt in outs)
    a = L.GumbelTopnArgs()
    _fill_rows(a, logits, rows, lo, hi)
    a.temperature, a.phi, a.g_parent, a.n = temperature, phi.data_ptr(), g_parent.data_ptr(), n
    a.uniform, a.ld_u = uniform.data_ptr(), max(uniform.stride(0), hi - lo)
    a.token_out, a.ld_tok = tok.data_ptr(), max(tok.stride(0), n)
    a.logprob_out, a.ld_lp = lp.data_ptr(), max(lp.stride(0), n)
    a.perturbed_out, a.ld_g = g.data_ptr(), max(g.stride(0), n)
    L.check(L.lib().cover_gumbel_topn(C.byref(a), _stream()), "gumbel_topn")
    return tok, lp, g


def beam_merge_gumbel(cum, cand_tok, cand_lp, cand_g, n_beams, feed_pad, out_parent=None, out_token=None, out_feed=None, out_cum=None,
                      out_step_lp=None, out_g=None, out_kappa=None):
    """beam_merge ordered by a stored key (cover_beam_merge_gumbel): cand_g fp32 [rows, n_beams] is gumbel_topn's perturbed list next to
    its tokens and logprobs. Candidate (b, j) is live iff cum[b] is finite, cand_tok[b][j] >= 0 and cand_lp[b][j] and cand_g[b][j] are
    finite; output beam r is the r-th live candidate by higher cand_g (the stored float), then lower b, then lower j. Returns (parent,
    token, feed, cum, step_lp, g, kappa): the first five as beam_merge (cum = cum[b] + cand_lp, one fp32 add), g fp32 [rows] the chosen
    cand_g (-inf for a dead output), kappa fp32 [rows / n_beams] the cand_g of the group's (n_beams + 1)-th candidate in that order, -inf
    when there is none: a kept sequence s was included with probability 1 - exp(-exp(cum_s - kappa)). out_cum must not be cum.
    Deterministic, one launch, recordable."""
    B = _chk_topn_n("beam_merge_gumbel", n_beams)
    if cum.dtype != torch.float32 or cum.dim() != 1 or not cum.is_contiguous() or cum.numel() % B != 0:
        raise L.CoverError("beam_merge_gumbel: cum must be contiguous fp32 [rows], rows a multiple of n_beams")
    rows = cum.numel()
    if int(feed_pad) < 0:
        raise L.CoverError(f"beam_merge_gumbel: feed_pad must be a valid token id (got {feed_pad})")
    _chk_rows_n_out("beam_merge_gumbel", rows, B, ("cand_tok", cand_tok, torch.int64), ("cand_lp", cand_lp, torch.float32),
                    ("cand_g", cand_g, torch.float32))
    outs = (("out_parent", out_parent, torch.int32), ("out_token", out_token, torch.int64), ("out_feed", out_feed, torch.int64),
            ("out_cum", out_cum, torch.float32), ("out_step_lp", out_step_lp, torch.float32), ("out_g", out_g, torch.float32))
    _chk_rows_out("beam_merge_gumbel", rows, *outs)
    _chk_rows_out("beam_merge_gumbel", rows // B, ("out_kappa", out_kappa, torch.float32))
    _chk_dev(cum, cand_tok, cand_lp, cand_g, out_parent, out_token, out_feed, out_cum, out_step_lp, out_g, out_kappa)
    if out_cum is not None and out_cum.data_ptr() == cum.data_ptr():
        raise L.CoverError("beam_merge_gumbel: out_cum must not alias cum")
    parent, token, feed, cum_o, step_lp, g = (torch.empty(rows, dtype=dt, device=cum.device) if t is None else t for _, t, dt in outs)
    kappa = torch.empty(rows // B, dtype=torch.float32, device=cum.device) if out_kappa is None else out_kappa
    a = L.BeamMergeGumbelArgs()
    a.cum, a.feed_pad, a.groups, a.B = cum.data_ptr(), int(feed_pad), rows // B, B
    a.cand_tok, a.ld_tok = cand_tok.data_ptr(), max(cand_tok.stride(0), B)
    a.cand_lp, a.ld_lp = cand_lp.data_ptr(), max(cand_lp.stride(0), B)
    a.cand_g, a.ld_g = cand_g.data_ptr(), max(cand_g.stride(0), B)
    a.parent_out, a.token_out, a.feed_out = parent.data_ptr(), token.data_ptr(), feed.data_ptr()
    a.cum_out, a.step_lp_out, a.g_out, a.kappa_out = cum_o.data_ptr(), step_lp.data_ptr(), g.data_ptr(), kappa.data_ptr()
    L.check(L.lib().cover_beam_merge_gumbel(C.byref(a), _stream()), "beam_merge_gumbel")
    return parent, token, feed, cum_o, step_lp, g, kappa
