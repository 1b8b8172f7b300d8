"""Reference, acceptance rules and the shared case table for cover_attention_bf16 (csrc/attention.hip): tests/test_attention_cpu.py and
tests/test_attention_gpu.py. Plain torch float64 on the CPU; the only project code used is the ctypes struct (plan queries with fake addresses).

The reference (`reference`) restates include/cover_hip.h, not the kernel: per query row (b, t, h) a softmax over the VISIBLE keys of all
segments, kv head h // (Hq / Hkv), scores in scaled-log2 units s_j = fp32(scale * log2 e) * <q, k_j>, masks written as a dense boolean array
    LEN     j < len_b                CAUSAL  j <= t + causal_offset and j < len_b             VISLEN  j < min(len_b, vis_len[t])
With M = max(m_in, max_j s_j), p_j = 2^(s_j - M) and w_in = l_in * 2^(m_in - M) (0 without a seed):
    l = w_in + sum_j p_j         o = (o_in * w_in + sum_j p_j v_j) / l         A = (|o_in| * w_in + sum_j p_j |v_j|) / l
A row with l = 0 (nothing visible, no seed) is 0, its state is l = 0, m = -inf.

Acceptance of random-weight cases, per element, every element (`check_out`):       |out - ref| <= u A + u |ref| + c A
  * u = 2^-8: pack_bf2 / f2bf of common.h are round-to-nearest-even conversions to bf16 (8 significant bits: half an ulp is 2^-9 of the next power
    of two above, at most 2^-8 of the value).
  * u A: the kernel rounds every probability to bf16 once before the PV product but sums the UN-rounded ones into l: the numerator moves by at most
    sum_j u p_j |v_j| = u A l.  u |ref|: the one rounding of the stored output.
  * c A: everything fp32. With e = 2^-24 (unit roundoff of fp32):
      - scores: a dot product of D bf16 x bf16 products (exact in fp32) summed in fp32 and one multiply by the scale: |ds_j| <= (D + 2) e S_j with
        S_j = scale_log2e * sum_d |q_d k_jd|; a probability moves by the factor 2^ds, i.e. relatively by ln 2 * delta, delta = max_j (D + 2) e S_j
        (computed per row by the reference, over the keys inside the length);
      - exp2f: 2 ulp = 4 e, and its argument s_j - m is one fp32 subtraction of numbers below 2^8 in magnitude wherever p_j is not 0 in fp32
        (|s - m| < 150): an absolute 150 e, relatively 150 ln 2 e; every key tile applies one more such factor (alpha) to what came before, the key-split
        merge one more: e_exp = (n_tiles + 2) (4 + 150 ln 2) e;
      - accumulation of n keys and the seed in any order (MFMA, tiles, the merge of 4 waves), the rescale multiplies, o_in * l_in, the reciprocal and
        the final product: e_acc = (n_keys + 2 n_tiles + 16) e.
    Numerator and denominator both carry the probability errors, so c0 = 2 (ln 2 * delta + e_exp) + e_acc; the value that is rounded at the end is
    itself off by (u + c0) A, which adds u (u + c0) A:  c = c0 (1 + u) + u^2.
  state_out: o is fp32 (no output rounding): |o - ref| <= u A + c A; |M_dev - M| <= delta + 2 e |M| (the fp32 dot product and scale); |l_dev - l| <= c l.

Visible-set cases (kind "vis") are exact: q = 0, so every score is 0, every visible probability exactly 1, l the visible count; V is an integer in
[-8, 8], a hash of (segment, slot, key, head, d), so the sums are integers below 2^24, exact in fp32 in any order. The device multiplies by a rounded
reciprocal, so the stored value is bf16(sum / count) or its immediate bf16 neighbour (`check_vis`); a key wrongly included or dropped, a wrong slot,
head or segment changes the sum by an integer and fails. Seeds there are m_in = 0, l_in = 4, o_in = integer / 4 (o_in * l_in exact); some cases give one
batch entry the empty seed m_in = -inf, l_in = 0, o_in = 0 in every kind.

Cases are dicts (`case`, `seg`); each id starts with the form it is placed to reach: f0 per-tile un-split, f1 key-split over 4 waves, f3 shared
keys, with "mx" for block-scaled output. `build` makes a case's logical CPU tensors, `geometry` the buffer layout shared by the fake-address plan query
(`plan_args`) and the device buffers of the GPU tests."""
import ctypes as C
import math

import torch

from tests.rowops_ref import _ordered, round_bf16_from64

BF = torch.bfloat16
U = 2.0 ** -8
E32 = 2.0 ** -24
LOG2E_F32 = 1.4426950408889634
MASK = {"len": 0, "causal": 1, "vis": 2}
SENT_OUT = 0x7FC3            # bf16 bit pattern (a NaN) the output storage is pre-filled with
STALE = 3.0e38               # finite garbage in the unread / masked parts of the caches
KINDS = ("w1", "w4", "vis")  # random weights with q x 1, q x 4 (peaked softmax), visible-set twin
FORM_NAME = {"f0": "PER_TILE", "f1": "KSPLIT4", "f3": "SHARED"}


# ------------------------------------------------------------------------------------------------ case table
def seg(keys, mask="len", lens=None, slots=None, causal_offset=0, vis=None, k_off=0, vt_off=0):
    """keys = the segment's `len` argument; lens = per-batch-entry lengths (<= keys) or None; slots = slot of every batch entry or None (slot = b):
    with a slot map the cache gets one more slot nobody maps to; vis = vis_len table [Tq]; k_off / vt_off = element offsets of the bases"""
    return dict(keys=keys, mask=mask, lens=lens, slots=slots, causal_offset=causal_offset, vis=vis, k_off=k_off, vt_off=vt_off)


def case(id, B, Tq, Hq, Hkv, D, segs, state_in=False, state_out=False, out8=False, q_layout="plain", o_gap=0, base_off=0, spike=None, scale=None, empty_seed=None):
    """q_layout "qkv": q rows inside a [B * Tq, 3 Hq D] buffer; o_gap: extra columns per output row that must keep the sentinel; base_off: elements the q and
    out views start into their storages; spike = (segment, key): the weights kinds put one key far above the rest there (scale 1, k x 0.1); empty_seed = a
    batch entry whose state_in rows are the state of a pass that saw nothing (m = -inf, l = 0, o = 0: what state_out leaves for such a row)"""
    return dict(id=id, B=B, Tq=Tq, Hq=Hq, Hkv=Hkv, D=D, segs=segs, state_in=state_in, state_out=state_out, out8=out8, q_layout=q_layout, o_gap=o_gap,
                base_off=base_off, spike=spike, scale=D ** -0.5 if scale is None else scale, empty_seed=empty_seed)


def _ramp(B, top, step=3, zero_at=None):
    v = [max(1, top - step * (i % 5)) for i in range(B)]
    if zero_at is not None:
        v[zero_at] = 0
    return v


def _cases():
    cs = []
    # ---- form 0: more than 1023 query tiles, not the shared form. Tq = 130 -> 9 tiles: 3 workgroups of 4 waves, the last with 3 idle waves
    for D in (64, 96, 256):
        cs.append(case(f"f0-d{D}-mha-len", 15, 130, 8, 8, D, [seg(70, lens=_ramp(15, 70, 7), k_off=8, vt_off=32)]))
    # causal offset 1 with G = 1: the wave of rows 16 .. 31 has t_hi + offset = 32, its last visible key is the first of a 32-key tile (so for 48 .. 63, ...)
    cs.append(case("f0-d128-mha-causal-tile-edge", 15, 130, 8, 8, 128, [seg(40, lens=_ramp(15, 40)), seg(133, "causal", causal_offset=1)]))
    cs.append(case("f0-d64-mha-vis", 15, 130, 8, 8, 64, [seg(33, slots=[0] * 15), seg(64, "vis", vis=[(7 * t) % 65 for t in range(130)])], q_layout="qkv", o_gap=8))
    # GQA with R = Tq * G = 40 ragged: 3 tiles per (b, kvh) -> workgroups of 3 waves
    cs.append(case("f0-d64-gqa8-ragged-3seg", 171, 5, 16, 2, 64, [seg(34, slots=[0] * 171), seg(31, lens=_ramp(171, 31, 6, zero_at=2), slots=[b % 3 for b in range(171)]),
                                                                  seg(8, "causal", causal_offset=3)], base_off=8))
    cs.append(case("f0-d256-gqa8-vis-late-v", 342, 5, 8, 1, 256, [seg(45, lens=_ramp(342, 45, 9), slots=[b % 2 for b in range(342)]), seg(5, "vis", vis=[1, 5, 5, 0, 5])]))
    cs.append(case("f0-d128-gqa2-state-out", 64, 33, 8, 4, 128, [seg(65, lens=_ramp(64, 65, 11))], state_out=True))
    # ---- form 1
    for D in (64, 96, 128, 256):
        cs.append(case(f"f1-d{D}-3seg-zero-middle", 3, 17, 4, 2, D, [seg(65, slots=[0, 0, 0]), seg(33, lens=[33, 0, 31], slots=[1, 0, 1]), seg(20, "causal", causal_offset=3)]))
    for keys in (1, 31, 32, 33, 64, 65, 127, 129):     # 1 .. 5 key tiles over 4 waves: waves without a tile, a wave with two
        cs.append(case(f"f1-d128-keys{keys}", 2, 16, 2, 2, 128, [seg(keys, lens=[keys, max(1, keys - 2)], k_off=8 * (keys % 2), vt_off=32 * (keys % 2))]))
    for Tq in (1, 15, 16, 17):
        for G in (1, 2, 8):
            off = 3 if (Tq + G) % 2 else 0
            cs.append(case(f"f1-d64-tq{Tq}-g{G}-causal{off}", 3, Tq, 8, 8 // G, 64, [seg(40, lens=[40, 9, 33]), seg(Tq + off + 2, "causal", causal_offset=off)]))
    cs.append(case("f1-d64-causal-tile-edge", 2, 40, 2, 2, 64, [seg(45, "causal", causal_offset=1)]))
    cs.append(case("f1-d128-causal-tile-edge-2seg", 2, 70, 2, 2, 128, [seg(33, lens=[33, 31]), seg(72, "causal", causal_offset=1)]))
    cs.append(case("f1-d96-empty-entry", 3, 5, 4, 4, 96, [seg(40, lens=[40, 0, 17]), seg(33, lens=[5, 0, 33], slots=[0, 1, 1])]))
    cs.append(case("f1-d256-gqa8-vis-zero", 4, 5, 8, 1, 256, [seg(90, lens=[80, 80, 0, 61], slots=[0, 0, 1, 1]), seg(5, "vis", vis=[0, 5, 5, 1, 5])]))
    cs.append(case("f1-d128-state-in", 5, 3, 4, 2, 128, [seg(70, lens=_ramp(5, 70, 13)), seg(6, "causal", causal_offset=2)], state_in=True, empty_seed=1))
    cs.append(case("f1-d64-state-out", 2, 37, 4, 4, 64, [seg(129, slots=[0, 0])], state_out=True))
    cs.append(case("f1-d128-state-in-out", 4, 17, 2, 1, 128, [seg(33, lens=[33, 1, 0, 32])], state_in=True, state_out=True, empty_seed=2))
    cs.append(case("f1-d256-state-in-out", 2, 9, 2, 2, 256, [seg(97)], state_in=True, state_out=True))
    cs.append(case("f1-d128-state-in-4064-tiles", 127, 1, 32, 32, 128, [seg(33, slots=[0] * 127), seg(9, lens=_ramp(127, 9, 2))], state_in=True))
    cs.append(case("f1-d64-qkv-gap-offset", 3, 20, 4, 2, 64, [seg(50, lens=[50, 31, 32], k_off=16, vt_off=64)], q_layout="qkv", o_gap=12, base_off=8))
    cs.append(case("f1-d64-spike-last-tile", 1, 16, 1, 1, 64, [seg(200)], spike=(0, 195), scale=1.0))
    cs.append(case("f1-d64-spike-other-wave", 1, 16, 1, 1, 64, [seg(200)], spike=(0, 40), scale=1.0))
    cs.append(case("f1-d64-spike-second-segment", 1, 16, 1, 1, 64, [seg(70), seg(130)], spike=(1, 101), scale=1.0))
    cs.append(case("f1mx-d128-out8", 3, 17, 2, 2, 128, [seg(77, lens=[77, 40, 1])], out8=True))
    # ---- form 3: D = 128, MHA, length masks, Tq >= 48, ceil(Tq / 64) * Hq * B >= 128
    for Tq, keys in ((48, 1), (64, 31), (70, 33), (128, 96), (130, 97), (70, 129)):     # ring of 4 stages: fewer tiles, exactly 3 / 4, more
        B = 16 if Tq <= 64 else 8
        cs.append(case(f"f3-tq{Tq}-keys{keys}", B, Tq, 8, 8, 128, [seg(keys, lens=_ramp(B, keys, 5))]))
    cs.append(case("f3-2seg-slots-qkv", 8, 70, 8, 8, 128, [seg(97, slots=[0] * 8, k_off=16, vt_off=64), seg(24, lens=_ramp(8, 24, 5))], q_layout="qkv", o_gap=4, base_off=8))
    cs.append(case("f3-3seg-zero-middle", 8, 130, 8, 8, 128, [seg(65, slots=[0] * 8), seg(33, lens=[0] * 8, slots=[b % 2 for b in range(8)]), seg(31, lens=_ramp(8, 31, 7))]))
    cs.append(case("f3-3seg-slots-lens", 16, 48, 8, 8, 128, [seg(33, slots=[0] * 16), seg(40, lens=_ramp(16, 40, 9, zero_at=3), slots=[b // 4 for b in range(16)]),
                                                            seg(5, lens=_ramp(16, 5, 1))]))
    cs.append(case("f3-empty-entry", 8, 70, 8, 8, 128, [seg(40, lens=[40, 0, 3, 33, 0, 40, 31, 32]), seg(9, lens=[9, 0, 0, 1, 0, 9, 8, 7])]))
    cs.append(case("f3-state-in", 8, 70, 8, 8, 128, [seg(129, slots=[0] * 8), seg(24, lens=_ramp(8, 24, 5))], state_in=True, q_layout="qkv", empty_seed=3))
    cs.append(case("f3-state-in-out", 16, 64, 8, 8, 128, [seg(33, lens=_ramp(16, 33, 8, zero_at=5))], state_in=True, state_out=True, empty_seed=5))
    cs.append(case("f3mx-out8", 8, 70, 8, 8, 128, [seg(97, slots=[0] * 8), seg(24, lens=_ramp(8, 24, 5))], out8=True))
    cs.append(case("f3mx-out8-state-in", 16, 64, 8, 8, 128, [seg(31, lens=_ramp(16, 31, 6))], out8=True, state_in=True, q_layout="qkv"))
    return cs


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# pairs (cover_attention_bf16_pair): (id, problem 0, problem 1, dual expected)
PAIRS = [
    ("dual-d64", case("p0", 3, 17, 4, 2, 64, [seg(65, slots=[0] * 3), seg(20, "causal", causal_offset=3)]),
     case("p1", 2, 5, 8, 2, 64, [seg(33, lens=[33, 7])]), True),
    ("dual-d96", case("p0", 1, 70, 4, 4, 96, [seg(72, "causal", causal_offset=1)]), case("p1", 4, 9, 4, 4, 96, [seg(70, slots=[0] * 4), seg(9, lens=[9, 0, 4, 1]), seg(12, "causal", causal_offset=3)]), True),
    ("dual-d128-equal-tiles", case("p0", 2, 16, 2, 2, 128, [seg(129)]), case("p1", 3, 16, 2, 2, 128, [seg(31, lens=[31, 1, 30]), seg(33)]), True),
    ("dual-d128-shared-alone", case("p0", 2, 64, 8, 8, 128, [seg(33)]), case("p1", 16, 64, 8, 8, 128, [seg(97, lens=_ramp(16, 97, 9))]), True),
    ("dual-d64-state-out-0", case("p0", 2, 9, 4, 2, 64, [seg(65)], state_out=True), case("p1", 2, 17, 2, 2, 64, [seg(40, lens=[40, 3])], state_in=True), True),
    ("split-d256", case("p0", 2, 5, 8, 1, 256, [seg(45)]), case("p1", 1, 17, 8, 1, 256, [seg(33)]), False),
    ("split-hkv", case("p0", 2, 5, 4, 2, 64, [seg(45)]), case("p1", 2, 5, 4, 4, 64, [seg(33)]), False),
    ("split-out8", case("p0", 2, 17, 2, 2, 128, [seg(45)], out8=True), case("p1", 2, 5, 2, 2, 128, [seg(33)]), False),
]


def form_of(c):
    """(form name, block-scaled) the id of a case says it reaches"""
    head = c["id"].split("-")[0]
    return FORM_NAME[head[:2]], head.endswith("mx")


def q_tiles(c):
    G = c["Hq"] // c["Hkv"]
    return (c["Tq"] * G + 15) // 16 * c["Hkv"] * c["B"]


# ------------------------------------------------------------------------------------------------ logical data
def _hash_v(si, slot, key, h, d, seed=0):
    """integer in [-8, 8] per (segment, slot, key, head, d): a 32-bit mix, not a linear form whose terms could cancel"""
    x = (si * 0x9E3779B1 + slot * 0x85EBCA77 + key * 0xC2B2AE3D + h * 0x27D4EB2F + d * 0x165667B1 + seed * 0x61C88647 + 0x1B873593) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    x = (x * 0x297A2D39) & 0xFFFFFFFF
    x ^= x >> 15
    return (x % 17) - 8


def seg_slots(c, s):
    """(slot of every batch entry, slots of the cache, valid keys per slot = the longest length among the entries that map to it)"""
    B = c["B"]
    slot_of = list(s["slots"]) if s["slots"] is not None else list(range(B))
    n_slots = max(slot_of, default=0) + 1 + (1 if s["slots"] is not None else 0)
    lens = list(s["lens"]) if s["lens"] is not None else [s["keys"]] * B
    valid = [0] * n_slots
    for b in range(B):
        valid[slot_of[b]] = max(valid[slot_of[b]], lens[b])
    return slot_of, n_slots, lens, valid


def build(c, kind, seed=0):
    """logical CPU tensors of a case: q bf16 [B, Tq, Hq, D]; per segment K, V bf16 [slots, cap, Hkv, D] (cap = keys + 3 rows: rows past a slot's valid
    length are never visible); state_in (o fp32 [B, Tq, Hq, D], ml fp32 [B, Tq, Hq, 2]) or None"""
    B, Tq, Hq, Hkv, D = c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"]
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, c["id"])) + 7 * D + Tq)
    vis_kind = kind == "vis"
    spike = c["spike"] if not vis_kind else None
    q = torch.zeros(B, Tq, Hq, D) if vis_kind else torch.randn(B, Tq, Hq, D, generator=g) * (4.0 if kind == "w4" and not spike else 1.0)
    q = q.to(BF)
    segs = []
    for si, s in enumerate(c["segs"]):
        slot_of, n_slots, lens, valid = seg_slots(c, s)
        cap = s["keys"] + 3
        k = (torch.randn(n_slots, cap, Hkv, D, generator=g) * (0.1 if spike else 1.0)).to(BF)
        if vis_kind:
            ix = torch.meshgrid(torch.arange(n_slots), torch.arange(cap), torch.arange(Hkv), torch.arange(D), indexing="ij")
            v = _hash_v(si, ix[0], ix[1], ix[2], ix[3], seed).to(BF)
        else:
            v = torch.randn(n_slots, cap, Hkv, D, generator=g).to(BF)
        if spike and spike[0] == si:
            k[slot_of[0], spike[1], 0] = (q[0, 3 % Tq, 0].float() * 4).to(BF)
        segs.append(dict(k=k, v=v, slot_of=slot_of, lens=lens, valid=valid, cap=cap))
    state = None
    if c["state_in"]:
        if vis_kind:
            ix = torch.meshgrid(torch.arange(B), torch.arange(Tq), torch.arange(Hq), torch.arange(D), indexing="ij")
            o = _hash_v(7, ix[0], ix[1], ix[2], ix[3], seed).float() / 4
            ml = torch.stack([torch.zeros(B, Tq, Hq), torch.full((B, Tq, Hq), 4.0)], -1)
        else:
            o = torch.randn(B, Tq, Hq, D, generator=g) * 0.3
            ml = torch.stack([torch.randn(B, Tq, Hq, generator=g), torch.rand(B, Tq, Hq, generator=g) + 0.5], -1)
        if c["empty_seed"] is not None:
            o[c["empty_seed"]] = 0
            ml[c["empty_seed"], ..., 0], ml[c["empty_seed"], ..., 1] = -math.inf, 0
        state = (o.contiguous(), ml.contiguous())
    return dict(q=q, segs=segs, state=state, kind=kind)


def visible(c, si, lens):
    """dense boolean [B, Tq, cap] of segment si from the header's definitions"""
    s = c["segs"][si]
    cap = s["keys"] + 3
    j = torch.arange(cap)[None, None, :]
    t = torch.arange(c["Tq"])[None, :, None]
    ln = torch.tensor(lens)[:, None, None]
    if s["mask"] == "len":
        return (j < ln).expand(c["B"], c["Tq"], cap)
    if s["mask"] == "causal":
        return (j <= t + s["causal_offset"]) & (j < ln)
    return j < torch.minimum(ln, torch.tensor(s["vis"])[None, :, None])


def reference(c, data):
    """float64 reference from the bf16 inputs: dict of ref, A [B, Tq, Hq, D]; M, l, delta [B, Tq, Hq]; count (visible keys); n_keys, n_tiles"""
    B, Tq, Hq, Hkv, D = c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"]
    G = Hq // Hkv
    sl2e = float(torch.tensor(c["scale"], dtype=torch.float32) * torch.tensor(LOG2E_F32, dtype=torch.float32))
    q = data["q"].double().view(B, Tq, Hkv, G, D)                   # q head h reads kv head h // G
    ss, sabs, vs, ms, inlen = [], [], [], [], []
    n_tiles = 0
    for si, sd in enumerate(data["segs"]):
        slot = torch.tensor(sd["slot_of"])
        k = sd["k"][slot].double()                                  # [B, cap, Hkv, D]
        ss.append((torch.einsum("btkgd,bjkd->btkgj", q, k) * sl2e).reshape(B, Tq, Hq, -1))
        sabs.append((torch.einsum("btkgd,bjkd->btkgj", q.abs(), k.abs()) * abs(sl2e)).reshape(B, Tq, Hq, -1))
        vs.append(sd["v"][slot].double())
        ms.append(visible(c, si, sd["lens"]))
        inlen.append((torch.arange(sd["cap"])[None, :] < torch.tensor(sd["lens"])[:, None]))
        n_tiles += (max(sd["lens"]) + 31) // 32
    s = torch.cat(ss, 3)                                            # [B, Tq, Hq, J]
    vis = torch.cat(ms, 2)[:, :, None, :].expand_as(s)
    v = torch.cat(vs, 1)                                            # [B, J, Hkv, D]
    inl = torch.cat(inlen, 1)[:, None, None, :].expand_as(s)
    delta = (torch.cat(sabs, 3) * inl).amax(3) * (D + 2) * E32
    neg = torch.full_like(s, -math.inf)
    M = torch.where(vis, s, neg).amax(3)
    if data["state"] is not None:
        o_in, ml = data["state"][0].double(), data["state"][1].double()
        M = torch.maximum(M, ml[..., 0])
    Ms = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    p = torch.where(vis, torch.exp2(s - Ms[..., None]), torch.zeros_like(s))
    l = p.sum(3)
    pk = p.view(B, Tq, Hkv, G, -1)
    num = torch.einsum("btkgj,bjkd->btkgd", pk, v).reshape(B, Tq, Hq, D)
    A = torch.einsum("btkgj,bjkd->btkgd", pk, v.abs()).reshape(B, Tq, Hq, D)
    if data["state"] is not None:
        w = ml[..., 1] * torch.exp2(ml[..., 0] - Ms)
        l = l + w
        num = num + o_in * w[..., None]
        A = A + o_in.abs() * w[..., None]
    ok = l > 0
    ln = torch.where(ok, l, torch.ones_like(l))[..., None]
    ref = torch.where(ok[..., None], num / ln, torch.zeros_like(num))
    A = torch.where(ok[..., None], A / ln, torch.zeros_like(A))
    n_keys = int(s.shape[3])
    return dict(ref=ref, A=A, M=M, l=l, delta=delta, count=vis.sum(3), num=num, n_keys=n_keys, n_tiles=n_tiles)


def bound_c(r):
    """c of the module docstring, per row [B, Tq, Hq]"""
    e_exp = (r["n_tiles"] + 2) * (4 + 150 * math.log(2)) * E32
    e_acc = (r["n_keys"] + 2 * r["n_tiles"] + 16) * E32
    c0 = 2 * (math.log(2) * r["delta"] + e_exp) + e_acc
    return c0 * (1 + U) + U * U


def check_out(got, r, rounded=True):
    """(every element inside the bound and finite, largest |got - ref| / bound). got bf16 (rounded) or the fp32 o of state_out."""
    c = bound_c(r)[..., None]
    bound = U * r["A"] + c * r["A"] + (U * r["ref"].abs() if rounded else 0)
    err = (got.double().cpu().view_as(r["ref"]) - r["ref"]).abs()
    finite = bool(torch.isfinite(got.float()).all())
    share = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return finite and bool((err <= bound).all()), float(share.max()) if share.numel() else 0.0


def worst(got, r):
    """where a result is furthest from the reference, for a failure message: (index, got, ref, A)"""
    err = (got.double().cpu().view_as(r["ref"]) - r["ref"]).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    i = tuple(int(x) for x in torch.unravel_index(err.argmax(), err.shape))
    return i, float(got.double().cpu().view_as(r["ref"])[i]), float(r["ref"][i]), float(r["A"][i]), int((err > 0.05).sum()), err.numel()


def check_ml(ml, r):
    """state_out statistics against the reference: (ok, message)"""
    ml = ml.double().cpu().view(*r["M"].shape, 2)
    m, l = ml[..., 0], ml[..., 1]
    empty = r["l"] == 0
    if not bool((m[empty] == -math.inf).all() and (l[empty] == 0).all()):
        return False, "a row with nothing visible must leave m = -inf, l = 0"
    fm, fl, rm, rl = m[~empty], l[~empty], r["M"][~empty], r["l"][~empty]
    if not bool(((fm - rm).abs() <= r["delta"][~empty] + 2 * E32 * rm.abs() + 1e-30).all()):
        return False, f"m off by {float((fm - rm).abs().max())}"
    if not bool(((fl - rl).abs() <= bound_c(r)[~empty] * rl).all()):
        return False, f"l off by {float(((fl - rl).abs() / rl).max())} relative"
    return True, ""


def vis_quotient(r):
    """float64 quotient of a visible-set case (the sums are integers, or quarter-integers times 4 with a seed: exact)"""
    return r["ref"]


def check_vis(got, r):
    """every element is the bf16 rounding of the float64 quotient or its immediate bf16 neighbour; rows with nothing visible are exactly 0"""
    ref = r["ref"]
    g = got.cpu().view_as(ref)
    d = (_ordered(g) - _ordered(round_bf16_from64(ref))).abs()
    ok = bool((d <= 1).all()) and not bool(g.float().isnan().any())
    zero_rows = (r["l"] == 0)[..., None].expand_as(ref)
    return ok and bool((g.float()[zero_rows] == 0).all())


def check_vis_state(o, ml, r):
    """state_out of a visible-set case: l the exact count (+ 4 with a seed), m = 0 (-inf for an empty row), o within 2 fp32 ulp of the quotient"""
    ml = ml.double().cpu().view(*r["M"].shape, 2)
    if not torch.equal(ml[..., 1], r["l"]) or not torch.equal(ml[..., 0], r["M"]):
        return False
    o = o.double().cpu().view_as(r["ref"])
    return bool(((o - r["ref"]).abs() <= 4 * E32 * r["ref"].abs()).all())


def tie_margin(r):
    """smallest relative distance of a visible-set quotient from a bf16 rounding tie (midpoint between two neighbouring bf16 values)"""
    x = r["ref"][r["ref"] != 0].abs()
    if x.numel() == 0:
        return math.inf
    e = torch.floor(torch.log2(x))
    frac = x / torch.exp2(e) * 128            # [128, 256): bf16 values are the integers, ties the half-integers
    dist = (frac - torch.floor(frac) - 0.5).abs() / frac
    return float(dist.min())


# ------------------------------------------------------------------------------------------------ buffer layout
def geometry(c):
    """element strides / sizes of the buffers of a case, shared by the fake-address plan query and the device buffers"""
    B, Tq, Hq, Hkv, D = c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"]
    rows = B * Tq
    q_ld = 3 * Hq * D if c["q_layout"] == "qkv" else Hq * D
    o_ld = Hq * D + c["o_gap"]
    g = dict(rows=rows, q_ld=q_ld, o_ld=o_ld, q_strides=(Tq * q_ld, q_ld, D), o_strides=(Tq * o_ld, o_ld, D), q_elems=c["base_off"] + rows * q_ld,
             o_guard=o_ld, o_elems=c["base_off"] + (rows + 2) * o_ld, o_start=c["base_off"] + o_ld, segs=[])
    for s in c["segs"]:
        _, n_slots, _, _ = seg_slots(c, s)
        cap = s["keys"] + 3
        tcap = (cap + 31) // 32 * 32
        g["segs"].append(dict(n_slots=n_slots, cap=cap, tcap=tcap, k_strides=(cap * Hkv * D, Hkv * D, D), vt_strides=(Hkv * D * tcap, D * tcap, tcap),
                              k_elems=s["k_off"] + n_slots * cap * Hkv * D, vt_elems=s["vt_off"] + n_slots * Hkv * D * tcap))
    return g


FAKE = dict(q=0x10000000, out=0x20000000, k=0x30000000, vt=0x40000000, tab=0x50000000, si=0x60000000, so=0x70000000, o8=0x80000000)


def plan_args(c, **over):
    """cover_attn_args of a case at fake (aligned, never dereferenced) addresses; `over` replaces struct fields afterwards"""
    from cover_vla_amd import _lib as L
    g = geometry(c)
    a = L.AttnArgs()
    a.q = FAKE["q"] + 2 * c["base_off"]
    a.out = None if (c["state_out"] or c["out8"]) else FAKE["out"] + 2 * g["o_start"]
    a.q_b_stride, a.q_t_stride, a.q_h_stride = g["q_strides"]
    a.o_b_stride, a.o_t_stride, a.o_h_stride = g["o_strides"]
    a.B, a.Tq, a.Hq, a.Hkv, a.D, a.scale = c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"], c["scale"]
    a.n_seg = len(c["segs"])
    for i, (s, gs) in enumerate(zip(c["segs"][:3], g["segs"])):
        sg = a.seg[i]
        sg.k, sg.vt = FAKE["k"] + 0x1000000 * i + 2 * s["k_off"], FAKE["vt"] + 0x1000000 * i + 2 * s["vt_off"]
        sg.k_slot_stride, sg.k_t_stride, sg.k_h_stride = gs["k_strides"]
        sg.vt_slot_stride, sg.vt_h_stride, sg.vt_d_stride = gs["vt_strides"]
        sg.slot_of_batch = FAKE["tab"] if s["slots"] is not None else None
        sg.len_of_batch = FAKE["tab"] + 0x1000 if s["lens"] is not None else None
        sg.vis_len = FAKE["tab"] + 0x2000 if s["vis"] is not None else None
        sg.len, sg.mask_mode, sg.causal_offset = s["keys"], MASK[s["mask"]], s["causal_offset"]
    if c["state_in"]:
        a.state_in_o, a.state_in_ml = FAKE["si"], FAKE["si"] + 0x8000000
    if c["state_out"]:
        a.state_out_o, a.state_out_ml = FAKE["so"], FAKE["so"] + 0x8000000
    if c["out8"]:
        a.out8, a.out8_mx, a.out8_rows = FAKE["o8"], FAKE["o8"] + 0x8000000, g["rows"]
    for name, val in over.items():
        if name.startswith("seg"):                   # seg0__k_t_stride=...
            i, f = int(name[3]), name.split("__")[1]
            setattr(a.seg[i], f, val)
        else:
            setattr(a, name, val)
    return a
