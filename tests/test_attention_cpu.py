"""The launch decision of cover_attention_bf16 one condition at a time (cover_attention_plan / cover_attention_pair_plan: nothing launched, no GPU),
the proof that the case table of tests/attention_ref.py reaches every form with every mask it supports, and self-checks of the float64 reference
that tests/test_attention_gpu.py compares the kernels with.

Pointers are fake addresses: the plan queries only check them for null and alignment."""
import math
import os

import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import ops
from tests import attention_ref as R

_KNOBS = [k for k in ("COVER_ATTN_SHARED", "COVER_ATTN_PAIR", "COVER_ATTN_KSPLIT_MAX", "COVER_ATTN_NW8_MAX") if k in os.environ]
assert not _KNOBS, f"{_KNOBS} set: the decision table below is the one without experiment knobs (they are read once per process)"

case, seg = R.case, R.seg


def plan(c, **over):
    return ops.attention_plan_of(R.plan_args(c, **over))


def refused(c, **over):
    with pytest.raises(L.CoverError, match=r"\(-1\)"):      # COVER_EINVAL
        plan(c, **over)
    return True


def mha(B, Tq, H=8, D=128, segs=None, **kw):
    return case("x", B, Tq, H, H, D, segs or [seg(40)], **kw)


# ------------------------------------------------------------------------------------------------ decision table
def test_plan_1023_vs_1024_query_tiles():
    assert plan(mha(1023, 1, 1, 64)) == ("KSPLIT4", False, 1023, 4)
    assert plan(mha(1024, 1, 1, 64)) == ("PER_TILE", False, 1024, 1)            # one tile per (b, kvh): a workgroup of one wave
    assert plan(case("x", 11, 130, 8, 8, 64, [seg(40)]))[0] == "KSPLIT4"        # 9 * 8 * 11 = 792
    assert plan(case("x", 15, 130, 8, 8, 64, [seg(40)])) == ("PER_TILE", False, 3 * 8 * 15, 4)   # 1080 tiles, 9 per (b, kvh) in 3 workgroups
    assert plan(case("x", 171, 5, 16, 2, 64, [seg(40)])) == ("PER_TILE", False, 342, 3)    # 3 tiles per (b, kvh): three waves


def test_plan_gqa_tiles_count_rows_of_a_kv_group():
    # R = Tq * G rows per kv head: 5 tokens x 8 heads = 40 rows = 3 tiles
    assert plan(case("x", 341, 5, 8, 1, 64, [seg(40)])) == ("KSPLIT4", False, 1023, 4)
    assert plan(case("x", 342, 5, 8, 1, 64, [seg(40)]))[0] == "PER_TILE"


@pytest.mark.parametrize("D", [64, 96, 128])
def test_plan_resumed_threshold_is_4095_up_to_d128(D):
    assert plan(mha(4095, 1, 1, D, state_in=True)) == ("KSPLIT4", False, 4095, 4)
    assert plan(mha(4096, 1, 1, D, state_in=True))[0] == "PER_TILE"
    assert plan(mha(1024, 1, 1, D))[0] == "PER_TILE"                            # without the state: 1023


def test_plan_resumed_threshold_stays_1023_at_d256():
    assert plan(mha(1023, 1, 1, 256, state_in=True))[0] == "KSPLIT4"
    assert plan(mha(1024, 1, 1, 256, state_in=True))[0] == "PER_TILE"


def test_plan_shared_form_conditions_one_at_a_time():
    assert plan(mha(16, 48)) == ("SHARED", False, 128, 4)
    assert plan(mha(16, 48, D=64))[0] == "KSPLIT4"                              # D != 128 (4 * 8 * 16 = 512 tiles)
    assert plan(mha(16, 48, D=256))[0] == "KSPLIT4"
    assert plan(case("x", 16, 48, 8, 4, 128, [seg(40)]))[0] == "KSPLIT4"        # GQA
    assert plan(mha(16, 47))[0] == "KSPLIT4"                                    # Tq 47 / 48
    assert plan(mha(16, 48, segs=[seg(40), seg(50, "causal")]))[0] == "KSPLIT4"
    assert plan(mha(16, 48, segs=[seg(50, "vis", vis=[1] * 48), seg(40)]))[0] == "KSPLIT4"
    assert plan(mha(16, 48, segs=[seg(40), seg(9), seg(50, "causal")]))[0] == "KSPLIT4"
    assert plan(case("x", 127, 48, 1, 1, 128, [seg(40)]))[0] == "KSPLIT4"       # ceil(Tq / 64) * Hq * B = 127 / 128
    assert plan(case("x", 128, 48, 1, 1, 128, [seg(40)])) == ("SHARED", False, 128, 4)
    assert plan(mha(8, 64))[0] == "KSPLIT4" and plan(mha(8, 65)) == ("SHARED", False, 128, 4)     # the product counts groups of 64 rows
    assert plan(mha(15, 130, segs=[seg(40), seg(133, "causal")]))[0] == "PER_TILE"   # a mask the shared form does not take, past 1023 tiles
    assert plan(mha(64, 130))[0] == "SHARED"                                    # the shared form has no upper bound
    assert plan(mha(16, 48, state_in=True))[0] == "SHARED" and plan(mha(16, 48, state_out=True))[0] == "SHARED"


def test_plan_out8_acceptances_and_refusals():
    ok = mha(3, 17, 2, out8=True)
    assert plan(ok) == ("KSPLIT4", True, 2 * 2 * 3, 4)
    assert plan(mha(16, 48, out8=True)) == ("SHARED", True, 128, 4)             # out8 under the shared form
    assert plan(mha(15, 130, out8=True)) == ("SHARED", True, 3 * 8 * 15, 4)     # 1080 tiles: only the shared form takes them
    assert plan(mha(1023, 1, 1, out8=True))[0] == "KSPLIT4"
    assert refused(mha(1024, 1, 1, out8=True))                                  # more than 1023 query tiles (and not the shared form)
    assert plan(mha(4095, 1, 1, out8=True, state_in=True)) == ("KSPLIT4", True, 4095, 4)
    assert refused(mha(4096, 1, 1, out8=True, state_in=True))                   # ... 4095 with state_in
    assert refused(mha(3, 17, 2, D=64, out8=True)) and refused(mha(3, 17, 2, D=256, out8=True))     # D = 128 only
    assert refused(case("x", 3, 17, 4, 2, 128, [seg(40)], out8=True))           # MHA only
    assert refused(mha(3, 17, 2, out8=True, state_out=True))                    # no state_out
    assert refused(ok, o_h_stride=256) and refused(ok, o_t_stride=2 * 128 + 128)     # o_h_stride = 128, o_t_stride = Hq * 128
    assert refused(ok, o_b_stride=17 * 256 + 128)                               # whole rows between batch entries
    assert plan(ok, o_b_stride=20 * 256)[1] is True
    assert refused(mha(0, 17, 2, out8=True)) and refused(mha(3, 0, 2, out8=True))    # nothing to write is not a block-scaled problem
    assert plan(ok, out8_mx=None) == ("KSPLIT4", False, 12, 4)                  # half a pair is no out8 (as before)


def test_plan_pair_conditions_one_at_a_time():
    def pair(c0, c1, o0=None, o1=None):
        return ops.attention_pair_plan(R.plan_args(c0, **(o0 or {})), R.plan_args(c1, **(o1 or {})))
    a, b = case("a", 3, 17, 4, 2, 64, [seg(65)]), case("b", 2, 5, 8, 2, 64, [seg(33), seg(9, "causal")])
    assert pair(a, b) is True
    for D in (96, 128):
        assert pair(dict(a, D=D), dict(b, D=D)) is True
    assert pair(dict(a, D=256), dict(b, D=256)) is False                        # D = 256
    assert pair(a, dict(b, D=128)) is False                                     # unequal D
    assert pair(a, dict(b, Hq=8, Hkv=4)) is False                               # unequal Hkv
    assert pair(dict(a, B=0), b) is False and pair(a, dict(b, Tq=0)) is False   # an empty problem
    assert pair(case("a", 1023, 1, 2, 2, 64, [seg(9)]), b) is False             # 2046 query tiles
    assert pair(case("a", 1023, 1, 1, 1, 64, [seg(9)]), case("b", 1023, 1, 1, 1, 64, [seg(9)])) is True
    assert pair(case("a", 1024, 1, 1, 1, 64, [seg(9)]), case("b", 1, 1, 1, 1, 64, [seg(9)])) is False
    assert pair(case("a", 1, 1, 1, 1, 64, [seg(9)]), case("b", 1024, 1, 1, 1, 64, [seg(9)], state_in=True)) is False   # the pair's bound has no resumed form
    m0, m1 = mha(2, 17, 2), mha(2, 5, 2)
    assert pair(m0, m1) is True
    assert pair(dict(m0, out8=True), m1) is False and pair(m0, dict(m1, out8=True)) is False     # out8 on either side: two launches
    assert pair(mha(2, 64), mha(16, 64)) is True                                # problem 1 alone takes the shared form; the pair runs it key-split
    with pytest.raises(L.CoverError):
        pair(a, b, o1=dict(n_seg=0))
    with pytest.raises(L.CoverError):
        pair(a, b, o0=dict(q=R.FAKE["q"] + 2))


@pytest.mark.parametrize("over", [
    dict(q=R.FAKE["q"] + 8), dict(q=R.FAKE["q"] + 2), dict(q_b_stride=17 * 256 + 4), dict(q_t_stride=260), dict(q_h_stride=68),
    dict(seg0__k=R.FAKE["k"] + 8), dict(seg1__k=R.FAKE["k"] + 4), dict(seg0__vt=R.FAKE["vt"] + 8), dict(seg1__vt=R.FAKE["vt"] + 2),
    dict(seg0__k_slot_stride=68 * 128 + 4), dict(seg0__k_t_stride=132), dict(seg0__k_h_stride=66),
    dict(seg1__vt_slot_stride=2 * 64 * 96 + 4), dict(seg1__vt_h_stride=64 * 96 + 2), dict(seg1__vt_d_stride=97), dict(seg1__vt_d_stride=100),
    dict(out=R.FAKE["out"] + 4), dict(out=R.FAKE["out"] + 2), dict(o_b_stride=17 * 256 + 2), dict(o_t_stride=258), dict(o_h_stride=66),
    dict(state_in_o=R.FAKE["si"] + 8), dict(state_in_o=R.FAKE["si"] + 4), dict(state_in_ml=R.FAKE["si"] + 4),
    dict(state_out_o=R.FAKE["so"] + 8), dict(state_out_ml=R.FAKE["so"] + 4)], ids=lambda o: "-".join(o))
def test_plan_refuses_misaligned_arguments(over):
    c = case("x", 2, 17, 4, 2, 64, [seg(65), seg(9, "causal")], state_in=True)
    if "state_out_o" in over or "state_out_ml" in over:
        c = dict(c, state_out=True)
        over = dict(dict(state_out_o=R.FAKE["so"], state_out_ml=R.FAKE["so"] + 0x8000000), **over)
    assert plan(c)[0] == "KSPLIT4"
    assert refused(c, **over)


def test_plan_accepts_every_aligned_layout():
    c = case("x", 2, 17, 4, 2, 64, [seg(65), seg(9, "causal")], state_in=True)
    assert plan(c, q=R.FAKE["q"] + 16, q_b_stride=0, q_t_stride=3 * 256 + 8, out=R.FAKE["out"] + 8, o_t_stride=260, o_h_stride=68,
                seg0__k=R.FAKE["k"] + 32, seg0__vt=R.FAKE["vt"] + 48, seg1__vt_d_stride=104, state_in_ml=R.FAKE["si"] + 8)[0] == "KSPLIT4"
    assert plan(dict(c, state_out=True), out=None)[0] == "KSPLIT4"              # no `out` with state_out


def test_plan_nothing_to_launch_and_invalid_counts():
    assert plan(mha(0, 17)) == (None, False, 0, 0) and plan(mha(3, 0)) == (None, False, 0, 0)
    assert plan(mha(0, 17, D=72))[0] is None                                    # (as the launch: an empty problem returns before D is looked at)
    assert refused(mha(3, 17, D=72)) and refused(mha(3, 17, D=32)) and refused(mha(3, 17, D=512))
    assert refused(mha(3, 17), n_seg=0) and refused(mha(3, 17), n_seg=4)
    assert refused(case("x", 3, 17, 8, 3, 64, [seg(40)])) and refused(case("x", 3, 17, 4, 8, 64, [seg(40)]))   # Hq % Hkv != 0
    assert refused(mha(3, 17, segs=[seg(40, "vis", vis=[1] * 17)]), seg0__vis_len=None)     # VISLEN without a table
    assert refused(mha(3, 17, state_in=True), state_in_ml=None) and refused(mha(3, 17, state_out=True), state_out_o=None)


# ------------------------------------------------------------------------------------------------ the case table covers the forms
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["id"])
def test_case_reaches_the_form_its_id_names(c):
    form, mxo = R.form_of(c)
    got = plan(c)
    assert got[:2] == (form, mxo), (c["id"], got)
    if form == "KSPLIT4":
        assert R.q_tiles(c) <= (4095 if c["state_in"] and c["D"] <= 128 else 1023)


def test_case_table_reaches_every_form_with_every_mask_it_supports():
    seen = {}
    for c in R.CASES:
        form, mxo = R.form_of(c)
        for s in c["segs"]:
            seen.setdefault((form, mxo), set()).add(s["mask"])
    assert seen[("PER_TILE", False)] == {"len", "causal", "vis"}
    assert seen[("KSPLIT4", False)] == {"len", "causal", "vis"}
    assert seen[("SHARED", False)] == {"len"} and seen[("SHARED", True)] == {"len"} and seen[("KSPLIT4", True)] == {"len"}
    for form in ("PER_TILE", "KSPLIT4", "SHARED"):
        cs = [c for c in R.CASES if R.form_of(c)[0] == form]
        assert any(c["state_in"] for c in cs) or form == "PER_TILE"             # (a resumed pass below 4096 tiles is key-split by definition)
        assert any(c["state_out"] for c in cs) and any(len(c["segs"]) == 3 for c in cs)
        assert any(s["slots"] is not None for c in cs for s in c["segs"]) and any(s["lens"] is not None and 0 in s["lens"] for c in cs for s in c["segs"])
    assert {c["D"] for c in R.CASES if R.form_of(c)[0] == "PER_TILE"} == {64, 96, 128, 256}
    assert {c["D"] for c in R.CASES if R.form_of(c)[0] == "KSPLIT4"} == {64, 96, 128, 256}
    # the thresholds: a key-split case that only the resumed bound keeps there, un-split cases just past 1023
    assert any(R.q_tiles(c) > 1023 for c in R.CASES if R.form_of(c)[0] == "KSPLIT4")
    assert min(R.q_tiles(c) for c in R.CASES if R.form_of(c)[0] == "PER_TILE") < 1100


def test_pair_table_is_reached_dual_and_split():
    got = {}
    for pid, c0, c1, dual in R.PAIRS:
        assert ops.attention_pair_plan(R.plan_args(c0), R.plan_args(c1)) is dual, pid
        got.setdefault(dual, []).append(pid)
    assert {c0["D"] for _, c0, _, dual in R.PAIRS if dual} == {64, 96, 128}
    assert len(got[False]) >= 3
    alone = {pid: (plan(c0)[0], plan(c1)[0]) for pid, c0, c1, _ in R.PAIRS}
    assert alone["dual-d128-shared-alone"] == ("KSPLIT4", "SHARED") and alone["dual-d64"] == ("KSPLIT4", "KSPLIT4")


# ------------------------------------------------------------------------------------------------ the reference
def _naive(c, data):
    """dense masked softmax in torch.float64, one (batch entry, head) at a time, natural-log form"""
    B, Tq, Hq, Hkv, D = c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"]
    out = torch.zeros(B, Tq, Hq, D, dtype=torch.float64)
    scale = float(torch.tensor(c["scale"], dtype=torch.float32) * torch.tensor(R.LOG2E_F32, dtype=torch.float32)) * math.log(2)
    for b in range(B):
        for h in range(Hq):
            ks, vs, ms = [], [], []
            for si, sd in enumerate(data["segs"]):
                ks.append(sd["k"][sd["slot_of"][b], :, h // (Hq // Hkv)].double())
                vs.append(sd["v"][sd["slot_of"][b], :, h // (Hq // Hkv)].double())
                ms.append(R.visible(c, si, sd["lens"])[b])
            s = data["q"][b, :, h].double() @ torch.cat(ks).T * scale
            s = s.masked_fill(~torch.cat(ms, 1), -math.inf)
            p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
            out[b, :, h] = p @ torch.cat(vs)
    return out


@pytest.mark.parametrize("cid", ["f1-d64-3seg-zero-middle", "f1-d256-gqa8-vis-zero", "f1-d96-empty-entry", "f1-d64-tq17-g8-causal3", "f3-empty-entry"])
def test_reference_equals_a_naive_dense_softmax(cid):
    c = R.BY_ID[cid]
    for kind in ("w1", "w4", "vis"):
        data = R.build(c, kind)
        r = R.reference(c, data)
        assert (r["ref"] - _naive(c, data)).abs().max() < 1e-12
        assert bool((r["A"] + 1e-15 >= r["ref"].abs()).all())


def test_reference_chaining_identity():
    """state_out of a pass over segment A, fed as state_in of a pass over segment B, is one pass over A | B"""
    sA, sB = seg(65, lens=[65, 0, 31], slots=[0, 0, 1]), seg(22, "causal", causal_offset=3)
    cA, cB, cAB = case("a", 3, 17, 4, 2, 64, [sA]), case("a", 3, 17, 4, 2, 64, [sB], state_in=True), case("a", 3, 17, 4, 2, 64, [sA, sB])
    dAB = R.build(cAB, "w1")
    rAB = R.reference(cAB, dAB)
    rA = R.reference(cA, dict(q=dAB["q"], segs=dAB["segs"][:1], state=None))
    ml = torch.stack([rA["M"], rA["l"]], -1)
    dB = dict(q=dAB["q"], segs=dAB["segs"][1:], state=(rA["ref"], ml))
    # (segment index 1 of the joint case is segment 0 of the second pass: same mask definition)
    rB = R.reference(cB, dB)
    assert (rB["ref"] - rAB["ref"]).abs().max() < 1e-12
    assert bool((rB["A"] <= rAB["A"] + 1e-12).all())        # (the chained A sees |o_in|, which is at most the first pass's own A)
    assert (rB["l"] - rAB["l"]).abs().max() < 1e-12 and torch.equal(rB["M"], rAB["M"])


@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["id"])
def test_visible_set_sums_are_exact_integers_away_from_bf16_ties(c):
    data = R.build(c, "vis")
    r = R.reference(c, data)
    num4 = r["num"] * (4 if c["state_in"] else 1)          # (seeds are quarter-integers times 4: o_in * l_in is an integer)
    assert torch.equal(num4, num4.round()) and float(r["num"].abs().max()) < 2 ** 24 and float(r["l"].max()) < 2 ** 24
    assert torch.equal(r["l"], r["count"].double() + (data["state"][1][..., 1].double() if c["state_in"] else 0))
    assert bool((r["M"][r["l"] > 0] == 0).all()) and bool(torch.isinf(r["M"][r["l"] == 0]).all())
    if c["empty_seed"] is not None:
        assert bool((data["state"][1][c["empty_seed"], ..., 1] == 0).all()) and bool(torch.isinf(data["state"][1][c["empty_seed"], ..., 0]).all())
    assert R.tie_margin(r) > 2.0 ** -20
    assert float(r["ref"].abs().max()) > 0.1                # the hash does not cancel
    assert r["delta"].max() == 0


def test_the_bound_is_dominated_by_the_two_bf16_roundings():
    """c (all fp32 terms together, with the worst-case linear dot-product term) stays below u, one bf16 rounding, in every case and kind"""
    for c in R.CASES:
        for kind in ("w1", "w4"):
            assert float(R.bound_c(R.reference(c, R.build(c, kind))).max()) < R.U, (c["id"], kind)


# ------------------------------------------------------------------------------------------------ the bound admits a faithful fp32 evaluation
def _flash_fp32(c, data, waves=1):
    """The documented arithmetic in plain fp32 torch: 32-key tiles in order, online softmax (running max m, sum l of the UN-rounded probabilities),
    probabilities rounded to bf16 before the PV product, fp32 accumulation; with waves > 1 the tiles are dealt round-robin to that many partial
    states which are merged at the end (the key-split form). Returns (out bf16, o fp32, ml fp32)."""
    B, Tq, Hq, Hkv, D = c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"]
    G = Hq // Hkv
    sl2e = torch.tensor(c["scale"], dtype=torch.float32) * torch.tensor(R.LOG2E_F32, dtype=torch.float32)
    q = data["q"].float().view(B, Tq, Hkv, G, D)
    m = torch.full((waves, B, Tq, Hq), -math.inf)
    l = torch.zeros(waves, B, Tq, Hq)
    o = torch.zeros(waves, B, Tq, Hq, D)
    if data["state"] is not None:
        m[0], l[0] = data["state"][1][..., 0], data["state"][1][..., 1]
        o[0] = data["state"][0] * l[0][..., None]
    tile = 0
    for si, sd in enumerate(data["segs"]):
        slot = torch.tensor(sd["slot_of"])
        k, v = sd["k"][slot].float(), sd["v"][slot].float()
        vis = R.visible(c, si, sd["lens"])
        for t0 in range(0, max(sd["lens"]), 32):
            w = tile % waves
            tile += 1
            s = (torch.einsum("btkgd,bjkd->btkgj", q, k[:, t0:t0 + 32]) * sl2e).reshape(B, Tq, Hq, -1)
            s = torch.where(vis[:, :, None, t0:t0 + 32], s, torch.full_like(s, -math.inf))
            m_new = torch.maximum(m[w], s.amax(3))
            ms = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp2(m[w] - ms)
            p = torch.exp2(s - ms[..., None])
            l[w] = l[w] * alpha + p.sum(3)
            pv = torch.einsum("btkgj,bjkd->btkgd", p.to(torch.bfloat16).float().view(B, Tq, Hkv, G, -1), v[:, t0:t0 + 32]).reshape(B, Tq, Hq, D)
            o[w] = o[w] * alpha[..., None] + pv
            m[w] = m_new
    M = m.amax(0)
    Ms = torch.where(torch.isinf(M), torch.zeros_like(M), M)
    f = torch.exp2(m - Ms)
    lt = (l * f).sum(0)
    ot = (o * f[..., None]).sum(0)
    inv = torch.where(lt > 0, 1 / lt, torch.zeros_like(lt))
    of = ot * inv[..., None]
    return of.to(torch.bfloat16), of, torch.stack([M, lt], -1)


@pytest.mark.parametrize("cid", ["f1-d64-3seg-zero-middle", "f1-d256-gqa8-vis-zero", "f1-d128-state-in", "f1-d128-state-in-out", "f1-d64-spike-other-wave",
                                 "f1-d128-keys129", "f3-state-in", "f3-3seg-slots-lens", "f0-d96-mha-len", "f0-d128-gqa2-state-out"])
def test_a_plain_fp32_evaluation_of_the_documented_arithmetic_meets_the_acceptance_rules(cid):
    """the bound is not so tight that a correct fp32 / bf16-probability evaluation fails it, in tile order or split over four partial states"""
    c = R.BY_ID[cid]
    for kind in R.KINDS:
        data = R.build(c, kind)
        r = R.reference(c, data)
        for waves in (1, 4):
            out, of, ml = _flash_fp32(c, data, waves)
            if kind == "vis":
                assert R.check_vis(out, r) and R.check_vis_state(of, ml, r), (kind, waves)
            else:
                ok, share = R.check_out(out, r)
                assert ok and share < 1, (kind, waves, share)
                ok2, _ = R.check_out(of, r, rounded=False)
                ok3, why = R.check_ml(ml, r)
                assert ok2 and ok3, (kind, waves, why)
