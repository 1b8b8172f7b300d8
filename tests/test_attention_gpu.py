"""cover_attention_bf16 / cover_attention_bf16_pair on the device against the float64 reference of tests/attention_ref.py: every case of the
shared table in three kinds (random weights, peaked random weights, the exact visible-set twin), every element checked against the derived bound
(no rel-L2), the plan asserted first. Every run uses caches whose unread parts hold +-3e38 (K rows and V^T columns past a slot's length, the
V^T padding to 32, slots nobody maps to) and must equal, bit for bit, the run with zeros there; every output lives between guard rows (and gap
columns, where the case has them) that must keep their sentinel."""
import dataclasses

import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import ops
from tests import attention_ref as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_REF = {}


def ref_of(c, kind):
    """(logical data, float64 reference) of a case: computed once per session, never modified"""
    key = (id(c), kind)
    if key not in _REF:
        data = R.build(c, kind)
        _REF[key] = (data, R.reference(c, data))
    return _REF[key]


def _fill(n, stale):
    if not stale:
        return torch.zeros(n, dtype=BF)
    return (R.STALE * (1 - 2 * (torch.arange(n) % 2)).float()).to(BF)


class Problem:
    """device buffers and the ops.attention arguments of one case"""

    def __init__(self, c, data, dev, stale=True):
        self.c, self.g = c, R.geometry(c)
        g, B, Tq, Hq, Hkv, D = self.g, c["B"], c["Tq"], c["Hq"], c["Hkv"], c["D"]
        rows, HD = g["rows"], Hq * D
        qs = torch.randn(g["q_elems"], generator=torch.Generator().manual_seed(11)).to(BF)     # (the k / v columns of a qkv buffer: unrelated finite values)
        qs[c["base_off"]:].view(rows, g["q_ld"])[:, :HD] = data["q"].reshape(rows, HD)
        self.q = qs.to(dev)
        self.ostore = torch.full((g["o_elems"],), R.SENT_OUT, dtype=torch.int16).view(BF).to(dev)
        self.out = None if (c["state_out"] or c["out8"]) else self.ostore[g["o_start"]:]
        self.segs = []
        for s, gs, sd in zip(c["segs"], g["segs"], data["segs"]):
            kf, vf = _fill(gs["k_elems"], stale), _fill(gs["vt_elems"], stale)
            kv = kf[s["k_off"]:].view(gs["n_slots"], gs["cap"], Hkv, D)
            vv = vf[s["vt_off"]:].view(gs["n_slots"], Hkv, D, gs["tcap"])
            for slot, n in enumerate(sd["valid"]):
                kv[slot, :n] = sd["k"][slot, :n]
                vv[slot, :, :, :n] = sd["v"][slot, :n].permute(1, 2, 0)
            i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=dev)
            self.segs.append(ops.Segment(kf.to(dev), vf.to(dev), gs["k_strides"], gs["vt_strides"], length=s["keys"], len_of_batch=i32(s["lens"]),
                                         slot_of_batch=i32(s["slots"]), mask=R.MASK[s["mask"]], causal_offset=s["causal_offset"], vis_len=i32(s["vis"]),
                                         k_offset=s["k_off"], vt_offset=s["vt_off"]))
        self.kw = {}
        if c["state_in"]:
            self.kw["state_in"] = tuple(t.to(dev) for t in data["state"])
        if c["state_out"]:
            self.so = (torch.full((B, Tq, Hq, D), float("nan"), device=dev), torch.full((B, Tq, Hq, 2), float("nan"), device=dev))
            self.kw["state_out"] = self.so
        if c["out8"]:
            self.o8 = (torch.full((rows, HD), 0xA5, dtype=torch.uint8, device=dev), torch.full((HD // 128, rows, 4), 0xA5, dtype=torch.uint8, device=dev))
            self.kw["out8"] = self.o8
        self.scalars = (B, Tq, Hq, Hkv, D, c["scale"])

    def args(self, **over):
        a = dict(q=self.q[self.c["base_off"]:], q_strides=self.g["q_strides"], out=self.out, o_strides=self.g["o_strides"], segs=self.segs)
        a.update(over)
        return (a["q"], a["q_strides"], a["out"], a["o_strides"], *self.scalars, a["segs"])

    def struct(self):
        return ops.attention_args(*self.args(), **self.kw)

    def run(self):
        ops.attention(*self.args(), **self.kw)
        return self.result()

    def result(self):
        """what the call left behind: (kind of result, tensors on the CPU); asserts the guard rows and gap columns kept their sentinel"""
        g, c = self.g, self.c
        st = self.ostore.cpu().view(torch.int16)
        body = st[g["o_start"]:g["o_start"] + g["rows"] * g["o_ld"]].view(g["rows"], g["o_ld"])
        HD = c["Hq"] * c["D"]
        assert bool((st[:g["o_start"]] == R.SENT_OUT).all()) and bool((st[g["o_start"] + g["rows"] * g["o_ld"]:] == R.SENT_OUT).all()), "guard rows written"
        assert bool((body[:, HD:] == R.SENT_OUT).all()), "gap columns written"
        if c["state_out"]:
            assert bool((body == R.SENT_OUT).all())
            return [self.so[0].cpu(), self.so[1].cpu()]
        if c["out8"]:
            assert bool((body == R.SENT_OUT).all())
            return [self.o8[0].cpu(), self.o8[1].cpu()]
        return [body[:, :HD].contiguous().view(BF).view(c["B"], c["Tq"], c["Hq"], c["D"])]


def same_bits(xs, ys):
    return all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(xs, ys))


def check_against_reference(c, kind, res, r):
    """the acceptance rules of attention_ref on one result; returns the largest share of the bound (weights kinds)"""
    if c["state_out"]:
        o, ml = res
        if kind == "vis":
            assert R.check_vis_state(o, ml, r)
            return 0.0
        ok, why = R.check_ml(ml, r)
        assert ok, why
        ok, share = R.check_out(o, r, rounded=False)
        assert ok, f"state_out o outside the bound: {share:.3f} of it; worst {R.worst(o, r)}"
        return share
    if kind == "vis":
        assert R.check_vis(res[0], r), f"worst (index, got, ref, A, elements off by > 0.05, of) {R.worst(res[0], r)}"
        return 0.0
    ok, share = R.check_out(res[0], r)
    assert ok, f"outside the bound: {share:.3f} of it; worst (index, got, ref, A, elements off by > 0.05, of) {R.worst(res[0], r)}"
    return share


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("c", R.CASES, ids=lambda c: c["id"])
def test_attention_case(dev, c, kind):
    data, r = ref_of(c, kind)
    p = Problem(c, data, dev, stale=True)
    form, mxo = R.form_of(c)
    assert ops.attention_plan_of(p.struct())[:2] == (form, mxo)
    res = p.run()
    clean = Problem(c, data, dev, stale=False).run()
    assert same_bits(res, clean), "finite garbage in the unread parts of the caches changed the result"
    if c["out8"]:
        # the block-scaled rows are, bit for bit, the quantiser's form of the bf16 rows the same problem stores without out8 -- which meet the reference
        c16 = dict(c, out8=False)
        p16 = Problem(c16, data, dev, stale=True)
        assert ops.attention_plan_of(p16.struct())[:2] == (form, False)
        res16 = p16.run()
        q_ref, mx_ref = ops.quantize_act_fp8_mx(res16[0].view(p.g["rows"], -1).to(dev))
        assert torch.equal(res[1], mx_ref.cpu())
        assert torch.equal(res[0].view(torch.float8_e4m3fn).float(), q_ref.cpu().view(torch.float8_e4m3fn).float())
        res, c = res16, c16
    share = check_against_reference(c, kind, res, r)
    print(f"share-of-bound {c['id']} {kind} {share:.4f}")


@pytest.mark.parametrize("kind", ["w1", "vis"])
@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: p[0])
def test_attention_pair(dev, pair, kind):
    """cover_attention_bf16_pair: the plan, then both outputs. A problem that plans the key-split form alone is the same arithmetic in the same order in
    the dual launch -- identical bits; one that plans the shared form alone is compared with the reference. Guard rows around both outputs."""
    pid, c0, c1, dual = pair
    cs = (c0, c1)
    refs = [ref_of(c, kind) for c in cs]
    ps = [Problem(c, d, dev) for c, (d, _) in zip(cs, refs)]
    a0, a1 = ps[0].struct(), ps[1].struct()
    assert ops.attention_pair_plan(a0, a1) is dual
    alone = [ops.attention_plan_of(a)[0] for a in (a0, a1)]
    ops.attention_pair(a0, a1)
    got = [p.result() for p in ps]
    for i, c in enumerate(cs):
        if not dual or alone[i] == "KSPLIT4":
            single = Problem(c, refs[i][0], dev).run()
            assert same_bits(got[i], single), f"problem {i} of the pair differs from its own launch"
        if c["out8"]:
            continue                                    # (bytes compared with the single launch above, which test_attention_case ties to the reference)
        check_against_reference(c, kind, got[i], refs[i][1])


def _untouched(p):
    return bool((p.ostore.cpu().view(torch.int16) == R.SENT_OUT).all())


def test_attention_refuses_misaligned_arguments_and_writes_nothing(dev):
    c = R.BY_ID["f1-d128-state-in"]
    data, _ = ref_of(c, "w1")
    p = Problem(c, data, dev)
    s0 = p.segs[0]
    qs, os_ = p.g["q_strides"], p.g["o_strides"]
    bad = [dict(q=p.q[4:]), dict(q=p.q[1:]), dict(q_strides=(qs[0], qs[1] + 4, qs[2])), dict(q_strides=(qs[0] + 2, qs[1], qs[2])),
           dict(out=p.out[2:]), dict(out=p.out[1:]), dict(o_strides=(os_[0], os_[1] + 2, os_[2])), dict(o_strides=(os_[0], os_[1], os_[2] + 1)),
           dict(segs=[dataclasses.replace(s0, k_offset=4), p.segs[1]]), dict(segs=[dataclasses.replace(s0, vt_offset=4), p.segs[1]]),
           dict(segs=[dataclasses.replace(s0, k_strides=(s0.k_strides[0], s0.k_strides[1] + 4, s0.k_strides[2])), p.segs[1]]),
           dict(segs=[dataclasses.replace(s0, vt_strides=(s0.vt_strides[0], s0.vt_strides[1], s0.vt_strides[2] - 1)), p.segs[1]])]
    for over in bad:
        with pytest.raises(L.CoverError):
            ops.attention(*p.args(**over), **p.kw)
    o, ml = p.kw["state_in"]
    for state in [(o.view(-1)[2:], ml), (o, ml.view(-1)[1:])]:
        with pytest.raises(L.CoverError):
            ops.attention(*p.args(), state_in=state)
    a0, a1 = p.struct(), ops.attention_args(*p.args(q=p.q[4:]), **p.kw)
    with pytest.raises(L.CoverError):
        ops.attention_pair(a0, a1)                      # the second problem is refused before the first one runs
    torch.cuda.synchronize()
    assert _untouched(p)
    res = p.run()                                       # and the same buffers run fine once the arguments are right
    check_against_reference(c, "w1", res, ref_of(c, "w1")[1])


def test_attention_refuses_out8_problems_the_header_excludes(dev):
    """out8 problems the header's comment excludes raise and leave the bytes alone"""
    c = R.BY_ID["f1mx-d128-out8"]
    data, _ = ref_of(c, "w1")
    p = Problem(c, data, dev)
    with pytest.raises(L.CoverError):
        ops.attention(*p.args(o_strides=(p.g["o_strides"][0], p.g["o_strides"][1], 64)), **p.kw)
    so = (torch.empty(c["B"], c["Tq"], c["Hq"], c["D"], device=dev), torch.empty(c["B"], c["Tq"], c["Hq"], 2, device=dev))
    with pytest.raises(L.CoverError):
        ops.attention(*p.args(), state_out=so, **p.kw)
    torch.cuda.synchronize()
    assert bool((p.o8[0].cpu() == 0xA5).all()) and bool((p.o8[1].cpu() == 0xA5).all())
