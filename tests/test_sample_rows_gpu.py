"""Sampling parameters per row on the GPU (ops.token_sample_rows / token_logprob_rows / token_topn_rows): against the float64 references of
tests/sample_rows_ref.py, against the scalar calls bit for bit, row independence, constructed and invalid rows, graph replay, and the two
policies that carry a ladder (OpenVLA.sample, PI0FASTTokens.generate_tokens)."""
import functools
import math

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd._lib import CoverError
from cover_vla_amd.host import sampling_ladder
from tests import logprob_ref as LR
from tests import sample_rows_ref as RR
from tests import sampling_ref as R
from tests import topn_ref as TR

pytestmark = pytest.mark.gpu

ONE_M = float(np.nextafter(np.float32(1), np.float32(0)))
DEV = "cuda:0"


def bits(t):
    """Floats compared as bit patterns: NaN equals NaN, -0.0 differs from +0.0."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def _dev(*arrays):
    return tuple(None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()
                 for a in arrays)


def _rows(x, lo, hi, u, T, k, p):
    """One token_sample_rows launch on device tensors -> (tok, logit, kept, logprob) on the device."""
    lp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    tok, lg, kept = ops.token_sample_rows(x, lo, hi, u, T, k, p, out_logprob=lp)
    return tok, lg, kept, lp


@functools.lru_cache(maxsize=None)
def mixed(name):
    """The case's inputs on the device and its one mixed launch: (xd, ud, lo, hi, (Td, kd, pd), (tok, logit, kept, logprob), refs)."""
    x, u, lo, hi, params, refs = RR.case_data(name)
    xd, ud = _dev(x, u)
    pd = _dev(*params)
    out = _rows(xd, lo, hi, ud, *pd)
    torch.cuda.synchronize()
    return xd, ud, lo, hi, pd, out, refs


def _idx(rows, j):
    return torch.tensor([r for r in range(rows) if r % len(RR.LADDER) == j], device=DEV)


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name", list(RR.CASES))
def test_mixed_launch_matches_reference(dev, name):
    xd, ud, lo, hi, pd, (tok, lg, kept, lp), refs = mixed(name)
    RR.check_rows(tok.cpu().numpy(), kept.cpu().numpy(), lp.cpu().numpy(), refs, lo, hi, what=name)
    assert same(lg, xd.gather(1, tok[:, None])[:, 0])                        # the logit of the pick, whatever the row's kind


# ------------------------------------------------------------------------------------------------ 2. against the scalar calls, bit for bit
@pytest.mark.parametrize("name", list(RR.CASES))
def test_mixed_launch_equals_scalar_calls_bit_for_bit(dev, name):
    xd, ud, lo, hi, pd, (tok, lg, kept, lp), refs = mixed(name)
    n, rows = hi - lo, xd.shape[0]
    for j, (T, k, p) in enumerate(RR.LADDER):
        idx = _idx(rows, j)
        xs, us = xd[idx].contiguous(), ud[idx].contiguous()
        if T == 0:                                                          # greedy rows
            s_tok, s_lg = ops.token_select(xs, lo, hi, uniform=None)
            assert same(tok[idx], s_tok) and same(lg[idx], s_lg), (name, j)
            assert same(lp[idx], ops.token_logprob(xs, lo, hi, s_tok, temperature=1.0)), (name, j)
            assert (kept[idx] == n).all()
            continue
        s_lp = torch.empty(idx.numel(), dtype=torch.float32, device=dev)
        s_tok, s_lg, s_kept = ops.token_sample(xs, lo, hi, us, temperature=T, top_k=k, top_p=p, out_logprob=s_lp)
        filtered = 0 < k < n or p < 1
        if filtered or n > 4096:                                            # the scalar call runs token_sample_k
            for a, b, what in ((tok, s_tok, "token"), (lg, s_lg, "logit"), (kept, s_kept, "kept"), (lp, s_lp, "logprob")):
                assert same(a[idx], b), (name, j, what)
        else:                                                               # the scalar call is token_select's float arithmetic
            assert same(lp[idx], ops.token_logprob(xs, lo, hi, tok[idx].contiguous(), temperature=T, top_k=k, top_p=p)), (name, j)
            assert (kept[idx] == n).all()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. row independence
@pytest.mark.parametrize("name", list(RR.CASES))
def test_rows_are_independent(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), out, refs = mixed(name)
    rows = xd.shape[0]
    rev = _rows(xd.flip(0).contiguous(), lo, hi, ud.flip(0).contiguous(), Td.flip(0).contiguous(), kd.flip(0).contiguous(), pd.flip(0).contiguous())
    assert all(same(a.flip(0), b) for a, b in zip(rev, out)), name
    for r in range(rows):                                                   # a 1-row launch of any row
        one = _rows(xd[r:r + 1], lo, hi, ud[r:r + 1], Td[r:r + 1].clone(), kd[r:r + 1].clone(), pd[r:r + 1].clone())
        assert all(same(a, b[r:r + 1]) for a, b in zip(one, out)), (name, r)
    for j in range(len(RR.LADDER)):                                         # a launch of the rows that share one parameter set
        idx = _idx(rows, j)
        sub = _rows(xd[idx].contiguous(), lo, hi, ud[idx].contiguous(), Td[idx].contiguous(), kd[idx].contiguous(), pd[idx].contiguous())
        assert all(same(a, b[idx]) for a, b in zip(sub, out)), (name, j)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. scoring and ranking
@pytest.mark.parametrize("name", list(RR.CASES))
def test_logprob_rows_and_topn_rows(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), (tok, lg, kept, lp), refs = mixed(name)
    rows = xd.shape[0]
    kept2 = torch.empty_like(kept)
    assert same(ops.token_logprob_rows(xd, lo, hi, tok, Td, kd, pd, out_kept=kept2), lp) and same(kept2, kept)
    for n in (5, 64):
        kept3 = torch.empty_like(kept)
        t_tok, t_lp, t_ent = ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, out_kept=kept3)
        assert same(kept3, kept)
        for j, (T, k, p) in enumerate(RR.LADDER):
            idx = _idx(rows, j)
            T, k, p = (1.0, 0, 1.0) if T == 0 else (T, k, p)                # a greedy row is ranked at temperature 1, unfiltered
            s_tok, s_lp, s_ent = ops.token_topn(xd[idx].contiguous(), lo, hi, n, temperature=T, top_k=k, top_p=p)
            assert same(t_tok[idx], s_tok) and same(t_lp[idx], s_lp) and same(t_ent[idx], s_ent), (name, n, j)
        TR.check_topn(t_tok.cpu().numpy(), t_lp.cpu().numpy(), t_ent.cpu().numpy(), kept3.cpu().numpy(), refs, lo, what=f"{name} n={n}", n=n)


# ------------------------------------------------------------------------------------------------ 5. constructed rows
def test_constructed_rows(dev):
    g = torch.Generator().manual_seed(5)
    # greedy rows with three equal maxima: the lowest index, at several widths and alignments
    for ld, lo, hi in ((300, 5, 261), (4200, 3, 4100), (9000, 1, 8999)):
        x = torch.randn(4, ld, generator=g)
        want = []
        for r in range(4):
            cols = lo + torch.randperm(hi - lo, generator=g)[:3]
            x[r, cols] = 9.0
            want.append(int(cols.min()))
        x[3, lo] = 9.0                                                      # the first column of the range among them
        want[3] = lo
        xd, ud, Td = _dev(x, torch.full((4,), 0.99), torch.zeros(4))
        tok, lg, kept, lp = _rows(xd, lo, hi, ud, Td, None, None)
        assert tok.tolist() == want and (lg == 9.0).all() and (kept == hi - lo).all()
        assert same(lp, ops.token_logprob(xd, lo, hi, tok, temperature=1.0))
    # an all-equal row of 4097 columns under top_k = 1: ties with the k-th value stay, all 4097 are kept; the pick follows the uniform
    x = torch.full((3, 4200), 0.25)
    u = torch.tensor([0.0, 0.5, ONE_M])
    xd, ud, Td, kd = _dev(x, u, torch.tensor([1.0, 0.7, 1.5]), torch.ones(3, dtype=torch.int32))
    tok, lg, kept, lp = _rows(xd, 3, 4100, ud, Td, kd, None)
    assert (kept == 4097).all() and tok.tolist() == [3, 3 + 2048, 3 + 4096]
    tol = float(LR.tolerance(0.0, math.log(4097)))
    assert (lp.cpu().double() + math.log(4097)).abs().max() <= tol
    # top_p arrays of all ones and top_k arrays of all zeros equal the NULL arrays
    xd, ud, lo, hi, (Td, kd, pd), out, refs = mixed("mid")
    base = _rows(xd, lo, hi, ud, Td, None, None)
    for k_arr, p_arr in ((torch.zeros_like(kd), None), (None, torch.ones_like(pd)), (torch.zeros_like(kd), torch.ones_like(pd))):
        assert all(same(a, b) for a, b in zip(_rows(xd, lo, hi, ud, Td, k_arr, p_arr), base))
    lp_n = ops.token_logprob_rows(xd, lo, hi, base[0], Td)
    assert same(lp_n, ops.token_logprob_rows(xd, lo, hi, base[0], Td, torch.zeros_like(kd), torch.ones_like(pd))) and same(lp_n, base[3])
    tn = ops.token_topn_rows(xd, lo, hi, 5, Td)
    assert all(same(a, b) for a, b in zip(tn, ops.token_topn_rows(xd, lo, hi, 5, Td, torch.zeros_like(kd), torch.ones_like(pd))))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. invalid rows
def _guarded(rows, dtype, cols=None, guard=16):
    """An output [rows] (or [rows, cols]) in the middle of a larger buffer filled with a pattern: (buffer, the view)."""
    n = rows * (cols or 1)
    buf = torch.full((n + 2 * guard,), float("nan") if dtype == torch.float32 else -77, dtype=dtype, device=DEV)
    view = buf[guard:guard + n]
    return buf, (view if cols is None else view.view(rows, cols))


def _guards_intact(buf, rows, cols=None, guard=16):
    n = rows * (cols or 1)
    edge = torch.cat([buf[:guard], buf[guard + n:]])
    return bool(torch.isnan(edge).all()) if buf.dtype == torch.float32 else bool((edge == -77).all())


def test_invalid_rows_report_themselves(dev):
    rows, ld, lo, hi = 8, 5000, 5, 4517                                     # 4512 columns: wider than the LDS candidate list
    x, u = R.lm_like_rows(7106, rows, ld, lo, hi)
    nan = float("nan")
    good = (torch.tensor([0, 1, 0.7, 1, 1, 1.5, 1.3, 0.5]), torch.tensor([0, 0, 64, 50, 0, 8, 20, 1], dtype=torch.int32),
            torch.tensor([1, 1, 0.95, 1, 0.9, 1, 0.8, 1.0]))
    T, k, p = (t.clone() for t in good)
    T[1], T[3], p[4], k[6] = -1.0, nan, 0.0, -1
    k[0], p[0] = -5, nan                                                    # a greedy row does not read its top_k / top_p: still valid
    invalid = [1, 3, 4, 6]
    valid = [r for r in range(rows) if r not in invalid]
    xd, ud = _dev(x, u)
    ref = _rows(xd, lo, hi, ud, *_dev(*good))
    Td, kd, pd = _dev(T, k, p)
    bufs = [_guarded(rows, dt) for dt in (torch.int64, torch.float32, torch.int32, torch.float32)]
    tok, lg, kept, lp = (v for _, v in bufs)
    ops.token_sample_rows(xd, lo, hi, ud, Td, kd, pd, out_tok=tok, out_logit=lg, out_kept=kept, out_logprob=lp)
    torch.cuda.synchronize()
    assert (tok[invalid] == -1).all() and torch.isnan(lg[invalid]).all() and (kept[invalid] == 0).all() and torch.isnan(lp[invalid]).all()
    assert all(same(a[valid], b[valid]) for a, b in zip((tok, lg, kept, lp), ref))
    assert all(_guards_intact(b, rows) for b, _ in bufs)
    # the scorer and the ranker on the same parameters
    (b_lp, lp2), (b_k, kept2) = _guarded(rows, torch.float32), _guarded(rows, torch.int32)
    ops.token_logprob_rows(xd, lo, hi, ref[0], Td, kd, pd, out=lp2, out_kept=kept2)
    assert torch.isnan(lp2[invalid]).all() and (kept2[invalid] == 0).all() and same(lp2[valid], ref[3][valid]) and same(kept2[valid], ref[2][valid])
    n = 5
    g_tok, g_lp, g_ent = ops.token_topn_rows(xd, lo, hi, n, *_dev(*good))
    (b_tt, tt), (b_tl, tl), (b_te, te), (b_tk, tk) = (_guarded(rows, torch.int64, n), _guarded(rows, torch.float32, n), _guarded(rows, torch.float32),
                                                      _guarded(rows, torch.int32))
    ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, out_tok=tt, out_logprob=tl, out_entropy=te, out_kept=tk)
    assert (tt[invalid] == -1).all() and torch.isneginf(tl[invalid]).all() and torch.isnan(te[invalid]).all() and (tk[invalid] == 0).all()
    assert same(tt[valid], g_tok[valid]) and same(tl[valid], g_lp[valid]) and same(te[valid], g_ent[valid]) and same(tk[valid], ref[2][valid])
    assert all(_guards_intact(b, rows) for b in (b_lp, b_k, b_te, b_tk)) and _guards_intact(b_tt, rows, n) and _guards_intact(b_tl, rows, n)
    torch.cuda.synchronize()                                                # no error was left behind


def test_c_entry_points_refuse_bad_launch_arguments(dev):
    import ctypes as C
    from cover_vla_amd import _lib as L
    x, u, T = torch.zeros(4, 64, device=dev), torch.zeros(4, device=dev), torch.ones(4, device=dev)
    tok = torch.full((4,), -7, dtype=torch.int64, device=dev)
    tok2 = torch.full((4, 4), -7, dtype=torch.int64, device=dev)
    lp = torch.full((4, 4), -7.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fill(a, **over):
        a.logits, a.ld, a.rows, a.lo, a.hi, a.temperature = x.data_ptr(), 64, 4, 0, 64, T.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def sample(**over):
        a = fill(L.TokenSampleRowsArgs(), **dict(dict(uniform=u.data_ptr(), token_out=tok.data_ptr()), **over))
        return L.lib().cover_token_sample_rows(C.byref(a), st)

    def logprob(**over):
        a = fill(L.TokenLogprobRowsArgs(), **dict(dict(token=tok.data_ptr(), logprob_out=lp.data_ptr()), **over))
        return L.lib().cover_token_logprob_rows(C.byref(a), st)

    def topn(**over):
        a = fill(L.TokenTopnRowsArgs(), **dict(dict(n=4, token_out=tok2.data_ptr(), ld_tok=4, logprob_out=lp.data_ptr(), ld_lp=4), **over))
        return L.lib().cover_token_topn_rows(C.byref(a), st)

    shape = (dict(hi=0), dict(lo=-1), dict(lo=0, hi=(1 << 20) + 1), dict(rows=-1), dict(logits=None), dict(temperature=None))
    for over in shape + (dict(uniform=None), dict(token_out=None)):
        assert sample(**over) == -1, over                                   # COVER_EINVAL
    for over in shape + (dict(token=None), dict(logprob_out=None)):
        assert logprob(**over) == -1, over
    for over in shape + (dict(n=0), dict(n=65), dict(ld_tok=3), dict(ld_lp=3), dict(token_out=None), dict(logprob_out=None)):
        assert topn(**over) == -1, over
    torch.cuda.synchronize()
    assert (tok == -7).all() and (tok2 == -7).all() and (lp == -7.0).all()   # nothing was launched
    assert sample() == 0 and topn() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. graph
def test_graph_replay_follows_the_parameter_tensors(dev):
    xd, ud, lo, hi, (Td, kd, pd), first, refs = mixed("mid")
    rows = xd.shape[0]
    roll = lambda t: torch.roll(t, 3).contiguous()
    second = _rows(xd, lo, hi, ud, roll(Td), roll(kd), roll(pd))            # another ladder over the same rows, eager
    assert not same(second[0], first[0])
    Ts, ks, ps = Td.clone(), kd.clone(), pd.clone()                         # the static parameter buffers of the capture
    tok = torch.empty(rows, dtype=torch.int64, device=dev)
    lg, lp = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    kept = torch.empty(rows, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with ops.Graph() as gr:
            ops.token_sample_rows(xd, lo, hi, ud, Ts, ks, ps, out_tok=tok, out_logit=lg, out_kept=kept, out_logprob=lp)
        for want, src in ((first, (Td, kd, pd)), (second, (roll(Td), roll(kd), roll(pd))), (first, (Td, kd, pd))):
            for dst, s in zip((Ts, ks, ps), src):
                dst.copy_(s)
            tok.fill_(-1)
            gr.launch()
            side.synchronize()
            assert all(same(a, b) for a, b in zip((tok, lg, kept, lp), want))
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ 8. OpenVLA
def _check_steps(logits, picks, kept, lps, lo, hi, u, T, k, p, what):
    """Per traced step: every decided pick equals the reference on that step's logits (greedy rows: the arg-max over [lo, hi) exactly);
    kept and log-probabilities where given. Returns (decided, all)."""
    n_dec = n_all = 0
    for i, lg in enumerate(logits):
        refs = RR.reference_rows(lg.float().cpu().numpy(), lo, hi, u[:, i].numpy(), T, k, p)
        for r, ref in enumerate(refs):
            n_all += 1
            t = int(picks[i][r])
            if ref["greedy"]:
                assert t == lo + ref["token"] and (kept is None or int(kept[i][r]) == hi - lo), (what, i, r)
            if ref["cut_decided"] and kept is not None:
                assert int(kept[i][r]) == ref["kept"], (what, i, r)
            if ref["cut_decided"] and ref["pick_decided"]:
                n_dec += 1
                assert t == lo + ref["token"], (what, i, r)
        if lps is not None:
            LR.check_logprobs(lps[i], picks[i], refs, lo, hi, what=f"{what} step {i}", cap=1.0)
    print(f"{what}: {n_dec} of {n_all} picks decided, all equal to the reference")
    assert n_dec >= 0.9 * n_all
    return n_dec, n_all


def test_openvla_ladder(dev):
    from cover_vla_amd.openvla import OpenVLA
    P, S, Lt, n_gen = 2, 4, 9, 7
    c = dict(synth.OPENVLA_SMALL)
    sd = synth.openvla_state(c, seed=3, std=0.08)
    g = torch.Generator().manual_seed(3)
    frame = torch.randint(0, 256, (1, c["image"], c["image"], 3), generator=g, dtype=torch.uint8)
    lens = torch.tensor([Lt, Lt - 3], dtype=torch.int32)
    toks = torch.zeros(P, Lt, dtype=torch.long)
    for q in range(P):
        toks[q, :lens[q]] = torch.randint(2, c["tok_vocab"] - c["n_bins"], (int(lens[q]),), generator=g)
    u = torch.rand(P * S, n_gen, generator=g)
    kw = dict(device="cuda:0", max_prompts=4, max_candidates=8, max_text=Lt)
    eager = OpenVLA(sd, c, **kw)
    eager.decode_graph = False                                              # what COVER_DECODE_GRAPH=0 sets
    model = OpenVLA(sd, c, **kw)
    assert model.decode_graph
    f, tk, ln, ud = frame.to(dev), toks.to(dev), lens.to(dev), u.to(dev)
    lo, hi = eager.action_lo, eager.action_hi
    scalar_before = [m.sample(f, tk, ln, S, ud, 0.9, top_k=50, top_p=0.9, return_logprobs=True) for m in (eager, model)]
    ladder = sampling_ladder(P, S, [0, 0.7, 1.0, 1.3], top_k=[0, 0, 50, 0])
    # eager with a trace: every pick against the reference on the traced logits, greedy rows = the arg-max over the action bins
    tr = {}
    t, sel, lps = eager.sample(f, tk, ln, S, ud, ladder[0], top_k=ladder[1], top_p=ladder[2], trace=tr, return_logprobs=True)
    assert len(tr["logits"]) == n_gen
    t_c, lps_c = t.cpu(), lps.cpu()
    _check_steps(tr["logits"], [t_c[:, i] for i in range(n_gen)], None, [lps_c[:, i].numpy() for i in range(n_gen)], lo, hi, u, *ladder, what="OpenVLA ladder")
    for i, lg in enumerate(tr["logits"]):
        assert float(sel[0, i]) == float(lg[0, int(t[0, i])]) and int(t[0, i]) == lo + int(lg[0, lo:hi].argmax())   # candidate 0 is greedy
    # the graph path equals eager; a second ladder reuses the captured graph
    e1 = eager.sample(f, tk, ln, S, ud, ladder[0], top_k=ladder[1], top_p=ladder[2], return_logprobs=True)
    assert all(same(a, b) for a, b in zip(e1, (t, sel, lps)))
    for _ in range(2):                                                      # the capturing call, then a replay
        g1 = model.sample(f, tk, ln, S, ud, ladder[0], top_k=ladder[1], top_p=ladder[2], return_logprobs=True)
        assert all(same(a, b) for a, b in zip(g1, e1))
    n_entries = len(model._dec)
    ladder2 = sampling_ladder(P, S, [0.5, 0, 1.5, 0.9], top_k=[5, 0, 0, 0], top_p=[1.0, 1.0, 0.8, 1.0])
    g2 = model.sample(f, tk, ln, S, ud, torch.from_numpy(ladder2[0]).to(dev), top_k=list(ladder2[1]), top_p=ladder2[2], return_logprobs=True)
    e2 = eager.sample(f, tk, ln, S, ud, ladder2[0], top_k=ladder2[1], top_p=ladder2[2], return_logprobs=True)
    assert len(model._dec) == n_entries and all(same(a, b) for a, b in zip(g2, e2)) and not same(g2[0], g1[0])
    g1b = model.sample(f, tk, ln, S, ud, ladder[0], top_k=ladder[1], top_p=ladder[2], return_logprobs=True)
    assert len(model._dec) == n_entries and all(same(a, b) for a, b in zip(g1b, e1))
    # one per-row argument is enough; top_logprobs ranks under each row's own distribution
    tl = eager.sample(f, tk, ln, S, ud, 0.9, top_k=ladder[1], top_logprobs=3)[2]
    assert tl.tokens.shape == (P * S, n_gen, 3) and (tl.tokens[:, :, 0] >= lo).all() and torch.isfinite(tl.entropy).all()
    with pytest.raises(ValueError):
        eager.sample(f, tk, ln, S, None, ladder[0])
    # device tensors are validated like host values (one read-back): an invalid row never becomes a -1 fed to the embedding gather;
    # natural dtypes (float64 temperature, int64 top_k) are cast
    T_dev = torch.from_numpy(ladder[0]).to(dev)
    for m in (eager, model):
        for bad in (dict(temperature=T_dev.clone().index_fill_(0, torch.tensor([2], device=dev), float("nan"))),
                    dict(temperature=T_dev, top_k=torch.tensor(ladder[1], device=dev).index_fill_(0, torch.tensor([5], device=dev), -1)),
                    dict(temperature=T_dev, top_p=torch.tensor(ladder[2], device=dev).index_fill_(0, torch.tensor([7], device=dev), 0.0))):
            with pytest.raises(CoverError):
                m.sample(f, tk, ln, S, ud, **bad)
        assert len(model._dec) == n_entries
        nat = m.sample(f, tk, ln, S, ud, T_dev.double(), top_k=torch.tensor(ladder[1], dtype=torch.int64, device=dev), top_p=ladder[2], return_logprobs=True)
        assert all(same(a, b) for a, b in zip(nat, e1))
    # an all-scalar call is untouched: the same results before and after the ladder calls, and a ladder of equal rungs is the scalar
    # filtered call bit for bit (one kernel body)
    for m, before in zip((eager, model), scalar_before):
        after = m.sample(f, tk, ln, S, ud, 0.9, top_k=50, top_p=0.9, return_logprobs=True)
        assert all(same(a, b) for a, b in zip(after, before))
        flat = m.sample(f, tk, ln, S, ud, [0.9] * (P * S), top_k=50, top_p=0.9, return_logprobs=True)
        assert all(same(a, b) for a, b in zip(flat, before))
    assert all(same(a, b) for a, b in zip(*scalar_before))


# ------------------------------------------------------------------------------------------------ 9. pi0-FAST
TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def test_pi0fast_ladder(dev):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, L, n_new = 6, 9, 12
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    toks, pad = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    toks[:, :L - 2] = torch.randint(2, 500, (L - 2,), generator=g)          # identical frames and prompt in every row
    pad[:, :L - 2] = 1
    args = ([img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev))
    g = torch.Generator().manual_seed(9)
    u = torch.rand(B, n_new, generator=g)
    force = torch.randint(2, 500, (B, n_new), generator=g)
    T = np.array([1.0, 0.0, 0.8, 1.0, 1.3, 0.5], dtype=np.float32)          # one greedy row
    k = np.array([0, 0, 50, 0, 20, 1], dtype=np.int32)
    p = np.array([1.0, 1.0, 0.9, 0.7, 1.0, 1.0], dtype=np.float32)
    scalar_before = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=0.8, top_k=50, top_p=0.9, eos_token_id=-1)
    for share in (False, True):
        tr = {}
        out, lps = model.generate_tokens(*args, n_new, force_tokens=force, trace=tr, uniforms=u.to(dev), temperature=T, top_k=list(k), top_p=torch.from_numpy(p),
                                         return_logprobs=True, share_prefix=share, eos_token_id=-1)
        assert len(tr["logits"]) == n_new == len(tr["picks"]) and all(lg.shape[0] == B for lg in tr["logits"])     # every row decoded on its own
        assert tr["prefix_slots"] == (1 if share else B)
        _check_steps(tr["logits"], [t.cpu() for t in tr["picks"]], [kk.cpu() for kk in tr["kept"]], None, 0, TINY["vocab"], u, T, k, p,
                     what=f"pi0-FAST ladder share_prefix={share}")
        assert torch.equal(out.cpu(), force) and torch.isfinite(lps).all() and torch.isfinite(lps.sum(dim=1)).all() and (lps <= 1e-6).all()
        # free-running: the greedy row is the arg-max of every step, the result is repeatable
        tr = {}
        free = model.generate_tokens(*args, n_new, trace=tr, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=-1)
        assert all(int(free[1, i]) == int(lg[1].argmax()) for i, lg in enumerate(tr["logits"]))
        assert torch.equal(model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=-1), free)
        # pad after EOS, and 0.0 log-probability on those steps
        eos = int(free[0, 2])
        out_e, lp_e = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=eos,
                                            return_logprobs=True)
        out_e, lp_e = out_e.cpu(), lp_e.cpu()
        hit = 0
        for r in range(B):
            pos = (out_e[r] == eos).nonzero()
            if pos.numel():
                first = int(pos[0])
                hit += 1
                assert (out_e[r, first + 1:] == 0).all() and (out_e[r, :first] != eos).all() and (lp_e[r, first + 1:] == 0).all()
        assert hit >= 1 and int((out_e[0] == eos).nonzero()[0]) <= 2 and torch.isfinite(lp_e.sum(dim=1)).all()
    tl = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_logprobs=3, eos_token_id=-1)[1]
    assert tl.tokens.shape == (B, n_new, 3) and (tl.tokens[:, :, 0] >= 0).all() and torch.isfinite(tl.entropy).all()
    with pytest.raises(ValueError):
        model.generate_tokens(*args, n_new, temperature=T)                  # per-row parameters need uniforms
    for share in (False, True):                                             # an invalid device-side row is refused before the decode loop
        for bad in (dict(temperature=torch.tensor(T, device=dev).index_fill_(0, torch.tensor([3], device=dev), -1.0)),
                    dict(temperature=T, top_k=torch.tensor([0, 0, -1, 0, 0, 0], device=dev)),
                    dict(temperature=T, top_p=torch.tensor(p, device=dev).double().index_fill_(0, torch.tensor([4], device=dev), float("nan")))):
            with pytest.raises(CoverError):
                model.generate_tokens(*args, n_new, uniforms=u.to(dev), share_prefix=share, eos_token_id=-1, **bad)
    nat = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=torch.tensor(T, device=dev).double(),
                                top_k=torch.tensor(k, dtype=torch.int64, device=dev), top_p=p, eos_token_id=-1)
    assert torch.equal(nat, model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, eos_token_id=-1))
    assert torch.equal(model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=0.8, top_k=50, top_p=0.9, eos_token_id=-1), scalar_before)
