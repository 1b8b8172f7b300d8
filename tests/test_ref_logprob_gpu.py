"""The reference score of the per-row sampler on the GPU (ops.token_sample_rows(ref_temperature=, out_ref_logprob=), cover_token_sample_rows_ref):
bit for bit against the scorer at (T_ref, 0, 1), nothing else moves, the float64 reference, the reuse branch, allowed-token sets, constructed
and invalid rows, row independence, graph replay, refused arguments, decode_feedback's second column, and the two policies that carry the
column up (OpenVLA.sample, PI0FASTTokens.generate_tokens, PI0FASTPolicy). Inputs: the three shapes and the eight-rung LADDER of
tests/sample_rows_ref.py (narrow: the list path; mid: unaligned head, one column more than the LDS list holds; wide: many tiles)."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd.host import sampling_ladder, sequence_logprob
from tests import allow_ref as AR
from tests import feedback_ref as FR
from tests import ref_logprob_ref as RF
from tests import sample_rows_ref as RR
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T_REFS = (1.0, 0.7, 2.0)
NAMES = list(RR.CASES)


def bits(t):
    """Floats compared as bit patterns: NaN equals NaN, -0.0 differs from +0.0."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def _dev(*arrays):
    return tuple(None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()
                 for a in arrays)


def _plain(x, lo, hi, u, T, k, p, allow=None):
    """The launch without the reference -> (tok, logit, kept, logprob)."""
    lp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    tok, lg, kept = ops.token_sample_rows(x, lo, hi, u, T, k, p, out_logprob=lp, allow=allow)
    return tok, lg, kept, lp


def _ref(x, lo, hi, u, T, k, p, t_ref, allow=None):
    """The launch with the reference -> (tok, logit, kept, logprob, ref); ref starts as a pattern the kernel must overwrite."""
    lp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    ref = torch.full((x.shape[0],), 77.0, dtype=torch.float32, device=x.device)
    tok, lg, kept = ops.token_sample_rows(x, lo, hi, u, T, k, p, out_logprob=lp, allow=allow, ref_temperature=t_ref, out_ref_logprob=ref)
    return tok, lg, kept, lp, ref


def _score(x, lo, hi, tok, t_ref, allow=None):
    """The scorer at (T_ref, 0, 1): what the reference column must equal bit for bit."""
    return ops.token_logprob_rows(x, lo, hi, tok, torch.full((x.shape[0],), t_ref, dtype=torch.float32, device=x.device), None, None, allow=allow)


@functools.lru_cache(maxsize=None)
def case(name):
    x, u, lo, hi, params, _ = RR.case_data(name)
    xd, ud = _dev(x, u)
    pd = _dev(*params)
    out = _plain(xd, lo, hi, ud, *pd)
    torch.cuda.synchronize()
    return xd, ud, lo, hi, pd, out


@functools.lru_cache(maxsize=None)
def with_ref(name, t_ref):
    xd, ud, lo, hi, pd, _ = case(name)
    out = _ref(xd, lo, hi, ud, *pd, t_ref)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def allowed_case(name):
    x, u, lo, hi, params, on, sor, _ = AR.case_data(name)
    xd, ud, lo, hi, pd, _ = case(name)
    words = torch.from_numpy(AR.pack_bits(on).view(np.int32)).view(torch.uint32).to(DEV)
    allow = ops.TokenAllow(words, _dev(sor)[0])
    return xd, ud, lo, hi, pd, allow, on, sor


def _idx(rows, j):
    return torch.tensor([r for r in range(rows) if r % len(RR.LADDER) == j], device=DEV)


# ------------------------------------------------------------------------------------------------ 1. + 2. the scorer, and nothing else moves
@pytest.mark.parametrize("t_ref", T_REFS)
@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_scorer_bit_for_bit_and_nothing_else_moves(dev, name, t_ref):
    xd, ud, lo, hi, pd, plain = case(name)
    tok, lg, kept, lp, ref = with_ref(name, t_ref)
    for a, b, what in zip((tok, lg, kept, lp), plain, ("token", "logit", "kept", "logprob")):
        assert same(a, b), (name, t_ref, what)
    want = _score(xd, lo, hi, tok, t_ref)
    rows = xd.shape[0]
    for j, rung in enumerate(RR.LADDER):                                    # greedy, unfiltered, compacted top-k, top-p, both, k = 1
        idx = _idx(rows, j)
        assert same(ref[idx], want[idx]), (name, t_ref, rung)
    assert torch.isfinite(ref).all() and (ref <= 0).all()


# ------------------------------------------------------------------------------------------------ 3. float64
@pytest.mark.parametrize("t_ref", T_REFS)
@pytest.mark.parametrize("name", NAMES)
def test_reference_matches_float64(dev, name, t_ref):
    x = RR.case_data(name)[0]
    xd, ud, lo, hi, pd, plain = case(name)
    tok, _, _, _, ref = with_ref(name, t_ref)
    RF.check_ref_logprobs(ref.cpu().numpy(), tok.cpu().numpy(), x.numpy(), lo, hi, t_ref, what=f"{name} T_ref={t_ref}")


# ------------------------------------------------------------------------------------------------ 4. reuse
@pytest.mark.parametrize("name", NAMES)
def test_rows_that_are_the_reference_reuse_their_own_score(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), plain = case(name)
    rows = xd.shape[0]
    tok, lg, kept, lp, ref = with_ref(name, 1.0)
    for j in (0, 1):                                                        # LADDER[0] greedy (scored at 1, unfiltered), LADDER[1] = (1, 0, 1)
        assert RR.LADDER[j] in ((0, 0, 1), (1, 0, 1))
        idx = _idx(rows, j)
        assert same(ref[idx], lp[idx]), (name, j)
    for t_ref in (0.7, 2.0):                                                # greedy rows are NOT the reference there; the ladder has no such rung
        r2 = with_ref(name, t_ref)[4]
        assert not same(r2[_idx(rows, 0)], lp[_idx(rows, 0)])
        # every row an unfiltered row at T_ref (top_k >= n and top_p = 1 count as unfiltered): the column is the launch's own log-probability
        Tf = torch.full_like(Td, t_ref)
        kf = torch.where(torch.arange(rows, device=DEV) % 2 == 0, 0, hi - lo).to(torch.int32)
        out = _ref(xd, lo, hi, ud, Tf, kf, torch.ones_like(pd), t_ref)
        assert same(out[4], out[3]) and same(out[4], _score(xd, lo, hi, out[0], t_ref)), (name, t_ref)
        assert all(same(a, b) for a, b in zip(out[:4], _plain(xd, lo, hi, ud, Tf, kf, torch.ones_like(pd))))


# ------------------------------------------------------------------------------------------------ 5. allowed-token sets
@pytest.mark.parametrize("t_ref", T_REFS)
@pytest.mark.parametrize("name", NAMES)
def test_allowed_sets(dev, name, t_ref):
    xd, ud, lo, hi, (Td, kd, pd), allow, on, sor = allowed_case(name)
    base = _ref(xd, lo, hi, ud, Td, kd, pd, t_ref, allow=allow)
    assert all(same(a, b) for a, b in zip(base[:4], _plain(xd, lo, hi, ud, Td, kd, pd, allow=allow))), (name, t_ref)
    assert same(base[4], _score(xd, lo, hi, base[0], t_ref, allow=allow)), (name, t_ref)
    assert torch.isfinite(base[4]).all()
    x = RR.case_data(name)[0]
    RF.check_ref_logprobs(base[4].cpu().numpy(), base[0].cpu().numpy(), x.numpy(), lo, hi, t_ref, allowed_rows=on[sor], what=f"{name} allowed T_ref={t_ref}")
    if t_ref == T_REFS[0]:
        # disallowed columns never reach the arithmetic
        dis = torch.from_numpy(~on[sor]).to(DEV)
        dis[:, :lo] = False
        dis[:, hi:] = False
        for v in (float("nan"), float("inf"), 3e38):
            got = _ref(torch.where(dis, torch.full_like(xd, v), xd), lo, hi, ud, Td, kd, pd, t_ref, allow=allow)
            assert all(same(a, b) for a, b in zip(got, base)), (name, v)
        # an all-ones set is the unmasked launch
        ones = ops.TokenAllow(torch.full((1, allow.bits.shape[1]), -1, dtype=torch.int32, device=DEV).view(torch.uint32))
        got = _ref(xd, lo, hi, ud, Td, kd, pd, t_ref, allow=ones)
        assert all(same(a, b) for a, b in zip(got, with_ref(name, t_ref))), name
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. constructed rows
def test_invalid_rows_and_rows_without_mass(dev):
    rows, ld, lo, hi = 8, 5000, 5, 4517                                     # 4512 columns: wider than the LDS candidate list
    x, u = R.lm_like_rows(7306, rows, ld, lo, hi)
    ninf, nan = float("-inf"), float("nan")
    x[2, lo:hi] = ninf                                                      # a sampled row without any mass
    x[5, lo:hi] = ninf                                                      # a greedy row of -inf
    x[7, lo + 100:lo + 3000] = ninf                                         # a row with a stretch of -inf
    good = (torch.tensor([1.0, 1, 0.7, 1, 1, 0, 1.3, 0.5]), torch.tensor([0, 0, 64, 50, 0, 0, 20, 1], dtype=torch.int32),
            torch.tensor([1, 1, 0.95, 1, 0.9, 1, 0.8, 1.0]))
    T, k, p = (t.clone() for t in good)
    T[1], p[4], k[6] = nan, 0.0, -1
    invalid = [1, 4, 6]
    valid = [r for r in range(rows) if r not in invalid]
    xd, ud = _dev(x, u)
    for t_ref in T_REFS:
        ref_good = _ref(xd, lo, hi, ud, *_dev(*good), t_ref)
        assert same(ref_good[4], _score(xd, lo, hi, ref_good[0], t_ref))     # the rows of -inf included: whatever the scorer writes
        got = _ref(xd, lo, hi, ud, *_dev(T, k, p), t_ref)
        torch.cuda.synchronize()
        assert torch.isnan(got[4][invalid]).all() and (got[0][invalid] == -1).all() and torch.isnan(got[3][invalid]).all()
        assert all(same(a[valid], b[valid]) for a, b in zip(got, ref_good)), t_ref
        assert all(same(a, b) for a, b in zip(got[:4], _plain(xd, lo, hi, ud, *_dev(T, k, p))))
    # sets: a bad set index, an empty set, and a row whose ALLOWED logits are all -inf (the pick is the first allowed column)
    on = np.zeros((3, ld), dtype=bool)
    on[0, lo + 50:lo + 90] = True
    on[1, ::3] = True                                                       # set 2 stays empty
    x2 = x.clone()
    x2[0, lo + 50:lo + 90] = ninf
    x2d = _dev(x2)[0]
    words = torch.from_numpy(AR.pack_bits(on).view(np.int32)).view(torch.uint32).to(DEV)
    sor_good = torch.tensor([0, 1, 1, 0, 1, 1, 0, 1], dtype=torch.int32, device=DEV)
    sor_bad = sor_good.clone()
    sor_bad[3], sor_bad[7] = 2, 5                                           # empty set, index out of range
    bad_rows = [3, 7]
    ok_rows = [r for r in range(rows) if r not in bad_rows]
    for t_ref in T_REFS:
        al = ops.TokenAllow(words, sor_good)
        ref_good = _ref(x2d, lo, hi, ud, *_dev(*good), t_ref, allow=al)
        assert int(ref_good[0][0]) == lo + 50
        assert same(ref_good[4], _score(x2d, lo, hi, ref_good[0], t_ref, allow=al))
        got = _ref(x2d, lo, hi, ud, *_dev(*good), t_ref, allow=ops.TokenAllow(words, sor_bad))
        torch.cuda.synchronize()
        assert torch.isnan(got[4][bad_rows]).all() and (got[0][bad_rows] == -1).all()
        assert all(same(a[ok_rows], b[ok_rows]) for a, b in zip(got, ref_good)), t_ref
    # rows without a maximum through both _ref kernels: allowed columns all NaN -> the first allowed column (row 0 sampled, row 3 greedy:
    # set 0; row 5 greedy: set 1, columns 0, 3, 6, ...); unmasked, the greedy row 5 of NaNs -> column lo. The reference score is the scorer's.
    x3 = x.clone()
    x3[0, lo + 50:lo + 90] = nan
    x3[3, lo + 50:lo + 90] = nan
    x3[5, lo:hi] = nan
    x3d = _dev(x3)[0]
    Tg = good[0].clone()
    Tg[3] = 0.0
    par = _dev(Tg, good[1], good[2])
    al = ops.TokenAllow(words, sor_good)
    for t_ref in T_REFS:
        got = _ref(x3d, lo, hi, ud, *par, t_ref, allow=al)
        assert [int(got[0][r]) for r in (0, 3, 5)] == [lo + 50, lo + 50, 6] and torch.isnan(got[1][[0, 3, 5]]).all()
        assert same(got[4], _score(x3d, lo, hi, got[0], t_ref, allow=al))
        assert all(same(a, b) for a, b in zip(got[:4], _plain(x3d, lo, hi, ud, *par, allow=al)))
        got = _ref(x3d, lo, hi, ud, *par, t_ref)
        assert int(got[0][5]) == lo and bool(torch.isnan(got[1][5])) and int(got[2][5]) == hi - lo
        assert same(got[4], _score(x3d, lo, hi, got[0], t_ref))
        assert all(same(a, b) for a, b in zip(got[:4], _plain(x3d, lo, hi, ud, *par)))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 7. row independence
@pytest.mark.parametrize("name", NAMES)
def test_rows_are_independent(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), _ = case(name)
    t_ref = 0.7
    out = with_ref(name, t_ref)
    fl = lambda t: t.flip(0).contiguous()
    rev = _ref(fl(xd), lo, hi, fl(ud), fl(Td), fl(kd), fl(pd), t_ref)
    assert all(same(a.flip(0), b) for a, b in zip(rev, out)), name
    for r in range(xd.shape[0]):
        one = _ref(xd[r:r + 1], lo, hi, ud[r:r + 1], Td[r:r + 1].clone(), kd[r:r + 1].clone(), pd[r:r + 1].clone(), t_ref)
        assert all(same(a, b[r:r + 1]) for a, b in zip(one, out)), (name, r)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. graph
@pytest.mark.parametrize("masked", (False, True))
def test_graph_replay_follows_the_buffers(dev, masked):
    xd, ud, lo, hi, (Td, kd, pd), allow, on, sor = allowed_case("mid")
    al = allow if masked else None
    t_ref = 0.7
    rows = xd.shape[0]
    roll = lambda t: torch.roll(t, 3, 0).contiguous()
    x2, u2 = roll(xd) * 1.25, (ud * 0.5 + 0.25).contiguous()
    first = _ref(xd, lo, hi, ud, Td, kd, pd, t_ref, allow=al)
    second = _ref(x2, lo, hi, u2, roll(Td), roll(kd), roll(pd), t_ref, allow=al)
    assert not same(second[0], first[0]) and not same(second[4], first[4])
    xs, us, Ts, ks, ps = xd.clone(), ud.clone(), Td.clone(), kd.clone(), pd.clone()     # the static buffers of the capture
    tok = torch.empty(rows, dtype=torch.int64, device=dev)
    lg, lp, ref = (torch.empty(rows, device=dev) for _ in range(3))
    kept = torch.empty(rows, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with ops.Graph() as gr:
            ops.token_sample_rows(xs, lo, hi, us, Ts, ks, ps, out_tok=tok, out_logit=lg, out_kept=kept, out_logprob=lp, allow=al,
                                  ref_temperature=t_ref, out_ref_logprob=ref)
        for want, src in ((first, (xd, ud, Td, kd, pd)), (second, (x2, u2, roll(Td), roll(kd), roll(pd))), (first, (xd, ud, Td, kd, pd))):
            for dst, s in zip((xs, us, Ts, ks, ps), src):
                dst.copy_(s)
            tok.fill_(-1)
            ref.fill_(77.0)
            gr.launch()
            side.synchronize()
            assert all(same(a, b) for a, b in zip((tok, lg, kept, lp, ref), want))
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ 9. refused arguments
def test_c_entry_point_refuses_bad_arguments(dev):
    from cover_vla_amd import _lib as L
    x, u, T = torch.zeros(4, 64, device=dev), torch.zeros(4, device=dev), torch.ones(4, device=dev)
    tok = torch.full((4,), -7, dtype=torch.int64, device=dev)
    out = torch.full((4,), -7.0, device=dev)
    words = torch.full((1, 2), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(t_ref=1.0, out_ptr=out.data_ptr(), null_ref=False, allow=None, **over):
        a = L.TokenSampleRowsArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi, a.temperature = x.data_ptr(), 64, 4, 0, 64, T.data_ptr()
        a.uniform, a.token_out = u.data_ptr(), tok.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        r = L.TokenRef()
        r.temperature, r.logprob_out = t_ref, out_ptr
        al = None
        if allow is not None:
            al = L.TokenAllow()
            al.bits, al.ld_words, al.n_sets, al.set_of_row = words.data_ptr(), 2, 1, None
            for k, v in allow.items():
                setattr(al, k, v)
            al = C.byref(al)
        return L.lib().cover_token_sample_rows_ref(C.byref(a), al, None if null_ref else C.byref(r), st)

    for t_ref in (0.0, -1.0, float("nan"), float("inf")):
        assert call(t_ref=t_ref) == -1 and call(t_ref=t_ref, allow={}) == -1, t_ref       # COVER_EINVAL
    assert call(out_ptr=None) == -1 and call(null_ref=True) == -1
    for over in (dict(hi=0), dict(lo=-1), dict(rows=-1), dict(logits=None), dict(temperature=None), dict(uniform=None), dict(token_out=None)):
        assert call(**over) == -1, over                                     # everything the underlying call refuses
    for al in (dict(bits=None), dict(n_sets=0), dict(ld_words=1)):
        assert call(allow=al) == -1, al
    assert L.lib().cover_token_sample_rows_ref(None, None, None, st) == -1
    torch.cuda.synchronize()
    assert (tok == -7).all() and (out == -7.0).all()                        # nothing was launched
    assert call() == 0 and call(allow={}) == 0
    torch.cuda.synchronize()
    assert (tok >= 0).all() and float((out + float(np.log(64.0))).abs().max()) < 1e-6    # 64 equal columns at any temperature
    a = L.DecodeFeedbackArgs()
    assert L.lib().cover_decode_feedback_lp2(None, None, None, 0, st) == -1
    done = torch.zeros(4, dtype=torch.bool, device=dev)
    a.pick, a.done, a.tok_out, a.ld_tok, a.rows = tok.data_ptr(), done.data_ptr(), tok.data_ptr(), 1, 4
    before = tok.clone()
    assert L.lib().cover_decode_feedback_lp2(C.byref(a), None, out.data_ptr(), 1, st) == -1
    assert L.lib().cover_decode_feedback_lp2(C.byref(a), out.data_ptr(), None, 1, st) == -1
    torch.cuda.synchronize()
    assert torch.equal(tok, before) and not done.any()


# ------------------------------------------------------------------------------------------------ 10. decode_feedback(lp2=)
def test_decode_feedback_second_column(dev):
    B, n, V, D, eos, pad = 9, 6, 40, 64, 3, 0
    g = torch.Generator().manual_seed(21)
    picks = torch.randint(4, V, (B, n), generator=g)
    picks[1, 0] = eos                                                       # finishes in the first step
    picks[4, 2] = eos                                                       # finishes in step 2: its value counts there, 0.0 afterwards
    picks[7, 5] = eos
    lps, lp2s = -torch.rand(B, n, generator=g), -torch.rand(B, n, generator=g) * 3
    table = (torch.randn(V, D, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    want_tok, want_done, want_lp, want_live = FR.run(picks.numpy(), eos, pad, lps=lps.numpy())
    want_lp2 = FR.run(picks.numpy(), eos, pad, lps=lp2s.numpy())[2]

    def run(second, first=True):
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        out = torch.full((B, n), -5, dtype=torch.int64, device=dev)
        lo1, lo2 = torch.full((B, n + 3), 9.0, device=dev), torch.full((B, n + 1), 9.0, device=dev)
        live = torch.zeros(n, dtype=torch.int32, device=dev)
        xs = []
        for i in range(n):
            x_out = torch.empty(B, D, dtype=torch.bfloat16, device=dev) if i + 1 < n else None
            kw = dict(lp2=lp2s[:, i].contiguous().to(dev), lp2_out=lo2) if second else {}
            if first:
                kw.update(lp=lps[:, i].contiguous().to(dev), lp_out=lo1)
            ops.decode_feedback(picks[:, i].contiguous().to(dev), done, out, i, eos, pad, table=table, scale=1.5, x_out=x_out, live=live, **kw)
            xs.append(x_out)
        torch.cuda.synchronize()
        return done, out, lo1, lo2, live, xs

    base = run(False)
    got = run(True)
    assert torch.equal(got[3][:, :n].cpu(), torch.from_numpy(want_lp2)) and (got[3][:, n:] == 9.0).all()
    assert torch.equal(got[2][:, :n].cpu(), torch.from_numpy(want_lp)) and torch.equal(got[1].cpu(), torch.from_numpy(want_tok))
    assert float(got[3][4, 2]) == float(lp2s[4, 2]) and (got[3][4, 3:n] == 0).all() and (got[3][1, 1:n] == 0).all()
    for a, b in zip((got[0], got[1], got[2], got[4]), (base[0], base[1], base[2], base[4])):       # every other output: the call without lp2
        assert torch.equal(a, b)
    assert all(a is None and b is None or same(a.float(), b.float()) for a, b in zip(got[5], base[5]))
    assert (base[3] == 9.0).all()
    only = run(True, first=False)                                           # the second column without the first
    assert torch.equal(only[3], got[3]) and (only[2] == 9.0).all() and torch.equal(only[1], got[1])


# ------------------------------------------------------------------------------------------------ 11. models
def _step_scores(logits, toks, lo, hi, t_ref, allow=None):
    """ops.token_logprob_rows at (T_ref, 0, 1) per traced step on that step's logits and picks -> fp32 [N, steps]."""
    cols = [_score(lg.float().contiguous(), lo, hi, toks[:, i].contiguous(), t_ref, allow=allow) for i, lg in enumerate(logits)]
    return torch.stack(cols, dim=1)


def test_openvla_prior_column(dev):
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
    eager.decode_graph = False
    model = OpenVLA(sd, c, **kw)
    assert model.decode_graph
    f, tk, ln, ud = frame.to(dev), toks.to(dev), lens.to(dev), u.to(dev)
    lo, hi = eager.action_lo, eager.action_hi
    # rung 0 is the arg-max, rung 1 top_k = 1 (which keeps the arg-max alone)
    ladder = sampling_ladder(P, S, [0, 0.5, 1.0, 1.3], top_k=[0, 1, 50, 0], top_p=[1.0, 1.0, 1.0, 0.9])
    lkw = dict(top_k=ladder[1], top_p=ladder[2])
    for m in (eager, model):
        plain = m.sample(f, tk, ln, S, ud, ladder[0], return_logprobs=True, **lkw)
        plain2 = m.sample(f, tk, ln, S, ud, ladder[0], **lkw)
        tr = {} if m is eager else None
        got = m.sample(f, tk, ln, S, ud, ladder[0], return_logprobs=True, prior_temperature=1.0, trace=tr, **lkw)
        assert len(got) == 4 and all(same(a, b) for a, b in zip(got[:3], plain))
        t, sel, lps, prior = got
        assert prior.dtype == torch.float32 and tuple(prior.shape) == (P * S, n_gen) and torch.isfinite(prior).all()
        got2 = m.sample(f, tk, ln, S, ud, ladder[0], prior_temperature=1.0, **lkw)          # without return_logprobs: the third tensor
        assert len(got2) == 3 and all(same(a, b) for a, b in zip(got2[:2], plain2)) and same(got2[2], prior)
        if m is eager:
            assert len(tr["logits"]) == n_gen
            assert same(prior, _step_scores(tr["logits"], t, lo, hi, 1.0))
            eager_prior = prior
        else:
            assert same(prior, eager_prior)
            again = m.sample(f, tk, ln, S, ud, ladder[0], return_logprobs=True, prior_temperature=1.0, **lkw)     # first and second replay
            third = m.sample(f, tk, ln, S, ud, ladder[0], return_logprobs=True, prior_temperature=1.0, **lkw)
            assert all(same(a, b) for a, b in zip(again, got)) and all(same(a, b) for a, b in zip(third, got))
        # own scores do not compare across rungs: a top_k = 1 rung scores each of its picks 0.0 (-log(ties) where several bins share the
        # maximum: ties with the k-th value stay, and this small model has them), the reference scores the same pick against every bin; a greedy
        # rung is scored at temperature 1, unfiltered, which T_ref = 1 is. The equal-tokens case is test_pi0fast_prior_column's.
        for q in range(P):
            a, b = q * S, q * S + 1
            assert (lps[b] > -1.5).all() and (prior[b] < -1e-3).all() and (lps[b] >= prior[b]).all() and not same(lps[b], prior[b])
            assert same(prior[a], lps[a]) and (lps[a] < -1e-3).all()
    # another reference temperature is another graph key and another value
    n_entries = len(model._dec)
    p07 = model.sample(f, tk, ln, S, ud, ladder[0], prior_temperature=0.7, **lkw)
    assert len(model._dec) == n_entries + 1
    e07 = eager.sample(f, tk, ln, S, ud, ladder[0], prior_temperature=0.7, **lkw)
    assert all(same(a, b) for a, b in zip(p07, e07)) and not same(p07[2], eager_prior)
    model.sample(f, tk, ln, S, ud, ladder[0], prior_temperature=0.7, **lkw)
    assert len(model._dec) == n_entries + 1
    # scalar parameters are broadcast; an all-greedy call is refused with a pointer to temperature=0 rows
    flat = eager.sample(f, tk, ln, S, ud, 0.9, top_k=50, top_p=0.9, return_logprobs=True, prior_temperature=2.0)
    base = eager.sample(f, tk, ln, S, ud, 0.9, top_k=50, top_p=0.9, return_logprobs=True)
    assert all(same(a, b) for a, b in zip(flat[:3], base)) and torch.isfinite(flat[3]).all()
    with pytest.raises(ValueError, match="temperature=0"):
        eager.sample(f, tk, ln, S, None, prior_temperature=1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ops.L.CoverError):
            eager.sample(f, tk, ln, S, ud, 0.9, prior_temperature=bad)


TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def test_pi0fast_prior_column(dev, monkeypatch):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, L, n_new, V = 6, 9, 12, TINY["vocab"]
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    toks, pad = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    toks[:, :L - 2] = torch.randint(2, 500, (L - 2,), generator=g)          # identical frames and prompt in every row
    pad[:, :L - 2] = 1
    args = ([img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev))
    u = torch.rand(B, n_new, generator=torch.Generator().manual_seed(9)).to(dev)
    T = np.array([0.0, 0.5, 0.8, 1.0, 1.3, 1.0], dtype=np.float32)          # rows 0 and 1: the arg-max and top_k = 1, the same tokens
    k = np.array([0, 1, 50, 0, 20, 0], dtype=np.int32)
    p = np.array([1.0, 1.0, 0.9, 0.7, 1.0, 1.0], dtype=np.float32)
    lkw = dict(uniforms=u, temperature=T, top_k=k, top_p=p)
    al = ops.TokenAllow(ops.token_allow_sets(V, [[(300, 380), 1, 7, 33], [(64, 96), (400, 512)]], dev),
                        torch.tensor([0, 0, 1, 1, 0, 1], dtype=torch.int32, device=dev))
    shown = 0
    for share in (False, True):
        for fused in (("1", "0") if share else ("1",)):                   # the torch bookkeeping twin exists on the shared path only
            monkeypatch.setenv("COVER_FAST_FEEDBACK", fused)
            for t_ref, akw in ((1.0, {}), (0.7, {}), (1.0, dict(allowed_tokens=al))):
                kw = dict(share_prefix=share, eos_token_id=-1, **lkw, **akw)
                plain = model.generate_tokens(*args, n_new, return_logprobs=True, **kw)
                tr = {}
                out, lps, prior = model.generate_tokens(*args, n_new, return_logprobs=True, prior_temperature=t_ref, trace=tr, **kw)
                assert torch.equal(out, plain[0]) and same(lps, plain[1])
                assert prior.dtype == torch.float32 and tuple(prior.shape) == (B, n_new) and torch.isfinite(prior).all()
                assert same(prior, _step_scores(tr["logits"], out, 0, V, t_ref, allow=akw.get("allowed_tokens"))), (share, fused, t_ref)
                o2, pr2 = model.generate_tokens(*args, n_new, prior_temperature=t_ref, **kw)           # without return_logprobs
                assert torch.equal(o2, out) and same(pr2, prior)
                if not akw:
                    # the point of the column: two rungs that emit the same tokens from the same prompt (rows 0 and 1 see equal logits at every
                    # step) have the same prior bit for bit, while their own scores differ: the arg-max at temperature 1, top_k = 1 at 0.0
                    assert (lps[1] >= prior[1]).all() and not same(lps[1], prior[1]) and (lps[0] < -1e-3).all() and (prior[1] < -1e-3).all()
                    if all(torch.equal(lg[0], lg[1]) for lg in tr["logits"]):
                        assert torch.equal(out[0], out[1]) and same(prior[0], prior[1]) and not same(lps[0], lps[1])
                        shown += 1
                    if t_ref == 1.0:
                        assert same(prior[0], lps[0]) and same(prior[5], lps[5])                       # greedy, and (1, 0, 1): the reuse rows
            # pads after EOS carry 0.0: sequence_logprob applies unchanged
            free = model.generate_tokens(*args, n_new, share_prefix=share, eos_token_id=-1, **lkw)
            eos = int(free[0, 2])
            o_e, lp_e, pr_e = model.generate_tokens(*args, n_new, share_prefix=share, eos_token_id=eos, return_logprobs=True, prior_temperature=0.7, **lkw)
            o_p = model.generate_tokens(*args, n_new, share_prefix=share, eos_token_id=eos, return_logprobs=True, **lkw)
            assert torch.equal(o_e, o_p[0]) and same(lp_e, o_p[1])
            hit = 0
            for r in range(B):
                pos = (o_e[r] == eos).nonzero()
                first = int(pos[0]) if pos.numel() else n_new - 1
                hit += bool(pos.numel())
                assert (pr_e[r, first + 1:] == 0).all() and (pr_e[r, :first + 1] < 0).all() and (o_e[r, first + 1:] == 0).all()
            assert hit >= 1
            assert torch.equal(sequence_logprob(pr_e, o_e, pad_token_id=0), pr_e.sum(dim=1))
    monkeypatch.delenv("COVER_FAST_FEEDBACK")
    assert shown >= 1                                                       # the ladder case was met
    # scalar parameters are broadcast; an all-greedy call is refused with a pointer to temperature=0 rows
    flat = model.generate_tokens(*args, n_new, uniforms=u, temperature=0.8, top_k=50, top_p=0.9, eos_token_id=-1, prior_temperature=2.0)
    assert torch.equal(flat[0], model.generate_tokens(*args, n_new, uniforms=u, temperature=0.8, top_k=50, top_p=0.9, eos_token_id=-1))
    with pytest.raises(ValueError, match="temperature=0"):
        model.generate_tokens(*args, n_new, prior_temperature=1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ops.L.CoverError):
            model.generate_tokens(*args, n_new, uniforms=u, prior_temperature=bad)


def test_pi0fast_policy_keeps_the_prior(dev):
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTPolicy, PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=384, max_new_tokens=24)
    tok = synth.CharTokenizer(vocab_size=512)
    fast = types.SimpleNamespace(bpe_tokenizer=types.SimpleNamespace(decode=lambda t: "".join(chr(max(0, min(int(i), 1000))) for i in t)),
                                 min_token=-40, scale=10.0)
    kw = dict(action_dim=7, chunk_size=5, n_action_steps=2, max_decoding_steps=24, resize_imgs_with_padding=(56, 56))
    g = torch.Generator().manual_seed(2)
    state = (torch.rand(1, 8, generator=g) * 2 - 1).repeat(4, 1)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(4, 1, 1, 1)
    batch = {"observation.state": state.to(dev), "observation.images.top": img.to(dev), "task": ["put the spoon on the towel"] * 4}
    ladder = dict(temperature=[0.0, 0.7, 1.0, 1.3], top_k=[0, 50, 0, 0], top_p=[1.0, 1.0, 0.9, 1.0], sample_seed=7)
    seen = {}
    orig = model.generate_tokens

    def spy(*a, **k):
        res = orig(*a, **k)
        seen["res"] = res
        return res
    for extra in (dict(), dict(return_logprobs=True), dict(top_logprobs=2), dict(return_logprobs=True, top_logprobs=2)):
        off = PI0FASTPolicy(PI0FASTConfig(**ladder, **extra, **kw), model, tok, fast)
        on = PI0FASTPolicy(PI0FASTConfig(**ladder, **extra, prior_temperature=1.0, **kw), model, tok, fast)
        assert on.last_sequence_prior_logprobs is None
        a0 = off.select_action(batch)
        model.generate_tokens = spy
        try:
            a1 = on.select_action(batch)
        finally:
            del model.generate_tokens
        assert torch.equal(a0, a1) and off.last_sequence_prior_logprobs is None
        s = on.last_sequence_prior_logprobs
        column = seen["res"][2 if extra.get("return_logprobs") else 1]
        assert s.dtype == torch.float32 and tuple(s.shape) == (4,) and s.is_cuda and torch.isfinite(s).all() and (s < 0).all()
        assert same(s, sequence_logprob(column))
        if extra.get("return_logprobs"):
            assert same(on.last_sequence_logprobs, off.last_sequence_logprobs)
            assert same(s[0], on.last_sequence_logprobs[0]) and not same(s[1], on.last_sequence_logprobs[1])     # row 0 is greedy, row 1 is not the reference
        if extra.get("top_logprobs"):
            assert on.last_top_logprobs.tokens.shape[2] == 2
