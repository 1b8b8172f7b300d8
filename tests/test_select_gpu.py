"""The older half of csrc/select.hip on the GPU, through cover_vla_amd.ops, against tests/select_ref.py: greedy cover_token_select on
both of its kernels and on each side of every clause of the host's dispatch predicate, its sampling path against the float64 inverse
CDF wherever the derived bound decides the pick, cover_score_select against the float64 cosine within its derived bound,
cover_group_argmax bit for bit, and the two history builders. tests/test_select_cpu.py holds the conditions that make the exact
comparisons legitimate. Every test prints its largest error next to its bound (pytest -s shows them)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import ops
from tests import member_scores_ref as MR
from tests import select_ref as SR

pytestmark = pytest.mark.gpu

F32 = np.float32
TOK_SENTINEL, LOGIT_SENTINEL = -777, -123.5


def _bits(x):
    return SR.bits(x.detach().cpu().numpy() if torch.is_tensor(x) else x)


def _same_bits(got, want):
    g, w = _bits(got), _bits(want)
    return g.shape == w.shape and np.array_equal(g, w)


# ================================================================================================ greedy token_select
def _greedy_view(dev, layout, names):
    buf, off, ld, lo, hi = SR.greedy_matrix(layout, names)
    d = torch.from_numpy(buf).to(dev)
    assert d.data_ptr() % 16 == 0
    view = torch.as_strided(d, (len(names), ld), (ld, 1), storage_offset=off)
    host = buf[off:off + len(names) * ld].reshape(len(names), ld)
    want = [SR.greedy(r, lo, hi) for r in host]
    return view, lo, hi, np.array([t for t, _ in want], dtype=np.int64), np.array([l for _, l in want], dtype=F32)


def _check_greedy(dev, layout, names):
    view, lo, hi, want_tok, want_lg = _greedy_view(dev, layout, names)
    rows = len(names)
    assert SR.is_wide(lo, hi - lo, view.stride(0), (view.data_ptr() % 16) // 4) == (SR.GREEDY_LAYOUTS[layout][4] == "wide")
    tok, lg = ops.token_select(view, lo, hi)
    assert np.array_equal(tok.cpu().numpy(), want_tok), (layout, names, tok.tolist(), want_tok.tolist())
    assert _same_bits(lg, want_lg), (layout, names)
    # outputs as one row of a [steps, rows] buffer: the other rows keep their sentinel
    tb = torch.full((3, rows), TOK_SENTINEL, dtype=torch.int64, device=dev)
    lb = torch.full((3, rows), LOGIT_SENTINEL, dtype=torch.float32, device=dev)
    ops.token_select(view, lo, hi, out_tok=tb[1], out_logit=lb[1])
    assert np.array_equal(tb[1].cpu().numpy(), want_tok) and _same_bits(lb[1], want_lg)
    assert bool((tb[[0, 2]] == TOK_SENTINEL).all()) and bool((lb[[0, 2]] == LOGIT_SENTINEL).all())
    # one greedy rule: the per-row sampler's temperature-0 row writes the same token and the same logit bits
    tok2, lg2, kept = ops.token_sample_rows(view, lo, hi, torch.zeros(rows, device=dev), torch.zeros(rows, device=dev))
    assert np.array_equal(tok2.cpu().numpy(), want_tok) and _same_bits(lg2, want_lg), (layout, names)
    assert kept.tolist() == [hi - lo] * rows
    return view, lo, hi, want_tok, want_lg


NUMBER_ROWS = tuple(n for n in SR.GREEDY_ROWS if n not in SR.GREEDY_NAN_ROWS)


@pytest.mark.parametrize("layout", list(SR.GREEDY_LAYOUTS))
def test_greedy_matches_reference_on_every_dispatch_clause(dev, layout):
    view, lo, hi, want_tok, want_lg = _check_greedy(dev, layout, NUMBER_ROWS)
    _check_greedy(dev, layout, NUMBER_ROWS[:5])                                   # rows = 5
    for name in ("tie-x3-first-wins", "max-in-tail"):                             # rows = 1
        _check_greedy(dev, layout, (name,))


@pytest.mark.parametrize("layout", list(SR.GREEDY_LAYOUTS))
def test_greedy_nan_rows_pick_inside_the_range(dev, layout):
    """A NaN never wins; a row of NaNs gives lo and the NaN stored at lo, payload included -- on both kernels, next to ordinary rows,
    and the per-row sampler's greedy row agrees bit for bit."""
    names = ("random", "all-nan", "nan-scattered", "max-at-hi-1", "all-nan")
    view, lo, hi, want_tok, want_lg = _check_greedy(dev, layout, names)
    assert want_tok[1] == lo == want_tok[4] and _bits(want_lg)[1] == SR.NAN_PAYLOAD
    assert lo < want_tok[2] < hi - 1 and want_lg[2] == F32(9.0)
    _check_greedy(dev, layout, ("all-nan",))


# ================================================================================================ sampling token_select
LO = 3                                                   # the sampled range starts three columns in; the columns outside are +inf


def _sample_matrix(dev, row, rows):
    n = row.size
    m = np.full((rows, LO + n + 2), np.inf, dtype=F32)
    m[:, LO:LO + n] = row
    return torch.from_numpy(m).to(dev)


@pytest.mark.parametrize("width", SR.WIDTHS)
def test_sampling_matches_the_float64_inverse_cdf_wherever_it_is_decided(dev, width):
    checked = 0
    for cell in [c for c in SR.CELLS if c[0] == width]:
        n, T, dist = cell
        c = SR.sampling_cell(cell)
        us = np.concatenate([c["kept"], np.array(SR.FIXED_U, dtype=F32)])
        logits = _sample_matrix(dev, c["row"], us.size)
        tok, lg = ops.token_select(logits, LO, LO + n, uniform=torch.from_numpy(us).to(dev), temperature=T)
        tok, lg = tok.cpu().numpy() - LO, lg.cpu().numpy()
        assert ((0 <= tok) & (tok < n)).all(), cell
        assert _same_bits(lg, c["row"][tok]), cell                                  # the input logit at the pick, bit for bit
        k = c["kept"].size
        assert k == SR.N_DRAWN and np.array_equal(tok[:k], c["picks"]), (cell, c["B"], tok[:k].tolist(), c["picks"].tolist())
        checked += k
        for j, u in enumerate(SR.FIXED_U):
            first, last = SR.fixed_expectation(cell, u)
            if dist == "flat" and n == 4096 and j == 2:                             # the fallback case: not asserted more sharply
                assert tok[k + j] >= n - 2
            else:
                assert first <= tok[k + j] <= last, (cell, float(u), int(tok[k + j]), first, last)
        if dist == "flat":
            assert tok[k] == 0                                                      # identical logits, u = 0: lo
        if T == 0.05 and dist == "peaked":
            assert (tok[:k] == int(np.argmax(c["row"]))).all()
    print(f"sampling width {width}: {checked} decided uniforms compared exactly, B up to "
          f"{max(SR.sampling_cell(c)['B'] for c in SR.CELLS if c[0] == width):.3e}")


def test_sampling_row_is_independent_of_its_position(dev):
    for cell in ((257, 0.7, "normal"), (4096, 1.0, "normal"), (1000, 20.0, "peaked")):
        n, T, _ = cell
        c = SR.sampling_cell(cell)
        u = c["kept"][:1]
        alone = ops.token_select(_sample_matrix(dev, c["row"], 1), LO, LO + n, uniform=torch.from_numpy(u).to(dev), temperature=T)
        others = SR.sampling_cell((n, T, "flat"))["row"]
        m = _sample_matrix(dev, others, 5)
        m[3, LO:LO + n] = torch.from_numpy(c["row"]).to(dev)
        us = torch.full((5,), 0.25, device=dev)
        us[3] = float(u[0])
        five = ops.token_select(m, LO, LO + n, uniform=us, temperature=T)
        assert int(five[0][3]) == int(alone[0][0]) == LO + int(c["picks"][0]) and _same_bits(five[1][3:4], alone[1])


def test_sampling_nan_row_stays_in_range_and_leaves_its_neighbours_alone(dev):
    for cell in ((257, 0.7, "normal"), (4096, 1.0, "normal")):
        n, T, _ = cell
        c = SR.sampling_cell(cell)
        m = _sample_matrix(dev, c["row"], 5)
        us = torch.from_numpy(c["kept"][:5].copy()).to(dev)
        tok0, lg0 = ops.token_select(m, LO, LO + n, uniform=us, temperature=T)
        for poison in ("one", "all"):
            bad = m.clone()
            if poison == "one":
                bad[2, LO + n // 2] = float("nan")
            else:
                bad[2, LO:LO + n] = float("nan")
            tok, lg = ops.token_select(bad, LO, LO + n, uniform=us, temperature=T)
            assert LO <= int(tok[2]) < LO + n, (cell, poison, int(tok[2]))
            keep = [0, 1, 3, 4]
            assert torch.equal(tok[keep], tok0[keep]) and _same_bits(lg[keep], lg0[keep]), (cell, poison)


def test_token_select_refusals_launch_nothing(dev):
    logits = torch.randn(4, 4200, device=dev)
    u = torch.full((4,), 0.5, device=dev)
    tok = torch.full((4,), TOK_SENTINEL, dtype=torch.int64, device=dev)
    lg = torch.full((4,), LOGIT_SENTINEL, dtype=torch.float32, device=dev)
    bad = [dict(lo=0, hi=4097, uniform=u, temperature=1.0), dict(lo=0, hi=256, uniform=u, temperature=0.0),
           dict(lo=0, hi=256, uniform=u, temperature=-1.0), dict(lo=0, hi=256, uniform=u, temperature=float("nan")),
           dict(lo=7, hi=7), dict(lo=8, hi=7), dict(lo=8, hi=7, uniform=u, temperature=1.0)]
    for kw in bad:
        with pytest.raises(L.CoverError):
            ops.token_select(logits, kw.pop("lo"), kw.pop("hi"), out_tok=tok, out_logit=lg, **kw)
    torch.cuda.synchronize()
    assert bool((tok == TOK_SENTINEL).all()) and bool((lg == LOGIT_SENTINEL).all())
    # rows = 0: success, nothing written
    a = L.TokenSelectArgs()
    a.logits, a.ld, a.rows, a.lo, a.hi = logits.data_ptr(), logits.stride(0), 0, 0, 256
    a.uniform, a.temperature = u.data_ptr(), 1.0
    a.token_out, a.logit_out = tok.data_ptr(), lg.data_ptr()
    assert L.lib().cover_token_select(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    a.uniform = None
    assert L.lib().cover_token_select(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert bool((tok == TOK_SENTINEL).all()) and bool((lg == LOGIT_SENTINEL).all())
    tok2, _ = ops.token_select(logits, 0, 4096, uniform=u, temperature=1.0, out_tok=tok, out_logit=lg)     # the limit itself is served
    assert bool(((tok2 >= 0) & (tok2 < 4096)).all())


# ================================================================================================ score_select
@pytest.mark.parametrize("case", SR.SCORE_CASES, ids=MR.case_id)
def test_score_select_within_the_derived_bound_of_float64(dev, case):
    M, N, gs, dim = case
    it, act = SR.score_inputs(case)
    scores, result, best, fit, fact = ops.score_select(torch.from_numpy(it).to(dev), torch.from_numpy(act).to(dev), gs)
    s, fit, fact = scores.cpu().numpy(), fit.cpu().numpy().astype(np.float64), fact.cpu().numpy().astype(np.float64)
    fit64, fact64, s64 = SR.fused_f64(it, act)
    eta_it, eta_act, bound = SR.score_bounds(it, act)
    err = np.abs(s.astype(np.float64) - s64)
    e_it, e_act = np.linalg.norm(fit - fit64), np.linalg.norm(fact - fact64, axis=-1)
    print(f"score_select {MR.case_id(case)}: score err {err.max():.3e} (bound {bound.max():.3e}), fused_it {e_it:.3e} ({eta_it:.3e}), "
          f"fused_act {e_act.max():.3e} ({eta_act.max():.3e})")
    assert (err <= bound).all(), (err.max(), bound.max())
    assert e_it <= eta_it and (e_act <= eta_act).all()
    assert abs(np.linalg.norm(fit) - 1) <= eta_it and (np.abs(np.linalg.norm(fact, axis=-1) - 1) <= eta_act).all()
    # the decision: group_argmax's fp32 chain on the device's own score bits, exactly -- and the float64 decision (margins > 2 x bound)
    want_r, want_b = SR.group_argmax(s, gs)
    assert np.array_equal(result.cpu().numpy(), want_r) and _same_bits(best, want_b)
    assert result.cpu().tolist()[:3] == SR.decision_f64(s64, gs)[0]


def test_score_select_candidate_position_does_not_change_its_bits(dev):
    M, N, gs, dim = SR.POSITIONS_CASE
    it, act = SR.score_inputs(SR.POSITIONS_CASE)
    act = act.copy()
    act[:, 19] = act[:, N - 1] = act[:, 3]               # wave 3 of block 0, wave 3 of block 1, wave 7 of the ragged block 2
    scores, _, _, _, fact = ops.score_select(torch.from_numpy(it).to(dev), torch.from_numpy(act).to(dev), gs)
    s, f = _bits(scores), _bits(fact)
    assert s[3] == s[19] == s[N - 1] and np.array_equal(f[3], f[19]) and np.array_equal(f[3], f[N - 1])
    _, _, s64 = SR.fused_f64(it, act)
    assert (np.abs(scores.cpu().numpy() - s64) <= SR.score_bounds(it, act)[2]).all()


def test_score_select_refusals(dev):
    for M, N, gs, dim in ((1, 2, 1, 4097), (2, 5, 2, 64), (1, 4097, 1, 1)):
        with pytest.raises(L.CoverError):
            ops.score_select(torch.ones(M, dim, device=dev), torch.ones(M, N, dim, device=dev), gs)
    torch.cuda.synchronize()


# ================================================================================================ group_argmax
def _check_group_argmax(dev, s, gs, what):
    result, best = ops.group_argmax(torch.from_numpy(s).to(dev), gs)
    want_r, want_b = SR.group_argmax(s, gs)
    assert np.array_equal(result.cpu().numpy(), want_r), (what, result.tolist(), want_r.tolist())
    assert _same_bits(best, want_b), (what, best.tolist(), want_b.tolist())
    return want_r


def test_group_argmax_matches_reference_bit_for_bit(dev):
    for N, gs in SR.GROUP_ARGMAX_SHAPES:
        _check_group_argmax(dev, SR.group_argmax_shape_scores(N, gs), gs, (N, gs))
    r = _check_group_argmax(dev, *SR.GROUP_ARGMAX_TIES["groups-5-and-261"](), "groups 5 and 261")
    assert r.tolist() == [10, 5, 0, 0]
    r = _check_group_argmax(dev, *SR.GROUP_ARGMAX_TIES["candidates-1-and-257"](), "candidates 1 and 257")
    assert r.tolist() == [1, 0, 1, 0]
    r = _check_group_argmax(dev, *SR.GROUP_ARGMAX_TIES["tie-after-fp32-rounding"](), "tie after rounding")
    assert r.tolist() == [3, 1, 0, 0]
    s = np.full(12, -np.inf, dtype=F32)
    assert _check_group_argmax(dev, s, 3, "all -inf").tolist() == [0, 0, 0, 0]
    for bad_n, bad_gs in ((12, 5), (4097, 1)):
        with pytest.raises(L.CoverError):
            ops.group_argmax(torch.zeros(bad_n, device=dev), bad_gs)


def test_group_argmax_nan_scores_pick_in_range(dev):
    """A NaN never wins at either level; where nothing wins the pick is index 0 and `best` carries the picked values' own bits."""
    want = {"all-nan": [0, 0, 0, 0], "all-nan-one-wide-group": [0, 0, 0, 0], "all-groups-nan-but-one": [2900 * 3 + 1, 2900, 1, 0],
            "every-mean-nan-numbers-in-group-0": [2, 0, 2, 0]}
    for name, make in SR.GROUP_ARGMAX_NAN.items():
        s, gs = make()
        r = _check_group_argmax(dev, s, gs, name)
        assert 0 <= r[0] < s.size and 0 <= r[1] < s.size // gs and 0 <= r[2] < gs
        if name in want:
            assert r.tolist() == want[name], name
    assert _check_group_argmax(dev, *SR.GROUP_ARGMAX_NAN["nan-in-best-group"](), "nan in best group")[1] != 1


# ================================================================================================ histories
@pytest.mark.parametrize("n_past,n_use", SR.HIST_STEPS)
def test_tokens_to_histories_is_the_table_lookup_exactly(dev, n_past, n_use):
    centers = SR.hist_centers()
    past = SR.hist_past(n_past)
    c_d = torch.from_numpy(centers).to(dev)
    p_d = None if past is None else torch.from_numpy(past).to(dev)
    for N in SR.HIST_N:
        tok = SR.hist_tokens(N, n_use)
        t_d = torch.from_numpy(tok).to(dev)
        assert t_d.stride(0) > 7 * n_use
        hist, pad = ops.tokens_to_histories(t_d, SR.TOK_VOCAB, c_d, p_d, pad_value=SR.PAD_VALUE, n_use=n_use)
        want_h, want_p = SR.histories_tokens(tok, SR.TOK_VOCAB, centers, past, n_use)
        assert _same_bits(hist, want_h), (N, n_past, n_use)
        assert np.array_equal(pad.cpu().numpy(), want_p)
        tight, _ = ops.tokens_to_histories(t_d[:, :7 * n_use].contiguous(), SR.TOK_VOCAB, c_d, p_d, pad_value=SR.PAD_VALUE, n_use=n_use)
        assert _same_bits(tight, want_h)                                             # ld == 7 n_use: the same rows


def test_tokens_to_histories_refusals(dev):
    c_d = torch.from_numpy(SR.hist_centers()).to(dev)
    tok = torch.from_numpy(SR.hist_tokens(4, 2)).to(dev)
    with pytest.raises(L.CoverError):                                                # n_past + n_use = 11
        ops.tokens_to_histories(tok, SR.TOK_VOCAB, c_d, torch.zeros(10, 7, device=dev), n_use=1)
    with pytest.raises(L.CoverError):                                                # ld < 7 n_use
        ops.tokens_to_histories(tok[:, :7].contiguous(), SR.TOK_VOCAB, c_d, None, n_use=2)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_past,n_use", SR.HIST_STEPS)
def test_actions_to_histories_within_the_derived_bound_of_float64(dev, n_past, n_use):
    past = SR.hist_past(n_past)
    p_d = None if past is None else torch.from_numpy(past).to(dev)
    worst, worst_bound = 0.0, 0.0
    for N in SR.HIST_N:
        x = SR.hist_actions(N, n_use)
        wide = torch.from_numpy(x).to(dev)
        for layout, a_d in (("contiguous [N, chunk, 7]", wide[:, :, :7].contiguous()), ("view of [N, chunk, 32]", wide[:, :, :7])):
            assert (a_d.stride(1) == 7) == layout.startswith("contiguous")
            for lo_hi in (SR.hist_lo_hi(), None):
                lh_d = None if lo_hi is None else torch.from_numpy(lo_hi).to(dev)
                hist, pad = ops.actions_to_histories(a_d, n_use, p_d, lh_d, pad_value=SR.PAD_VALUE)
                want_h, want_p, bound = SR.histories_actions(x, n_use, lo_hi, past)
                got = hist.cpu().numpy()
                err = np.abs(got.astype(np.float64) - want_h)
                assert (err <= bound).all(), (N, layout, lo_hi is None, err.max(), bound.max())
                exact = bound == 0                                                   # pad and past rows, the gripper, the pass-through
                assert _same_bits(got[exact], want_h[exact].astype(F32)), (N, layout, lo_hi is None)
                assert exact[..., 6].all() and exact[:, :10 - n_use].all()
                assert np.array_equal(pad.cpu().numpy(), want_p)
                if lo_hi is not None:
                    worst, worst_bound = max(worst, err.max()), max(worst_bound, bound.max())
    print(f"actions_to_histories ({n_past}, {n_use}): largest error {worst:.3e}, bound up to {worst_bound:.3e}")
