"""Self-checks of tests/select_ref.py, without a GPU: the references agree with the ones they extend, the conditions under which
tests/test_select_gpu.py compares exactly hold for every case of the tables, and the bounds reject perturbed stand-ins of the kernels."""
import numpy as np
import pytest

from tests import member_scores_ref as MR
from tests import select_ref as SR

F32 = np.float32


# ------------------------------------------------------------------------------------------------ references against their elders
def test_group_argmax_equals_member_scores_ref_on_nan_free_inputs():
    rng = np.random.default_rng(1)
    for k in range(200):
        gs = int(rng.integers(1, 9))
        G = int(rng.integers(1, 40))
        s = rng.normal(size=G * gs).astype(F32)
        if k % 4 == 0:                                    # ties, signed zeros and -inf
            s[rng.integers(0, s.size, size=3)] = s[0]
            s[rng.integers(0, s.size)] = -0.0
        if k % 7 == 0:
            s[rng.integers(0, s.size)] = -np.inf
        r0, b0 = MR.group_argmax(s, gs)
        r1, b1 = SR.group_argmax(s, gs)
        assert np.array_equal(r0, r1) and np.array_equal(SR.bits(b0), SR.bits(b1)), (k, s, gs)
    s = np.full(12, -np.inf, dtype=F32)                   # every group -inf: group 0, candidate 0
    assert SR.group_argmax(s, 3)[0].tolist() == [0, 0, 0, 0] == MR.group_argmax(s, 3)[0].tolist()


def test_greedy_equals_argmax_on_nan_free_rows():
    rng = np.random.default_rng(2)
    for k in range(100):
        n = int(rng.integers(1, 400))
        row = rng.normal(size=n + 8).astype(F32)
        if k % 3 == 0:
            row[rng.integers(0, row.size, size=4)] = row.max()
        if k % 5 == 0:
            row[:] = -np.inf
        lo = int(rng.integers(0, 8))
        tok, lg = SR.greedy(row, lo, lo + n)
        assert tok == lo + int(np.argmax(row[lo:lo + n])) and SR.bits(lg) == SR.bits(row[tok])


def test_nan_rule_of_the_references():
    nan = np.nan
    assert SR.greedy(np.array([9, nan, 1, 3, 3, nan], dtype=F32), 1, 6)[0] == 3
    tok, lg = SR.greedy(np.array([9, nan, nan, 9], dtype=F32), 1, 3)
    assert tok == 1 and np.isnan(lg)
    for name, make in SR.GROUP_ARGMAX_NAN.items():
        s, gs = make()
        result, best = SR.group_argmax(s, gs)
        assert 0 <= result[0] < s.size and result[0] == result[1] * gs + result[2] and 0 <= result[2] < gs, name
        assert SR.bits(best[0]) == SR.bits(s[result[0]]), name
    assert SR.group_argmax(*SR.GROUP_ARGMAX_NAN["all-nan"]())[0].tolist() == [0, 0, 0, 0]
    assert SR.group_argmax(*SR.GROUP_ARGMAX_NAN["all-groups-nan-but-one"]())[0].tolist() == [2900 * 3 + 1, 2900, 1, 0]
    assert SR.group_argmax(*SR.GROUP_ARGMAX_NAN["every-mean-nan-numbers-in-group-0"]())[0].tolist() == [2, 0, 2, 0]
    r, _ = SR.group_argmax(*SR.GROUP_ARGMAX_NAN["nan-in-best-group"]())
    assert r[1] != 1
    s, gs = SR.GROUP_ARGMAX_TIES["tie-after-fp32-rounding"]()
    assert SR.group_argmax(s, gs)[0].tolist() == [3, 1, 0, 0]            # the chain ties the two groups: the first wins
    assert s.astype(np.float64).reshape(-1, gs).sum(axis=1).argmax() == 2  # ... where the exact sums would not


def test_greedy_layouts_take_the_kernel_they_are_named_for():
    for name, (lo, width, ld_mod, base_off, kernel) in SR.GREEDY_LAYOUTS.items():
        buf, off, ld, lo2, hi = SR.greedy_matrix(name, SR.GREEDY_ROWS)
        assert (lo2, hi - lo2, ld % 4, off) == (lo, width, ld_mod, base_off)
        assert SR.is_wide(lo, width, ld, off) == (kernel == "wide"), name
        m = buf[off:off + len(SR.GREEDY_ROWS) * ld].reshape(-1, ld)
        assert np.isposinf(m[:, :lo]).all() and np.isposinf(m[:, hi:]).all()
        picks = {r: SR.greedy(m[i], lo, hi)[0] for i, r in enumerate(SR.GREEDY_ROWS)}
        assert picks["max-at-lo"] == lo and picks["max-at-hi-1"] == hi - 1 and picks["all-neg-inf"] == lo and picks["all-nan"] == lo
        assert picks["max-in-tail"] >= hi - 3 and picks["signed-zero-tie"] == lo + width // 2
        assert picks["tie-x3-first-wins"] == lo + min(4 * 700 + 1, width - 2)
    # 20483 = 4 * 4096 + 4 * 1024 + 3 from lo = 4: float4 slots 0 .. 4095 go through the four-in-flight loop, 4096 .. 5119 through the
    # single-load loop, and three floats are left; at 8192 (2048 slots) no thread has c + 3072 < n4
    assert SR.W3 // 4 == 4096 + 1024 and SR.W3 % 4 == 3 and SR.WIDE_MIN // 4 == 2048 < 3 * 1024 + 1


# ------------------------------------------------------------------------------------------------ sampling: the conditions
@pytest.mark.parametrize("width", SR.WIDTHS)
def test_every_sampling_cell_has_sixteen_decided_uniforms(width):
    for cell in [c for c in SR.CELLS if c[0] == width]:
        n, T, dist = cell
        c = SR.sampling_cell(cell)
        assert c["drawn"].size == SR.OVERSAMPLE * SR.N_DRAWN and c["kept"].size == SR.N_DRAWN, (cell, c["kept"].size, c["B"])
        assert 0 < c["B"] < 3 * n * SR.U + 1e-6, (cell, c["B"])
        for u, want in zip(c["kept"], c["picks"]):
            if dist == "flat":                           # decided exactly: csum[c] = c + 1, tgt = fl(u n)
                assert want == SR.flat_pick(n, u)
                tok, _ = SR.emulate_sampler(c["row"], 0, n, u, T)
                assert tok == want
                first, last = SR.pick_bracket(c["F"], u, c["B"])
                assert first <= want <= last              # and the exact rule sits inside the general bracket
            else:
                assert SR.decided(c["F"], u, c["B"])
                assert SR.pick_bracket(c["F"], u, c["B"]) == (want, want) and want == SR.inverse_cdf(c["row"], 0, n, u, T)[0]
        if dist == "flat":
            assert np.allclose(c["F"], np.arange(1, n + 1) / n, rtol=0, atol=1e-12)
            ones = np.cumsum(np.ones(n, dtype=F32), dtype=F32)   # the exact rule's premise: running sums of ones are exact in fp32
            assert np.array_equal(ones, np.arange(1, n + 1, dtype=F32))
        # u = 0 is decided exactly in every cell, the other fixed uniforms wherever their bracket is one index
        first, last = SR.fixed_expectation(cell, SR.FIXED_U[0])
        assert first == last, cell
        if dist == "flat":
            assert first == 0
        for u in SR.FIXED_U:
            first, last = SR.fixed_expectation(cell, u)
            assert 0 <= first <= last <= n - 1
            tok, _ = SR.emulate_sampler(c["row"], 0, n, u, T)
            assert first <= tok <= last, (cell, u)


def test_extreme_temperature_picks_the_maximum():
    for cell in [c for c in SR.CELLS if c[1] == 0.05 and c[2] == "peaked"]:   # every other exponent is below -200: the weights are 0
        c = SR.sampling_cell(cell)
        top = int(np.argmax(c["row"]))
        below = c["kept"] < 1 - c["B"]
        assert below.all() and (c["picks"] == top).all(), cell


@pytest.mark.parametrize("cell", [(4096, 1.0, "normal"), (257, 0.7, "normal"), (1000, 20.0, "peaked")], ids=SR.cell_id)
def test_sampling_bound_holds_for_the_kernel_arithmetic_and_rejects_a_wrong_scan(cell):
    n, T, _ = cell
    c = SR.sampling_cell(cell)
    u = F32(0.37)
    _, q = SR.emulate_sampler(c["row"], 0, n, u, T)
    err = np.abs(q - c["F"]).max()
    assert err <= c["B"], (err, c["B"])
    # a pairwise scan has the smaller worst case (gamma(log2 n)): a sound bound on the sequential chain cannot reject it, and it gives
    # the same decided picks -- the order of the adds is invisible to this test wherever the weights are not all equal
    _, q = SR.emulate_sampler(c["row"], 0, n, u, T, scan="pairwise")
    assert np.abs(q - c["F"]).max() <= c["B"]
    assert all(SR.emulate_sampler(c["row"], 0, n, uu, T, scan="pairwise")[0] == want for uu, want in zip(c["kept"], c["picks"]))
    # a scan that is wrong -- the running sum without the element itself -- breaks the bound and moves decided picks
    _, q = SR.emulate_sampler(c["row"], 0, n, u, T, scan="exclusive")
    assert np.abs(q - c["F"]).max() > c["B"]
    moved = sum(SR.emulate_sampler(c["row"], 0, n, uu, T, scan="exclusive")[0] != want for uu, want in zip(c["kept"], c["picks"]))
    same = sum(SR.emulate_sampler(c["row"], 0, n, uu, T)[0] != want for uu, want in zip(c["kept"], c["picks"]))
    assert same == 0 and moved > 0


# ------------------------------------------------------------------------------------------------ fused scores: margins and teeth
@pytest.mark.parametrize("case", SR.SCORE_CASES + [SR.POSITIONS_CASE], ids=MR.case_id)
def test_score_case_margins_exceed_twice_the_bound(case):
    M, N, gs, dim = case
    it, act = SR.score_inputs(case)
    _, _, s64 = SR.fused_f64(it, act)
    eta_it, eta_act, bound = SR.score_bounds(it, act)
    assert np.isfinite(bound).all() and bound.max() < (2e-6 if dim <= 64 else 2e-5), (bound.max(), eta_it, eta_act.max())
    _, m_g, m_i = SR.decision_f64(s64, gs)
    assert m_g > 2 * bound.max() and m_i > 2 * bound.max(), (m_g, m_i, bound.max())
    if N > 4:
        assert s64.max() - s64.min() > 0.3                # spread, not crowded at 0
    assert np.array_equal(MR.fused_scores_f64(it, act), s64.astype(F32))     # the same reference, unrounded


@pytest.mark.parametrize("case", SR.SCORE_CASES, ids=MR.case_id)
def test_score_bound_holds_for_the_kernel_arithmetic_and_rejects_a_dropped_lane(case):
    it, act = SR.score_inputs(case)
    _, _, s64 = SR.fused_f64(it, act)
    _, _, bound = SR.score_bounds(it, act)
    err = np.abs(SR.emulate_score(it, act).astype(np.float64) - s64)
    assert (err <= bound).all(), (err.max(), bound.max())
    bad = np.abs(SR.emulate_score(it, act, drop_lane=5).astype(np.float64) - s64)
    assert (bad > bound).any(), (bad.max(), bound.max())


# ------------------------------------------------------------------------------------------------ histories
def test_history_references_and_their_edge_inputs():
    centers = SR.hist_centers()
    assert centers[100] == F32(0.5) and centers[101] < F32(0.5) and np.isnan(centers[102])
    for n_past, n_use in SR.HIST_STEPS:
        tok = SR.hist_tokens(26, n_use)
        assert tok.shape[1] > 7 * n_use and tok.min() == -1 and tok.max() == 2 ** 31 - 1
        past = SR.hist_past(n_past)
        hist, pad = SR.histories_tokens(tok, SR.TOK_VOCAB, centers, past, n_use)
        n_pad = 10 - n_past - n_use
        assert (hist[:, :n_pad] == F32(SR.PAD_VALUE)).all() and pad[:, :n_pad].all() and not pad[:, n_pad:].any()
        new = hist[0, n_pad + n_past]
        assert new[0] == centers[0] and new[1] == centers[-1] and new[2] == centers[0] and new[3] == centers[-1]
        assert new[4] == centers[-1] and new[5] == centers[0] and new[6] == 1.0           # -1, 2^31 - 1, and 0.5 -> 1
        assert hist[1, n_pad + n_past, 6] == 0.0         # the float below 0.5 -> 0
        assert hist[25, 9, 6] == 1.0                                                     # NaN -> 1
        assert set(np.unique(hist[:, n_pad + n_past:, 6])) <= {0.0, 1.0}
        x = SR.hist_actions(26, n_use)
        for lo_hi in (SR.hist_lo_hi(), None):
            h, p, b = SR.histories_actions(x, n_use, lo_hi, past)
            assert np.array_equal(p, pad) and np.isfinite(h).all() and (b[..., 6] == 0).all() and (b[:, :n_pad + n_past] == 0).all()
            assert h[0, n_pad + n_past, 6] == 1.0 and h[25, n_pad + n_past + n_use - 1, 6] == 0.0 and h[1, n_pad + n_past, 6] == 1.0
            if lo_hi is None:
                assert (b == 0).all()
            else:
                assert 0 < b[:, n_pad + n_past:, :6].max() < 1e-6
                assert h[0, n_pad + n_past, 0] == float(lo_hi[0]) and abs(h[0, n_pad + n_past, 1] - float(lo_hi[7])) < 1e-12
