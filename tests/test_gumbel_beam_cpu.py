"""Stochastic beam search, the part that needs no GPU: the reference search of tests/gumbel_ref.py is a sample without replacement (rank-0
frequencies against the exact sequence probabilities, inclusion frequencies against a flat Gumbel-top-k over the enumerated sequences,
distinctness), merge_gumbel's order, padding and kappa on hand-made ties, and the distance between the fp32 restatement of the formula and
float64 on the kernel test cases -- the number the device tolerance of tests/test_gumbel_beam_gpu.py is taken from."""
import numpy as np
import pytest

from tests import gumbel_ref as GR

NINF = np.float32(-np.inf)
V, S, B, RUNS = 4, 3, 3, 20000


@pytest.fixture(scope="module")
def toy_run():
    tables, p = GR.toy_tree(V, S, 7)
    rng = np.random.default_rng(11)
    u = rng.random(size=(S, RUNS * B, V), dtype=np.float32)
    step = lambda prefixes: np.broadcast_to(tables[prefixes.shape[1]][tuple(np.clip(prefixes, 0, None).T)], (RUNS * B, V))
    tokens, logprobs, scores, pert, kappa, _ = GR.search(step, RUNS, B, S, 0, V, u)
    return p, tokens.reshape(RUNS, B, S), logprobs.reshape(RUNS, B, S), scores.reshape(RUNS, B), pert.reshape(RUNS, B), kappa


def test_reference_search_rank0_is_a_draw_from_the_policy(toy_run):
    p, tokens = toy_run[0], toy_run[1]
    GR.rank0_frequencies_ok(tokens[:, 0], p, "reference search")


def test_reference_search_inclusion_matches_flat_gumbel_top_k(toy_run):
    p, tokens = toy_run[0], toy_run[1]
    idx = (tokens * (V ** np.arange(S - 1, -1, -1))).sum(2)                      # [RUNS, B]
    incl = np.bincount(idx.ravel(), minlength=V ** S) / RUNS
    rng = np.random.default_rng(12)
    flat = np.log(p.ravel())[None] + rng.gumbel(size=(RUNS, V ** S))
    want = np.bincount(np.argsort(-flat, axis=1)[:, :B].ravel(), minlength=V ** S) / RUNS
    sigma = np.sqrt(2 * np.maximum(want, 1.0 / RUNS) * (1 - np.minimum(want, 1 - 1.0 / RUNS)) / RUNS)     # two independent estimates
    dev = np.abs(incl - want)
    print(f"inclusion frequencies: worst deviation {dev.max():.4f}, worst in sigmas {(dev / sigma).max():.2f}")
    assert (dev <= 4 * sigma).all()


def test_reference_search_results_are_distinct_ordered_and_scored(toy_run):
    p, tokens, logprobs, scores, pert, kappa = toy_run
    idx = (tokens * (V ** np.arange(S - 1, -1, -1))).sum(2)
    assert (np.sort(idx, 1)[:, 1:] != np.sort(idx, 1)[:, :-1]).all()
    assert (np.diff(pert, axis=1) <= 0).all() and (pert <= 0).all() and (kappa <= pert.min(1)).all() and np.isfinite(kappa).all()
    s = np.zeros(scores.shape, np.float32)
    for i in range(S):
        s = (s + logprobs[:, :, i]).astype(np.float32)
    assert np.array_equal(s.view(np.int32), scores.view(np.int32))
    assert np.abs(np.exp(scores.astype(np.float64)) - p.ravel()[idx]).max() < 1e-6


def test_merge_gumbel_order_padding_and_kappa_on_ties():
    f = np.float32
    cum = np.array([-1.0, -2.0, -3.0], f)
    tok = np.array([[10, 11, 12], [20, 21, -1], [30, 31, 32]], np.int64)
    lp = np.array([[-0.5, -1.0, -1.5], [-0.25, -0.75, NINF], [-0.125, -1.0, -2.0]], f)
    # equal keys across beams (1.5 three times) and inside a row (beam 2: 0.5 twice); beam 1's third entry is padding
    g = np.array([[1.5, 0.5, -0.0], [1.5, 0.0, NINF], [1.5, 0.5, 0.5]], f)
    parent, token, feed, cum_o, step_lp, g_o, kappa = GR.merge_gumbel(cum, tok, lp, g, 3, 99)
    assert parent.tolist() == [0, 1, 2] and token.tolist() == [10, 20, 30] and feed.tolist() == [10, 20, 30]
    assert cum_o.tolist() == [-1.5, -2.25, -3.125] and step_lp.tolist() == [-0.5, -0.25, -0.125] and g_o.tolist() == [1.5, 1.5, 1.5]
    assert kappa.tolist() == [0.5]                                               # the fourth: (b 0, j 1) ahead of (b 2, j 1)
    # one live beam with two live children: one padded output, kappa -inf; then exactly B + 1 live: kappa is the last
    cum2 = np.array([-1.0, NINF, np.nan], f)
    g2 = g.copy()
    g2[0, 2] = NINF
    parent, token, feed, cum_o, step_lp, g_o, kappa = GR.merge_gumbel(cum2, tok, lp, g2, 3, 99)
    assert parent.tolist() == [0, 0, -1] and token.tolist() == [10, 11, -1] and feed.tolist() == [10, 11, 99]
    assert cum_o.tolist()[:2] == [-1.5, -2.0] and cum_o[2] == NINF and step_lp[2] == NINF and g_o[2] == NINF and kappa[0] == NINF
    parent, token, _, _, _, g_o, kappa = GR.merge_gumbel(np.array([-1.0, -2.0, NINF], f), tok, lp, g, 3, 99)
    assert parent.tolist() == [0, 1, 0] and token.tolist() == [10, 20, 11] and g_o.tolist() == [1.5, 1.5, 0.5]
    assert kappa.tolist() == [0.0] and np.signbit(kappa[0])                       # -0 == +0: (b 0, j 2) is ahead of (b 1, j 1); the stored float comes back
    # B = 1: a single candidate, nothing behind it
    out = GR.merge_gumbel(np.array([0.0], f), np.array([[7]]), np.array([[-0.5]], f), np.array([[-0.25]], f), 1, 0)
    assert out[0].tolist() == [0] and out[5].tolist() == [-0.25] and out[6][0] == NINF


def test_row_step_maximum_inherits_the_parent_and_dead_rows_pad():
    c = GR.case_data("w256-n5")
    tok, lp, g = GR.row_step(c["logits"], c["lo"], c["hi"], c["n"], c["T"], c["phi"], c["G"], c["u"])
    for r in range(GR.ROWS):
        if r in (0, 1, 3):                                                       # dead beams and the row without a finite logit
            assert (tok[r] == -1).all() and (lp[r] == NINF).all() and (g[r] == NINF).all()
        else:
            assert g[r, 0].tobytes() == c["G"][r].tobytes() and (np.diff(g[r]) <= 0).all() and (g[r] <= c["G"][r]).all()
    assert tok[5, :2].tolist() == [c["lo"] + 1, c["hi"] - 1] and g[5, 1].tobytes() == c["G"][5].tobytes()    # two equal maxima, by column
    assert (c["logits"][2, tok[2]] > -np.inf).all()


@pytest.mark.parametrize("name", [c[0] for c in GR.CASES])
def test_restate_f32_distance_to_float64(name):
    """e32, the worst |g~ error| of the formula in np.float32 arithmetic against float64 on a kernel test case's inputs: the device
    tolerance is MARGIN * e32 (gumbel_ref.check_lists). Printed; the bound here only says that fp32 evaluates the formula at all --
    an error of 1e-2 would mean the restatement (or the formula) is wrong, not rounded."""
    _, gt, e32 = GR.case_reference(name)
    print(f"{name}: e32 = {e32:.3e} over {int((gt > -np.inf).sum())} live columns")
    assert 0.0 < e32 < 1e-2
