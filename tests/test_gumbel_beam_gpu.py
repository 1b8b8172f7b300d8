"""Stochastic beam search on the GPU: cover_gumbel_topn against the float64 reference of tests/gumbel_ref.py (exact log-probabilities, padding,
order and inheritance of the parent's score; the perturbed scores within a tolerance taken from the fp32 restatement of the formula),
cover_beam_merge_gumbel against merge_gumbel bit for bit, the two chained over a toy tree as a distribution check, and
OpenVLA.stochastic_beam_search on synth.OPENVLA_SMALL: its own lists replayed, ancestry by teacher forcing, the per-prompt invariants, the
one-beam case against beam_search, reproducibility and the argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth  # noqa: F401
from tests import beam_ref as BR
from tests import gumbel_ref as GR
from tests import sampling_ref as SR

pytestmark = pytest.mark.gpu

NINF = np.float32(-np.inf)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, names, what):
    for name, g, w in zip(names, got, want):
        g, w = _bits(g), _bits(w)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


# ------------------------------------------------------------------------------------------------ row kernel
@pytest.mark.parametrize("name", [c[0] for c in GR.CASES])
def test_gumbel_topn_against_float64_reference(dev, name):
    """Exact: the log-probabilities are ops.token_logprob's bits, the padding, the first slot inherits g_parent's bits, the order descends
    on the launch's own values (equal values by ascending column), two equal maxima both carry g_parent, a second launch (the out_* form,
    strided outputs and uniforms) gives the same bits. Within 4 * e32: the perturbed scores (gumbel_ref.check_lists).
    Measured on MI355X (worst |g~ error| / its bound 4 * e32, undecided share of the live slots):
      w256-n1   0 / 2.675e-05, 0             w256-n5  5.076e-06 / 4.545e-05, 0       w256-n64  6.509e-06 / 2.595e-05, 0
      w4096-n64 5.650e-06 / 5.254e-05, 0.0069 (4 of 576)                             w5-n8     2.882e-06 / 1.153e-05, 0"""
    c = GR.case_data(name)
    lo, hi, n, T, rows = c["lo"], c["hi"], c["n"], c["T"], GR.ROWS
    lp64, gt64, e32 = GR.case_reference(name)
    lg, phi, G = (torch.from_numpy(c[k]).to(dev) for k in ("logits", "phi", "G"))
    u = torch.from_numpy(c["u"]).to(dev)
    tok, lp, g = ops.gumbel_topn(lg, lo, hi, n, phi, G, u, T)
    torch.cuda.synchronize()
    assert tok.shape == (rows, n) and tok.dtype == torch.int64 and lp.dtype == torch.float32 and g.dtype == torch.float32
    tok_h, lp_h, g_h = tok.cpu().numpy(), lp.cpu().numpy(), g.cpu().numpy()
    GR.check_lists(tok_h, g_h, lo, n, gt64, e32, name, SR.CAP)
    for j in range(n):                                                           # -1 (padding) scores -inf
        want = ops.token_logprob(lg, lo, hi, tok[:, j].contiguous(), T, 0, 1.0)
        assert np.array_equal(_bits(want), _bits(lp[:, j].contiguous())), (name, j)
    for r in range(rows):
        k = int((tok_h[r] >= 0).sum())
        if r in (0, 1, 3):                                                       # dead beams, and the row without a finite logit
            assert k == 0
            continue
        assert k == min(n, int((gt64[r] > -np.inf).sum())) and k >= 1
        assert g_h[r, 0].tobytes() == c["G"][r].tobytes(), (name, r)
        d = np.diff(g_h[r, :k])
        assert (d <= 0).all() and (np.diff(tok_h[r, :k])[d == 0] > 0).all(), (name, r)
        assert np.isfinite(lp_h[r, :k]).all()
    if n >= 2:
        assert tok_h[5, :2].tolist() == [lo + 1, hi - 1] and g_h[5, 1].tobytes() == c["G"][5].tobytes()
    # out_* form: row strides on every output and on the uniforms; same bits
    w = hi - lo
    u2 = torch.full((rows, w + 3), 0.5, device=dev)
    u2[:, :w] = u
    o_tok = torch.full((rows, n + 2), -9, dtype=torch.int64, device=dev)
    o_lp, o_g = torch.full((rows, n + 1), 9.0, device=dev), torch.full((rows, n + 5), 9.0, device=dev)
    got = ops.gumbel_topn(lg, lo, hi, n, phi, G, u2[:, :w], T, out_tok=o_tok[:, :n], out_logprob=o_lp[:, :n], out_perturbed=o_g[:, :n])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == o_tok.data_ptr() and got[2].data_ptr() == o_g.data_ptr()
    _same((o_tok[:, :n], o_lp[:, :n], o_g[:, :n]), (tok_h, lp_h, g_h), ("tok", "lp", "g"), name)
    assert (o_tok[:, n:] == -9).all() and (o_lp[:, n:] == 9.0).all() and (o_g[:, n:] == 9.0).all()


def test_gumbel_topn_argument_errors(dev):
    from cover_vla_amd import _lib as L
    lg, z = torch.zeros(2, 5000, device=dev), torch.zeros(2, device=dev)
    u = torch.full((2, 8), 0.5, device=dev)
    for kw in (dict(hi=4097 + 3, uniform=torch.zeros(2, 4097, device=dev)), dict(n=0), dict(n=65), dict(temperature=0.0), dict(uniform=u[:, :7])):
        a = dict(logits=lg, lo=3, hi=11, n=2, phi=z, g_parent=z, uniform=u, temperature=1.0)
        a.update(kw)
        with pytest.raises(L.CoverError):
            ops.gumbel_topn(**a)
    st = torch.cuda.current_stream().cuda_stream
    assert L.lib().cover_gumbel_topn(None, st) == -1
    assert L.lib().cover_gumbel_topn(C.byref(L.GumbelTopnArgs()), st) == -1
    a = L.GumbelTopnArgs()                                                       # everything set, the range one column too wide
    a.logits, a.ld, a.rows, a.lo, a.hi, a.temperature = lg.data_ptr(), 5000, 2, 0, 4097, 1.0
    wide = torch.zeros(2, 4097, device=dev)
    out = torch.zeros(2, 2, device=dev)
    a.phi, a.g_parent, a.uniform, a.ld_u, a.n = z.data_ptr(), z.data_ptr(), wide.data_ptr(), 4097, 2
    a.token_out, a.ld_tok = torch.zeros(2, 2, dtype=torch.int64, device=dev).data_ptr(), 2
    a.logprob_out, a.ld_lp, a.perturbed_out, a.ld_g = out.data_ptr(), 2, out.data_ptr(), 2
    assert L.lib().cover_gumbel_topn(C.byref(a), st) == -1


# ------------------------------------------------------------------------------------------------ merge
def _group(kind, B, rng):
    """One group's (cum [B], tok / lp / g [B, B]) in cover_gumbel_topn's list format."""
    cum = -rng.uniform(0, 20, size=B).astype(np.float32)
    pert = (cum + rng.gumbel(size=B)).astype(np.float32)
    tok, lp, g = GR.row_step(rng.normal(0, 3.0, size=(B, 256)).astype(np.float32), 100, 256, B, 1.0, cum, pert,
                             rng.random(size=(B, 156), dtype=np.float32))
    if kind == "ties":        # equal keys across beams (every row the same list) and inside a row (neighbours share a value), -0 and +0
        row = -0.25 * (np.arange(B) // 2).astype(np.float32)
        row[0] = -0.0
        g = np.repeat(row[None], B, 0).astype(np.float32)
        if B > 1:
            g[1, 0] = 0.0
    elif kind == "step0":
        cum[1:] = NINF
        cum[0] = 0.0
        tok, lp, g = np.repeat(tok[:1], B, 0), np.repeat(lp[:1], B, 0), np.repeat(g[:1], B, 0)
    elif kind == "few_live":  # one live beam whose list holds B // 2 children: fewer than B live
        cum[1:] = NINF
        tok[0, B // 2:], lp[0, B // 2:], g[0, B // 2:] = -1, NINF, NINF
    elif kind == "b_live":    # exactly B live candidates: every output live, nothing behind them (kappa = -inf)
        cum[1:] = NINF
    elif kind == "nan_cum":
        cum[0] = np.nan
    elif kind == "dead_key":  # a candidate with a token and a log-probability but no finite key is not live
        g[B - 1, 0] = NINF
        g[0, B - 1] = np.nan
    return cum, tok, lp, g


NAMES = ("parent", "token", "feed", "cum", "step_lp", "g", "kappa")


@pytest.mark.parametrize("B", [1, 2, 5, 64])
@pytest.mark.parametrize("kinds,pad", [(("random", "ties", "step0", "dead_key"), 0), (("few_live", "b_live", "nan_cum", "random"), 3)])
def test_merge_gumbel_matches_reference_bit_for_bit(dev, B, kinds, pad):
    rng = np.random.default_rng(100 * B + pad)
    cum, tok, lp, g = (np.concatenate(x) for x in zip(*[_group(k, B, rng) for k in kinds]))
    want = GR.merge_gumbel(cum, tok, lp, g, B, 77)
    rows = cum.shape[0]
    tok_d = torch.full((rows, B + pad), -5, dtype=torch.int64, device=dev)      # ld > B: the columns behind the list are not read
    lp_d, g_d = torch.full((rows, B + pad), 5.0, device=dev), torch.full((rows, B + 2 * pad), 50.0, device=dev)
    tok_d[:, :B], lp_d[:, :B], g_d[:, :B] = torch.from_numpy(tok).to(dev), torch.from_numpy(lp).to(dev), torch.from_numpy(g).to(dev)
    dts = (torch.int32, torch.int64, torch.int64, torch.float32, torch.float32, torch.float32)
    outs = [torch.full((rows,), -7, dtype=dt, device=dev) for dt in dts] + [torch.full((len(kinds),), -7.0, device=dev)]
    got = ops.beam_merge_gumbel(torch.from_numpy(cum).to(dev), tok_d[:, :B], lp_d[:, :B], g_d[:, :B], B, 77, *outs)
    torch.cuda.synchronize()
    _same(got, want, NAMES, (B, kinds))
    assert all(a.data_ptr() == o.data_ptr() for a, o in zip(got, outs))
    for i, k in enumerate(kinds):
        if k == "few_live":
            assert (want[0][i * B:(i + 1) * B] == -1).sum() == B - B // 2 and want[6][i] == NINF
        if k == "b_live":
            assert (want[0][i * B:(i + 1) * B] == 0).all() and want[6][i] == NINF
        if k == "ties" and B >= 2:
            assert np.isfinite(want[6][i]) and (np.diff(want[5][i * B:(i + 1) * B]) == 0).any(), "the constructed case must hold exact key ties"
    # allocating form, same bits
    _same(ops.beam_merge_gumbel(torch.from_numpy(cum).to(dev), tok_d[:, :B], lp_d[:, :B], g_d[:, :B], B, 77), want, NAMES, (B, kinds, "alloc"))


def test_merge_gumbel_argument_errors(dev):
    from cover_vla_amd import _lib as L
    cum, tok = torch.zeros(4, device=dev), torch.zeros(4, 2, dtype=torch.int64, device=dev)
    lp, g = torch.zeros(4, 2, device=dev), torch.zeros(4, 2, device=dev)
    with pytest.raises(L.CoverError):
        ops.beam_merge_gumbel(cum, tok, lp, g, 2, 0, out_cum=cum)
    st = torch.cuda.current_stream().cuda_stream
    assert L.lib().cover_beam_merge_gumbel(None, st) == -1
    assert L.lib().cover_beam_merge_gumbel(C.byref(L.BeamMergeGumbelArgs()), st) == -1
    a = L.BeamMergeGumbelArgs()                                                  # cover_beam_merge's arguments without a key list
    outs = [torch.zeros(4, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64, torch.float32, torch.float32, torch.float32)]
    a.cum, a.cand_tok, a.ld_tok, a.cand_lp, a.ld_lp, a.groups, a.B = cum.data_ptr(), tok.data_ptr(), 2, lp.data_ptr(), 2, 2, 2
    a.parent_out, a.token_out, a.feed_out, a.cum_out, a.step_lp_out, a.g_out = (o.data_ptr() for o in outs)
    assert L.lib().cover_beam_merge_gumbel(C.byref(a), st) == -1
    a.cand_g, a.ld_g, a.cum_out = g.data_ptr(), 2, cum.data_ptr()               # the aliasing rule through the C entry
    assert L.lib().cover_beam_merge_gumbel(C.byref(a), st) == -1
    a.cum_out = outs[3].data_ptr()
    assert L.lib().cover_beam_merge_gumbel(C.byref(a), st) == 0                  # kappa_out is optional


def test_abi_sizes(dev):
    from cover_vla_amd import _lib as L
    h = L.lib()
    assert h.cover_abi_version() == 1
    assert h.cover_sizeof(b"cover_gumbel_topn_args") == C.sizeof(L.GumbelTopnArgs) == 120
    assert h.cover_sizeof(b"cover_beam_merge_gumbel_args") == C.sizeof(L.BeamMergeGumbelArgs) == 128
    assert [h.cover_sizeof(n) for n in (b"cover_beam_merge_args", b"cover_kv_gather_slots_args", b"cover_beam_backtrack_args")] == [96, 96, 56]


# ------------------------------------------------------------------------------------------------ chained kernels, distribution
def test_chained_kernels_sample_without_replacement(dev):
    """gumbel_topn -> beam_merge_gumbel over 3 steps of a 4-token tree, 8192 independent groups of 3 beams, then beam_backtrack: the rank-0
    sequence is a draw from the tree's exact sequence distribution (4 sigma binomial per sequence) and a group's three sequences differ."""
    V, S, B, RUNS, lo, ld = 4, 3, 3, 8192, 2, 8
    tables, p = GR.toy_tree(V, S, 7)
    tabs = [torch.from_numpy(t).to(dev) for t in tables]
    rows = RUNS * B
    u = torch.rand(S, rows, V, generator=torch.Generator().manual_seed(21)).to(dev)
    cum = torch.full((S + 1, rows), float("-inf"), device=dev)
    pert = torch.full((S + 1, rows), float("-inf"), device=dev)
    cum[0, ::B], pert[0, ::B] = 0.0, 0.0
    parent = torch.empty(S, rows, dtype=torch.int32, device=dev)
    token, step_lp = torch.empty(S, rows, dtype=torch.int64, device=dev), torch.empty(S, rows, device=dev)
    lg = torch.full((rows, ld), 30.0, device=dev)                                # the columns outside [lo, lo + V) would win if they were read
    prefix = torch.zeros(rows, 0, dtype=torch.int64, device=dev)
    base = (torch.arange(rows, device=dev) // B) * B
    for i in range(S):
        lg[:, lo:lo + V] = tabs[i][tuple(prefix.t())] if i else tabs[0][None]
        ct, cl, cg = ops.gumbel_topn(lg, lo, lo + V, B, cum[i], pert[i], u[i], 1.0)
        ops.beam_merge_gumbel(cum[i], ct, cl, cg, B, 0, out_parent=parent[i], out_token=token[i], out_cum=cum[i + 1], out_step_lp=step_lp[i],
                              out_g=pert[i + 1])
        assert (parent[i] >= 0).all() if i else (parent[0] == 0).all()           # 4 >= 3 children at step 0, 12 afterwards: no dead output
        prefix = torch.cat([prefix[base + parent[i].long()], token[i][:, None] - lo], 1)
    tokens, lps = ops.beam_backtrack(parent, token, step_lp, B)
    assert torch.equal(tokens - lo, prefix)
    seqs = (tokens - lo).cpu().numpy().reshape(RUNS, B, S)
    GR.rank0_frequencies_ok(seqs[:, 0], p, "chained kernels")
    idx = np.sort((seqs * (V ** np.arange(S - 1, -1, -1))).sum(2), 1)
    assert (idx[:, 1:] != idx[:, :-1]).all()
    assert np.abs(np.exp(cum[S].cpu().numpy().astype(np.float64)).reshape(RUNS, B) - p.ravel()[(seqs * (V ** np.arange(S - 1, -1, -1))).sum(2)]).max() < 1e-5


# ------------------------------------------------------------------------------------------------ model
P, NB, T = 3, 4, 0.8


def _uniforms(m, n_beams, seed, dev):
    return torch.rand(m.n_gen, P * n_beams, m.action_hi - m.action_lo, generator=torch.Generator().manual_seed(seed)).to(dev)


@pytest.fixture(scope="module")
def run(dev):
    """One model (built with twice the candidates) and one traced stochastic beam search, shared and left unchanged. The checkpoint is the
    peaked one: under the flat head of an i.i.d. checkpoint the kept sequences of a prompt part at the first token and every beam keeps
    its rank (the arg-max child inherits its parent's score), so no step would re-parent a beam and the gathers would go untested."""
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_openvla_gpu import _case
    c, sd, frame, toks, lens, _ = _case(P=P, peaked=True)
    model = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=2 * P * NB, max_text=toks.shape[1])
    inputs = (frame.to(dev), toks.to(dev), lens.to(dev))
    u = _uniforms(model, NB, 33, dev)
    tr = {}
    out = model.stochastic_beam_search(*inputs, NB, u, T, trace=tr)
    torch.cuda.synchronize()
    names = ("tokens", "logprobs", "scores", "perturbed", "kappa")
    return dict(model=model, inputs=inputs, c=c, sd=sd, trace=tr, u=u, **{k: v.clone() for k, v in zip(names, out)})


def test_model_lists_and_merges_replayed(dev, run):
    """Every step's traced lists are ops.gumbel_topn of the traced logits and the traced phi / G of the step before, bit for bit, and pass the
    float64 slot check; merge_gumbel and beam_ref.backtrack on those lists reproduce every output, bit for bit.
    Measured on MI355X, steps 0..6 (worst |g~ error| / bound): 9.9e-07 / 8.7e-06, 4.9e-06 / 2.0e-05, 1.6e-06 / 1.6e-05, 1.5e-06 / 2.0e-05,
    6.3e-06 / 2.5e-05, 3.4e-05 / 1.7e-04, 3.2e-06 / 1.9e-05; no undecided slot among the 12 + 6 * 48 live ones."""
    m, tr, u = run["model"], run["trace"], run["u"]
    S, N, lo, hi = m.n_gen, P * NB, m.action_lo, m.action_hi
    assert len(tr["logits"]) == S and len(tr["beam"]) == S and run["tokens"].shape == (N, S) and run["kappa"].shape == (P,)
    cum, pert = np.full(N, NINF, np.float32), np.full(N, NINF, np.float32)
    cum[::NB], pert[::NB] = 0.0, 0.0
    parents, toks, lps, kappa = [], [], [], None
    for i in range(S):
        b = tr["beam"][i]
        tt, tl, tg = ops.gumbel_topn(tr["logits"][i], lo, hi, NB, torch.from_numpy(cum).to(dev), torch.from_numpy(pert).to(dev), u[i], T)
        _same((tt, tl, tg), (b["cand_tok"], b["cand_lp"], b["cand_g"]), ("cand_tok", "cand_lp", "cand_g"), i)
        l32 = tr["logits"][i][:, lo:hi].cpu().numpy()
        _, gt64 = GR.perturbed64(l32, T, cum, pert, u[i].cpu().numpy())
        g32 = GR.restate_f32(l32, T, cum, pert, u[i].cpu().numpy())
        live = gt64 > -np.inf
        e32 = float(np.abs(g32.astype(np.float64)[live] - gt64[live]).max())
        GR.check_lists(b["cand_tok"].cpu().numpy(), b["cand_g"].cpu().numpy(), lo, NB, gt64, e32, f"model step {i}", SR.CAP)
        want = GR.merge_gumbel(cum, b["cand_tok"].cpu().numpy(), b["cand_lp"].cpu().numpy(), b["cand_g"].cpu().numpy(), NB, lo)
        parent, token, _, cum, step_lp, pert, kappa = want
        _same((b["parent"], b["token"], b["cum"], b["g"], b["kappa"]), (parent, token, cum, pert, kappa), ("parent", "token", "cum", "g", "kappa"), i)
        parents.append(parent), toks.append(token), lps.append(step_lp)
    want_t, want_l = BR.backtrack(np.stack(parents), np.stack(toks), np.stack(lps), NB)
    assert np.array_equal(run["tokens"].cpu().numpy(), want_t) and np.array_equal(_bits(run["logprobs"]), _bits(want_l))
    _same((run["scores"], run["perturbed"], run["kappa"]), (cum, pert, kappa), ("scores", "perturbed", "kappa"), "final")


def test_model_ancestry_by_teacher_forcing(dev, run):
    """As test_beam_gpu.test_ancestry_by_teacher_forcing: the returned sequences forced through the existing sample() must score, at the
    search's temperature, what the search returned -- only if every gather brought the right parent's K/V. Allowance: twice e0, the
    difference the existing sample() itself shows when the rows of each group swap places, plus 1e-6.
    Measured on MI355X: e0 = 0.0, difference = 0.0 (exactly zero)."""
    m, tokens = run["model"], run["tokens"]
    S, N = m.n_gen, P * NB
    ident = torch.arange(N, device=dev) % NB
    assert any(not torch.equal(b["parent"].long(), ident) for b in run["trace"]["beam"][1:]), \
        "no step of this run re-parents a beam: a wrong gather would pass; pick another seed"

    def forced_lp(tk):
        tr = {}
        m.sample(*run["inputs"], NB, None, 1.0, trace=tr, force_tokens=tk)
        return torch.stack([ops.token_logprob(tr["logits"][i], m.action_lo, m.action_hi, tk[:, i].contiguous(), T, 0, 1.0) for i in range(S)], 1)

    lp1 = forced_lp(tokens)
    swap = (torch.arange(N, device=dev) // NB) * NB + (NB - 1 - torch.arange(N, device=dev) % NB)     # rows of each group reversed
    lp2 = forced_lp(tokens[swap].contiguous())
    e0 = (lp2 - lp1[swap]).abs().max().item()
    diff = (lp1 - run["logprobs"]).abs().max().item()
    print(f"ancestry: e0 = {e0!r}, difference = {diff!r}")
    assert torch.isfinite(lp1).all() and diff <= 2 * e0 + 1e-6, (diff, e0)


def test_model_per_prompt_invariants(dev, run):
    tokens, logprobs, scores, pert, kappa = (run[k].cpu().numpy() for k in ("tokens", "logprobs", "scores", "perturbed", "kappa"))
    m = run["model"]
    assert ((tokens >= m.action_lo) & (tokens < m.action_hi)).all() and np.isfinite(logprobs).all()
    for g in range(P):
        rows = slice(g * NB, (g + 1) * NB)
        assert len({tuple(r) for r in tokens[rows]}) == NB
        assert (np.diff(pert[rows]) <= 0).all() and (pert[rows] <= 0).all() and kappa[g] <= pert[rows].min()
    s = np.zeros(P * NB, np.float32)
    for i in range(logprobs.shape[1]):
        s = (s + logprobs[:, i]).astype(np.float32)
    assert np.array_equal(_bits(s), _bits(scores)) and np.isfinite(scores).all() and np.isfinite(kappa).all()


def test_model_one_beam_with_equal_noise_is_beam_search(dev, run):
    """uniforms all 0.5: every column gets the same noise, so the arg-max child is the most probable one and inherits G = 0 exactly."""
    m = run["model"]
    u = torch.full((m.n_gen, P, m.action_hi - m.action_lo), 0.5, device=dev)
    tokens, logprobs, scores, pert, kappa = m.stochastic_beam_search(*run["inputs"], 1, u, 1.0)
    want_t, want_l, want_s = m.beam_search(*run["inputs"], 1)
    assert torch.equal(tokens, want_t) and np.array_equal(_bits(logprobs), _bits(want_l)) and np.array_equal(_bits(scores), _bits(want_s))
    assert np.array_equal(_bits(pert), np.zeros(P, np.int32)) and (kappa < 0).all()


def test_model_same_uniforms_same_bits_other_uniforms_other_candidates(dev, run):
    m = run["model"]
    again = m.stochastic_beam_search(*run["inputs"], NB, run["u"], T)
    _same(again, [run[k] for k in ("tokens", "logprobs", "scores", "perturbed", "kappa")], ("tokens", "logprobs", "scores", "perturbed", "kappa"), "rerun")
    other = m.stochastic_beam_search(*run["inputs"], NB, _uniforms(m, NB, 34, dev), T)[0].cpu().numpy()
    mine = run["tokens"].cpu().numpy()
    assert any({tuple(r) for r in other[g * NB:(g + 1) * NB]} != {tuple(r) for r in mine[g * NB:(g + 1) * NB]} for g in range(P))


def test_model_argument_errors(dev, run):
    from cover_vla_amd.openvla import OpenVLA
    m, u = run["model"], run["u"]
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match="n_beams"):
            m.stochastic_beam_search(*run["inputs"], bad, u)
    with pytest.raises(ValueError, match="twice the candidates"):
        m.stochastic_beam_search(*run["inputs"], NB + 1, u)                    # 2 * 15 > 24
    for bad_u in (u[:-1], u[:, :-1], u[:, :, :-1], u.double(), u.cpu()):
        with pytest.raises(ValueError, match="uniforms"):
            m.stochastic_beam_search(*run["inputs"], NB, bad_u)
    for bad_t in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            m.stochastic_beam_search(*run["inputs"], NB, u, bad_t)
    own = OpenVLA(run["sd"], run["c"], device="cuda:0", max_prompts=4, max_candidates=8, max_text=run["inputs"][1].shape[1], own_kv="bf16")
    with pytest.raises(ValueError, match="own_kv"):
        own.stochastic_beam_search(*run["inputs"], 1, u)
