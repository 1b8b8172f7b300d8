"""Beam search on the GPU: cover_beam_merge / cover_kv_gather_slots / cover_beam_backtrack against the references of tests/beam_ref.py,
bit for bit (none of them has a tolerance), and OpenVLA.beam_search on synth.OPENVLA_SMALL: one beam against the action-bin arg-max of
sample(), the merge rule replayed on the run's own traced lists, ancestry by teacher-forcing the returned sequences through the existing
sample(), distinctness and score sums, and the argument errors."""
import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth  # noqa: F401
from tests import beam_ref as BR

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, what):
    for name, g, w in zip(("parent", "token", "feed", "cum", "step_lp"), got, want):
        g, w = _bits(g), _bits(w)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


# ------------------------------------------------------------------------------------------------ merge
def _group(kind, B, rng):
    """One group's (cum [B], tok [B, B], lp [B, B]) in cover_token_topn's list format."""
    tok, lp = BR.topn_lists(rng.normal(0, 3.0, size=(B, 256)).astype(np.float32), 100, 256, B)
    cum = -rng.uniform(0, 20, size=B).astype(np.float32)
    if kind == "ties":   # equal cum and equal lists across beams, equal neighbours inside a row, sums that tie from different (cum, lp) pairs
        cum[:] = np.float32(-1.5)
        cum[B // 2:] = np.float32(-2.0)
        row = -0.25 * (np.arange(B) // 2).astype(np.float32)
        lp = np.stack([row - np.float32(1.0 if b < B // 2 else 0.5) for b in range(B)]).astype(np.float32)
    elif kind == "step0":
        cum[:] = NINF
        cum[0] = 0.0
        tok, lp = np.repeat(tok[:1], B, 0), np.repeat(lp[:1], B, 0)
    elif kind == "few_live":   # one live beam whose list holds B // 2 tokens: fewer than B live candidates
        cum[1:] = NINF
        tok[0, B // 2:], lp[0, B // 2:] = -1, NINF
    elif kind == "nan_cum":
        cum[0] = np.nan
    return cum, tok, lp


@pytest.mark.parametrize("B", [1, 2, 5, 64])
@pytest.mark.parametrize("kinds,pad", [(("random", "ties", "step0"), 0), (("few_live", "nan_cum", "random"), 3)])
def test_merge_matches_reference_bit_for_bit(dev, B, kinds, pad):
    rng = np.random.default_rng(100 * B + pad)
    cum, tok, lp = (np.concatenate(x) for x in zip(*[_group(k, B, rng) for k in kinds]))
    want = BR.merge(cum, tok, lp, B, 77)
    rows = cum.shape[0]
    tok_d = torch.full((rows, B + pad), -5, dtype=torch.int64, device=dev)      # ld > B: the columns behind the list are not read
    lp_d = torch.full((rows, B + pad), 5.0, dtype=torch.float32, device=dev)
    tok_d[:, :B], lp_d[:, :B] = torch.from_numpy(tok).to(dev), torch.from_numpy(lp).to(dev)
    outs = [torch.full((rows,), -7, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64, torch.float32, torch.float32)]
    got = ops.beam_merge(torch.from_numpy(cum).to(dev), tok_d[:, :B], lp_d[:, :B], B, 77, *outs)
    torch.cuda.synchronize()
    _same(got, want, (B, kinds))
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    if "few_live" in kinds:
        assert (want[0][:B] == -1).sum() == B - B // 2 and (want[2][:B] == 77).sum() == B - B // 2
    if "ties" in kinds and B >= 2:
        c = want[3][B:2 * B]
        assert (c[:-1] == c[1:]).any(), "the constructed case must hold exact score ties among its outputs"
    # allocating form, same bits
    _same(ops.beam_merge(torch.from_numpy(cum).to(dev), tok_d[:, :B], lp_d[:, :B], B, 77), want, (B, kinds, "alloc"))


def test_merge_argument_errors(dev):
    from cover_vla_amd import _lib as L
    cum, tok, lp = torch.zeros(4, device=dev), torch.zeros(4, 2, dtype=torch.int64, device=dev), torch.zeros(4, 2, device=dev)
    with pytest.raises(L.CoverError):
        ops.beam_merge(cum, tok, lp, 2, 0, out_cum=cum)
    a = L.BeamMergeArgs()
    st = torch.cuda.current_stream().cuda_stream
    assert L.lib().cover_beam_merge(None, st) == -1
    import ctypes as C
    assert L.lib().cover_beam_merge(C.byref(a), st) == -1                          # null pointers, B = 0
    assert L.lib().cover_beam_backtrack(C.byref(L.BeamBacktrackArgs()), st) == -1
    assert L.lib().cover_kv_gather_slots(C.byref(L.KvGatherSlotsArgs()), st) == -1


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("n_t", [0, 1, 5, 32])
def test_gather_on_a_hand_made_cache(dev, n_t):
    layers, Hkv, D, cap, n_slots, off = 2, 2, 16, 32, 8, 64
    slot = cap * Hkv * D
    n = n_slots * slot
    # every element of every layer's K and V^T holds a different 16-bit pattern; `off` elements in front of the region and behind it are guards
    tot = off + n + off
    host = [np.arange(i * tot, (i + 1) * tot).astype(np.uint16).view(np.int16) for i in range(2 * layers)]
    assert 2 * layers * tot <= 2 ** 16
    dev_t = [torch.from_numpy(h.copy()).to(dev) for h in host]
    k_l, vt_l = dev_t[:layers], dev_t[layers:]
    tab = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev)
    # parents permuted, two rows share source 0, one source -1, one source >= n_slots, one destination out of range
    src = [1, 0, 0, -1, 8, 2]
    dst = [4, 5, 6, 7, 3, 8]
    ops.kv_gather_slots(tab(k_l), tab(vt_l), torch.tensor(src, dtype=torch.int32, device=dev), torch.tensor(dst, dtype=torch.int32, device=dev), n_t,
                        k_offset=off, vt_offset=off, k_slot_stride=slot, vt_slot_stride=slot, n_slots=n_slots, cap=cap, Hkv=Hkv, D=D)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in dev_t]
    kb = [h[off:off + n].reshape(n_slots, cap, Hkv, D) for h in host[:layers]]
    vb = [h[off:off + n].reshape(n_slots, Hkv, D, cap) for h in host[layers:]]
    ka = [g[off:off + n].reshape(n_slots, cap, Hkv, D) for g in got[:layers]]
    va = [g[off:off + n].reshape(n_slots, Hkv, D, cap) for g in got[layers:]]
    copied = {4: 1, 5: 0, 6: 0}
    n8 = (n_t + 7) // 8 * 8
    for l in range(layers):
        for d, s in copied.items():
            assert np.array_equal(ka[l][d, :n_t], kb[l][s, :n_t]) and np.array_equal(va[l][d, :, :, :n_t], vb[l][s, :, :, :n_t]), (l, d)
            # K is copied exactly, V^T in whole 16-byte runs: nothing behind them moves
            assert np.array_equal(ka[l][d, n_t:], kb[l][d, n_t:]) and np.array_equal(va[l][d, :, :, n8:], vb[l][d, :, :, n8:]), (l, d)
        for s in range(n_slots):
            if s not in copied or n_t == 0:                     # sources, skipped rows' destinations and bystanders: bit-identical
                assert np.array_equal(ka[l][s], kb[l][s]) and np.array_equal(va[l][s], vb[l][s]), (l, s)
    for g, h in zip(got, host):
        assert np.array_equal(g[:off], h[:off]) and np.array_equal(g[off + n:], h[off + n:])
    want_k, want_v = BR.gather(kb, vb, src, dst, n_t, n_slots)
    for l in range(layers):
        assert np.array_equal(ka[l], want_k[l]) and np.array_equal(va[l][..., :n_t], want_v[l][..., :n_t])


# ------------------------------------------------------------------------------------------------ backtrack
def test_backtrack_matches_reference(dev):
    S, B, G = 7, 4, 3
    rng = np.random.default_rng(5)
    parent = rng.integers(0, B, size=(S, G * B)).astype(np.int32)
    token = rng.integers(0, 1000, size=(S, G * B)).astype(np.int64)
    lp = -rng.uniform(0, 9, size=(S, G * B)).astype(np.float32)
    for broken in (False, True):
        if broken:                                              # every chain of group 1 runs through beam 1 of step 3, whose parent is -1
            parent[4, B:2 * B] = 1
            parent[3, B + 1] = -1
        want_t, want_l = BR.backtrack(parent, token, lp, B)
        got_t, got_l = ops.beam_backtrack(torch.from_numpy(parent).to(dev), torch.from_numpy(token).to(dev), torch.from_numpy(lp).to(dev), B)
        assert np.array_equal(got_t.cpu().numpy(), want_t) and np.array_equal(_bits(got_l), _bits(want_l))
        assert (want_t[B:2 * B, :3] == -1).all() == broken and not (want_t[:B] == -1).any()


# ------------------------------------------------------------------------------------------------ model
P, NB = 3, 4


@pytest.fixture(scope="module")
def run(dev):
    """One model (built with twice the candidates) and one traced beam search, shared and left unchanged."""
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_openvla_gpu import _case
    c, sd, frame, toks, lens, _ = _case(P=P)
    model = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=2 * P * NB, max_text=toks.shape[1])
    inputs = (frame.to(dev), toks.to(dev), lens.to(dev))
    tr = {}
    tokens, logprobs, scores = model.beam_search(*inputs, NB, trace=tr)
    torch.cuda.synchronize()
    return dict(model=model, inputs=inputs, c=c, sd=sd, trace=tr, tokens=tokens.clone(), logprobs=logprobs.clone(), scores=scores.clone())


def test_one_beam_is_the_action_bin_argmax(dev, run):
    m = run["model"]
    tokens, logprobs, scores = m.beam_search(*run["inputs"], 1)
    want, _ = m.sample(*run["inputs"], 1, uniforms=torch.zeros(P, m.n_gen, device=dev), temperature=[0.0] * P, trace={})
    assert tokens.shape == (P, m.n_gen) and torch.equal(tokens, want)
    assert ((tokens >= m.action_lo) & (tokens < m.action_hi)).all() and torch.isfinite(logprobs).all() and (scores <= 0).all()


def test_merge_rule_replayed_on_the_runs_own_lists(dev, run):
    m, tr = run["model"], run["trace"]
    S, N = m.n_gen, P * NB
    assert len(tr["logits"]) == S and len(tr["beam"]) == S
    cum = np.full(N, NINF, np.float32)
    cum[::NB] = 0.0
    parents, toks, lps = [], [], []
    for i in range(S):
        b = tr["beam"][i]
        # the traced lists are token_topn's of the traced logits
        tt, tl, _ = ops.token_topn(tr["logits"][i], m.action_lo, m.action_hi, NB, 1.0, 0, 1.0)
        assert torch.equal(tt, b["cand_tok"]) and np.array_equal(_bits(tl), _bits(b["cand_lp"])), i
        parent, token, _, cum, step_lp = BR.merge(cum, b["cand_tok"].cpu().numpy(), b["cand_lp"].cpu().numpy(), NB, m.action_lo)
        _same((b["parent"], b["token"], token, b["cum"], step_lp), (parent, token, token, cum, step_lp), i)
        parents.append(parent), toks.append(token), lps.append(step_lp)
    want_t, want_l = BR.backtrack(np.stack(parents), np.stack(toks), np.stack(lps), NB)
    assert np.array_equal(run["tokens"].cpu().numpy(), want_t) and np.array_equal(_bits(run["logprobs"]), _bits(want_l))
    assert np.array_equal(_bits(run["scores"]), _bits(cum))


def test_ancestry_by_teacher_forcing(dev, run):
    """The returned log-probabilities are those of the returned sequences: forced through the existing sample(), whose rows keep their own
    K/V from the first token on, every step's log-probability of the forced token must be the one beam_search returned -- it is only if
    every gather brought the right parent's K/V. Allowance: twice e0, the difference the existing sample() itself shows when the rows of
    each group swap places (measured here, from code that predates beam_search), plus 1e-6.
    Measured on MI355X: e0 = 0.0, difference = 0.0 (exactly zero)."""
    m, tokens = run["model"], run["tokens"]
    S, N = m.n_gen, P * NB
    ident = torch.arange(N, device=dev) % NB
    assert any(not torch.equal(b["parent"].long(), ident) for b in run["trace"]["beam"][1:]), \
        "no step of this run re-parents a beam: a wrong gather would pass; pick another seed"

    def forced_lp(tk):
        tr = {}
        m.sample(*run["inputs"], NB, None, 1.0, trace=tr, force_tokens=tk)
        return torch.stack([ops.token_logprob(tr["logits"][i], m.action_lo, m.action_hi, tk[:, i].contiguous(), 1.0, 0, 1.0) for i in range(S)], 1)

    lp1 = forced_lp(tokens)
    swap = (torch.arange(N, device=dev) // NB) * NB + (NB - 1 - torch.arange(N, device=dev) % NB)     # rows of each group reversed
    lp2 = forced_lp(tokens[swap].contiguous())
    e0 = (lp2 - lp1[swap]).abs().max().item()
    diff = (lp1 - run["logprobs"]).abs().max().item()
    print(f"ancestry: e0 = {e0!r}, difference = {diff!r}")
    assert torch.isfinite(lp1).all() and diff <= 2 * e0 + 1e-6, (diff, e0)


def test_sequences_distinct_scores_descend_and_sum(dev, run):
    tokens, logprobs, scores = (run[k].cpu().numpy() for k in ("tokens", "logprobs", "scores"))
    for g in range(P):
        rows = slice(g * NB, (g + 1) * NB)
        assert len({tuple(r) for r in tokens[rows]}) == NB and (np.diff(scores[rows]) <= 0).all()
    s = np.zeros(P * NB, np.float32)
    for i in range(logprobs.shape[1]):
        s = (s + logprobs[:, i]).astype(np.float32)
    assert np.array_equal(_bits(s), _bits(scores)) and np.isfinite(scores).all()


def test_argument_errors(dev, run):
    from cover_vla_amd.openvla import OpenVLA
    m = run["model"]
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match="n_beams"):
            m.beam_search(*run["inputs"], bad)
    with pytest.raises(ValueError, match="twice the candidates"):
        m.beam_search(*run["inputs"], NB + 1)                          # 2 * 15 > 24
    own = OpenVLA(run["sd"], run["c"], device="cuda:0", max_prompts=4, max_candidates=8, max_text=run["inputs"][1].shape[1], own_kv="bf16")
    with pytest.raises(ValueError, match="own_kv"):
        own.beam_search(*run["inputs"], 1)
