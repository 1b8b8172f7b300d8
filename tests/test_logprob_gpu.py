"""Per-token log-probabilities on the GPU: cover_token_sample_scored / cover_token_logprob against the float64 reference of
tests/logprob_ref.py (tolerance derived there, membership exact on every row whose cut is decided), bit-identity of the scored sampler
with the plain one, determinism and graph replay, argument errors, and the two policies' return_logprobs."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd import _lib as L
from cover_vla_amd._lib import CoverError
from tests import logprob_ref as LR
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def _bits(t):
    return t.cpu().view(torch.int32)


def _scored(xd, lo, hi, ud, T, k, p):
    lp = torch.full((xd.shape[0],), 7.0, dtype=torch.float32, device=xd.device)
    tok, lg, kept = ops.token_sample(xd, lo, hi, ud, temperature=T, top_k=k, top_p=p, out_logprob=lp)
    torch.cuda.synchronize()
    return tok, lg, kept, lp


# ------------------------------------------------------------------------------------------------ 1. the scored sampler
@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_scored_sampler_is_the_sampler_plus_logprob(dev, case):
    x, u, lo, hi, T, k, p, refs = LR.case_data(case)
    xd, ud = x.to(dev), u.to(dev)
    tok0, lg0, kept0 = ops.token_sample(xd, lo, hi, ud, temperature=T, top_k=k, top_p=p)
    tok, lg, kept, lp = _scored(xd, lo, hi, ud, T, k, p)
    assert torch.equal(tok, tok0) and torch.equal(_bits(lg), _bits(lg0)) and torch.equal(kept, kept0)
    R.check_against_reference(tok.cpu(), kept.cpu(), refs, lo, k, p, LR.case_id(case))
    LR.check_logprobs(lp.cpu().numpy(), tok.cpu().numpy(), refs, lo, hi, f"scored sampler {LR.case_id(case)}")
    assert torch.isfinite(lp).all()                                        # a pick is always in the kept set


# ------------------------------------------------------------------------------------------------ 2. scoring given tokens
@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_logprob_of_reference_picks_and_of_own_picks(dev, case):
    x, u, lo, hi, T, k, p, refs = LR.case_data(case)
    xd, ud = x.to(dev), u.to(dev)
    ref_tok = np.array([lo + r["token"] for r in refs], dtype=np.int64)
    kept = torch.empty(R.ROWS, dtype=torch.int32, device=dev)
    lp = ops.token_logprob(xd, lo, hi, torch.from_numpy(ref_tok).to(dev), temperature=T, top_k=k, top_p=p, out_kept=kept)
    LR.check_logprobs(lp.cpu().numpy(), ref_tok, refs, lo, hi, f"logprob of the reference's picks {LR.case_id(case)}")
    tok, _, kept_s, lp_s = _scored(xd, lo, hi, ud, T, k, p)
    lp_own = ops.token_logprob(xd, lo, hi, tok, temperature=T, top_k=k, top_p=p)
    assert torch.equal(_bits(lp_own), _bits(lp_s))                          # same code, same integers
    assert torch.equal(kept.cpu(), kept_s.cpu())


# ------------------------------------------------------------------------------------------------ 3. kept and non-kept tokens, ids outside
@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_teacher_tokens_and_ids_outside_the_range(dev, case):
    x, u, lo, hi, T, k, p, refs = LR.case_data(case)
    xd = x.to(dev)
    teach = LR.teacher_tokens(refs, lo, hi)
    teach[3], teach[10], teach[20], teach[30], teach[40] = hi, -1, lo - 1, hi + 5, -(1 << 40)      # a pad id, negative ids, hi
    teach[50], teach[51] = lo, hi - 1                                                             # the edges of the range
    lp = ops.token_logprob(xd, lo, hi, torch.from_numpy(teach).to(dev), temperature=T, top_k=k, top_p=p)
    torch.cuda.synchronize()
    got = lp.cpu().numpy()
    LR.check_logprobs(got, teach, refs, lo, hi, f"teacher tokens {LR.case_id(case)}")
    assert all(got[i] == NINF for i in (3, 10, 20, 30, 40))
    n_inf = int(np.isneginf(got).sum())
    filtered = (0 < k < hi - lo) or p < 1.0
    assert n_inf >= 50 if filtered else n_inf == 5


# ------------------------------------------------------------------------------------------------ 4. consistency with the kept count
@pytest.mark.parametrize("ci", range(len(R.NARROW_CASES)))
def test_every_column_of_the_256_bin_row(dev, ci):
    case = ("narrow", ci, 0)
    x, u, lo, hi, T, k, p, refs = LR.case_data(case)
    xd = x.to(dev)
    n = hi - lo
    kept = torch.empty(R.ROWS, dtype=torch.int32, device=dev)
    cols = torch.empty(n, R.ROWS, dtype=torch.float32, device=dev)
    for c in range(n):
        ops.token_logprob(xd, lo, hi, torch.full((R.ROWS,), lo + c, dtype=torch.int64, device=dev), temperature=T, top_k=k, top_p=p,
                          out=cols[c], out_kept=kept)
    torch.cuda.synchronize()
    lp = cols.t().cpu().numpy().astype(np.float64)                          # [rows, n]
    kept = kept.cpu().numpy()
    worst = 0.0
    for r, ref in enumerate(refs):
        fin = np.isfinite(lp[r])
        assert int(fin.sum()) == int(kept[r]), r
        assert (np.isneginf(lp[r]) | fin).all()
        lse = float(np.log(np.exp(lp[r][fin]).sum()))
        # each term is within tolerance() of the exact value and the exact values sum to 1: the log-sum-exp is off by at most the largest
        bound = float(LR.tolerance(ref["x"][fin], lp[r][fin]).max())
        worst = max(worst, abs(lse) / bound)
        assert abs(lse) <= bound, (r, lse, bound)
        if ref["cut_decided"]:
            assert np.array_equal(fin, ref["keep"]), r
    print(f"{LR.case_id(case)}: largest |logsumexp| / bound over 64 rows {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 5. determinism
def test_deterministic_across_row_positions_launches_and_graph_replay(dev):
    V = R.WIDE_V
    x, u = R.lm_like_rows(4242, 64, V, 0, V)
    x[17], x[63] = x[0], x[0]
    u[17], u[63] = u[0], u[0]
    xd, ud = x.to(dev), u.to(dev)
    u2 = torch.rand(64, generator=torch.Generator().manual_seed(3))
    for T, k, p in [(1.0, 0, 1.0), (0.7, 64, 0.95), (1.5, 0, 0.8), (1.0, 50, 1.0)]:
        a = _scored(xd, 0, V, ud, T, k, p)
        b = _scored(xd, 0, V, ud, T, k, p)
        assert all(torch.equal(_bits(i), _bits(j)) if i.dtype == torch.float32 else torch.equal(i, j) for i, j in zip(a, b))
        lp = a[3].cpu()
        assert _bits(lp)[0] == _bits(lp)[17] == _bits(lp)[63] and a[0][0] == a[0][17] == a[0][63]
        teach = torch.from_numpy(np.arange(64, dtype=np.int64) * 4001 % V)
        teach[17], teach[63] = teach[0], teach[0]
        s1 = ops.token_logprob(xd, 0, V, teach.to(dev), temperature=T, top_k=k, top_p=p)
        s2 = ops.token_logprob(xd, 0, V, teach.to(dev), temperature=T, top_k=k, top_p=p)
        assert torch.equal(_bits(s1), _bits(s2)) and _bits(s1)[0] == _bits(s1)[17] == _bits(s1)[63]
        # recorded into a graph and replayed twice with other uniforms in the static buffer; compare with eager on the same uniforms
        want2 = _scored(xd, 0, V, u2.to(dev), T, k, p)
        us = ud.clone()
        tok = torch.empty(64, dtype=torch.int64, device=dev)
        lg = torch.empty(64, dtype=torch.float32, device=dev)
        kept = torch.empty(64, dtype=torch.int32, device=dev)
        lpo = torch.empty(64, dtype=torch.float32, device=dev)
        lpt = torch.empty(64, dtype=torch.float32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with ops.Graph() as gr:
                ops.token_sample(xd, 0, V, us, temperature=T, top_k=k, top_p=p, out_tok=tok, out_logit=lg, out_kept=kept, out_logprob=lpo)
                ops.token_logprob(xd, 0, V, tok, temperature=T, top_k=k, top_p=p, out=lpt)
            for src, want in ((ud, a), (u2.to(dev), want2), (ud, a)):
                us.copy_(src)
                tok.fill_(-1)
                lpo.fill_(3.0)
                gr.launch()
                side.synchronize()
                assert torch.equal(tok, want[0]) and torch.equal(_bits(lg), _bits(want[1])) and torch.equal(kept, want[2])
                assert torch.equal(_bits(lpo), _bits(want[3])) and torch.equal(_bits(lpt), _bits(want[3]))
        torch.cuda.current_stream().wait_stream(side)


def test_unfiltered_narrow_range_scores_the_token_select_pick(dev):
    """Both filters off and a range of at most 4096 columns: the pick is cover_token_select's, bit for bit, with or without the score."""
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(9, 32064, generator=g)
    u = torch.rand(9, generator=g)
    lg = logits.to(dev)
    for lo, hi, T in ((31744, 32000, 0.7), (0, 4096, 1.3), (5, 4001, 0.9)):
        t0, l0 = ops.token_select(lg, lo, hi, uniform=u.to(dev), temperature=T)
        t1, l1, kept, lp = _scored(lg, lo, hi, u.to(dev), T, 0, 1.0)
        assert torch.equal(t0, t1) and torch.equal(_bits(l0), _bits(l1)) and (kept == hi - lo).all()
        refs = LR.reference_logprob_rows(logits, lo, hi, u, T, 0, 1.0)
        LR.check_logprobs(lp.cpu().numpy(), t1.cpu().numpy(), refs, lo, hi, f"unfiltered [{lo}, {hi}) T={T}")


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors_raise_and_launch_nothing(dev):
    x = torch.zeros(4, 64, device=dev)
    u = torch.zeros(4, device=dev)
    tok = torch.full((4,), -7, dtype=torch.int64, device=dev)
    lp = torch.full((4,), 5.0, dtype=torch.float32, device=dev)
    given = torch.zeros(4, dtype=torch.int64, device=dev)
    for kw in (dict(temperature=0.0), dict(temperature=-2.0), dict(top_p=0.0), dict(top_p=-1.0), dict(top_k=-3)):
        with pytest.raises(CoverError):
            ops.token_sample(x, 0, 64, u, out_tok=tok, out_logprob=lp, **kw)
        with pytest.raises(CoverError):
            ops.token_logprob(x, 0, 64, given, out=lp, **kw)
    with pytest.raises(CoverError):
        ops.token_sample(x, 10, 10, u, out_tok=tok, out_logprob=lp)
    with pytest.raises(CoverError):
        ops.token_logprob(x, 10, 10, given, out=lp)
    stream = torch.cuda.current_stream().cuda_stream

    def scored(**over):
        a = L.TokenSampleScoredArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi = x.data_ptr(), 64, 4, 0, 64
        a.uniform, a.temperature, a.top_k, a.top_p = u.data_ptr(), 1.0, 0, 1.0
        a.token_out, a.logit_out, a.kept_out, a.logprob_out = tok.data_ptr(), None, None, lp.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return L.lib().cover_token_sample_scored(C.byref(a), stream)

    def logprob(**over):
        a = L.TokenLogprobArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi = x.data_ptr(), 64, 4, 0, 64
        a.temperature, a.top_k, a.top_p = 1.0, 0, 1.0
        a.token, a.logprob_out, a.kept_out = given.data_ptr(), lp.data_ptr(), None
        for k, v in over.items():
            setattr(a, k, v)
        return L.lib().cover_token_logprob(C.byref(a), stream)

    bad = (dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1), dict(hi=0), dict(logprob_out=None), dict(lo=0, hi=(1 << 20) + 1))
    for over in bad + (dict(uniform=None),):
        assert scored(**over) == -1, over                    # COVER_EINVAL
    for over in bad + (dict(token=None),):
        assert logprob(**over) == -1, over
    torch.cuda.synchronize()
    assert (tok == -7).all() and (lp == 5.0).all()            # nothing was launched
    assert scored() == 0 and logprob() == 0
    torch.cuda.synchronize()
    assert np.abs(lp.cpu().numpy().astype(np.float64) + np.log(64.0)).max() <= float(LR.tolerance(0.0, np.log(64.0)))   # 64 equal logits


# ------------------------------------------------------------------------------------------------ 7. OpenVLA
def _ov_case(seed=13, P=3, Lt=9, n_samples=2, n_gen=7):
    c = dict(synth.OPENVLA_SMALL)
    sd = synth.openvla_state(c, seed=seed, std=0.08)
    g = torch.Generator().manual_seed(seed)
    frame = torch.randint(0, 256, (1, c["image"], c["image"], 3), generator=g, dtype=torch.uint8)
    lens = torch.tensor([Lt, Lt - 3, Lt - 1][:P], dtype=torch.int32)
    toks = torch.zeros(P, Lt, dtype=torch.long)
    for p in range(P):
        toks[p, :lens[p]] = torch.randint(2, c["tok_vocab"] - c["n_bins"], (int(lens[p]),), generator=g)
    u = torch.rand(P * n_samples, n_gen, generator=g)
    return c, sd, frame, toks, lens, u


def _check_steps(lps, tokens, logits_per_step, lo, hi, u, T, k, p, what, total=None):
    """lps / tokens [N, steps] from the device; logits_per_step: the traced fp32 logits [N, >= hi] of each step."""
    lps, tokens = lps.cpu().numpy(), tokens.cpu().numpy()
    n_cnt = n_all = 0
    for i, lg in enumerate(logits_per_step):
        uu = u[:, i] if u is not None else torch.zeros(lg.shape[0])
        refs = LR.reference_logprob_rows(lg.float(), lo, hi, uu, T, k, p)
        LR.check_logprobs(lps[:, i], tokens[:, i], refs, lo, hi, f"{what} step {i}", cap=1.0)   # a step is a handful of rows: capped in total below
        n_all += len(refs)
        n_cnt += sum(r["cut_decided"] for r in refs)
    assert np.isfinite(lps).all()
    if total is None:
        assert n_cnt >= (1 - R.CAP) * n_all, (what, n_cnt, n_all)
    else:                                                     # the caller caps what several calls leave out together
        total[0] += n_cnt
        total[1] += n_all


def test_openvla_return_logprobs(dev):
    from cover_vla_amd.openvla import OpenVLA
    c, sd, frame, toks, lens, u = _ov_case()
    kw = dict(device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    eager = OpenVLA(sd, c, **kw)
    eager.decode_graph = False
    model = OpenVLA(sd, c, **kw)
    assert model.decode_graph
    f, tk, ln, ud = frame.to(dev), toks.to(dev), lens.to(dev), u.to(dev)
    lo, hi = eager.action_lo, eager.action_hi
    settings = [("greedy", None, 1.0, 0, 1.0, 0, c["tok_vocab"]), ("unfiltered", ud, 0.9, 0, 1.0, lo, hi),
                ("filtered", ud, 0.9, 50, 0.9, lo, hi), ("top-k", ud, 1.2, 5, 1.0, lo, hi)]
    for name, uni, T, k, p, rlo, rhi in settings:
        n_s = 1 if uni is None else 2
        base_t, base_s = eager.sample(f, tk, ln, n_s, uni, T, top_k=k, top_p=p)
        n_keys = len(model._dec)
        outs = [eager.sample(f, tk, ln, n_s, uni, T, top_k=k, top_p=p, return_logprobs=True)]
        outs += [model.sample(f, tk, ln, n_s, uni, T, top_k=k, top_p=p, return_logprobs=True) for _ in range(3)]   # capture, replay, replay
        assert len(model._dec) == n_keys + 1                               # the flag is part of the decode-graph key
        for t, s, lp in outs:
            assert torch.equal(t, base_t) and torch.equal(_bits(s), _bits(base_s)), name
            assert lp.dtype == torch.float32 and tuple(lp.shape) == tuple(t.shape)
            assert torch.equal(_bits(lp), _bits(outs[0][2])), name
        t2, s2 = model.sample(f, tk, ln, n_s, uni, T, top_k=k, top_p=p)     # without the flag: the two-tensor return, its own graph
        assert torch.equal(t2, base_t) and torch.equal(_bits(s2), _bits(base_s))
        tr = {}
        t3, _, lp3 = eager.sample(f, tk, ln, n_s, uni, T, top_k=k, top_p=p, trace=tr, return_logprobs=True)
        assert torch.equal(t3, base_t) and torch.equal(_bits(lp3), _bits(outs[0][2]))
        _check_steps(lp3, t3, tr["logits"], rlo, rhi, None if uni is None else u, T, k, p, f"OpenVLA {name}")
    # force_tokens: still this path's own picks that are scored
    force = torch.randint(lo, hi, (6, 7), generator=torch.Generator().manual_seed(4)).to(dev)
    tr = {}
    t4, _, lp4 = eager.sample(f, tk, ln, 2, ud, 0.9, top_k=50, top_p=0.9, trace=tr, force_tokens=force, return_logprobs=True)
    _check_steps(lp4, t4, tr["logits"], lo, hi, u, 0.9, 50, 0.9, "OpenVLA teacher-forced")
    # the sliced action head: same picks and selected logits with and without the flag, log-probabilities over the 256 bins
    sl = OpenVLA(sd, c, **kw)
    sl.slice_action_head = True
    for k, p in ((50, 0.9), (0, 1.0)):
        s_t, s_l = sl.sample(f, tk, ln, 2, ud, 0.9, top_k=k, top_p=p)
        a_t, a_l, a_lp = sl.sample(f, tk, ln, 2, ud, 0.9, top_k=k, top_p=p, return_logprobs=True)
        b_t, b_l, b_lp = sl.sample(f, tk, ln, 2, ud, 0.9, top_k=k, top_p=p, return_logprobs=True)
        assert torch.equal(a_t, s_t) and torch.equal(_bits(a_l), _bits(s_l)) and torch.equal(b_t, s_t) and torch.equal(_bits(b_lp), _bits(a_lp))
        # the sliced head's logits are not traced, but its static buffer still holds the last step's: that step is checked against the
        # reference over the 256 columns; the earlier steps (overwritten) are checked for being log-probabilities at all
        N = a_t.shape[0]
        last = sl.logits_actions[:N].cpu()
        refs = LR.reference_logprob_rows(last, 0, c["n_bins"], u[:, -1], 0.9, k, p)
        LR.check_logprobs(a_lp[:, -1].cpu().numpy(), (a_t[:, -1] - lo).cpu().numpy(), refs, 0, c["n_bins"], f"OpenVLA sliced head k={k} p={p}")
        assert torch.isfinite(a_lp).all() and (a_lp <= 0).all()


# ------------------------------------------------------------------------------------------------ 8. pi0-FAST
TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def _fast_inputs(dev, B=6, L=9, seed=5, distinct=False):
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    toks = torch.zeros(B, L, dtype=torch.long)
    pad = torch.zeros(B, L, dtype=torch.long)
    row = torch.randint(2, 500, (L - 2,), generator=g)
    toks[:, :L - 2] = row
    if distinct:                                              # two distinct prompts, interleaved
        toks[1::2, 0] = 7
    pad[:, :L - 2] = 1
    return [img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev)


def test_pi0fast_return_logprobs(dev):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, n_new, V = 6, 12, TINY["vocab"]
    args = _fast_inputs(dev, B)
    u = torch.rand(B, n_new, generator=torch.Generator().manual_seed(9))
    # sampled: tokens unchanged by the flag, log-probabilities against the traced logits
    counted = [0, 0]
    for T, k, p in [(1.0, 0, 1.0), (0.8, 50, 0.9), (1.0, 0, 0.7)]:
        kw = dict(uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, eos_token_id=-1)
        plain = model.generate_tokens(*args, n_new, **kw)
        tr = {}
        out, lps = model.generate_tokens(*args, n_new, trace=tr, return_logprobs=True, **kw)
        assert torch.equal(out, plain) and lps.dtype == torch.float32 and tuple(lps.shape) == (B, n_new)
        assert len(tr["logits"]) == n_new
        _check_steps(lps, out, tr["logits"], 0, V, u, T, k, p, f"pi0-FAST sampled T={T} k={k} p={p}", total=counted)
    print(f"pi0-FAST sampled: {counted[0]} of {counted[1]} rows counted")
    assert counted[0] >= (1 - R.CAP) * counted[1]             # over the three settings, as tests/test_sampling_gpu.py caps its picks
    # 0.0 after a row's EOS; the steps before it are scored
    kw = dict(uniforms=u.to(dev), temperature=1.0, top_k=50, top_p=0.95)
    free = model.generate_tokens(*args, n_new, eos_token_id=-1, **kw).cpu()
    eos = int(free[0, 2])
    out_e, lp_e = model.generate_tokens(*args, n_new, eos_token_id=eos, return_logprobs=True, **kw)
    assert torch.equal(out_e, model.generate_tokens(*args, n_new, eos_token_id=eos, **kw))
    out_e, lp_e = out_e.cpu(), lp_e.cpu()
    hit = 0
    for r in range(B):
        pos = (out_e[r] == eos).nonzero()
        first = int(pos[0]) if pos.numel() else n_new - 1
        hit += bool(pos.numel())
        assert (lp_e[r, first + 1:] == 0.0).all() and (lp_e[r, :first + 1] <= 0.0).all() and torch.isfinite(lp_e[r]).all()
        assert float(lp_e[r, :first + 1].sum()) < 0.0
    assert hit >= 1
    from cover_vla_amd.host import sequence_logprob
    assert torch.equal(sequence_logprob(lp_e, out_e, pad_token_id=0), lp_e.sum(dim=1))
    # greedy: temperature 1, unfiltered, over the vocabulary; the de-duplicated call equals the row-by-row call
    args2 = _fast_inputs(dev, B, distinct=True)
    greedy = model.generate_tokens(*args2, n_new, eos_token_id=-1)
    tr = {}
    g_out, g_lp = model.generate_tokens(*args2, n_new, eos_token_id=-1, trace=tr, return_logprobs=True)
    assert torch.equal(g_out, greedy) and tr["logits"][0].shape[0] == 2         # two distinct rows were generated
    assert torch.equal(_bits(g_lp[0]), _bits(g_lp[2])) and torch.equal(_bits(g_lp[1]), _bits(g_lp[5])) and not torch.equal(g_lp[0], g_lp[1])
    # row by row: the two distinct rows as a batch of their own (nothing to de-duplicate, every row decoded) give what was broadcast
    two = [[a[:2] for a in args2[0]], [m[:2] for m in args2[1]], args2[2][:2], args2[3][:2]]
    tr2 = {}
    o2, l2 = model.generate_tokens(*two, n_new, eos_token_id=-1, trace=tr2, return_logprobs=True)
    assert tr2["logits"][0].shape[0] == 2
    for r in range(B):
        assert torch.equal(o2[r % 2], g_out[r]) and torch.equal(_bits(l2[r % 2]), _bits(g_lp[r]))
    _check_steps(g_lp[:2], g_out[:2], tr["logits"], 0, V, None, 1.0, 0, 1.0, "pi0-FAST greedy de-duplicated")
    # early stop: every row finished -> the skipped steps carry 0.0 and pad
    model.eos_check_every = 2
    eos_g = int(greedy[0, 1])
    same = _fast_inputs(dev, B)
    o_s, l_s = model.generate_tokens(*same, n_new, eos_token_id=eos_g, return_logprobs=True)
    assert torch.equal(o_s, model.generate_tokens(*same, n_new, eos_token_id=eos_g))
    first = int((o_s[0] == eos_g).nonzero()[0])
    assert first <= 1 and (o_s[:, first + 1:] == 0).all() and (l_s[:, first + 1:] == 0.0).all() and (l_s[:, :first + 1] < 0).all()


def test_pi0fast_policy_keeps_sequence_logprobs(dev):
    import types
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
    for seed in (None, 7):
        off = PI0FASTPolicy(PI0FASTConfig(temperature=1.0, top_k=50, top_p=0.95, sample_seed=seed, **kw), model, tok, fast)
        on = PI0FASTPolicy(PI0FASTConfig(temperature=1.0, top_k=50, top_p=0.95, sample_seed=seed, return_logprobs=True, **kw), model, tok, fast)
        assert on.last_sequence_logprobs is None
        a0, a1 = off.select_action(batch), on.select_action(batch)
        assert torch.equal(a0, a1) and off.last_sequence_logprobs is None
        s = on.last_sequence_logprobs
        assert s.dtype == torch.float32 and tuple(s.shape) == (4,) and torch.isfinite(s).all() and (s < 0).all()
        if seed is None:
            assert all(torch.equal(s[0], s[r]) for r in range(4))            # greedy: identical rows, identical sequence log-probability
