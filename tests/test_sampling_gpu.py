"""Device-side top-k / top-p sampling on the GPU: ops.token_sample against the float64 reference of tests/sampling_ref.py (every
decided row exact, at most 10 % of a case's rows undecided at the DELTA derived there), constructed rows, determinism, and the two
policies that use it (pi0-FAST generate_tokens / PI0FASTPolicy, OpenVLA.sample)."""
import types

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd._lib import CoverError
from tests import sampling_ref as R

pytestmark = pytest.mark.gpu

ONE_M = float(np.nextafter(np.float32(1), np.float32(0)))


def _sample(x, lo, hi, u, T=1.0, k=0, p=1.0):
    tok, lg, kept = ops.token_sample(x, lo, hi, u, temperature=T, top_k=k, top_p=p)
    torch.cuda.synchronize()
    return tok.cpu(), lg.cpu(), kept.cpu()


# ------------------------------------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("ci", range(len(R.WIDE_CASES)))
@pytest.mark.parametrize("ri", range(len(R.WIDE_RANGES)))
def test_wide_rows_match_reference(dev, ci, ri):
    T, k, p = R.WIDE_CASES[ci]
    lo, hi = R.WIDE_RANGES[ri]
    x, u = R.lm_like_rows(R.case_seed("wide", ci, ri), R.ROWS, R.WIDE_V, lo, hi)
    tok, lg, kept = _sample(x.to(dev), lo, hi, u.to(dev), T, k, p)
    assert ((tok >= lo) & (tok < hi)).all()
    assert torch.equal(lg, x[torch.arange(R.ROWS), tok])                       # the raw logit of the pick
    refs = R.reference_rows(x, lo, hi, u, T, k, p)
    R.check_against_reference(tok, kept, refs, lo, k, p, f"wide T={T} top_k={k} top_p={p} [{lo},{hi})")


@pytest.mark.parametrize("ci", range(len(R.NARROW_CASES)))
def test_narrow_rows_match_reference(dev, ci):
    T, k, p = R.NARROW_CASES[ci]
    lo, hi = R.NARROW_LO, R.NARROW_HI
    x, u = R.lm_like_rows(R.case_seed("narrow", ci), R.ROWS, R.NARROW_LD, lo, hi)
    tok, lg, kept = _sample(x.to(dev), lo, hi, u.to(dev), T, k, p)
    assert torch.equal(lg, x[torch.arange(R.ROWS), tok])
    refs = R.reference_rows(x, lo, hi, u, T, k, p)
    R.check_against_reference(tok, kept, refs, lo, k, p, f"narrow T={T} top_k={k} top_p={p}")


def test_flat_rows_take_the_row_passes_and_match_reference(dev):
    """i.i.d. Gaussian rows (no head): the top-p cut and a large k fall into the flat tail, far more than the candidate list
    holds. Such rows are rarely decided at the cut, so only what is exact by construction is demanded: the kept count under top-k
    alone, tokens inside the kept set, and the reference wherever it is decided."""
    g = torch.Generator().manual_seed(31)
    V = 70001
    x = 4 * torch.randn(16, V, generator=g)
    u = torch.rand(16, generator=g)
    for T, k, p in [(1.0, 20000, 1.0), (1.0, 0, 0.97), (1.0, 30000, 0.9)]:
        tok, _, kept = _sample(x.to(dev), 1, V, u.to(dev), T, k, p)
        refs = R.reference_rows(x, 1, V, u, T, k, p)
        for r, ref in enumerate(refs):
            if p >= 1.0:
                assert int(kept[r]) == ref["kept"] and ref["keep"][int(tok[r]) - 1]
            if ref["cut_decided"]:
                assert int(kept[r]) == ref["kept"], (T, k, p, r)
                if ref["pick_decided"]:
                    assert int(tok[r]) == 1 + ref["token"], (T, k, p, r)
            assert 1 <= int(tok[r]) < V and 1 <= int(kept[r]) <= V - 1


# ------------------------------------------------------------------------------------------------ 2. constructed rows
def test_constructed_rows(dev):
    V = 257152
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, V, generator=g)
    u = torch.tensor([0.3, 0.6, 0.0, ONE_M])
    # exact ties at the k-th value: all tied tokens stay
    tied = [11, 70000, 140003, 257151]
    x[0, 5] = 30.0
    x[0, tied] = 25.0
    tok, _, kept = _sample(x.to(dev), 0, V, u.to(dev), 1.0, 3, 1.0)
    assert int(kept[0]) == 5 and int(tok[0]) in [5] + tied
    assert kept[1:].tolist() == [3, 3, 3]
    # u = 0 / u = nextafter(1, 0): the first / last kept index
    top3 = torch.topk(x, 3, dim=-1).indices
    assert int(tok[2]) == int(top3[2].min()) and int(tok[3]) == int(top3[3].max())
    ua = torch.tensor([0.0, 0.0, ONE_M, ONE_M])
    tok, _, kept = _sample(x.to(dev), 0, V, ua.to(dev), 1.0, 3, 1.0)
    assert int(tok[0]) == 5 and int(tok[2]) == int(top3[2].max())
    tok, _, _ = _sample(x.to(dev), 0, V, torch.tensor([ONE_M] * 4).to(dev), 1.0, 3, 1.0)
    assert int(tok[0]) == 257151
    # top_k = 1 with a unique maximum = greedy for any u
    y = torch.randn(8, V, generator=g)
    uy = torch.rand(8, generator=g)
    greedy, glg = ops.token_select(y.to(dev), 0, V)
    tok, lg, kept = _sample(y.to(dev), 0, V, uy.to(dev), 0.8, 1, 1.0)
    assert torch.equal(tok, greedy.cpu()) and torch.equal(lg, glg.cpu()) and (kept == 1).all()
    # top_p so small that one token stays
    tok, _, kept = _sample(y.to(dev), 0, V, uy.to(dev), 1.0, 0, 1e-6)
    assert torch.equal(tok, greedy.cpu()) and (kept == 1).all()
    tok, _, kept = _sample(y.to(dev), 0, V, uy.to(dev), 1.0, 40, 1e-6)
    assert torch.equal(tok, greedy.cpu()) and (kept == 1).all()
    # every kept token in the scalar tail of an unaligned range: [3, 257150) has its float4 body end before the last columns
    z = torch.randn(3, V, generator=g)
    z[:, 257149] = 40.0
    z[:, 257148] = 39.0
    z[:, 257150] = 90.0                                       # outside the range
    z[:, 0] = 90.0
    for uu, want in ((0.0, 257148), (ONE_M, 257149)):
        tok, _, kept = _sample(z.to(dev), 3, 257150, torch.full((3,), uu).to(dev), 1.0, 2, 1.0)
        assert (tok == want).all() and (kept == 2).all()
    tok, _, kept = _sample(z.to(dev), 3, 257150, torch.full((3,), 0.5).to(dev), 1.0, 0, 0.5)
    assert (tok == 257149).all() and (kept == 1).all()
    # top_k >= width and top_p = 1 are the unfiltered result of the same kernel
    base = _sample(y.to(dev), 0, V, uy.to(dev), 1.1, 0, 1.0)
    for k, p in ((V, 1.0), (V + 5, 1.0), (0, 1.0), (V, 2.0)):
        other = _sample(y.to(dev), 0, V, uy.to(dev), 1.1, k, p)
        assert all(torch.equal(a, b) for a, b in zip(base, other))
    assert (base[2] == V).all()
    # equal weights at the top-p cut: the tied tokens enter by ascending index
    e = torch.full((2, 9000), -20.0)
    e[:, [100, 4000, 8000, 8999]] = 5.0
    tok, _, kept = _sample(e.to(dev), 0, 9000, torch.tensor([ONE_M, 0.0]).to(dev), 1.0, 0, 0.6)
    assert kept.tolist() == [3, 3] and tok.tolist() == [8000, 100]


# ------------------------------------------------------------------------------------------------ 3. the unfiltered narrow range
def test_unfiltered_narrow_range_is_token_select(dev):
    g = torch.Generator().manual_seed(2)                      # the inputs of test_kernels_gpu.py::test_token_select
    logits = torch.randn(9, 32064, generator=g)
    logits[4, 100] = logits[4, 31999] = 50.0
    u = torch.rand(9, generator=g)
    lg = logits.to(dev)
    for lo, hi, T in ((31744, 32000, 0.7), (31744, 32000, 1.0), (0, 4096, 1.3), (5, 4001, 0.9)):
        t0, l0 = ops.token_select(lg, lo, hi, uniform=u.to(dev), temperature=T)
        t1, l1, kept = ops.token_sample(lg, lo, hi, u.to(dev), temperature=T)
        assert torch.equal(t0, t1) and torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and (kept == hi - lo).all()
        t2, l2, _ = ops.token_sample(lg, lo, hi, u.to(dev), temperature=T, top_k=hi - lo, top_p=1.0)
        assert torch.equal(t0, t2) and torch.equal(l0.view(torch.int32), l2.view(torch.int32))


def test_pick_token_equals_the_direct_calls(dev):
    """ops.pick_token against the calls it stands for, bit for bit on tok, logit, kept and logprob: greedy, sampled unfiltered and
    sampled filtered, with and without out_logprob, into fresh tensors and into rows of [steps, rows] buffers."""
    rows, V, T, k, p = 5, 300, 0.8, 20, 0.9
    g = torch.Generator().manual_seed(31)
    lg = (torch.randn(rows, V, generator=g) * 3).to(dev)
    u = torch.rand(rows, generator=g).to(dev)
    bits = lambda t: t.view(torch.int32)
    for lo, hi in ((0, V), (44, V)):
        for mode in ("greedy", "unfiltered", "filtered"):
            # the direct calls
            if mode == "filtered":
                w_lp = torch.empty(rows, dtype=torch.float32, device=dev)
                w_tok, w_logit, w_kept = ops.token_sample(lg, lo, hi, u, temperature=T, top_k=k, top_p=p, out_logprob=w_lp)
                plain = ops.token_sample(lg, lo, hi, u, temperature=T, top_k=k, top_p=p)
                assert torch.equal(plain[0], w_tok) and torch.equal(plain[2], w_kept)
            else:
                kw = dict() if mode == "greedy" else dict(uniform=u, temperature=T)
                w_tok, w_logit = ops.token_select(lg, lo, hi, **kw)
                w_lp = ops.token_logprob(lg, lo, hi, w_tok, temperature=1.0 if mode == "greedy" else T)
                w_kept = None
            assert ((w_tok >= lo) & (w_tok < hi)).all() and torch.isfinite(w_lp).all()
            args = (None, 1.7, (3, 0.2)) if mode == "greedy" else (u, T, (k, p) if mode == "filtered" else None)   # greedy ignores both
            for with_lp in (False, True):
                for prealloc in (False, True):
                    out = {}
                    if prealloc:
                        bufs = dict(out_tok=torch.full((3, rows), -7, dtype=torch.int64, device=dev),
                                    out_logit=torch.full((3, rows), 9.0, dtype=torch.float32, device=dev),
                                    out_kept=torch.full((3, rows), -7, dtype=torch.int32, device=dev))
                        out = {n: b[1] for n, b in bufs.items()}
                    lp_buf = torch.full((3, rows), 9.0, dtype=torch.float32, device=dev)
                    if with_lp:
                        out["out_logprob"] = lp_buf[1]
                    tok, logit, kept = ops.pick_token(lg, lo, hi, *args, **out)
                    case = (lo, hi, mode, with_lp, prealloc)
                    assert torch.equal(tok, w_tok) and torch.equal(bits(logit), bits(w_logit)), case
                    assert (kept is None) == (mode != "filtered") and (kept is None or torch.equal(kept, w_kept)), case
                    if with_lp:
                        assert torch.equal(bits(lp_buf[1]), bits(w_lp)), case
                    assert (lp_buf[0] == 9.0).all() and (lp_buf[2] == 9.0).all() and (with_lp or (lp_buf[1] == 9.0).all()), case
                    if prealloc:
                        assert tok.data_ptr() == out["out_tok"].data_ptr() and logit.data_ptr() == out["out_logit"].data_ptr()
                        assert kept is None or kept.data_ptr() == out["out_kept"].data_ptr()
                        for n, b in bufs.items():
                            sentinel = 9.0 if n == "out_logit" else -7
                            assert (b[0] == sentinel).all() and (b[2] == sentinel).all(), (case, n)
                        assert mode == "filtered" or (bufs["out_kept"] == -7).all(), case   # only token_sample writes a kept count


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_deterministic_across_launch_shapes_and_graph_replay(dev):
    V = R.WIDE_V
    x, u = R.lm_like_rows(4242, 64, V, 0, V)
    xd, ud = x.to(dev), u.to(dev)
    for T, k, p in [(1.0, 0, 1.0), (0.7, 64, 0.95), (1.5, 0, 0.8), (1.0, 50, 1.0)]:
        a = _sample(xd, 0, V, ud, T, k, p)
        b = _sample(xd, 0, V, ud, T, k, p)
        assert all(torch.equal(i, j) for i, j in zip(a, b))
        g = torch.Generator().manual_seed(1)
        perm = torch.randperm(64, generator=g)[:23]
        c = _sample(xd[perm.to(dev)].contiguous(), 0, V, ud[perm.to(dev)].contiguous(), T, k, p)
        assert all(torch.equal(i[perm], j) for i, j in zip(a, c))
        # recorded into a graph and replayed (static inputs and outputs)
        tok = torch.empty(64, dtype=torch.int64, device=dev)
        lg = torch.empty(64, dtype=torch.float32, device=dev)
        kept = torch.empty(64, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with ops.Graph() as gr:
                ops.token_sample(xd, 0, V, ud, temperature=T, top_k=k, top_p=p, out_tok=tok, out_logit=lg, out_kept=kept)
            for _ in range(2):
                tok.fill_(-1)
                gr.launch()
                side.synchronize()
                assert torch.equal(tok.cpu(), a[0]) and torch.equal(lg.cpu(), a[1]) and torch.equal(kept.cpu(), a[2])
        torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ 5. argument errors
def test_argument_errors_raise(dev):
    x = torch.zeros(4, 64, device=dev)
    u = torch.zeros(4, device=dev)
    tok = torch.full((4,), -7, dtype=torch.int64, device=dev)
    for kw in (dict(temperature=0.0), dict(temperature=-2.0), dict(top_p=0.0), dict(top_p=-1.0), dict(top_k=-3)):
        with pytest.raises(CoverError):
            ops.token_sample(x, 0, 64, u, out_tok=tok, **kw)
    with pytest.raises(CoverError):
        ops.token_sample(x, 10, 10, u, out_tok=tok)
    with pytest.raises(CoverError):
        ops.token_sample(x, 0, 64, None, out_tok=tok)
    # the C entry point itself refuses them (COVER_EINVAL), whatever the Python wrapper checks
    import ctypes as C
    from cover_vla_amd import _lib as L
    kept = torch.empty(4, dtype=torch.int32, device=dev)

    def call(**over):
        a = L.TokenSampleArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi = x.data_ptr(), 64, 4, 0, 64
        a.uniform, a.temperature, a.top_k, a.top_p = u.data_ptr(), 1.0, 0, 1.0
        a.token_out, a.logit_out, a.kept_out = tok.data_ptr(), None, kept.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return L.lib().cover_token_sample(C.byref(a), torch.cuda.current_stream().cuda_stream)

    for over in (dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1), dict(hi=0), dict(uniform=None), dict(lo=0, hi=(1 << 20) + 1)):
        assert call(**over) == -1, over                      # COVER_EINVAL
    torch.cuda.synchronize()
    assert (tok == -7).all()                                  # nothing was launched
    assert call() == 0


# ------------------------------------------------------------------------------------------------ 6. pi0-FAST
TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def _fast_inputs(dev, B=6, L=9, seed=5):
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    toks = torch.zeros(B, L, dtype=torch.long)
    pad = torch.zeros(B, L, dtype=torch.long)
    row = torch.randint(2, 500, (L - 2,), generator=g)
    toks[:, :L - 2] = row                                     # identical frames and prompt in every row
    pad[:, :L - 2] = 1
    return [img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev)


def test_pi0fast_sampled_generation(dev):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, n_new = 6, 12
    args = _fast_inputs(dev, B)
    g = torch.Generator().manual_seed(9)
    u = torch.rand(B, n_new, generator=g)
    # uniforms=None: exactly the call without the new arguments
    greedy = model.generate_tokens(*args, n_new)
    assert torch.equal(model.generate_tokens(*args, n_new, uniforms=None, temperature=0.5, top_k=3, top_p=0.2), greedy)
    tr0 = {}
    model.generate_tokens(*args, n_new, trace=tr0)
    assert tr0["logits"][0].shape[0] == 1                     # greedy still generates identical rows once
    # teacher-forced: every step's pick is the reference applied to that step's traced device logits
    force = torch.randint(2, 500, (B, n_new), generator=g)
    n_dec = n_all = 0
    for T, k, p in [(1.0, 0, 1.0), (0.8, 50, 0.9), (1.0, 0, 0.7)]:
        tr = {}
        model.generate_tokens(*args, n_new, force_tokens=force, trace=tr, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p)
        assert len(tr["logits"]) == n_new == len(tr["picks"])
        for i in range(n_new):
            assert tr["logits"][i].shape[0] == B              # every row decoded on its own
            refs = R.reference_rows(tr["logits"][i].float(), 0, TINY["vocab"], u[:, i], T, k, p)
            picks, kept = tr["picks"][i].cpu(), tr["kept"][i].cpu()
            for r, ref in enumerate(refs):
                n_all += 1
                if ref["cut_decided"]:
                    assert int(kept[r]) == ref["kept"], (T, k, p, i, r)
                    if ref["pick_decided"]:
                        n_dec += 1
                        assert int(picks[r]) == ref["token"], (T, k, p, i, r)
    print(f"pi0-FAST teacher-forced picks: {n_dec} of {n_all} decided, all equal to the reference")
    assert n_dec >= 0.9 * n_all
    # identical frames and prompt, different uniforms: the rows diverge; identical uniforms: identical rows
    out = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=1.0, top_k=50, top_p=0.95, eos_token_id=-1).cpu()
    assert len({tuple(r.tolist()) for r in out}) > 1
    same = u[:1].repeat(B, 1)
    out_s = model.generate_tokens(*args, n_new, uniforms=same.to(dev), temperature=1.0, top_k=50, top_p=0.95, eos_token_id=-1).cpu()
    assert all(torch.equal(out_s[0], out_s[r]) for r in range(B))
    assert torch.equal(model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=1.0, top_k=50, top_p=0.95, eos_token_id=-1).cpu(), out)
    # top_k = 1 is greedy wherever each step's maximum is unique
    tr1 = {}
    out1 = model.generate_tokens(*args, n_new, uniforms=u.to(dev), top_k=1, trace=tr1).cpu()
    uniq = all(bool((lg == lg.amax(-1, keepdim=True)).sum(-1).eq(1).all()) for lg in tr1["logits"])
    assert uniq and torch.equal(out1, greedy.cpu())
    # pad after EOS under sampling
    eos = int(out[0, 2])
    out_e = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=1.0, top_k=50, top_p=0.95, eos_token_id=eos).cpu()
    hit = 0
    for r in range(B):
        pos = (out_e[r] == eos).nonzero()
        if pos.numel():
            first = int(pos[0])
            hit += 1
            assert (out_e[r, first + 1:] == 0).all() and (out_e[r, :first] != eos).all()
    assert hit >= 1 and int((out_e[0] == eos).nonzero()[0]) <= 2
    with pytest.raises(ValueError):
        model.generate_tokens(*args, n_new, uniforms=u[:, :3].to(dev))


def test_pi0fast_policy_sample_seed(dev):
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

    def run(cfg, n=4):
        pol = PI0FASTPolicy(cfg, model, tok, fast)
        return torch.stack([pol.select_action(batch).cpu() for _ in range(n)])

    greedy = run(PI0FASTConfig(**kw))
    a = run(PI0FASTConfig(temperature=1.0, top_k=50, top_p=0.95, sample_seed=7, **kw))
    b = run(PI0FASTConfig(temperature=1.0, top_k=50, top_p=0.95, sample_seed=7, **kw))
    c = run(PI0FASTConfig(temperature=1.0, top_k=50, top_p=0.95, sample_seed=8, **kw))
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(a, greedy) and not torch.equal(a, c)
    assert all(torch.equal(greedy[0, 0], greedy[0, r]) for r in range(4))     # greedy: identical rows, identical actions
    assert not all(torch.equal(a[0, 0], a[0, r]) for r in range(4))            # sampled: the candidates differ


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


def test_openvla_top_k_top_p(dev):
    from cover_vla_amd.openvla import OpenVLA
    c, sd, frame, toks, lens, u = _ov_case()
    kw = dict(device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    eager = OpenVLA(sd, c, **kw)
    eager.decode_graph = False
    model = OpenVLA(sd, c, **kw)
    assert model.decode_graph
    f, tk, ln, ud = frame.to(dev), toks.to(dev), lens.to(dev), u.to(dev)
    # defaults: bit-identical with and without the new arguments spelled out, eager and through the decode graph
    base_t, base_l = eager.sample(f, tk, ln, 2, ud, 0.9)
    for m in (eager, model, model):
        t, l = m.sample(f, tk, ln, 2, ud, 0.9)
        t2, l2 = m.sample(f, tk, ln, 2, ud, 0.9, top_k=0, top_p=1.0)
        assert torch.equal(t, base_t) and torch.equal(l, base_l) and torch.equal(t2, base_t) and torch.equal(l2, base_l)
    assert len(model._dec) == 1
    # filtered: every pick is the reference on the traced logits where decided
    lo, hi = eager.action_lo, eager.action_hi
    n_dec = n_all = 0
    for k, p in ((50, 0.9), (5, 1.0)):
        tr = {}
        t, sel = eager.sample(f, tk, ln, 2, ud, 0.9, trace=tr, top_k=k, top_p=p)
        t, sel = t.cpu(), sel.cpu()
        for i, lg in enumerate(tr["logits"]):
            refs = R.reference_rows(lg.float(), lo, hi, u[:, i], 0.9, k, p)
            for r, ref in enumerate(refs):
                n_all += 1
                if ref["pick_decided"] and ref["cut_decided"]:
                    n_dec += 1
                    assert int(t[r, i]) == lo + ref["token"], (k, p, i, r)
                    assert float(sel[r, i]) == float(lg[r, int(t[r, i])])
                assert ref["keep"][int(t[r, i]) - lo] or not ref["cut_decided"]
    print(f"OpenVLA filtered picks: {n_dec} of {n_all} decided, all equal to the reference")
    assert n_dec >= 0.9 * n_all
    # graph replay equals eager; changing top_k re-keys the graph and the results follow the new value
    seen = {}
    for k, p in ((50, 0.9), (50, 0.9), (2, 0.9), (50, 0.9), (2, 0.9), (0, 0.5)):
        a_t, a_l = model.sample(f, tk, ln, 2, ud, 0.9, top_k=k, top_p=p)
        b_t, b_l = eager.sample(f, tk, ln, 2, ud, 0.9, top_k=k, top_p=p)
        assert torch.equal(a_t, b_t) and torch.equal(a_l, b_l), (k, p)
        seen[(k, p)] = a_t.cpu()
    assert len(model._dec) == 4 and all(st["graph"].captured for st in model._dec.values())
    assert not torch.equal(seen[(50, 0.9)], seen[(2, 0.9)])
    # greedy ignores the filters
    g0, _ = model.sample(f, tk, ln, 1, None, 1.0)
    g1, _ = model.sample(f, tk, ln, 1, None, 1.0, top_k=5, top_p=0.5)
    assert torch.equal(g0, g1)
    # the sliced action head (logits of the 256 action rows only) takes the same filters: same picks as the full head
    sl = OpenVLA(sd, c, **kw)
    sl.slice_action_head = True
    s_t, s_l = sl.sample(f, tk, ln, 2, ud, 0.9, top_k=50, top_p=0.9)
    tr = {}
    e_t, _ = eager.sample(f, tk, ln, 2, ud, 0.9, top_k=50, top_p=0.9, trace=tr, force_tokens=s_t)
    assert ((s_t >= lo) & (s_t < hi)).all()
    s_t, e_t = s_t.cpu(), e_t.cpu()
    for i, lg in enumerate(tr["logits"]):
        for r, ref in enumerate(R.reference_rows(lg.float(), lo, hi, u[:, i], 0.9, 50, 0.9)):
            if ref["pick_decided"] and ref["cut_decided"]:
                assert int(s_t[r, i]) == int(e_t[r, i]) == lo + ref["token"], (i, r)
