"""Prior-weighted selection on the GPU: cover_prior_select against the fp32 reference of tests/prior_ref.py, bit for bit (the order of
every rounding is specified, so no tolerance is needed), the beta = 0 identity with cover_group_argmax, graph replay, argument errors
of the C entry, and the prior flowing from the two token policies into EfficientEnsembleMerged.score_histories."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd import _lib as L
from tests import prior_ref as PR

pytestmark = pytest.mark.gpu

KEYS = ("prior", "combined", "group_mean", "result", "best", "ranked")


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, got[k], want[k])


def _laid_out(x, layout, dev):
    """x [N, steps] on the host -> a device view of that shape over a candidate-major or a step-major buffer (never a copy afterwards)."""
    if x is None:
        return None
    t = torch.from_numpy(x)
    if layout == "step-major":
        return t.t().contiguous().to(dev).t()
    return t.contiguous().to(dev)


def _run_case(c, dev):
    scores, lps, tokens = PR.make_inputs(c)
    N, gs, steps, top_m = c["shape"]
    lp_d, tok_d = _laid_out(lps, c["layout"], dev), _laid_out(tokens, c["layout"], dev)
    if steps > 1 and N > 1:
        assert (lp_d.stride(1) == 1) == (c["layout"] == "candidate-major")
    return ops.prior_select(torch.from_numpy(scores).to(dev), lp_d, gs, c["beta"], tokens=tok_d, pad_token_id=PR.PAD_ID if c["with_tokens"] else None,
                            length_normalize=c["length_normalize"], top_m=top_m)


# ------------------------------------------------------------------------------------------------ 1. every case of the table
@pytest.mark.parametrize("variant", PR.VARIANTS)
@pytest.mark.parametrize("shape", PR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_reference_bit_for_bit(dev, shape, variant):
    cs = PR.cases(variants=(variant,), shapes=(shape,))
    assert len(cs) == 24
    for c in cs:
        got = _run_case(c, dev)
        want = PR.case_reference(c)
        _assert_same(got, want, PR.case_id(c))
        if shape[3] > 0:
            assert int(got["ranked"][0]) == int(got["result"][0])


def test_logprobs_of_one_dimension_are_a_summed_prior(dev):
    c = dict(shape=(40, 5, 7, 5), layout="candidate-major", with_tokens=False, length_normalize=False, beta=0.05, variant="uniform")
    scores, lps, _ = PR.make_inputs(c)
    summed = PR.case_reference(c)["prior"]
    got = ops.prior_select(torch.from_numpy(scores).to(dev), torch.from_numpy(summed).to(dev), 5, 0.05, top_m=5)
    _assert_same(got, PR.case_reference(c), "summed prior")
    col = torch.from_numpy(np.stack([summed, summed], axis=1)).to(dev)[:, 1]       # [N] with stride 2
    _assert_same(ops.prior_select(torch.from_numpy(scores).to(dev), col, 5, 0.05, top_m=5), PR.case_reference(c), "strided [N]")


# ------------------------------------------------------------------------------------------------ 2. beta = 0 is cover_group_argmax
@pytest.mark.parametrize("shape", PR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_beta_zero_is_group_argmax(dev, shape):
    N, gs, steps, top_m = shape
    for variant in PR.VARIANTS:
        c = dict(shape=shape, layout="candidate-major", with_tokens=False, length_normalize=False, beta=0.0, variant=variant)
        scores = torch.from_numpy(PR.make_inputs(c)[0]).to(dev)
        got = _run_case(c, dev)
        result, best = ops.group_argmax(scores, gs)
        assert np.array_equal(_bits(got["combined"]), _bits(scores))
        assert np.array_equal(_bits(got["result"]), _bits(result)) and np.array_equal(_bits(got["best"]), _bits(best)), variant


# ------------------------------------------------------------------------------------------------ 3. graph replay, 4. argument errors
class _Raw:
    """The C entry over preallocated, sentinel-filled buffers."""

    def __init__(self, dev, N, steps, gs, top_m):
        self.N, self.steps, self.gs, self.top_m = N, steps, gs, top_m
        self.scores = torch.zeros(N, device=dev)
        self.lps = torch.zeros(N, steps, device=dev)
        self.tokens = torch.ones(N, steps, dtype=torch.int64, device=dev)
        self.out = {"prior": torch.empty(N, device=dev), "combined": torch.empty(N, device=dev), "group_mean": torch.empty(N // gs, device=dev),
                    "result": torch.empty(4, dtype=torch.int32, device=dev), "best": torch.empty(2, device=dev),
                    "ranked": torch.empty(top_m, dtype=torch.int32, device=dev)}
        self.fill()

    def fill(self):
        for k, t in self.out.items():
            t.fill_(-7)

    def untouched(self):
        return all(bool((t == -7).all()) for t in self.out.values())

    def args(self, beta, length_normalize, **over):
        a = L.PriorSelectArgs()
        a.scores, a.logprobs, a.lp_n_stride, a.lp_t_stride = self.scores.data_ptr(), self.lps.data_ptr(), self.steps, 1
        a.tokens, a.tok_n_stride, a.tok_t_stride, a.pad_token_id = self.tokens.data_ptr(), self.steps, 1, PR.PAD_ID
        a.N, a.steps, a.group_size, a.top_m, a.beta, a.length_normalize = self.N, self.steps, self.gs, self.top_m, beta, int(length_normalize)
        for k in KEYS:
            setattr(a, k + "_out", self.out[k].data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, beta=0.05, length_normalize=True, **over):
        a = self.args(beta, length_normalize, **over)
        return L.lib().cover_prior_select(C.byref(a), torch.cuda.current_stream().cuda_stream)


def test_graph_replay_follows_the_input_buffers(dev):
    shape = (40, 5, 7, 5)
    N, gs, steps, top_m = shape
    raw = _Raw(dev, N, steps, gs, top_m)
    inputs = [PR.make_inputs(dict(shape=shape, variant=v, with_tokens=True)) for v in ("uniform", "quantised", "neginf")]
    wants = [PR.reference(s, lp, tok, PR.PAD_ID, gs, 0.05, True, top_m) for s, lp, tok in inputs]
    assert len({int(w["result"][0]) for w in wants}) > 1                   # the replays have different answers
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with ops.Graph() as gr:
            assert raw.call() == 0
        side.synchronize()
        assert raw.untouched()                                             # the capture itself executed nothing
        for (s, lp, tok), want in zip(inputs, wants):
            raw.scores.copy_(torch.from_numpy(s))
            raw.lps.copy_(torch.from_numpy(lp))
            raw.tokens.copy_(torch.from_numpy(tok))
            raw.fill()
            gr.launch()
            side.synchronize()
            _assert_same(raw.out, want, "replay")
    torch.cuda.current_stream().wait_stream(side)


def test_argument_errors_return_einval_and_launch_nothing(dev):
    raw = _Raw(dev, 48, 4, 6, 3)
    bad = (dict(N=0), dict(N=-48), dict(group_size=0), dict(group_size=5), dict(N=8192, group_size=1), dict(N=8192, group_size=8192),
           dict(steps=0), dict(steps=4097), dict(top_m=-1), dict(top_m=7), dict(group_size=1, top_m=2),
           dict(beta=-0.5), dict(beta=float("nan")), dict(beta=float("inf")),
           dict(scores=None), dict(logprobs=None), dict(prior_out=None), dict(combined_out=None), dict(result_out=None), dict(best_out=None),
           dict(ranked_out=None))
    for over in bad:
        kw = dict(over)
        beta = kw.pop("beta", 0.05)
        assert raw.call(beta=beta, **kw) == -1, over                       # COVER_EINVAL
    assert L.lib().cover_prior_select(None, torch.cuda.current_stream().cuda_stream) == -1
    wide = _Raw(dev, 256, 1, 128, 64)
    assert wide.call(top_m=65) == -1                                       # within the group, beyond 64
    torch.cuda.synchronize()
    assert raw.untouched() and wide.untouched()                            # nothing was launched
    # the optional pointers: no tokens, no group means, no ranking
    assert raw.call(tokens=None, group_mean_out=None, ranked_out=None, top_m=0) == 0
    torch.cuda.synchronize()
    assert bool((raw.out["group_mean"] == -7).all()) and bool((raw.out["ranked"] == -7).all())
    assert raw.out["prior"].tolist() == [0.0] * 48 and raw.out["result"].tolist() == [0, 0, 0, 0]
    assert raw.call() == 0
    torch.cuda.synchronize()
    assert raw.out["ranked"].tolist() == [0, 1, 2] and raw.out["group_mean"].tolist() == [0.0] * 8


# ------------------------------------------------------------------------------------------------ 5. model level
def _verifier(dev, N, seed=9):
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    ver = EfficientEnsembleMerged(synth.verifier_checkpoint(2, seed=seed), device="cuda:0")
    pf, tf, hists = synth.verifier_inputs(N, seed=seed)
    return ver, ver.image_text_embeddings(pf.to(dev), tf.to(dev)), hists


def _ref_of(r, lps, tokens, pad_id, gs, beta, length_normalize, top_m):
    return PR.reference(r["scores"].cpu().numpy(), lps.cpu().numpy(), None if tokens is None else tokens.cpu().numpy(), pad_id, gs, beta,
                        length_normalize, top_m)


def test_openvla_sample_logprobs_into_score_histories(dev):
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_topn_gpu import _ov_case
    c, sd, frame, toks, lens, u = _ov_case()
    P, S = toks.shape[0], 2
    policy = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    tokens, _, lps = policy.sample(frame.to(dev), toks.to(dev), lens.to(dev), S, u.to(dev), 0.9, top_k=50, top_p=0.9, return_logprobs=True)
    N = P * S
    assert tuple(lps.shape) == (N, policy.n_gen) and lps.dtype == torch.float32 and bool(torch.isfinite(lps).all())
    ver, its, _ = _verifier(dev, N)
    bins = np.linspace(-1, 1, c["n_bins"])
    centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=dev)
    past = torch.from_numpy((np.random.default_rng(0).normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)
    hb, pad = ops.tokens_to_histories(tokens, c["tok_vocab"], centers, past)
    # the default call: what ops.score_select gives, and nothing else
    base = ver.score_histories(its, hb, S, pad=pad)
    plain = ver.score_histories(its, hb, S, pad=pad, prior=None, top_m=0)
    scores, result, best, fit, fact = ops.score_select(base["its"], base["acts"], S)
    assert set(plain) == {"scores", "result", "best", "its", "acts", "fused_it", "fused_act"}
    for k, t in (("scores", scores), ("result", result), ("best", best), ("fused_it", fit), ("fused_act", fact)):
        assert np.array_equal(_bits(plain[k]), _bits(t)) and np.array_equal(_bits(base[k]), _bits(t)), k
    # with the prior
    for beta, ln in ((0.05, False), (1.0, True), (0.0, False)):
        r = ver.score_histories(its, hb, S, pad=pad, prior=lps, prior_beta=beta, length_normalize=ln, top_m=S)
        assert np.array_equal(_bits(r["scores"]), _bits(scores))
        _assert_same(r, _ref_of(r, lps, None, None, S, beta, ln, S), f"OpenVLA beta {beta}")
    # top_m without a prior ranks by the verifier score alone
    r = ver.score_histories(its, hb, S, pad=pad, top_m=S)
    assert "prior" not in r
    _assert_same(r, _ref_of(r, torch.zeros(N, 1), None, None, S, 0.0, False, S), "ranking only", keys=KEYS[1:])
    assert np.array_equal(_bits(r["result"]), _bits(result)) and np.array_equal(_bits(r["best"]), _bits(best))


TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def test_pi0fast_logprobs_into_score_histories(dev):
    from cover_vla_amd.host import sequence_logprob
    from cover_vla_amd.pi0fast import PI0FASTTokens
    from tests.test_topn_gpu import _fast_inputs
    model = PI0FASTTokens(synth.pi0_state(TINY, seed=11), TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, n_new, S = 6, 12, 3
    args = _fast_inputs(dev, B)
    u = torch.rand(B, n_new, generator=torch.Generator().manual_seed(9)).to(dev)
    kw = dict(uniforms=u, temperature=1.0, top_k=50, top_p=0.95)
    free = model.generate_tokens(*args, n_new, eos_token_id=-1, **kw).cpu()
    eos = int(free[0, 2])                                                      # row 0 finishes within three steps
    out, lps = model.generate_tokens(*args, n_new, eos_token_id=eos, pad_token_id=0, return_logprobs=True, **kw)
    n_pad = (out == 0).sum(dim=1).cpu()
    assert bool((out == eos).any()) and int(n_pad.max()) > 0                                        # some rows stop early
    ver, its, hists = _verifier(dev, B, seed=4)
    # per-step values with the emitted tokens: pads left out, length-normalised
    r = ver.score_histories(its, hists, S, prior=lps, prior_beta=0.05, prior_tokens=out, pad_token_id=0, length_normalize=True, top_m=S)
    _assert_same(r, _ref_of(r, lps, out, 0, S, 0.05, True, S), "pi0-FAST per step")
    # the summed prior: steps = 1
    summed = sequence_logprob(lps)
    r1 = ver.score_histories(its, hists, S, prior=summed, prior_beta=0.05, top_m=S)
    _assert_same(r1, _ref_of(r1, summed, None, None, S, 0.05, False, S), "pi0-FAST summed")
    assert np.array_equal(_bits(r1["prior"]), _bits(summed))
    # the device's chain against torch's sum: not the same order, so the chain bound steps * 2^-24 * sum |lp| (pads carry 0.0)
    r2 = ver.score_histories(its, hists, S, prior=lps, prior_beta=0.05)
    got, want = r2["prior"].cpu().numpy().astype(np.float64), summed.cpu().numpy().astype(np.float64)
    bound = n_new * PR.U * np.abs(lps.cpu().numpy().astype(np.float64)).sum(axis=1)
    print("pi0-FAST prior - host.sequence_logprob:", np.abs(got - want).max(), "bound", bound.min())
    assert (np.abs(got - want) <= bound).all()
    assert set(r2) >= {"prior", "combined", "group_mean", "ranked"} and r2["ranked"].numel() == 0
