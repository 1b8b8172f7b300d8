"""Gaussian proposal augmentation on the GPU: cover_augment_tokens / cover_augment_actions against the fp32 reference of
tests/augment_ref.py, bit for bit (every rounding is specified, so there is no tolerance), every output cell stored, graph replay,
argument errors of the C entries, and the two policies' thin methods end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, host, ops, synth
from cover_vla_amd import _lib as L
from tests import augment_ref as AR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("out", "mean", "sd", "votes")
SENTINEL_BITS = 0x7FC12345          # a NaN payload no result carries


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, got[k], want[k])


def _laid_out(c, inp, dev):
    """The case's input as the device sees it: tokens with a row stride beyond 7 h at every other shape, actions through the strides
    (chunk * 32, 32) of a [N, chunk, 32] buffer at the strided shape; the cells outside the view hold junk."""
    G, n, K, h = c["shape"]
    rng = np.random.default_rng(1)
    if c["form"] == "tokens":
        tok = inp["tokens"]
        ld = 7 * h + (3 if AR.SHAPES.index(c["shape"]) % 2 else 0)
        buf = rng.integers(AR.TOK_VOCAB - 256, AR.TOK_VOCAB, (tok.shape[0], ld)).astype(np.int64)
        buf[:, :7 * h] = tok
        view = torch.from_numpy(buf).to(dev)[:, :7 * h]
        assert view.stride(0) == ld
        return view
    x = inp["actions"]
    if c["shape"] == AR.STRIDED:
        chunk = h + 2
        buf = rng.uniform(-1, 1, (x.shape[0], chunk, 32)).astype(np.float32)
        buf[:, :h, :7] = x
        view = torch.from_numpy(buf).to(dev)[:, :h, :7]
        assert view.stride() == (chunk * 32, 32, 1)
        return view
    return torch.from_numpy(x).to(dev)


def _run_case(c, dev):
    inp = AR.make_inputs(c)
    src, z = _laid_out(c, inp, dev), torch.from_numpy(inp["normals"]).to(dev)
    kw = dict(sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"], stats=True)
    if c["form"] == "tokens":
        out, st = ops.augment_tokens(src, inp["n"], inp["K"], z, torch.from_numpy(inp["centers"]).to(dev), AR.TOK_VOCAB, steps=c["shape"][3], **kw)
    else:
        out, st = ops.augment_actions(src, inp["n"], inp["K"], z, **kw)
    return dict(out=out, mean=st.mean, sd=st.sd, votes=st.votes)


# ------------------------------------------------------------------------------------------------ 1. every case of the table
def _shape_params():
    return [(f, s) for f in ("tokens", "actions") for s in AR.SHAPES + (AR.FLOAT_ONLY if f == "actions" else [])]


@pytest.mark.parametrize("form,shape", _shape_params(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_matches_reference_bit_for_bit(dev, form, shape):
    cs = AR.cases(forms=(form,), shapes=(shape,))
    assert len(cs) >= 5
    for c in cs:
        _assert_same(_run_case(c, dev), AR.case_reference(c), AR.case_id(c))


# ------------------------------------------------------------------------------------------------ the C entry over caller-owned buffers
class _Raw:
    """One form of the C entry over preallocated, sentinel-filled buffers (contiguous input)."""

    def __init__(self, dev, form, G, n, K, h):
        self.form, self.G, self.n, self.K, self.h = form, G, n, K, h
        S = n + K
        if form == "tokens":
            self.src = torch.full((G * n, 7 * h), AR.TOK_VOCAB - 128, dtype=torch.int64, device=dev)
            self.out = torch.empty(G * S, 7 * h, dtype=torch.int64, device=dev)
        else:
            self.src = torch.zeros(G * n, h, 7, device=dev)
            self.out = torch.empty(G * S, h, 7, device=dev)
        self.normals = torch.zeros(G, K, h, 6, device=dev)
        self.centers = torch.from_numpy(AR.openvla_centers()).to(dev)
        self.mean, self.sd = torch.empty(G, h, 6, device=dev), torch.empty(G, h, 6, device=dev)
        self.votes = torch.empty(G, h, 2, dtype=torch.int32, device=dev)
        self.fill()

    def outputs(self):
        return dict(out=self.out, mean=self.mean, sd=self.sd, votes=self.votes)

    def fill(self):
        for t in self.outputs().values():
            if t.dtype == torch.float32:
                t.view(torch.int32).fill_(SENTINEL_BITS)
            else:
                t.fill_(-7)

    def sentinels(self):
        """-> how many cells still hold the sentinel, per output."""
        return {k: int(((t.view(torch.int32) == SENTINEL_BITS) if t.dtype == torch.float32 else (t == -7)).sum()) for k, t in self.outputs().items()}

    def untouched(self):
        return all(v == t.numel() for v, t in zip(self.sentinels().values(), self.outputs().values()))

    def load(self, inp):
        self.src.copy_(torch.from_numpy(inp["tokens"] if self.form == "tokens" else inp["actions"]))
        self.normals.copy_(torch.from_numpy(inp["normals"]))
        self.centers.copy_(torch.from_numpy(inp["centers"]))

    def args(self, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0), **over):
        a = L.AugmentArgs()
        a.src, a.normals, a.out = self.src.data_ptr(), self.normals.data_ptr(), self.out.data_ptr()
        a.n_stride, a.t_stride = self.src.stride(0), (7 if self.form == "tokens" else self.src.stride(1))
        if self.form == "tokens":
            a.centers, a.n_centers, a.tok_vocab = self.centers.data_ptr(), self.centers.numel(), AR.TOK_VOCAB
        a.G, a.n, a.K, a.h = self.G, self.n, self.K, self.h
        a.sigma, a.sd_floor, a.clip_lo, a.clip_hi = sigma, sd_floor, clip[0], clip[1]
        a.mean_out, a.sd_out, a.votes_out = self.mean.data_ptr(), self.sd.data_ptr(), self.votes.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, **kw):
        a = self.args(**kw)
        fn = L.lib().cover_augment_tokens if self.form == "tokens" else L.lib().cover_augment_actions
        return fn(C.byref(a), torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 2. stores
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_every_output_cell_is_stored_and_the_originals_are_copied(dev, form):
    for shape, variant in (((3, 4, 65, 2), "spread"), ((2, 5, 123, 8), "clip"), ((1, 1, 1, 1), "spread"), ((2, 5, 32, 1), "k0")):
        c = dict(form=form, shape=shape, variant=variant)
        inp = AR.make_inputs(c)
        G, n, K, h = shape
        raw = _Raw(dev, form, G, n, inp["K"], h)
        raw.load(inp)
        assert raw.call(sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"]) == 0
        torch.cuda.synchronize()
        assert raw.sentinels() == dict(out=0, mean=0, sd=0, votes=0), AR.case_id(c)
        rows = raw.out.reshape(G, n + inp["K"], -1)[:, :n].reshape(raw.src.shape)
        assert np.array_equal(_bits(rows), _bits(raw.src)), AR.case_id(c)
        _assert_same(raw.outputs(), AR.case_reference(c), AR.case_id(c))
        # the optional outputs left out: nothing is written to them
        raw.fill()
        assert raw.call(sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"], mean_out=None, sd_out=None, votes_out=None) == 0
        torch.cuda.synchronize()
        s = raw.sentinels()
        assert s["out"] == 0 and (s["mean"], s["sd"], s["votes"]) == (raw.mean.numel(), raw.sd.numel(), raw.votes.numel())


# ------------------------------------------------------------------------------------------------ 3. graph replay
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_graph_replay_follows_the_static_buffers(dev, form):
    shape = (3, 4, 65, 2)
    G, n, K, h = shape
    raw = _Raw(dev, form, G, n, K, h)
    g, rc = graphs.capture(lambda: raw.call(sd_floor=0.02), dev)
    assert rc == 0
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # the capture itself executed nothing
    seen = []
    for variant in ("spread", "floor", "tie1"):
        inp = AR.make_inputs(dict(form=form, shape=shape, variant=variant))
        assert inp["centers"] is not None and inp["K"] == K
        raw.load(inp)
        raw.fill()
        g.launch()
        torch.cuda.synchronize()
        replayed = {k: t.clone() for k, t in raw.outputs().items()}
        raw.fill()
        assert raw.call(sd_floor=0.02) == 0                                # the eager launch on the same buffers
        torch.cuda.synchronize()
        _assert_same(replayed, raw.outputs(), f"replay {variant}")
        want = AR.reference_of(dict(inp, sigma=1.0, sd_floor=0.02, clip=(-1.0, 1.0)), form)
        _assert_same(replayed, want, f"replay {variant} vs reference")
        seen.append(_bits(replayed["out"]).tobytes())
    assert len(set(seen)) == 3                                             # the replays had different answers


# ------------------------------------------------------------------------------------------------ 4. argument errors
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_argument_errors_return_einval_and_launch_nothing(dev, form):
    raw = _Raw(dev, form, 2, 3, 4, 2)
    nan, inf = float("nan"), float("inf")
    bad = [dict(n=0), dict(n=-3), dict(n=4097), dict(K=-1), dict(K=4097), dict(h=0), dict(h=65), dict(G=0), dict(G=-2),
           dict(G=(1 << 20) // 7 + 1), dict(G=1 << 20, n=1, K=1),
           dict(sigma=-0.5), dict(sigma=nan), dict(sigma=inf), dict(sd_floor=-0.5), dict(sd_floor=nan), dict(sd_floor=inf),
           dict(clip=(0.5, -0.5)), dict(clip=(nan, 1.0)), dict(clip=(-1.0, nan)),
           dict(src=None), dict(out=None), dict(normals=None)]
    if form == "tokens":
        bad += [dict(n_stride=13), dict(n_stride=0), dict(centers=None), dict(n_centers=0), dict(n_centers=-1)]
    fn = L.lib().cover_augment_tokens if form == "tokens" else L.lib().cover_augment_actions
    for over in bad:
        assert raw.call(**over) == -1, over                                # COVER_EINVAL
        assert "augment" in L.lib().cover_last_error().decode()
    assert fn(None, torch.cuda.current_stream().cuda_stream) == -1
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # nothing was launched
    # at the limits, and the cases that are no errors: +-inf clip = no clip; K == 0 needs no normals
    assert raw.call(clip=(-inf, inf), sigma=0.0, sd_floor=0.0) == 0
    torch.cuda.synchronize()
    assert raw.sentinels() == dict(out=0, mean=0, sd=0, votes=0)
    k0 = _Raw(dev, form, 2, 3, 0, 2)
    assert k0.call(normals=None) == 0
    torch.cuda.synchronize()
    assert k0.sentinels()["out"] == 0 and np.array_equal(_bits(k0.out), _bits(k0.src))


# ------------------------------------------------------------------------------------------------ 5. OpenVLA end to end
def test_openvla_sample_augment_histories_score(dev):
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_prior_select_gpu import _verifier
    from tests.test_topn_gpu import _ov_case
    P, n, K = 2, 4, 12
    S = n + K
    c, sd, frame, toks, lens, u = _ov_case(P=P, n_samples=n)
    policy = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    tokens = policy.sample(frame.to(dev), toks.to(dev), lens.to(dev), n, u.to(dev), 0.9, top_k=50, top_p=0.9)[0]
    assert tuple(tokens.shape) == (P * n, 7)
    z = host.augmentation_normals(P, K, policy.n_gen // 7, seed=3)
    aug = policy.augment(tokens, n, K, z.to(dev), sigma=1.5, sd_floor=0.01)
    assert aug.dtype == torch.int64 and tuple(aug.shape) == (P * S, 7)
    centers = policy.bin_centers()
    assert policy.bin_centers() is centers and centers.dtype == torch.float32 and tuple(centers.shape) == (c["n_bins"] - 1,)
    want = AR.reference_tokens(tokens.cpu().numpy(), n, K, z.numpy(), centers.cpu().numpy(), c["tok_vocab"], 1, sigma=1.5, sd_floor=0.01)
    assert np.array_equal(aug.cpu().numpy(), want["out"])
    assert len({row.tobytes() for row in want["out"].reshape(P, S, 7)[0, n:]}) > 1                                        # distinct proposals
    assert int(aug.min()) >= policy.action_lo and int(aug.max()) < policy.action_hi
    assert torch.equal(aug.view(P, S, 7)[:, :n].reshape(P * n, 7), tokens)
    # de-tokenised on the host as sampled tokens are
    acts = policy.tokens_to_actions(aug.cpu().numpy())
    assert acts.shape == (P * S, 7) and np.abs(acts).max() <= 1.0
    # the verifier takes the S rows per prompt as it takes sampled candidates
    ver, its, _ = _verifier(dev, P * S)
    past = torch.from_numpy((np.random.default_rng(0).normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)
    hb, pad = ops.tokens_to_histories(aug, c["tok_vocab"], centers, past)
    r = ver.score_histories(its, hb, S, pad=pad)
    res = r["result"].cpu().tolist()
    assert 0 <= res[0] < P * S and res[0] // S == res[1] and res[0] % S == res[2]
    h1, _ = ops.tokens_to_histories(aug[res[0]:res[0] + 1], c["tok_vocab"], centers, past)
    assert np.array_equal(_bits(hb[res[0]]), _bits(h1[0]))


# ------------------------------------------------------------------------------------------------ 6. pi0 end to end
def test_pi0_select_action_augment(dev):
    from cover_vla_amd.pi0 import PI0Config, PI0FlowMatching, PI0Policy
    from tests.episode_replay import WordTokenizer, scripted_inputs
    from tests.helpers import pi0_case
    _, tiny, sd, _ = pi0_case(os.path.join(ROOT, "tests", "golden", "pi0_tiny_b6.npz"))
    G, n, K, steps, Lmax = 2, 3, 5, 4, 12
    S, B = n + K, G * n
    model = PI0FlowMatching(sd, tiny, device="cuda:0", max_batch=8, max_prompts=8, max_lang=Lmax)
    pol = PI0Policy(PI0Config(n_action_steps=steps, chunk_size=tiny["chunk"], tokenizer_max_length=Lmax, resize_imgs_with_padding=None), model,
                    WordTokenizer(tiny["vocab"]).policy)
    obs = scripted_inputs(1, B, tiny["chunk"], tiny["image"], seed=21)[0]
    tasks = [t for t in ("put the spoon on the towel", "move the spoon to the cloth") for _ in range(n)]
    batch = {"observation.images.top": obs["frame"].repeat(B, 1, 1, 1).to(dev), "observation.state": obs["state"].repeat(B, 1).to(dev), "task": tasks}
    noise = obs["noise"].to(dev)
    q = pol.select_action(batch, noise=noise)
    plain = torch.stack([a.clone() for a in q], dim=1)                     # [B, steps, 7]
    assert tuple(plain.shape) == (B, steps, 7)
    q.clear()
    z = host.augmentation_normals(G, K, steps, seed=5)
    q = pol.select_action(batch, noise=noise, augment=host.Augment(n, K, z.to(dev), sigma=0.8, sd_floor=0.0, clip=(-float("inf"), float("inf"))))
    assert len(q) == steps and all(tuple(a.shape) == (G * S, 7) and a.dtype == torch.float32 for a in q)
    aug = torch.stack([a.clone() for a in q], dim=1)                       # [G * S, steps, 7]
    q.clear()
    for g in range(G):
        assert np.array_equal(_bits(aug[g * S:g * S + n]), _bits(plain[g * n:(g + 1) * n]))    # the policy's own rows, bit for bit
    want = AR.reference_actions(plain.cpu().numpy(), n, K, z.numpy(), sigma=0.8, sd_floor=0.0, clip=(-np.inf, np.inf))
    assert np.array_equal(_bits(aug), _bits(want["out"]))
    assert len(pol.select_action(batch, noise=noise)) == steps and tuple(pol._action_queue[0].shape) == (B, 7)   # None: as before
