"""Verifier-guided refinement on the GPU: cover_refine_tokens / cover_refine_actions against the reference of tests/refine_ref.py, bit for
bit (every rounding is specified, so there is no tolerance), the composition identity with cover_augment_*, every output cell stored and
nothing outside the view read, graph replay, argument errors of the C entries, OpenVLA.refine and score_refined end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, host, ops
from cover_vla_amd import _lib as L
from tests import augment_ref as AR
from tests import refine_ref as RR

pytestmark = pytest.mark.gpu
KEYS = ("out", "elite_rows", "elite_scores", "mean", "sd", "votes")
SENTINEL_BITS = 0x7FC12345          # a NaN payload no result carries


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, got[k], want[k])


def _laid_out(c, inp, dev, junk=1):
    """The case's input as the device sees it: tokens through the table's row stride (beyond 7 h at every other shape), actions through
    the strides (chunk * 32, 32) of a [N, chunk, 32] buffer at the strided shape; the cells outside the view hold junk."""
    h = c["shape"][4]
    rng = np.random.default_rng(junk)
    if c["form"] == "tokens":
        tok = inp["tokens"]
        ld = RR.token_row_stride(c["shape"]) if c["shape"] in RR.SHAPES else 7 * h
        buf = rng.integers(RR.TOK_VOCAB - 256, RR.TOK_VOCAB, (tok.shape[0], ld)).astype(np.int64)
        buf[:, :7 * h] = tok
        view = torch.from_numpy(buf).to(dev)[:, :7 * h]
        assert view.stride(0) == ld
        return view
    x = inp["actions"]
    if c["shape"] == RR.STRIDED:
        chunk = h + 2
        buf = rng.uniform(-1, 1, (x.shape[0], chunk, 32)).astype(np.float32)
        buf[:, :h, :7] = x
        view = torch.from_numpy(buf).to(dev)[:, :h, :7]
        assert view.stride() == (chunk * 32, 32, 1)
        return view
    return torch.from_numpy(x).to(dev)


def _refine(form, src, scores, S, m, K, z, centers, h, **kw):
    if form == "tokens":
        return ops.refine_tokens(src, scores, S, m, K, z, centers, RR.TOK_VOCAB, steps=h, **kw)
    return ops.refine_actions(src, scores, S, m, K, z, **kw)


def _augment(form, src, n, K, z, centers, h, **kw):
    if form == "tokens":
        return ops.augment_tokens(src, n, K, z, centers, RR.TOK_VOCAB, steps=h, **kw)
    return ops.augment_actions(src, n, K, z, **kw)


def _run_case(c, dev, junk=1):
    inp = RR.make_inputs(c)
    src, z = _laid_out(c, inp, dev, junk), torch.from_numpy(inp["normals"]).to(dev)
    out, st, el = _refine(c["form"], src, torch.from_numpy(inp["scores"]).to(dev), inp["S"], inp["m"], inp["K"], z,
                          torch.from_numpy(inp["centers"]).to(dev), c["shape"][4], sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"],
                          stats=True, elites=True)
    return dict(out=out, elite_rows=el.rows, elite_scores=el.scores, mean=st.mean, sd=st.sd, votes=st.votes)


# ------------------------------------------------------------------------------------------------ 1. every case of the table
def _shape_params():
    return [(f, s) for f in ("tokens", "actions") for s in RR.SHAPES + (RR.FLOAT_ONLY if f == "actions" else [])]


@pytest.mark.parametrize("form,shape", _shape_params(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_matches_reference_bit_for_bit(dev, form, shape):
    cs = RR.cases(forms=(form,), shapes=(shape,))
    assert len(cs) >= 2
    for c in cs:
        _assert_same(_run_case(c, dev), RR.case_reference(c), RR.case_id(c))


# ------------------------------------------------------------------------------------------------ 2. composition identity
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_new_rows_are_augment_of_the_gathered_rows(dev, form):
    for shape, variant in (((3, 37, 4, 65, 2), "ties"), ((2, 64, 8, 56, 4), "nan"), ((1, 2, 1, 3, 1), "distinct"), ((1, 300, 5, 7, 2), "neg_inf")):
        c = dict(form=form, shape=shape, variant=variant)
        inp, got = RR.make_inputs(c), _run_case(c, dev)
        G, S, m, K, h = shape
        out = got["out"]
        elites = out.reshape((G, m + K) + tuple(out.shape[1:]))[:, :m].reshape((G * m,) + tuple(out.shape[1:])).contiguous()
        aug, st = _augment(form, elites, m, K, torch.from_numpy(inp["normals"]).to(dev), torch.from_numpy(inp["centers"]).to(dev), h,
                           sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"], stats=True)
        _assert_same(dict(out=aug, mean=st.mean, sd=st.sd, votes=st.votes), got, RR.case_id(c), keys=("out", "mean", "sd", "votes"))


@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_all_rows_elite_in_descending_order_is_augment(dev, form):
    G, n, K, h = 3, 6, 40, 2
    rng = np.random.default_rng(8)
    b = rng.integers(20, 235, (G * n, h, 7))
    centers = AR.openvla_centers()
    if form == "tokens":
        src = torch.from_numpy((RR.TOK_VOCAB - 1 - b).astype(np.int64).reshape(G * n, 7 * h)).to(dev)
    else:
        src = torch.from_numpy((centers[b] + rng.uniform(-0.003, 0.003, b.shape)).astype(np.float32)).to(dev)
    z = host.augmentation_normals(G, K, h, seed=2).to(dev)
    cen = torch.from_numpy(centers).to(dev)
    scores = torch.from_numpy(np.tile(-np.arange(n, dtype=np.float32), G)).to(dev)              # strictly descending inside every group
    kw = dict(sigma=0.9, sd_floor=0.01, clip=(-0.8, 0.8), stats=True)
    out, st, el = _refine(form, src, scores, n, n, K, z, cen, h, elites=True, **kw)
    aug, st2 = _augment(form, src, n, K, z, cen, h, **kw)
    _assert_same(dict(out=out, mean=st.mean, sd=st.sd, votes=st.votes), dict(out=aug, mean=st2.mean, sd=st2.sd, votes=st2.votes), form,
                 keys=("out", "mean", "sd", "votes"))
    assert np.array_equal(el.rows.cpu().numpy().reshape(-1), np.arange(G * n)) and np.array_equal(_bits(el.scores).reshape(-1), _bits(scores))


# ------------------------------------------------------------------------------------------------ the C entry over caller-owned buffers
class _Raw:
    """One form of the C entry over preallocated, sentinel-filled buffers (contiguous input)."""

    def __init__(self, dev, form, G, S, m, K, h):
        self.form, self.G, self.S, self.m, self.K, self.h = form, G, S, m, K, h
        if form == "tokens":
            self.src = torch.full((G * S, 7 * h), RR.TOK_VOCAB - 128, dtype=torch.int64, device=dev)
            self.out = torch.empty(G * (m + K), 7 * h, dtype=torch.int64, device=dev)
        else:
            self.src = torch.zeros(G * S, h, 7, device=dev)
            self.out = torch.empty(G * (m + K), h, 7, device=dev)
        self.scores = torch.zeros(G * S, device=dev)
        self.normals = torch.zeros(G, K, h, 6, device=dev)
        self.centers = torch.from_numpy(AR.openvla_centers()).to(dev)
        self.elite_rows = torch.empty(G, m, dtype=torch.int32, device=dev)
        self.elite_scores = torch.empty(G, m, device=dev)
        self.mean, self.sd = torch.empty(G, h, 6, device=dev), torch.empty(G, h, 6, device=dev)
        self.votes = torch.empty(G, h, 2, dtype=torch.int32, device=dev)
        self.fill()

    def outputs(self):
        return dict(out=self.out, elite_rows=self.elite_rows, elite_scores=self.elite_scores, mean=self.mean, sd=self.sd, votes=self.votes)

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
        self.src.copy_(torch.from_numpy(inp[self.form]))
        self.scores.copy_(torch.from_numpy(inp["scores"]))
        self.normals.copy_(torch.from_numpy(inp["normals"]))
        self.centers.copy_(torch.from_numpy(inp["centers"]))

    def args(self, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0), **over):
        a = L.RefineArgs()
        a.src, a.scores, a.normals, a.out = self.src.data_ptr(), self.scores.data_ptr(), self.normals.data_ptr(), self.out.data_ptr()
        a.n_stride, a.t_stride = self.src.stride(0), (7 if self.form == "tokens" else self.src.stride(1))
        if self.form == "tokens":
            a.centers, a.n_centers, a.tok_vocab = self.centers.data_ptr(), self.centers.numel(), RR.TOK_VOCAB
        a.G, a.group_rows, a.n_elite, a.K, a.h = self.G, self.S, self.m, self.K, self.h
        a.sigma, a.sd_floor, a.clip_lo, a.clip_hi = sigma, sd_floor, clip[0], clip[1]
        a.elite_rows_out, a.elite_scores_out = self.elite_rows.data_ptr(), self.elite_scores.data_ptr()
        a.mean_out, a.sd_out, a.votes_out = self.mean.data_ptr(), self.sd.data_ptr(), self.votes.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, **kw):
        a = self.args(**kw)
        fn = L.lib().cover_refine_tokens if self.form == "tokens" else L.lib().cover_refine_actions
        return fn(C.byref(a), torch.cuda.current_stream().cuda_stream)


ALL_STORED = dict(out=0, elite_rows=0, elite_scores=0, mean=0, sd=0, votes=0)


# ------------------------------------------------------------------------------------------------ 3. stores and reads
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_every_output_cell_is_stored(dev, form):
    for shape, variant in (((3, 37, 4, 65, 2), "distinct"), ((1, 300, 5, 7, 2), "ties"), ((1, 1, 1, 1, 1), "distinct"), ((2, 5, 2, 32, 1), "k0")):
        c = dict(form=form, shape=shape, variant=variant)
        inp = RR.make_inputs(c)
        G, S, m, K, h = shape
        raw = _Raw(dev, form, G, S, m, inp["K"], h)
        raw.load(inp)
        kw = dict(sigma=inp["sigma"], sd_floor=inp["sd_floor"], clip=inp["clip"])
        assert raw.call(**kw) == 0
        torch.cuda.synchronize()
        assert raw.sentinels() == ALL_STORED, RR.case_id(c)
        _assert_same(raw.outputs(), RR.case_reference(c), RR.case_id(c))
        # the optional outputs left out: nothing is written to them
        raw.fill()
        assert raw.call(elite_rows_out=None, elite_scores_out=None, mean_out=None, sd_out=None, votes_out=None, **kw) == 0
        torch.cuda.synchronize()
        s = raw.sentinels()
        assert s.pop("out") == 0 and all(s[k] == getattr(raw, k).numel() for k in s), RR.case_id(c)
        _assert_same(raw.outputs(), RR.case_reference(c), RR.case_id(c), keys=("out",))


def test_cells_outside_the_view_are_not_read(dev):
    for c in (dict(form="tokens", shape=(3, 37, 4, 65, 2), variant="ties"), dict(form="actions", shape=RR.STRIDED, variant="distinct"),
              dict(form="tokens", shape=(1, 300, 5, 7, 2), variant="nan")):
        assert c["form"] == "actions" or RR.token_row_stride(c["shape"]) > 7 * c["shape"][4]
        a, b = _run_case(c, dev, junk=1), _run_case(c, dev, junk=2)
        _assert_same(a, b, RR.case_id(c))
        _assert_same(a, RR.case_reference(c), RR.case_id(c))


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_graph_replay_follows_the_static_buffers(dev, form):
    shape = (3, 37, 4, 65, 2)
    G, S, m, K, h = shape
    raw = _Raw(dev, form, G, S, m, K, h)
    g, rc = graphs.capture(lambda: raw.call(sd_floor=0.02), dev)
    assert rc == 0
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # the capture itself executed nothing
    seen = []
    for variant in ("distinct", "ties", "nan"):
        inp = RR.make_inputs(dict(form=form, shape=shape, variant=variant))
        raw.load(inp)
        raw.fill()
        g.launch()
        torch.cuda.synchronize()
        replayed = {k: t.clone() for k, t in raw.outputs().items()}
        raw.fill()
        assert raw.call(sd_floor=0.02) == 0                                # the eager launch on the same buffers
        torch.cuda.synchronize()
        _assert_same(replayed, raw.outputs(), f"replay {variant}")
        want = RR.reference_of(dict(inp, sigma=1.0, sd_floor=0.02, clip=(-1.0, 1.0)), form)
        _assert_same(replayed, want, f"replay {variant} vs reference")
        seen.append(_bits(replayed["out"]).tobytes())
    assert len(set(seen)) == 3                                             # the replays had different answers


# ------------------------------------------------------------------------------------------------ 5. argument errors
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_argument_errors_return_einval_and_launch_nothing(dev, form):
    raw = _Raw(dev, form, 2, 6, 3, 4, 2)
    nan, inf = float("nan"), float("inf")
    bad = [dict(G=0), dict(G=-2), dict(n_elite=0), dict(n_elite=-1), dict(n_elite=7), dict(group_rows=2), dict(group_rows=4097, n_elite=4097),
           dict(group_rows=4097), dict(K=-1), dict(K=4097), dict(h=0), dict(h=65),
           dict(G=(1 << 20) // 6 + 1), dict(G=(1 << 20) // 7 + 1, group_rows=3), dict(G=1 << 20, group_rows=1, n_elite=1, K=1),
           dict(sigma=-0.5), dict(sigma=nan), dict(sigma=inf), dict(sd_floor=-0.5), dict(sd_floor=nan), dict(sd_floor=inf),
           dict(clip=(0.5, -0.5)), dict(clip=(nan, 1.0)), dict(clip=(-1.0, nan)),
           dict(src=None), dict(scores=None), dict(out=None), dict(normals=None)]
    if form == "tokens":
        bad += [dict(n_stride=13), dict(n_stride=0), dict(centers=None), dict(n_centers=0), dict(n_centers=-1)]
    fn = L.lib().cover_refine_tokens if form == "tokens" else L.lib().cover_refine_actions
    for over in bad:
        assert raw.call(**over) == -1, over                                # COVER_EINVAL
        assert "refine" in L.lib().cover_last_error().decode()
    assert fn(None, torch.cuda.current_stream().cuda_stream) == -1
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # nothing was launched
    # at the limits, and the cases that are no errors: +-inf clip = no clip; K == 0 needs no normals; every row an elite
    assert raw.call(clip=(-inf, inf), sigma=0.0, sd_floor=0.0) == 0
    torch.cuda.synchronize()
    assert raw.sentinels() == ALL_STORED
    k0 = _Raw(dev, form, 2, 6, 6, 0, 2)
    assert k0.call(normals=None) == 0
    torch.cuda.synchronize()
    assert k0.sentinels()["out"] == 0 and np.array_equal(_bits(k0.out), _bits(k0.src))          # equal scores: rows 0..S-1 in place


# ------------------------------------------------------------------------------------------------ 6. OpenVLA.refine
def test_openvla_refine_is_refine_tokens_with_the_models_table(dev):
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_topn_gpu import _ov_case
    P, n, K0, m, K = 2, 4, 12, 3, 9
    S = n + K0
    c, sd, frame, toks, lens, u = _ov_case(P=P, n_samples=n)
    policy = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    tokens = policy.sample(frame.to(dev), toks.to(dev), lens.to(dev), n, u.to(dev), 0.9, top_k=50, top_p=0.9)[0]
    aug = policy.augment(tokens, n, K0, host.augmentation_normals(P, K0, policy.n_gen // 7, seed=3).to(dev), sigma=1.5, sd_floor=0.01)
    scores = torch.from_numpy(np.random.default_rng(4).normal(size=P * S).astype(np.float32)).to(dev)
    z = host.augmentation_normals(P, K, policy.n_gen // 7, seed=6).to(dev)
    ref, el = policy.refine(aug, scores, S, m, z, sigma=0.7, sd_floor=0.02, elites=True)
    want, wel = ops.refine_tokens(aug, scores, S, m, K, z, policy.bin_centers(), c["tok_vocab"], steps=policy.n_gen // 7, sigma=0.7, sd_floor=0.02,
                                  elites=True)
    assert ref.dtype == torch.int64 and tuple(ref.shape) == (P * (m + K), 7) and torch.equal(ref, want)
    assert torch.equal(el.rows, wel.rows) and np.array_equal(_bits(el.scores), _bits(wel.scores))
    assert torch.equal(policy.refine(aug, scores, S, m, z, sigma=0.7, sd_floor=0.02), ref)
    r = RR.reference(aug.cpu().numpy(), scores.cpu().numpy(), S, m, K, z.cpu().numpy(), "tokens", policy.bin_centers().cpu().numpy(), 1, 0.7, 0.02,
                     tok_vocab=c["tok_vocab"])
    assert np.array_equal(ref.cpu().numpy(), r["out"]) and np.array_equal(el.rows.cpu().numpy(), r["elite_rows"])
    assert int(ref.min()) >= policy.action_lo and int(ref.max()) < policy.action_hi
    # the result goes where augment's goes, with group_size = m + K and n_fit = m
    past = torch.from_numpy((np.random.default_rng(0).normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)
    hb, pad = ops.tokens_to_histories(ref, c["tok_vocab"], policy.bin_centers(), past)
    assert tuple(hb.shape) == (P * (m + K), 10, 7) and tuple(pad.shape) == (P * (m + K), 10)
    prior, st = ops.proposal_prior_tokens(ref, m + K, m, policy.bin_centers(), c["tok_vocab"], steps=1, sigma=0.7, sd_floor=0.02, stats=True)
    assert tuple(prior.shape) == (P * (m + K),) and np.array_equal(_bits(policy.proposal_prior(ref, m + K, m, sigma=0.7, sd_floor=0.02)), _bits(prior))
    assert np.array_equal(_bits(st.mean), _bits(r["mean"])) and np.array_equal(_bits(st.sd), _bits(r["sd"]))   # the fit the rows were drawn from


# ------------------------------------------------------------------------------------------------ 7. score_refined
def _token_pipeline(dev, P, S, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(20, 235, (P * S, 7))
    cands = torch.from_numpy((RR.TOK_VOCAB - 1 - b).astype(np.int64)).to(dev)
    cen = torch.from_numpy(AR.openvla_centers()).to(dev)
    past = torch.from_numpy((rng.normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)
    to_hist = lambda t: ops.tokens_to_histories(t, RR.TOK_VOCAB, cen, past)
    refine = lambda t, v, S_, m, z: ops.refine_tokens(t, v, S_, m, z.shape[1], z, cen, RR.TOK_VOCAB, sigma=0.8, sd_floor=0.01, elites=True)
    prior_fn = lambda t, S_, n_fit: ops.proposal_prior_tokens(t, S_, n_fit if n_fit is not None else 4, cen, RR.TOK_VOCAB, sigma=1.0, sd_floor=0.01)
    return cands, to_hist, refine, prior_fn


def _same_dict(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


@pytest.mark.parametrize("kw,key", ((dict(), "scores"), (dict(member_kappa=0.5, prior_beta=0.3, top_m=3), "combined")), ids=("plain", "robust-prior"))
def test_score_refined_equals_the_hand_written_sequence(dev, kw, key):
    from tests.test_prior_select_gpu import _verifier
    P, S, m = 3, 20, 4
    ver, its, _ = _verifier(dev, P * S)
    cands, to_hist, refine, prior_fn = _token_pipeline(dev, P, S, seed=11)
    if "prior_beta" not in kw:
        prior_fn = None
    normals = [host.augmentation_normals(P, K, 1, seed=20 + i).to(dev) for i, K in enumerate((12, 6))]
    got = ver.score_refined(its, cands, S, to_histories=to_hist, refine=refine, normals=normals, n_elite=m, prior_fn=prior_fn, **kw)
    # the same calls by hand
    t, gs, n_fit, outs, rows = cands, S, None, [], [None]
    for r in range(3):
        if r:
            t, el = refine(t, outs[-1][key], gs, m, normals[r - 1])
            gs, n_fit = m + normals[r - 1].shape[1], m
            rows.append(el.rows)
        hb, pad = to_hist(t)
        k2 = dict(kw, prior=prior_fn(t, gs, n_fit)) if prior_fn is not None else dict(kw)
        outs.append(ver.score_histories(its, hb, gs, pad=pad, **k2))
    assert key in outs[-1] and (key == "scores" or "robust" in outs[-1])
    _same_dict({k: v for k, v in got.items() if k not in ("candidates", "rounds")}, outs[-1], "last round")
    assert torch.equal(got["candidates"], t) and tuple(t.shape) == (P * (m + 6), 7)
    assert len(got["rounds"]) == 3 and got["rounds"][0]["elite_rows"] is None
    for r in range(3):
        assert torch.equal(got["rounds"][r]["result"], outs[r]["result"]) and np.array_equal(_bits(got["rounds"][r]["best"]), _bits(outs[r]["best"]))
        if r:
            assert torch.equal(got["rounds"][r]["elite_rows"], rows[r])
    res = got["result"].cpu().tolist()
    assert 0 <= res[0] < P * (m + 6) and res[0] // (m + 6) == res[1]
    # no rounds: one score_histories call, the given candidates
    one = ver.score_refined(its, cands, S, to_histories=to_hist, refine=None, normals=[], n_elite=m, prior_fn=prior_fn, **kw)
    _same_dict({k: v for k, v in one.items() if k not in ("candidates", "rounds")}, outs[0], "no rounds")
    assert one["candidates"] is cands and len(one["rounds"]) == 1


class _RowWiseScorer:
    """A scorer whose value of a row depends on that row alone, on the device: the closeness of the row's own action to a target."""

    def __init__(self, target):
        self.target, self.calls = target, 0

    def score_histories(self, its, hb, group_size, pad=None, **kw):
        self.calls += 1
        scores = -((hb[:, -1, :6] - self.target) ** 2).sum(dim=1).contiguous()
        result, best = ops.group_argmax(scores, group_size)
        return {"scores": scores, "result": result, "best": best, "group_best": scores.reshape(-1, group_size).max(dim=1).values}


def test_best_value_never_decreases_under_a_row_wise_scorer(dev):
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    P, S, m = 4, 16, 3
    cands, to_hist, refine, _ = _token_pipeline(dev, P, S, seed=12)
    scorer = _RowWiseScorer(torch.tensor([0.3, -0.2, 0.1, 0.0, 0.4, -0.5], device=dev))
    normals = [host.augmentation_normals(P, 13, 1, seed=30 + i).to(dev) for i in range(3)]
    best, group_best = [], []

    def spy(t, v, S_, m_, z):
        group_best.append(v.reshape(-1, S_).max(dim=1).values)
        return refine(t, v, S_, m_, z)
    got = EfficientEnsembleMerged.score_refined(scorer, None, cands, S, to_histories=to_hist, refine=spy, normals=normals, n_elite=m)
    assert scorer.calls == 4 and len(got["rounds"]) == 4 and tuple(got["candidates"].shape) == (P * (m + 13), 7)
    group_best.append(got["group_best"])
    for a, b in zip(group_best[:-1], group_best[1:]):
        assert bool((b >= a).all())                                        # every prompt: its elites are carried verbatim
    best = [float(r["best"][0]) for r in got["rounds"]]
    assert all(y >= x for x, y in zip(best[:-1], best[1:])), best
    assert best[-1] > best[0]                                              # and the refinement found something: not a vacuous chain
