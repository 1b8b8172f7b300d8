"""Neighbourhood-smoothed scores on the GPU: cover_smooth_scores_tokens / cover_smooth_scores_actions against the reference of
tests/smooth_ref.py, bit for bit (every rounding is specified, so there is no tolerance), special rows as bit patterns, every output cell
stored and nothing outside the view read, graph replay, argument errors of the C entries, and the layers above them end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, host, ops
from cover_vla_amd import _lib as L
from tests import augment_ref as AR
from tests import smooth_ref as SR

pytestmark = pytest.mark.gpu
KEYS = ("smoothed", "density", "neighbours", "group_mean")
SENTINEL_BITS = 0x7FC12345          # a NaN payload no result carries
F32 = np.float32


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, got[k], want[k])


def _laid_out(form, shape, inp, dev, junk=1):
    """The input as the device sees it: tokens through the table's row stride (beyond 7 h at every other shape), actions through the
    strides (chunk * 32, 32, 1) of a [N, chunk, 32] buffer at the strided shape; the cells outside the view hold junk."""
    h = shape[2]
    rng = np.random.default_rng(junk)
    if form == "tokens":
        tok = inp["tokens"]
        ld = SR.token_row_stride(shape)
        buf = rng.integers(SR.TOK_VOCAB - 256, SR.TOK_VOCAB, (tok.shape[0], ld)).astype(np.int64)
        buf[:, :7 * h] = tok
        view = torch.from_numpy(buf).to(dev)[:, :7 * h]
        assert view.stride(0) == ld or tok.shape[0] == 1
        return view
    x = inp["actions"]
    if shape == SR.STRIDED:
        chunk = h + 2
        buf = rng.uniform(-1, 1, (x.shape[0], chunk, 32)).astype(np.float32)
        buf[:, :h, :7] = x
        view = torch.from_numpy(buf).to(dev)[:, :h, :7]
        assert view.stride() == (chunk * 32, 32, 1)
        return view
    return torch.from_numpy(x).to(dev)


def _smooth(form, src, scores, S, centers, h, **kw):
    if form == "tokens":
        return ops.smooth_scores_tokens(src, scores, S, centers, SR.TOK_VOCAB, steps=h, **kw)
    return ops.smooth_scores_actions(src, scores, S, **kw)


def _run(form, shape, inp, dev, junk=1, scores=None):
    src = _laid_out(form, shape, inp, dev, junk)
    s = torch.from_numpy(inp["scores"] if scores is None else scores).to(dev)
    sm, st = _smooth(form, src, s, inp["S"], torch.from_numpy(inp["centers"]).to(dev), shape[2], radius=inp["radius"],
                     dim_scale=inp["dim_scale"], shrink=inp["shrink"], split_gripper=bool(inp["split"]), stats=True)
    return dict(smoothed=sm, density=st.density, neighbours=st.neighbours, group_mean=st.group_mean)


def _run_case(c, dev, junk=1):
    return _run(c["form"], c["shape"], SR.make_inputs(c), dev, junk)


# ------------------------------------------------------------------------------------------------ 1. every case of the table
def _shape_params():
    return [(f, s) for f in ("tokens", "actions") for s in SR.shapes_of(f)]


@pytest.mark.parametrize("form,shape", _shape_params(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_matches_reference_bit_for_bit(dev, form, shape):
    cs = SR.cases(forms=(form,), shapes=(shape,))
    assert len(cs) == 4                                                    # shrink in {0, 0.5} x split_gripper in {0, 1}
    for c in cs:
        _assert_same(_run_case(c, dev), SR.case_reference(c), SR.case_id(c))


# ------------------------------------------------------------------------------------------------ 2. special rows
def test_special_scores_pass_through_and_leave_their_neighbours_alone(dev):
    for form in ("tokens", "actions"):
        c = dict(form=form, shape=(2, 65, 1), shrink=0.5, split=0)
        inp = SR.make_inputs(c)
        s = inp["scores"].copy()
        s.view(np.uint32)[[3, 70]] = 0x7FC00ABC, 0xFFC12345                # NaNs with payloads, both signs
        s[[10, 80]], s[[20, 90]] = np.inf, -np.inf
        special = [3, 70, 10, 80, 20, 90]
        x = SR.values_of(inp, form, 1)
        got = _run(form, c["shape"], inp, dev, scores=s)
        _assert_same(got, SR.reference(x, s, 65, inp["dim_scale"], inp["radius"], 0.5, 0), form)
        assert np.array_equal(_bits(got["smoothed"])[special], s.view(np.int32)[special])
        if form == "actions":                                              # the same rows moved out of every radius: the others do not change
            far = dict(inp, actions=inp["actions"].copy())
            far["actions"][special, 0, 0] += F32(50.0) + np.arange(6, dtype=F32)
            moved = _run(form, c["shape"], far, dev, scores=s)
            rest = np.setdiff1d(np.arange(130), special)
            assert np.array_equal(_bits(moved["smoothed"])[rest], _bits(got["smoothed"])[rest])
            assert np.array_equal(_bits(moved["group_mean"]), _bits(got["group_mean"]))
            assert (moved["neighbours"].cpu().numpy()[special] == 1).all()


def test_nan_element_isolates_its_row_only(dev):
    c = dict(form="actions", shape=(3, 17, 1), shrink=0.0, split=1)
    inp = SR.make_inputs(c)
    clean = _run("actions", c["shape"], inp, dev)
    row = int(np.argmax(clean["neighbours"].cpu().numpy()))                # a row that has neighbours
    assert int(clean["neighbours"][row]) > 1
    bad = dict(inp, actions=inp["actions"].copy())
    bad["actions"][row, 0, 2] = np.nan
    got = _run("actions", c["shape"], bad, dev)
    _assert_same(got, SR.reference(bad["actions"], inp["scores"], 17, inp["dim_scale"], inp["radius"], 0.0, 1), "nan element")
    assert int(got["neighbours"][row]) == 1 and _bits(got["smoothed"])[row] == inp["scores"].view(np.int32)[row]
    others = [i for i in range(51) if i // 17 != row // 17]                # the other groups: untouched
    assert np.array_equal(_bits(got["smoothed"])[others], _bits(clean["smoothed"])[others])
    assert not np.isnan(got["smoothed"].cpu().numpy()).any()


def test_group_without_a_finite_score(dev):
    c = dict(form="actions", shape=(3, 17, 1), shrink=0.5, split=1)
    inp = SR.make_inputs(c)
    s = inp["scores"].copy()
    s[17:34] = [np.nan, np.inf, -np.inf] * 5 + [np.nan, -np.inf]
    got = _run("actions", c["shape"], inp, dev, scores=s)
    _assert_same(got, SR.reference(inp["actions"], s, 17, inp["dim_scale"], inp["radius"], 0.5, 1), "no finite score")
    assert np.array_equal(_bits(got["smoothed"])[17:34], s.view(np.int32)[17:34]) and _bits(got["group_mean"])[1] == 0
    assert np.isfinite(got["smoothed"].cpu().numpy()[:17]).all()


# ------------------------------------------------------------------------------------------------ the C entry over caller-owned buffers
class _Raw:
    """One form of the C entry over preallocated, sentinel-filled buffers (contiguous input)."""

    def __init__(self, dev, form, G, S, h):
        self.form, self.G, self.S, self.h = form, G, S, h
        if form == "tokens":
            self.src = torch.full((G * S, 7 * h), SR.TOK_VOCAB - 128, dtype=torch.int64, device=dev)
        else:
            self.src = torch.zeros(G * S, h, 7, device=dev)
        self.scores = torch.zeros(G * S, device=dev)
        self.dim_scale = torch.tensor(SR.DIM_SCALE, dtype=torch.float32, device=dev)
        self.centers = torch.from_numpy(AR.openvla_centers()).to(dev)
        self.smoothed, self.density = torch.empty(G * S, device=dev), torch.empty(G * S, device=dev)
        self.neighbours = torch.empty(G * S, dtype=torch.int32, device=dev)
        self.group_mean = torch.empty(G, device=dev)
        self.fill()

    def outputs(self):
        return dict(smoothed=self.smoothed, density=self.density, neighbours=self.neighbours, group_mean=self.group_mean)

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
        self.dim_scale.copy_(torch.tensor(inp["dim_scale"], dtype=torch.float32))

    def args(self, radius=0.1, shrink=0.0, split=1, **over):
        a = L.SmoothArgs()
        a.src, a.scores, a.dim_scale = self.src.data_ptr(), self.scores.data_ptr(), self.dim_scale.data_ptr()
        a.n_stride, a.t_stride = self.src.stride(0), (7 if self.form == "tokens" else self.src.stride(1))
        if self.form == "tokens":
            a.centers, a.n_centers, a.tok_vocab = self.centers.data_ptr(), self.centers.numel(), SR.TOK_VOCAB
        a.G, a.group_rows, a.h, a.split_gripper = self.G, self.S, self.h, split
        a.radius2, a.shrink = float(F32(radius) * F32(radius)), shrink
        a.smoothed_out, a.density_out = self.smoothed.data_ptr(), self.density.data_ptr()
        a.neighbours_out, a.group_mean_out = self.neighbours.data_ptr(), self.group_mean.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, **kw):
        a = self.args(**kw)
        fn = L.lib().cover_smooth_scores_tokens if self.form == "tokens" else L.lib().cover_smooth_scores_actions
        return fn(C.byref(a), torch.cuda.current_stream().cuda_stream)


ALL_STORED = dict(smoothed=0, density=0, neighbours=0, group_mean=0)


# ------------------------------------------------------------------------------------------------ 3. stores and reads
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_every_output_cell_is_stored(dev, form):
    for shape in ((3, 17, 1), (1, 130, 3), (1, 1, 1), (2, 65, 1)):
        c = dict(form=form, shape=shape, shrink=0.5, split=1)
        inp = SR.make_inputs(c)
        raw = _Raw(dev, form, *shape)
        raw.load(inp)
        kw = dict(radius=inp["radius"], shrink=0.5, split=1)
        assert raw.call(**kw) == 0
        torch.cuda.synchronize()
        assert raw.sentinels() == ALL_STORED, SR.case_id(c)
        _assert_same(raw.outputs(), SR.case_reference(c), SR.case_id(c))
        # the optional outputs left out: nothing is written to them, and smoothed is what it was
        raw.fill()
        assert raw.call(density_out=None, neighbours_out=None, group_mean_out=None, **kw) == 0
        torch.cuda.synchronize()
        s = raw.sentinels()
        assert s.pop("smoothed") == 0 and all(s[k] == getattr(raw, k).numel() for k in s), SR.case_id(c)
        _assert_same(raw.outputs(), SR.case_reference(c), SR.case_id(c), keys=("smoothed",))


def test_cells_outside_the_view_are_not_read(dev):
    for c in (dict(form="tokens", shape=(3, 17, 1), shrink=0.5, split=1), dict(form="actions", shape=SR.STRIDED, shrink=0.0, split=1),
              dict(form="tokens", shape=(1, 130, 3), shrink=0.0, split=0)):
        assert c["form"] == "actions" or SR.token_row_stride(c["shape"]) > 7 * c["shape"][2]
        a, b = _run_case(c, dev, junk=1), _run_case(c, dev, junk=2)
        _assert_same(a, b, SR.case_id(c))
        _assert_same(a, SR.case_reference(c), SR.case_id(c))


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_graph_replay_follows_the_static_buffers(dev, form):
    shape = (2, 65, 1)
    raw = _Raw(dev, form, *shape)
    radius = SR.case_radius(shape)
    g, rc = graphs.capture(lambda: raw.call(radius=radius, shrink=0.5), dev)
    assert rc == 0
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # the capture itself executed nothing
    seen = []
    base = SR.make_inputs(dict(form=form, shape=shape, shrink=0.5, split=1))
    for k in range(2):
        inp = dict(base, scores=np.roll(base["scores"], 7 * k) + F32(0.125 * k))    # refreshed inputs
        raw.load(inp)
        raw.fill()
        g.launch()
        torch.cuda.synchronize()
        replayed = {n: t.clone() for n, t in raw.outputs().items()}
        raw.fill()
        assert raw.call(radius=radius, shrink=0.5) == 0                    # the eager launch on the same buffers
        torch.cuda.synchronize()
        _assert_same(replayed, raw.outputs(), f"replay {k}")
        _assert_same(replayed, SR.reference_of(inp, form, 1), f"replay {k} vs reference")
        seen.append(_bits(replayed["smoothed"]).tobytes())
    assert len(set(seen)) == 2                                             # the replays had different answers


# ------------------------------------------------------------------------------------------------ 5. argument errors
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_argument_errors_return_einval_and_launch_nothing(dev, form):
    raw = _Raw(dev, form, 2, 6, 2)
    nan, inf = float("nan"), float("inf")
    bad = [dict(G=0), dict(G=-2), dict(group_rows=0), dict(group_rows=-1), dict(group_rows=4097), dict(h=0), dict(h=65),
           dict(G=(1 << 20) // 6 + 1), dict(G=(1 << 20) + 1, group_rows=1),
           dict(radius2=0.0), dict(radius2=-1.0), dict(radius2=nan), dict(radius2=inf),
           dict(shrink=-0.5), dict(shrink=nan), dict(shrink=inf),
           dict(src=None), dict(scores=None), dict(dim_scale=None), dict(smoothed_out=None)]
    if form == "tokens":
        bad += [dict(n_stride=13), dict(n_stride=0), dict(centers=None), dict(n_centers=0), dict(n_centers=-1)]
    fn = L.lib().cover_smooth_scores_tokens if form == "tokens" else L.lib().cover_smooth_scores_actions
    for over in bad:
        assert raw.call(**over) == -1, over                                # COVER_EINVAL
        assert "smooth_scores" in L.lib().cover_last_error().decode()
    assert fn(None, torch.cuda.current_stream().cuda_stream) == -1
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # nothing was launched
    assert raw.call(shrink=0.0, radius=1e-3) == 0                          # and the plain call is none
    torch.cuda.synchronize()
    assert raw.sentinels() == ALL_STORED
    # a scale the host wrappers refuse, on the device: every pair weight is 0, the launch reports nothing
    for v in (-1.0, nan, inf):
        raw.fill()
        raw.dim_scale.copy_(torch.tensor([1.0, 1.0, v, 1.0, 1.0, 1.0]))
        assert raw.call(radius=10.0) == 0                                  # identical rows: without the rule all 6 would be neighbours
        torch.cuda.synchronize()
        assert raw.sentinels() == ALL_STORED and (raw.neighbours == 1).all(), v
        assert np.array_equal(_bits(raw.smoothed), _bits(raw.scores))
    raw.dim_scale.copy_(torch.tensor(SR.DIM_SCALE))
    assert raw.call(radius=10.0) == 0
    torch.cuda.synchronize()
    assert (raw.neighbours == 6).all()


# ------------------------------------------------------------------------------------------------ 6. end to end
def _same_dict(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


@pytest.fixture(scope="module")
def verifier_case(dev):
    """The tiny synthetic verifier over P * S = 3 * 8 candidate histories on the device, the histories of a group made neighbours."""
    from tests.test_prior_select_gpu import _verifier
    P, S = 3, 8
    ver, its, hists = _verifier(dev, P * S)
    hb = ver._pad_histories(hists)
    for g in range(P):                                                     # rows of a group: the group's first history plus a small jitter
        hb[g * S:(g + 1) * S] = hb[g * S] + torch.from_numpy(np.random.default_rng(g).uniform(-0.01, 0.01, (S, 10, 7)).astype(np.float32))
    pad = torch.zeros(P * S, 10, dtype=torch.uint8, device=dev)
    return ver, its, hb.to(dev).contiguous(), pad, P, S, host.Smooth(0.12, SR.DIM_SCALE, shrink=0.5, split_gripper=False)


def test_score_histories_without_smooth_is_unchanged(dev, verifier_case):
    ver, its, hb, pad, P, S, smooth = verifier_case
    a, b = ver.score_histories(its, hb, S, pad=pad), ver.score_histories(its, hb, S, pad=pad, smooth=None)
    assert set(a) == {"scores", "result", "best", "its", "acts", "fused_it", "fused_act"}
    _same_dict(a, b, "smooth=None")
    on = ver.score_histories(its, hb, S, pad=pad, smooth=smooth)
    assert set(on) == set(a) | {"smoothed", "density", "neighbours", "smooth_group_mean"}
    assert np.array_equal(_bits(on["scores"]), _bits(a["scores"]))


def test_score_histories_smooths_its_base(dev, verifier_case):
    ver, its, hb, pad, P, S, smooth = verifier_case
    kw = smooth.kwargs(dev)
    out = ver.score_histories(its, hb, S, pad=pad, smooth=smooth)
    want, st = ops.smooth_scores_actions(hb, out["scores"], S, stats=True, **kw)
    assert int(st.neighbours.max()) > 1                                    # not a vacuous smoothing
    _same_dict(dict(smoothed=out["smoothed"], density=out["density"], neighbours=out["neighbours"], gm=out["smooth_group_mean"]),
               dict(smoothed=want, density=st.density, neighbours=st.neighbours, gm=st.group_mean), "plain")
    ref = SR.reference(hb.cpu().numpy(), out["scores"].cpu().numpy(), S, smooth.dim_scale, smooth.radius, smooth.shrink, 0)
    assert np.array_equal(_bits(out["smoothed"]), _bits(ref["smoothed"])) and np.array_equal(_bits(out["neighbours"]), ref["neighbours"])
    result, best = ops.group_argmax(want, S)
    assert torch.equal(out["result"], result) and np.array_equal(_bits(out["best"]), _bits(best))
    # with member_kappa the base is robust
    out = ver.score_histories(its, hb, S, pad=pad, smooth=smooth, member_kappa=0.7)
    want = ops.smooth_scores_actions(hb, out["robust"], S, **kw)
    assert np.array_equal(_bits(out["smoothed"]), _bits(want)) and not np.array_equal(_bits(out["robust"]), _bits(out["scores"]))
    result, best = ops.group_argmax(want, S)
    assert torch.equal(out["result"], result) and np.array_equal(_bits(out["best"]), _bits(best))
    # with a prior: combined = smoothed + beta * prior through prior_select
    prior = torch.from_numpy(np.random.default_rng(3).normal(size=P * S).astype(np.float32)).to(dev)
    out = ver.score_histories(its, hb, S, pad=pad, smooth=smooth, prior=prior, prior_beta=0.25, top_m=2)
    sel = ops.prior_select(out["smoothed"], prior, S, 0.25, top_m=2)
    assert np.array_equal(_bits(out["smoothed"]), _bits(ops.smooth_scores_actions(hb, out["scores"], S, **kw)))
    _same_dict({k: out[k] for k in sel}, sel, "prior")
    with np.errstate(all="ignore"):
        comb = out["smoothed"].cpu().numpy() + F32(0.25) * prior.cpu().numpy()
    assert np.array_equal(_bits(out["combined"]), _bits(comb.astype(F32)))
    with pytest.raises(L.CoverError, match="host.Smooth"):
        ver.score_histories(its, hb, S, pad=pad, smooth=dict(radius=0.1))


def test_constructed_decision_flips_on_the_device(dev):
    d = SR.constructed_decision()
    x, s = torch.from_numpy(d["actions"]).to(dev), torch.from_numpy(d["scores"]).to(dev)
    raw_pick = ops.group_argmax(s, 12)[0]
    sm, st = ops.smooth_scores_actions(x, s, 12, radius=d["radius"], dim_scale=d["dim_scale"], shrink=d["shrink"], split_gripper=True, stats=True)
    pick = ops.group_argmax(sm, 12)[0]
    assert int(raw_pick[0]) == 8 and int(pick[0]) < 8
    _assert_same(dict(smoothed=sm, density=st.density, neighbours=st.neighbours, group_mean=st.group_mean),
                 SR.reference(d["actions"], d["scores"], 12, d["dim_scale"], d["radius"], d["shrink"], 1), "constructed")


def test_openvla_smooth_scores_is_the_ops_call(dev):
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_topn_gpu import _ov_case
    P, n, K0 = 2, 4, 12
    S = n + K0
    c, sd, frame, toks, lens, u = _ov_case(P=P, n_samples=n)
    policy = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    tokens = policy.sample(frame.to(dev), toks.to(dev), lens.to(dev), n, u.to(dev), 0.9, top_k=50, top_p=0.9)[0]
    aug = policy.augment(tokens, n, K0, host.augmentation_normals(P, K0, policy.n_gen // 7, seed=3).to(dev), sigma=1.5, sd_floor=0.01)
    scores = torch.from_numpy(np.random.default_rng(4).normal(size=P * S).astype(np.float32)).to(dev)
    smooth = host.Smooth(0.2, SR.DIM_SCALE, shrink=0.5)
    got, st = policy.smooth_scores(aug, scores, S, smooth, stats=True)
    want, wst = ops.smooth_scores_tokens(aug, scores, S, policy.bin_centers(), c["tok_vocab"], steps=policy.n_gen // 7, radius=0.2,
                                         dim_scale=list(SR.DIM_SCALE), shrink=0.5, split_gripper=True, stats=True)
    assert np.array_equal(_bits(got), _bits(want)) and torch.equal(st.neighbours, wst.neighbours) and tuple(got.shape) == (P * S,)
    assert np.array_equal(_bits(policy.smooth_scores(aug, scores, S, smooth)), _bits(want))
    x = SR.detokenise(aug.cpu().numpy(), policy.bin_centers().cpu().numpy(), policy.n_gen // 7, c["tok_vocab"])
    ref = SR.reference(x, scores.cpu().numpy(), S, SR.DIM_SCALE, 0.2, 0.5, 1)
    assert np.array_equal(_bits(got), _bits(ref["smoothed"])) and np.array_equal(st.neighbours.cpu().numpy(), ref["neighbours"])
    assert smooth.scale_on(dev) is smooth.scale_on(dev)                    # one upload per device


def test_score_refined_refines_on_smoothed(dev):
    from tests.test_prior_select_gpu import _verifier
    P, S, m, K = 3, 20, 4, 12
    ver, its, _ = _verifier(dev, P * S)
    rng = np.random.default_rng(11)
    b = rng.integers(100, 110, (P * S, 7))                                 # a few bins wide: the rows are neighbours
    cands = torch.from_numpy((SR.TOK_VOCAB - 1 - b).astype(np.int64)).to(dev)
    cen = torch.from_numpy(AR.openvla_centers()).to(dev)
    past = torch.from_numpy((rng.normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)
    to_hist = lambda t: ops.tokens_to_histories(t, SR.TOK_VOCAB, cen, past)
    seen = []

    def refine(t, v, S_, m_, z):
        seen.append(v)
        return ops.refine_tokens(t, v, S_, m_, z.shape[1], z, cen, SR.TOK_VOCAB, sigma=0.8, sd_floor=0.01, elites=True)
    smooth = host.Smooth(0.1, SR.DIM_SCALE, shrink=0.5)
    z = host.augmentation_normals(P, K, 1, seed=20).to(dev)
    got = ver.score_refined(its, cands, S, to_histories=to_hist, refine=refine, normals=[z], n_elite=m, smooth=smooth)
    hb, pad = to_hist(cands)
    r0 = ver.score_histories(its, hb, S, pad=pad, smooth=smooth)
    assert len(seen) == 1 and np.array_equal(_bits(seen[0]), _bits(r0["smoothed"]))
    assert int(r0["neighbours"].max()) > 1 and not np.array_equal(_bits(r0["smoothed"]), _bits(r0["scores"]))
    t1 = ops.refine_tokens(cands, r0["smoothed"], S, m, K, z, cen, SR.TOK_VOCAB, sigma=0.8, sd_floor=0.01)
    assert torch.equal(got["candidates"], t1) and "smoothed" in got and tuple(got["smoothed"].shape) == (P * (m + K),)
    hb1, pad1 = to_hist(t1)
    _same_dict({k: v for k, v in got.items() if k not in ("candidates", "rounds")}, ver.score_histories(its, hb1, m + K, pad=pad1, smooth=smooth),
               "last round")
