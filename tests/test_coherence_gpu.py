"""The chunk-coherence prior on the GPU: cover_coherence_prior_tokens / cover_coherence_prior_actions against the reference of
tests/coherence_ref.py, bit for bit (every rounding is specified, so there is no tolerance), special values as bit patterns, every output
cell stored and nothing outside the views read, graph replay, argument errors of the C entries, and the layers above them end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, host, ops
from cover_vla_amd import _lib as L
from tests import augment_ref as AR
from tests import coherence_ref as CR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("prior", "min_dist", "nearest")
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
    """The candidates as the device sees them: tokens through the table's row stride (beyond 7 h at every other shape), actions through
    the strides (chunk * 32, 32, 1) of a [N, chunk, 32] buffer at the strided shape; the cells outside the view hold junk."""
    h = shape[3]
    rng = np.random.default_rng(junk)
    if form == "tokens":
        tok = inp["tokens"]
        ld = CR.token_row_stride(shape)
        buf = rng.integers(CR.TOK_VOCAB - 256, CR.TOK_VOCAB, (tok.shape[0], ld)).astype(np.int64)
        buf[:, :7 * h] = tok
        view = torch.from_numpy(buf).to(dev)[:, :7 * h]
        assert view.stride(0) == ld or tok.shape[0] == 1
        return view
    x = inp["actions"]
    if shape == CR.STRIDED:
        chunk = h + 2
        buf = rng.uniform(-1, 1, (x.shape[0], chunk, 32)).astype(np.float32)
        buf[:, :h, :7] = x
        view = torch.from_numpy(buf).to(dev)[:, :h, :7]
        assert view.stride() == (chunk * 32, 32, 1)
        return view
    return torch.from_numpy(x).to(dev)


def _prior(form, src, S, ref, weight, centers, h, **kw):
    if form == "tokens":
        return ops.coherence_prior_tokens(src, S, ref, weight, centers, CR.TOK_VOCAB, steps=h, **kw)
    return ops.coherence_prior_actions(src, S, ref, weight, **kw)


def _run(form, shape, inp, dev, junk=1, stats=True, **over):
    src = _laid_out(form, shape, inp, dev, junk)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(over.get(k, inp[k]))).to(dev)
    dim_scale = over.get("dim_scale", inp["dim_scale"])
    out = _prior(form, src, inp["S"], t("ref"), t("weight"), t("centers"), shape[3], shift=inp["shift"], step_weight=t("step_weight"),
                 dim_scale=dim_scale.to(dev) if torch.is_tensor(dim_scale) else dim_scale, gripper_penalty=inp["penalty"], stats=stats)
    if not stats:
        return dict(prior=out)
    return dict(prior=out[0], min_dist=out[1].min_dist, nearest=out[1].nearest)


def _run_case(c, dev, junk=1, stats=True):
    return _run(c["form"], c["shape"], CR.make_inputs(c), dev, junk, stats)


# ------------------------------------------------------------------------------------------------ 1. every case of the table
def _shape_params():
    return [(f, s) for f in ("tokens", "actions") for s in CR.shapes_of(f)]


@pytest.mark.parametrize("form,shape", _shape_params(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_matches_reference_bit_for_bit(dev, form, shape):
    cs = CR.cases(forms=(form,), shapes=(shape,))
    assert len(cs) == 4                                                    # shared / per-group references x gripper_penalty in {0, 0.25}
    for c in cs:
        want = CR.case_reference(c)
        _assert_same(_run_case(c, dev), want, CR.case_id(c))
        _assert_same(_run_case(c, dev, stats=False), want, CR.case_id(c), keys=("prior",))   # the optional outputs NULL: the same bits


def test_cells_outside_the_views_are_not_read(dev):
    for c in (dict(form="tokens", shape=(3, 17, 1, 4, 6, 2), per_group=1, penalty=0.25), dict(form="actions", shape=CR.STRIDED, per_group=0, penalty=0.25),
              dict(form="tokens", shape=(2, 16, 64, 8, 8, 0), per_group=0, penalty=0.0)):
        assert c["form"] == "actions" or CR.token_row_stride(c["shape"]) > 7 * c["shape"][3]
        a, b = _run_case(c, dev, junk=1), _run_case(c, dev, junk=2)
        _assert_same(a, b, CR.case_id(c))
        _assert_same(a, CR.case_reference(c), CR.case_id(c))
    # the reference steps outside the overlap are NaN in every case of the table; here they are finite junk instead
    c = dict(form="actions", shape=(3, 17, 1, 4, 6, 2), per_group=1, penalty=0.25)
    inp = CR.make_inputs(c)
    assert np.isnan(inp["ref"][:, :, :2]).all()
    junk = np.where(np.isnan(inp["ref"]) & (np.arange(7) != CR.DIM_SCALE.index(0.0)), F32(0.5), inp["ref"])
    _assert_same(_run(c["form"], c["shape"], inp, dev, ref=junk), CR.case_reference(c), "junk outside the overlap")


# ------------------------------------------------------------------------------------------------ 2. special values
def _special_case(form):
    c = dict(form=form, shape=(2, 33, 63, 3, 3, 0), per_group=1, penalty=0.25)
    inp = CR.make_inputs(c)
    return c, inp, CR.values_of(inp, form, 3)


def _ref_of(inp, x, **over):
    v = dict(inp, **over)
    return CR.reference(x, v["ref"], v["weight"], v["S"], v["shift"], v["step_weight"], v["dim_scale"], v["penalty"])


def test_nan_candidate_element_isolates_its_own_row(dev):
    c, inp, x = _special_case("actions")
    clean = CR.case_reference(c)
    bad = dict(inp, actions=inp["actions"].copy())
    bad["actions"][[5, 40], [0, 2], [1, 4]] = np.nan
    got = _run("actions", c["shape"], bad, dev)
    _assert_same(got, _ref_of(bad, bad["actions"]), "nan element")
    p = _bits(got["prior"])
    assert (p[[5, 40]] == 0x7FC00000).all() and (got["nearest"].cpu().numpy()[[5, 40]] == -1).all()
    assert np.isposinf(got["min_dist"].cpu().numpy()[[5, 40]]).all()
    rest = np.setdiff1d(np.arange(66), [5, 40])
    for k in KEYS:
        assert np.array_equal(_bits(got[k])[rest], _bits(clean[k])[rest]), k


@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_nan_in_a_reference(dev, form):
    c, inp, x = _special_case(form)
    w = inp["weight"]
    zeros = np.argwhere(w == 0)
    assert len(zeros) >= 2
    # in references of weight 0: nothing changes
    ref = inp["ref"].copy()
    for g, r in zeros:
        ref[g, r] = np.nan
    _assert_same(_run(form, c["shape"], inp, dev, ref=ref), CR.case_reference(c), "zero-weight NaN reference")
    # in a weighted reference of group 1: every row of that group has the one NaN, nearest skips the reference, group 0 is untouched
    r_bad = int(np.flatnonzero(w[1] != 0)[3])
    ref = inp["ref"].copy()
    ref[1, r_bad, 1, 0] = np.nan
    got = _run(form, c["shape"], inp, dev, ref=ref)
    _assert_same(got, _ref_of(inp, x, ref=ref), "weighted NaN reference")
    assert (_bits(got["prior"])[33:] == 0x7FC00000).all() and (got["nearest"].cpu().numpy()[33:] != r_bad).all()
    assert np.isfinite(got["min_dist"].cpu().numpy()).all()
    assert np.array_equal(_bits(got["prior"])[:33], _bits(CR.case_reference(c)["prior"])[:33])
    # shared by all groups: every row of the launch
    cs = dict(c, per_group=0)
    inps = CR.make_inputs(cs)
    ref = inps["ref"].copy()
    ref[int(np.flatnonzero(inps["weight"] != 0)[3]), 1, 0] = np.nan
    got = _run(form, c["shape"], inps, dev, ref=ref)
    _assert_same(got, _ref_of(inps, x, ref=ref), "shared weighted NaN reference")
    assert (_bits(got["prior"]) == 0x7FC00000).all()


def test_unusable_dim_scale_gives_every_row_nan_and_reports_nothing(dev):
    c, inp, x = _special_case("actions")
    for v in (-1.0, float("nan"), float("inf")):
        scale = torch.tensor([1.0, 1.0, 0.0, v, 0.5, 0.25])                # a device tensor is taken as it is
        got = _run("actions", c["shape"], inp, dev, dim_scale=scale)
        assert (_bits(got["prior"]) == 0x7FC00000).all() and (got["nearest"] == -1).all() and bool(torch.isposinf(got["min_dist"]).all()), v
        _assert_same(got, _ref_of(inp, x, dim_scale=scale.numpy()), f"scale {v}")


def test_candidate_equal_to_its_only_reference_stores_minus_zero(dev):
    x = torch.from_numpy(np.random.default_rng(0).uniform(-1, 1, (1, 4, 7)).astype(F32)).to(dev)
    coh = host.Coherence((1.0,) * 6, 0.5, 0.25)
    p, st = ops.coherence_prior_actions(x, 1, x.clone(), torch.ones(1, device=dev), stats=True, **coh.kwargs(dev, 4))
    assert _bits(p).view(np.uint32)[0] == 0x80000000 and float(st.min_dist[0]) == 0.0 and int(st.nearest[0]) == 0
    none = ops.coherence_prior_actions(x, 1, x.clone(), torch.zeros(1, device=dev), stats=True, **coh.kwargs(dev, 4))
    assert _bits(none[0]).view(np.uint32)[0] == 0x80000000 and int(none[1].nearest[0]) == -1 and bool(torch.isposinf(none[1].min_dist[0]))


# ------------------------------------------------------------------------------------------------ the C entry over caller-owned buffers
class _Raw:
    """One form of the C entry over preallocated, sentinel-filled buffers (contiguous input, one reference set per group)."""

    def __init__(self, dev, form, G, S, R, h, hr, shift):
        self.form, self.G, self.S, self.R, self.h, self.hr, self.shift = form, G, S, R, h, hr, shift
        if form == "tokens":
            self.src = torch.full((G * S, 7 * h), CR.TOK_VOCAB - 128, dtype=torch.int64, device=dev)
        else:
            self.src = torch.zeros(G * S, h, 7, device=dev)
        self.ref = torch.zeros(G, R, hr, 7, device=dev)
        self.weight = torch.ones(G, R, device=dev)
        self.step_weight = torch.from_numpy(CR.step_weights(h)).to(dev)
        self.dim_scale = torch.tensor(CR.DIM_SCALE, dtype=torch.float32, device=dev)
        self.centers = torch.from_numpy(AR.openvla_centers()).to(dev)
        self.prior, self.min_dist = torch.empty(G * S, device=dev), torch.empty(G * S, device=dev)
        self.nearest = torch.empty(G * S, dtype=torch.int32, device=dev)
        self.fill()

    def outputs(self):
        return dict(prior=self.prior, min_dist=self.min_dist, nearest=self.nearest)

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
        self.ref.copy_(torch.from_numpy(inp["ref"]))
        self.weight.copy_(torch.from_numpy(inp["weight"]))

    def args(self, penalty=0.0, **over):
        a = L.CoherenceArgs()
        a.src, a.ref, a.ref_weight = self.src.data_ptr(), self.ref.data_ptr(), self.weight.data_ptr()
        a.step_weight, a.dim_scale = self.step_weight.data_ptr(), self.dim_scale.data_ptr()
        a.n_stride, a.t_stride = self.src.stride(0), (7 if self.form == "tokens" else self.src.stride(1))
        if self.form == "tokens":
            a.centers, a.n_centers, a.tok_vocab = self.centers.data_ptr(), self.centers.numel(), CR.TOK_VOCAB
        a.ref_g_stride, a.ref_r_stride, a.w_g_stride = self.R * self.hr * 7, self.hr * 7, self.R
        a.G, a.group_rows, a.h, a.R, a.hr, a.shift, a.gripper_penalty = self.G, self.S, self.h, self.R, self.hr, self.shift, penalty
        a.prior_out, a.min_dist_out, a.nearest_out = self.prior.data_ptr(), self.min_dist.data_ptr(), self.nearest.data_ptr()
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, **kw):
        a = self.args(**kw)
        fn = L.lib().cover_coherence_prior_tokens if self.form == "tokens" else L.lib().cover_coherence_prior_actions
        return fn(C.byref(a), torch.cuda.current_stream().cuda_stream)


ALL_STORED = dict(prior=0, min_dist=0, nearest=0)


# ------------------------------------------------------------------------------------------------ 3. stores
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_every_output_cell_is_stored(dev, form):
    for shape in ((3, 17, 1, 4, 6, 2), (2, 33, 63, 3, 3, 0), (1, 1, 1, 1, 1, 0), (1, 15, 65, 8, 9, 8)):
        c = dict(form=form, shape=shape, per_group=1, penalty=0.25)
        raw = _Raw(dev, form, *shape)
        raw.load(CR.make_inputs(c))
        assert raw.call(penalty=0.25) == 0
        torch.cuda.synchronize()
        assert raw.sentinels() == ALL_STORED, CR.case_id(c)
        _assert_same(raw.outputs(), CR.case_reference(c), CR.case_id(c))
        # either optional output left out: nothing is written to it, and the others are what they were
        for off in (dict(min_dist_out=None), dict(nearest_out=None), dict(min_dist_out=None, nearest_out=None)):
            raw.fill()
            assert raw.call(penalty=0.25, **off) == 0
            torch.cuda.synchronize()
            s = raw.sentinels()
            kept = [k for k in KEYS if f"{k}_out" not in off]
            assert all(s[k] == (0 if k in kept else getattr(raw, k).numel()) for k in KEYS), (CR.case_id(c), off)
            _assert_same(raw.outputs(), CR.case_reference(c), CR.case_id(c), keys=kept)


# ------------------------------------------------------------------------------------------------ 4. graph replay
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_graph_replay_follows_the_references_overwritten_in_place(dev, form):
    shape = (2, 33, 63, 3, 3, 0)
    raw = _Raw(dev, form, *shape)
    g, rc = graphs.capture(lambda: raw.call(penalty=0.25), dev)
    assert rc == 0
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # the capture itself executed nothing
    seen = []
    base = CR.make_inputs(dict(form=form, shape=shape, per_group=1, penalty=0.25))
    for k in range(2):
        inp = dict(base, ref=np.roll(base["ref"], 5 * k, axis=1) + F32(0.125 * k), weight=np.roll(base["weight"], 3 * k, axis=1))
        raw.load(inp)                                                      # the references and weights overwritten in place
        raw.fill()
        g.launch()
        torch.cuda.synchronize()
        replayed = {n: t.clone() for n, t in raw.outputs().items()}
        raw.fill()
        assert raw.call(penalty=0.25) == 0                                 # the eager launch on the same buffers
        torch.cuda.synchronize()
        _assert_same(replayed, raw.outputs(), f"replay {k}")
        _assert_same(replayed, CR.reference_of(inp, form, 3), f"replay {k} vs reference")
        seen.append(_bits(replayed["prior"]).tobytes())
    assert len(set(seen)) == 2                                             # the replays had different answers


# ------------------------------------------------------------------------------------------------ 5. argument errors
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_argument_errors_return_einval_and_launch_nothing(dev, form):
    raw = _Raw(dev, form, 2, 6, 3, 2, 4, 1)                                # ref_r_stride = 28, ref_g_stride = 84, w_g_stride = 3
    nan, inf = float("nan"), float("inf")
    bad = [dict(G=0), dict(G=-2), dict(group_rows=0), dict(group_rows=-1), dict(group_rows=4097), dict(R=0), dict(R=-1), dict(R=4097),
           dict(h=0), dict(h=65), dict(hr=0), dict(hr=65), dict(hr=-1), dict(shift=-1), dict(shift=4), dict(shift=5),
           dict(G=(1 << 20) // 6 + 1), dict(G=(1 << 20) + 1, group_rows=1),
           dict(ref_g_stride=83), dict(ref_g_stride=27), dict(ref_g_stride=-84), dict(ref_g_stride=1, R=1, w_g_stride=1),
           dict(ref_r_stride=27), dict(ref_r_stride=0), dict(ref_r_stride=-28), dict(ref_r_stride=29),   # (R - 1) * 29 + 28 > 84
           dict(ref_r_stride=(1 << 62)), dict(w_g_stride=2), dict(w_g_stride=-3), dict(w_g_stride=4),
           dict(gripper_penalty=-0.5), dict(gripper_penalty=nan), dict(gripper_penalty=inf),
           dict(src=None), dict(ref=None), dict(ref_weight=None), dict(step_weight=None), dict(dim_scale=None), dict(prior_out=None)]
    if form == "tokens":
        bad += [dict(n_stride=13), dict(n_stride=0), dict(centers=None), dict(n_centers=0), dict(n_centers=-1)]
    fn = L.lib().cover_coherence_prior_tokens if form == "tokens" else L.lib().cover_coherence_prior_actions
    for over in bad:
        assert raw.call(**over) == -1, over                                # COVER_EINVAL
        assert "coherence_prior" in L.lib().cover_last_error().decode()
    assert fn(None, torch.cuda.current_stream().cuda_stream) == -1
    assert f"cover_coherence_prior_{form}" in L.lib().cover_last_error().decode()
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # nothing was launched
    for over in (dict(), dict(ref_g_stride=0), dict(w_g_stride=0), dict(ref_g_stride=0, w_g_stride=0), dict(shift=3), dict(shift=0),
                 dict(gripper_penalty=3.0e38)):                            # and these are none
        raw.fill()
        assert raw.call(**over) == 0, over
        torch.cuda.synchronize()
        assert raw.sentinels() == ALL_STORED, over


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_openvla_coherence_prior_is_the_ops_call_and_the_forward_contrast_recipe(dev):
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_topn_gpu import _ov_case
    P, n, K0 = 2, 4, 12
    S = n + K0
    c, sd, frame, toks, lens, u = _ov_case(P=P, n_samples=n)
    policy = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    tokens = policy.sample(frame.to(dev), toks.to(dev), lens.to(dev), n, u.to(dev), 0.9, top_k=50, top_p=0.9)[0]
    aug = policy.augment(tokens, n, K0, host.augmentation_normals(P, K0, policy.n_gen // 7, seed=3).to(dev), sigma=1.5, sd_floor=0.01)
    h = policy.n_gen // 7
    cen = policy.bin_centers()
    coh = host.Coherence(CR.DIM_SCALE, 0.8, 0.25)
    x = CR.detokenise(aug.cpu().numpy(), cen.cpu().numpy(), h, c["tok_vocab"])
    sw = CR.step_weights(h, 0.8)
    # backward coherence: one committed chunk, given as tokens (out of the vocabulary's action range at one end: the clamp rule)
    committed = aug[3:4].clone()
    committed[0, 0], committed[0, 1] = c["tok_vocab"] + 5, 0
    got, st = policy.coherence_prior(aug, S, coh, ref_tokens=committed, stats=True)
    y = CR.detokenise(committed.cpu().numpy(), cen.cpu().numpy(), h, c["tok_vocab"])
    want, wst = ops.coherence_prior_tokens(aug, S, torch.from_numpy(y).to(dev), torch.ones(1, device=dev), cen, c["tok_vocab"], steps=h,
                                           stats=True, **coh.kwargs(dev, h))
    assert tuple(got.shape) == (P * S,) and np.array_equal(_bits(got), _bits(want)) and torch.equal(st.nearest, wst.nearest)
    ref = CR.reference(x, y, np.ones(1, F32), S, 0, sw, CR.DIM_SCALE, 0.25)
    _assert_same(dict(prior=got, min_dist=st.min_dist, nearest=st.nearest), ref, "backward coherence")
    assert np.array_equal(_bits(policy.coherence_prior(aug, S, coh, ref_actions=torch.from_numpy(y).to(dev))), _bits(got))
    assert coh.scale_on(dev) is coh.scale_on(dev) and coh.steps_on(dev, h) is coh.steps_on(dev, h)   # one upload per device
    # forward contrast: the group's own rows at +1/S, a weak policy's rows (here: other draws) at -1/S', one reference set per prompt
    Sw = 5
    weak = policy.augment(tokens, n, Sw - n, host.augmentation_normals(P, Sw - n, h, seed=8).to(dev), sigma=4.0, sd_floor=0.05)
    refs = torch.cat([aug.view(P, S, 7 * h), weak.view(P, Sw, 7 * h)], dim=1)               # [P, S + S', 7 h]
    w = torch.cat([torch.full((S,), 1.0 / S), torch.full((Sw,), -1.0 / Sw)]).to(dev)
    got, st = policy.coherence_prior(aug, S, coh, ref_tokens=refs, ref_weight=w, stats=True)
    y = CR.detokenise(refs.reshape(P * (S + Sw), 7 * h).cpu().numpy(), cen.cpu().numpy(), h, c["tok_vocab"]).reshape(P, S + Sw, h, 7)
    ref = CR.reference(x, y, w.cpu().numpy(), S, 0, sw, CR.DIM_SCALE, 0.25)
    _assert_same(dict(prior=got, min_dist=st.min_dist, nearest=st.nearest), ref, "forward contrast")
    assert (st.min_dist == 0).all()                                        # every row is among its own references
    per_group_w = policy.coherence_prior(aug, S, coh, ref_tokens=refs, ref_weight=w.repeat(P, 1).contiguous())
    assert np.array_equal(_bits(per_group_w), _bits(got))


def test_score_histories_takes_the_coherence_prior(dev):
    from tests import prior_ref as PR
    from tests.test_prior_select_gpu import _verifier
    P, S, h = 3, 8, 1
    ver, its, hists = _verifier(dev, P * S)
    hb = ver._pad_histories(hists).to(dev).contiguous()
    pad = torch.zeros(P * S, 10, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(6)
    acts = rng.uniform(-1, 1, (P * S, h, 7)).astype(F32)
    ref = rng.uniform(-1, 1, (2, h, 7)).astype(F32)
    w = np.array([1.0, -0.5], dtype=F32)
    coh = host.Coherence(CR.DIM_SCALE, 0.8, 0.25)
    prior = ops.coherence_prior_actions(torch.from_numpy(acts).to(dev), S, torch.from_numpy(ref).to(dev), torch.from_numpy(w).to(dev),
                                        **coh.kwargs(dev, h))
    want = CR.reference(acts, ref, w, S, 0, CR.step_weights(h, 0.8), CR.DIM_SCALE, 0.25)["prior"]
    assert np.array_equal(_bits(prior), _bits(want))
    for beta in (0.25, 2.0):
        r = ver.score_histories(its, hb, S, pad=pad, prior=prior, prior_beta=beta)
        sel = PR.reference(r["scores"].cpu().numpy(), want, None, None, S, beta, False, 1)   # the reference prior, not the device's
        assert np.array_equal(_bits(r["result"]), sel["result"]) and np.array_equal(_bits(r["combined"]), _bits(sel["combined"]))
    plain = ver.score_histories(its, hb, S, pad=pad)
    assert "combined" not in plain


def _pi0_policy(model, tiny, steps, Lmax, **kw):
    from cover_vla_amd.pi0 import PI0Config, PI0Policy
    from tests.episode_replay import WordTokenizer
    return PI0Policy(PI0Config(n_action_steps=steps, chunk_size=tiny["chunk"], tokenizer_max_length=Lmax, resize_imgs_with_padding=None), model,
                     WordTokenizer(tiny["vocab"]).policy, **kw)


def test_pi0_commit_and_coherence_prior(dev):
    from cover_vla_amd.pi0 import PI0FlowMatching
    from tests.episode_replay import scripted_inputs
    from tests.helpers import pi0_case
    _, tiny, sd, _ = pi0_case(os.path.join(ROOT, "tests", "golden", "pi0_tiny_b6.npz"))
    G, n, K, steps, Lmax = 2, 3, 5, 2, 12
    chunk, B, S = tiny["chunk"], G * n, n + K
    assert chunk > steps
    model = PI0FlowMatching(sd, tiny, device="cuda:0", max_batch=8, max_prompts=8, max_lang=Lmax)
    mean = torch.linspace(-0.2, 0.2, 7)
    std = torch.linspace(0.5, 1.5, 7)
    pol = _pi0_policy(model, tiny, steps, Lmax, action_mean=mean, action_std=std)
    full = _pi0_policy(model, tiny, chunk, Lmax)                           # no normalisation, the whole chunk: the normalised rows
    plain = _pi0_policy(model, tiny, steps, Lmax)                          # no normalisation, the executed steps
    obs = scripted_inputs(2, B, chunk, tiny["image"], seed=21)
    tasks = [t for t in ("put the spoon on the towel", "move the spoon to the cloth") for _ in range(n)]
    batch = lambda o: {"observation.images.top": o["frame"].repeat(B, 1, 1, 1).to(dev), "observation.state": o["state"].repeat(B, 1).to(dev),
                       "task": tasks}

    def rows(p, o, **kw):
        q = p.select_action(batch(o), noise=o["noise"].to(dev), **kw)
        out = torch.stack([a.clone() for a in q], dim=1)
        q.clear()
        return out
    chunks0, chunks1 = rows(full, obs[0]), rows(full, obs[1])             # [B, chunk, 7], normalised
    coh = host.Coherence(CR.DIM_SCALE, 0.8, 0.25)
    sw = CR.step_weights(steps, 0.8)

    # coherence = None: nothing is kept, with or without a committed tail
    assert pol.coherence is None and pol.committed_tail is None and pol.last_coherence_prior is None
    with pytest.raises(L.CoverError, match="no sampled batch"):
        pol.commit(0)
    first = rows(pol, obs[0])
    assert np.array_equal(_bits(first), _bits(chunks0[:, :steps] * std.to(dev) + mean.to(dev)))
    tail = pol.commit(4)
    assert pol.last_coherence_prior is None and tail is pol.committed_tail
    assert tuple(tail.shape) == (1, chunk - steps, 7) and tail.dtype == torch.float32 and tail.is_cuda
    assert np.array_equal(_bits(tail[0]), _bits(chunks0[4, steps:]))       # the normalised steps beyond the executed ones
    rows(pol, obs[1])
    assert pol.last_coherence_prior is None                                # coherence is None: nothing launched
    for bad in (-1, B, 1.0, True):
        with pytest.raises(L.CoverError, match="row must"):
            pol.commit(bad)

    # coherence set, no committed tail: nothing either; after commit: the prior of the next sampled batch against the tail
    pol.reset()
    assert pol.committed_tail is None
    pol.coherence = coh
    rows(pol, obs[0])
    assert pol.last_coherence_prior is None
    pol.commit(4)
    second = rows(pol, obs[1])
    assert np.array_equal(_bits(second), _bits(chunks1[:, :steps] * std.to(dev) + mean.to(dev)))   # the actions are what they were
    prior = pol.last_coherence_prior
    assert tuple(prior.shape) == (B,) and prior.dtype == torch.float32 and prior.is_cuda
    want = CR.reference(chunks1[:, :steps].cpu().numpy(), chunks0[4:5, steps:].cpu().numpy(), np.ones(1, F32), B, 0, sw, CR.DIM_SCALE, 0.25)
    assert np.array_equal(_bits(prior), _bits(want["prior"])) and bool((prior < 0).all())
    # a call that finds the queue filled leaves it alone
    q = pol.select_action(batch(obs[0]), noise=obs[0]["noise"].to(dev))
    pol.select_action(batch(obs[1]), noise=obs[1]["noise"].to(dev))
    assert pol.last_coherence_prior is not prior and len(q) == steps
    kept = pol.last_coherence_prior
    pol.select_action(batch(obs[1]), noise=obs[1]["noise"].to(dev))
    assert pol.last_coherence_prior is kept
    q.clear()

    # with augment=: the prior covers the augmented rows, on the normalised view; an augmented row cannot be committed
    z = host.augmentation_normals(G, K, steps, seed=5)
    aug = host.Augment(n, K, z.to(dev), sigma=0.8, sd_floor=0.0, clip=(-float("inf"), float("inf")))
    norm_aug = rows(plain, obs[1], augment=aug)                            # [G * S, steps, 7], normalised
    rows(pol, obs[1], augment=aug)
    want = CR.reference(norm_aug.cpu().numpy(), chunks0[4:5, steps:].cpu().numpy(), np.ones(1, F32), G * S, 0, sw, CR.DIM_SCALE, 0.25)
    assert tuple(pol.last_coherence_prior.shape) == (G * S,) and np.array_equal(_bits(pol.last_coherence_prior), _bits(want["prior"]))
    with pytest.raises(L.CoverError, match="augmented"):
        pol.commit(n)                                                      # row n of group 0 is the first augmented one
    tail = pol.commit(S + 1)                                               # group 1, sample 1 = batch row n + 1
    assert np.array_equal(_bits(tail[0]), _bits(chunks1[n + 1, steps:]))

    # reset() clears both; a wrong record is refused before the policy runs; chunk_size == n_action_steps keeps None
    pol.reset()
    assert pol.committed_tail is None and pol.last_coherence_prior is None
    pol.coherence = dict(decay=0.8)
    with pytest.raises(L.CoverError, match="host.Coherence"):
        pol.select_action(batch(obs[0]), noise=obs[0]["noise"].to(dev))
    full.coherence = coh
    rows(full, obs[0])
    assert full.commit(2) is None and full.committed_tail is None
    rows(full, obs[1])
    assert full.last_coherence_prior is None
