"""Diverse candidate subsets on the GPU: cover_diverse_subset_tokens / cover_diverse_subset_actions against the reference of
tests/diverse_ref.py, bit for bit (every rounding is specified, so there is no tolerance), every output cell stored, the cross-check with
cover_refine_* at weight 0, graph replay, argument errors of the C entries, and the layers above them end to end.

The file name sorts behind every other GPU test file on purpose: tests/test_fullsize_gpu.py::test_fullsize_pi0_profile_b40 compares the
first (eager) full-size pi0 decision of the process with the second bit for bit, and whether those agree depends on what the tests in front
of it left behind (it fails when it is run alone). New GPU tests therefore run behind it, so that it sees the sequence it always saw."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, host, ops
from cover_vla_amd import _lib as L
from tests import augment_ref as AR
from tests import diverse_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("picked", "count", "value", "dist", "assign", "row_dist")
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
    """The rows as the device sees them: tokens through the table's row stride (beyond 7 h at every other shape), actions through the
    strides (chunk * 32, 32, 1) of a [N, chunk, 32] buffer at the strided shape; the cells outside the view hold junk, NaN included."""
    h = shape[3]
    rng = np.random.default_rng(junk)
    if form == "tokens":
        tok = inp["tokens"]
        ld = DR.token_row_stride(shape)
        buf = rng.integers(DR.TOK_VOCAB - 256, DR.TOK_VOCAB, (tok.shape[0], ld)).astype(np.int64)
        buf[:, :7 * h] = tok
        view = torch.from_numpy(buf).to(dev)[:, :7 * h]
        assert view.stride(0) == ld or tok.shape[0] == 1
        return view
    x = inp["actions"]
    if shape == DR.STRIDED:
        chunk = h + 2
        buf = rng.uniform(-1, 1, (x.shape[0], chunk, 32)).astype(np.float32)
        buf[rng.random(buf.shape) < 0.2] = np.nan
        buf[:, :h, :7] = x
        view = torch.from_numpy(buf).to(dev)[:, :h, :7]
        assert view.stride() == (chunk * 32, 32, 1)
        return view
    return torch.from_numpy(x).to(dev)


def _as_dict(sub):
    return dict(picked=sub.picked, count=sub.count, value=sub.value, dist=sub.dist, assign=sub.assign, row_dist=sub.row_dist, rows=sub.rows)


def _run(form, shape, inp, dev, junk=1, **over):
    src = _laid_out(form, shape, inp, dev, junk)
    t = lambda k: torch.from_numpy(np.ascontiguousarray(over.get(k, inp[k]))).to(dev)
    dim_scale = over.get("dim_scale", inp["dim_scale"])
    kw = dict(quality=None if inp["quality"] is None else t("quality"), weight=inp["weight"], cover_dist=inp["cover"], step_weight=t("step_weight"),
              dim_scale=dim_scale.to(dev) if torch.is_tensor(dim_scale) else dim_scale, gripper_penalty=inp["penalty"])
    if form == "tokens":
        return _as_dict(ops.diverse_subset_tokens(src, inp["S"], inp["m"], t("centers"), DR.TOK_VOCAB, steps=shape[3], **kw))
    return _as_dict(ops.diverse_subset_actions(src, inp["S"], inp["m"], **kw))


def _input_rows(form, inp):
    return inp["tokens"] if form == "tokens" else inp["actions"][..., :7]


def _check_case(c, dev, junk=1):
    inp = DR.make_inputs(c)
    got, want = _run(c["form"], c["shape"], inp, dev, junk), DR.case_reference(c)
    _assert_same(got, want, DR.case_id(c))
    rows = DR.gathered(_input_rows(c["form"], inp), want["picked"], inp["S"])
    assert got["rows"].is_contiguous() and np.array_equal(_bits(got["rows"]), _bits(rows)), DR.case_id(c)   # NaN cells too: bit patterns
    return got, want


# ------------------------------------------------------------------------------------------------ 1. every case of the table
def _shape_params():
    return [(f, s) for f in ("tokens", "actions") for s in DR.shapes_of(f)]


@pytest.mark.parametrize("form,shape", _shape_params(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_matches_reference_bit_for_bit(dev, form, shape):
    cs = DR.cases(forms=(form,), shapes=(shape,))
    assert len(cs) == 8                                                    # quality given / None x weight {0, 0.5} x cover_dist {-1, 0}
    short = False
    for c in cs:
        got, want = _check_case(c, dev)
        short = short or bool((want["count"] < shape[2]).any())
    if shape[2] == shape[1] and shape[1] >= 64:
        assert short                                                       # the planted duplicates: count < m occurs


def test_dispatch_boundary_shapes_take_both_paths():
    lo, hi = DR.boundary_shapes()
    assert lo in DR.SHAPES and hi in DR.SHAPES and DR.lds_resident(*lo[1:]) and not DR.lds_resident(*hi[1:])


def test_cells_outside_the_views_are_not_read(dev):
    for c in (dict(form="tokens", shape=(3, 4, 4, 1), quality=1, weight=0.5, cover=0.0),
              dict(form="actions", shape=DR.STRIDED, quality=1, weight=0.5, cover=-1.0),
              dict(form="tokens", shape=DR.boundary_shapes()[1], quality=0, weight=0.5, cover=-1.0)):   # the rows re-read from global memory
        assert c["form"] == "actions" or DR.token_row_stride(c["shape"]) > 7 * c["shape"][3]
        a, _ = _check_case(c, dev, junk=1)
        b, _ = _check_case(c, dev, junk=2)
        _assert_same(a, b, DR.case_id(c), keys=KEYS + ("rows",))


# ------------------------------------------------------------------------------------------------ 2. special values
def test_unusable_dim_scale_gives_count_zero_and_row_zero(dev):
    c = dict(form="actions", shape=(2, 65, 9, 3), quality=1, weight=0.5, cover=-1.0)
    inp = DR.make_inputs(c)
    for v in (-1.0, float("nan"), float("inf")):
        scale = torch.tensor([1.0, 1.0, 0.0, v, 0.5, 0.25])                # a device tensor is taken as it is
        got = _run("actions", c["shape"], inp, dev, dim_scale=scale)
        want = DR.reference(inp["actions"], 65, 9, inp["quality"], 0.5, -1.0, inp["step_weight"], scale.numpy(), inp["penalty"])
        _assert_same(got, want, f"scale {v}")
        assert (got["count"] == 0).all() and (got["picked"] == -1).all() and (got["assign"] == -1).all()
        assert np.array_equal(_bits(got["rows"]), _bits(inp["actions"][[0] * 9 + [65] * 9]))


def test_nan_quality_and_nan_elements_are_never_picked(dev):
    c = dict(form="actions", shape=(2, 64, 64, 1), quality=1, weight=0.5, cover=-1.0)
    inp = DR.make_inputs(c)
    got, want = _check_case(c, dev)
    q, x = inp["quality"], inp["actions"]
    bad = np.flatnonzero(np.isnan(q) | np.isnan(x[:, :, [0, 1, 3, 4, 5]]).any(axis=(1, 2)))
    assert len(bad) >= 2 and not set(bad.tolist()) & set(got["picked"].cpu().numpy().reshape(-1).tolist())
    assert np.isnan(x[:, :, 2]).any() and np.isnan(x[:, :, 6]).any()       # the invisible ones are there
    assert (want["count"] == 64 - np.array([np.sum(bad < 64), np.sum(bad >= 64)])).all()   # and every other row is picked


# ------------------------------------------------------------------------------------------------ the C entry over caller-owned buffers
class _Raw:
    """One form of the C entry over preallocated, sentinel-filled buffers (contiguous input)."""
    OUT = {"picked": "picked_rows_out", "count": "count_out", "value": "pick_value_out", "dist": "pick_dist_out", "assign": "assign_out",
           "row_dist": "row_dist_out", "rows": "out"}

    def __init__(self, dev, form, G, S, m, h):
        self.form, self.G, self.S, self.m, self.h = form, G, S, m, h
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        if form == "tokens":
            self.src = torch.full((G * S, 7 * h), DR.TOK_VOCAB - 128, dtype=torch.int64, device=dev)
            self.rows = torch.empty(G * m, 7 * h, dtype=torch.int64, device=dev)
        else:
            self.src = torch.zeros(G * S, h, 7, device=dev)
            self.rows = torch.empty(G * m, h, 7, device=dev)
        self.quality = torch.zeros(G * S, device=dev)
        self.step_weight = torch.from_numpy(DR.step_weights(h, DR.DECAY)).to(dev)
        self.dim_scale = torch.tensor(DR.DIM_SCALE, dtype=torch.float32, device=dev)
        self.centers = torch.from_numpy(AR.openvla_centers()).to(dev)
        self.picked, self.count = torch.empty(G, m, **i32), torch.empty(G, **i32)
        self.value, self.dist = torch.empty(G, m, **f32), torch.empty(G, m, **f32)
        self.assign, self.row_dist = torch.empty(G * S, **i32), torch.empty(G * S, **f32)
        self.fill()

    def outputs(self):
        return {k: getattr(self, k) for k in self.OUT}

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
        self.src.copy_(torch.from_numpy(inp[self.form] if self.form == "tokens" else np.ascontiguousarray(inp["actions"][..., :7])))
        if inp["quality"] is not None:
            self.quality.copy_(torch.from_numpy(inp["quality"]))

    def args(self, weight=0.5, cover_dist=-1.0, gripper_penalty=DR.PENALTY, **over):
        a = L.DiverseArgs()
        a.src, a.quality, a.step_weight, a.dim_scale = self.src.data_ptr(), self.quality.data_ptr(), self.step_weight.data_ptr(), self.dim_scale.data_ptr()
        a.n_stride, a.t_stride = self.src.stride(0), (7 if self.form == "tokens" else self.src.stride(1))
        if self.form == "tokens":
            a.centers, a.n_centers, a.tok_vocab = self.centers.data_ptr(), self.centers.numel(), DR.TOK_VOCAB
        a.G, a.group_rows, a.m, a.h = self.G, self.S, self.m, self.h
        a.weight, a.cover_dist, a.gripper_penalty = weight, cover_dist, gripper_penalty
        for k, name in self.OUT.items():
            setattr(a, name, getattr(self, k).data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def call(self, **kw):
        a = self.args(**kw)
        fn = L.lib().cover_diverse_subset_tokens if self.form == "tokens" else L.lib().cover_diverse_subset_actions
        return fn(C.byref(a), torch.cuda.current_stream().cuda_stream)


ALL_STORED = dict.fromkeys(_Raw.OUT, 0)
ALL_KEYS = tuple(_Raw.OUT)


def _want_with_rows(c, inp):
    want = dict(DR.case_reference(c))
    want["rows"] = DR.gathered(_input_rows(c["form"], inp), want["picked"], inp["S"])
    return want


# ------------------------------------------------------------------------------------------------ 3. stores
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_every_output_cell_is_stored(dev, form):
    for shape, cover in (((3, 4, 4, 1), 0.0), ((2, 64, 64, 1), 0.0), ((1, 1, 1, 1), -1.0), ((2, 65, 9, 3), -1.0), (DR.boundary_shapes()[1], 0.0)):
        c = dict(form=form, shape=shape, quality=1, weight=0.5, cover=cover)
        inp = DR.make_inputs(c)
        want = _want_with_rows(c, inp)
        raw = _Raw(dev, form, *shape)
        raw.load(inp)
        assert raw.call(cover_dist=cover) == 0
        torch.cuda.synchronize()
        assert raw.sentinels() == ALL_STORED, DR.case_id(c)
        _assert_same(raw.outputs(), want, DR.case_id(c), keys=ALL_KEYS)
        # the unfilled-slot conventions
        picked, count = raw.picked.cpu().numpy(), raw.count.cpu().numpy()
        slot = np.arange(shape[2])[None, :]
        assert ((picked >= 0) == (slot < count[:, None])).all()
        assert (_bits(raw.value)[picked < 0] == 0x7FC00000).all() and np.isposinf(raw.dist.cpu().numpy()[picked < 0]).all()
        assert np.isposinf(raw.dist.cpu().numpy()[:, 0]).all()
        if shape == (2, 64, 64, 1):
            assert (count < 64).all()                                      # unfilled slots occur here
        # an optional output left out: nothing is written to it, and the others are what they were
        for off in ({"count_out": None}, {"pick_value_out": None, "pick_dist_out": None}, {"assign_out": None}, {"row_dist_out": None}, {"out": None},
                    {n: None for n in _Raw.OUT.values() if n != "picked_rows_out"}):
            raw.fill()
            assert raw.call(cover_dist=cover, **off) == 0
            torch.cuda.synchronize()
            s = raw.sentinels()
            kept = [k for k in ALL_KEYS if _Raw.OUT[k] not in off]
            assert all(s[k] == (0 if k in kept else getattr(raw, k).numel()) for k in ALL_KEYS), (DR.case_id(c), off)
            _assert_same(raw.outputs(), want, DR.case_id(c), keys=kept)
        raw.fill()
        assert raw.call(cover_dist=cover, quality=None, weight=0.0) == 0   # quality NULL: every quality is 0.0f
        torch.cuda.synchronize()
        _assert_same(raw.outputs(), _want_with_rows(dict(c, quality=0, weight=0.0), inp), "quality NULL", keys=ALL_KEYS)


# ------------------------------------------------------------------------------------------------ 4. the cross-check with refine
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_weight_zero_is_refines_top_m(dev, form):
    for shape in ((3, 4, 4, 1), (2, 65, 9, 3), (1, 1025, 1025, 1), (2, 37, 8, 50)):
        G, S, m, h = shape
        c = dict(form=form, shape=shape, quality=0, weight=0.0, cover=-1.0)
        inp = DR.make_inputs(c)
        if form == "actions":                                              # finite rows: refine gathers whatever it is given
            inp["actions"] = np.nan_to_num(inp["actions"], nan=0.25)
        scores = np.random.default_rng(7).permutation(G * S).astype(F32) / 8 - 3   # finite and distinct
        got = _run(form, shape, dict(inp, quality=scores), dev)
        src, sc = _laid_out(form, shape, inp, dev), torch.from_numpy(scores).to(dev)
        z = torch.empty(G, 0, h, 6, device=dev)
        if form == "tokens":
            out, el = ops.refine_tokens(src, sc, S, m, 0, z, torch.from_numpy(inp["centers"]).to(dev), DR.TOK_VOCAB, steps=h, elites=True)
        else:
            out, el = ops.refine_actions(src, sc, S, m, 0, z, elites=True)
        assert torch.equal(got["picked"], el.rows) and np.array_equal(_bits(got["value"]), _bits(el.scores)), shape
        assert got["rows"].shape == out.shape and np.array_equal(_bits(got["rows"]), _bits(out)), shape
        assert (got["count"] == m).all()


# ------------------------------------------------------------------------------------------------ 5. graph replay
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_graph_replay_follows_the_rows_overwritten_in_place(dev, form):
    shape = (2, 65, 9, 3)
    raw = _Raw(dev, form, *shape)
    g, rc = graphs.capture(lambda: raw.call(cover_dist=0.0), dev)
    assert rc == 0
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # the capture itself executed nothing
    seen = []
    c = dict(form=form, shape=shape, quality=1, weight=0.5, cover=0.0)
    base = DR.make_inputs(c)
    for k in range(2):
        inp = dict(base, quality=np.roll(base["quality"], 7 * k))
        inp[form] = np.roll(base[form], 3 * k, axis=0)                     # the rows and qualities overwritten in place
        raw.load(inp)
        raw.fill()
        g.launch()
        torch.cuda.synchronize()
        replayed = {n: t.clone() for n, t in raw.outputs().items()}
        raw.fill()
        assert raw.call(cover_dist=0.0) == 0                               # the eager launch on the same buffers
        torch.cuda.synchronize()
        _assert_same(replayed, raw.outputs(), f"replay {k}", keys=ALL_KEYS)
        _assert_same(replayed, DR.reference_of(inp, form, 3), f"replay {k} vs reference")
        seen.append(_bits(replayed["picked"]).tobytes())
    assert len(set(seen)) == 2                                             # the replays had different answers


# ------------------------------------------------------------------------------------------------ 6. argument errors
@pytest.mark.parametrize("form", ("tokens", "actions"))
def test_argument_errors_return_einval_and_launch_nothing(dev, form):
    raw = _Raw(dev, form, 2, 6, 3, 2)
    nan, inf = float("nan"), float("inf")
    bad = [dict(G=0), dict(G=-2), dict(group_rows=0), dict(group_rows=-1), dict(group_rows=4097, m=1), dict(group_rows=2), dict(m=0), dict(m=-1),
           dict(m=7), dict(h=0), dict(h=65), dict(h=-1), dict(G=(1 << 20) // 6 + 1), dict(G=(1 << 20) + 1, group_rows=1, m=1),
           dict(weight=-0.5), dict(weight=nan), dict(weight=inf), dict(cover_dist=nan), dict(cover_dist=inf),
           dict(gripper_penalty=-0.5), dict(gripper_penalty=nan), dict(gripper_penalty=inf),
           dict(src=None), dict(step_weight=None), dict(dim_scale=None), dict(picked_rows_out=None)]
    if form == "tokens":
        bad += [dict(n_stride=13), dict(n_stride=0), dict(centers=None), dict(n_centers=0), dict(n_centers=-1)]
    fn = L.lib().cover_diverse_subset_tokens if form == "tokens" else L.lib().cover_diverse_subset_actions
    for over in bad:
        assert raw.call(**over) == -1, over                                # COVER_EINVAL
        assert "diverse_subset" in L.lib().cover_last_error().decode()
    assert fn(None, torch.cuda.current_stream().cuda_stream) == -1
    assert f"cover_diverse_subset_{form}" in L.lib().cover_last_error().decode()
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # nothing was launched
    for over in (dict(), dict(cover_dist=-inf), dict(cover_dist=3.0e38), dict(weight=0.0), dict(weight=3.0e38), dict(gripper_penalty=0.0),
                 dict(m=1), dict(quality=None)):                           # and these are none
        raw.fill()
        assert raw.call(**over) == 0, over
        torch.cuda.synchronize()
        if "m" not in over:                                                # m = 1 fills the first cells of the m = 3 buffers only
            assert raw.sentinels() == ALL_STORED, over


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_openvla_prune_then_score_and_spread_back(dev):
    from cover_vla_amd.openvla import OpenVLA
    from tests.test_prior_select_gpu import _verifier
    from tests.test_topn_gpu import _ov_case
    P, n, K0, m = 2, 4, 12, 5
    S = n + K0
    c, sd, frame, toks, lens, u = _ov_case(P=P, n_samples=n)
    policy = OpenVLA(sd, c, device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    tokens = policy.sample(frame.to(dev), toks.to(dev), lens.to(dev), n, u.to(dev), 0.9, top_k=50, top_p=0.9)[0]
    aug = policy.augment(tokens, n, K0, host.augmentation_normals(P, K0, policy.n_gen // 7, seed=3).to(dev), sigma=1.5, sd_floor=0.01)
    h = policy.n_gen // 7
    cen = policy.bin_centers()
    div = host.Diversity(m, 0.5, DR.DIM_SCALE, 0.8, 0.25, cover_dist=0.0)
    quality = policy.proposal_prior(aug, S, n, sigma=1.0, sd_floor=0.05)
    sub = policy.diverse_subset(aug, S, div, quality=quality, steps=h)
    want = DR.reference(DR.detokenise(aug.cpu().numpy(), cen.cpu().numpy(), h, c["tok_vocab"]), S, m, quality.cpu().numpy(), 0.5, 0.0,
                        DR.step_weights(h, 0.8), DR.DIM_SCALE, 0.25)
    _assert_same(_as_dict(sub), want, "OpenVLA.diverse_subset")
    assert sub.rows.dtype == torch.int64 and tuple(sub.rows.shape) == (P * m, 7 * h) and torch.equal(sub.valid, sub.picked >= 0)
    picked = sub.picked.cpu().numpy()
    host_rows = aug.cpu()[torch.from_numpy(DR.gathered(np.arange(P * S), picked, S))].to(dev)    # the same rows gathered on the host
    assert torch.equal(sub.rows, host_rows)
    none = policy.diverse_subset(aug, S, host.Diversity(m, 0.0, DR.DIM_SCALE, 0.8, 0.25), steps=h)   # no quality, weight 0: rows 0..m-1
    assert none.picked.cpu().tolist() == [list(range(g * S, g * S + m)) for g in range(P)]
    # the verifier on the G * m kept rows, against the same rows gathered on the host: the same M, hence the same bits
    ver, its, _ = _verifier(dev, P * m)
    past = torch.from_numpy((np.random.default_rng(0).normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)

    def score(t):
        hb, pad = ops.tokens_to_histories(t, c["tok_vocab"], cen, past)
        return ver.score_histories(its, hb, m, pad=pad)
    r, rh = score(sub.rows), score(host_rows)
    assert tuple(r["scores"].shape) == (P * m,) and np.array_equal(_bits(r["scores"]), _bits(rh["scores"])) and torch.equal(r["result"], rh["result"])
    win, grp, slot = r["result"].cpu().tolist()[:3]
    assert win == grp * m + slot and picked[grp, slot] >= 0
    assert torch.equal(aug[int(picked[grp, slot])], sub.rows[win])         # the winner maps back through picked to the original row
    # spread back to the P * S input rows: the grouped arg-max names a row whose nearest pick is the best slot of its group
    full = host.spread_scores(r["scores"], sub, S)
    assert tuple(full.shape) == (P * S,) and full.is_cuda
    kept, assign = r["scores"].cpu().numpy().reshape(P, m), sub.assign.cpu().numpy()
    want_full = np.where(assign >= 0, kept[np.arange(P * S) // S, np.maximum(assign, 0)], -np.inf).astype(F32)
    assert np.array_equal(_bits(full), _bits(want_full))
    res, _ = ops.group_argmax(full, S)
    row, g2 = res.cpu().tolist()[:2]
    valid = picked[g2] >= 0
    assert assign[row] == int(np.argmax(np.where(valid, kept[g2], -np.inf)))
    assert float(full[row]) == float(np.max(kept[g2][valid]))


def _pi0_policy(model, tiny, steps, Lmax, **kw):
    from cover_vla_amd.pi0 import PI0Config, PI0Policy
    from tests.episode_replay import WordTokenizer
    return PI0Policy(PI0Config(n_action_steps=steps, chunk_size=tiny["chunk"], tokenizer_max_length=Lmax, resize_imgs_with_padding=None), model,
                     WordTokenizer(tiny["vocab"]).policy, **kw)


def test_pi0_diverse_off_path_and_gathered_queue(dev):
    from cover_vla_amd.pi0 import PI0FlowMatching
    from tests.episode_replay import scripted_inputs
    from tests.helpers import pi0_case
    _, tiny, sd, _ = pi0_case(os.path.join(ROOT, "tests", "golden", "pi0_tiny_b6.npz"))
    G, n, K, steps, Lmax, keep = 2, 3, 5, 2, 12, 3
    chunk, B, S = tiny["chunk"], G * n, n + K
    model = PI0FlowMatching(sd, tiny, device="cuda:0", max_batch=8, max_prompts=8, max_lang=Lmax)
    mean, std = torch.linspace(-0.2, 0.2, 7), torch.linspace(0.5, 1.5, 7)
    pol = _pi0_policy(model, tiny, steps, Lmax, action_mean=mean, action_std=std)
    plain = _pi0_policy(model, tiny, steps, Lmax)                          # no normalisation: the normalised rows
    obs = scripted_inputs(2, B, chunk, tiny["image"], seed=21)
    tasks = [t for t in ("put the spoon on the towel", "move the spoon to the cloth") for _ in range(n)]
    batch = lambda o: {"observation.images.top": o["frame"].repeat(B, 1, 1, 1).to(dev), "observation.state": o["state"].repeat(B, 1).to(dev),
                       "task": tasks}

    def rows(p, o, **kw):
        q = p.select_action(batch(o), noise=o["noise"].to(dev), **kw)
        out = torch.stack([a.clone() for a in q], dim=1)
        q.clear()
        return out
    aug = host.Augment(n, K, host.augmentation_normals(G, K, steps, seed=5).to(dev), sigma=0.8, sd_floor=0.0, clip=(-float("inf"), float("inf")))
    unnorm = lambda t: t * std.to(dev) + mean.to(dev)
    # diverse = None (the default): the queue is the parent's -- the policy's rows unnormalised, nothing kept
    assert pol.diverse is None and pol.last_diverse is None
    norm_own, norm_aug = rows(plain, obs[0]), rows(plain, obs[1], augment=aug)   # [B, steps, 7], [G * S, steps, 7], normalised
    assert np.array_equal(_bits(rows(pol, obs[0])), _bits(unnorm(norm_own))) and pol.last_diverse is None
    pol.commit(1)
    pol.proposal_prior = host.ProposalPrior(n, 1.0, 0.05)
    pol.coherence = host.Coherence(DR.DIM_SCALE, 0.8, 0.25)
    base = rows(pol, obs[1], augment=aug)
    assert np.array_equal(_bits(base), _bits(unnorm(norm_aug))) and pol.last_diverse is None
    base_pp, base_coh = pol.last_proposal_prior.clone(), pol.last_coherence_prior.clone()
    assert tuple(base_pp.shape) == (G * S,) and tuple(base_coh.shape) == (G * S,)
    # diverse set: the queue holds the gathered rows, the priors are gathered alike
    div = host.Diversity(keep, 0.5, DR.DIM_SCALE, 0.8, 0.25)
    pol.diverse = div
    got = rows(pol, obs[1], augment=aug)
    sub = pol.last_diverse
    want = DR.reference(norm_aug.cpu().numpy(), S, keep, base_pp.cpu().numpy(), 0.5, -1.0, DR.step_weights(steps, 0.8), DR.DIM_SCALE, 0.25)
    _assert_same(_as_dict(sub), want, "PI0Policy.diverse")
    idx = sub.picked.reshape(-1).long()
    assert bool(sub.valid.all()) and tuple(got.shape) == (G * keep, steps, 7)
    assert np.array_equal(_bits(sub.rows), _bits(norm_aug[idx])) and np.array_equal(_bits(got), _bits(base[idx]))
    assert np.array_equal(_bits(pol.last_proposal_prior), _bits(base_pp[idx])) and np.array_equal(_bits(pol.last_coherence_prior), _bits(base_coh[idx]))
    # a covering distance beyond every pair: one pick per prompt, the unfilled slots repeat it and carry -inf priors
    pol.diverse = host.Diversity(keep, 0.5, DR.DIM_SCALE, 0.8, 0.25, cover_dist=1.0e6)
    got = rows(pol, obs[1], augment=aug)
    sub = pol.last_diverse
    assert sub.count.cpu().tolist() == [1, 1] and sub.valid.cpu().tolist() == [[True, False, False]] * G
    first = sub.picked[:, 0].long().repeat_interleave(keep)
    assert np.array_equal(_bits(got), _bits(base[first]))
    pp = pol.last_proposal_prior.view(G, keep).cpu()
    assert np.array_equal(_bits(pp[:, 0]), _bits(base_pp[sub.picked[:, 0].long()])) and bool(torch.isneginf(pp[:, 1:]).all())
    assert bool(torch.isneginf(pol.last_coherence_prior.view(G, keep)[:, 1:]).all())
    # without augment the prompt's rows are the proposal prior's samples_per_prompt; keep beyond them is refused before the policy runs
    pol.diverse = host.Diversity(2, 0.5, DR.DIM_SCALE, 0.8, 0.25)
    got = rows(pol, obs[0])
    assert tuple(got.shape) == (G * 2, steps, 7) and tuple(pol.last_diverse.assign.shape) == (B,)
    assert np.array_equal(_bits(got), _bits(unnorm(norm_own)[pol.last_diverse.picked.reshape(-1).long()]))
    pol.diverse = host.Diversity(n + 1, 0.5, DR.DIM_SCALE, 0.8, 0.25)
    with pytest.raises(L.CoverError, match="exceeds"):
        pol.select_action(batch(obs[0]), noise=obs[0]["noise"].to(dev))
    pol.reset()
    assert pol.last_diverse is None
