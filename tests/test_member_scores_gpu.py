"""Per-member verifier scores on the GPU: cover_member_scores against the fp32 reference of tests/member_scores_ref.py, bit for bit (the
order of every rounding is specified, so no tolerance is needed), between NaN-payload canaries; its agreement with cover_group_argmax,
ties, the constructed flip, graph replay behind cover_score_select, the argument errors of the C entry, and the option flowing through
EfficientEnsembleMerged.score_histories into cover_prior_select."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, ops, synth
from cover_vla_amd import _lib as L
from tests import member_scores_ref as MR
from tests import prior_ref as PR

pytestmark = pytest.mark.gpu

CANARY = 0x7FC0BEEF                 # a quiet NaN with a payload no arithmetic produces, as int32 bits
PAD = 64                            # canary words either side of every output
FLOAT_KEYS = ("member_scores", "mean", "spread", "min", "robust", "best", "member_best")


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what, keys=MR.KEYS):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, got[k], want[k])


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Raw:
    """The C entries over preallocated static buffers; every output of cover_member_scores lies between two runs of canaries."""

    def __init__(self, dev, M, N, gs, dim):
        self.M, self.N, self.gs, self.dim = M, N, gs, dim
        self.it = torch.zeros(M, dim, device=dev)
        self.act = torch.zeros(M, N, dim, device=dev)
        self.scores = torch.zeros(N, device=dev)
        self.sel = (torch.empty(4, dtype=torch.int32, device=dev), torch.empty(2, device=dev), torch.empty(dim, device=dev),
                    torch.empty(N, dim, device=dev))
        shapes = dict(member_scores=(M, N), mean=(N,), spread=(N,), min=(N,), min_member=(N,), robust=(N,), result=(4,), best=(2,),
                      member_result=(M, 4), member_best=(M, 2))
        self.buf = {k: torch.empty(int(np.prod(s)) + 2 * PAD, dtype=torch.int32, device=dev) for k, s in shapes.items()}
        self.out = {}
        for k, s in shapes.items():
            mid = self.buf[k][PAD:-PAD]
            self.out[k] = (mid.view(torch.float32) if k in FLOAT_KEYS else mid).view(*s)
        self.fill()

    def load(self, it, act):
        self.it.copy_(torch.from_numpy(it))
        self.act.copy_(torch.from_numpy(act))

    def fill(self):
        for b in self.buf.values():
            b.fill_(CANARY)

    def untouched(self):
        return all(bool((b == CANARY).all()) for b in self.buf.values())

    def guards_intact_and_outputs_written(self):
        return all(bool((b[:PAD] == CANARY).all()) and bool((b[-PAD:] == CANARY).all()) and not bool((b[PAD:-PAD] == CANARY).any())
                   for b in self.buf.values())

    def score_select(self):
        a = L.ScoreSelectArgs()
        a.it, a.act = self.it.data_ptr(), self.act.data_ptr()
        a.n_members, a.N, a.dim, a.group_size = self.M, self.N, self.dim, self.gs
        a.scores_out, a.result_out, a.best_out = self.scores.data_ptr(), self.sel[0].data_ptr(), self.sel[1].data_ptr()
        a.fused_it_out, a.fused_act_out = self.sel[2].data_ptr(), self.sel[3].data_ptr()
        return L.lib().cover_score_select(C.byref(a), _stream())

    def call(self, kappa=0.5, mode=0, **over):
        a = L.MemberScoresArgs()
        a.it, a.act, a.scores = self.it.data_ptr(), self.act.data_ptr(), self.scores.data_ptr()
        a.n_members, a.N, a.dim, a.group_size, a.kappa, a.mode = self.M, self.N, self.dim, self.gs, kappa, mode
        for k, t in self.out.items():
            setattr(a, k + "_out", t.data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return L.lib().cover_member_scores(C.byref(a), _stream())


# ------------------------------------------------------------------------------------------------ 1. every case of the table
@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_matches_reference_bit_for_bit(dev, case):
    M, N, gs, dim = case
    it, act = MR.case_inputs(case)
    raw = _Raw(dev, M, N, gs, dim)
    raw.load(it, act)
    scores, *_ = ops.score_select(raw.it, raw.act, gs)           # the device's own fused scores: the reference takes these bits
    raw.scores.copy_(scores)
    s_host = scores.cpu().numpy()
    assert np.isfinite(s_host).all()
    for mode, kappa in MR.RUNS:
        want = MR.reference(it, act, s_host, gs, kappa, mode)
        raw.fill()
        assert raw.call(kappa, ops.MEMBER_MODES[mode]) == 0
        torch.cuda.synchronize()
        _assert_same(raw.out, want, (MR.case_id(case), mode, kappa))
        assert raw.guards_intact_and_outputs_written(), (mode, kappa)
        assert np.array_equal(_bits(raw.scores), _bits(s_host))  # read only
        got = ops.member_scores(raw.it, raw.act, raw.scores, gs, kappa, mode)
        assert set(got) == set(MR.KEYS)
        _assert_same(got, want, ("ops", MR.case_id(case), mode, kappa))
    assert np.array_equal(_bits(raw.it), _bits(it)) and np.array_equal(_bits(raw.act), _bits(act))


# ------------------------------------------------------------------------------------------------ 2. consistency with existing launches
@pytest.mark.parametrize("case", MR.CASES, ids=MR.case_id)
def test_decisions_are_group_argmax_on_their_rows(dev, case):
    M, N, gs, dim = case
    it, act = (torch.from_numpy(x).to(dev) for x in MR.case_inputs(case))
    scores = ops.score_select(it, act, gs)[0]
    for mode, kappa in (("lcb", 0.5), ("min", 0.0)):
        r = ops.member_scores(it, act, scores, gs, kappa, mode)
        result, best = ops.group_argmax(r["robust"], gs)
        assert np.array_equal(_bits(r["result"]), _bits(result)) and np.array_equal(_bits(r["best"]), _bits(best)), mode
        for m in range(M):
            result, best = ops.group_argmax(r["member_scores"][m], gs)
            assert np.array_equal(_bits(r["member_result"][m]), _bits(result)), (mode, m)
            assert np.array_equal(_bits(r["member_best"][m]), _bits(best)), (mode, m)
    r0 = ops.member_scores(it, act, scores, gs)                   # the defaults: lcb at kappa 0 is score_select's own decision
    _, result, best, _, _ = ops.score_select(it, act, gs)
    assert np.array_equal(_bits(r0["robust"]), _bits(scores))
    assert np.array_equal(_bits(r0["result"]), _bits(result)) and np.array_equal(_bits(r0["best"]), _bits(best))


# ------------------------------------------------------------------------------------------------ 3. ties, 4. the constructed flip
def test_ties_go_to_the_first(dev):
    case, it, act = MR.tie_inputs()
    M, N, gs, dim = case
    it_d, act_d = torch.from_numpy(it).to(dev), torch.from_numpy(act).to(dev)
    scores = ops.score_select(it_d, act_d, gs)[0]
    for mode, kappa in (("lcb", 0.0), ("lcb", 0.5), ("min", 0.0)):
        r = ops.member_scores(it_d, act_d, scores, gs, kappa, mode)
        _assert_same(r, MR.reference(it, act, scores.cpu().numpy(), gs, kappa, mode), ("ties", mode, kappa))
        rb = _bits(r["robust"])
        assert rb[0] == rb[1] and np.array_equal(rb[0:4], rb[4:8])                # two equal candidates, two equal groups
        assert r["result"].tolist() == [0, 0, 0, 0] and r["member_result"].tolist() == [[0, 0, 0, 0]] * M
    # a score that is the same under every member: the first member is the minimum
    same_it, same_act = it_d[:1].repeat(M, 1), act_d[:1].repeat(M, 1, 1)
    s2 = ops.score_select(same_it, same_act, gs)[0]
    r = ops.member_scores(same_it, same_act, s2, gs, 0.0, "min")
    ms = _bits(r["member_scores"])
    assert np.array_equal(ms[0], ms[1]) and np.array_equal(ms[0], ms[2])
    assert r["min_member"].tolist() == [0] * N and np.array_equal(_bits(r["min"]), ms[0])


def test_constructed_flip(dev):
    it, act = MR.flip_inputs()
    it_d, act_d = torch.from_numpy(it).to(dev), torch.from_numpy(act).to(dev)
    scores = ops.score_select(it_d, act_d, 2)[0]
    s = scores.cpu().numpy()
    assert abs(s[0] - 0.90370) < 1e-5 and abs(s[1] - 0.89113) < 1e-5
    want = {}
    for mode, kappa, winner in (("lcb", 0.0, 0), ("lcb", 0.1, 1), ("min", 0.0, 1)):
        r = ops.member_scores(it_d, act_d, scores, 2, kappa, mode)
        _assert_same(r, MR.reference(it, act, s, 2, kappa, mode), ("flip", mode, kappa))
        assert r["result"].tolist() == [winner, 0, winner, 0], (mode, kappa)
        want[(mode, kappa)] = r
    r = want[("lcb", 0.1)]
    assert abs(float(r["spread"][0]) - 0.42426) < 1e-5 and float(r["spread"][1]) == 0.0
    assert abs(float(r["robust"][0]) - 0.86127) < 1e-5 and abs(float(r["robust"][1]) - 0.89113) < 1e-5
    assert r["member_result"][:, 0].tolist() == [0, 0, 1] and r["min_member"].tolist() == [2, 0]


# ------------------------------------------------------------------------------------------------ 5. graph replay
def test_graph_replay_follows_the_input_buffers(dev):
    case = (3, 40, 5, 512)
    M, N, gs, dim = case
    raw = _Raw(dev, M, N, gs, dim)
    first, second = MR.case_inputs(case), MR.make_inputs(case, seed=31)
    raw.load(*first)
    torch.cuda.synchronize()

    def pair():
        assert raw.score_select() == 0
        assert raw.call(0.5, 0) == 0

    gr, _ = graphs.capture(pair, dev)
    torch.cuda.synchronize()
    assert raw.untouched() and not bool(raw.scores.any())                 # the capture itself executed nothing
    results = []
    for it, act in (first, second):
        raw.load(it, act)
        raw.fill()
        gr.launch()
        torch.cuda.synchronize()
        s_host = raw.scores.cpu().numpy()
        assert np.array_equal(_bits(s_host), _bits(ops.score_select(raw.it, raw.act, gs)[0]))
        _assert_same(raw.out, MR.reference(it, act, s_host, gs, 0.5, "lcb"), "replay")
        assert raw.guards_intact_and_outputs_written()
        results.append(_bits(raw.out["robust"]).copy())
    assert not np.array_equal(results[0], results[1])                     # the replays had different answers


# ------------------------------------------------------------------------------------------------ 6. argument errors of the C entry
def test_argument_errors_return_einval_and_launch_nothing(dev):
    raw = _Raw(dev, 3, 48, 6, 64)
    bad = [dict(n_members=0), dict(n_members=-1), dict(n_members=17), dict(N=0), dict(N=-48), dict(group_size=0), dict(group_size=-6),
           dict(group_size=5), dict(N=8192, group_size=1), dict(dim=0), dict(dim=-64), dict(dim=4097),
           dict(kappa=-0.5), dict(kappa=float("nan")), dict(kappa=float("inf")), dict(kappa=float("-inf")),
           dict(mode=2), dict(mode=-1), dict(mode=1, kappa=0.5)]
    bad += [{k: None} for k in ("it", "act", "scores")] + [{k + "_out": None} for k in MR.KEYS]
    for over in bad:
        kw = dict(over)
        kappa, mode = kw.pop("kappa", 0.5), kw.pop("mode", 0)
        assert raw.call(kappa, mode, **kw) == -1, over                     # COVER_EINVAL
    assert L.lib().cover_member_scores(None, _stream()) == -1
    torch.cuda.synchronize()
    assert raw.untouched()                                                 # nothing was launched
    for kappa, mode in ((0.5, 0), (0.0, 1)):                               # ... and the same buffers take a valid call
        assert raw.call(kappa, mode) == 0
        torch.cuda.synchronize()
        assert raw.guards_intact_and_outputs_written()
        raw.fill()


# ------------------------------------------------------------------------------------------------ 7. verifier level
def test_score_histories_member_kappa(dev):
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    N, S = 12, 3
    ver = EfficientEnsembleMerged(synth.verifier_checkpoint(3, seed=9), device="cuda:0")
    pf, tf, hists = synth.verifier_inputs(N, seed=9)
    its = ver.image_text_embeddings(pf.to(dev), tf.to(dev))
    assert ver.last_member_stats is None
    # the default call: what ops.score_select gives, and nothing else
    base = ver.score_histories(its, hists, S)
    plain = ver.score_histories(its, hists, S, member_kappa=None, member_mode="lcb")
    scores, result, best, fit, fact = ops.score_select(base["its"], base["acts"], S)
    for r in (base, plain):
        assert set(r) == {"scores", "result", "best", "its", "acts", "fused_it", "fused_act"}
        for k, t in (("scores", scores), ("result", result), ("best", best), ("fused_it", fit), ("fused_act", fact)):
            assert np.array_equal(_bits(r[k]), _bits(t)), k
    assert ver.last_member_stats is None
    it_h, act_h, s_h = base["its"].cpu().numpy(), base["acts"].cpu().numpy(), scores.cpu().numpy()
    # kappa 0: the default decision's bits, plus the new keys
    r0 = ver.score_histories(its, hists, S, member_kappa=0.0)
    assert set(r0) == set(base) | set(MR.KEYS) and ver.last_member_stats is r0
    assert np.array_equal(_bits(r0["result"]), _bits(result)) and np.array_equal(_bits(r0["best"]), _bits(best))
    assert np.array_equal(_bits(r0["scores"]), _bits(scores))
    _assert_same(r0, MR.reference(it_h, act_h, s_h, S, 0.0, "lcb"), "kappa 0")
    # a penalty and the worst member: the robust decision, the fused score kept
    for mode, kappa in (("lcb", 0.5), ("min", 0.0)):
        r = ver.score_histories(its, hists, S, member_kappa=kappa, member_mode=mode)
        assert np.array_equal(_bits(r["scores"]), _bits(scores)) and ver.last_member_stats is r
        _assert_same(r, MR.reference(it_h, act_h, s_h, S, kappa, mode), (mode, kappa))
    # with a prior: cover_prior_select is fed robust in place of scores
    prior = torch.from_numpy(-np.random.default_rng(3).uniform(0.1, 4.0, (N, 5)).astype(np.float32)).to(dev)
    for beta in (0.05, 0.0):
        r = ver.score_histories(its, hists, S, prior=prior, prior_beta=beta, top_m=S, member_kappa=0.5)
        robust = MR.reference(it_h, act_h, s_h, S, 0.5, "lcb")["robust"]
        assert np.array_equal(_bits(r["robust"]), _bits(robust)) and np.array_equal(_bits(r["scores"]), _bits(scores))
        want = PR.reference(robust, prior.cpu().numpy(), None, 0, S, beta, False, S)
        _assert_same(r, want, f"prior on robust, beta {beta}", keys=("prior", "combined", "group_mean", "result", "best", "ranked"))
    # top_m alone ranks by the robust score
    r = ver.score_histories(its, hists, S, top_m=S, member_kappa=0.5)
    want = PR.reference(robust, np.zeros((N, 1), dtype=np.float32), None, 0, S, 0.0, False, S)
    assert "prior" not in r
    _assert_same(r, want, "ranking on robust", keys=("combined", "group_mean", "result", "best", "ranked"))
    # score_features passes the keywords through
    rf = ver.score_features(pf, tf, hists, S, member_kappa=0.5, member_mode="lcb")
    _assert_same(rf, MR.reference(it_h, act_h, s_h, S, 0.5, "lcb"), "score_features")
