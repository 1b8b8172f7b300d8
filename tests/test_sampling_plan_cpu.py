"""cover_vla_amd.sampling.PickPlan on the host: what a call's sampling arguments resolve to, which ops calls one step's pick issues with
which arguments, the error texts of both samplers and the decode-graph key. No GPU: ops.pick_token, ops.token_topn, ops.token_topn_rows
and ops.row_param_tensors are recorders (the style of test_sampling_cpu.test_pick_token_dispatch)."""
import itertools

import pytest
import torch

ROWS, COLS, LO, HI, DEV = 2, 16, 3, 11, "the-device"
RP = (torch.zeros(ROWS), torch.zeros(ROWS, dtype=torch.int32), torch.ones(ROWS))      # what the recorded row_param_tensors returns
OUT_KEYS = {"out_tok", "out_logit", "out_kept", "out_logprob"}


@pytest.fixture
def calls(monkeypatch):
    from cover_vla_amd import ops
    rec = []
    ret = dict(pick_token=("tok", "logit", "kept"), token_topn=None, token_topn_rows=None, row_param_tensors=RP)
    for name, value in ret.items():
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _v=value, **k: (rec.append((_n, a, k)), _v)[1])
    return rec


def _allow():
    from cover_vla_amd import ops
    return ops.TokenAllow(torch.zeros(1, 1, dtype=torch.int32))


# name -> (has_uniforms, (temperature, top_k, top_p), prior_temperature, with allow, the row_param_tensors arguments or None)
CASES = {
    "greedy": (False, (1.0, 0, 1.0), None, False, None),
    "unfiltered": (True, (0.8, 0, 1.0), None, False, None),
    "filtered": (True, (0.8, 20, 0.9), None, False, None),
    "row-temperature": (True, ([0.0, 0.7], 0, 1.0), None, False, ([0.0, 0.7], 0, 1.0)),
    "row-top_k": (True, (0.8, [0, 5], 1.0), None, False, (0.8, [0, 5], 1.0)),
    "row-top_p": (True, (0.8, 0, [1.0, 0.9]), None, False, (0.8, 0, [1.0, 0.9])),
    "prior": (True, (0.8, 0, 1.0), 1.0, False, (0.8, 0, 1.0)),
    "allow": (True, (0.8, 0, 1.0), None, True, (0.8, 0, 1.0)),
    "greedy-allow": (False, (1.0, 0, 1.0), None, True, (0.0, 0, 1.0)),
}
TABLE = list(itertools.product((False, True), CASES))


def _resolve(filter_always, case, n_top=0):
    from cover_vla_amd.sampling import PickPlan
    has_u, params, prior, with_allow, _ = CASES[case]
    allow = _allow() if with_allow else None
    what, unit = ("generate_tokens", "row") if filter_always else ("sample", "candidate")
    plan = PickPlan.resolve(what, unit, ROWS, DEV, has_uniforms=has_u, params=params, top_logprobs=n_top, prior_temperature=prior, allow=allow,
                            filter_always=filter_always)
    return plan, allow


def _expected(filter_always, case, n_top):
    """(greedy, temperature, filt, rp is None, allow is None, t_ref, n_top) of the table's cell."""
    has_u, (T, k, p), prior, with_allow, rpt = CASES[case]
    if rpt is not None:                                   # rows mode: per-row parameter, prior_temperature or allow
        return (not has_u, None, None, False, not with_allow, prior, n_top)
    # pi0-FAST (filter_always): always (top_k, top_p); OpenVLA: None for greedy and for filters that filter nothing
    filt = (k, p) if filter_always or case == "filtered" else None
    return (not has_u, T, filt, True, True, None, n_top)


@pytest.mark.parametrize("filter_always,case", TABLE)
def test_resolution_table(calls, filter_always, case):
    for n_top in (0, 3):
        del calls[:]
        plan, allow = _resolve(filter_always, case, n_top)
        got = (plan.greedy, plan.temperature, plan.filt, plan.rp is None, plan.allow is None, plan.t_ref, plan.n_top)
        assert got == _expected(filter_always, case, n_top)
        assert plan.allow is allow
        rpt = CASES[case][4]
        if rpt is None:
            assert calls == []
        else:                                             # one upload, with the scalars as given (greedy + allow: every row greedy)
            assert calls == [("row_param_tensors", (ROWS,) + rpt + (DEV,), {})] and plan.rp is RP


@pytest.mark.parametrize("filter_always,case", TABLE)
def test_pick_dispatch(calls, filter_always, case):
    """plan.pick is ONE ops.pick_token and, with top, ONE top-n launch: positional values and the exact keyword set. Keywords of features
    that are off are absent, not None; temperature and filt travel only outside rows mode."""
    plan, allow = _resolve(filter_always, case, 3)
    has_u, (T, k, p) = CASES[case][0], CASES[case][1]
    lg, u = torch.zeros(ROWS, COLS), (torch.zeros(ROWS) if has_u or plan.rp is not None else None)
    tok, sel, kept, lp, ref = (torch.zeros(ROWS) for _ in range(5))
    top = (torch.zeros(ROWS, 3), torch.zeros(ROWS, 3), torch.zeros(ROWS))
    for with_top in (False, True):
        del calls[:]
        r = plan.pick(lg, LO, HI, u, out_tok=tok, out_logit=sel, out_kept=kept, out_logprob=lp, out_ref=ref, top=top if with_top else None)
        assert r == ("tok", "logit", "kept") and len(calls) == (2 if with_top else 1)
        name, a, kw = calls[0]
        assert name == "pick_token" and a[0] is lg and a[1:3] == (LO, HI) and a[3] is u
        assert kw["out_tok"] is tok and kw["out_logit"] is sel and kw["out_kept"] is kept and kw["out_logprob"] is lp
        if plan.rp is None:
            assert a[4:] == (T, plan.filt) and set(kw) == OUT_KEYS
        else:
            extra = {"row_params"} | ({"allow"} if allow is not None else set()) | ({"ref"} if plan.t_ref is not None else set())
            assert a[4:] == () and set(kw) == OUT_KEYS | extra and kw["row_params"] is RP
            assert kw.get("allow") is allow
            if plan.t_ref is not None:
                assert kw["ref"][0] == plan.t_ref and kw["ref"][1] is ref
        if not with_top:
            continue
        name, a, kw = calls[1]
        assert a[0] is lg and a[1:4] == (LO, HI, 3)
        assert kw["out_tok"] is top[0] and kw["out_logprob"] is top[1] and kw["out_entropy"] is top[2]
        if plan.rp is not None:
            assert name == "token_topn_rows" and all(x is y for x, y in zip(a[4:], RP)) and len(a) == 7
            assert set(kw) == {"out_tok", "out_logprob", "out_entropy"} | ({"allow"} if allow is not None else set()) and kw.get("allow") is allow
        else:
            # a greedy pick ranks at temperature 1, unfiltered; an unfiltered sampled OpenVLA plan (filt None) at (T, 0, 1.0)
            want = (1.0, 0, 1.0) if not has_u else (T, k, p)
            assert name == "token_topn" and a[4:] == want and set(kw) == {"out_tok", "out_logprob", "out_entropy"}
    if case == "unfiltered" and not filter_always:
        assert plan.filt is None and calls[1][1][4:] == (0.8, 0, 1.0)
    if case == "greedy":
        assert calls[1][1][4:] == (1.0, 0, 1.0)


PRIOR_TEXT = ("prior_temperature needs uniforms: the reference score comes from the per-row sampler, in which a greedy "
              "candidate is a row with temperature=0 (pass uniforms and temperature=0 rows instead of uniforms=None)")


def test_errors_and_graph_key(calls):
    """Every error of the two samplers' argument handling keeps its exception type and text (the texts are OpenVLA.sample's and
    PI0FASTTokens.generate_tokens' before the fold); graph_key tells apart exactly what a captured decode loop depends on."""
    from cover_vla_amd import _lib
    from cover_vla_amd.sampling import PickPlan

    def resolve(model, has_uniforms=True, params=(0.8, 0, 1.0), **kw):
        what, unit = ("generate_tokens", "row") if model == "pi0fast" else ("sample", "candidate")
        return PickPlan.resolve(what, unit, ROWS, DEV, has_uniforms=has_uniforms, params=params, filter_always=model == "pi0fast", **kw)

    per_row = {"openvla": "per-candidate temperature / top_k / top_p need uniforms (a greedy candidate is a temperature of 0)",
               "pi0fast": "per-row temperature / top_k / top_p need uniforms (a greedy row is a temperature of 0)"}
    bad_ref = {"openvla": "sample: prior_temperature must be finite and > 0 (got 0.0)",
               "pi0fast": "generate_tokens: prior_temperature must be finite and > 0 (got 0.0)"}
    for model in ("openvla", "pi0fast"):
        for n in (-1, 65):
            with pytest.raises(ValueError) as e:
                resolve(model, top_logprobs=n)
            assert str(e.value) == "top_logprobs must be in 0..64"
        with pytest.raises(ValueError) as e:
            resolve(model, has_uniforms=False, prior_temperature=1.0)
        assert str(e.value) == PRIOR_TEXT
        with pytest.raises(_lib.CoverError) as e:
            resolve(model, prior_temperature=0.0)
        assert str(e.value) == bad_ref[model]
        for params in (([0.0, 0.7], 0, 1.0), (0.8, [0, 5], 1.0), (0.8, 0, torch.tensor([1.0, 0.9]))):
            with pytest.raises(ValueError) as e:
                resolve(model, has_uniforms=False, params=params)
            assert str(e.value) == per_row[model]
        # the range check comes first, then the reference temperature, then the per-row rule
        with pytest.raises(ValueError, match="top_logprobs"):
            resolve(model, has_uniforms=False, params=([0.0, 0.7], 0, 1.0), top_logprobs=65, prior_temperature=0.0)
        with pytest.raises(_lib.CoverError):
            resolve(model, has_uniforms=False, params=([0.0, 0.7], 0, 1.0), prior_temperature=0.0)
    assert calls == []                                                     # no error path uploads anything

    key = lambda logprobs=False, **kw: resolve("openvla", **kw).graph_key(logprobs)
    # a new ladder of the same shape is not a new capture
    assert key(params=([0.0, 0.7], 0, 1.0)) == key(params=([0.3, 1.1], [0, 5], 0.9)) == key(params=(0.5, 0, [1.0, 0.9]))
    hash(key(params=([0.0, 0.7], 0, 1.0), prior_temperature=1.0, top_logprobs=3))
    pairs = [(key(has_uniforms=False, params=(1.0, 0, 1.0)), key(params=(1.0, 0, 1.0))),              # greedy vs sampled
             (key(params=(0.8, 0, 1.0)), key(params=(0.9, 0, 1.0))),                                  # two scalar temperatures
             (key(params=(0.8, 0, 1.0)), key(params=(0.8, 20, 0.9))),                                 # filt None vs set
             (key(params=(0.8, 20, 0.9)), key(params=(0.8, 20, 0.8))),
             (key(False), key(True)),                                                                # with vs without log-probabilities
             (key(top_logprobs=2), key(top_logprobs=3)), (key(), key(top_logprobs=1)),                # two n_top values
             (key(prior_temperature=1.0), key(prior_temperature=1.5)),                                # two t_ref values
             (key(params=([0.8, 0.8], 0, 1.0)), key(prior_temperature=1.0)),
             (key(params=([0.8, 0.8], 0, 1.0)), key(params=(0.8, 0, 1.0)))]                           # rows vs scalar
    for a, b in pairs:
        assert a != b
