"""Allowed-token sets per row on the GPU (ops.token_sample_rows / token_logprob_rows / token_topn_rows with allow=): against the float64
reference of tests/allow_ref.py, against the unmasked calls on a materialised -inf copy bit for bit, an all-ones set, independence of set
index / stride / position, constructed and invalid rows, the C entry points, graph replay, and pi0-FAST (generate_tokens, the policy)."""
import functools

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd._lib import CoverError
from tests import allow_ref as AR
from tests import logprob_ref as LR
from tests import sample_rows_ref as RR
from tests import sampling_ref as R
from tests import topn_ref as TR

pytestmark = pytest.mark.gpu

ONE_M = float(np.nextafter(np.float32(1), np.float32(0)))
DEV = "cuda:0"


def bits(t):
    """Floats compared as bit patterns: NaN equals NaN, -0.0 differs from +0.0."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def _dev(*arrays):
    return tuple(None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV).contiguous()
                 for a in arrays)


def _words(on):
    """bool [n_sets, cols] -> the device uint32 tensor of its bits (the test-side packer, not the builder)."""
    return torch.from_numpy(AR.pack_bits(on).view(np.int32)).view(torch.uint32).to(DEV)


def _allow(on, sor=None):
    return ops.TokenAllow(_words(on), None if sor is None else _dev(np.asarray(sor, dtype=np.int32))[0])


def _rows(x, lo, hi, u, T, k, p, allow=None):
    """One token_sample_rows launch -> (tok, logit, kept, logprob) on the device."""
    lp = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    tok, lg, kept = ops.token_sample_rows(x, lo, hi, u, T, k, p, out_logprob=lp, allow=allow)
    return tok, lg, kept, lp


@functools.lru_cache(maxsize=None)
def mixed(name):
    """The case on the device and its one mixed allowed launch: (xd, ud, lo, hi, (Td, kd, pd), allow, on, sor, (tok, logit, kept, logprob), refs)."""
    x, u, lo, hi, params, on, sor, refs = AR.case_data(name)
    xd, ud = _dev(x, u)
    pd = _dev(*params)
    allow = _allow(on, sor)
    out = _rows(xd, lo, hi, ud, *pd, allow=allow)
    torch.cuda.synchronize()
    return xd, ud, lo, hi, pd, allow, on, sor, out, refs


@functools.lru_cache(maxsize=None)
def materialised(name):
    """The -inf copy of the case's rows on the device: what the unmasked calls are given by the second oracle."""
    x, u, lo, hi, params, on, sor, refs = AR.case_data(name)
    return _dev(AR.masked_copy(x.numpy(), on[sor], lo, hi))[0]


# ------------------------------------------------------------------------------------------------ 1. against the float64 reference
@pytest.mark.parametrize("name", list(RR.CASES))
def test_mixed_launch_matches_reference(dev, name):
    xd, ud, lo, hi, pd, allow, on, sor, (tok, lg, kept, lp), refs = mixed(name)
    AR.check_rows(tok.cpu().numpy(), kept.cpu().numpy(), lp.cpu().numpy(), refs, lo, hi, what=name)
    assert same(lg, xd.gather(1, tok[:, None])[:, 0])                        # the logit of the pick, bit for bit


# ------------------------------------------------------------------------------------------------ 2. against the unmasked calls on the -inf copy
@pytest.mark.parametrize("name", list(RR.CASES))
def test_equals_unmasked_calls_on_minus_inf_copy(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), allow, on, sor, (tok, lg, kept, lp), refs = mixed(name)
    xm = materialised(name)
    m_tok, m_lg, m_kept, m_lp = _rows(xm, lo, hi, ud, Td, kd, pd)
    assert same(tok, m_tok) and same(lg, m_lg) and same(lp, m_lp), name
    kept2 = torch.empty_like(kept)
    a_lp = ops.token_logprob_rows(xd, lo, hi, tok, Td, kd, pd, out_kept=kept2, allow=allow)
    assert same(a_lp, lp) and same(kept2, kept)                             # the scorer on the sampler's own picks
    assert same(a_lp, ops.token_logprob_rows(xm, lo, hi, tok, Td, kd, pd))
    onr = torch.from_numpy(on[sor]).to(DEV)
    for n in (5, 64):
        kept3 = torch.empty_like(kept)
        t_tok, t_lp, t_ent = ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, out_kept=kept3, allow=allow)
        assert same(kept3, kept)
        u_tok, u_lp, _ = ops.token_topn_rows(xm, lo, hi, n, Td, kd, pd)
        # the unmasked ranker may list -inf (disallowed) columns behind the allowed ones: those become -1 / -inf
        dis = (u_tok >= 0) & ~onr.gather(1, u_tok.clamp(min=0))
        assert same(t_tok, torch.where(dis, torch.full_like(u_tok, -1), u_tok)), (name, n)
        assert same(t_lp, torch.where(dis, torch.full_like(u_lp, float("-inf")), u_lp)), (name, n)
        TR.check_topn(t_tok.cpu().numpy(), t_lp.cpu().numpy(), t_ent.cpu().numpy(), kept3.cpu().numpy(), refs, lo, what=f"{name} n={n}", n=n)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. an all-ones set is the unmasked call
@pytest.mark.parametrize("name", list(RR.CASES))
def test_all_ones_set_equals_unmasked_call(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), *_ = mixed(name)
    ones = _allow(np.ones((1, xd.shape[1]), dtype=bool))
    base = _rows(xd, lo, hi, ud, Td, kd, pd)
    got = _rows(xd, lo, hi, ud, Td, kd, pd, allow=ones)
    assert all(same(a, b) for a, b in zip(got, base)), name
    k0, k1 = torch.empty_like(base[2]), torch.empty_like(base[2])
    assert same(ops.token_logprob_rows(xd, lo, hi, base[0], Td, kd, pd, out_kept=k0, allow=ones),
                ops.token_logprob_rows(xd, lo, hi, base[0], Td, kd, pd, out_kept=k1)) and same(k0, k1)
    for n in (5, 64):
        a = ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, out_kept=k0, allow=ones)
        b = ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, out_kept=k1)
        assert all(same(p, q) for p, q in zip(a, b)) and same(k0, k1), (name, n)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("name", list(RR.CASES))
def test_rows_and_set_indices_are_independent(dev, name):
    xd, ud, lo, hi, (Td, kd, pd), allow, on, sor, out, refs = mixed(name)
    rows = xd.shape[0]
    fl = lambda t: t.flip(0).contiguous()
    rev = _rows(fl(xd), lo, hi, fl(ud), fl(Td), fl(kd), fl(pd), allow=ops.TokenAllow(allow.bits, fl(allow.set_of_row)))
    assert all(same(a.flip(0), b) for a, b in zip(rev, out)), name
    for r in range(rows):                                                   # a 1-row launch of every row
        one = _rows(xd[r:r + 1], lo, hi, ud[r:r + 1], Td[r:r + 1].clone(), kd[r:r + 1].clone(), pd[r:r + 1].clone(),
                    allow=ops.TokenAllow(allow.bits, allow.set_of_row[r:r + 1].clone()))
        assert all(same(a, b[r:r + 1]) for a, b in zip(one, out)), (name, r)
    # the same bits at other set indices (reversed, behind an empty set) in a buffer with a larger stride
    words = allow.bits.shape[1]
    wide = torch.zeros(5, words + 7, dtype=torch.int32, device=DEV)
    for s in range(3):
        wide[4 - s, :words].copy_(allow.bits[s].view(torch.int32))
    view = wide.view(torch.uint32)[:, :words]
    moved = ops.TokenAllow(view, (4 - allow.set_of_row).to(torch.int32).contiguous())
    assert view.stride(0) == words + 7
    assert all(same(a, b) for a, b in zip(_rows(xd, lo, hi, ud, Td, kd, pd, allow=moved), out)), name
    a_top = ops.token_topn_rows(xd, lo, hi, 5, Td, kd, pd, allow=allow)
    assert all(same(a, b) for a, b in zip(ops.token_topn_rows(xd, lo, hi, 5, Td, kd, pd, allow=moved), a_top))
    assert same(ops.token_logprob_rows(xd, lo, hi, out[0], Td, kd, pd, allow=moved), out[3])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. constructed rows
def _all_outputs(xd, lo, hi, ud, Td, kd, pd, allow, n=5):
    tok, lg, kept, lp = _rows(xd, lo, hi, ud, Td, kd, pd, allow=allow)
    return (tok, lg, kept, lp, ops.token_logprob_rows(xd, lo, hi, tok, Td, kd, pd, allow=allow)) + \
        tuple(ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, allow=allow))


def test_disallowed_columns_are_never_looked_at(dev):
    xd, ud, lo, hi, (Td, kd, pd), allow, on, sor, out, refs = mixed("mid")
    base = _all_outputs(xd, lo, hi, ud, Td, kd, pd, allow)
    assert all(same(a, b) for a, b in zip(base[:4], out))
    dis = ~torch.from_numpy(on[sor]).to(DEV)
    for v in (float("nan"), float("inf"), 3e38, float(xd.max()) + 5.0):     # the last: above every row's maximum
        xv = torch.where(dis, torch.full_like(xd, v), xd)
        got = _all_outputs(xv, lo, hi, ud, Td, kd, pd, allow)
        assert all(same(a, b) for a, b in zip(got, base)), v
    torch.cuda.synchronize()


def test_constructed_rows(dev):
    g = torch.Generator().manual_seed(5)
    # greedy ties: three equal maxima, the lowest-index one disallowed -> the second; at several widths and alignments
    for ld, lo, hi in ((300, 5, 261), (4200, 3, 4100), (9000, 1, 8999)):
        x = torch.randn(4, ld, generator=g)
        on = np.ones((4, ld), dtype=bool)
        want = []
        for r in range(4):
            cols = np.sort((lo + torch.randperm(hi - lo, generator=g)[:3]).numpy())
            x[r, cols] = 9.0
            on[r, cols[0]] = False
            on[r, ::3] &= bool(r % 2)                                       # and a thinned set on every other row
            on[r, cols[1:]] = True
            want.append(int(cols[1]))
        xd, ud, Td = _dev(x, torch.full((4,), 0.99), torch.zeros(4))
        al = _allow(on, np.arange(4))
        tok, lg, kept, lp = _rows(xd, lo, hi, ud, Td, None, None, allow=al)
        assert tok.tolist() == want and (lg == 9.0).all() and kept.tolist() == on[:, lo:hi].sum(axis=1).tolist()
        xm = _dev(AR.masked_copy(x.numpy(), on, lo, hi))[0]
        assert same(lp, ops.token_logprob_rows(xm, lo, hi, tok, Td)) and same(lp, ops.token_logprob_rows(xd, lo, hi, tok, Td, allow=al))
    # a single allowed column: that token, log-probability 0, kept 1, for any uniform and any parameters
    ld, lo, hi = 5000, 5, 4517
    x, _ = R.lm_like_rows(7110, 8, ld, lo, hi)
    T, k, p = RR.ladder_params(8)
    cols = [lo, lo + 1, lo + 31, 2000, 2047, 2048, hi - 2, hi - 1]
    on = np.zeros((8, ld), dtype=bool)
    on[np.arange(8), cols] = True
    al = _allow(on, np.arange(8))
    xd, Td, kd, pd = _dev(x, T, k, p)
    for u in (0.0, 0.37, ONE_M):
        tok, lg, kept, lp = _rows(xd, lo, hi, torch.full((8,), u, device=DEV), Td, kd, pd, allow=al)
        assert tok.tolist() == cols and (kept == 1).all() and (lp == 0).all() and same(lg, xd[torch.arange(8), cols])
    t_tok, t_lp, t_ent = ops.token_topn_rows(xd, lo, hi, 4, Td, kd, pd, allow=al)
    assert t_tok[:, 0].tolist() == cols and (t_tok[:, 1:] == -1).all() and (t_lp[:, 0] == 0).all() and torch.isneginf(t_lp[:, 1:]).all()
    assert (t_ent == 0).all()
    # the allowed set exactly at the absolute columns {31, 32, 63, 64}: word edges, behind lo = 3 and lo = 29
    for lo in (3, 29):
        ld, hi = 4200, lo + 4097
        x, u = R.lm_like_rows(7111 + lo, 8, ld, lo, hi)
        on = np.zeros((1, ld), dtype=bool)
        on[0, [31, 32, 63, 64]] = True
        al = _allow(on)
        xd, ud = _dev(x, u)
        tok, lg, kept, lp = _rows(xd, lo, hi, ud, Td, kd, pd, allow=al)
        refs = [AR.reference_row(x.numpy()[r, lo:hi], on[0, lo:hi], float(u[r]), float(T[r]), int(k[r]), float(p[r])) for r in range(8)]
        AR.check_rows(tok.cpu().numpy(), kept.cpu().numpy(), lp.cpu().numpy(), refs, lo, hi, what=f"columns 31/32/63/64 behind lo={lo}")
        xm = _dev(AR.masked_copy(x.numpy(), np.repeat(on, 8, axis=0), lo, hi))[0]
        m = _rows(xm, lo, hi, ud, Td, kd, pd)
        assert same(tok, m[0]) and same(lg, m[1]) and same(lp, m[3])
        # top-n with fewer allowed columns than n pads with -1 / -inf
        t_tok, t_lp, t_ent = ops.token_topn_rows(xd, lo, hi, 8, Td, kd, pd, allow=al)
        TR.check_topn(t_tok.cpu().numpy(), t_lp.cpu().numpy(), t_ent.cpu().numpy(), kept.cpu().numpy(), refs, lo, what=f"top-8 of 4, lo={lo}", n=8)
        assert (t_tok[:, 4:] == -1).all() and torch.isneginf(t_lp[:, 4:]).all() and (t_tok[:, 0] >= 31).all()
        # the scorer: a disallowed token and a token outside the range get -inf; an allowed one is finite on an unfiltered row
        for t, fin in ((33, False), (lo, False), (hi, False), (0, False), (64, True)):
            s = ops.token_logprob_rows(xd, lo, hi, torch.full((8,), t, dtype=torch.int64, device=DEV), Td, None, None, allow=al)
            assert bool(torch.isfinite(s).all()) if fin else bool(torch.isneginf(s).all()), (lo, t)
    # rows without a maximum (the kernels' stated fallbacks): allowed columns all NaN -> the first allowed column, greedy and sampled
    # alike; an unmasked greedy row of NaNs -> column lo
    ld, lo, hi = 300, 5, 261
    x = torch.randn(3, ld, generator=g)
    cols = [lo + 7, lo + 40, hi - 1]
    on = np.zeros((3, ld), dtype=bool)
    on[:, cols] = True
    x[:, cols] = float("nan")
    x[2, lo:hi] = float("nan")
    xd, ud, Td = _dev(x, torch.full((3,), 0.37), torch.tensor([0.0, 0.8, 0.0]))
    tok, lg, kept, lp = _rows(xd, lo, hi, ud, Td, None, None, allow=_allow(on, np.arange(3)))
    assert tok.tolist() == [lo + 7] * 3 and torch.isnan(lg).all() and kept[[0, 2]].tolist() == [3, 3]
    tok, lg, kept, lp = _rows(xd[2:3], lo, hi, ud[2:3], Td[2:3], None, None)
    assert tok.tolist() == [lo] and torch.isnan(lg).all() and kept.tolist() == [hi - lo]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. invalid rows
def _guarded(rows, dtype, cols=None, guard=16):
    """An output [rows] (or [rows, cols]) in the middle of a larger buffer filled with a pattern: (buffer, the view)."""
    n = rows * (cols or 1)
    buf = torch.full((n + 2 * guard,), float("nan") if dtype == torch.float32 else -77, dtype=dtype, device=DEV)
    view = buf[guard:guard + n]
    return buf, (view if cols is None else view.view(rows, cols))


def _guards_intact(buf, rows, cols=None, guard=16):
    n = rows * (cols or 1)
    edge = torch.cat([buf[:guard], buf[guard + n:]])
    return bool(torch.isnan(edge).all()) if buf.dtype == torch.float32 else bool((edge == -77).all())


def test_invalid_rows_report_themselves(dev):
    rows, ld, lo, hi = 8, 5000, 37, 4549                                    # 4512 columns: wider than the LDS candidate list
    x, u = R.lm_like_rows(7106, rows, ld, lo, hi)
    T, k, p = RR.ladder_params(rows)
    on = np.zeros((3, ld), dtype=bool)
    on[0, ::2] = True
    on[1, lo + 100: lo + 300] = True
    on[2, :lo] = on[2, hi:] = True                                          # bits only outside [lo, hi)
    good = np.array([0, 1, 0, 1, 1, 0, 1, 0], dtype=np.int32)
    sor = good.copy()
    sor[1], sor[3], sor[4], sor[6] = -1, 3, 2, 2                            # below, n_sets, and the set without a column in range (twice)
    invalid = [1, 3, 4, 6]
    valid = [r for r in range(rows) if r not in invalid]
    xd, ud, Td, kd, pd = _dev(x, u, T, k, p)
    ref = _rows(xd, lo, hi, ud, Td, kd, pd, allow=_allow(on, good))
    al = _allow(on, sor)
    bufs = [_guarded(rows, dt) for dt in (torch.int64, torch.float32, torch.int32, torch.float32)]
    tok, lg, kept, lp = (v for _, v in bufs)
    ops.token_sample_rows(xd, lo, hi, ud, Td, kd, pd, out_tok=tok, out_logit=lg, out_kept=kept, out_logprob=lp, allow=al)
    torch.cuda.synchronize()
    assert (tok[invalid] == -1).all() and torch.isnan(lg[invalid]).all() and (kept[invalid] == 0).all() and torch.isnan(lp[invalid]).all()
    assert all(same(a[valid], b[valid]) for a, b in zip((tok, lg, kept, lp), ref))
    assert all(_guards_intact(b, rows) for b, _ in bufs)
    (b_lp, lp2), (b_k, kept2) = _guarded(rows, torch.float32), _guarded(rows, torch.int32)
    ops.token_logprob_rows(xd, lo, hi, ref[0], Td, kd, pd, out=lp2, out_kept=kept2, allow=al)
    assert torch.isnan(lp2[invalid]).all() and (kept2[invalid] == 0).all() and same(lp2[valid], ref[3][valid]) and same(kept2[valid], ref[2][valid])
    n = 5
    g_tok, g_lp, g_ent = ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, allow=_allow(on, good))
    (b_tt, tt), (b_tl, tl), (b_te, te), (b_tk, tk) = (_guarded(rows, torch.int64, n), _guarded(rows, torch.float32, n), _guarded(rows, torch.float32),
                                                      _guarded(rows, torch.int32))
    ops.token_topn_rows(xd, lo, hi, n, Td, kd, pd, out_tok=tt, out_logprob=tl, out_entropy=te, out_kept=tk, allow=al)
    assert (tt[invalid] == -1).all() and torch.isneginf(tl[invalid]).all() and torch.isnan(te[invalid]).all() and (tk[invalid] == 0).all()
    assert same(tt[valid], g_tok[valid]) and same(tl[valid], g_lp[valid]) and same(te[valid], g_ent[valid]) and same(tk[valid], ref[2][valid])
    assert all(_guards_intact(b, rows) for b in (b_lp, b_k, b_te, b_tk)) and _guards_intact(b_tt, rows, n) and _guards_intact(b_tl, rows, n)
    torch.cuda.synchronize()                                                # no error was left behind


# ------------------------------------------------------------------------------------------------ 7. the C entry points
def test_c_entry_points_refuse_bad_launch_arguments(dev):
    import ctypes as C
    from cover_vla_amd import _lib as L
    x, u, T = torch.zeros(4, 64, device=dev), torch.zeros(4, device=dev), torch.ones(4, device=dev)
    tok = torch.full((4,), -7, dtype=torch.int64, device=dev)
    tok2 = torch.full((4, 4), -7, dtype=torch.int64, device=dev)
    lp = torch.full((4, 4), -7.0, device=dev)
    words = torch.full((2, 4), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    NO_ALLOW = object()

    def allow_of(over):
        if over.get("allow", None) is NO_ALLOW:
            return None
        al = L.TokenAllow()
        al.bits, al.ld_words, al.n_sets, al.set_of_row = words.data_ptr(), 4, 2, None
        for k_, v in over.items():
            if k_ in ("bits", "ld_words", "n_sets"):
                setattr(al, k_, v)
        return C.byref(al)

    def fill(a, **over):
        a.logits, a.ld, a.rows, a.lo, a.hi, a.temperature = x.data_ptr(), 64, 4, 0, 64, T.data_ptr()
        for k_, v in over.items():
            if k_ not in ("allow", "bits", "ld_words", "n_sets"):
                setattr(a, k_, v)
        return a

    def sample(**over):
        a = fill(L.TokenSampleRowsArgs(), **dict(dict(uniform=u.data_ptr(), token_out=tok.data_ptr()), **over))
        return L.lib().cover_token_sample_rows_allowed(C.byref(a), allow_of(over), st)

    def logprob(**over):
        a = fill(L.TokenLogprobRowsArgs(), **dict(dict(token=tok.data_ptr(), logprob_out=lp.data_ptr()), **over))
        return L.lib().cover_token_logprob_rows_allowed(C.byref(a), allow_of(over), st)

    def topn(**over):
        a = fill(L.TokenTopnRowsArgs(), **dict(dict(n=4, token_out=tok2.data_ptr(), ld_tok=4, logprob_out=lp.data_ptr(), ld_lp=4), **over))
        return L.lib().cover_token_topn_rows_allowed(C.byref(a), allow_of(over), st)

    shape = (dict(hi=0), dict(lo=-1), dict(lo=0, hi=(1 << 20) + 1), dict(rows=-1), dict(logits=None), dict(temperature=None))
    sets = (dict(allow=NO_ALLOW), dict(bits=None), dict(n_sets=0), dict(n_sets=-1), dict(ld_words=1), dict(bits=words.data_ptr() + 2),
            dict(bits=words.data_ptr() + 1))
    for over in shape + sets + (dict(uniform=None), dict(token_out=None)):
        assert sample(**over) == -1, over                                   # COVER_EINVAL
    for over in shape + sets + (dict(token=None), dict(logprob_out=None)):
        assert logprob(**over) == -1, over
    for over in shape + sets + (dict(n=0), dict(n=65), dict(ld_tok=3), dict(ld_lp=3), dict(token_out=None), dict(logprob_out=None)):
        assert topn(**over) == -1, over
    torch.cuda.synchronize()
    assert (tok == -7).all() and (tok2 == -7).all() and (lp == -7.0).all()   # nothing was launched
    assert sample() == 0 and sample(ld_words=2, n_sets=1) == 0 and topn() == 0 and logprob() == 0
    torch.cuda.synchronize()
    assert (tok == 0).all()
    # the Python wrappers: a set too short for hi, set_of_row of another length, allow without row_params
    al = ops.TokenAllow(words[:, :1].contiguous().view(torch.uint32))
    for call in (lambda: ops.token_sample_rows(x, 0, 64, u, T, allow=al),
                 lambda: ops.token_topn_rows(x, 0, 64, 4, T, allow=ops.TokenAllow(words.view(torch.uint32), torch.zeros(3, dtype=torch.int32, device=dev))),
                 lambda: ops.pick_token(x, 0, 64, u, allow=ops.TokenAllow(words.view(torch.uint32))),
                 lambda: ops.token_logprob_rows(x, 0, 64, tok, T, allow=words)):
        with pytest.raises(CoverError):
            call()


# ------------------------------------------------------------------------------------------------ 8. graph
def test_graph_replay_follows_the_set_tensors(dev):
    xd, ud, lo, hi, (Td, kd, pd), allow, on, sor, first, refs = mixed("mid")
    rows = xd.shape[0]
    sor2 = torch.roll(allow.set_of_row, 1).contiguous()
    second = _rows(xd, lo, hi, ud, Td, kd, pd, allow=ops.TokenAllow(allow.bits, sor2))         # other sets for the same rows, eager
    on3 = on.copy()
    on3[0] = ~on3[0]
    on3[2, lo + 7] = True
    third = _rows(xd, lo, hi, ud, Td, kd, pd, allow=_allow(on3, sor))                          # other bits
    assert not same(second[0], first[0]) and not same(third[0], first[0])
    bits_s, sor_s = allow.bits.view(torch.int32).clone().view(torch.uint32), allow.set_of_row.clone()                              # the static buffers of the capture
    tok = torch.empty(rows, dtype=torch.int64, device=dev)
    lg, lp = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    kept = torch.empty(rows, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with ops.Graph() as gr:
            ops.token_sample_rows(xd, lo, hi, ud, Td, kd, pd, out_tok=tok, out_logit=lg, out_kept=kept, out_logprob=lp,
                                  allow=ops.TokenAllow(bits_s, sor_s))
        for want, b, s in ((first, allow.bits, allow.set_of_row), (second, allow.bits, sor2), (third, _words(on3), allow.set_of_row),
                           (first, allow.bits, allow.set_of_row)):
            bits_s.view(torch.int32).copy_(b.view(torch.int32))
            sor_s.copy_(s)
            tok.fill_(-1)
            gr.launch()
            side.synchronize()
            assert all(same(a, b_) for a, b_ in zip((tok, lg, kept, lp), want))
    torch.cuda.current_stream().wait_stream(side)


# ------------------------------------------------------------------------------------------------ 9. pi0-FAST
TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def _check_steps(logits, picks, kept, lps, on_rows, u, T, k, p, what):
    """Per traced step: every decided pick equals the restricted reference on that step's logits (greedy rows: the first allowed arg-max,
    kept = |allowed|), kept wherever the cut is decided, log-probabilities where given. At least 90 % of the picks decided."""
    n_dec = n_all = 0
    V = on_rows.shape[1]
    for i, lg in enumerate(logits):
        lgn = lg.float().cpu().numpy()
        refs = [AR.reference_row(lgn[r], on_rows[r], float(u[r, i]), float(T[r]), int(k[r]), float(p[r])) for r in range(lgn.shape[0])]
        for r, ref in enumerate(refs):
            n_all += 1
            t = int(picks[i][r])
            assert 0 <= t < V and on_rows[r, t], (what, i, r, t)
            if ref["greedy"]:
                assert t == ref["token"] and int(kept[i][r]) == int(on_rows[r].sum()), (what, i, r)
            if ref["cut_decided"]:
                assert int(kept[i][r]) == ref["kept"], (what, i, r)
            if ref["cut_decided"] and ref["pick_decided"]:
                n_dec += 1
                assert t == ref["token"], (what, i, r)
        if lps is not None:
            LR.check_logprobs(lps[i], picks[i], refs, 0, V, what=f"{what} step {i}", cap=1.0)
    print(f"{what}: {n_dec} of {n_all} picks decided, all equal to the reference")
    assert n_dec >= 0.9 * n_all


def test_pi0fast_allowed_tokens(dev):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, L, n_new, V = 6, 9, 12, TINY["vocab"]
    g = torch.Generator().manual_seed(5)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    toks, pad = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    toks[:, :L - 2] = torch.randint(2, 500, (L - 2,), generator=g)          # identical frames and prompt in every row
    pad[:, :L - 2] = 1
    args = ([img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev))
    g = torch.Generator().manual_seed(9)
    u = torch.rand(B, n_new, generator=g)
    T = np.array([1.0, 0.0, 0.8, 1.0, 1.3, 0.5], dtype=np.float32)          # one greedy row
    k = np.array([0, 0, 50, 0, 20, 1], dtype=np.int32)
    p = np.array([1.0, 1.0, 0.9, 0.7, 1.0, 1.0], dtype=np.float32)
    sets = [[(300, 380), 1, 7, 33], [(64, 96), (400, 512)]]                 # "a band plus a few ids", and a second set
    sor = np.array([0, 1, 0, 1, 0, 1], dtype=np.int32)
    al = ops.TokenAllow(ops.token_allow_sets(V, sets, dev), torch.from_numpy(sor).to(dev))
    on = np.zeros((2, V), dtype=bool)
    on[0, 300:380] = on[0, [1, 7, 33]] = True
    on[1, 64:96] = on[1, 400:512] = True
    on_rows = on[sor]
    before = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, eos_token_id=-1, return_logprobs=True)
    greedy_before = model.generate_tokens(*args, n_new, eos_token_id=-1)
    ones = ops.TokenAllow(ops.token_allow_sets(V, [[(0, V)]], dev))
    for share in (False, True):
        # the ladder, and greedy (no uniforms: temperature 0 for every row), on the traced logits
        for what, kw, (Tr, kr, pr) in (("ladder", dict(uniforms=u.to(dev), temperature=T, top_k=list(k), top_p=torch.from_numpy(p)), (T, k, p)),
                                       ("greedy", dict(), (np.zeros(B), np.zeros(B, dtype=np.int32), np.ones(B)))):
            tr = {}
            out, lps, tl = model.generate_tokens(*args, n_new, trace=tr, return_logprobs=True, top_logprobs=3, share_prefix=share, eos_token_id=-1,
                                                 allowed_tokens=al, **kw)
            assert len(tr["logits"]) == n_new == len(tr["picks"]) and all(lg.shape[0] == B for lg in tr["logits"])   # every row on its own
            assert tr["prefix_slots"] == (1 if share else B)
            out_c, lps_c = out.cpu(), lps.cpu()
            assert all(torch.equal(out_c[:, i], tr["picks"][i].cpu()) for i in range(n_new))
            assert on_rows[np.arange(B)[:, None], out_c.numpy()].all()      # every emitted token is in its row's set
            _check_steps(tr["logits"], [t.cpu() for t in tr["picks"]], [kk.cpu() for kk in tr["kept"]], [lps_c[:, i].numpy() for i in range(n_new)],
                         on_rows, u, Tr, kr, pr, what=f"pi0-FAST allowed {what} share_prefix={share}")
            tt = tl.tokens.cpu().numpy()
            assert tt.shape == (B, n_new, 3) and (tt[:, :, 0] >= 0).all() and torch.isfinite(tl.entropy).all()
            assert (on_rows[np.arange(B)[:, None, None], np.maximum(tt, 0)] | (tt < 0)).all()     # -1 where a row keeps fewer than 3 (top_k = 1)
            assert torch.equal(model.generate_tokens(*args, n_new, share_prefix=share, eos_token_id=-1, allowed_tokens=al, **kw), out)
        # pad after EOS: the pad id (0) is in no set, it is bookkeeping and not a draw
        free = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=-1, allowed_tokens=al)
        eos = int(free[0, 2])
        out_e = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=eos,
                                      allowed_tokens=al).cpu()
        first = int((out_e[0] == eos).nonzero()[0])
        assert first <= 2 and (out_e[0, first + 1:] == 0).all() and not on_rows[0, 0]
        nonpad = out_e != 0
        assert on_rows[np.arange(B)[:, None], out_e.numpy()][nonpad.numpy()].all()
        # an all-ones set equals the per-row path
        got = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=-1,
                                    return_logprobs=True, allowed_tokens=ones)
        want = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, share_prefix=share, eos_token_id=-1,
                                     return_logprobs=True)
        assert torch.equal(got[0], want[0]) and same(got[1], want[1])
    # refused on the host, before the loop
    for bad in (np.array([0, 1, 2, 0, 0, 0]), np.array([0, -1, 0, 0, 0, 0]), np.array([0, 1, 0])):
        with pytest.raises(CoverError):
            model.generate_tokens(*args, n_new, eos_token_id=-1, allowed_tokens=ops.TokenAllow(al.bits, torch.from_numpy(bad.astype(np.int32)).to(dev)))
    empty = ops.TokenAllow(torch.zeros(1, V // 32, dtype=torch.int32, device=dev).view(torch.uint32))
    with pytest.raises(CoverError):
        model.generate_tokens(*args, n_new, eos_token_id=-1, allowed_tokens=empty)
    with pytest.raises(CoverError):
        model.generate_tokens(*args, n_new, eos_token_id=-1, allowed_tokens=ops.TokenAllow(al.bits.view(torch.int32)[:, :8].contiguous().view(torch.uint32)))
    # allowed_tokens=None is what it was before the allowed calls ran
    after = model.generate_tokens(*args, n_new, uniforms=u.to(dev), temperature=T, top_k=k, top_p=p, eos_token_id=-1, return_logprobs=True)
    assert torch.equal(after[0], before[0]) and same(after[1], before[1])
    assert torch.equal(model.generate_tokens(*args, n_new, eos_token_id=-1), greedy_before)


# ------------------------------------------------------------------------------------------------ 10. the policy
def test_policy_allowed_token_ranges(dev):
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTPolicy, PI0FASTTokens
    import types
    c = TINY
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=384, max_new_tokens=24)
    tok = synth.CharTokenizer(vocab_size=512)
    fast = types.SimpleNamespace(bpe_tokenizer=types.SimpleNamespace(decode=lambda t: "".join(chr(max(0, min(int(i), 1000))) for i in t)),
                                 min_token=-40, scale=10.0)
    NoFast = lambda: fast
    g = torch.Generator().manual_seed(2)
    batch = {"observation.state": (torch.rand(3, 8, generator=g) * 2 - 1).to(dev), "task": ["pick up the cube", "open the drawer", "pick up the cube"],
             "observation.images.top": (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(3, 1, 1, 1).to(dev)}
    ranges = [(200, 260), (40, 41), (58, 59)]
    eos, pad = tok.eos_token_id, (tok.pad_token_id if hasattr(tok, "pad_token_id") else tok.eos_token_id)
    ok = np.zeros(c["vocab"], dtype=bool)
    for a, b in ranges:
        ok[a:b] = True
    ok[eos] = True
    seen = {}
    orig = model.generate_tokens

    def spy(*a, **kw):
        seen["kw"] = kw
        seen["out"] = orig(*a, **kw)
        return seen["out"]

    model.generate_tokens = spy
    outs = {}
    for seed in (None, 4):
        for rg in (None, ranges):
            cfg = PI0FASTConfig(resize_imgs_with_padding=(56, 56), max_decoding_steps=8, chunk_size=4, n_action_steps=2, action_dim=3, sample_seed=seed,
                                temperature=1.2, top_k=0, top_p=0.95, allowed_token_ranges=rg)
            pol = PI0FASTPolicy(cfg, model, tok, NoFast())
            act = pol.select_action(dict(batch))
            assert tuple(act.shape) == (3, 3)
            out = seen["out"].cpu().numpy()
            outs[(seed, rg is None)] = out
            if rg is None:
                assert "allowed_tokens" not in seen["kw"] and pol.allowed_tokens is None
                continue
            assert seen["kw"]["allowed_tokens"] is pol.allowed_tokens and pol.allowed_tokens.n_sets == 1
            for r in range(out.shape[0]):                                   # ids inside the ranges, EOS, and pad after EOS only
                hit = np.nonzero(out[r] == eos)[0]
                end = int(hit[0]) + 1 if hit.size else out.shape[1]
                assert ok[out[r, :end]].all() and (out[r, end:] == pad).all(), (seed, r, out[r])
        assert not ok[outs[(seed, True)]].all()                             # the unconstrained run does leave the ranges: the set matters
    # None reproduces the unconstrained result: a second policy with the same seed, after the constrained ones ran
    cfg = PI0FASTConfig(resize_imgs_with_padding=(56, 56), max_decoding_steps=8, chunk_size=4, n_action_steps=2, action_dim=3, sample_seed=4,
                        temperature=1.2, top_k=0, top_p=0.95)
    PI0FASTPolicy(cfg, model, tok, NoFast()).select_action(dict(batch))
    assert np.array_equal(seen["out"].cpu().numpy(), outs[(4, True)])
    with pytest.raises(ValueError):
        PI0FASTPolicy(PI0FASTConfig(allowed_token_ranges=[(0, c["vocab"] + 1)]), model, tok, NoFast())
