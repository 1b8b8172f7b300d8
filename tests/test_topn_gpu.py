"""Top-n alternatives and entropy on the GPU: cover_token_topn against the float64 reference of tests/topn_ref.py (ids and padding exact,
values within the tolerances derived there), bit-identity of its log-probabilities with cover_token_logprob, ties and padding,
determinism and graph replay, argument errors, and top_logprobs of the two policies."""
import ctypes as C

import numpy as np
import pytest
import torch

from cover_vla_amd import ops, synth
from cover_vla_amd import _lib as L
from tests import logprob_ref as LR
from tests import sampling_ref as R
from tests import topn_ref as TR

pytestmark = pytest.mark.gpu

NINF = float("-inf")


def _bits(t):
    return t.cpu().view(torch.int32)


def _topn(xd, lo, hi, n, T, k, p):
    """One launch into sentinel-filled buffers: every slot must be written."""
    rows = xd.shape[0]
    tok = torch.full((rows, n), -7, dtype=torch.int64, device=xd.device)
    lp = torch.full((rows, n), 7.0, dtype=torch.float32, device=xd.device)
    ent = torch.full((rows,), -7.0, dtype=torch.float32, device=xd.device)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=xd.device)
    ops.token_topn(xd, lo, hi, n, temperature=T, top_k=k, top_p=p, out_tok=tok, out_logprob=lp, out_entropy=ent, out_kept=kept)
    torch.cuda.synchronize()
    return tok, lp, ent, kept


def _same(a, b):
    return all(torch.equal(_bits(i), _bits(j)) if i.dtype == torch.float32 else torch.equal(i, j) for i, j in zip(a, b))


def _check_bit_identity(xd, lo, hi, T, k, p, tok, lp, kept, cols, what):
    """Slot j of `cols` carries the bits ops.token_logprob gives for that token (a padded slot, -1, scores -inf there as well), and the
    kept counts agree."""
    kept_s = torch.empty_like(kept)
    for j in cols:
        want = ops.token_logprob(xd, lo, hi, tok[:, j].contiguous(), temperature=T, top_k=k, top_p=p, out_kept=kept_s)
        assert torch.equal(_bits(lp[:, j]), _bits(want)), (what, j)
    assert torch.equal(kept.cpu(), kept_s.cpu()), what


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_topn_matches_reference_and_token_logprob(dev, case):
    x, u, lo, hi, T, k, p, _ = LR.case_data(case)
    refs = TR.case_refs(case)
    xd = x.to(dev)
    for n in (1, 5, 64):
        what = f"{LR.case_id(case)} n={n}"
        tok, lp, ent, kept = _topn(xd, lo, hi, n, T, k, p)
        TR.check_topn(tok.cpu().numpy(), lp.cpu().numpy(), ent.cpu().numpy(), kept.cpu().numpy(), refs, lo, what, n=n)
        _check_bit_identity(xd, lo, hi, T, k, p, tok, lp, kept, range(0, n, 9), what)
        # padding on every row, decided or not: exactly the slots past the kept set
        assert torch.equal(tok == -1, torch.arange(n, device=dev)[None, :] >= kept[:, None]) and torch.equal(tok == -1, lp == NINF), what
        h, logk = ent.cpu().numpy().astype(np.float64), np.log(kept.cpu().numpy().astype(np.float64))
        assert (h >= -TR.TOL_H_ABS).all() and (h <= logk + TR.tolerance_entropy(logk)).all(), what


def test_bit_identity_with_token_logprob_every_slot(dev):
    for case in (("narrow", 1, 0), ("narrow", 0, 0), ("wide", 3, 1)):
        x, u, lo, hi, T, k, p, _ = LR.case_data(case)
        xd = x.to(dev)
        tok, lp, ent, kept = _topn(xd, lo, hi, 16, T, k, p)
        _check_bit_identity(xd, lo, hi, T, k, p, tok, lp, kept, range(16), LR.case_id(case))


# ------------------------------------------------------------------------------------------------ 2. ties and padding
@pytest.mark.parametrize("name", list(TR.tie_inputs()))
def test_ties_and_padding(dev, name):
    x, lo, hi, n, T, k = TR.tie_inputs()[name]
    refs = TR.reference_topn_rows(x, lo, hi, n, T, k, 1.0)
    xd = x.to(dev)
    tok, lp, ent, kept = _topn(xd, lo, hi, n, T, k, 1.0)
    TR.check_topn(tok.cpu().numpy(), lp.cpu().numpy(), ent.cpu().numpy(), kept.cpu().numpy(), refs, lo, name, cap=0.0)
    _check_bit_identity(xd, lo, hi, T, k, 1.0, tok, lp, kept, range(0, n, max(1, n // 8)), name)


# ------------------------------------------------------------------------------------------------ 3. determinism
def test_deterministic_across_row_positions_alignment_launches_and_graph_replay(dev):
    V = R.WIDE_V
    x, _ = R.lm_like_rows(4243, 24, V, 0, V)
    x[17], x[23] = x[0], x[0]
    x[5, :6000] = 1.5                                        # a plateau on the row path, with a tie at every rank
    x[5, 6000:] = -2.0
    x[11] = x[5]
    xd = x.to(dev)
    flat = torch.empty(24 * V + 1, dtype=torch.float32, device=dev)
    shifted = flat[1:].view(24, V)                           # the same rows, one float off: the float4 body starts elsewhere
    shifted.copy_(xd)
    assert shifted.data_ptr() % 16 != xd.data_ptr() % 16
    x2, _ = R.lm_like_rows(4244, 24, V, 0, V)
    for lo, hi, n, T, k, p in [(0, V, 8, 1.0, 0, 1.0), (3, V - 2, 64, 0.7, 64, 0.95), (0, V, 5, 1.5, 0, 0.8), (1, V, 8, 1.0, 50, 1.0)]:
        a = _topn(xd, lo, hi, n, T, k, p)
        assert _same(a, _topn(xd, lo, hi, n, T, k, p))
        assert _same(a, _topn(shifted, lo, hi, n, T, k, p))
        for o in a:
            assert torch.equal(_bits(o[0]), _bits(o[17])) and torch.equal(_bits(o[0]), _bits(o[23])) and torch.equal(_bits(o[5]), _bits(o[11]))
        # recorded into a graph and replayed with other logits in the static buffer; compare with eager on the same logits
        want2 = _topn(x2.to(dev), lo, hi, n, T, k, p)
        xs = xd.clone()
        outs = (torch.empty(24, n, dtype=torch.int64, device=dev), torch.empty(24, n, dtype=torch.float32, device=dev),
                torch.empty(24, dtype=torch.float32, device=dev), torch.empty(24, dtype=torch.int32, device=dev))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with ops.Graph() as gr:
                ops.token_topn(xs, lo, hi, n, temperature=T, top_k=k, top_p=p, out_tok=outs[0], out_logprob=outs[1], out_entropy=outs[2],
                               out_kept=outs[3])
            for src, want in ((xd, a), (x2.to(dev), want2), (xd, a)):
                xs.copy_(src)
                outs[0].fill_(-9)
                outs[1].fill_(3.0)
                gr.launch()
                side.synchronize()
                assert _same(outs, want)
        torch.cuda.current_stream().wait_stream(side)


def test_strided_outputs_are_written_in_place(dev):
    x, u, lo, hi, T, k, p, _ = LR.case_data(("narrow", 1, 0))
    xd = x.to(dev)
    want = _topn(xd, lo, hi, 4, T, k, p)
    tok = torch.full((3, R.ROWS, 6), -9, dtype=torch.int64, device=dev)
    lp = torch.full((3, R.ROWS, 6), 9.0, dtype=torch.float32, device=dev)
    ent = torch.full((3, R.ROWS), 9.0, dtype=torch.float32, device=dev)
    t, l, e = ops.token_topn(xd, lo, hi, 4, temperature=T, top_k=k, top_p=p, out_tok=tok[1, :, :4], out_logprob=lp[1, :, 1:5], out_entropy=ent[1])
    torch.cuda.synchronize()
    assert t.data_ptr() == tok[1].data_ptr() and torch.equal(tok[1, :, :4], want[0]) and torch.equal(_bits(lp[1, :, 1:5]), _bits(want[1]))
    assert torch.equal(_bits(ent[1]), _bits(want[2]))
    assert (tok[0] == -9).all() and (tok[2] == -9).all() and (tok[1, :, 4:] == -9).all()
    assert (lp[0] == 9.0).all() and (lp[2] == 9.0).all() and (lp[1, :, 0] == 9.0).all() and (lp[1, :, 5] == 9.0).all()
    assert (ent[0] == 9.0).all() and (ent[2] == 9.0).all()


# ------------------------------------------------------------------------------------------------ 4. argument errors
def test_argument_errors_return_einval_and_launch_nothing(dev):
    x = torch.zeros(4, 64, device=dev)
    tok = torch.full((4, 8), -7, dtype=torch.int64, device=dev)
    lp = torch.full((4, 8), 5.0, dtype=torch.float32, device=dev)
    ent = torch.full((4,), 5.0, dtype=torch.float32, device=dev)
    kept = torch.full((4,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**over):
        a = L.TokenTopnArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi = x.data_ptr(), 64, 4, 0, 64
        a.temperature, a.top_k, a.top_p, a.n = 1.0, 0, 1.0, 8
        a.token_out, a.ld_tok, a.logprob_out, a.ld_lp = tok.data_ptr(), 8, lp.data_ptr(), 8
        a.entropy_out, a.kept_out = ent.data_ptr(), kept.data_ptr()
        for key, v in over.items():
            setattr(a, key, v)
        return L.lib().cover_token_topn(C.byref(a), stream)

    bad = (dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1), dict(hi=0), dict(lo=-1), dict(lo=0, hi=(1 << 20) + 1), dict(n=0), dict(n=65),
           dict(n=-3), dict(ld_tok=7), dict(ld_lp=7), dict(ld_tok=0), dict(token_out=None), dict(logprob_out=None), dict(logits=None), dict(rows=-1))
    for over in bad:
        assert call(**over) == -1, over                       # COVER_EINVAL
    assert L.lib().cover_token_topn(None, stream) == -1
    torch.cuda.synchronize()
    assert (tok == -7).all() and (lp == 5.0).all() and (ent == 5.0).all() and (kept == -7).all()       # nothing was launched
    assert call(entropy_out=None, kept_out=None) == 0
    torch.cuda.synchronize()
    assert (ent == 5.0).all() and (kept == -7).all() and torch.equal(tok.cpu(), torch.arange(8).expand(4, 8))
    assert call() == 0
    torch.cuda.synchronize()
    assert (kept == 64).all()                                                                        # 64 equal logits
    assert np.abs(lp.cpu().numpy().astype(np.float64) + np.log(64.0)).max() <= float(LR.tolerance(0.0, np.log(64.0)))
    assert np.abs(ent.cpu().numpy().astype(np.float64) - np.log(64.0)).max() <= float(TR.tolerance_entropy(np.log(64.0)))


# ------------------------------------------------------------------------------------------------ 5. OpenVLA
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


def _same_top(a, b):
    return torch.equal(a.tokens, b.tokens) and torch.equal(_bits(a.logprobs), _bits(b.logprobs)) and torch.equal(_bits(a.entropy), _bits(b.entropy))


def _check_pick_slot(top, tokens, lps, what):
    """Wherever the pick ranks inside the alternatives, its slot carries the bits of the return_logprobs value."""
    hit = top.tokens == tokens[..., None]
    assert int(hit.sum()) > 0 and (hit.sum(dim=-1) <= 1).all(), what
    assert torch.equal(_bits(top.logprobs[hit]), _bits(lps[..., None].expand_as(top.logprobs)[hit])), what
    return int(hit.sum())


def _check_steps(top, logits_per_step, lo, hi, n, T, k, p, what, total):
    """top: TopLogprobs [N, steps, ...] from the device; logits_per_step: the traced fp32 logits of each step. A step is a handful of
    rows, so the rows left out are capped by the caller in total."""
    for i, lg in enumerate(logits_per_step):
        refs = TR.reference_topn_rows(lg.float().cpu(), lo, hi, n, T, k, p)
        total[0] += len(refs) - TR.check_topn(top.tokens[:, i].cpu().numpy(), top.logprobs[:, i].cpu().numpy(), top.entropy[:, i].cpu().numpy(),
                                              None, refs, lo, f"{what} step {i}", cap=1.0)
        total[1] += len(refs)
        kept = np.array([r["kept"] for r in refs], dtype=np.float64)
        ent = top.entropy[:, i].cpu().numpy().astype(np.float64)
        assert (ent >= -TR.TOL_H_ABS).all() and (ent <= np.log(kept) + TR.tolerance_entropy(np.log(kept))).all(), (what, i)


def test_openvla_top_logprobs(dev):
    from cover_vla_amd.host import TopLogprobs
    from cover_vla_amd.openvla import OpenVLA
    c, sd, frame, toks, lens, u = _ov_case()
    kw = dict(device="cuda:0", max_prompts=4, max_candidates=8, max_text=toks.shape[1])
    eager = OpenVLA(sd, c, **kw)
    eager.decode_graph = False
    model = OpenVLA(sd, c, **kw)
    assert model.decode_graph
    f, tk, ln, ud = frame.to(dev), toks.to(dev), lens.to(dev), u.to(dev)
    lo, hi = eager.action_lo, eager.action_hi
    n = 4
    counted = [0, 0]
    for name, uni, T, k, p, rlo, rhi in [("greedy", None, 1.0, 0, 1.0, 0, c["tok_vocab"]), ("filtered", ud, 0.9, 50, 0.9, lo, hi),
                                         ("unfiltered", ud, 1.2, 0, 1.0, lo, hi)]:
        n_s = 1 if uni is None else 2
        args = (f, tk, ln, n_s, uni, T)
        base_t, base_s, base_lp = eager.sample(*args, top_k=k, top_p=p, return_logprobs=True)
        n_keys = len(model._dec)
        outs = [eager.sample(*args, top_k=k, top_p=p, return_logprobs=True, top_logprobs=n)]
        outs += [model.sample(*args, top_k=k, top_p=p, return_logprobs=True, top_logprobs=n) for _ in range(3)]   # capture, replay, replay
        assert len(model._dec) == n_keys + 1                               # n is part of the decode-graph key
        N = base_t.shape[0]
        for t, s, lp, top in outs:
            assert torch.equal(t, base_t) and torch.equal(_bits(s), _bits(base_s)) and torch.equal(_bits(lp), _bits(base_lp)), name
            assert isinstance(top, TopLogprobs) and top.tokens.dtype == torch.int64 and tuple(top.tokens.shape) == (N, eager.n_gen, n)
            assert top.logprobs.dtype == torch.float32 and tuple(top.logprobs.shape) == (N, eager.n_gen, n)
            assert top.entropy.dtype == torch.float32 and tuple(top.entropy.shape) == (N, eager.n_gen)
            assert _same_top(top, outs[0][3]), name
        _check_pick_slot(outs[0][3], base_t, base_lp, name)
        t2, s2, top2 = model.sample(*args, top_k=k, top_p=p, top_logprobs=n)          # without return_logprobs: appended after the two
        assert torch.equal(t2, base_t) and torch.equal(_bits(s2), _bits(base_s)) and _same_top(top2, outs[0][3])
        assert len(model._dec) == n_keys + 2
        t3, s3 = model.sample(*args, top_k=k, top_p=p)                                  # top_logprobs=0: the two-tensor return
        assert torch.equal(t3, base_t) and torch.equal(_bits(s3), _bits(base_s))
        # teacher-forced, traced: the alternatives of every step against the reference on that step's logits
        force = torch.randint(lo, hi, (N, eager.n_gen), generator=torch.Generator().manual_seed(4)).to(dev)
        tr = {}
        t4, _, lp4, top4 = eager.sample(*args, top_k=k, top_p=p, trace=tr, force_tokens=force, return_logprobs=True, top_logprobs=n)
        _check_steps(top4, tr["logits"], rlo, rhi, n, T, k, p, f"OpenVLA {name}", counted)
        _check_pick_slot(top4, t4, lp4, name + " forced")
    print(f"OpenVLA: {counted[0]} of {counted[1]} rows counted")
    assert counted[0] >= (1 - R.CAP) * counted[1]
    # the sliced action head: ids offset by action_lo as its tokens are
    sl = OpenVLA(sd, c, **kw)
    sl.slice_action_head = True
    s_t, s_l, s_lp = sl.sample(f, tk, ln, 2, ud, 0.9, top_k=3, top_p=1.0, return_logprobs=True)
    a_t, a_l, a_lp, a_top = sl.sample(f, tk, ln, 2, ud, 0.9, top_k=3, top_p=1.0, return_logprobs=True, top_logprobs=n)
    assert torch.equal(a_t, s_t) and torch.equal(_bits(a_l), _bits(s_l)) and torch.equal(_bits(a_lp), _bits(s_lp))
    tt, tl = a_top.tokens, a_top.logprobs
    pad = tt == -1
    print(f"OpenVLA sliced head: {int(pad[..., 3].sum())} of {pad[..., 3].numel()} steps keep exactly three tokens")
    # top_k = 3 keeps the three largest and whatever ties with the third: slots 0-2 are action ids, slot 3 is a fourth id only in a tie
    assert (pad | ((tt >= lo) & (tt < hi))).all() and not pad[..., :3].any() and torch.equal(pad, tl == NINF)
    # the sliced head's static buffer still holds the last step's logits: that step against the reference over the 256 columns,
    # ids as the reference's relative ids plus action_lo
    N = a_t.shape[0]
    refs = TR.reference_topn_rows(sl.logits_actions[:N].cpu(), 0, c["n_bins"], n, 0.9, 3, 1.0)
    TR.check_topn(tt[:, -1].cpu().numpy(), tl[:, -1].cpu().numpy(), a_top.entropy[:, -1].cpu().numpy(), None, refs, lo, "OpenVLA sliced head", cap=0.0)
    # the pick is one of the kept tokens: wherever exactly three are kept it is among the alternatives, with the bits of its log-probability
    hit = tt == a_t[..., None]
    _check_pick_slot(a_top, a_t, a_lp, "sliced head")
    assert hit.any(dim=-1)[pad[..., 3]].all()


# ------------------------------------------------------------------------------------------------ 6. pi0-FAST
TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def _fast_inputs(dev, B=6, L=9, seed=5, n_prompts=None):
    """One frame for all rows; pairwise distinct prompts unless n_prompts (row b carries prompt b % n_prompts)."""
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    toks = torch.zeros(B, L, dtype=torch.long)
    pad = torch.zeros(B, L, dtype=torch.long)
    toks[:, :L - 2] = torch.randint(2, 500, (L - 2,), generator=g)
    toks[:, 0] = 2 + torch.arange(B) % (n_prompts or B)
    pad[:, :L - 2] = 1
    return [img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev)


def test_pi0fast_top_logprobs(dev):
    from cover_vla_amd.host import TopLogprobs, step_entropy_summary
    from cover_vla_amd.pi0fast import PI0FASTTokens
    sd = synth.pi0_state(TINY, seed=11)
    model = PI0FASTTokens(sd, TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, n_new, V, n = 6, 12, TINY["vocab"], 4
    args = _fast_inputs(dev, B)
    u = torch.rand(B, n_new, generator=torch.Generator().manual_seed(9)).to(dev)
    counted = [0, 0]
    for T, k, p in [(0.8, 50, 0.9), (1.0, 0, 1.0)]:
        kw = dict(uniforms=u, temperature=T, top_k=k, top_p=p, eos_token_id=-1)
        plain, plain_lp = model.generate_tokens(*args, n_new, return_logprobs=True, **kw)
        tr = {}
        out, lps, top = model.generate_tokens(*args, n_new, trace=tr, return_logprobs=True, top_logprobs=n, **kw)
        assert torch.equal(out, plain) and torch.equal(_bits(lps), _bits(plain_lp))
        assert isinstance(top, TopLogprobs) and tuple(top.tokens.shape) == (B, n_new, n) and tuple(top.logprobs.shape) == (B, n_new, n)
        assert tuple(top.entropy.shape) == (B, n_new) and top.tokens.dtype == torch.int64 and top.entropy.dtype == torch.float32
        _check_steps(top, tr["logits"], 0, V, n, T, k, p, f"pi0-FAST T={T} k={k} p={p}", counted)
        _check_pick_slot(top, out, lps, "pi0-FAST")
        out2, top2 = model.generate_tokens(*args, n_new, top_logprobs=n, **kw)                       # without return_logprobs
        assert torch.equal(out2, plain) and _same_top(top2, top)
        # pairwise distinct prompts: the shared-prefix path (one feedback launch per step) is the per-row path, bit for bit
        out3, lps3, top3 = model.generate_tokens(*args, n_new, return_logprobs=True, top_logprobs=n, share_prefix=True, **kw)
        assert torch.equal(out3, plain) and torch.equal(_bits(lps3), _bits(plain_lp)) and _same_top(top3, top)
    print(f"pi0-FAST: {counted[0]} of {counted[1]} rows counted")
    assert counted[0] >= (1 - R.CAP) * counted[1]
    # steps after a row's EOS: -1 / -inf / 0.0 on both paths; the steps up to it are reported
    kw = dict(uniforms=u, temperature=1.0, top_k=50, top_p=0.95)
    free = model.generate_tokens(*args, n_new, eos_token_id=-1, **kw).cpu()
    eos = int(free[0, 2])
    plain, plain_lp = model.generate_tokens(*args, n_new, eos_token_id=eos, return_logprobs=True, **kw)
    res = [model.generate_tokens(*args, n_new, eos_token_id=eos, return_logprobs=True, top_logprobs=n, share_prefix=share, **kw) for share in (False, True)]
    for out_e, lp_e, top_e in res:
        assert torch.equal(out_e, plain) and torch.equal(_bits(lp_e), _bits(plain_lp)) and _same_top(top_e, res[0][2])
    out_e, _, top_e = res[0]
    out_e, tt, tl, te = out_e.cpu(), top_e.tokens.cpu(), top_e.logprobs.cpu(), top_e.entropy.cpu()
    hit = 0
    for r in range(B):
        pos = (out_e[r] == eos).nonzero()
        first = int(pos[0]) if pos.numel() else n_new - 1
        hit += bool(pos.numel())
        assert (tt[r, first + 1:] == -1).all() and (tl[r, first + 1:] == NINF).all() and (te[r, first + 1:] == 0.0).all()
        assert (tt[r, :first + 1, 0] >= 0).all() and torch.isfinite(tl[r, :first + 1, 0]).all() and (te[r, :first + 1] > 0).all()
    assert hit >= 1
    mean, mx = step_entropy_summary(top_e.entropy, out_e, 0)
    assert tuple(mean.shape) == (B,) and (mean > 0).all() and (mx >= mean).all()
    # greedy: temperature 1, unfiltered, over the vocabulary; the de-duplicated call broadcasts its rows' alternatives
    args2 = _fast_inputs(dev, B, n_prompts=2)
    g_out, g_lp = model.generate_tokens(*args2, n_new, eos_token_id=-1, return_logprobs=True)
    tr = {}
    o, l, g_top = model.generate_tokens(*args2, n_new, eos_token_id=-1, trace=tr, return_logprobs=True, top_logprobs=n)
    assert torch.equal(o, g_out) and torch.equal(_bits(l), _bits(g_lp)) and tr["logits"][0].shape[0] == 2
    assert torch.equal(g_top.tokens[0], g_top.tokens[2]) and torch.equal(_bits(g_top.logprobs[1]), _bits(g_top.logprobs[5]))
    assert torch.equal(g_top.tokens[:, :, 0], g_out)                                                # the arg-max is rank 0
    assert torch.equal(_bits(g_top.logprobs[:, :, 0]), _bits(g_lp))
    _check_steps(TopLogprobs(g_top.tokens[:2], g_top.logprobs[:2], g_top.entropy[:2]), tr["logits"], 0, V, n, 1.0, 0, 1.0, "pi0-FAST greedy", [0, 0])


def test_pi0fast_policy_keeps_top_logprobs(dev):
    import types
    from cover_vla_amd.host import TopLogprobs
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
    for seed, with_lp in ((None, False), (7, True)):
        sampling = dict(temperature=1.0, top_k=50, top_p=0.95, sample_seed=seed)
        off = PI0FASTPolicy(PI0FASTConfig(return_logprobs=with_lp, **sampling, **kw), model, tok, fast)
        on = PI0FASTPolicy(PI0FASTConfig(return_logprobs=with_lp, top_logprobs=3, **sampling, **kw), model, tok, fast)
        assert on.last_top_logprobs is None
        a0, a1 = off.select_action(batch), on.select_action(batch)
        assert torch.equal(a0, a1) and off.last_top_logprobs is None
        top = on.last_top_logprobs
        assert isinstance(top, TopLogprobs) and tuple(top.tokens.shape) == (4, 24, 3) and tuple(top.entropy.shape) == (4, 24)
        assert (top.tokens[:, 0, 0] >= 0).all() and torch.isfinite(top.logprobs[:, 0, 0]).all() and (top.entropy >= 0).all()
        if with_lp:
            assert torch.equal(_bits(on.last_sequence_logprobs), _bits(off.last_sequence_logprobs))
