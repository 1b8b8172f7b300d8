"""Token grammars on the device: cover_decode_feedback_fsm against tests/fsm_ref.py and against cover_decode_feedback on the same
inputs (bit for bit: integers and the unchanged embedding arithmetic), the pick + feedback loop with no host round trip, its graph
replay, and pi0-FAST's generate_tokens(grammar=) on both feedback paths.

The two-kernel loop uses eos = {4}: the issue that introduced it named eos = {1} together with lo = 3, and an id below lo can never be
drawn, so "..., end, eos" could not be emitted at all. 4 keeps the EOS in the unaligned head word of [3, 297)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import host, ops, synth
from tests import fsm_ref as FR

pytestmark = pytest.mark.gpu

TINY = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
            vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)


def _bits(x):
    return x.contiguous().view(torch.int32)


class _env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("COVER_FAST_FEEDBACK")
        if self.value is None:
            os.environ.pop("COVER_FAST_FEEDBACK", None)
        else:
            os.environ["COVER_FAST_FEEDBACK"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("COVER_FAST_FEEDBACK", None)
        else:
            os.environ["COVER_FAST_FEEDBACK"] = self.old


# ------------------------------------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("dim", [8, 2048])
def test_feedback_fsm_matches_reference_and_plain_feedback(dev, dim):
    B, V, S, K, EOS, PAD = 7, 70, 6, 4, 1, 0
    rng = np.random.default_rng(dim)
    cls = rng.integers(0, K, V).astype(np.uint8)
    trans = rng.integers(0, S, (S, K)).astype(np.int32)
    sos = rng.integers(0, 5, S).astype(np.int32)
    fsm = ops.TokenFsm(cls, trans, sos)
    g = torch.Generator().manual_seed(dim)
    table = torch.randn(V, dim, generator=g).to(torch.bfloat16).to(dev)
    #        live  done  forced  -1  vocab  bad state  live, emits EOS
    pick0 = [17, 23, 5, -1, V, 40, EOS]
    force0 = [17, 23, 61, -1, V, 40, EOS]                     # row 2 is teacher-forced away from its pick
    done0 = [False, True, False, False, False, False, False]
    state0 = [2, 3, 0, 4, 5, S, 1]                              # row 5 enters with state n_states
    lp0 = -torch.rand(B, generator=g) - 0.01
    lp20 = -torch.rand(B, generator=g) - 0.01
    for use_force in (False, True):
        for use_lp2 in (False, True):
            for last in (False, True):                          # last: no x_out, the vocabulary size comes from the automaton alone
                res = {}
                for with_fsm in (False, True):
                    pick = torch.tensor(pick0, dtype=torch.int64, device=dev)
                    force = torch.tensor(force0, dtype=torch.int64, device=dev)
                    done = torch.tensor(done0, device=dev)
                    wide = torch.full((B, 9), -7, dtype=torch.int64, device=dev)          # ld_tok = 9, the step's column in the middle
                    lp_wide = torch.full((B, 5), 9.0, dtype=torch.float32, device=dev)    # ld_lp = 5
                    lp2_wide = torch.full((B, 6), 9.0, dtype=torch.float32, device=dev)
                    live = torch.zeros(4, dtype=torch.int32, device=dev)
                    xd = torch.full((B, dim), 3.0, dtype=torch.bfloat16, device=dev)
                    state = torch.tensor(state0, dtype=torch.int32, device=dev)
                    sor = torch.full((B,), 99, dtype=torch.int32, device=dev)
                    kw = dict(fsm=fsm, fsm_state=state, fsm_set_of_row=sor) if with_fsm else {}
                    if use_lp2:
                        kw.update(lp2=lp20.to(dev), lp2_out=lp2_wide)
                    ops.decode_feedback(pick, done, wide, 3, EOS, PAD, force=force if use_force else None, lp=lp0.to(dev), lp_out=lp_wide,
                                        table=table, scale=1.5, x_out=None if last else xd, live=live, **kw)
                    torch.cuda.synchronize()
                    res[with_fsm] = [t.cpu() for t in (wide, lp_wide, lp2_wide, done.view(torch.uint8), xd.view(torch.int16), live, state, sor)]
                what = (dim, use_force, use_lp2, last)
                for a, b in zip(res[False][:6], res[True][:6]):   # every output of cover_decode_feedback(_lp2), byte for byte
                    assert torch.equal(a, b) and a.dtype == b.dtype, what
                assert torch.equal(_bits(res[False][1]), _bits(res[True][1])) and torch.equal(_bits(res[False][2]), _bits(res[True][2])), what
                assert torch.equal(res[False][6], torch.tensor(state0, dtype=torch.int32)) and (res[False][7] == 99).all()
                emitted = res[True][0][:, 3].numpy()
                assert emitted.tolist() == [17, PAD, 61 if use_force else 5, -1, V, 40, EOS], what
                want_state = np.array(state0, dtype=np.int32)
                want_sor = FR.fsm_step(want_state, emitted, np.array(done0), cls, trans, sos)
                assert np.array_equal(res[True][6].numpy(), want_state) and np.array_equal(res[True][7].numpy(), want_sor), what
                # the cases the rows were chosen for: a finished row, ids outside the vocabulary and a bad state keep their state
                assert want_state[[1, 3, 4, 5]].tolist() == [3, 4, 5, S] and want_sor[5] == -1 and (want_sor[:5] >= 0).all()
                assert want_state[0] == trans[2, cls[17]] and want_state[6] == trans[1, cls[EOS]]
                if not last:
                    assert (res[True][4][[3, 4]] == 0).all() and not (res[True][4][0] == 0).all()
                assert (res[True][0][:, :3] == -7).all() and (res[True][0][:, 4:] == -7).all()


# ------------------------------------------------------------------------------------------------ 2. refused arguments
def test_feedback_fsm_refuses_bad_arguments(dev):
    B, V, dim, S, K = 6, 50, 256, 3, 2
    g = torch.Generator().manual_seed(4)
    table = torch.randn(V, dim, generator=g).to(torch.bfloat16).to(dev)
    pick = torch.randint(2, V, (B,), generator=g).to(dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    tok = torch.full((B, 1), -7, dtype=torch.int64, device=dev)
    xd = torch.full((B, dim), 3.0, dtype=torch.bfloat16, device=dev)
    lp = torch.zeros(B, device=dev)
    lp_out = torch.full((B, 1), 9.0, device=dev)
    cls = torch.zeros(V, dtype=torch.uint8, device=dev)
    trans = torch.ones(S, K, dtype=torch.int32, device=dev)
    sos = torch.tensor([4, 5, 6], dtype=torch.int32, device=dev)
    state = torch.zeros(B, dtype=torch.int32, device=dev)
    sor = torch.full((B,), 99, dtype=torch.int32, device=dev)

    def call(fsm_null=False, lp2=None, lp2_out=None, args=None, **over):
        a = L.DecodeFeedbackArgs()
        a.pick, a.done, a.tok_out, a.ld_tok, a.rows = pick.data_ptr(), done.data_ptr(), tok.data_ptr(), 1, B
        a.eos, a.pad = 1, 0
        a.table, a.vocab, a.dim, a.scale, a.x_out, a.ldo = table.data_ptr(), V, dim, 1.0, xd.data_ptr(), dim
        for k, v in (args or {}).items():
            setattr(a, k, v)
        f = L.TokenFsm()
        f.class_of_token, f.trans, f.set_of_state, f.n_states, f.n_classes = cls.data_ptr(), trans.data_ptr(), sos.data_ptr(), S, K
        f.state, f.set_of_row = state.data_ptr(), sor.data_ptr()
        for k, v in over.items():
            setattr(f, k, v)
        return L.lib().cover_decode_feedback_fsm(C.byref(a), None if fsm_null else C.byref(f), lp2, lp2_out, 1, torch.cuda.current_stream().cuda_stream)

    for over in (dict(class_of_token=None), dict(trans=None), dict(set_of_state=None), dict(state=None), dict(set_of_row=None),
                 dict(n_classes=257), dict(n_classes=0), dict(n_states=0), dict(fsm_null=True),
                 dict(lp2=lp.data_ptr()), dict(lp2_out=lp_out.data_ptr()),
                 dict(args=dict(pick=None)), dict(args=dict(dim=252)), dict(args=dict(vocab=0)), dict(args=dict(rows=-1)),
                 dict(args=dict(lp=lp.data_ptr())), dict(args=dict(x_out=None, table=None, dim=0, vocab=0))):
        assert call(**over) == -1, over                        # COVER_EINVAL
    torch.cuda.synchronize()
    assert (tok == -7).all() and (sor == 99).all() and (state == 0).all() and (xd == 3.0).all() and (lp_out == 9.0).all() and not done.any()
    assert call() == 0 and call(lp2=lp.data_ptr(), lp2_out=lp_out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(tok[:, 0], pick) and (state == 1).all() and (sor == 5).all() and (lp_out == 0.0).all()
    with pytest.raises(L.CoverError):
        ops.decode_feedback(pick, done, tok, 0, 1, 0, fsm=ops.TokenFsm(cls, trans, sos))                    # the three go together
    with pytest.raises(L.CoverError):
        ops.decode_feedback(pick, done, tok, 0, 1, 0, fsm=ops.TokenFsm(cls, trans, sos), fsm_state=state.long(), fsm_set_of_row=sor)
    with pytest.raises(L.CoverError):
        ops.decode_feedback(pick, done, tok, 0, 1, 0, table=table[:40].contiguous(), x_out=xd, fsm=ops.TokenFsm(cls, trans, sos), fsm_state=state,
                            fsm_set_of_row=sor)


# ------------------------------------------------------------------------------------------------ 3. pick + feedback, no host in between
ROWS, COLS, LO, HI, STEPS = 6, 300, 3, 297, 8
G_BODY, G_END, G_EOS, G_MIN, G_MAX, G_PAD = (40, 200), [210], [4], 2, 4, 0
LOOP_T = [1.0, 0.0, 0.8, 1.5, 1.0, 2.0]                          # row 1 is greedy
LOOP_K = [0, 0, 50, 0, 0, 0]                                     # row 2 is filtered (top-k and top-p)
LOOP_P = [1.0, 1.0, 0.9, 1.0, 0.7, 1.0]

_loop_cache = {}


def _loop_inputs(dev):
    """Logits drawn once per step with a large logit planted on the EOS and on a column of no class (20), uniforms, parameters, and the
    host-stepped result (set_of_row computed by tests/fsm_ref.py between launches): computed once, shared, never written to."""
    if _loop_cache:
        return _loop_cache
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(STEPS, ROWS, COLS, generator=g)
    logits[:, :, G_EOS[0]] = 30.0
    logits[:, :, 20] = 29.0
    u = torch.rand(STEPS, ROWS, generator=g)
    par = (torch.tensor(LOOP_T, device=dev), torch.tensor(LOOP_K, dtype=torch.int32, device=dev), torch.tensor(LOOP_P, device=dev))
    allow, fsm = host.length_grammar(COLS, G_BODY, G_END, G_EOS, G_MIN, G_MAX, device=dev)
    ops.token_fsm_check(fsm, allow, LO, HI)
    logits_d, u_d = logits.to(dev), u.to(dev)
    # the inputs have teeth: without the sets every row takes a planted column at once
    free, _, _ = ops.token_sample_rows(logits_d[0], LO, HI, u_d[0], *par)
    assert all(int(t) in (G_EOS[0], 20) for t in free.cpu())
    # host-stepped: plain feedback, tokens read back, the automaton of the reference, set_of_row uploaded
    cls, trans, _ = FR.length_tables(COLS, G_BODY, G_END, G_EOS, G_MIN, G_MAX)
    state = np.zeros(ROWS, dtype=np.int32)
    sor = torch.full((ROWS,), int(fsm.set_of_state_np[0]), dtype=torch.int32, device=dev)
    done = torch.zeros(ROWS, dtype=torch.bool, device=dev)
    out = torch.full((ROWS, STEPS), -5, dtype=torch.int64, device=dev)
    lps = torch.full((ROWS, STEPS), 9.0, device=dev)
    tsel, lp = torch.empty(ROWS, dtype=torch.int64, device=dev), torch.empty(ROWS, device=dev)
    for i in range(STEPS):
        ops.token_sample_rows(logits_d[i], LO, HI, u_d[i], *par, out_tok=tsel, out_logprob=lp, allow=ops.TokenAllow(allow.bits, sor))
        was = done.cpu().numpy().copy()
        ops.decode_feedback(tsel, done, out, i, G_EOS[0], G_PAD, lp=lp, lp_out=lps)
        sor.copy_(torch.from_numpy(FR.fsm_step(state, out[:, i].cpu().numpy(), was, cls, trans, fsm.set_of_state_np)).to(dev))
    _loop_cache.update(logits=logits_d, u=u_d, par=par, allow=allow, fsm=fsm, out=out.cpu(), lps=lps.cpu(), state=state.copy())
    return _loop_cache


def _full_match(row):
    """min..max body ids, the end id, the EOS, pad to the end: the whole regular expression, nothing cut off (STEPS >= G_MAX + 2)."""
    row = [int(t) for t in row]
    n = 0
    while n < len(row) and G_BODY[0] <= row[n] < G_BODY[1]:
        n += 1
    return G_MIN <= n <= G_MAX and row[n:n + 2] == [G_END[0], G_EOS[0]] and all(t == G_PAD for t in row[n + 2:])


def test_pick_and_feedback_loop_follows_the_grammar(dev):
    c = _loop_inputs(dev)
    fsm, allow = c["fsm"], c["allow"]
    state, sor = fsm.rows(ROWS, dev)
    assert (sor == int(fsm.set_of_state_np[0])).all()
    al = ops.TokenAllow(allow.bits, sor)
    done = torch.zeros(ROWS, dtype=torch.bool, device=dev)
    out = torch.full((ROWS, STEPS), -5, dtype=torch.int64, device=dev)
    lps = torch.full((ROWS, STEPS), 9.0, device=dev)
    tsel, lp = torch.empty(ROWS, dtype=torch.int64, device=dev), torch.empty(ROWS, device=dev)
    for i in range(STEPS):                                     # nothing is read back inside the loop
        ops.token_sample_rows(c["logits"][i], LO, HI, c["u"][i], *c["par"], out_tok=tsel, out_logprob=lp, allow=al)
        ops.decode_feedback(tsel, done, out, i, G_EOS[0], G_PAD, lp=lp, lp_out=lps, fsm=fsm, fsm_state=state, fsm_set_of_row=sor)
    torch.cuda.synchronize()
    out_c, lps_c = out.cpu(), lps.cpu()
    print("grammar loop rows:", out_c.tolist())
    assert torch.equal(out_c, c["out"]) and torch.equal(_bits(lps_c), _bits(c["lps"]))       # token for token, bit for bit
    assert np.array_equal(state.cpu().numpy(), c["state"]) and done.all()
    for r in range(ROWS):
        assert _full_match(out_c[r]), (r, out_c[r].tolist())
        assert FR.obeys_length_grammar(out_c[r].tolist(), G_BODY, G_END, G_EOS, G_PAD, G_MIN, G_MAX, COLS)
    assert torch.isfinite(lps_c).all() and (lps_c <= 0).all()
    # a token outside the current set scores -inf: the EOS under the start state's set
    start = ops.TokenAllow(allow.bits, fsm.rows(ROWS, dev)[1])
    eos_tok = torch.full((ROWS,), G_EOS[0], dtype=torch.int64, device=dev)
    assert (ops.token_logprob_rows(c["logits"][0], LO, HI, eos_tok, *c["par"], allow=start) == float("-inf")).all()
    lengths = {int((out_c[r] == G_END[0]).nonzero()[0]) for r in range(ROWS)}
    assert all(G_MIN <= n <= G_MAX for n in lengths)


def test_pick_and_feedback_step_replays_from_a_graph(dev):
    c = _loop_inputs(dev)
    fsm, allow = c["fsm"], c["allow"]
    state, sor = fsm.rows(ROWS, dev)
    al = ops.TokenAllow(allow.bits, sor)
    done = torch.zeros(ROWS, dtype=torch.bool, device=dev)
    out1 = torch.full((ROWS, 1), -5, dtype=torch.int64, device=dev)                       # the captured step's column
    lps1 = torch.full((ROWS, 1), 9.0, device=dev)
    out = torch.full((ROWS, STEPS), -5, dtype=torch.int64, device=dev)
    lps = torch.full((ROWS, STEPS), 9.0, device=dev)
    tsel, lp = torch.empty(ROWS, dtype=torch.int64, device=dev), torch.empty(ROWS, device=dev)
    lg, kept = torch.empty(ROWS, device=dev), torch.empty(ROWS, dtype=torch.int32, device=dev)
    x_s, u_s = c["logits"][0].clone(), c["u"][0].clone()                                  # the static inputs of the capture
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with ops.Graph() as gr:
            ops.token_sample_rows(x_s, LO, HI, u_s, *c["par"], out_tok=tsel, out_logit=lg, out_kept=kept, out_logprob=lp, allow=al)
            ops.decode_feedback(tsel, done, out1, 0, G_EOS[0], G_PAD, lp=lp, lp_out=lps1, fsm=fsm, fsm_state=state, fsm_set_of_row=sor)
        for i in range(STEPS):                                 # device copies only: nothing is read back between replays
            x_s.copy_(c["logits"][i])
            u_s.copy_(c["u"][i])
            gr.launch()
            out[:, i].copy_(out1[:, 0])
            lps[:, i].copy_(lps1[:, 0])
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(out.cpu(), c["out"]) and torch.equal(_bits(lps.cpu()), _bits(c["lps"]))
    assert np.array_equal(state.cpu().numpy(), c["state"])


# ------------------------------------------------------------------------------------------------ 4. pi0-FAST
M_BODY, M_END, M_EOS, M_PAD, M_MIN, M_MAX, N_NEW = (300, 380), [33], 1, 0, 2, 4, 8


def _inputs(dev, B, n_prompts, L=9, seed=5):
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(B, 1, 1, 1)
    lens = [L - (p * 2) % (L - 2) for p in range(n_prompts)]
    prompts = [torch.randint(2, 500, (lens[p],), generator=g) for p in range(n_prompts)]
    toks, pad = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        p = b % n_prompts
        prompts[p][0] = 2 + p
        toks[b, :lens[p]] = prompts[p]
        pad[b, :lens[p]] = 1
    return [img.to(dev)], [torch.ones(B, dtype=torch.bool, device=dev)], toks.to(dev), pad.to(dev)


def _model_ok(row):
    row = [int(t) for t in row]
    n = 0
    while n < len(row) and M_BODY[0] <= row[n] < M_BODY[1]:
        n += 1
    return M_MIN <= n <= M_MAX and row[n:n + 2] == [M_END[0], M_EOS] and all(t == M_PAD for t in row[n + 2:])


def test_pi0fast_grammar(dev):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    model = PI0FASTTokens(synth.pi0_state(TINY, seed=11), TINY, device="cuda:0", max_batch=8, max_prompt=9, max_new_tokens=16)
    B, V = 6, TINY["vocab"]
    shared = _inputs(dev, B, n_prompts=2)                       # P = 2 < B = 6
    own = _inputs(dev, B, n_prompts=B)                          # P = B
    g = torch.Generator().manual_seed(9)
    u = torch.rand(B, N_NEW, generator=g).to(dev)
    T = np.array([1.5, 0.0, 1.5, 2.0, 1.5, 1.2], dtype=np.float32)           # a ladder with one greedy row
    k = np.array([0, 0, 50, 0, 0, 0], dtype=np.int32)
    p = np.array([1.0, 1.0, 0.9, 1.0, 0.8, 1.0], dtype=np.float32)
    gram = host.length_grammar(V, M_BODY, M_END, [M_EOS], M_MIN, M_MAX, device=dev)
    samp = dict(uniforms=u, temperature=T, top_k=k, top_p=p, eos_token_id=M_EOS, pad_token_id=M_PAD)
    scal = dict(uniforms=u, temperature=1.5, top_k=0, top_p=1.0, eos_token_id=M_EOS, pad_token_id=M_PAD)
    before = model.generate_tokens(*shared, N_NEW, share_prefix=True, return_logprobs=True, **samp)
    before_own = model.generate_tokens(*own, N_NEW, return_logprobs=True, **scal)
    # the inputs have teeth: without a grammar at least one row is not "2..4 body, end, eos, pad..."
    assert not all(_model_ok(r) for r in before[0].cpu()), before[0].cpu().tolist()
    force = torch.tensor([[310, 311, 33, 1, 0, 0, 0, 0]] * B)
    force[0, 0] = M_EOS                                         # a forced EOS outside the start state's set: the row ends, the state stays
    force[1, :] = torch.tensor([310, 5, 311, 312, 313, 33, 1, 0])                        # a forced id of no class in the middle
    cases = [("ladder", dict(samp)), ("scalar", dict(scal)), ("greedy", dict(eos_token_id=M_EOS, pad_token_id=M_PAD)),
             ("forced", dict(samp, force_tokens=force))]
    for name, kw in cases:
        res = {}
        for mode in ("0", None):                                # the torch statements, then the fused launch (read per call)
            with _env(mode):
                tr = {}
                extra = {} if name == "greedy" else dict(prior_temperature=1.3)
                r = model.generate_tokens(*shared, N_NEW, share_prefix=True, return_logprobs=True, top_logprobs=2, trace=tr, grammar=gram,
                                          **extra, **kw)
            res[mode] = [t.cpu() for t in r[:-1]] + [r[-1].tokens.cpu(), torch.stack([kk.cpu() for kk in tr["kept"]])]
        for a, b in zip(res["0"], res[None]):                   # tokens, log-probabilities, reference log-probabilities, top-n, kept: identical
            assert torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(_bits(a), _bits(b)), name
        tok, lps = res[None][0], res[None][1]
        print(f"pi0-FAST grammar {name}:", tok.tolist())
        if name == "forced":
            assert tok[0].tolist() == [M_EOS] + [M_PAD] * 7 and (lps[0, 1:] == 0.0).all()
            assert torch.equal(tok[1:], force[1:]) and torch.isfinite(lps).all()
            kept = res[None][-1]                                 # [steps, B]: an unfiltered or greedy row keeps its whole set, so kept names the state
            assert kept[:, 3].tolist() == [80, 80, 81, 1, 1, 1, 1, 1]           # body, body, body or end, eos; FINISHED draws from eos too
            assert kept[:, 1].tolist() == [80, 80, 80, 81, 81, 1, 1, 1]         # the id of no class (5) moves nothing: four body ids still fit
            assert kept[:, 0].tolist() == [80] * 8                              # the forced EOS is no move of state 0, and a finished row stays
            continue
        for r in range(B):
            assert _model_ok(tok[r]), (name, r, tok[r].tolist())
        assert torch.isfinite(lps).all()
        top = res[None][-2]                                      # [B, steps, 2]: step 0 ranks body ids only
        assert ((top[:, 0] >= M_BODY[0]) & (top[:, 0] < M_BODY[1])).all()
    # P == B: the shared path reproduces the per-row path bit for bit (test_prefix_share_gpu.py's singleton criterion), grammar included
    a = model.generate_tokens(*own, N_NEW, return_logprobs=True, grammar=gram, **samp)
    b = model.generate_tokens(*own, N_NEW, return_logprobs=True, share_prefix=True, grammar=gram, **samp)
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and all(_model_ok(r) for r in a[0].cpu())
    # P < B: rows of one prompt with equal uniforms and parameters agree; the state is per row (different uniforms diverge)
    slot = [0, 1] * 3
    u_same = u[:2][slot]
    s = model.generate_tokens(*shared, N_NEW, share_prefix=True, grammar=gram, **dict(scal, uniforms=u_same)).cpu()
    assert all(torch.equal(s[r], s[slot[r]]) for r in range(B)) and all(_model_ok(r) for r in s)
    d = model.generate_tokens(*shared, N_NEW, share_prefix=True, grammar=gram, **scal).cpu()
    assert len({tuple(d[r].tolist()) for r in range(0, B, 2)}) > 1 and all(_model_ok(r) for r in d)
    # refused on the host
    with pytest.raises(ValueError):
        model.generate_tokens(*shared, N_NEW, grammar=gram, allowed_tokens=gram.allow, **scal)
    with pytest.raises(L.CoverError):
        model.generate_tokens(*shared, N_NEW, grammar=host.length_grammar(V + 1, M_BODY, M_END, [M_EOS], 1, 2, device=dev), **scal)
    dead = host.TokenGrammar(ops.TokenAllow(torch.zeros_like(gram.allow.bits.view(torch.int32)).view(torch.uint32)), gram.fsm)
    with pytest.raises(L.CoverError, match="state 0 "):
        model.generate_tokens(*shared, N_NEW, grammar=dead, **scal)
    # grammar=None is what it was before any grammar ran
    after = model.generate_tokens(*shared, N_NEW, share_prefix=True, return_logprobs=True, **samp)
    after_own = model.generate_tokens(*own, N_NEW, return_logprobs=True, **scal)
    assert torch.equal(after[0], before[0]) and torch.equal(_bits(after[1]), _bits(before[1]))
    assert torch.equal(after_own[0], before_own[0]) and torch.equal(_bits(after_own[1]), _bits(before_own[1]))


def test_policy_token_grammar(dev):
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTPolicy, PI0FASTTokens, fast_chunk_grammar
    model = PI0FASTTokens(synth.pi0_state(TINY, seed=11), TINY, device="cuda:0", max_batch=8, max_prompt=384, max_new_tokens=24)
    tok = synth.CharTokenizer(vocab_size=512)
    fast = types.SimpleNamespace(bpe_tokenizer=types.SimpleNamespace(decode=lambda t: "".join(chr(max(0, min(int(i), 1000))) for i in t)),
                                 min_token=-40, scale=10.0)
    g = torch.Generator().manual_seed(2)
    batch = {"observation.state": (torch.rand(3, 8, generator=g) * 2 - 1).to(dev), "task": ["pick up the cube", "open the drawer", "pick up the cube"],
             "observation.images.top": (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(3, 1, 1, 1).to(dev)}
    base = dict(resize_imgs_with_padding=(56, 56), max_decoding_steps=8, chunk_size=4, n_action_steps=2, action_dim=3, sample_seed=4,
                temperature=1.3, top_k=0, top_p=1.0)
    bar = 3 + ord("|")
    gram = fast_chunk_grammar(PI0FASTConfig(**base), 2, 5, vocab_size=512, fast_vocab_size=60, end_token_id=bar, eos_token_id=tok.eos_token_id,
                              device=dev)
    a, b = 512 - 128 - 60, 512 - 128
    assert gram.fsm.n_states == 8 and gram.allow.n_sets == 4
    seen = {}
    orig = model.generate_tokens

    def spy(*args, **kw):
        seen["kw"], seen["out"] = kw, orig(*args, **kw)
        return seen["out"]

    model.generate_tokens = spy
    for share in (False, True):
        pol = PI0FASTPolicy(PI0FASTConfig(token_grammar=gram, share_prefix=share, **base), model, tok, fast)
        assert tuple(pol.select_action(dict(batch)).shape) == (3, 3) and seen["kw"]["grammar"] is gram and "allowed_tokens" not in seen["kw"]
        for row in seen["out"].cpu().tolist():
            n = 0
            while n < len(row) and a <= row[n] < b:
                n += 1
            assert 2 <= n <= 5 and row[n:n + 2] == [bar, tok.eos_token_id] and all(t == tok.pad_token_id for t in row[n + 2:]), row
    PI0FASTPolicy(PI0FASTConfig(**base), model, tok, fast).select_action(dict(batch))
    assert "grammar" not in seen["kw"]
    with pytest.raises(ValueError):
        PI0FASTPolicy(PI0FASTConfig(token_grammar=gram, allowed_token_ranges=[(a, b)], **base), model, tok, fast)
