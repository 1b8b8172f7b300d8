"""The pi0-FAST de-tokeniser on the GPU: cover_fast_decode against the reference of tests/fast_decode_ref.py -- the coefficients, symbol
counts and status bits exactly, the actions bit for bit (every rounding is specified, so there is no tolerance) -- at the shapes that reach
each code path, through both token layouts and a strided output, under graph replay, and in PI0FASTPolicy end to end."""
import os
import types

import numpy as np
import pytest
import torch

from cover_vla_amd import graphs, host, ops, synth
from tests import fast_decode_ref as FR
from tests import smooth_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("actions", "coeff", "n_symbols", "status")
SENTINEL_BITS = 0x7FC12345          # a NaN payload no result carries
F32 = np.float32


def _bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int32) if x.dtype == np.float32 else x


def _assert_same(got, want, what, keys=KEYS):
    for k in keys:
        g, w = _bits(got[k]), _bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k, got[k], want[k])


def _basis(H, dev):
    return torch.from_numpy(host.fast_idct_basis(H)).to(dev)


def _decode(tokens, pieces, basis, dev, layout="rows", **kw):
    """ops.fast_decode on host tokens int64 [B, L], laid out candidate-major or step-major on the device -> dict of KEYS."""
    t = torch.from_numpy(tokens).to(dev)
    if layout == "steps":
        t = t.t().contiguous().t()                                         # a [L, B] buffer, read through its transposed view
        assert t.shape == tokens.shape and (t.stride() == (1, tokens.shape[0]) or 1 in tokens.shape)
    return ops.fast_decode(t, pieces, basis, stats=True, **kw)._asdict()


# ------------------------------------------------------------------------------------------------ 1. every shape
@pytest.mark.parametrize("L", FR.LENGTHS)
@pytest.mark.parametrize("H,D", FR.SHAPES, ids=lambda v: str(v))
def test_matches_reference_bit_for_bit(dev, H, D, L):
    host_pieces = FR.case_pieces(H, D)
    pieces, basis = ops.fast_piece_table(host_pieces, dev), _basis(H, dev)
    for B in (1, 5):
        tokens = FR.case_tokens(B, L, H, D)
        for relaxed in (True, False):
            kw = FR.case_kwargs(H, D, relaxed)
            want = FR.reference(tokens, host_pieces, basis.cpu().numpy(), **kw)
            got = _decode(tokens, pieces, basis, dev, **kw)
            _assert_same(got, want, (B, L, H, D, relaxed))
            _assert_same(_decode(tokens, pieces, basis, dev, layout="steps", **kw), want, (B, L, H, D, relaxed, "step-major"))
        plain = ops.fast_decode(torch.from_numpy(tokens).to(dev), pieces, basis, **FR.case_kwargs(H, D))        # stats=False: the same bits
        assert torch.is_tensor(plain) and np.array_equal(_bits(plain), _bits(FR.reference(tokens, host_pieces, basis.cpu().numpy(),
                                                                                              **FR.case_kwargs(H, D))["actions"]))


def test_constructed_status_rows(dev):
    names, tokens, relaxed, strict, coeffs = FR.status_rows()
    pieces, basis = ops.fast_piece_table(FR.STATUS_PIECES, dev), _basis(FR.STATUS_H, dev)
    for flag, expect in ((True, relaxed), (False, strict)):
        kw = FR.status_kwargs(flag)
        got = _decode(tokens, pieces, basis, dev, **kw)
        assert dict(zip(names, got["status"].tolist())) == dict(zip(names, expect))
        _assert_same(got, FR.reference(tokens, FR.STATUS_PIECES, basis.cpu().numpy(), **kw), f"relaxed={flag}")
        zero = [i for i, s in enumerate(expect) if s & FR.FATAL]
        assert zero and not _bits(got["actions"])[zero].any() and not got["coeff"][zero].any()    # +0.0f in every cell
    fit = names.index("exact fit")
    assert got["coeff"][fit].tolist() == [s + FR.STATUS_MIN_TOKEN for s in coeffs[fit]] and got["actions"][fit].abs().max() > 0


def test_output_into_the_first_columns_of_a_wider_buffer(dev):
    H, D, B, L = 50, 7, 5, 65
    host_pieces = FR.case_pieces(H, D)
    pieces, basis = ops.fast_piece_table(host_pieces, dev), _basis(H, dev)
    tokens = FR.case_tokens(B, L, H, D)
    buf = torch.empty(B, 50, 32, dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(SENTINEL_BITS)
    out = ops.fast_decode(torch.from_numpy(tokens).to(dev), pieces, basis, out=buf[:, :, :D], **FR.case_kwargs(H, D))
    assert out.data_ptr() == buf.data_ptr() and out.stride() == (50 * 32, 32, 1)
    want = FR.reference(tokens, host_pieces, basis.cpu().numpy(), **FR.case_kwargs(H, D))
    assert np.array_equal(_bits(buf[:, :, :D]), _bits(want["actions"])) and want["actions"].any()
    assert bool((buf.view(torch.int32)[:, :, D:] == SENTINEL_BITS).all())  # nothing else was touched
    # a buffer with more steps than the horizon: the steps beyond it keep the sentinel too
    tall = torch.empty(B, 60, 32, dtype=torch.float32, device=dev)
    tall.view(torch.int32).fill_(SENTINEL_BITS)
    ops.fast_decode(torch.from_numpy(tokens).to(dev), pieces, basis, out=tall[:, :H, :D], **FR.case_kwargs(H, D))
    assert np.array_equal(_bits(tall[:, :H, :D]), _bits(want["actions"]))
    assert bool((tall.view(torch.int32)[:, H:] == SENTINEL_BITS).all()) and bool((tall.view(torch.int32)[:, :, D:] == SENTINEL_BITS).all())


def test_reference_golden_through_the_kernel(dev):
    z = np.load(os.path.join(ROOT, "tests", "golden", "pi0fast_dct_decode.npz"))
    seqs = [z["seq0"], z["seq1"], z["seq2"]]
    n_pieces = int(max(s.max() for s in seqs)) + 1
    band = (500 - n_pieces, 500)
    tokens = np.zeros((3, 36), dtype=np.int64)
    for i, s in enumerate(seqs):
        tokens[i, :len(s)] = band[1] - 1 - s
        tokens[i, len(s)] = 50
    pieces = ops.fast_piece_table([[i] for i in range(n_pieces)], dev)     # the identity table
    got = _decode(tokens, pieces, _basis(4, dev), dev, band=band, stop_ids=(50, 1, 0), min_token=-20, scale=10.0, horizon=4, action_dim=7)
    assert got["n_symbols"].tolist() == [28, 20, 35] and got["status"].tolist() == [0, FR.PADDED, FR.TRUNCATED]
    err = np.abs(got["actions"].cpu().numpy().astype(np.float64) - z["actions"])
    assert (err <= FR.error_bound(got["coeff"].cpu().numpy(), 10.0, 4, 7)).all()


# ------------------------------------------------------------------------------------------------ 2. graph replay
def test_graph_replay_follows_the_token_buffer(dev):
    H, D, B, L = 4, 7, 5, 65
    host_pieces = FR.case_pieces(H, D)
    pieces, basis = ops.fast_piece_table(host_pieces, dev), _basis(H, dev)
    kw = FR.case_kwargs(H, D)
    tok = torch.zeros(L, B, dtype=torch.int64, device=dev)                 # the decode graph's step-major buffer
    out = torch.empty(B, H, D, dtype=torch.float32, device=dev)
    out.view(torch.int32).fill_(SENTINEL_BITS)
    g, ret = graphs.capture(lambda: ops.fast_decode(tok.t(), pieces, basis, out=out, **kw), dev)
    torch.cuda.synchronize()
    assert ret is out and bool((out.view(torch.int32) == SENTINEL_BITS).all())     # the capture itself executed nothing
    seen = []
    for k in range(2):
        tokens = FR.case_tokens(B, L, H, D, seed=7 + k)
        tok.copy_(torch.from_numpy(tokens).to(dev).t())                    # the tokens overwritten in place
        out.view(torch.int32).fill_(SENTINEL_BITS)
        g.launch()
        torch.cuda.synchronize()
        want = FR.reference(tokens, host_pieces, basis.cpu().numpy(), **kw)
        assert np.array_equal(_bits(out), _bits(want["actions"])), k
        seen.append(_bits(out).tobytes())
    assert len(set(seen)) == 2                                             # the replays had different answers


# ------------------------------------------------------------------------------------------------ 3. the policy
@pytest.fixture(scope="module")
def policy_case(dev):
    from cover_vla_amd.pi0fast import PI0FASTTokens
    tiny = dict(lm_dim=256, lm_mlp=512, ex_dim=128, ex_mlp=256, layers=2, Hq=4, Hkv=1, D=64, vocab=512, vit_dim=128, vit_mlp=200,
                vit_layers=2, vit_heads=4, patch=14, image=56, chunk=4)
    model = PI0FASTTokens(synth.pi0_state(tiny, seed=11), tiny, device="cuda:0", max_batch=8, max_prompt=384, max_new_tokens=24)
    tok = synth.CharTokenizer(vocab_size=512)
    decode = lambda t: "".join(chr(max(0, min(int(i), 1000))) for i in t)
    fast = types.SimpleNamespace(bpe_tokenizer=types.SimpleNamespace(decode=decode), min_token=-40, scale=10.0)
    g = torch.Generator().manual_seed(2)
    state = (torch.rand(1, 8, generator=g) * 2 - 1).repeat(4, 1)
    img = (torch.rand(1, 3, 56, 56, generator=g) * 2 - 1).repeat(4, 1, 1, 1)
    batch = {"observation.state": state.to(dev), "observation.images.top": img.to(dev), "task": ["put the spoon on the towel", "open drawer"] * 2}
    return model, tok, fast, batch, state, img


FAST_VOCAB = 256
FORMAT_IDS = tuple(3 + ord(ch) for ch in "Action:")                        # the stand-in tokenizer's ids of the format characters
END_ID = 3 + ord("|")


def _policy_ref(toks, tok, fast, cfg):
    """The reference applied to generated tokens, then select_action's slicing and un-normalisation (identity here)."""
    band = (tok.vocab_size - cfg.fast_skip_tokens - FAST_VOCAB, tok.vocab_size - cfg.fast_skip_tokens)
    pieces = host.fast_pieces_from_decoder(fast.bpe_tokenizer.decode, FAST_VOCAB)
    return FR.reference(toks.cpu().numpy(), pieces, host.fast_idct_basis(cfg.chunk_size), band=band,
                        stop_ids=(END_ID, tok.eos_token_id, tok.pad_token_id), skip_ids=FORMAT_IDS + (tok.bos_token_id,), min_token=fast.min_token,
                        scale=fast.scale, horizon=cfg.chunk_size, action_dim=cfg.action_dim, relaxed=cfg.relaxed_action_decoding)


@pytest.mark.parametrize("restricted", (False, True), ids=("free", "band-only"))
def test_policy_select_action_on_the_device(dev, policy_case, restricted):
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTPolicy
    model, tok, fast, batch, state, img = policy_case
    base = dict(action_dim=7, chunk_size=5, n_action_steps=2, max_decoding_steps=24, resize_imgs_with_padding=(56, 56))
    if restricted:     # the model may only emit the band, "|" and EOS: the rows decode to chunks, not to the zeros of a stray id
        base["allowed_token_ranges"] = [(512 - 128 - FAST_VOCAB, 512 - 128), (END_ID, END_ID + 1)]
    on_cfg = PI0FASTConfig(device_detokenize=True, fast_vocab_size=FAST_VOCAB, action_end_token_id=END_ID, action_format_token_ids=FORMAT_IDS, **base)
    on = PI0FASTPolicy(on_cfg, model, tok, fast)
    a0 = on.select_action(dict(batch))
    chunks, status = on.last_chunks, on.last_decode_status
    assert tuple(chunks.shape) == (4, 5, 7) and chunks.dtype == torch.float32 and chunks.is_cuda
    assert tuple(status.shape) == (4,) and status.dtype == torch.int32 and status.is_cuda
    ids, mask = on.create_input_tokens(state.to(dev), batch["task"])
    extra = dict(allowed_tokens=on.allowed_tokens) if restricted else {}
    toks = model.generate_tokens([img.to(dev)], [torch.ones(4, dtype=torch.bool, device=dev)], ids.to(dev), mask.to(dev), 24,
                                 eos_token_id=tok.eos_token_id, pad_token_id=tok.pad_token_id, **extra)
    want = _policy_ref(toks, tok, fast, on_cfg)
    assert np.array_equal(_bits(chunks), _bits(want["actions"])) and np.array_equal(status.cpu().numpy(), want["status"])
    assert np.array_equal(_bits(a0), _bits(want["actions"][:, 0, :7]))
    assert np.array_equal(_bits(on.select_action(dict(batch))), _bits(want["actions"][:, 1, :7]))       # the queue's second step
    if restricted:
        assert not (want["status"] & FR.FATAL).any() and np.abs(want["actions"]).max() > 0
        # a candidate-row family runs in place on the chunks: the geometry pi0-FAST rows were missing
        scores = torch.linspace(-1, 1, 4, device=dev)
        dim_scale, radius = (1.0, 1.0, 0.75, 0.5, 0.5, 0.25), 0.5 * float(np.sqrt(5))
        sm, st = ops.smooth_scores_actions(chunks[..., :7], scores, 4, radius=radius, dim_scale=dim_scale, shrink=0.5, stats=True)
        ref = SR.reference(chunks.cpu().numpy(), scores.cpu().numpy(), 4, dim_scale, radius, 0.5, 1)
        assert np.array_equal(_bits(sm), _bits(ref["smoothed"])) and np.array_equal(st.neighbours.cpu().numpy(), ref["neighbours"])
    # the flag off: the host path, the same as a policy built without the new fields
    off = PI0FASTPolicy(PI0FASTConfig(device_detokenize=False, fast_vocab_size=FAST_VOCAB, action_end_token_id=END_ID, **base), model, tok, fast)
    plain = PI0FASTPolicy(PI0FASTConfig(**base), model, tok, fast)
    assert torch.equal(off.select_action(dict(batch)), plain.select_action(dict(batch)))
    assert off.last_chunks is None and off.last_decode_status is None and plain.last_chunks is None
    with pytest.raises(ops.L.CoverError, match="device_detokenize"):
        plain.extract_actions_device(toks)
    with pytest.raises(ValueError, match="fast_vocab_size"):
        PI0FASTPolicy(PI0FASTConfig(device_detokenize=True, **base), model, tok, fast)
