"""The pi0-FAST de-tokeniser without a GPU: the reference of tests/fast_decode_ref.py against the reference implementation's golden
and against pi0fast.fast_coefficients_to_actions within a derived bound, the host helpers, the binding, and every precondition
ops.fast_decode checks before a launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cover_vla_amd import host, ops
from cover_vla_amd._lib import CoverError
from tests import fast_decode_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


def _basis(H):
    return host.fast_idct_basis(H)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_matches_the_reference_golden():
    z = np.load(os.path.join(GOLD, "pi0fast_dct_decode.npz"))
    seqs = [z["seq0"], z["seq1"], z["seq2"]]
    assert [len(s) for s in seqs] == [28, 20, 35]                          # fits 4 x 7 exactly, is padded, is truncated
    n_pieces = int(max(s.max() for s in seqs)) + 1
    pieces = [[i] for i in range(n_pieces)]                                # the identity table: FAST id i is the symbol i
    band = (500 - n_pieces, 500)
    tokens = np.zeros((3, 36), dtype=np.int64)                             # pad = 0 after the terminator 50
    for i, s in enumerate(seqs):
        tokens[i, :len(s)] = band[1] - 1 - s
        tokens[i, len(s)] = 50
    kw = dict(band=band, stop_ids=(50, 1, 0), min_token=int(z["min_token"]), scale=float(z["scale"]), horizon=4, action_dim=7)
    assert kw["min_token"] == -20 and kw["scale"] == 10.0
    got = FR.reference(tokens, pieces, _basis(4), **kw)
    assert got["n_symbols"].tolist() == [28, 20, 35] and got["status"].tolist() == [0, FR.PADDED, FR.TRUNCATED]
    assert np.array_equal(got["coeff"][0], seqs[0] - 20) and np.array_equal(got["coeff"][2], seqs[2][:28] - 20)
    assert np.array_equal(got["coeff"][1], np.concatenate([seqs[1] - 20, np.zeros(8, dtype=np.int64)]))
    err = np.abs(got["actions"].astype(np.float64) - z["actions"])
    bound = FR.error_bound(got["coeff"], 10.0, 4, 7)
    assert (err <= bound).all() and err.max() > 0, (err.max(), bound.max())
    strict = FR.reference(tokens, pieces, _basis(4), relaxed=False, **kw)
    assert strict["status"].tolist() == [0, FR.MISMATCH, FR.MISMATCH] and not strict["actions"][1:].any()
    assert np.array_equal(strict["actions"][0].view(np.int32), got["actions"][0].view(np.int32))


@pytest.mark.parametrize("H,D", [(1, 1), (4, 7), (50, 32), (64, 7), (128, 32)])
def test_reference_against_the_host_decoder_within_the_derived_bound(H, D):
    from cover_vla_amd.pi0fast import fast_coefficients_to_actions
    rng = np.random.default_rng(H * 100 + D)
    HD, n_pieces, min_token, scale = H * D, 600, -300, 10.0               # |q| <= 300
    pieces = [[i] for i in range(n_pieces)]
    band = (2000 - n_pieces, 2000)
    lens = [HD, max(HD - 5, 0), HD + 9, max(HD // 2, 1)]
    fast = [rng.integers(0, n_pieces, size=n) for n in lens]
    L = max(lens) + 1
    tokens = np.zeros((len(lens), L), dtype=np.int64)
    for i, f in enumerate(fast):
        tokens[i, :len(f)] = band[1] - 1 - f
        tokens[i, len(f)] = 50
    got = FR.reference(tokens, pieces, _basis(H), band=band, stop_ids=(50, 1, 0), min_token=min_token, scale=scale, horizon=H, action_dim=D)
    want = fast_coefficients_to_actions([f.tolist() for f in fast], lambda t: "".join(chr(i) for i in t), min_token=min_token, scale=scale,
                                        time_horizon=H, action_dim=D)
    assert want.dtype == np.float64 and want.shape == (len(lens), H, D) and got["actions"].dtype == F32
    err = np.abs(got["actions"].astype(np.float64) - want)
    bound = FR.error_bound(got["coeff"], scale, H, D)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"H={H} D={D}: worst error / bound = {ratio:.3f}, worst error {err.max():.3e}")
    assert (err <= bound).all(), ratio
    if HD > 1:
        assert np.abs(want).max() > 1.0                                    # not a comparison of zeros


def test_status_bits_on_the_constructed_rows():
    names, tokens, relaxed, strict, coeffs = FR.status_rows()
    basis = _basis(FR.STATUS_H)
    got = FR.reference(tokens, FR.STATUS_PIECES, basis, **FR.status_kwargs(True))
    assert dict(zip(names, got["status"].tolist())) == dict(zip(names, relaxed))
    for i, want in enumerate(coeffs):
        q = [0] * 6 if want is None else [s + FR.STATUS_MIN_TOKEN for s in want] + [0] * (6 - len(want))
        assert got["coeff"][i].tolist() == q, names[i]
        if want is None:
            assert got["actions"][i].view(np.int32).tolist() == [[0] * 3] * 2, names[i]    # +0.0f, not -0.0f
    assert got["n_symbols"].tolist() == [0, 6, 3, 6, 6, 6, 6, 6, 8, 6, 7, 1]
    got = FR.reference(tokens, FR.STATUS_PIECES, basis, **FR.status_kwargs(False))
    assert dict(zip(names, got["status"].tolist())) == dict(zip(names, strict))
    zero = [i for i, s in enumerate(strict) if s & FR.FATAL]
    assert len(zero) == 9 and not got["coeff"][zero].any() and not got["actions"][zero].any()
    assert got["coeff"][names.index("exact fit")].tolist() == [s + FR.STATUS_MIN_TOKEN for s in (13, 14, 15, 11, 12, 10)]


def test_random_case_rows_reach_every_kind():
    H, D = 4, 7
    pieces = FR.case_pieces(H, D)
    assert sorted({len(p) for p in pieces if p is not None}) == list(range(10)) + [H * D + 3] and pieces[FR.N_SHORT] is None
    seen = 0
    for L in FR.LENGTHS:
        st = FR.reference(FR.case_tokens(5, L, H, D), pieces, _basis(H), **FR.case_kwargs(H, D))["status"]
        for s in st:
            seen |= int(s)
        if L > 1:
            assert st[3] & FR.STRAY and st[4] & FR.UNDECODABLE and st[1] & FR.NO_TERMINATOR and not st[0] & FR.FATAL
    assert seen == 63 - FR.MISMATCH                                        # relaxed never reports a mismatch
    strict = FR.reference(FR.case_tokens(5, 65, H, D), pieces, _basis(H), **FR.case_kwargs(H, D, relaxed=False))
    assert (strict["status"] & FR.MISMATCH).all() and not strict["actions"].any()


# ------------------------------------------------------------------------------------------------ host helpers
@pytest.mark.parametrize("H", [1, 2, 4, 50, 128])
def test_idct_basis_is_scipys_to_fp32_rounding(H):
    from scipy.fft import idct
    b = host.fast_idct_basis(H)
    want = idct(np.eye(H), axis=0, norm="ortho")
    assert b.dtype == F32 and b.shape == (H, H)
    assert np.abs(b.astype(np.float64) - want).max() <= 2.0 ** -24 * np.abs(want).max() + 1e-15    # half an ulp of the largest entry
    assert np.array_equal(b, FR.basis64(H).astype(F32))
    assert np.allclose(b.astype(np.float64) @ b.astype(np.float64).T, np.eye(H), atol=1e-5)


def test_idct_basis_rejects_bad_sizes():
    for bad in (0, 129, -1, 4.0, True, None):
        with pytest.raises(ValueError):
            host.fast_idct_basis(bad)


def test_pieces_from_a_decoder_that_raises():
    def decode(ids):
        (f,) = ids
        if f in (2, 5):
            raise KeyError(f)
        return "" if f == 3 else "ab" * f + chr(0x1F600)
    pieces = host.fast_pieces_from_decoder(decode, 7)
    assert pieces[2] is None and pieces[5] is None and pieces[3] == [] and pieces[0] == [0x1F600]
    assert pieces[1] == [97, 98, 0x1F600] and len(pieces) == 7 and len(pieces[6]) == 13
    with pytest.raises(ValueError):
        host.fast_pieces_from_decoder(decode, 0)
    assert "concatenation" in host.fast_pieces_from_decoder.__doc__
    tab = ops.fast_piece_table(pieces)
    assert tab.n_pieces == 7 and tab.piece_off.dtype == torch.int32 and tab.piece_off.tolist() == [0, 1, 4, 5, 5, 14, 15, 28]
    assert tab.piece_sym[4].item() == -1 and tab.piece_sym[14].item() == -1 and not tab.piece_sym.is_cuda


def test_piece_table_checks():
    for bad in ([], None, "ab", [[-1]], [[0x110000]], [[1.5]], [[True]], [[0]] * 3 + [[1] * ((1 << 18) - 2)]):
        with pytest.raises(CoverError):
            ops.fast_piece_table(bad)
    empty = ops.fast_piece_table([[], []])                                 # only empty pieces: still a pointer for the kernel
    assert empty.n_pieces == 2 and empty.piece_off.tolist() == [0, 0, 0] and empty.piece_sym.numel() == 1
    assert ops.fast_piece_table(["ab", (99,), np.array([5, 6])]).piece_sym.tolist() == [97, 98, 99, 5, 6]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    for off, sym in (([0], [1]), ([1, 2], [1, 2]), ([0, 2, 1], [1, 2]), ([0, 3], [1, 2]), ([0, 2], [1, -1]), ([0, 1], [0x110000])):
        with pytest.raises(CoverError):
            ops.FastPieces(i32(off), i32(sym))
    with pytest.raises(CoverError):
        ops.FastPieces(torch.tensor([0, 1]), i32([1]))                     # int64 offsets
    with pytest.raises(CoverError):
        ops.FastPieces(i32([0, 0]), i32([]))
    assert ops.FastPieces(i32([0, 1, 2]), i32([-1, 7])).n_pieces == 2


# ------------------------------------------------------------------------------------------------ binding
def test_binding_mirrors_the_header():
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_fast_decode_args"] is L.FastDecodeArgs
    assert L.SYMBOLS["cover_fast_decode"] == (C.c_int, [C.POINTER(L.FastDecodeArgs), C.c_void_p])
    hdr = open(os.path.join(ROOT, "include", "cover_hip.h")).read()
    assert "int cover_fast_decode(const cover_fast_decode_args* args, void* stream);" in hdr
    body = hdr[hdr.index("typedef struct cover_fast_decode_args {"):hdr.index("} cover_fast_decode_args;")]
    body = re.sub(r"/\*.*?\*/", "", body)
    pos = [re.search(rf"\b{name}\b", body).start() for name, _ in L.FastDecodeArgs._fields_]   # the header's fields in the header's order
    assert pos == sorted(pos)
    assert C.sizeof(L.FastDecodeArgs) == 248
    for name, bit in (("TRUNCATED", 1), ("PADDED", 2), ("MISMATCH", 4), ("STRAY", 8), ("UNDECODABLE", 16), ("NO_TERMINATOR", 32)):
        assert f"#define COVER_FAST_{name} {bit}\n" in hdr and getattr(ops, f"FAST_{name}") == bit == getattr(FR, name)
    csrc = os.path.join(ROOT, "cover_vla_amd", "csrc")
    text = open(os.path.join(csrc, "fast_decode.hip")).read()
    assert "#pragma clang fp contract(off)" in text and "atomic" not in text.lower() and "cosf" not in text and "fmaf" not in text
    assert " fast_decode.hip " in open(os.path.join(csrc, "Makefile")).read()
    capi = open(os.path.join(csrc, "capi.hip")).read()
    assert "SZ(cover_fast_decode_args)" in capi and "int cover_fast_decode(" in capi
    if os.path.exists(L.LIB_PATH):                                         # cover_sizeof and cover_abi_version are host code: no GPU call
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_fast_decode")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_fast_decode_args") == C.sizeof(L.FastDecodeArgs)
        assert h.cover_sizeof(b"cover_diverse_args") == C.sizeof(L.DiverseArgs) and h.cover_abi_version() == 1


# ------------------------------------------------------------------------------------------------ the wrapper's checks
def test_fast_decode_rejects_bad_arguments_before_any_launch():
    H, D = 4, 7
    tokens = torch.zeros(3, 12, dtype=torch.int64)
    pieces = ops.fast_piece_table([[i] for i in range(10)])
    basis = torch.from_numpy(_basis(H))
    ok = dict(band=(100, 110), stop_ids=(50, 1, 0), skip_ids=(60, 61, 2), min_token=-20, scale=10.0, horizon=H, action_dim=D)
    nan, inf = float("nan"), float("inf")
    bad = [
        (dict(tokens=tokens.to(torch.int32)), "int64"), (dict(tokens=tokens[0]), "int64"), (dict(tokens=tokens.numpy()), "int64"),
        (dict(tokens=torch.zeros(3, 4097, dtype=torch.int64)), "L <= 4096"), (dict(tokens=torch.zeros(0, 4, dtype=torch.int64)), "1 <= B"),
        (dict(tokens=torch.zeros(3, 0, dtype=torch.int64)), "1 <= L"),
        (dict(pieces=(pieces.piece_off, pieces.piece_sym)), "FastPieces"), (dict(pieces=None), "FastPieces"),
        (dict(horizon=0), "horizon"), (dict(horizon=129), "horizon"), (dict(horizon=4.0), "integers"), (dict(horizon=True), "integers"),
        (dict(action_dim=0), "action_dim"), (dict(action_dim=33), "action_dim"), (dict(action_dim=7.0), "integers"),
        (dict(min_token=-20.0), "integers"), (dict(min_token=(1 << 30) + 1), "min_token"),
        (dict(basis=torch.zeros(4, 5)), "basis"), (dict(basis=basis.double()), "basis"), (dict(basis=basis.numpy()), "basis"),
        (dict(basis=torch.zeros(8, 8)[::2, ::2]), "basis"), (dict(horizon=5), "basis"),
        (dict(band=(110, 100)), "band"), (dict(band=(-1, 5)), "band"), (dict(band=100), "band"), (dict(band=(100.0, 110)), "integers"),
        (dict(stop_ids=(1, 2, 3, 4, 5)), "stop_ids"), (dict(stop_ids=5), "stop_ids"), (dict(stop_ids=(1.0,)), "stop_ids"),
        (dict(skip_ids=tuple(range(9))), "skip_ids"), (dict(skip_ids=("a",)), "skip_ids"),
        (dict(scale=0.0), "scale"), (dict(scale=nan), "scale"), (dict(scale=inf), "scale"), (dict(scale=1e-60), "scale"),
        (dict(scale=1e60), "scale"), (dict(scale="10"), "scale"), (dict(scale=True), "scale"),
        (dict(relaxed=1), "relaxed"), (dict(relaxed=None), "relaxed"),
        (dict(out=torch.zeros(3, 4, 8)), "out must"), (dict(out=torch.zeros(3, 4, 7, dtype=torch.float64)), "out must"),
        (dict(out=torch.zeros(3, 7, 4).transpose(1, 2)), "out must"), (dict(out=torch.zeros(1, 4, 7).expand(3, 4, 7)), "overlap"),
        (dict(out=torch.zeros(3, 1, 7).expand(3, 4, 7)), "overlap"),
    ]
    for over, word in bad:
        kw = dict(ok, tokens=tokens, pieces=pieces, basis=basis)
        kw.update(over)
        t, p, b = kw.pop("tokens"), kw.pop("pieces"), kw.pop("basis")
        with pytest.raises(CoverError, match=re.escape(word)):
            ops.fast_decode(t, p, b, **kw)
    # everything in order but the device: there is no CPU path, and nothing is launched
    with pytest.raises(CoverError, match="no CPU path"):
        ops.fast_decode(tokens, pieces, basis, **ok)
    with pytest.raises(CoverError, match="no CPU path"):                   # a step-major view and a view of a wider buffer pass the checks
        ops.fast_decode(torch.zeros(12, 3, dtype=torch.int64).t(), pieces, basis, out=torch.zeros(3, 6, 32)[:, :4, :7], stats=True, **ok)
    with pytest.raises(TypeError):
        ops.fast_decode(tokens, pieces, basis, **{k: v for k, v in ok.items() if k != "scale"})    # no default scale


def test_policy_config_defaults_leave_the_host_path():
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTPolicy
    cfg = PI0FASTConfig()
    assert cfg.device_detokenize is False and cfg.fast_vocab_size is None and cfg.action_end_token_id is None
    assert tuple(cfg.action_format_token_ids) == ()
    assert "not" in PI0FASTPolicy.extract_actions_device.__doc__.lower() and "BOS" in PI0FASTPolicy.extract_actions_device.__doc__
