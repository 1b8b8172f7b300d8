"""The reference score of the per-row sampler without a device: the header's declarations, the ctypes mirror against a compiled probe of
include/cover_hip.h, the wrappers' host validation, and the float64 reference's self-consistency."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import logprob_ref as LR
from tests import ref_logprob_ref as RF
from tests import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "cover_hip.h")).read()


def test_header_declares_the_struct_and_both_entry_points():
    hdr = " ".join(_header().split())
    assert "typedef struct cover_token_ref {" in hdr and "} cover_token_ref;" in hdr
    assert ("int cover_token_sample_rows_ref(const cover_token_sample_rows_args* args, const cover_token_allow* allow /* NULL: unmasked */, "
            "const cover_token_ref* ref, void* stream);") in hdr
    assert ("int cover_decode_feedback_lp2(const cover_decode_feedback_args* args, const float* lp2, float* lp2_out, long long ld_lp2, "
            "void* stream);") in hdr
    assert "#define COVER_ABI_VERSION 1" in hdr
    # additions only: the structs the new calls reuse are declared before them, unchanged calls still there
    assert hdr.index("} cover_token_allow;") < hdr.index("typedef struct cover_token_ref {")
    assert hdr.index("int cover_decode_feedback(") < hdr.index("int cover_decode_feedback_lp2(")
    assert "int cover_token_sample_rows(const cover_token_sample_rows_args* args, void* stream);" in hdr


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cover_hip.h"
#define F(f) printf(#f " %zu\n", offsetof(cover_token_ref, f));
int main(void) {
    printf("sizeof %zu\n", sizeof(cover_token_ref));
    F(temperature) F(_pad) F(logprob_out)
    printf("abi %d\n", COVER_ABI_VERSION);
    printf("feedback %zu\n", sizeof(cover_decode_feedback_args));
    printf("rows %zu\n", sizeof(cover_token_sample_rows_args));
    return 0;
}
"""


def test_struct_mirror_matches_a_compiled_probe_of_the_header(tmp_path):
    from cover_vla_amd import _lib as L
    assert L._STRUCTS["cover_token_ref"] is L.TokenRef
    assert L.SYMBOLS["cover_token_sample_rows_ref"] == (C.c_int, [C.POINTER(L.TokenSampleRowsArgs), C.POINTER(L.TokenAllow), C.POINTER(L.TokenRef),
                                                                 C.c_void_p])
    assert L.SYMBOLS["cover_decode_feedback_lp2"] == (C.c_int, [C.POINTER(L.DecodeFeedbackArgs), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p])
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "a C compiler is needed to probe include/cover_hip.h"
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(_PROBE)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out.pop("abi")) == 1
    assert int(out.pop("feedback")) == C.sizeof(L.DecodeFeedbackArgs) and int(out.pop("rows")) == C.sizeof(L.TokenSampleRowsArgs)   # untouched
    assert int(out.pop("sizeof")) == C.sizeof(L.TokenRef) == 16
    assert list(out) == [f[0] for f in L.TokenRef._fields_]
    for name, _ in L.TokenRef._fields_:
        assert int(out[name]) == getattr(L.TokenRef, name).offset, name
    if os.path.exists(L.LIB_PATH):
        h = C.CDLL(L.LIB_PATH)
        assert hasattr(h, "cover_token_sample_rows_ref") and hasattr(h, "cover_decode_feedback_lp2")
        h.cover_sizeof.restype = C.c_size_t
        assert h.cover_sizeof(b"cover_token_ref") == C.sizeof(L.TokenRef)
        h.cover_abi_version.restype = C.c_int
        assert h.cover_abi_version() == 1


def test_wrapper_validation_needs_no_device(monkeypatch):
    from cover_vla_amd import _lib as L
    from cover_vla_amd import ops
    from cover_vla_amd._lib import CoverError

    def touched():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(L, "lib", touched)
    rows = 4
    x, u = torch.zeros(rows, 64), torch.zeros(rows)
    T = [1.0] * rows
    out = torch.zeros(rows)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), "warm", None):
        with pytest.raises(CoverError, match="ref_temperature"):
            ops.token_sample_rows(x, 0, 64, u, T, ref_temperature=bad, out_ref_logprob=out)
    with pytest.raises(CoverError, match="together"):
        ops.token_sample_rows(x, 0, 64, u, T, ref_temperature=1.0)
    for bad_out in (out.double(), torch.zeros(rows + 1), torch.zeros(rows, 1), torch.zeros(2 * rows)[::2], out.numpy()):
        with pytest.raises(CoverError, match="out_ref_logprob"):
            ops.token_sample_rows(x, 0, 64, u, T, ref_temperature=1.0, out_ref_logprob=bad_out)
    with pytest.raises(CoverError, match="device"):                          # valid arguments, host tensors: no CPU path
        ops.token_sample_rows(x, 0, 64, u, T, ref_temperature=1.0, out_ref_logprob=out)
    # pick_token: the reference belongs to the per-row call
    with pytest.raises(CoverError, match="row_params"):
        ops.pick_token(x, 0, 64, u, 1.0, (0, 1.0), ref=(1.0, out))
    with pytest.raises(CoverError, match="row_params"):
        ops.pick_token(x, 0, 64, None, ref=(1.0, out))
    with pytest.raises(CoverError, match="ref_temperature"):
        ops.pick_token(x, 0, 64, u, row_params=(T, None, None), ref=(0.0, out))
    # decode_feedback: the second column comes in pairs
    pick, done, tok = torch.zeros(rows, dtype=torch.int64), torch.zeros(rows, dtype=torch.bool), torch.zeros(rows, 3, dtype=torch.int64)
    for kw in (dict(lp2=torch.zeros(rows)), dict(lp2_out=torch.zeros(rows, 3))):
        with pytest.raises(CoverError, match="lp2 and lp2_out"):
            ops.decode_feedback(pick, done, tok, 0, 1, 0, **kw)


def test_new_arguments_default_to_off():
    from cover_vla_amd import ops
    from cover_vla_amd.openvla import OpenVLA
    from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTTokens
    p = inspect.signature(ops.token_sample_rows).parameters
    assert p["ref_temperature"].default is None and p["out_ref_logprob"].default is None
    assert inspect.signature(ops.pick_token).parameters["ref"].default is None
    p = inspect.signature(ops.decode_feedback).parameters
    assert p["lp2"].default is None and p["lp2_out"].default is None
    assert inspect.signature(OpenVLA.sample).parameters["prior_temperature"].default is None
    assert inspect.signature(PI0FASTTokens.generate_tokens).parameters["prior_temperature"].default is None
    assert PI0FASTConfig().prior_temperature is None


def test_reference_is_the_own_logprob_when_the_row_is_the_reference():
    """T_ref == T, unfiltered: the reference score of the row's own pick is that pick's own log-probability (the same float64 value), and
    it differs from it at another T_ref; a set restricts the mass to its columns."""
    x, u = R.lm_like_rows(7301, 6, 700, 5, 661)
    x, u = x.numpy(), u.numpy()
    lo, hi = 5, 661
    for r in range(x.shape[0]):
        for T in (1.0, 0.7, 2.0):
            own = LR.reference_logprob_row(x[r, lo:hi], u[r], T, 0, 1.0)
            t = own["token"]
            lp, xt = RF.reference_ref_logprob(x[r, lo:hi], t, T)
            assert lp == own["lp"][t] and xt == own["x"][t] and np.isfinite(lp) and lp < 0
            other, _ = RF.reference_ref_logprob(x[r, lo:hi], t, 2 * T)
            assert other != lp
    # by hand: two allowed columns with logits a > b, token b at T_ref: lp = (b - a) / T - log(1 + exp((b - a) / T))
    l = np.array([0.5, 3.0, -1.0, 2.0], dtype=np.float32)
    allowed = np.array([False, True, False, True])
    lp, xt = RF.reference_ref_logprob(l, 3, 0.5, allowed)
    assert xt == -2.0 and abs(lp - (-2.0 - np.log1p(np.exp(-2.0)))) < 1e-15
    # a filtered rung's own score is not the reference: top_k = 1 scores its pick 0.0, the reference does not
    own = LR.reference_logprob_row(x[0, lo:hi], u[0], 0.5, 1, 1.0)
    assert own["lp"][own["token"]] == 0.0 and RF.reference_ref_logprob(x[0, lo:hi], own["token"], 1.0)[0] < 0
