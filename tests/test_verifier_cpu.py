"""The verifier heads are written once, in the batched form, and a lone member is a stack of one (cover_vla_amd/verifier.py::_Stack). At
batch 1 the fp32 GEMM never dereferences through a batch stride, but its plan (cover_gemm_f32_plan: no launch, no GPU) reads their low bits,
so the strides a stack of one passes must leave every GEMM of the heads on the kernel the unbatched call (all batch strides 0) runs on.

The heads run here on CPU tensors with the library replaced by a recorder that keeps every cover_gemm_f32 argument block and launches
nothing (the outputs are never-read empties); the plans are then asked of the real library with aligned fake pointers."""
import pytest
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import ops, synth
from tests import f32_ref as R


class _Recorder:
    """Stands in for the loaded library: keeps the argument block of every fp32 GEMM, answers success to every other entry."""

    def __init__(self):
        self.gemms = []

    def cover_gemm_f32(self, ref, stream):
        self.gemms.append({f: getattr(ref._obj, f) for f, _ in L.GemmF32Args._fields_})
        return 0

    def __getattr__(self, name):
        if not name.startswith("cover_"):
            raise AttributeError(name)
        return lambda *a: 0


def _head_gemms(use_transformer, num_patches, rows):
    """Argument blocks of every GEMM of one member's heads on `rows` (image, text, history) triples, through the public single-model class."""
    from cover_vla_amd.verifier import VLASigLIP2Bridge
    L.lib()                                                   # the real library (its absence is an error, not a reason to record)
    ck = synth.verifier_checkpoint(1, use_transformer=use_transformer, num_patches=num_patches)
    pf, tf, hist = synth.verifier_batch_inputs(rows, num_patches=num_patches)
    rec = _Recorder()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(L, "lib", lambda: rec)
        mp.setattr(ops, "_chk_dev", lambda *ts: None)
        mp.setattr(ops, "_stream", lambda: None)
        net = VLASigLIP2Bridge(ck["ensemble_components"][0], device="cpu")
        net.forward_features(pf, tf, hist)
    return rec.gemms


@pytest.mark.parametrize("rows", [1, 32], ids=["NT10", "NT320"])
@pytest.mark.parametrize("num_patches", [576, 16])
@pytest.mark.parametrize("use_transformer", [True, False], ids=["transformer", "mlp"])
def test_stack_of_one_keeps_the_plan_of_the_unbatched_gemm(use_transformer, num_patches, rows):
    gemms = _head_gemms(use_transformer, num_patches, rows)
    heads = [g for g in gemms if (g["a_batch_stride"], g["b_batch_stride"], g["c_batch_stride"]) != (0, 0, 0)]
    # per (image, text) pair: similarity + attended features + 2 poolings x (K/V + 4 blocks x 4) + input projection; per batch of histories:
    # 1 + 4 layers x 4 (transformer) or 2 (MLP); the two logit GEMMs behind them are plain unbatched calls
    assert len(heads) == rows * (2 + 2 * (1 + 4 * 4) + 1) + (1 + 4 * 4 if use_transformer else 2)
    assert len(gemms) == len(heads) + 2
    plans = set()
    for g in gemms:
        assert g["batch"] == 1
        args = (R.FAKE_A, g["a_row_stride"], g["a_k_stride"], R.FAKE_B, g["b_row_stride"], g["b_k_stride"], R.FAKE_C, g["c_row_stride"],
                g["M"], g["N"], g["K"])
        passed = ops.gemm_f32_plan(*args, batch=1, a_bs=g["a_batch_stride"], b_bs=g["b_batch_stride"], c_bs=g["c_batch_stride"])
        assert passed == ops.gemm_f32_plan(*args, batch=1), g
        plans.add(passed[0])
    assert "DIRECT_FM1" in plans                              # the k-contiguous nn.Linear of the heads do reach the kernel the strides could lose
