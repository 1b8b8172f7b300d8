"""Host bookkeeping of the PaliGemma prefix that pi0 and pi0-FAST share (cover_vla_amd/paligemma.py) and of pi0's sample_actions
steps that run before any launch: the row-grouping rule, the prefix plan, the camera-pattern partition and the normalisation pair.
CPU tensors only; nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from cover_vla_amd.paligemma import IDENTITY, normalize_state, row_groups, unnormalize_action
from cover_vla_amd.pi0 import PI0FlowMatching
from cover_vla_amd.pi0fast import prefix_groups
from tests.test_prefix_share_cpu import _rows


# ------------------------------------------------------------------------------------------------ row_groups
def test_row_groups_first_occurrence_and_reconstruction():
    a, b, c = [9, 8, 7], [1, 2], [5, 5, 5, 5]
    tok, pad = _rows(a, b, a, c, b, a, c)                       # `a` sorts last but occurs first
    first, slot = row_groups(tok, pad)
    assert first.tolist() == [0, 1, 3] and slot.tolist() == [0, 1, 0, 2, 1, 0, 2]
    assert first.dtype == np.int64 and slot.dtype == np.int64
    assert np.array_equal(tok[first][slot], tok) and np.array_equal(pad[first][slot], pad)
    # a [B] column in front (pi0's frame class) splits rows that agree in everything else
    first, slot = row_groups(np.array([0, 0, 1, 0, 0, 0, 0]), torch.from_numpy(tok), torch.from_numpy(pad).bool())
    assert first.tolist() == [0, 1, 2, 3] and slot.tolist() == [0, 1, 2, 3, 1, 0, 3]
    with pytest.raises(ValueError):
        row_groups(tok, pad[:3])


def test_row_groups_pad_mask_difference_splits_rows():
    tok = np.array([[4, 5, 0], [4, 5, 0], [4, 5, 0]], dtype=np.int64)
    pad = np.array([[1, 1, 0], [1, 1, 1], [1, 1, 0]], dtype=np.int64)     # row 1: the trailing 0 is a real token
    first, slot = row_groups(tok, pad)
    assert first.tolist() == [0, 1] and slot.tolist() == [0, 1, 0]


def test_row_groups_equals_prefix_groups():
    g = np.random.default_rng(11)
    cases = [_rows([9, 8, 7], [1, 2], [9, 8, 7], [5, 5, 5, 5], [1, 2])]
    tok = g.integers(0, 50, size=(5, 4))[g.integers(0, 5, size=33)]      # many repeats
    cases.append((tok, np.ones_like(tok)))
    tok = g.permutation(40 * 6).reshape(40, 6).astype(np.int64)          # all rows distinct
    cases.append((tok, np.ones_like(tok)))
    cases.append((np.tile(tok[:1], (7, 1)), np.ones((7, 6), dtype=np.int64)))   # one group
    for tok, pad in cases:
        for got, want in zip(row_groups(tok, pad), prefix_groups(tok, pad)):
            assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ pi0: _prefix_plan
B, L = 6, 8


def _model(max_prompts=8):
    """A PI0FlowMatching with the fields the host steps read and nothing on a device."""
    m = PI0FlowMatching.__new__(PI0FlowMatching)
    m.dev, m.max_prompts = torch.device("cpu"), max_prompts
    return m


def _prompts(lens=(3, 5, 3, 5, 2, 3)):
    """B right-padded prompts; rows of equal length carry equal tokens."""
    tok, mask = torch.zeros(B, L, dtype=torch.int64), torch.zeros(B, L, dtype=torch.bool)
    for b, n in enumerate(lens):
        tok[b, :n] = torch.arange(1, n + 1) * (10 + n)
        mask[b, :n] = True
    return tok, mask


def _frames(distinct_rows=()):
    """One camera; the rows named carry a second frame. A frame has at most one non-zero pixel, so the float64 fingerprint of
    _image_classes (a matrix product, whose summation order over a row is the BLAS library's) is exact whatever that order is."""
    im = torch.zeros(B, 3, 4, 4)
    for r in distinct_rows:
        im[r, 0, 0, 0] = 1.0
    return [im]


def _key(plan_inputs, img_class):
    tok, mask = plan_inputs
    return np.concatenate([np.asarray(img_class)[:, None], tok.numpy(), mask.numpy().astype(np.int64)], axis=1)


def test_prefix_plan_frame_classes_and_group_consistency():
    m = _model()
    tok, mask = _prompts()
    one = m._prefix_plan(_frames(), tok, mask)
    assert one.ic_first.tolist() == [0] and one.ic_of_group.tolist() == [0] * one.U and one.U == 3
    assert one.first_row.tolist() == [0, 1, 4] and one.prompt_of_row.tolist() == [0, 1, 0, 1, 2, 0]
    two = m._prefix_plan(_frames(distinct_rows=(2, 5)), tok, mask)       # rows 2 and 5: a second frame under prompt 0's tokens
    assert two.ic_first.tolist() == [0, 2] and two.U == 4
    assert two.first_row.tolist() == [0, 1, 2, 4] and two.ic_of_group.tolist() == [0, 0, 1, 0]
    for plan, cls in ((one, [0] * B), (two, [0, 0, 1, 0, 0, 1])):
        key = _key((tok, mask), cls)
        assert np.array_equal(key[plan.first_row.numpy()][plan.prompt_of_row.numpy()], key)
        assert plan.prompt_of_row.dtype == torch.int64 and plan.first_row.dtype == torch.int64
    with pytest.raises(ValueError):                                       # more distinct pairs than prefix slots
        _model(max_prompts=3)._prefix_plan(_frames(distinct_rows=(2, 5)), tok, mask)


def test_prefix_plan_calls_image_classes_through_the_instance():
    m = _model()
    m._image_classes = lambda cams, B_: np.arange(B_, dtype=np.int64)    # what test_fullsize_gpu.py does: every row its own frame
    plan = m._prefix_plan(_frames(), *_prompts())
    assert plan.U == B and plan.ic_first.tolist() == list(range(B)) and plan.prompt_of_row.tolist() == list(range(B))


def test_prefix_plan_trims_trailing_pad_only(monkeypatch):
    m = _model()
    tok, mask = _prompts()
    plan = m._prefix_plan(_frames(), tok, mask)
    assert (plan.Lg, plan.Lfull) == (5, L)                               # the longest prompt
    holes = mask.clone()
    holes[0, 1] = False                                                   # not a contiguous run from column 0
    plan = m._prefix_plan(_frames(), tok, holes)
    assert (plan.Lg, plan.Lfull) == (L, L)
    monkeypatch.setenv("COVER_PI0_TRIM_PAD", "0")
    plan = m._prefix_plan(_frames(), tok, mask)
    assert (plan.Lg, plan.Lfull) == (L, L)


# ------------------------------------------------------------------------------------------------ pi0: camera patterns
def test_camera_parts_partition_rows_by_pattern():
    on = torch.ones(B, dtype=torch.bool)
    mixed = on.clone()
    mixed[1::2] = False
    parts = PI0FlowMatching._camera_parts([on, mixed], B)
    assert sorted(cams for _, cams in parts) == [[0], [0, 1]]
    rows = np.concatenate([r for r, _ in parts])
    assert sorted(rows.tolist()) == list(range(B))                        # disjoint and covering
    for r, cams in parts:
        assert r.tolist() == ([0, 2, 4] if cams == [0, 1] else [1, 3, 5])
    assert [(r.tolist(), c) for r, c in PI0FlowMatching._camera_parts([on, ~on], B)] == [(list(range(B)), [0])]
    none = mixed.clone()
    with pytest.raises(ValueError):                                       # rows 1, 3, 5 have no camera at all
        PI0FlowMatching._camera_parts([none, mixed], B)
    with pytest.raises(ValueError):
        PI0FlowMatching._camera_parts([on[:3]], B)


# ------------------------------------------------------------------------------------------------ normalisation pair
def test_normalisation_pair_formulas_and_round_trip():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 7, generator=g)
    mean, std = torch.randn(7, generator=g) * 0.1, torch.rand(7, generator=g) + 0.5
    lo, hi = -torch.rand(7, generator=g) - 0.5, torch.rand(7, generator=g) + 0.5
    assert normalize_state(x, IDENTITY) is x and unnormalize_action(x, IDENTITY) is x
    ms = ("MEAN_STD", mean, std)
    assert torch.equal(normalize_state(x, ms), (x - mean) / (std + 1e-8))                 # normalize.py:169
    assert torch.equal(unnormalize_action(x, ms), x * std + mean)                         # :243
    mm = ("MIN_MAX", lo, hi)
    assert torch.equal(normalize_state(x, mm), (x - lo) / (hi - lo + 1e-8) * 2 - 1)       # :177-179
    assert torch.equal(unnormalize_action(x, mm), (x + 1) / 2 * (hi - lo) + lo)           # :250-251
    for t in (ms, mm):      # fp32: a few ulps of the statistics' range
        assert torch.allclose(unnormalize_action(normalize_state(x, t), t), x, atol=1e-5)
    with pytest.raises(ValueError):
        normalize_state(x, ("MEDIAN", mean, std))
