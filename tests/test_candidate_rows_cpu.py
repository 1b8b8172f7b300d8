"""The checks the six families over candidate rows share (augment, proposal prior, refine, smooth, coherence, diverse; ops._Rows and the
checkers beside it): every condition is refused with CoverError by both forms of every family that has it. The inputs are the smallest
of the families' own tables -- 6 rows, 2 steps, 255 centres -- on the CPU, so a call that is in order ends at "there is no CPU path":
that case is part of the table, it shows that each other case holds exactly one fault."""
import pytest
import torch

X = torch.zeros(6, 2, 7)
TOK = torch.zeros(6, 14, dtype=torch.int64)
CEN = torch.zeros(255)
S6 = torch.zeros(6)
ONES = [1.0] * 6
NAMES = {"augment": "augment", "proposal_prior": "proposal_prior", "refine": "refine", "smooth": "smooth_scores", "coherence": "coherence_prior",
         "diverse": "diverse_subset"}
BASE = {
    "augment": dict(n_samples=3, n_augmented=1, normals=torch.zeros(2, 1, 2, 6)),
    "proposal_prior": dict(group_rows=3, n_fit=2, sigma=1.0, sd_floor=0.1),
    "refine": dict(scores=S6, group_rows=3, n_elite=2, n_new=1, normals=torch.zeros(2, 1, 2, 6)),
    "smooth": dict(scores=S6, group_rows=3, radius=0.1, dim_scale=ONES),
    "coherence": dict(group_rows=3, ref=torch.zeros(3, 4, 7), ref_weight=torch.ones(3), step_weight=torch.ones(2), dim_scale=ONES),
    "diverse": dict(group_rows=3, keep=2, quality=S6, weight=0.5, step_weight=torch.ones(2), dim_scale=ONES),
}
OUT_ROWS = {"augment": 8, "proposal_prior": None, "refine": 6, "smooth": None, "coherence": None}   # gathered rows; None: fp32 [6]
GROUPED = ("proposal_prior", "refine", "smooth", "coherence", "diverse")
FORMS = ("tokens", "actions")


def _call(family, form, **over):
    from cover_vla_amd import ops
    kw = dict(BASE[family], **over)
    steps, centers = kw.pop("steps", 2), kw.pop("centers", CEN)
    if form == "tokens":
        return getattr(ops, NAMES[family] + "_tokens")(TOK, centers=centers, tok_vocab=32000, steps=steps, **kw)
    return getattr(ops, NAMES[family] + "_actions")(X, **kw)


def _strided_out(family, form):
    """A tensor of the output's dtype and shape that is not contiguous."""
    R = OUT_ROWS[family]
    shape, dtype = ((6,), torch.float32) if R is None else (((R, 14), torch.int64) if form == "tokens" else ((R, 2, 7), torch.float32))
    return torch.zeros(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]


def _cases():
    both = lambda fams: [(f, form) for f in fams for form in FORMS]
    for f, form in both(BASE):
        yield "in_order_but_on_the_cpu", f, form, {}, "no CPU path"
    for f, form in both(GROUPED):
        yield "group_rows_not_an_integer", f, form, dict(group_rows=3.0), "group_rows must be integers"
        yield "rows_not_a_multiple", f, form, dict(group_rows=4), "rows % group_rows == 0"
    for form in FORMS:
        yield "rows_not_a_multiple", "augment", form, dict(n_samples=4), "rows % n_samples == 0"
    for f in BASE:
        yield "steps_beyond_the_columns", f, "tokens", dict(steps=3), "7 \\* steps <= columns"
        yield "centers_not_fp32", f, "tokens", dict(centers=CEN.double()), "centers must be contiguous fp32"
    for f, form in both(("refine", "smooth")):
        yield "scores_float64", f, form, dict(scores=S6.double()), "scores must be contiguous fp32"
    for form in FORMS:
        yield "scores_float64", "diverse", form, dict(quality=S6.double()), "quality must be contiguous fp32"
    for f, form in both(OUT_ROWS):
        yield "out_not_contiguous", f, form, dict(out=_strided_out(f, form)), "out must be a contiguous"
    for f, form in both(("smooth", "coherence", "diverse")):
        yield "dim_scale_of_five", f, form, dict(dim_scale=[1.0] * 5), "dim_scale must have 6 entries"
    # tensors on two devices cannot be expressed without a device: every CPU tensor is refused before the devices are compared


CASES = list(_cases())


@pytest.mark.parametrize("cond,family,form,over,msg", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in CASES])
def test_shared_conditions_are_refused_by_every_family(cond, family, form, over, msg):
    from cover_vla_amd._lib import CoverError
    if "out" in over:
        assert not over["out"].is_contiguous()
    with pytest.raises(CoverError, match=msg):
        _call(family, form, **over)


def test_the_table_covers_the_twelve_wrappers():
    from cover_vla_amd import ops
    assert {(f, form) for _, f, form, _, _ in CASES} == {(f, form) for f in BASE for form in FORMS} and len(BASE) == 6
    assert all(callable(getattr(ops, f"{NAMES[f]}_{form}")) for f in BASE for form in FORMS)
    rows = ops._action_rows("x", X)
    assert rows.out_shape(5) == (5, 2, 7) and ops._token_rows("x", TOK, 2, CEN, 32000).out_shape(5) == (5, 14)
    with pytest.raises(AttributeError):
        rows.N = 7                                                         # the record is immutable
