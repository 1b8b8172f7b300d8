"""What the two token samplers share (OpenVLA.sample, PI0FASTTokens.generate_tokens): the resolved sampling mode of a call (PickPlan),
its one pick per step and the per-step output buffers (StepOutputs). "Row" below is a candidate of sample / a batch row of
generate_tokens, R their number, S the number of steps, "the range" the columns a model picks over (its docstring names them).

uniforms fp32 [R, S] in [0, 1): column i drives step i's inverse-CDF draw at `temperature`, filtered by top_k / top_p after the temperature
in the order and with the meaning of Hugging Face's `generate(do_sample=True, top_k, top_p)` (0 / 1.0 = off). None = greedy; the three are unused.
Parameters per row: temperature, top_k and top_p each accept a scalar or a length-R sequence / tensor (host.sampling_ladder builds them).
All scalars is the scalar path, untouched. As soon as one of the three is per row, all three are validated on the host (temperature >= 0,
top_k >= 0, top_p > 0, all finite, else CoverError; a device tensor of any numeric dtype is read back once for it, so no pick is ever the
-1 of an invalid row), broadcast to fp32 / int32 / fp32 [R] device tensors (ops.row_param_tensors) and every step's pick is ONE
ops.token_sample_rows launch over the range (ops.pick_token(row_params=)): uniforms is then required, a row with temperature 0 is greedy
(the arg-max over the range, scored at temperature 1 unfiltered; its uniforms are not read).
return_logprobs: a fp32 [R, S] tensor, the log-probability of each step's own pick under the distribution it was drawn from (sampled:
temperature, top_k, top_p over the range; greedy: temperature 1, unfiltered; per-row mode: that launch's log-probability). With
force_tokens it is still the path's own picks that are scored. The default launches exactly what it launched without the argument.
top_logprobs = n in 1..64: appends host.TopLogprobs(tokens int64 [R, S, n], logprobs fp32 [R, S, n], entropy fp32 [R, S]) to the return:
per step the n most probable tokens of the distribution return_logprobs documents (descending logit, equal logits by ascending id; -1 /
-inf where it keeps fewer than n), their log-probabilities (cover_token_logprob's, bit for bit) and its entropy in nats -- one
ops.token_topn launch per step on the logits the pick used (per-row mode: ops.token_topn_rows). 0: today's launches.
prior_temperature = T_ref (> 0, finite): the return gains a fp32 [R, S] tensor (after the return_logprobs tensor if present, before
TopLogprobs): the log-probability of each pick under ONE reference distribution for every row -- temperature T_ref, unfiltered, over the
range (over the row's allowed set where there is one) -- written by the pick's own launch (cover_token_sample_rows_ref;
ops.token_logprob_rows at (T_ref, 0, 1) on the pick, bit for bit). It is the prior that compares across the rungs of a ladder:
return_logprobs scores every row under its own rung. Scalar parameters are broadcast and the per-row path is taken (the only one that carries
the reference); uniforms is required: a greedy candidate is a row with temperature 0. None launches exactly what it launched before.
The deterministic alternative to drawing -- the B most probable distinct sequences per prompt -- is OpenVLA.beam_search; it takes none of the above.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import ops
from .host import TopLogprobs


class PickPlan(NamedTuple):
    """The resolved sampling mode of one call. Rows mode (rp set): every pick is the per-row launch and temperature / filt are None."""
    greedy: bool                          # no uniforms
    temperature: Optional[float]          # the scalar temperature
    filt: Optional[Tuple[int, float]]     # None = the unfiltered ops.token_select pick; (top_k, top_p) = ops.token_sample
    rp: Optional[tuple]                   # (temperature fp32, top_k int32, top_p fp32) device tensors [rows]
    allow: Optional[ops.TokenAllow]       # rp is then set
    t_ref: Optional[float]                # rp is then set
    n_top: int

    @classmethod
    def resolve(cls, what, unit, rows, device, *, has_uniforms, params, top_logprobs=0, prior_temperature=None, allow=None, filter_always):
        """The checks and promotions of a call `what` whose rows are called `unit`; params = (temperature, top_k, top_p).
        filter_always: a sampled scalar call is ops.token_sample also with filters that filter nothing (pi0-FAST); False: top_k <= 0 and
        top_p >= 1 is the unfiltered ops.token_select pick (OpenVLA). Rows mode is taken if a parameter is per row, prior_temperature is
        given or allow is given: scalars are then broadcast, with allow and no uniforms as (0.0, 0, 1.0) = every row greedy."""
        n_top = int(top_logprobs)
        if not 0 <= n_top <= 64:
            raise ValueError("top_logprobs must be in 0..64")
        t_ref = None
        if prior_temperature is not None:
            t_ref = ops.ref_temperature_value(f"{what}: prior_temperature", prior_temperature)
            if not has_uniforms:
                raise ValueError("prior_temperature needs uniforms: the reference score comes from the per-row sampler, in which a greedy "
                                 "candidate is a row with temperature=0 (pass uniforms and temperature=0 rows instead of uniforms=None)")
        temperature, top_k, top_p = params
        if any(ops.is_per_row(v) for v in params):
            if not has_uniforms:
                raise ValueError(f"per-{unit} temperature / top_k / top_p need uniforms (a greedy {unit} is a temperature of 0)")
        elif t_ref is None and allow is None:
            unfiltered = not has_uniforms or (top_k <= 0 and top_p >= 1.0)
            filt = (top_k, top_p) if filter_always else None if unfiltered else (int(top_k), float(top_p))
            return cls(not has_uniforms, temperature, filt, None, None, None, n_top)
        elif not has_uniforms:
            params = (0.0, 0, 1.0)
        return cls(not has_uniforms, None, None, ops.row_param_tensors(rows, *params, device), allow, t_ref, n_top)

    def pick(self, logits, lo, hi, u, *, out_tok=None, out_logit=None, out_kept=None, out_logprob=None, out_ref=None, top=None):
        """ONE ops.pick_token over columns [lo, hi) with step uniforms u; out_ref fp32 [rows] receives the reference score (t_ref set).
        top = (tok, logprob, entropy) slabs of this step: one top-n launch under the distribution the pick came from follows (a greedy
        pick ranks at temperature 1, unfiltered). Returns what pick_token returns; no arithmetic or allocation of its own."""
        out = dict(out_tok=out_tok, out_logit=out_logit, out_kept=out_kept, out_logprob=out_logprob)
        akw = {} if self.allow is None else dict(allow=self.allow)      # None: exactly the calls made before the argument existed
        if self.rp is None:
            res = ops.pick_token(logits, lo, hi, u, self.temperature, self.filt, **out)
        else:
            rkw = {} if self.t_ref is None else dict(ref=(self.t_ref, out_ref))
            res = ops.pick_token(logits, lo, hi, u, row_params=self.rp, **out, **akw, **rkw)
        if top is not None:
            tkw = dict(out_tok=top[0], out_logprob=top[1], out_entropy=top[2])
            if self.rp is not None:
                ops.token_topn_rows(logits, lo, hi, top[0].shape[1], self.rp[0], self.rp[1], self.rp[2], **tkw, **akw)
            else:
                T, (k, p) = (1.0, (0, 1.0)) if self.greedy else (self.temperature, self.filt or (0, 1.0))
                ops.token_topn(logits, lo, hi, top[0].shape[1], T, k, p, **tkw)
        return res

    def graph_key(self, logprobs):
        """What a captured decode loop depends on: not the per-row VALUES (static buffers), but t_ref (by value in the launch)."""
        return (self.greedy, "rows" if self.rp is not None else float(self.temperature), self.filt, bool(logprobs), self.n_top, self.t_ref)


class StepOutputs(NamedTuple):
    """The output buffers of a decode loop; sel / lps / prior / top are None when not asked for. top = (tokens [S, R, n], logprobs
    [S, R, n], entropy [S, R]) is always step-major: slab i is what step i's top-n launch writes."""
    tokens: torch.Tensor
    sel: Optional[torch.Tensor]
    lps: Optional[torch.Tensor]
    prior: Optional[torch.Tensor]
    top: Optional[tuple]
    step_major: bool

    @classmethod
    def alloc(cls, steps, rows, device, *, logit, logprob, ref, n_top, fill):
        """fill None (OpenVLA): everything step-major [S, R] and uninitialised -- row i of each is contiguous, so step i's kernels write it
        in place. fill = the pad token id (pi0-FAST): tokens / lps / prior candidate-major [R, S], as ops.decode_feedback writes them, and
        every buffer padded with what a step that never runs leaves: pad id / 0.0 / -1 / -inf / 0.0."""
        def buf(want, dtype, pad, shape):
            if not want:
                return None
            return torch.empty(shape, dtype=dtype, device=device) if fill is None else torch.full(shape, pad, dtype=dtype, device=device)
        flat, slab = (steps, rows) if fill is None else (rows, steps), (steps, rows, n_top)
        top = (buf(n_top, torch.int64, -1, slab), buf(n_top, torch.float32, float("-inf"), slab), buf(n_top, torch.float32, 0.0, (steps, rows)))
        return cls(buf(True, torch.int64, fill, flat), buf(logit, torch.float32, 0.0, flat), buf(logprob, torch.float32, 0.0, flat),
                   buf(ref, torch.float32, 0.0, flat), top if n_top else None, fill is None)

    def top_at(self, i):
        return None if self.top is None else (self.top[0][i], self.top[1][i], self.top[2][i])

    def result(self, fin=None):
        """Candidate-major tokens[, sel][, logprobs][, prior][, TopLogprobs]. fin bool [R, S] (pi0-FAST): the steps after a row's EOS,
        whose top-n slabs become padding (a finished row's pad is not a choice)."""
        major = (lambda b: b.t().contiguous()) if self.step_major else (lambda b: b)
        out = tuple(major(b) for b in (self.tokens, self.sel, self.lps, self.prior) if b is not None)
        if self.top is None:
            return out
        tok, lp, ent = (b.transpose(0, 1) for b in self.top)
        if fin is None:
            return out + (TopLogprobs(tok.contiguous(), lp.contiguous(), ent.contiguous()),)
        return out + (TopLogprobs(torch.where(fin[:, :, None], torch.full_like(tok, -1), tok),
                                  torch.where(fin[:, :, None], torch.full_like(lp, float("-inf")), lp),
                                  torch.where(fin, torch.zeros_like(ent), ent)),)
