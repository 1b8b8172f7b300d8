"""Host-side glue of the evaluation loop, restated for the candidate batch (float64 numpy, vectorised).

The reference does this work in a B x 4 Python loop that rebuilds the statistics arrays 160 times per decision
(eval_utils.py:172-221 -> simpler.py:96-166); here it is a handful of array expressions with the same arithmetic.
  denormalize_bound            INT-ACT/src/experiments/env_adapters/base.py:20-31
  postprocess_verifier         .../simpler.py:96-121 (+ BridgeSimplerAdapter.postprocess_gripper_verifier :222-226)
  postprocess (execution)      .../simpler.py:123-166 (+ postprocess_gripper :211-220, euler2axangle INT-ACT/src/utils/geometry.py:261-436)
  process_inputs               CoVer_VLA/inference/experiments/robot/simpler/eval_utils.py:172-221
  two-stage verification, gripper vote, chunk extraction
                               .../run_simpler_eval_with_openpi.py:329-401
"""
from __future__ import annotations

import json
import math
import os
from collections import deque
from typing import Any, List, NamedTuple, Optional, Sequence

import numpy as np

_STATS = None


def bridge_statistics() -> dict:
    global _STATS
    if _STATS is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "bridge_statistics.json")) as f:
            _STATS = json.load(f)
    return _STATS


def sequence_logprob(logprobs, tokens=None, pad_token_id=None, length_normalize=False):
    """Per-candidate sequence log-probability from the per-step values OpenVLA.sample / PI0FASTTokens.generate_tokens return with
    return_logprobs: logprobs [N, steps] (torch tensor on any device, or numpy) -> [N] of the same kind, the sum over steps. With
    tokens [N, steps] and pad_token_id the steps whose token is the pad are left out (generate_tokens already gives them 0.0; this
    also serves values scored elsewhere, where a pad scores -inf); length_normalize divides by the number of counted steps (at least 1).
    Index bookkeeping on N x steps values."""
    if isinstance(logprobs, np.ndarray):
        count = np.ones(logprobs.shape, dtype=bool)
        if tokens is not None and pad_token_id is not None:
            count = np.asarray(tokens) != pad_token_id
        total = np.where(count, logprobs, 0.0).sum(axis=1)
        return total / np.maximum(count.sum(axis=1), 1) if length_normalize else total
    import torch
    count = torch.ones_like(logprobs, dtype=torch.bool)
    if tokens is not None and pad_token_id is not None:
        count = tokens.to(logprobs.device) != pad_token_id
    total = torch.where(count, logprobs, torch.zeros_like(logprobs)).sum(dim=1)
    return total / count.sum(dim=1).clamp(min=1).to(total.dtype) if length_normalize else total


class TopLogprobs(NamedTuple):
    """What OpenVLA.sample / PI0FASTTokens.generate_tokens append with top_logprobs = n: per candidate and step the n most probable
    tokens of the distribution the step's pick came from (descending logit, equal logits by ascending id), their log-probabilities
    and the entropy of that distribution in nats. Slots beyond the kept set carry token -1 / log-probability -inf."""
    tokens: Any        # int64 [N, steps, n]
    logprobs: Any      # fp32 [N, steps, n]
    entropy: Any       # fp32 [N, steps]


def sampling_ladder(n_prompts: int, n_samples: int, temperature, top_k=0, top_p=1.0):
    """The per-candidate sampling parameters of a best-of-N proposal ladder: every prompt's n_samples candidates get the same ladder
    (typically one greedy candidate, temperature 0, then samples at rising temperatures or looser filters). Each argument is a scalar
    or a length-n_samples sequence; returns (temperature float32, top_k int32, top_p float32) numpy arrays [n_prompts * n_samples] in
    which candidate i carries entry i % n_samples -- the "candidate i belongs to prompt i // n_samples" order of OpenVLA.sample, whose
    temperature / top_k / top_p arguments take these arrays. Values must be finite with temperature >= 0, top_k >= 0 (an integer) and
    top_p > 0. Index bookkeeping only.
    The return_logprobs of a ladder are each taken under their own rung's distribution and do not compare across rungs (a greedy rung is
    scored at temperature 1, a top_k = 1 rung scores every pick 0.0, a hot rung is penalised for its own flatness): a candidate_prior for
    verify_and_select / cover_prior_select under a ladder should be the prior_temperature tensor of OpenVLA.sample /
    PI0FASTTokens.generate_tokens (PI0FASTPolicy.last_sequence_prior_logprobs), every pick scored at one reference temperature, unfiltered."""
    if int(n_prompts) < 1 or int(n_samples) < 1:
        raise ValueError("sampling_ladder: n_prompts and n_samples must be >= 1")
    out = []
    for name, v, dt, ok in (("temperature", temperature, np.float32, lambda a: a >= 0), ("top_k", top_k, np.int32, lambda a: a >= 0),
                            ("top_p", top_p, np.float32, lambda a: a > 0)):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(int(n_samples), float(a))
        if a.shape != (int(n_samples),):
            raise ValueError(f"sampling_ladder: {name} must be a scalar or have one entry per sample ({n_samples}), got shape {a.shape}")
        if not np.all(np.isfinite(a)) or not np.all(ok(a)) or (dt is np.int32 and np.any(a != np.rint(a))):
            raise ValueError(f"sampling_ladder: {name} out of range (temperature >= 0, integer top_k >= 0, top_p > 0, all finite)")
        out.append(np.tile(a, int(n_prompts)).astype(dt))
    return tuple(out)


def augmentation_normals(n_prompts: int, n_augmented: int, steps: int, seed: int):
    """The standard normals of one Gaussian proposal augmentation (ops.augment_tokens / ops.augment_actions, OpenVLA.augment,
    PI0Policy.select_action(augment=)): a host fp32 torch tensor [n_prompts, n_augmented, steps, 6] drawn from a CPU torch.Generator
    seeded with `seed` -- element (g, k, t, d) perturbs dim d of step t of prompt g's k-th augmented candidate. The caller supplies them
    as it supplies the samplers' uniforms: the same seed gives the same tensor and so the same augmented candidates, bit for bit; move it
    to the policy's device once per decision. No seed schedule is chosen here."""
    import torch
    n_prompts, n_augmented, steps = int(n_prompts), int(n_augmented), int(steps)
    if n_prompts < 1 or n_augmented < 0 or steps < 1:
        raise ValueError("augmentation_normals: n_prompts >= 1, n_augmented >= 0 and steps >= 1 are required")
    return torch.randn(n_prompts, n_augmented, steps, 6, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


class _AugmentFields(NamedTuple):
    samples_per_prompt: int
    n_augmented: int
    normals: Any
    sigma: float = 1.0
    sd_floor: float = 0.0
    clip: Any = (-1.0, 1.0)


class Augment(_AugmentFields):
    """What PI0Policy.select_action(augment=) takes: every prompt's samples_per_prompt policy samples (contiguous rows of the batch) are
    followed by n_augmented candidates drawn from the diagonal Gaussian fitted to them in the policy's normalised action space
    (ops.augment_actions: the arithmetic, the clip and the gripper vote -- on a gripper tie the augmented rows take the class of sample 0,
    so the in-group vote of verify_and_select may then differ from the reference's "winner's sign" rule). normals: fp32
    [prompts, n_augmented, n_action_steps, 6] on the policy's device (augmentation_normals). sigma scales the fitted standard deviation,
    sd_floor is its lower bound, clip = (lo, hi) bounds the drawn values (+-inf = no clip). Values are checked here (CoverError), shapes
    against the batch in ops.augment_actions. No default n_augmented, sigma or floor is recommended."""
    __slots__ = ()

    def __new__(cls, samples_per_prompt, n_augmented, normals, sigma=1.0, sd_floor=0.0, clip=(-1.0, 1.0)):
        import torch
        from ._lib import CoverError
        ints = (int, np.integer)
        if not (isinstance(samples_per_prompt, ints) and isinstance(n_augmented, ints)) or not 1 <= samples_per_prompt <= 4096 \
                or not 0 <= n_augmented <= 4096:
            raise CoverError(f"Augment: integers 1 <= samples_per_prompt <= 4096 and 0 <= n_augmented <= 4096 are required "
                             f"(got {samples_per_prompt!r}, {n_augmented!r})")
        if not torch.is_tensor(normals) or normals.dtype != torch.float32 or normals.dim() != 4 or normals.shape[1] != n_augmented \
                or normals.shape[3] != 6:
            raise CoverError(f"Augment: normals must be an fp32 tensor [prompts, n_augmented = {n_augmented}, steps, 6]")
        for name, v in (("sigma", sigma), ("sd_floor", sd_floor)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v >= 0):
                raise CoverError(f"Augment: {name} must be a finite number >= 0 (got {v!r})")
        if not isinstance(clip, (tuple, list)) or len(clip) != 2 or not all(isinstance(v, (int, float)) for v in clip) or not clip[0] <= clip[1]:
            raise CoverError(f"Augment: clip must be a (lo, hi) pair of numbers with lo <= hi (got {clip!r})")
        return super().__new__(cls, int(samples_per_prompt), int(n_augmented), normals, float(sigma), float(sd_floor), (float(clip[0]), float(clip[1])))


def vote_log_shares(n_fit: int, alpha: float) -> np.ndarray:
    """The gripper term of the proposal log-density prior (ops.proposal_prior_tokens / ops.proposal_prior_actions, log_share=): fp32
    numpy [n_fit + 1], entry c = float32(log((c + alpha) / (n_fit + 2 alpha))) computed in float64 -- the add-alpha estimate of the
    share of a gripper class that c of the n_fit fitted samples voted for. It is made on the host so that the device takes no
    logarithm and the prior stays a fixed bit pattern; move it to the device once (torch.from_numpy(...).to(dev)). alpha = 0 gives -inf
    at c = 0: a row whose class no sample voted for can then never win (cover_prior_select's rule for -inf). No alpha is recommended."""
    if isinstance(n_fit, bool) or not isinstance(n_fit, (int, np.integer)) or not 1 <= n_fit <= 4096:
        raise ValueError(f"vote_log_shares: an integer 1 <= n_fit <= 4096 is required (got {n_fit!r})")
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.floating, np.integer)) or not (math.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"vote_log_shares: alpha must be a finite number >= 0 (got {alpha!r})")
    c = np.arange(int(n_fit) + 1, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.log((c + float(alpha)) / (float(n_fit) + 2.0 * float(alpha))).astype(np.float32)


class _ProposalPriorFields(NamedTuple):
    samples_per_prompt: int
    sigma: float
    sd_floor: float
    log_share: Any = None


class ProposalPrior(_ProposalPriorFields):
    """What PI0Policy.proposal_prior is set to (policy.proposal_prior = ProposalPrior(...); None = off): every row of the action batch gets the unnormalised log-density of the
    diagonal Gaussian fitted to its prompt's samples_per_prompt policy samples (ops.proposal_prior_actions, in the policy's normalised
    action space; with augment= the augmented rows behind the samples are scored under the same fit), kept as
    policy.last_proposal_prior for verify_and_select(candidate_prior=, prior_beta=). sigma scales the fitted standard deviation and
    sd_floor is its lower bound, both > 0 and both required; log_share: None or fp32 [samples_per_prompt + 1] on the policy's device
    (vote_log_shares), the gripper term. Values are checked here (CoverError), shapes against the batch in ops.proposal_prior_actions.
    No default sigma, floor or alpha is recommended."""
    __slots__ = ()

    def __new__(cls, samples_per_prompt, sigma, sd_floor, log_share=None):
        import ctypes
        import torch
        from ._lib import CoverError
        f32 = lambda v: ctypes.c_float(v).value                     # the value the launch receives
        if isinstance(samples_per_prompt, bool) or not isinstance(samples_per_prompt, (int, np.integer)) or not 1 <= samples_per_prompt <= 4096:
            raise CoverError(f"ProposalPrior: an integer 1 <= samples_per_prompt <= 4096 is required (got {samples_per_prompt!r})")
        for name, v in (("sigma", sigma), ("sd_floor", sd_floor)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and math.isfinite(f32(v)) and f32(v) > 0):
                raise CoverError(f"ProposalPrior: {name} must be a finite number > 0 in fp32 (got {v!r})")
        if not f32(f32(sigma) * f32(sd_floor)) > 0:
            raise CoverError(f"ProposalPrior: the fp32 product sigma * sd_floor must be > 0 (got {sigma!r} * {sd_floor!r})")
        if log_share is not None and (not torch.is_tensor(log_share) or log_share.dtype != torch.float32
                                      or tuple(log_share.shape) != (samples_per_prompt + 1,)):
            raise CoverError(f"ProposalPrior: log_share must be None or an fp32 tensor [samples_per_prompt + 1 = {samples_per_prompt + 1}]")
        return super().__new__(cls, int(samples_per_prompt), float(sigma), float(sd_floor), log_share)


class _SmoothFields(NamedTuple):
    radius: float
    dim_scale: Any
    shrink: float = 0.0
    split_gripper: bool = True


def _finite_f32(who, **named):
    """Every value is a finite Python number (bools rejected) that is finite in fp32 as well, the value the launch receives."""
    import ctypes
    from ._lib import CoverError
    for name, v in named.items():
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and math.isfinite(ctypes.c_float(v).value)):
            raise CoverError(f"{who}: {name} must be a finite number (got {v!r})")


_UPLOADS = {}            # ("scale", dim_scale, device) / ("steps", decay, h, device) -> the fp32 device tensor: one upload per device


def _scale_on(dim_scale, device):
    """A checked dim_scale tuple as the fp32 [6] tensor the launch reads, uploaded once per device."""
    import torch
    key = ("scale", dim_scale, str(torch.device(device)))
    if key not in _UPLOADS:
        _UPLOADS[key] = torch.tensor(dim_scale, dtype=torch.float32).to(device)
    return _UPLOADS[key]


def _steps_on(decay, h, device):
    """coherence_step_weights(h, decay) as the fp32 [h] tensor the launch reads, uploaded once per device and h."""
    import torch
    key = ("steps", decay, int(h), str(torch.device(device)))
    if key not in _UPLOADS:
        _UPLOADS[key] = torch.from_numpy(coherence_step_weights(int(h), decay)).to(device)
    return _UPLOADS[key]


class Smooth(_SmoothFields):
    """What score_histories(smooth=), verify_and_select(smooth=) and OpenVLA.smooth_scores take: every candidate's score is replaced by
    the kernel-weighted mean of its prompt group's scores, weight max(0, 1 - d2 / radius^2) with d2 the squared distance of the rows'
    translation / rotation values scaled per dim by dim_scale (a 6-sequence of finite numbers >= 0; 0 leaves a dim out), shrunk towards
    the group's mean score: (sum w s + shrink * mean) / (sum w + shrink) (ops.smooth_scores_tokens: the arithmetic). split_gripper: rows
    of different gripper class (value >= 0.5) do not back each other. radius > 0 and shrink >= 0, both finite. Values are checked here
    (CoverError), shapes against the rows in ops. No default radius or scale exists and no radius, scale or shrink is recommended: there
    is no task-success data to choose them on."""
    __slots__ = ()

    def __new__(cls, radius, dim_scale, shrink=0.0, split_gripper=True):
        import ctypes
        from ._lib import CoverError
        from .ops import smooth_dim_scale
        f32 = lambda v: ctypes.c_float(v).value                     # the value the launch receives
        _finite_f32("Smooth", radius=radius, shrink=shrink)
        if not (f32(radius) > 0 and math.isfinite(f32(f32(radius) * f32(radius))) and f32(f32(radius) * f32(radius)) > 0):
            raise CoverError(f"Smooth: radius must be > 0 with a finite fp32 square > 0 (got {radius!r})")
        if not shrink >= 0:
            raise CoverError(f"Smooth: shrink must be >= 0 (got {shrink!r})")
        scale = tuple(float(v) for v in smooth_dim_scale(dim_scale, "Smooth"))
        return super().__new__(cls, float(radius), scale, float(shrink), bool(split_gripper))

    def scale_on(self, device):
        """dim_scale as the fp32 [6] tensor the launch reads, uploaded once per device."""
        return _scale_on(self.dim_scale, device)

    def kwargs(self, device) -> dict:
        """The keywords of ops.smooth_scores_tokens / ops.smooth_scores_actions."""
        return dict(radius=self.radius, dim_scale=self.scale_on(device), shrink=self.shrink, split_gripper=self.split_gripper)


def coherence_step_weights(h: int, decay: float) -> np.ndarray:
    """The step weights of the chunk-coherence prior (ops.coherence_prior_tokens / ops.coherence_prior_actions, step_weight=): fp32 numpy
    [h], entry t = float32(decay ** t) computed in float64 -- step t of a candidate counts decay^t, the early steps (which are executed
    first) the most. It is made on the host so that the device takes no pow and the prior stays a fixed bit pattern; move it to the
    device once (torch.from_numpy(...).to(dev); host.Coherence does). decay must be finite and in (0, 1]; 1 weighs every step alike.
    No decay is recommended."""
    if isinstance(h, bool) or not isinstance(h, (int, np.integer)) or not 1 <= h <= 64:
        raise ValueError(f"coherence_step_weights: an integer 1 <= h <= 64 is required (got {h!r})")
    if isinstance(decay, bool) or not isinstance(decay, (int, float, np.floating, np.integer)) or not (math.isfinite(decay) and 0 < decay <= 1):
        raise ValueError(f"coherence_step_weights: decay must be a finite number in (0, 1] (got {decay!r})")
    return (np.float64(decay) ** np.arange(int(h), dtype=np.float64)).astype(np.float32)


def fast_idct_basis(H: int) -> np.ndarray:
    """The basis of the pi0-FAST de-tokeniser (ops.fast_decode, basis=): fp32 numpy [H, H], the orthonormal inverse DCT-II matrix
    scipy.fft.idct(x, axis=0, norm="ortho") multiplies by -- B[t][0] = sqrt(1 / H), B[t][k] = sqrt(2 / H) * cos(pi * (2 t + 1) * k / (2 H))
    -- computed in float64 and rounded to fp32 once. It is made on the host so that the device takes no cosine and the chunk stays a
    fixed bit pattern; move it to the device once (torch.from_numpy(...).to(dev); PI0FASTPolicy does)."""
    if isinstance(H, bool) or not isinstance(H, (int, np.integer)) or not 1 <= H <= 128:
        raise ValueError(f"fast_idct_basis: an integer 1 <= H <= 128 is required (got {H!r})")
    H = int(H)
    t, k = np.arange(H, dtype=np.float64)[:, None], np.arange(H, dtype=np.float64)[None, :]
    basis = np.sqrt(2.0 / H) * np.cos(np.pi * (2.0 * t + 1.0) * k / (2.0 * H))
    basis[:, 0] = np.sqrt(1.0 / H)
    return basis.astype(np.float32)


def fast_pieces_from_decoder(bpe_decode, n_pieces: int) -> list:
    """The piece list ops.fast_piece_table takes, from a BPE decoder (the FAST processor's bpe_tokenizer.decode): entry f is the list of
    code points of bpe_decode([f]), each FAST id decoded ON ITS OWN; an id whose decode raises becomes None (undecodable: a row that
    holds it decodes to zeros, as the reference's decoder does when the sequence raises).
    The assumption this rests on, which the caller owns: the BPE's decode of a sequence is the concatenation of its pieces' decodes.
    That holds for the FAST processor's character-level BPE (a token is a string of symbols and decode joins them); it does not hold
    for a decoder that cleans up spaces between tokens, merges byte fallbacks across tokens or strips at the sequence ends."""
    if isinstance(n_pieces, bool) or not isinstance(n_pieces, (int, np.integer)) or n_pieces < 1:
        raise ValueError(f"fast_pieces_from_decoder: an integer n_pieces >= 1 is required (got {n_pieces!r})")
    pieces = []
    for f in range(int(n_pieces)):
        try:
            pieces.append([ord(ch) for ch in bpe_decode([f])])
        except Exception:
            pieces.append(None)
    return pieces


class _CoherenceFields(NamedTuple):
    dim_scale: Any
    decay: float
    gripper_penalty: float = 0.0


class Coherence(_CoherenceFields):
    """What OpenVLA.coherence_prior takes and PI0Policy.coherence holds: every candidate gets the prior -sum_r w_r D(candidate, r) over
    a set of reference chunks, D the sum over the overlapping steps t of decay^t * (the squared distance of the translation / rotation
    values scaled per dim by dim_scale, plus gripper_penalty where the gripper classes (value >= 0.5) differ) (ops.coherence_prior_tokens:
    the arithmetic). dim_scale: a 6-sequence of finite numbers >= 0 (0 leaves a dim out); decay finite and in (0, 1]; gripper_penalty
    finite and >= 0. Values are checked here (CoverError), shapes against the rows in ops. The references, their weights and the weight
    the prior gets beside other priors are the caller's. No default decay or scale exists and no decay, scale, penalty or mixing weight
    is recommended: there is no task-success data to choose them on."""
    __slots__ = ()

    def __new__(cls, dim_scale, decay, gripper_penalty=0.0):
        from ._lib import CoverError
        from .ops import smooth_dim_scale
        _finite_f32("Coherence", decay=decay, gripper_penalty=gripper_penalty)
        if not 0 < decay <= 1:
            raise CoverError(f"Coherence: decay must be in (0, 1] (got {decay!r})")
        if not gripper_penalty >= 0:
            raise CoverError(f"Coherence: gripper_penalty must be >= 0 (got {gripper_penalty!r})")
        scale = tuple(float(v) for v in smooth_dim_scale(dim_scale, "Coherence"))
        return super().__new__(cls, scale, float(decay), float(gripper_penalty))

    def scale_on(self, device):
        """dim_scale as the fp32 [6] tensor the launch reads, uploaded once per device."""
        return _scale_on(self.dim_scale, device)

    def steps_on(self, device, h):
        """coherence_step_weights(h, decay) as the fp32 [h] tensor the launch reads, uploaded once per device and h."""
        return _steps_on(self.decay, h, device)

    def kwargs(self, device, h) -> dict:
        """The keywords of ops.coherence_prior_tokens / ops.coherence_prior_actions for candidates of h steps."""
        return dict(step_weight=self.steps_on(device, h), dim_scale=self.scale_on(device), gripper_penalty=self.gripper_penalty)


class _DiversityFields(NamedTuple):
    keep: int
    weight: float
    dim_scale: Any
    decay: float
    gripper_penalty: float
    cover_dist: float = -1.0


class Diversity(_DiversityFields):
    """What OpenVLA.diverse_subset takes and PI0Policy.diverse holds: of every prompt's candidate rows at most `keep` are kept, picked
    greedily by quality + weight * (distance to the nearest row already picked), the distance being Coherence's between two rows of the
    group: the sum over the steps t of decay^t * (the squared distance of the translation / rotation values scaled per dim by dim_scale,
    plus gripper_penalty where the gripper classes (value >= 0.5) differ) (ops.diverse_subset_tokens: the arithmetic). Rows whose
    distance to a pick is <= cover_dist are left out: 0 removes exact duplicates, r > 0 ends the selection once the group is covered,
    a negative value (the default) switches the rule off. keep: an integer 1..4096; weight finite and >= 0 (0 = a pure top-keep by
    quality); dim_scale: a 6-sequence of finite numbers >= 0 (0 leaves a dim out); decay finite and in (0, 1]; gripper_penalty finite and
    >= 0; cover_dist any number below +inf. Values are checked here (CoverError), shapes against the rows in ops. No default keep,
    weight, decay or scale exists and no value of any field is recommended: there is no task-success data to choose them on."""
    __slots__ = ()

    def __new__(cls, keep, weight, dim_scale, decay, gripper_penalty, cover_dist=-1.0):
        import ctypes
        from ._lib import CoverError
        from .ops import smooth_dim_scale
        f32 = lambda v: ctypes.c_float(v).value                     # the value the launch receives
        if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or not 1 <= keep <= 4096:
            raise CoverError(f"Diversity: keep must be an integer in [1, 4096] (got {keep!r})")
        _finite_f32("Diversity", weight=weight, decay=decay, gripper_penalty=gripper_penalty)
        if not weight >= 0:
            raise CoverError(f"Diversity: weight must be >= 0 (got {weight!r})")
        if not 0 < decay <= 1:
            raise CoverError(f"Diversity: decay must be in (0, 1] (got {decay!r})")
        if not gripper_penalty >= 0:
            raise CoverError(f"Diversity: gripper_penalty must be >= 0 (got {gripper_penalty!r})")
        if isinstance(cover_dist, bool) or not isinstance(cover_dist, (int, float)) or math.isnan(cover_dist) or not f32(cover_dist) < math.inf:
            raise CoverError(f"Diversity: cover_dist must be a number below +inf in fp32; negative = off (got {cover_dist!r})")
        scale = tuple(float(v) for v in smooth_dim_scale(dim_scale, "Diversity"))
        return super().__new__(cls, int(keep), float(weight), scale, float(decay), float(gripper_penalty), float(cover_dist))

    def kwargs(self, device, h) -> dict:
        """The keywords of ops.diverse_subset_tokens / ops.diverse_subset_actions for rows of h steps (keep is positional there). The
        step weights and the scale are the uploads a Coherence of the same values has: one per device."""
        return dict(weight=self.weight, cover_dist=self.cover_dist, step_weight=_steps_on(self.decay, h, device),
                    dim_scale=_scale_on(self.dim_scale, device), gripper_penalty=self.gripper_penalty)


def spread_scores(scores_kept, subset, group_rows):
    """The scores of a pruned verifier call on the rows they stand for: scores_kept fp32 [G * keep] (score_histories' scores of
    subset.rows, group_size = keep), subset the ops.DiverseSubset of G groups of group_rows rows -> fp32 [G * group_rows], every input
    row carrying the score of the slot subset.assign names (its nearest pick; a picked row its own slot, or an earlier pick's it equals)
    and -inf where assign is -1 (a row with a non-finite element, or a group with no pick): such a row never wins ops.group_argmax /
    ops.prior_select. The result goes where scores of the original rows go -- ops.group_argmax, smooth_scores, refine -- with
    group_size = group_rows. Plain torch indexing on the scores' device, no host synchronisation."""
    import torch
    if isinstance(group_rows, bool) or not isinstance(group_rows, (int, np.integer)) or group_rows < 1:
        raise ValueError(f"spread_scores: group_rows must be an integer >= 1 (got {group_rows!r})")
    G, keep = subset.picked.shape
    if not torch.is_tensor(scores_kept) or scores_kept.dtype != torch.float32 or tuple(scores_kept.shape) != (G * keep,):
        raise ValueError(f"spread_scores: scores_kept must be fp32 [G * keep] = [{G * keep}] "
                         f"(got {tuple(scores_kept.shape) if torch.is_tensor(scores_kept) else type(scores_kept).__name__})")
    if tuple(subset.assign.shape) != (G * int(group_rows),):
        raise ValueError(f"spread_scores: subset.assign has {tuple(subset.assign.shape)} entries, not G * group_rows = {G * int(group_rows)}")
    assign = subset.assign.to(torch.int64)
    group = torch.arange(G * int(group_rows), device=assign.device) // int(group_rows)
    taken = scores_kept[group * keep + assign.clamp(min=0)]
    return torch.where(assign >= 0, taken, torch.full_like(taken, -math.inf))


class TokenGrammar(NamedTuple):
    """What PI0FASTTokens.generate_tokens(grammar=) takes: the allowed-token sets and the per-row automaton that picks among them."""
    allow: Any         # ops.TokenAllow (bits over the vocabulary; set_of_row is made per call)
    fsm: Any           # ops.TokenFsm


def _id_mask(vocab, ids, what):
    """bool [vocab] of an id list or one half-open (lo, hi) range."""
    on = np.zeros(vocab, dtype=bool)
    if isinstance(ids, tuple) and len(ids) == 2:
        a, b = int(ids[0]), int(ids[1])
        if not 0 <= a < b <= vocab:
            raise ValueError(f"length_grammar: {what} range ({a}, {b}) must be non-empty inside [0, {vocab})")
        on[a:b] = True
        return on
    ids = [int(t) for t in (ids if isinstance(ids, (list, set, frozenset, np.ndarray)) else [ids])]
    if not ids or min(ids) < 0 or max(ids) >= vocab:
        raise ValueError(f"length_grammar: {what} needs at least one id, all inside [0, {vocab})")
    on[ids] = True
    return on


def length_grammar(vocab, body, end, eos, min_len, max_len, extra_sets=None, device=None):
    """The grammar "min_len..max_len body tokens, one end token, then EOS" as a token-class automaton for generate_tokens(grammar=) /
    ops.decode_feedback(fsm=). body, end and eos are id lists (or one id) or a half-open (lo, hi) tuple, pairwise disjoint.
    States 0..max_len count the body tokens emitted so far, then ENDED = max_len + 1 (after an end token) and FINISHED = max_len + 2
    (after EOS). Classes: 0 body, 1 end, 2 eos, 3 every other id. A state allows
        n < min_len: body        min_len <= n < max_len: body or end        n == max_len: end        ENDED, FINISHED: eos
    and a token of an allowed class moves (body: n + 1, end: ENDED, eos: FINISHED); a token whose class the state does not allow (only a
    teacher-forced one can be) leaves the state where it is. The bit sets are the distinct rows of that table in order of first use
    (at most four, however large max_len is: the states share them through set_of_state); extra_sets (token_allow_sets' format) are
    appended after them for the caller's own use. Returns TokenGrammar(ops.TokenAllow, ops.TokenFsm), the bits on device if given."""
    from . import ops
    vocab, min_len, max_len = int(vocab), int(min_len), int(max_len)
    if not 0 <= min_len <= max_len:
        raise ValueError("length_grammar: 0 <= min_len <= max_len is required")
    m_body, m_end, m_eos = _id_mask(vocab, body, "body"), _id_mask(vocab, end, "end"), _id_mask(vocab, eos, "eos")
    if (m_body & m_end).any() or (m_body & m_eos).any() or (m_end & m_eos).any():
        raise ValueError("length_grammar: body, end and eos must be pairwise disjoint")
    BODY, END, EOS, OTHER = 0, 1, 2, 3
    cls = np.full(vocab, OTHER, dtype=np.uint8)
    cls[m_body], cls[m_end], cls[m_eos] = BODY, END, EOS
    ended, finished = max_len + 1, max_len + 2
    n_states = max_len + 3
    allowed = [(n < max_len, n >= min_len, False) for n in range(max_len + 1)] + [(False, False, True)] * 2    # (body, end, eos) per state
    trans = np.repeat(np.arange(n_states, dtype=np.int32)[:, None], 4, axis=1)                                   # default: stay
    for s, (b, e, z) in enumerate(allowed):
        if b:
            trans[s, BODY] = s + 1
        if e:
            trans[s, END] = ended
        if z:
            trans[s, EOS] = finished
    kinds, set_of_state = [], np.zeros(n_states, dtype=np.int32)
    for s, k in enumerate(allowed):
        if k not in kinds:
            kinds.append(k)
        set_of_state[s] = kinds.index(k)
    masks = [(m_body & b) | (m_end & e) | (m_eos & z) for b, e, z in kinds]
    sets = [list(np.nonzero(m)[0]) for m in masks] + list(extra_sets or [])
    allow = ops.TokenAllow(ops.token_allow_sets(vocab, sets, device))
    fsm = ops.TokenFsm(cls, trans, set_of_state, start_state=0)
    fsm.check_sets(allow)
    return TokenGrammar(allow, fsm)


def step_entropy_summary(entropy, tokens=None, pad_id=None):
    """Per-candidate (mean, max) of the per-step entropies over the steps the candidate was live: entropy [N, steps] (torch tensor on
    any device, or numpy) -> two [N] of the same kind. With tokens [N, steps] and pad_id the steps whose emitted token is the pad are
    left out (a finished pi0-FAST row; generate_tokens gives them entropy 0.0); a candidate with no live step gets 0.0 for both.
    Index bookkeeping on N x steps values."""
    if isinstance(entropy, np.ndarray):
        live = np.ones(entropy.shape, dtype=bool)
        if tokens is not None and pad_id is not None:
            live = np.asarray(tokens) != pad_id
        mean = np.where(live, entropy, 0.0).sum(axis=1) / np.maximum(live.sum(axis=1), 1)
        return mean, np.where(live, entropy, 0.0).max(axis=1)
    import torch
    live = torch.ones_like(entropy, dtype=torch.bool)
    if tokens is not None and pad_id is not None:
        live = tokens.to(entropy.device) != pad_id
    kept = torch.where(live, entropy, torch.zeros_like(entropy))
    return kept.sum(dim=1) / live.sum(dim=1).clamp(min=1).to(kept.dtype), kept.max(dim=1).values


def denormalize_bound(data, data_min, data_max, clip_min=-1.0, clip_max=1.0):
    return (data - clip_min) / (clip_max - clip_min) * (data_max - data_min) + data_min


def euler2axangle_sxyz(roll, pitch, yaw):
    """euler2quat('sxyz') followed by quat2axangle, vectorised over leading dims. Returns axis*angle [..., 3]."""
    ai, aj, ak = np.asarray(roll) / 2.0, np.asarray(pitch) / 2.0, np.asarray(yaw) / 2.0
    ci, si, cj, sj, ck, sk = np.cos(ai), np.sin(ai), np.cos(aj), np.sin(aj), np.cos(ak), np.sin(ak)
    cc, cs, sc, ss = ci * ck, ci * sk, si * ck, si * sk
    q = np.stack([cj * cc + sj * ss, cj * sc - sj * cs, cj * ss + sj * cc, cj * cs - sj * sc], axis=-1)
    eps = np.finfo(np.float64).eps
    nq = np.sum(q ** 2, axis=-1, keepdims=True)
    qn = np.where(nq != 1, q / np.sqrt(np.where(nq > 0, nq, 1.0)), q)
    xyz = qn[..., 1:]
    len2 = np.sum(xyz ** 2, axis=-1, keepdims=True)
    ident = (len2 < (eps * 3) ** 2) | (nq < eps ** 2)
    theta = 2.0 * np.arccos(np.clip(qn[..., :1], -1.0, 1.0))
    axis = xyz / np.sqrt(np.where(ident, 1.0, len2))
    axis = np.where(ident, np.array([1.0, 0.0, 0.0]), axis)
    theta = np.where(ident, 0.0, theta)
    return axis * theta


def postprocess_verifier(actions: np.ndarray, stats: Optional[dict] = None) -> np.ndarray:
    """[n,7] normalised policy actions -> verifier format: dims 0-5 un-normalised with p01/p99, gripper 0 if a<0.5 else 1."""
    st = (stats or bridge_statistics())["action"]
    lo, hi = np.array(st["p01"])[:-1], np.array(st["p99"])[:-1]
    out = np.zeros((len(actions), 7))
    out[:, :6] = denormalize_bound(actions[:, :-1], lo, hi)
    out[:, 6] = np.where(actions[:, -1] < 0.5, 0, 1)
    return out


def postprocess_execution(actions: np.ndarray, stats: Optional[dict] = None) -> np.ndarray:
    """[n,7] -> execution format: xyz, axis-angle rotation, gripper 2*(a>0.5)-1."""
    st = (stats or bridge_statistics())["action"]
    lo, hi = np.array(st["p01"])[:-1], np.array(st["p99"])[:-1]
    raw = denormalize_bound(actions[:, :-1], lo, hi)
    out = np.zeros((len(actions), 7))
    out[:, :3] = raw[:, :3]
    out[:, 3:6] = euler2axangle_sxyz(raw[:, 3], raw[:, 4], raw[:, 5])
    out[:, 6] = 2.0 * (actions[:, -1] > 0.5) - 1.0
    return out


def process_inputs(action_queue: Sequence[np.ndarray], verifier_action: bool, action_history: Sequence[np.ndarray],
                   n_action_steps: int = 4, stats: Optional[dict] = None) -> List[np.ndarray]:
    """action_queue: n_action_steps arrays [B,7] (float32 from the policy) -> list of B trajectories [num_past + steps, 7]."""
    fn = postprocess_verifier if verifier_action else postprocess_execution
    fut = np.stack([fn(np.asarray(action_queue[i]), stats) for i in range(n_action_steps)])      # [steps, B, 7]
    fut = fut.transpose(1, 0, 2)
    B = fut.shape[0]
    num_past = min(len(action_history), 6)
    if num_past > 0:
        past = np.stack(list(action_history)[-num_past:])
        full = np.concatenate([np.repeat(past[None], B, axis=0), fut], axis=1)
    else:
        full = fut
    return [full[i] for i in range(B)]


def verify_and_select(verifier, raw_image, task_description: str, task_list: Sequence[str], action_queue, action_history,
                      samples_per_prompt: int, n_action_steps: int = 4, threshold: float = 0.1, stats=None,
                      process_image: bool = True, candidate_prior=None, prior_beta: float = 0.0, member_kappa: Optional[float] = None,
                      member_mode: str = "lcb", smooth: Optional["Smooth"] = None):
    """run_simpler_eval_with_openpi.py:329-401: stage 1 scores candidate 0 under the current instruction; if its score
    is < threshold, stage 2 scores all candidates grouped per prompt; then the gripper majority vote inside the winner's
    prompt group and extraction of the winner's remaining steps.
    action_queue: n_action_steps arrays [B,7] (host). Returns dict(execute_action, max_score, max_instruction,
    global_action_idx, remaining (deque of [1,7]), history_row, prior_beta, member_kappa).
    candidate_prior ([B] sequence log-probabilities of the candidates under the policy, e.g. PI0FASTPolicy.last_sequence_logprobs, or
    [B, steps] per-step values) with prior_beta > 0: stage 2 selects on score + prior_beta * prior (stage 1 scores one candidate: a
    prior cannot change it). The two keywords reach the verifier only then, so a verifier that does not know them keeps working;
    max_score is then the winner's combined score and the dict also carries the winner's `prior`.
    When the candidates were drawn with per-candidate sampling parameters (sampling_ladder), candidate_prior should be the reference
    log-probabilities -- the tensor OpenVLA.sample / generate_tokens return with prior_temperature, or
    PI0FASTPolicy.last_sequence_prior_logprobs -- which score every candidate at ONE temperature, unfiltered; the return_logprobs values
    are taken under each candidate's own rung and do not compare across rungs. No reference temperature or prior_beta is chosen here.
    member_kappa (finite, >= 0; None = off) with member_mode ("lcb" or "min") makes BOTH stages disagreement-aware
    (EfficientEnsembleMerged.score_histories): the stage-1 gate compares candidate 0's robust score -- its fused score less member_kappa
    times the spread of the ensemble members' own scores, or the worst member's score -- with the threshold, a pessimistic gate, and
    stage 2 selects on the robust score (plus the prior, when one is used). The two keywords reach the verifier only when member_kappa
    is not None. The dict carries member_kappa and, when the verifier keeps last_member_stats, the winner's `spread` and
    `member_agreement`, the number of members whose own grouped arg-max is the decision. No member_kappa is recommended.
    smooth (a Smooth; None = off): stage 2 selects on the neighbourhood-smoothed score (EfficientEnsembleMerged.score_histories), the
    smoothed robust score with member_kappa, plus the prior when one is used. Forwarded as candidate_prior is: to stage 2 only (stage 1
    scores one candidate, which has no neighbours), and only when not None. When the verifier keeps last_smooth_stats and stage 2 ran,
    the dict carries the winner's `neighbours`. No radius, scale or shrink is recommended."""
    if smooth is not None and not isinstance(smooth, Smooth):
        raise ValueError("verify_and_select: smooth must be a host.Smooth or None")
    if not (prior_beta >= 0.0 and math.isfinite(prior_beta)):
        raise ValueError(f"verify_and_select: prior_beta must be finite and >= 0 (got {prior_beta})")
    if member_kappa is not None and not (member_kappa >= 0.0 and math.isfinite(member_kappa)):
        raise ValueError(f"verify_and_select: member_kappa must be finite and >= 0 (got {member_kappa})")
    member_kw = {} if member_kappa is None else dict(member_kappa=member_kappa, member_mode=member_mode)
    use_prior = candidate_prior is not None and prior_beta > 0
    B = len(task_list)
    num_past = min(len(action_history), 6)
    hist_v = process_inputs(action_queue, True, action_history, n_action_steps, stats)
    if process_image:      # images_list = [process_raw_image_to_jpg(raw_img)] * B  (run_simpler_eval_with_openpi.py:342)
        from .imaging import process_raw_image_to_jpg
        raw_image = process_raw_image_to_jpg(raw_image)
    images = [raw_image] * B
    max_score, max_instruction, max_hist, gidx = verifier.compute_max_similarity_scores_batch(
        images=images[0:1], instructions=[task_description], all_action_histories=hist_v[0:1],
        cfg_repeat_language_instructions=1, **member_kw)
    stage2 = False
    if max_score < threshold:
        max_score, _, max_hist, gidx = verifier.compute_max_similarity_scores_batch(
            images=images, instructions=[task_description] * B, all_action_histories=hist_v,
            cfg_repeat_language_instructions=samples_per_prompt,
            **(dict(candidate_prior=candidate_prior, prior_beta=prior_beta) if use_prior else {}), **member_kw,
            **({} if smooth is None else dict(smooth=smooth)))
        max_instruction = task_list[int(gidx)]
        stage2 = True
    gidx = int(gidx)
    hist_e = process_inputs(action_queue, False, action_history, n_action_steps, stats)
    execute_action = hist_e[gidx][num_past].copy()
    g0 = (gidx // samples_per_prompt) * samples_per_prompt
    grippers = np.stack(hist_e[g0:g0 + samples_per_prompt])[:, num_past, -1]
    close_votes, open_votes = int((grippers >= 0).sum()), int((grippers < 0).sum())
    if close_votes > open_votes:
        execute_action[-1] = 1.0
    elif open_votes > close_votes:
        execute_action[-1] = -1.0
    else:
        execute_action[-1] = 1.0 if execute_action[-1] >= 0 else -1.0
    execute_action[-1] = float(np.sign(execute_action[-1]))
    remaining = deque(np.asarray(action_queue[t])[gidx:gidx + 1] for t in range(1, n_action_steps))
    out = dict(execute_action=execute_action, max_score=max_score, max_instruction=max_instruction,
               global_action_idx=gidx, remaining=remaining, history_row=max_hist[num_past].copy(), prior_beta=float(prior_beta))
    if use_prior and stage2:
        out["prior"] = _winner_prior(candidate_prior, gidx)
    out["member_kappa"] = None if member_kappa is None else float(member_kappa)
    stats = getattr(verifier, "last_member_stats", None) if member_kappa is not None else None
    if stats is not None:      # the latest scoring call's: stage 2's when it ran, else stage 1's one candidate
        out["spread"] = float(_host_array(stats["spread"])[gidx])
        out["member_agreement"] = int((_host_array(stats["member_result"])[:, 0] == gidx).sum())
    stats = getattr(verifier, "last_smooth_stats", None) if smooth is not None and stage2 else None
    if stats is not None:
        out["neighbours"] = int(_host_array(stats["neighbours"])[gidx])
    return out


def _host_array(x) -> np.ndarray:
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _winner_prior(candidate_prior, gidx: int) -> float:
    """The selected candidate's sequence log-probability, for the record: [B] as given, [B, steps] summed over its steps."""
    p = candidate_prior[gidx]
    if hasattr(p, "detach"):
        p = p.detach().cpu().numpy()
    return float(np.asarray(p, dtype=np.float64).sum())


class EpisodeLog:
    """The per-episode record the driver pickles (run_simpler_eval_with_openpi.py:238-247 schema; filled at :404-407 on a
    verified decision, :419-422 on a queued step, closed at :454-455) -- the e2e parity artefact analyze_success_rate.py reads.
    Same field names and per-step value types, so records written next to this path load in the reference's analysis."""

    FIELDS = ("verifier_scores", "selected_instructions", "execute_actions", "step_timestamps", "original_task_description",
              "used_task_description", "success", "episode_length")

    def __init__(self, original_task_description: str, task_description: str):
        self.data = {"verifier_scores": [], "selected_instructions": [], "execute_actions": [], "step_timestamps": [],
                     "original_task_description": original_task_description, "used_task_description": task_description,
                     "success": False, "episode_length": 0}

    def record_decision(self, max_score: float, max_instruction: str, execute_action, t: int) -> None:
        d = self.data
        d["verifier_scores"].append(max_score)
        d["selected_instructions"].append(max_instruction)
        d["execute_actions"].append(np.asarray(execute_action).copy())
        d["step_timestamps"].append(t)

    def record_queued(self, task_description: str, execute_action, t: int) -> None:
        d = self.data
        d["verifier_scores"].append(None)
        d["selected_instructions"].append(task_description)
        d["execute_actions"].append(np.asarray(execute_action).copy())
        d["step_timestamps"].append(t)

    def finish(self, success: bool, t: int) -> dict:
        self.data["success"] = success
        self.data["episode_length"] = t
        return self.data

    def save(self, path: str) -> None:
        import pickle
        with open(path, "wb") as f:
            pickle.dump(self.data, f)
