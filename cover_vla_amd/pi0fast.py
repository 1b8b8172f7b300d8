"""pi0-FAST token path on MI355X: the autoregressive action-token head of the reference's second policy family
(lerobot_custom/lerobot/common/policies/pi0fast/modeling_pi0fast.py).

  PI0FAST.generate_actions(batch)                                          :861-884
      embed_inputs(images, img_masks, tokens, pad_mask, ...)               :888-946   image tokens then token embeddings
      pi0_paligemma.generate(inputs_embeds, attention_mask, position_ids, max_new_tokens, do_sample=False)
          block_causal_update_causal_mask                                   :236-330   prefix bidirectional, generated tokens causal
          prepare_inputs_for_generation                                     :333-386   positions 1-indexed
      extract_actions -> decode_actions_with_fast                           :794-859, :735-792

Boundary here = token ids in, token ids out: `PI0FASTTokens.generate_tokens` takes what `embed_inputs` takes (camera
frames, prompt token ids, pad mask) and returns what `generate` returns (the greedy new tokens, pad after EOS). The two
tokenizers on either side -- PaliGemma's sentencepiece model and the `physical-intelligence/fast` BPE + DCT processor --
are un-vendored downloads: the text side is the caller's, the DCT half of the de-tokeniser is `fast_coefficients_to_actions`
with the BPE decoder injected.

Same kernels as the OpenVLA profile's decode loop (prefill GEMMs, weight-streaming decode GEMMs, KV cache segments, lm_head +
arg-max on the device) on PaliGemma's Gemma-2B geometry: MQA 8:1, head_dim 256, tied lm_head over the 257 152-entry
vocabulary. Work that is done once instead of per step: the prefix (image + prompt) is prefilled once and cached; HF
`generate` does the same through its KV cache.
"""
from __future__ import annotations

import os
from collections import deque
from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .host import TopLogprobs
from .ops import RowParam
from .models import BF, Decoder, KvGeometry
from .paligemma import PaliGemmaPrefix, frames_shared, normalize_state, row_groups, sub_state, unnormalize_action
from .sampling import PickPlan, StepOutputs


def prefix_groups(tokens, pad_mask) -> Tuple[np.ndarray, np.ndarray]:
    """paligemma.row_groups over (tokens [B, L], pad_mask [B, L]): rows that are equal in both form a group, numbered in order of
    first occurrence; (first int64 [P], slot int64 [B]) with tokens[first][slot] == tokens."""
    if len(tokens.shape) != 2 or tuple(pad_mask.shape) != tuple(tokens.shape):
        raise ValueError("prefix_groups: tokens and pad_mask must be [B, L] of one shape")
    return row_groups(tokens, pad_mask)


class _Prefilled(NamedTuple):
    """What PI0FASTTokens._prefill hands to _decode."""
    h: torch.Tensor           # bf16 [B, D]: the hidden row the first new token is picked from
    plen: torch.Tensor        # int32 [B]: valid keys of each row's prefix
    slot_t: torch.Tensor      # int32 [B]: the prefix slot each row reads
    Tp: int                   # prefix width


class PI0FASTTokens:
    def __init__(self, sd: Dict[str, torch.Tensor], c: dict, *, device="cuda:0", max_batch=64, max_prompt=96, max_new_tokens=256,
                 n_cams=1, max_prompts=None):
        """sd: neutral state dict with vision.*, projector.*, lm.* (cover_vla_amd.synth.pi0_state layout / loader output);
        c: size dict (lm_dim, lm_mlp, layers, Hq, Hkv, D, vocab, vit_*, patch, image).
        max_prompts: slots of the prefix region of the KV cache (None = max_batch). `generate_tokens(share_prefix=True)` holds one
        prefix per DISTINCT (frames, prompt): a model for 8 prompts x 5 samples is built with max_prompts=8, max_batch=40. Calls
        without share_prefix prefill every row, so they need max_prompts >= their batch."""
        self.c, self.dev = dict(c), torch.device(device)
        self.pg = pg = PaliGemmaPrefix(sd, c, device=device, n_cams=n_cams)
        self.vit, self.projector, self.embed, self.emb_scale = pg.vit, pg.projector, pg.embed, pg.emb_scale
        self.n_img, self.n_cams = pg.n_img, n_cams
        self.lm_head = ops.pack_linear(self.embed)                       # tied (PaliGemma ties lm_head to embed_tokens)
        self.Tp_cap = self.n_img * n_cams + max_prompt
        self.max_prompts = max_batch if max_prompts is None else int(max_prompts)
        geom = KvGeometry(c["Hkv"], c["D"], [self.max_prompts, max_batch], [self.Tp_cap, max_new_tokens])
        self.lm = Decoder(sub_state(sd, "lm."), dim=c["lm_dim"], layers=c["layers"], Hq=c["Hq"], Hkv=c["Hkv"], D=c["D"], mlp=c["lm_mlp"],
                          act="gelu_tanh", norm="gemma", eps=1e-6, rope="hf", n_pos=self.Tp_cap + max_new_tokens + 8, device=device,
                          cache=geom)
        self.max_batch, self.max_prompt, self.max_new = max_batch, max_prompt, max_new_tokens
        self.eos_check_every = 8          # decode steps between `done.all()` read-backs (0 = never stop early)

    def generate_tokens(self, images: List[torch.Tensor], img_masks: List[torch.Tensor], tokens: torch.Tensor, pad_mask: torch.Tensor,
                        max_new_tokens: int, eos_token_id: int = 1, pad_token_id: int = 0,
                        force_tokens: Optional[torch.Tensor] = None, trace: Optional[dict] = None,
                        uniforms: Optional[torch.Tensor] = None, temperature: RowParam = 1.0, top_k: RowParam = 0,
                        top_p: RowParam = 1.0, return_logprobs: bool = False, share_prefix: bool = False, top_logprobs: int = 0,
                        allowed_tokens: Optional[ops.TokenAllow] = None, prior_temperature: Optional[float] = None, grammar=None):
        """images: list (cameras) of [B,3,H,W]; tokens int64 [B,L] RIGHT padded with pad_mask [B,L] (the reference pads left for
        generation: positions come from the cumulative pad mask and padded keys are masked, so the side does not enter the
        arithmetic). Returns int64 [B, max_new_tokens] on the device: the greedy continuation, `pad_token_id` after a row's EOS
        (what `generate(do_sample=False)` returns after the prompt). force_tokens (tests): teacher-force the fed-back tokens.
        uniforms fp32 [B, max_new_tokens] on the device, temperature / top_k / top_p (scalars or length-B sequences / tensors), return_logprobs,
        top_logprobs and prior_temperature: the sampling arguments cover_vla_amd.sampling documents (S = max_new_tokens steps, the range is the
        vocabulary; a sampled scalar call is always ops.token_sample, a per-row one ops.token_sample_rows). Sampled and per-row calls decode every row
        on its own (no greedy de-duplication): rows that share frames and prompt diverge with their uniforms. With return_logprobs / prior_temperature
        the return is a tuple; steps at which a row emits `pad_token_id` because it has finished, and steps the early stop skips, carry
        0.0 in both (a row sum is the sequence log-probability, host.sequence_logprob) and -1 / -inf / 0.0 in TopLogprobs.
        share_prefix: rows with equal (frames, prompt) share ONE prefilled prefix (greedy, sampled and forced alike): the prefill
        runs over the P distinct rows, every candidate row still decodes and picks on its own, reading its prompt's prefix K/V through
        the segment's slot_of_batch. Needs P <= max_prompts and B <= max_batch. GEMM row counts differ from the per-row path, so
        results agree with it to bf16 rounding (bit for bit when P == B). The default launches exactly what it launched before.
        allowed_tokens = ops.TokenAllow (bits over the vocabulary's ids, optionally set_of_row int32 [B]): every row draws from its set
        only -- each step's pick is ONE cover_token_sample_rows_allowed launch (scalar parameters are broadcast through
        ops.row_param_tensors; uniforms None = temperature 0 for every row, and rows are decoded on their own: no greedy
        de-duplication), return_logprobs and top_logprobs are taken under the restricted distribution (the allowed scorer and ranker).
        The sets are validated on the host once (one read-back), CoverError otherwise: set_of_row has B entries inside [0, n_sets) and
        every set a row names holds an id below the vocabulary size, so no pick is the -1 of an invalid row. share_prefix,
        force_tokens, the EOS / pad bookkeeping (a finished row's pad is not a draw and need not be allowed) and the fused feedback are
        untouched. None launches exactly what it launched before.
        grammar = host.TokenGrammar(allow, fsm) (host.length_grammar builds one; exclusive with allowed_tokens, it carries its own sets):
        a token-class automaton per candidate row chooses the set every step's pick draws from. Each row starts in fsm.start_state, so
        the first pick reads that state's set; between two steps the row's automaton advances on the token it emitted (sampled, greedy
        and teacher-forced alike; a finished row stops moving) and the next pick -- the same cover_token_sample_rows_allowed launch as
        with allowed_tokens -- reads the new state's set. With share_prefix the step's feedback launch is cover_decode_feedback_fsm
        and nothing returns to the host; otherwise (and with COVER_FAST_FEEDBACK=0) the same update runs in device tensors
        (ops.TokenFsm.step_torch). return_logprobs, prior_temperature and top_logprobs are taken under each step's own set; a forced
        token outside the current set scores -inf. ops.token_fsm_check runs once before the loop (CoverError names a reachable state
        whose set is empty), so no pick is the -1 of an invalid row. The state is per candidate row, never per prompt slot.
        None launches exactly what it launched before."""
        dev = self.dev
        fsm = None
        if grammar is not None:
            if allowed_tokens is not None:
                raise ValueError("grammar and allowed_tokens are mutually exclusive: a grammar carries its own sets")
            g_allow, g_fsm = grammar
            if not isinstance(g_allow, ops.TokenAllow) or not isinstance(g_fsm, ops.TokenFsm):
                raise ops.L.CoverError("grammar must hold an ops.TokenAllow and an ops.TokenFsm (host.TokenGrammar)")
            if g_fsm.vocab != self.c["vocab"]:
                raise ops.L.CoverError(f"grammar: class_of_token has {g_fsm.vocab} entries, the vocabulary {self.c['vocab']}")
            if g_allow.bits.device != dev:
                raise ops.L.CoverError(f"grammar: the allowed-token bits must be on {dev}")
            ops.token_fsm_check(g_fsm, g_allow, 0, self.c["vocab"])
            state, set_of_row = g_fsm.rows(tokens.shape[0], dev)
            allowed_tokens = ops.TokenAllow(g_allow.bits, set_of_row)     # the picks read the tensor the feedback step rewrites
            fsm = (g_fsm, state, set_of_row)
        plan = PickPlan.resolve("generate_tokens", "row", tokens.shape[0], dev, has_uniforms=uniforms is not None, params=(temperature, top_k, top_p),
                                top_logprobs=top_logprobs, prior_temperature=prior_temperature, allow=allowed_tokens, filter_always=True)
        u_t = None
        if uniforms is not None:
            if tuple(uniforms.shape) != (tokens.shape[0], max_new_tokens):
                raise ValueError("uniforms must be [B, max_new_tokens]")
            u_t = uniforms.to(device=dev, dtype=torch.float32).t().contiguous()       # step-major: row i is step i's [B]
        if allowed_tokens is not None and fsm is None:
            self._check_allowed(allowed_tokens, tokens.shape[0])
        # Greedy decoding is a function of (frames, prompt): candidates that share both (the samples of one rephrased prompt)
        # are generated once and the tokens broadcast -- index bookkeeping on the host, B x 2L integers
        if (allowed_tokens is None and not share_prefix and uniforms is None and force_tokens is None and tokens.shape[0] > 1
                and all(frames_shared(im) for im in images)):
            first, slot = row_groups(tokens, pad_mask)
            if first.shape[0] < tokens.shape[0]:
                fi = torch.from_numpy(first).to(dev)
                sub_out = self.generate_tokens([im[fi] for im in images], [m[fi] for m in img_masks], tokens[fi], pad_mask[fi],
                                               max_new_tokens, eos_token_id, pad_token_id, None, trace, return_logprobs=return_logprobs,
                                               top_logprobs=top_logprobs)
                back = torch.from_numpy(slot).to(dev)
                if not isinstance(sub_out, tuple):
                    return sub_out[back]
                return tuple(TopLogprobs(*(t[back] for t in o)) if isinstance(o, TopLogprobs) else o[back] for o in sub_out)
        res = self._generate((images, img_masks, tokens, pad_mask), max_new_tokens, (eos_token_id, pad_token_id), force_tokens, trace, u_t,
                             plan, return_logprobs, share_prefix, fsm)
        return res if len(res) > 1 else res[0]

    def _check_allowed(self, allow, B):
        """generate_tokens' host check of its allowed-token sets (one read-back of the bits and the row indices)."""
        if not isinstance(allow, ops.TokenAllow):
            raise ops.L.CoverError("allowed_tokens must be an ops.TokenAllow")
        vocab = self.c["vocab"]
        if allow.bits.shape[1] * 32 < vocab:
            raise ops.L.CoverError(f"allowed_tokens: {allow.bits.shape[1]} words per set do not cover the {vocab} ids of the vocabulary")
        used = np.zeros(1, dtype=np.int64)
        if allow.set_of_row is not None:
            if allow.set_of_row.numel() != B:
                raise ops.L.CoverError(f"allowed_tokens: set_of_row must have one entry per row ({B})")
            used = np.unique(allow.set_of_row.detach().cpu().numpy().astype(np.int64))
            if used[0] < 0 or used[-1] >= allow.n_sets:
                raise ops.L.CoverError(f"allowed_tokens: set_of_row must lie in [0, {allow.n_sets})")
        words = allow.bits.detach().cpu().view(torch.int32).numpy().view(np.uint32)[used, :(vocab + 31) // 32].copy()
        if vocab & 31:
            words[:, -1] &= np.uint32((1 << (vocab & 31)) - 1)
        if not np.all(words.any(axis=1)):
            raise ops.L.CoverError(f"allowed_tokens: a set that a row uses allows no id below the vocabulary size {vocab}")

    def _generate(self, inputs, max_new_tokens, stop_ids, force_tokens, trace, u_t, plan, return_logprobs, share, fsm=None):
        """The one prefill + decode loop; returns StepOutputs.result(): (tokens[, logprobs][, prior][, TopLogprobs]).
        inputs = (images, img_masks, tokens, pad_mask), stop_ids = (eos_token_id, pad_token_id), plan the call's sampling.PickPlan.
        Region 0 of the cache holds P prefixes, region 1 every row's own tokens (slot b).
        share False: P = B, every row prefills its own prefix; between two steps the torch statements, one ops.embed_gather and, every
        `eos_check_every` steps, the `done.all()` read-back.
        share True: the P distinct prefixes (slots 0..P-1, in order of first occurrence) are prefilled once and every row reads its
        prompt's through segment 0's slot_of_batch; between two steps ONE ops.decode_feedback launch settles the token, the
        log-probability, the done flag, the live count and the next step's embedding row. COVER_FAST_FEEDBACK=0 (read per call) issues
        the torch statements of the other path instead.
        plan.t_ref: the reference score of each pick is settled like the log-probabilities (fused: decode_feedback's lp2).
        fsm (ops.TokenFsm, state int32 [B], set_of_row int32 [B]) or None (plan.allow.set_of_row is then that set_of_row): every step
        advances each row's automaton on its emitted token and rewrites set_of_row for the next pick -- fused: in decode_feedback's
        launch, otherwise TokenFsm.step_torch on device tensors."""
        pre = self._prefill(inputs, max_new_tokens, share, trace)
        return self._decode(pre, max_new_tokens, stop_ids, force_tokens, trace, u_t, plan, return_logprobs, share, fsm)

    def _prefill(self, inputs, max_new_tokens, share, trace) -> _Prefilled:
        """Size checks, the grouping of share_prefix, the prefix of the P prefilled rows, the prefix pass and every row's first hidden row."""
        dev, pg = self.dev, self.pg
        images, img_masks, tokens, pad_mask = inputs
        B, L = tokens.shape
        if (B > (self.max_batch if share else min(self.max_batch, self.max_prompts)) or L > self.max_prompt
                or max_new_tokens > self.max_new or len(images) > self.n_cams):
            raise ValueError("batch / prompt length / new tokens / cameras exceed the sizes this model was built for")
        if len(images) != len(img_masks) or not all(bool(m.to(torch.bool).all()) for m in img_masks):
            raise NotImplementedError("masked-out cameras are not supported on the pi0-FAST path (prepare_images :494-536 "
                                      "produces all-True masks for present cameras)")
        same = [frames_shared(im) for im in images]                                  # the evaluation driver's case: one frame for all rows
        P = B
        take = lambda t: t                           # the rows that are prefilled: all of them, or (share) the first of each group
        slot_t = torch.arange(B, device=dev, dtype=torch.int32)
        if share:
            first = slot = np.arange(B, dtype=np.int64)                              # rows with frames of their own: every row is its own group
            if all(same):
                first, slot = row_groups(tokens, pad_mask)
            P = int(first.shape[0])
            if P > self.max_prompts:
                raise ValueError(f"{P} distinct prompts exceed the {self.max_prompts} prefix slots this model was built for (max_prompts)")
            fi = torch.from_numpy(first).to(dev)
            take = lambda t: t[fi]
            slot_t = torch.from_numpy(slot).to(device=dev, dtype=torch.int32)
        D = pg.D
        n_img_all = self.n_img * len(images)
        Tp = n_img_all + L
        # ---- prefill of the P prefix rows
        x = torch.empty(P, Tp, D, dtype=BF, device=dev)
        for ci, im in enumerate(images):
            pg.place(x, ci * self.n_img, pg.image_tokens(im[:1] if same[ci] else take(im)))       # one frame: broadcast to the P slots
        te = ops.embed_gather(self.embed, take(tokens).reshape(-1).contiguous(), self.emb_scale)
        pg.place(x, n_img_all, te.view(P, L, D))
        if trace is not None:
            trace["prefix_embs"] = x.clone()
            trace["prefill_rows"], trace["prefix_slots"] = P * Tp, P
        plen = (n_img_all + pad_mask.to(torch.int32).sum(dim=1)).to(torch.int32).contiguous()          # [B] valid keys: a contiguous prefix
        pos = (1 + torch.arange(Tp, dtype=torch.int32, device=dev))[None].expand(P, Tp).contiguous()   # 1-indexed (:352-354)
        g0 = self.lm.group(P, Tp, pos.view(-1), [dict(region=0, length=Tp, len_of_batch=take(plen).contiguous())], 0)
        xf = x.view(P * Tp, D)
        self.lm.forward(xf, [g0], final_norm=False)
        # ---- first new token: the last valid position of every row's prompt
        last = (slot_t * Tp + plen - 1).to(torch.int32)
        h = torch.empty(B, D, dtype=BF, device=dev)
        ops.copy_rows(xf, h, B, D, last, None)
        if trace is not None:
            trace["first_hidden"] = h.clone()
        return _Prefilled(h, plen, slot_t, Tp)

    def _decode(self, pre: _Prefilled, max_new_tokens, stop_ids, force_tokens, trace, u_t, plan, return_logprobs, share, fsm):
        """The step loop: pick a token from the hidden row (final norm, lm_head, plan.pick), settle it (feedback), run the next pass."""
        dev, c = self.dev, self.c
        (h, plen, slot_t, Tp), (eos_token_id, pad_token_id) = pre, stop_ids
        B, D = h.shape
        fused = share and os.environ.get("COVER_FAST_FEEDBACK", "1") != "0"
        # HF generate(do_sample=False) stops once every row has emitted EOS (modeling_pi0fast.py:861-946 runs it with
        # max_new_tokens = max_decoding_steps = 256, a FAST sequence is a few dozen tokens): every `eos_check_every` steps `done.all()`
        # (fused: live[i - 1]) is read back, and the rest of `out` is the pad the finished rows would have emitted anyway
        outs = StepOutputs.alloc(max_new_tokens, B, dev, logit=False, logprob=return_logprobs, ref=plan.t_ref is not None, n_top=plan.n_top, fill=pad_token_id)
        out, lps, rls = outs.tokens, outs.lps, outs.prior
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        live = torch.zeros(max_new_tokens, dtype=torch.int32, device=dev) if fused else None   # live[i]: rows still running after step i
        lp = torch.empty(B, dtype=torch.float32, device=dev) if return_logprobs else None      # each step's scores, settled by the feedback
        rl = torch.empty(B, dtype=torch.float32, device=dev) if rls is not None else None
        force = force_tokens
        if share and force is not None:
            force = force.to(device=dev, dtype=torch.int64)                          # the per-row form moves one column per step
        logits = torch.empty(B, self.lm_head.N, dtype=torch.float32, device=dev)
        head_ws = ops.gemm_workspace(B, self.lm_head.N, self.lm_head.K, dev)
        tsel = torch.empty(B, dtype=torch.int64, device=dev)
        xd = torch.empty(B, D, dtype=BF, device=dev)
        u_none = torch.zeros(B, dtype=torch.float32, device=dev) if plan.rp is not None and u_t is None else None   # greedy rows read no uniform
        fkw = {} if rls is None else dict(lp2=rl, lp2_out=rls)
        if fsm is not None:
            fkw.update(fsm=fsm[0], fsm_state=fsm[1], fsm_set_of_row=fsm[2])
        seg0 = dict(region=0, length=Tp, len_of_batch=plen)
        if share:
            seg0["slot_of_batch"] = slot_t                                           # its prompt's prefix, wherever that was prefilled
        hidden = h                                                                   # step 0 picks from the prefill's last valid row
        for i in range(max_new_tokens):
            if i > 0:
                if force is None and self.eos_check_every > 0 and i % self.eos_check_every == 0:
                    if (int(live[i - 1]) == 0) if fused else bool(done.all()):       # one 4-byte (1-byte) D2H
                        break
                if not fused:
                    ops.embed_gather(self.embed, out[:, i - 1].contiguous(), self.emb_scale, out=xd)
                pos_i = (plen + i).to(torch.int32).contiguous()                       # token i-1 sits at 1-indexed position plen + i
                g = self.lm.group(B, 1, pos_i, [seg0, dict(region=1, length=i)], 1, write_t_off=i - 1)
                self.lm.forward(xd, [g], final_norm=False)
                hidden = xd
            # ---- step i's pick
            hn = ops.rmsnorm(hidden, self.lm.final_norm, 1e-6, w_offset=1.0, style=0)
            lg = ops.gemm(hn, self.lm_head, out=logits, ws=head_ws)
            if trace is not None:
                trace.setdefault("logits", []).append(lg[:, :c["vocab"]].clone())
            t, _, kept = plan.pick(lg, 0, c["vocab"], u_none if u_t is None else u_t[i], out_tok=tsel, out_logprob=lp, out_ref=rl,
                                   top=outs.top_at(i))
            if (u_t is not None or plan.allow is not None) and trace is not None:
                trace.setdefault("picks", []).append(t.clone())
                trace.setdefault("kept", []).append(kept)
            if fused:      # the statements below and the next step's embed_gather, one launch
                ops.decode_feedback(t, done, out, i, eos_token_id, pad_token_id, force=None if force is None else force[:, i], lp=lp,
                                    lp_out=lps, table=self.embed, scale=self.emb_scale, x_out=xd if i + 1 < max_new_tokens else None,
                                    live=live, **fkw)
                continue
            if rl is not None:
                rls[:, i].copy_(torch.where(done, torch.zeros_like(rl), rl))
            if lp is not None:
                lps[:, i].copy_(torch.where(done, torch.zeros_like(lp), lp))          # a finished row's pad is not a choice: 0
            if force is not None:
                t = force[:, i].to(dev)
            t = torch.where(done, torch.full_like(t, pad_token_id), t)               # index bookkeeping: finished rows emit pad
            out[:, i].copy_(t)
            if fsm is not None:
                fsm[0].step_torch(fsm[1], fsm[2], t, ~done)                          # done as it was before this step
            done.logical_or_(t == eos_token_id)
        if outs.top is None:
            return outs.result()
        # a row is finished at step i once an earlier step emitted EOS: its pad is not a choice (index bookkeeping on the emitted tokens)
        eos = out == eos_token_id
        return outs.result(fin=(eos.cumsum(dim=1) - eos.to(torch.int64)) > 0)        # [B, steps]


@dataclass
class PI0FASTConfig:
    """The fields of configuration_pi0fast.PI0FASTConfig the inference path reads."""
    image_keys: Tuple[str, ...] = ("observation.images.top",)
    state_key: str = "observation.state"
    action_dim: int = 7                 # config.action_feature.shape[0]
    chunk_size: int = 10                # action horizon handed to the FAST decoder
    n_action_steps: int = 5
    max_state_dim: int = 32
    max_decoding_steps: int = 256
    fast_skip_tokens: int = 128
    relaxed_action_decoding: bool = True
    resize_imgs_with_padding: Optional[Tuple[int, int]] = (224, 224)
    device: str = "cuda:0"
    # sampled decoding (`generate(do_sample=True, ...)`): sample_seed None = greedy, the reference's setting
    # each of the three: a scalar, or one entry per row of the batch (generate_tokens' per-row form; 0.0 in temperature = a greedy row)
    temperature: RowParam = 1.0
    top_k: RowParam = 0
    top_p: RowParam = 1.0
    sample_seed: Optional[int] = None
    return_logprobs: bool = False       # keep each row's sequence log-probability of the last generation (last_sequence_logprobs)
    top_logprobs: int = 0               # keep the n most probable tokens / log-probabilities / entropy of every step (last_top_logprobs)
    # T_ref: keep each row's sequence log-probability under ONE reference temperature, unfiltered (last_sequence_prior_logprobs): the prior
    # that compares across rows with different (temperature, top_k, top_p); needs sample_seed. None = not computed
    prior_temperature: Optional[float] = None
    share_prefix: bool = False          # candidates with equal frames and prompt share one prefill (generate_tokens(share_prefix=True))
    # half-open (a, b) ranges of PaliGemma ids every row may draw (generate_tokens(allowed_tokens=)): the FAST band from
    # fast_action_token_range plus (b = a + 1) the format tokens; the EOS id is always added. None = the whole vocabulary
    allowed_token_ranges: Optional[Sequence[Tuple[int, int]]] = None
    # host.TokenGrammar (fast_chunk_grammar / host.length_grammar): a per-row automaton picks each step's allowed set
    # (generate_tokens(grammar=)); exclusive with allowed_token_ranges. None = no grammar
    token_grammar: Optional[object] = None
    # de-tokenise on the device (PI0FASTPolicy.extract_actions_device: one ops.fast_decode launch on the generated ids, no host copy)
    # instead of extract_actions' text round trip. Defined on ids, so not the reference's text artefacts: off by default. With it the
    # caller supplies, as for allowed_token_ranges, the size of the FAST BPE vocabulary, the PaliGemma id of the terminator "|" and the
    # ids of the format tokens ("Action", ":"; the tokenizer's BOS is always added) that carry no symbols
    device_detokenize: bool = False
    fast_vocab_size: Optional[int] = None
    action_end_token_id: Optional[int] = None
    action_format_token_ids: Sequence[int] = ()


class _DeviceDetokenizer(NamedTuple):
    """What PI0FASTPolicy builds once for extract_actions_device: the arguments of ops.fast_decode that do not change between calls."""
    pieces: ops.FastPieces
    basis: torch.Tensor                 # fp32 [chunk_size, chunk_size] on the device
    band: Tuple[int, int]
    stop_ids: Tuple[int, ...]
    skip_ids: Tuple[int, ...]


class PI0FASTPolicy:
    """PI0FASTPolicy.select_action (modeling_pi0fast.py:193-233) on `PI0FASTTokens`: state discretisation + prompt text
    (`create_input_tokens` :570-640), greedy (or, with `config.sample_seed`, sampled) generation on the device, `extract_actions` (:794-859) and the action queue. The two
    tokenizers are the caller's objects (HF `AutoTokenizer("google/paligemma-3b-pt-224")` and the `physical-intelligence/fast`
    processor in production; `cover_vla_amd.synth.CharTokenizer` in the tests): only the methods the reference calls are used."""

    def __init__(self, config: PI0FASTConfig, model: PI0FASTTokens, paligemma_tokenizer, fast_processor, normalization: Optional[dict] = None):
        self.config, self.model = config, model
        self.paligemma_tokenizer, self.fast_tokenizer = paligemma_tokenizer, fast_processor
        self.normalization = normalization or {"state": ("IDENTITY", None, None), "action": ("IDENTITY", None, None)}
        self.pad_token_id = paligemma_tokenizer.pad_token_id if hasattr(paligemma_tokenizer, "pad_token_id") else paligemma_tokenizer.eos_token_id
        # the source of randomness of sampled decoding: a host generator seeded ONCE, so a seed and an observation sequence fix the actions
        self._gen = None if config.sample_seed is None else torch.Generator().manual_seed(int(config.sample_seed))
        self.last_sequence_logprobs = None        # fp32 [B] on the device, set by a generation that ran with config.return_logprobs
        self.last_sequence_prior_logprobs = None  # fp32 [B] on the device, set by a generation that ran with config.prior_temperature
        self.last_top_logprobs = None             # host.TopLogprobs on the device, set by a generation that ran with config.top_logprobs > 0
        self.allowed_tokens = None                # one set for every row, built once; EOS is always in it, otherwise a row can never finish
        if config.allowed_token_ranges is not None:
            ranges = [(int(a), int(b)) for a, b in config.allowed_token_ranges]
            bits = ops.token_allow_sets(model.c["vocab"], [ranges + [int(paligemma_tokenizer.eos_token_id)]], model.dev)
            self.allowed_tokens = ops.TokenAllow(bits)
        if config.token_grammar is not None and config.allowed_token_ranges is not None:
            raise ValueError("token_grammar and allowed_token_ranges are mutually exclusive: a grammar carries its own sets")
        self.last_chunks = None                   # fp32 [B, chunk_size, action_dim] on the device, before un-normalisation (device_detokenize)
        self.last_decode_status = None            # int32 [B] on the device: the ops.FAST_* bits of each row of last_chunks
        self._detok = self._device_detokenizer() if config.device_detokenize else None
        self.reset()

    def _device_detokenizer(self) -> _DeviceDetokenizer:
        """The piece table (every FAST id decoded on its own by the injected BPE), the IDCT basis and the id sets, on the device, once."""
        from .host import fast_idct_basis, fast_pieces_from_decoder
        c, tok, ft = self.config, self.paligemma_tokenizer, self.fast_tokenizer
        if c.fast_vocab_size is None or c.action_end_token_id is None:
            raise ValueError("device_detokenize needs fast_vocab_size and action_end_token_id (the PaliGemma id of \"|\")")
        band = fast_action_token_range(tok.vocab_size, c.fast_vocab_size, c.fast_skip_tokens)
        stop = dict.fromkeys(int(t) for t in (c.action_end_token_id, tok.eos_token_id, self.pad_token_id))
        skip = dict.fromkeys([int(t) for t in c.action_format_token_ids] + [int(t) for t in [getattr(tok, "bos_token_id", None)] if t is not None])
        pieces = ops.fast_piece_table(fast_pieces_from_decoder(ft.bpe_tokenizer.decode, c.fast_vocab_size), self.model.dev)
        basis = torch.from_numpy(fast_idct_basis(c.chunk_size)).to(self.model.dev)
        return _DeviceDetokenizer(pieces, basis, band, tuple(stop), tuple(skip))

    def reset(self):
        self._action_queue = deque([], maxlen=self.config.n_action_steps)

    # ---- create_input_tokens(state, lang_text, actions=None) :570-640 (generation: the prefix only)
    def create_input_tokens(self, state: torch.Tensor, lang_text: Sequence[str]):
        bins = torch.linspace(-1, 1, 256 + 1, device=state.device)[:-1]
        discretized = (torch.bucketize(state, bins) - 1)[:, :32]
        prefix_texts = []
        for txt, disc in zip(lang_text, discretized):
            cleaned = txt.lower().strip().replace("_", " ")
            state_str = " ".join(str(val.detach()) for val in disc)     # (sic: the reference joins the tensors' repr, :582-585)
            prefix_texts.append(f"Task: {cleaned}, State: {state_str};\n")
        out = self.paligemma_tokenizer(prefix_texts, add_special_tokens=True, return_tensors="pt", padding="longest", truncation=False)
        ids, mask = out["input_ids"], out["attention_mask"]
        # compact every row's valid tokens to the left (a left-padding tokenizer: the side does not enter the arithmetic)
        B, Lp = ids.shape
        order = torch.argsort((mask == 0).to(torch.int8), dim=1, stable=True)
        return torch.gather(ids, 1, order), torch.gather(mask, 1, order)

    # ---- extract_actions(tokens, action_horizon, action_dim) :794-859
    def extract_actions(self, tokens: torch.Tensor, action_horizon: int, action_dim: int) -> torch.Tensor:
        decoded = self.paligemma_tokenizer.batch_decode(tokens, skip_special_tokens=True)
        cleaned = [seq.replace("Action:", "").replace(":", "").strip().split("|")[0].strip() for seq in decoded]
        outs = []
        for text in cleaned:
            raw = self.paligemma_tokenizer.encode(text, return_tensors="pt", padding=False)
            fast_ids = self.paligemma_tokenizer.vocab_size - 1 - self.config.fast_skip_tokens - raw      # _act_tokens_to_paligemma_tokens
            ft = self.fast_tokenizer
            acts = fast_coefficients_to_actions(fast_ids.tolist(), ft.bpe_tokenizer.decode, min_token=ft.min_token, scale=ft.scale,
                                                time_horizon=action_horizon, action_dim=action_dim,
                                                relaxed_decoding=self.config.relaxed_action_decoding)
            outs.append(torch.tensor(acts, device=tokens.device).squeeze(0))
        return torch.stack(outs, dim=0)

    def extract_actions_device(self, tokens: torch.Tensor) -> torch.Tensor:
        """extract_actions on the device (config.device_detokenize): ONE ops.fast_decode launch on the generated ids int64 [B, L], where they
        are -> fp32 [B, chunk_size, action_dim] on the device; each row's ops.FAST_* bits are kept in last_decode_status.
        Defined on ids, not on text: the tokens before the first of ("|", EOS, pad) are walked in order, an id of the FAST band
        contributes its piece's code points (each FAST id decoded on its own by the injected BPE: host.fast_pieces_from_decoder states the
        assumption), the format ids and BOS contribute nothing, and any other id zeroes the row. extract_actions' text round trip --
        batch_decode, string clean-up, encode (which prepends BOS and lets sentencepiece re-segment), the id mirror -- has artefacts that
        are deliberately NOT reproduced, so the two agree where the generated ids are a clean "Action: <band ids>|" and can differ
        elsewhere; that is why the option is off by default."""
        if self._detok is None:
            raise ops.L.CoverError("extract_actions_device needs a policy built with PI0FASTConfig(device_detokenize=True)")
        d, ft = self._detok, self.fast_tokenizer
        dec = ops.fast_decode(tokens, d.pieces, d.basis, band=d.band, stop_ids=d.stop_ids, skip_ids=d.skip_ids, min_token=int(ft.min_token),
                              scale=float(ft.scale), horizon=self.config.chunk_size, action_dim=self.config.action_dim,
                              relaxed=bool(self.config.relaxed_action_decoding), stats=True)
        self.last_decode_status = dec.status
        return dec.actions

    @torch.no_grad()
    def select_action(self, batch: dict) -> torch.Tensor:
        if len(self._action_queue) == 0:
            dev = self.model.dev
            state = normalize_state(batch[self.config.state_key].to(torch.float32), self.normalization["state"])
            present = [k for k in self.config.image_keys if k in batch]
            if not present:
                raise ValueError(f"All image features are missing from the batch. At least one expected. (batch: {batch.keys()})")
            images = []
            for k in present:
                img = batch[k]
                if self.config.resize_imgs_with_padding is not None and tuple(img.shape[-2:]) != tuple(self.config.resize_imgs_with_padding):
                    from . import imaging
                    img = imaging.resize_with_pad(img, *self.config.resize_imgs_with_padding, pad_value=0)
                images.append(img.to(dev))
            ids, mask = self.create_input_tokens(state, batch["task"])
            B = ids.shape[0]
            sampling = dict(return_logprobs=True) if self.config.return_logprobs else {}
            if self.config.top_logprobs:
                sampling.update(top_logprobs=self.config.top_logprobs)
            if self.config.share_prefix:
                sampling.update(share_prefix=True)
            if self.allowed_tokens is not None:
                sampling.update(allowed_tokens=self.allowed_tokens)
            if self.config.token_grammar is not None:
                sampling.update(grammar=self.config.token_grammar)
            if self.config.prior_temperature is not None:
                sampling.update(prior_temperature=self.config.prior_temperature)
            if self._gen is not None:
                u = torch.rand(B, self.config.max_decoding_steps, generator=self._gen, dtype=torch.float32)
                sampling.update(uniforms=u.to(dev), temperature=self.config.temperature, top_k=self.config.top_k, top_p=self.config.top_p)
            toks = self.model.generate_tokens(images, [torch.ones(B, dtype=torch.bool, device=dev) for _ in images], ids.to(dev), mask.to(dev),
                                              self.config.max_decoding_steps, eos_token_id=self.paligemma_tokenizer.eos_token_id,
                                              pad_token_id=self.pad_token_id, **sampling)
            if self.config.top_logprobs:
                toks, self.last_top_logprobs = toks[:-1], toks[-1]
                toks = toks if self.config.return_logprobs or self.config.prior_temperature is not None else toks[0]
            if self.config.prior_temperature is not None:
                from .host import sequence_logprob
                toks, prior = toks[:-1], toks[-1]
                self.last_sequence_prior_logprobs = sequence_logprob(prior)
                toks = toks if self.config.return_logprobs else toks[0]
            if self.config.return_logprobs:
                from .host import sequence_logprob
                toks, lps = toks
                self.last_sequence_logprobs = sequence_logprob(lps)
            if self._detok is not None:
                actions = self.last_chunks = self.extract_actions_device(toks)
            else:
                actions = self.extract_actions(toks.cpu(), self.config.chunk_size, self.config.action_dim)
            actions = actions[:, : self.config.n_action_steps, : self.config.action_dim]
            actions = unnormalize_action(actions.to(torch.float32), self.normalization["action"])
            self._action_queue.extend(actions.transpose(0, 1))
        return self._action_queue.popleft()


def fast_coefficients_to_actions(token_lists: Sequence[Sequence[int]], bpe_decode: Callable[[Sequence[int]], str], *, min_token: int,
                                 scale: float, time_horizon: int, action_dim: int, relaxed_decoding: bool = True) -> np.ndarray:
    """decode_actions_with_fast (:735-792): FAST token ids -> BPE-decoded string whose code points + min_token are the quantised
    DCT coefficients -> (relaxed) truncate / zero-pad to time_horizon x action_dim -> idct(coeff / scale, axis 0, ortho).
    `bpe_decode` is the FAST processor's `bpe_tokenizer.decode` (un-vendored); a sequence that fails to decode yields zeros, as
    in the reference. Host numpy on a few hundred integers."""
    from scipy.fft import idct
    outs = []
    for toks in token_lists:
        try:
            coeff = np.array(list(map(ord, bpe_decode(toks)))) + min_token
            if relaxed_decoding:
                want = time_horizon * action_dim
                diff = want - coeff.shape[0]
                if diff < 0:
                    coeff = coeff[:want]
                elif diff > 0:
                    coeff = np.pad(coeff, (0, diff), mode="constant", constant_values=0)
            coeff = coeff.reshape(-1, action_dim)
            if coeff.shape != (time_horizon, action_dim):
                raise ValueError(f"decoded DCT coefficients have shape {coeff.shape}, expected ({time_horizon}, {action_dim})")
        except Exception:
            coeff = np.zeros((time_horizon, action_dim))
        outs.append(idct(coeff / scale, axis=0, norm="ortho"))
    return np.stack(outs)


def fast_tokens_to_paligemma_tokens(tokens: np.ndarray, vocab_size: int, fast_skip_tokens: int = 128) -> np.ndarray:
    """_act_tokens_to_paligemma_tokens (:538-540): FAST ids live at the top of PaliGemma's vocabulary, mirrored (an involution)."""
    return vocab_size - 1 - fast_skip_tokens - np.asarray(tokens)


def fast_action_token_range(vocab_size: int, fast_vocab_size: int, fast_skip_tokens: int = 128) -> Tuple[int, int]:
    """The half-open band (a, b) of PaliGemma ids that fast_tokens_to_paligemma_tokens maps the FAST ids 0 .. fast_vocab_size - 1 onto:
    what PI0FASTConfig.allowed_token_ranges takes for the action tokens, next to the ids of the format tokens ("Action", ":", "|")."""
    b = int(vocab_size) - int(fast_skip_tokens)
    a = b - int(fast_vocab_size)
    if fast_vocab_size < 1 or a < 0:
        raise ValueError("fast_action_token_range: 1 <= fast_vocab_size <= vocab_size - fast_skip_tokens is required")
    return a, b


def fast_chunk_grammar(config: PI0FASTConfig, min_len: int, max_len: int, *, vocab_size: int, fast_vocab_size: int, end_token_id: int,
                       eos_token_id: int, device=None):
    """host.length_grammar for one FAST action chunk: min_len..max_len ids of the action band (fast_action_token_range with
    config.fast_skip_tokens), then the terminator extract_actions splits at (the PaliGemma id of "|", end_token_id), then the
    tokenizer's EOS. The ids are the caller's tokenizers', as for allowed_token_ranges; "Action" and ":" are outside this grammar, so it
    fits a model that is to emit the band directly. Returns the host.TokenGrammar that PI0FASTConfig.token_grammar and
    generate_tokens(grammar=) take. Nothing uses it by default."""
    from .host import length_grammar
    band = fast_action_token_range(vocab_size, fast_vocab_size, config.fast_skip_tokens)
    return length_grammar(vocab_size, band, [int(end_token_id)], [int(eos_token_id)], min_len, max_len, device=device)
