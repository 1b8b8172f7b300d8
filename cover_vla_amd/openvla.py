"""OpenVLA-7B / Prismatic candidate sampler (profile P2: the shapes BASELINE.json's metric is quoted on).

No OpenVLA code exists in the reference; this profile assembles the same kernel library
into DINOv2-L/14 + SigLIP-So400m/14 (features of the second-to-last block) -> 3-layer GELU projector -> Llama-2-7B ->
7 action tokens per step (256 bins, the de-tokeniser arithmetic the reference carries at
INT-ACT/src/experiments/policies/policy_wrapper.py:259-266). Its parity pin is the CPU oracle
(oracle/cover_ref/openvla.py), itself pinned to HF transformers modules.

Work that is provably identical across candidates is done once:
  * both vision towers and the projector: once per camera frame
  * Llama prefill: the [BOS + 256 patch] prefix is causal, so its K/V do not depend on the prompt -> ONE shared
    prefix segment; each distinct prompt only adds its ~20 text tokens. Prefix rows and all prompts' text rows go
    through the 32 layers in a single pass (one read of the 13.5 GB of weights).
  * decode: all N candidates advance together (M = N rows per weight pass); every candidate attends
    [shared image prefix | its prompt's text | its own generated tokens] as three KV segments, no copies.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import os
import weakref

import numpy as np
import torch

from . import _lib as L
from . import host, ops
from .graphs import ReplayGraph
from .ops import RowParam
from .models import BF, Decoder, KvGeometry, VitTower, _f32
from .sampling import PickPlan, StepOutputs

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# What the decode loop of one decision reads and writes, the decision's own tensors (eager) or a shape's static buffers (graph):
# prompt_of_cand / cand_len / last_row int32 [N], pos_all int32 [n_gen, N], u step-major uniforms fp32 [n_gen, N] or None, prompt_slots /
# prompt_lens int32 [P], outs the StepOutputs, fed int64 [n_gen, N] the tokens fed back (outs.tokens, or the forced ones)
_DecodeState = NamedTuple("_DecodeState", [(f, object) for f in ("prompt_of_cand", "cand_len", "last_row", "pos_all", "u", "prompt_slots",
                                                                  "prompt_lens", "outs", "fed")])


class OpenVLA:
    def __init__(self, sd: Dict[str, torch.Tensor], c: dict, *, device="cuda:0", max_prompts=8, max_candidates=32,
                 max_text=32, horizon=1, n_cams=1, weight_dtype="bf16", own_kv=None):
        """weight_dtype "fp8" (BASELINE config 5): the Llama projections and the lm_head are quantised to e4m3 with per-channel
        power-of-two scales (cover_vla_amd.ops.pack_linear). Passes with at most 64 rows (the decode passes up to N = 64) stream the e4m3
        weight image with bf16 activations -- bit-identical to a bf16 GEMM on the de-quantised weights. Passes with MORE than 64 rows --
        the 448-row prefill of every fp8 run, and every decode pass of config 5 (N = 512) -- also quantise the input rows of each
        projection to e4m3 (per-row power-of-two scale) and run on the MX-scaled fp8 MFMA; COVER_FP8_MFMA=0 keeps those passes on the
        bf16 MFMA with the bf16 image of the same quantised weights (weights-only quantisation). The vision towers and the projector
        stay bf16.
        own_kv "bf16" / "fp8" (large N, config 5): the candidates' own-token KV segment is kept head-major (K and V [slot][h][t][d],
        bf16 or e4m3 with per-row scales = the "fp8 KV" of config 5) and every decode pass runs the own-token VALU pass + ONE MFMA pass
        over [shared prefix | prompt text] instead of the fused 16-candidate kernel (cover_decode_own_attention). None = legacy layout."""
        self.c, self.dev = dict(c), torch.device(device)
        dev = self.dev
        sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
        self.n_patches = (c["image"] // c["patch"]) ** 2
        self.n_cams = n_cams
        # second-to-last block features: only layers-1 blocks are ever executed, so only those are packed
        self.dino = VitTower(sub("dino."), dim=c["dino_dim"], layers=c["dino_layers"], heads=c["dino_heads"], mlp=c["dino_mlp"],
                             patch=c["patch"], act="gelu_erf", eps=1e-6, layerscale=True, prefix_tokens=c["dino_prefix"],
                             device=device, n_layers_used=c["dino_layers"] - 1)
        self.siglip = VitTower(sub("siglip."), dim=c["sig_dim"], layers=c["sig_layers"], heads=c["sig_heads"], mlp=c["sig_mlp"],
                               patch=c["patch"], act="gelu_tanh", eps=1e-6, device=device, n_layers_used=c["sig_layers"] - 1)
        self.fused = c["dino_dim"] + c["sig_dim"]
        self.proj = [ops.pack_linear(sd[f"projector.fc{i}.weight"].to(dev), sd[f"projector.fc{i}.bias"]) for i in (1, 2, 3)]
        self.embed = sd["llm.embed_tokens.weight"].to(BF).contiguous().to(dev)
        fp8 = weight_dtype == "fp8"
        if weight_dtype not in ("bf16", "fp8"):
            raise ValueError("weight_dtype must be 'bf16' or 'fp8'")
        self.weight_dtype = weight_dtype
        if own_kv not in (None, "bf16", "fp8"):
            raise ValueError("own_kv must be None, 'bf16' or 'fp8'")
        self.own_kv = own_kv
        self.lm_head = ops.pack_linear(sd["lm_head.weight"].to(dev), fp8=fp8)
        # Sampling draws from the softmax over the n_bins ACTION tokens only (the last n_bins entries of the tokenizer vocabulary,
        # policy_wrapper.py:259-266): their logits are n_bins rows of the lm_head -- 2 MB instead of the 262 MB the full head streams
        # per step. Same rows, same arithmetic, same logits for those tokens; greedy decoding (arg-max over the whole vocabulary)
        # and traced runs keep the full head. Opt-in (slice_action_head below).
        lo, hi = c["tok_vocab"] - c["n_bins"], c["tok_vocab"]
        self.lm_head_actions = ops.pack_linear(sd["lm_head.weight"][lo:hi].to(dev), fp8=fp8)
        self.n_gen = 7 * horizon
        self.T0 = 1 + self.n_patches * n_cams          # [BOS] + patches
        geom = KvGeometry(c["Hkv"], c["D"], [1, max_prompts, max_candidates], [self.T0, max_text, self.n_gen])
        self.llm = Decoder(sub("llm."), dim=c["llm_dim"], layers=c["llm_layers"], Hq=c["Hq"], Hkv=c["Hkv"], D=c["D"],
                           mlp=c["llm_mlp"], act="silu", norm="llama", eps=1e-5, rope="hf", n_pos=self.T0 + max_text + self.n_gen + 8,
                           device=device, cache=geom, fp8_weights=fp8)
        self.max_prompts, self.max_candidates, self.max_text = max_prompts, max_candidates, max_text
        # the largest pass this model can run (patch rows + every prompt's text rows): sized once, so that the decode graphs captured for
        # one (P, Lt) never see the workspace move when a later decision has more prompt rows
        self.llm.reserve(self.T0 + max_prompts * max_text)
        D = c["llm_dim"]
        self.action_lo = c["tok_vocab"] - c["n_bins"]
        self.action_hi = c["tok_vocab"]
        # static buffers (fixed addresses -> the whole decision can be captured in a hipGraph)
        self.x_pre = torch.empty(self.T0 + max_prompts * max_text, D, dtype=BF, device=dev)
        self.x_dec = torch.empty(max_candidates, D, dtype=BF, device=dev)
        self.h_sel = torch.empty(max_candidates, D, dtype=BF, device=dev)
        self.logits = torch.empty(max_candidates, c["vocab"], dtype=torch.float32, device=dev)
        self.head_ws = ops.gemm_workspace(max_candidates, c["vocab"], D, dev)
        self.logits_actions = torch.empty(max_candidates, c["n_bins"], dtype=torch.float32, device=dev)
        self.head_ws_actions = ops.gemm_workspace(max_candidates, c["n_bins"], D, dev)
        self.hn = torch.empty(max_candidates, D, dtype=BF, device=dev)
        self.kept_sel = torch.empty(max_candidates, dtype=torch.int32, device=dev)   # ops.token_sample's kept-set sizes (last step's)
        self.zero_slots = torch.zeros(max(max_prompts, max_candidates), dtype=torch.int32, device=dev)
        self.bos = torch.tensor([1], dtype=torch.int64, device=dev)
        self._side = None
        # what the replayed bodies kept in _vis / _dec reach this model through: a strong reference would leave a dropped model to the cyclic collector
        self._weak = weakref.proxy(self)
        self._vis = {}
        self._bos_ready = False
        # measurement switches (bench.py's profiled decision): hipGraph replay hides launches from the in-library kernel
        # timer, and the SigLIP tower on a side stream inflates the durations of the kernels it overlaps
        self.vision_graph = os.environ.get("COVER_VISION_GRAPH", "1") != "0"
        # opt-in (COVER_ACTION_HEAD=1 or the attribute): measured 34.18-34.48 vs 34.26-34.28 ms per decision at N = 32 -- the seven
        # lm_head launches hide behind the host work between decode passes -- so the default keeps the full head
        self.slice_action_head = os.environ.get("COVER_ACTION_HEAD", "0") == "1"
        self.vision_overlap = True
        # the head + decode loop of a decision (first action token, then n_gen - 1 passes of 32 layers + head: ~1 350 launches at 7 B) replayed
        # as ONE hipGraph over static buffers: bit-identical to the eager loop; the GPU time is the same (the loop is
        # GPU-bound), the host is done with a decision's policy side after the prefill. COVER_DECODE_GRAPH=0 keeps the eager loop.
        self.decode_graph = os.environ.get("COVER_DECODE_GRAPH", "1") != "0"
        self._dec = {}

    def _ensure_bos_kv(self):
        """The BOS token sits at position 0 of a causal prefix: it attends only to itself, so its hidden states and its K/V
        in every layer depend on nothing but the weights. They are computed once (a 1-row pass) and stay in slot 0 /
        position 0 of the shared cache segment; every decision then prefills 256 patch rows + the text rows =
        448 = 7 x 64 rows instead of 449 (a whole 64-row GEMM tile for one row, 12.5 % of the prefill)."""
        if self._bos_ready:
            return
        x = ops.embed_gather(self.embed, self.bos)
        pos = torch.zeros(1, dtype=torch.int32, device=self.dev)
        g = self.llm.group(1, 1, pos, [dict(region=0, length=1, mask=ops.MASK_CAUSAL)], 0)
        self.llm.forward(x, [g], final_norm=False)
        self._bos_ready = True

    # ---------------------------------------------------------------------------------------------- vision
    def _vision_static(self, n, H, W):
        key = (n, H, W)
        st = self._vis.get(key)
        if st is None:
            c, P, dev = self.c, self.n_patches, self.dev
            bufs = dict(frame=torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev),
                        d=self.dino.static_bufs(n, H, W), s=self.siglip.static_bufs(n, H, W),
                        fused=torch.empty(n * P, self.fused, dtype=BF, device=dev),
                        h=[torch.empty(n * P, lin.n_out, dtype=BF, device=dev) for lin in self.proj],
                        ws=[ops.gemm_workspace(n * P, lin.N, lin.K, dev) for lin in self.proj])
            me, dino, siglip = self._weak, self.dino, self.siglip
            st = self._vis[key] = dict(bufs, graph=ReplayGraph(lambda: me._encode_static(bufs), dev, gen=lambda: (dino.ws_gen, siglip.ws_gen)))
        return st

    def _encode_static(self, st) -> torch.Tensor:
        """Both towers + projector on persistent buffers (no allocation: recordable into a hipGraph)."""
        c = self.c
        n, P = st["frame"].shape[0], self.n_patches
        mul_d = [1.0 / (255.0 * s) for s in IMAGENET_STD]
        add_d = [-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]
        # the two towers are independent and individually too small to fill 256 CUs: run SigLIP on a side stream
        main = torch.cuda.current_stream()
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        side = self._side if self.vision_overlap else main
        side.wait_stream(main)
        with torch.cuda.stream(side):
            xs = self.siglip.embed(st["frame"], [1.0 / (255.0 * 0.5)] * 3, [-1.0] * 3, bufs=st["s"])
            xs = self.siglip.forward(xs)
        xd = self.dino.embed(st["frame"], mul_d, add_d, bufs=st["d"])
        xd = self.dino.forward(xd)
        main.wait_stream(side)
        fused = st["fused"].view(n, P, self.fused)                       # channel concat (strided device copies)
        fused[:, :, :c["dino_dim"]].copy_(xd[:, c["dino_prefix"]:, :])
        fused[:, :, c["dino_dim"]:].copy_(xs)
        h = ops.gemm(st["fused"], self.proj[0], act="gelu_erf", out=st["h"][0], ws=st["ws"][0])
        h = ops.gemm(h, self.proj[1], act="gelu_erf", out=st["h"][1], ws=st["ws"][1])
        return ops.gemm(h, self.proj[2], out=st["h"][2], ws=st["ws"][2])

    def encode_image(self, frame_u8: torch.Tensor) -> torch.Tensor:
        """frame uint8 [n_cams, H, W, 3] -> projected patch embeddings bf16 [n_cams*256, llm_dim] (a persistent buffer,
        overwritten by the next call). The ~400 launches of the two towers are recorded into a hipGraph on first use
        (COVER_VISION_GRAPH=0 disables): queued one after the other from the host, the second tower starts ~1 ms late."""
        n, H, W, _ = frame_u8.shape
        st = self._vision_static(n, H, W)
        st["frame"].copy_(frame_u8)
        if not self.vision_graph:
            return self._encode_static(st)
        st["graph"].run()                                                # stale when a tower workspace moved (a larger frame batch ran since)
        return st["h"][2]

    # ---------------------------------------------------------------------------------------------- sampler
    def _prefill(self, frame_u8, prompt_tokens, mark=lambda name: None, on_vision_enqueued=None, on_prefill_enqueued=None):
        """Vision pass and prefill of one decision (sample and beam_search): the patch rows and the P x Lt text rows through the decoder
        in one pass, their K/V left in regions 0 and 1. Returns the pass's rows x (hidden states: the patch rows, then P x Lt text rows)."""
        dev = self.dev
        P, Lt = prompt_tokens.shape
        T0 = self.T0
        Tp = T0 - 1                                   # patch rows; the BOS row is input-independent (see _ensure_bos_kv)
        self._ensure_bos_kv()
        # ---- prefill input rows: the patches (positions 1..Tp) then P x Lt text rows
        x = self.x_pre[: Tp + P * Lt]
        mark("start")
        x[:Tp].copy_(self.encode_image(frame_u8))
        if on_vision_enqueued is not None:
            on_vision_enqueued()
        mark("vision")
        ops.embed_gather(self.embed, prompt_tokens.reshape(-1).contiguous(), out=x[Tp:])
        pos0 = 1 + torch.arange(Tp, dtype=torch.int32, device=dev)
        pos1 = (T0 + torch.arange(Lt, dtype=torch.int32, device=dev))[None].expand(P, Lt).contiguous()
        # patch row t (position t+1) sees keys 0..t+1 of the shared segment: BOS (cached) + patches up to itself
        g0 = self.llm.group(1, Tp, pos0, [dict(region=0, length=T0, mask=ops.MASK_CAUSAL, causal_offset=1)], 0, write_t_off=1)
        g1 = self.llm.group(P, Lt, pos1.view(-1),
                            [dict(region=0, length=T0, slot_of_batch=self.zero_slots),
                             dict(region=1, length=Lt, mask=ops.MASK_CAUSAL)], 1)
        self.llm.forward(x, [g0, g1], final_norm=False)
        mark("prefill")
        if on_prefill_enqueued is not None:
            on_prefill_enqueued()
        return x

    def _cand_rows(self, prompt_lens, P, Lt, per_prompt):
        """Row bookkeeping of N = P * per_prompt candidates, candidate i of prompt i // per_prompt: (prompt_of_cand, cand_len, last_row --
        the prefill row of the last valid text position, where the first action token is read -- and pos_all [n_gen, N])."""
        dev, T0 = self.dev, self.T0
        N = P * per_prompt
        prompt_of_cand = (torch.arange(N, device=dev) // per_prompt).to(torch.int32)
        cand_len = prompt_lens.to(torch.int32)[prompt_of_cand.long()].contiguous()
        last_row = (T0 - 1 + prompt_of_cand * Lt + cand_len - 1).to(torch.int32)
        pos_all = ((T0 + cand_len)[None, :] + torch.arange(self.n_gen, dtype=torch.int32, device=dev)[:, None]).contiguous()
        return prompt_of_cand, cand_len, last_row, pos_all

    def sample(self, frame_u8: torch.Tensor, prompt_tokens: torch.Tensor, prompt_lens: torch.Tensor, n_samples: int,
               uniforms: Optional[torch.Tensor] = None, temperature: RowParam = 1.0, trace: Optional[dict] = None,
               force_tokens: Optional[torch.Tensor] = None, on_prefill_enqueued=None, on_vision_enqueued=None,
               top_k: RowParam = 0, top_p: RowParam = 1.0, return_logprobs: bool = False, top_logprobs: int = 0,
               prior_temperature: Optional[float] = None):
        """frame_u8 [n_cams,H,W,3] uint8; prompt_tokens int64 [P, Lt] right padded, prompt_lens int32 [P] (device);
        n_samples candidates per prompt (N = P*n_samples, candidate i belongs to prompt i // n_samples);
        uniforms fp32 [N, n_gen], temperature / top_k / top_p (scalars or length-N sequences / tensors), return_logprobs, top_logprobs and
        prior_temperature: the sampling arguments cover_vla_amd.sampling documents (S = n_gen steps). Their range here: a sampled or
        per-candidate call picks over the 256 action tokens [action_lo, action_hi); an all-greedy call (uniforms=None) takes its arg-max
        over the tokenizer vocabulary and is scored over it, whereas a temperature-0 candidate of a per-candidate call takes the arg-max
        over the action bins, the range of its ops.token_sample_rows launch. Scalar top_k <= 0 and top_p >= 1 is the unfiltered ops.token_select path.
        force_tokens int64 [N, n_gen] (tests): teacher-force the fed-back tokens while still
        returning this path's own picks. on_prefill_enqueued: optional callable invoked once the prefill launches are
        queued -- the point where a caller should queue independent side-stream work (the verifier towers): the
        HBM-bound decode passes that follow tolerate concurrent kernels, the MFMA-bound prefill does not.
        Returns (tokens int64 [N, n_gen], selected-logit fp32 [N, n_gen][, logprobs][, prior][, TopLogprobs]).
        The decode graph is keyed on PickPlan.graph_key: on the fact "per-row parameters", not on their values (the three tensors are
        static buffers filled before each replay, so a new ladder is not a new capture), and on the value of prior_temperature."""
        dev = self.dev
        P, Lt = prompt_tokens.shape
        N = P * n_samples
        plan = PickPlan.resolve("sample", "candidate", N, dev, has_uniforms=uniforms is not None, params=(temperature, top_k, top_p),
                                top_logprobs=top_logprobs, prior_temperature=prior_temperature, filter_always=False)

        def mark(name):   # optional phase timing (tools/phases.py): trace["events"] collects (name, event) pairs
            if trace is not None and "events" in trace:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                trace["events"].append((name, ev))

        if P > self.max_prompts or N > self.max_candidates or Lt > self.max_text:
            raise ValueError("prompts/candidates/text length exceed the sizes this model was built for")
        x = self._prefill(frame_u8, prompt_tokens, mark, on_vision_enqueued, on_prefill_enqueued)
        prompt_of_cand, cand_len, last_row, pos_all = self._cand_rows(prompt_lens, P, Lt, n_samples)
        u_t = None if uniforms is None else uniforms.to(torch.float32).t().contiguous()
        new_outs = lambda: StepOutputs.alloc(self.n_gen, N, dev, logit=True, logprob=return_logprobs, ref=plan.t_ref is not None, n_top=plan.n_top, fill=None)
        if self.decode_graph and trace is None and force_tokens is None and not self.slice_action_head:
            # static buffers per batch shape and mode; the per-decision values (prompt lengths -> rows / positions, uniforms, per-row parameters) are copied in
            key = (P, n_samples, Lt) + plan.graph_key(return_logprobs)
            st = self._dec.get(key)
            if st is None:
                outs = new_outs()
                st_plan = plan._replace(rp=None if plan.rp is None else tuple(torch.empty_like(t) for t in plan.rp))
                st_state = _DecodeState(prompt_of_cand.clone(), torch.empty_like(cand_len), torch.empty_like(last_row), torch.empty_like(pos_all),
                                        None if u_t is None else torch.empty_like(u_t), torch.arange(P, dtype=torch.int32, device=dev),
                                        torch.empty(P, dtype=torch.int32, device=dev), outs, outs.tokens)
                # x is the same rows of the static x_pre on every call of this key (P and Lt are part of it), so the body may keep it
                me, llm = self._weak, self.llm
                st = self._dec[key] = dict(graph=ReplayGraph(lambda: me._decode_body(x, st_plan, st_state), dev, gen=lambda: llm.ws_gen), plan=st_plan, state=st_state)
            s = st["state"]
            s.cand_len.copy_(cand_len); s.last_row.copy_(last_row); s.pos_all.copy_(pos_all)
            s.prompt_lens.copy_(prompt_lens.to(torch.int32))
            if u_t is not None:
                s.u.copy_(u_t)
            for dst, src in zip(st["plan"].rp or (), plan.rp or ()):
                dst.copy_(src)
            st["graph"].run()       # stale when the decoder workspace moved under the captured pointer; the eager pass before a capture fills the same buffers
            return s.outs.result()
        outs = new_outs()
        state = _DecodeState(prompt_of_cand, cand_len, last_row, pos_all, u_t, torch.arange(P, dtype=torch.int32, device=dev),
                             prompt_lens.to(torch.int32).contiguous(), outs, outs.tokens if force_tokens is None else force_tokens.t().contiguous())
        self._decode_body(x, plan, state, trace, mark)
        return outs.result()

    def _decode_body(self, x, plan, s, trace=None, mark=lambda name: None):
        """Head on the last prompt rows, then n_gen - 1 decode passes + heads. Launches only (no allocation, no host read): recordable."""
        D, T0 = self.c["llm_dim"], self.T0
        N, P = s.cand_len.shape[0], s.prompt_slots.shape[0]
        Lt = (x.shape[0] - (T0 - 1)) // P             # x: the patch rows, then P x Lt text rows
        ops.copy_rows(x, self.h_sel, N, D, s.last_row, None)
        self._head_pick(self.h_sel[:N], 0, plan, s, trace)
        xd = self.x_dec[:N]
        own = {}
        if self.own_kv is not None:   # regular structure of the batch: the n_samples candidates of prompt p are rows [p S, (p + 1) S)
            own = dict(own_kv=self.own_kv, seg1_group=N // P, seg1_slot_of_group=s.prompt_slots, seg1_len_of_group=s.prompt_lens)
        for i in range(1, self.n_gen):
            ops.embed_gather(self.embed, s.fed[i - 1], out=xd)
            g = self.llm.group(N, 1, s.pos_all[i - 1],
                               [dict(region=0, length=T0, slot_of_batch=self.zero_slots),
                                dict(region=1, length=Lt, len_of_batch=s.cand_len, slot_of_batch=s.prompt_of_cand),
                                dict(region=2, length=i)], 2, write_t_off=i - 1, seg0_shared=True, **own)
            self.llm.forward(xd, [g], final_norm=False)
            self._head_pick(xd, i, plan, s, trace)
            mark(f"decode{i}")

    def _head_pick(self, h, i, plan, s, trace):
        """Norm, head GEMM and step i's plan.pick into row i of the state's output buffers (the top-n slab i with it)."""
        N, o = h.shape[0], s.outs
        u = None if s.u is None else s.u[i]
        # out_kept: written by the filtered pick (ops.token_sample) only
        out = dict(out_logit=o.sel[i], out_kept=self.kept_sel[:N], out_logprob=None if o.lps is None else o.lps[i],
                   out_ref=None if o.prior is None else o.prior[i], top=o.top_at(i))
        hn = self._final_norm(h)
        if not plan.greedy and (trace is None or "events" in trace) and self.slice_action_head:
            lg = ops.gemm(hn, self.lm_head_actions, out=self.logits_actions[:N], ws=self.head_ws_actions)
            t, _, _ = plan.pick(lg, 0, self.c["n_bins"], u, **out)
            torch.add(t, self.action_lo, out=o.tokens[i])
            if o.top is not None:
                o.top[0][i].add_((o.top[0][i] >= 0) * self.action_lo)      # ids as the tokens are; the -1 padding stays
            return
        lg = self._full_head(hn, trace)
        lo, hi = (0, self.c["tok_vocab"]) if plan.greedy else (self.action_lo, self.action_hi)   # greedy: the tokenizer vocabulary
        plan.pick(lg, lo, hi, u, out_tok=o.tokens[i], **out)

    def _final_norm(self, h):
        return ops.rmsnorm(h, self.llm.final_norm, 1e-5, w_offset=0.0, style=1, out=self.hn[:h.shape[0]])

    def _full_head(self, hn, trace):
        """The full lm_head on normed rows, into the static logits buffer; a trace (not a phase-timing one) keeps a clone."""
        lg = ops.gemm(hn, self.lm_head, out=self.logits[:hn.shape[0]], ws=self.head_ws)
        if trace is not None and "events" not in trace:
            trace.setdefault("logits", []).append(lg.clone())
        return lg

    # ---------------------------------------------------------------------------------------------- beam search
    def beam_search(self, frame_u8: torch.Tensor, prompt_tokens: torch.Tensor, prompt_lens: torch.Tensor, n_beams: int, *,
                    trace: Optional[dict] = None):
        """The n_beams most probable DISTINCT action chunks of every prompt found by step-synchronous beam search, each with its exact
        sequence log-probability: the deterministic alternative to n_samples i.i.d. draws of sample(), whose candidates of one prompt
        often coincide under a peaked head. Inputs as sample(); N = P * n_beams, candidate i belongs to prompt i // n_beams.
        Ranking distribution: softmax at temperature 1, unfiltered, over the action bins [action_lo, action_hi) -- the range of a
        per-candidate sample(). Every step is the final norm and the full lm_head, ops.token_topn(n_beams) per row, ops.beam_merge per
        prompt (higher score, then lower beam, then lower rank), and before the next decode pass ops.kv_gather_slots brings each parent's
        own-token K/V into its child's slot; ops.beam_backtrack follows the parents at the end.
        Returns (tokens int64 [N, n_gen], logprobs fp32 [N, n_gen], scores fp32 [N]): scores is the beams' final cumulative
        log-probability, the fp32 left-to-right sum of logprobs; within a prompt the candidates are pairwise distinct and come in
        descending score. (tokens, logprobs) are what ops.prior_select and host.verify_and_select(candidate_prior=...) take.
        The own-token K/V ping-pong between slots [0, N) and [N, 2 N) of the candidates' cache region, so the model must be BUILT WITH
        TWICE THE CANDIDATES: ValueError when 2 * N > max_candidates, when n_beams is outside 1..64, and when own_kv is not None (the
        head-major own-token cache has no gather). The loop is launches only (no host read, no allocation) and runs eagerly.
        trace={}: trace["logits"] gets every step's logits clone, trace["beam"] a dict per step of the raw parent / token / cum of the
        merge (and its inputs cand_tok / cand_lp).
        Out of scope: pi0-FAST, EOS / length handling, allowed sets and grammars, slice_action_head (the full head is used whatever
        that switch says) and hipGraph capture of the loop. stochastic_beam_search is the sampled counterpart."""
        return self._beam_loop("beam_search", frame_u8, prompt_tokens, prompt_lens, n_beams, trace)[:3]

    def stochastic_beam_search(self, frame_u8: torch.Tensor, prompt_tokens: torch.Tensor, prompt_lens: torch.Tensor, n_beams: int,
                               uniforms: torch.Tensor, temperature: float = 1.0, *, trace: Optional[dict] = None):
        """n_beams pairwise DISTINCT action chunks per prompt, an exact sample WITHOUT REPLACEMENT from the policy's sequence distribution
        -- softmax at `temperature`, unfiltered, over the action bins -- by stochastic beam search (Kool, van Hoof and Welling, 2019), at
        the cost of a beam search: sample()'s i.i.d. candidates repeat under a peaked head, beam_search()'s are distinct but no sample.
        Inputs, sizes and ValueErrors as beam_search (the model is built with twice the candidates), plus ValueErrors for uniforms that
        are not fp32 [n_gen, N, n_bins] on the model's device and for temperature <= 0. uniforms[i, r] perturbs the children of beam r
        at step i, one number per action bin; at step 0 only the first row of each prompt is live and the other rows' are unused.
        beam_search's loop with the other list and merge pair: ops.gumbel_topn(n_beams) per row -- each child's perturbed score, the row's
        Gumbel-perturbed log-probabilities conditioned on their maximum being the beam's own -- and ops.beam_merge_gumbel per prompt, which
        keeps the n_beams children with the largest perturbed score.
        Returns (tokens int64 [N, n_gen], logprobs fp32 [N, n_gen], scores fp32 [N], perturbed fp32 [N], kappa fp32 [P]): logprobs under
        the softmax at `temperature`, scores their fp32 left-to-right sum, perturbed the candidates' final perturbed scores (<= 0,
        descending within a prompt), kappa the last step's threshold: the perturbed score of the best child that was not kept (-inf if
        none). Candidate s was included with probability q(s) = 1 - exp(-exp(scores[s] - kappa)), so sum_s exp(scores[s]) / q(s) f(s)
        over a prompt's candidates estimates the policy's expectation of f (the paper's importance weights).
        trace={}: as beam_search, each step's dict also holding cand_g, g and kappa.
        Out of scope: as beam_search."""
        return self._beam_loop("stochastic_beam_search", frame_u8, prompt_tokens, prompt_lens, n_beams, trace, uniforms, temperature)

    def _beam_loop(self, what, frame_u8, prompt_tokens, prompt_lens, n_beams, trace, uniforms=None, temperature=1.0):
        """The loop of beam_search (uniforms None: ops.token_topn lists at temperature 1, merged by score) and stochastic_beam_search
        (ops.gumbel_topn lists, merged by perturbed score): prefill, head, per-row lists, merge, kv_gather_slots, decode pass, back-track.
        Returns (tokens, logprobs, scores, perturbed, kappa), the last two None without uniforms."""
        dev = self.dev
        P, Lt = prompt_tokens.shape
        B = int(n_beams)
        if not 1 <= B <= 64:
            raise ValueError(f"{what}: 1 <= n_beams <= 64 is required (got {n_beams})")
        N = P * B
        if self.own_kv is not None:
            raise ValueError(f"{what}: the head-major own-token cache (own_kv) is not supported; build the model with own_kv=None")
        if 2 * N > self.max_candidates:
            raise ValueError(f"{what}: the own-token K/V ping-pong between two sets of N = {N} slots: build the model with "
                             f"max_candidates >= {2 * N} (twice the candidates; it has {self.max_candidates})")
        if P > self.max_prompts or Lt > self.max_text:
            raise ValueError("prompts/text length exceed the sizes this model was built for")
        S, T0, lo, hi = self.n_gen, self.T0, self.action_lo, self.action_hi
        keyed = uniforms is not None
        if keyed:
            if not temperature > 0:
                raise ValueError(f"{what}: temperature > 0 is required (got {temperature})")
            if uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (S, N, hi - lo) or uniforms.device != torch.device(dev):
                raise ValueError(f"{what}: uniforms must be fp32 [n_gen, N, n_bins] = [{S}, {N}, {hi - lo}] on {dev} "
                                 f"(got {uniforms.dtype} {tuple(uniforms.shape)} on {uniforms.device})")
            uniforms = uniforms.contiguous()
        x = self._prefill(frame_u8, prompt_tokens)
        prompt_of_cand, cand_len, last_row, pos_all = self._cand_rows(prompt_lens, P, Lt, B)
        # ---- everything the loop touches, allocated here
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        parent = torch.empty(S, N, **i32)
        token, feed = torch.empty(S, N, dtype=torch.int64, device=dev), torch.empty(S, N, dtype=torch.int64, device=dev)
        step_lp = torch.empty(S, N, **f32)
        cum = torch.full((S + 1, N), float("-inf"), **f32)            # row i: the scores step i starts from; row S: the final ones
        cum[0, ::B] = 0.0                                             # the B rows of a prompt carry identical logits at step 0
        cand_tok, cand_lp = torch.empty(N, B, dtype=torch.int64, device=dev), torch.empty(N, B, **f32)
        ent = torch.empty(N, **f32)
        if keyed:                                                     # the perturbed scores, laid out as cum; a root's is 0
            pert = torch.full((S + 1, N), float("-inf"), **f32)
            pert[0, ::B] = 0.0
            cand_g, kappa = torch.empty(N, B, **f32), torch.empty(P, **f32)
        rows = torch.arange(N, **i32)
        slots = (rows, rows + N)                                      # the candidates' slots of pass parity h
        src_base = tuple(s - s % B for s in (rows + N, rows))         # parity h reads parity 1 - h: (1 - h) N + g B, the parent is added per step
        src, dead = torch.empty(N, **i32), torch.empty(N, dtype=torch.bool, device=dev)
        k_tab, vt_tab = self.llm.kv_tables()
        region = self.llm.kv_region(2)
        out_tokens, out_lps = torch.empty(N, S, dtype=torch.int64, device=dev), torch.empty(N, S, **f32)
        xd = self.x_dec[:N]

        def head_merge(h, i):
            lg = self._full_head(self._final_norm(h), trace)
            outs = dict(out_parent=parent[i], out_token=token[i], out_feed=feed[i], out_cum=cum[i + 1], out_step_lp=step_lp[i])
            if keyed:
                ops.gumbel_topn(lg, lo, hi, B, cum[i], pert[i], uniforms[i], temperature, out_tok=cand_tok, out_logprob=cand_lp,
                                out_perturbed=cand_g)
                ops.beam_merge_gumbel(cum[i], cand_tok, cand_lp, cand_g, B, lo, out_g=pert[i + 1], out_kappa=kappa, **outs)
            else:
                ops.token_topn(lg, lo, hi, B, 1.0, 0, 1.0, out_tok=cand_tok, out_logprob=cand_lp, out_entropy=ent)
                ops.beam_merge(cum[i], cand_tok, cand_lp, B, lo, **outs)
            if trace is not None:
                step = dict(parent=parent[i].clone(), token=token[i].clone(), cum=cum[i + 1].clone(),
                            cand_tok=cand_tok.clone(), cand_lp=cand_lp.clone())
                if keyed:
                    step.update(cand_g=cand_g.clone(), g=pert[i + 1].clone(), kappa=kappa.clone())
                trace.setdefault("beam", []).append(step)

        ops.copy_rows(x, self.h_sel, N, self.c["llm_dim"], last_row, None)
        head_merge(self.h_sel[:N], 0)
        for i in range(1, S):
            h = i & 1
            ops.embed_gather(self.embed, feed[i - 1], out=xd)
            # the child's slot of this parity takes tokens t < i - 1 of its parent's slot of the other parity (dead beam: no copy)
            torch.lt(parent[i - 1], 0, out=dead)
            torch.add(src_base[h], parent[i - 1], out=src)
            src.masked_fill_(dead, -1)
            ops.kv_gather_slots(k_tab, vt_tab, src, slots[h], i - 1, **region)
            g = self.llm.group(N, 1, pos_all[i - 1],
                               [dict(region=0, length=T0, slot_of_batch=self.zero_slots),
                                dict(region=1, length=Lt, len_of_batch=cand_len, slot_of_batch=prompt_of_cand),
                                dict(region=2, length=i, slot_of_batch=slots[h])], 2, write_slot=slots[h], write_t_off=i - 1, seg0_shared=True)
            self.llm.forward(xd, [g], final_norm=False)               # writes t = i - 1 itself
            head_merge(xd, i)
        ops.beam_backtrack(parent, token, step_lp, B, out_tokens=out_tokens, out_logprobs=out_lps)
        return out_tokens, out_lps, cum[S], (pert[S] if keyed else None), (kappa if keyed else None)

    # ---------------------------------------------------------------------------------------------- de-tokeniser
    def tokens_to_actions(self, tokens: np.ndarray) -> np.ndarray:
        """256-bin de-tokeniser (policy_wrapper.py:259-266 arithmetic): discretized = vocab - token, clip(d-1, 0, 254),
        bin centres of linspace(-1, 1, 256). Host numpy on N x 7 integers."""
        bins = np.linspace(-1, 1, self.c["n_bins"])
        centers = (bins[:-1] + bins[1:]) / 2.0
        d = self.c["tok_vocab"] - np.asarray(tokens)
        d = np.clip(d - 1, a_min=0, a_max=centers.shape[0] - 1)
        return centers[d]

    # ---------------------------------------------------------------------------------------------- proposal augmentation
    def bin_centers(self) -> torch.Tensor:
        """The de-tokeniser's bin centres as the device kernels take them: tokens_to_actions' float64 arithmetic cast to fp32 [n_bins - 1],
        built once per model."""
        if getattr(self, "_centers", None) is None:
            bins = np.linspace(-1, 1, self.c["n_bins"])
            self._centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=self.dev)
        return self._centers

    def augment(self, tokens: torch.Tensor, n_samples: int, n_augmented: int, normals: torch.Tensor, *, sigma=1.0, sd_floor=0.0):
        """Gaussian proposal augmentation of sampled chunks (ops.augment_tokens with this model's tok_vocab, bin centres and
        steps = n_gen // 7): tokens int64 [P * n_samples, n_gen] as sample returns them -> int64 [P * S, n_gen], S = n_samples +
        n_augmented; per prompt the n_samples policy rows verbatim, then n_augmented rows drawn from the diagonal Gaussian fitted to their
        de-tokenised translation / rotation values (clipped to the bins' range [-1, 1], re-tokenised to the nearest bin centre) with the
        gripper token of the samples' majority class; on a gripper tie the augmented rows take the class of sample 0. normals fp32
        [P, n_augmented, n_gen // 7, 6] on the device (host.augmentation_normals). Every token of the result is an action token whenever
        the sampled ones are; ops.tokens_to_histories, score_histories(group_size=S) and tokens_to_actions take it as they take sampled
        tokens. One launch; the policy is not run. Off by default: nothing calls this."""
        return ops.augment_tokens(tokens, n_samples, n_augmented, normals, self.bin_centers(), self.c["tok_vocab"], steps=self.n_gen // 7,
                                  sigma=sigma, sd_floor=sd_floor)

    def refine(self, tokens: torch.Tensor, scores: torch.Tensor, group_rows: int, n_elite: int, normals: torch.Tensor, *, sigma=1.0,
               sd_floor=0.0, elites=False):
        """Verifier-guided refinement of scored chunks, one round of the cross-entropy method (ops.refine_tokens with this model's
        tok_vocab, bin centres and steps = n_gen // 7): tokens int64 [P * group_rows, n_gen] (sampled, augmented or already refined) and
        their scores fp32 [P * group_rows] (score_histories' scores, robust or combined) -> int64 [P * (n_elite + n_new), n_gen],
        n_new = normals.shape[1]; per prompt the n_elite best-scored rows verbatim, best first (equal scores by ascending row, a NaN
        last), then n_new rows drawn as augment draws them from the Gaussian refitted on those elites; on a gripper tie they take the
        class of the best elite. normals fp32 [P, n_new, n_gen // 7, 6] on the device (host.augmentation_normals, a fresh seed per
        round). The result goes where augment's goes, with group_size = n_elite + n_new and n_fit = n_elite. elites=True ->
        (tokens, ops.RefineElites). One launch; the policy is not run. Off by default: nothing calls this."""
        if not torch.is_tensor(normals) or normals.dim() != 4:
            raise L.CoverError("OpenVLA.refine: normals must be an fp32 tensor [prompts, n_new, n_gen // 7, 6]")
        return ops.refine_tokens(tokens, scores, group_rows, n_elite, normals.shape[1], normals, self.bin_centers(), self.c["tok_vocab"],
                                 steps=self.n_gen // 7, sigma=sigma, sd_floor=sd_floor, elites=elites)

    def smooth_scores(self, tokens: torch.Tensor, scores: torch.Tensor, group_rows: int, smooth, *, stats=False):
        """Neighbourhood-smoothed scores of scored chunks (ops.smooth_scores_tokens with this model's tok_vocab, bin centres and
        steps = n_gen // 7): tokens int64 [P * group_rows, n_gen] (sampled, augmented or refined) and their scores fp32 [P * group_rows]
        (score_histories' scores or robust) -> fp32 [P * group_rows], every score replaced by the kernel-weighted mean of its prompt's
        scores over the rows' de-tokenised translation / rotation values, shrunk towards the prompt's mean score. smooth: a host.Smooth
        (radius, dim_scale, shrink, split_gripper; none has a default or a recommended value). The result goes where scores go:
        ops.group_argmax, ops.prior_select, refine. stats=True -> (smoothed, ops.SmoothStats). One launch; the policy is not run. Off by
        default: nothing calls this."""
        if not isinstance(smooth, host.Smooth):
            raise L.CoverError("OpenVLA.smooth_scores: smooth must be a host.Smooth")
        return ops.smooth_scores_tokens(tokens, scores, group_rows, self.bin_centers(), self.c["tok_vocab"], steps=self.n_gen // 7,
                                        stats=stats, **smooth.kwargs(tokens.device))

    def coherence_prior(self, tokens: torch.Tensor, group_rows: int, coherence, *, ref_tokens=None, ref_actions=None, ref_weight=None,
                        shift=0, stats=False):
        """The chunk-coherence prior of action-token chunks (ops.coherence_prior_tokens with this model's tok_vocab, bin centres and
        steps = n_gen // 7): tokens int64 [P * group_rows, n_gen] (sampled, augmented or refined) -> fp32 [P * group_rows], per row minus
        the weighted, step-decayed squared distance to the reference chunks. Exactly one of ref_tokens (int64 [R, 7 hr] or
        [P, R, 7 hr], de-tokenised here through bin_centers() with tokens_to_histories' clamp rule, in torch) and ref_actions (fp32
        [R, hr, 7] or [P, R, hr, 7], in the de-tokenised space) is given. ref_weight: fp32 [R] or [P, R], signed; None = all ones.
        shift: candidate step t meets reference step t + shift (the steps of the reference chunk already executed). coherence: a
        host.Coherence (dim_scale, decay, gripper_penalty; none has a default or a recommended value). One reference holding the last
        committed chunk, shift = the steps executed since, is the backward coherence; the group's own rows at +1/S with a weak policy's
        at -1/S' is the forward contrast. The result is a prior: ops.prior_select's, score_histories(prior=),
        verify_and_select(candidate_prior=). stats=True -> (prior, ops.CoherenceStats). One launch; the policy is not run. Off by
        default: nothing calls this."""
        if not isinstance(coherence, host.Coherence):
            raise L.CoverError("OpenVLA.coherence_prior: coherence must be a host.Coherence")
        if (ref_tokens is None) == (ref_actions is None):
            raise L.CoverError("OpenVLA.coherence_prior: exactly one of ref_tokens and ref_actions is required")
        steps = self.n_gen // 7
        if ref_tokens is not None:
            if not torch.is_tensor(ref_tokens) or ref_tokens.dtype != torch.int64 or ref_tokens.dim() not in (2, 3) or ref_tokens.shape[-1] % 7 != 0:
                raise L.CoverError("OpenVLA.coherence_prior: ref_tokens must be int64 [R, 7 hr] or [prompts, R, 7 hr]")
            cen = self.bin_centers()
            b = (self.c["tok_vocab"] - ref_tokens.to(cen.device) - 1).clamp(0, cen.numel() - 1)
            ref_actions = cen[b].reshape(*ref_tokens.shape[:-1], ref_tokens.shape[-1] // 7, 7).contiguous()
        if not torch.is_tensor(ref_actions) or ref_actions.dim() not in (3, 4):
            raise L.CoverError("OpenVLA.coherence_prior: ref_actions must be fp32 [R, hr, 7] or [prompts, R, hr, 7]")
        if ref_weight is None:
            ref_weight = torch.ones(ref_actions.shape[-3], dtype=torch.float32, device=ref_actions.device)
        return ops.coherence_prior_tokens(tokens, group_rows, ref_actions, ref_weight, self.bin_centers(), self.c["tok_vocab"], steps=steps,
                                          shift=shift, stats=stats, **coherence.kwargs(tokens.device, steps))

    def diverse_subset(self, tokens: torch.Tensor, group_rows: int, diversity, *, quality=None, steps=1):
        """A diverse subset of action-token chunks (ops.diverse_subset_tokens with this model's tok_vocab and bin centres): tokens int64
        [P * group_rows, >= 7 steps] (sampled, augmented or refined) -> ops.DiverseSubset with diversity.keep rows per prompt, picked
        greedily by quality + diversity.weight * (distance to the nearest row already picked); rows within diversity.cover_dist of a pick
        are left out (0: exact duplicates; negative: off). quality: fp32 [P * group_rows] or None -- before the verifier a policy
        log-probability or a prior, after it the scores (then .rows is the diverse shortlist). steps: the action steps a row holds, as
        tokens_to_histories' n_use; the distance runs over them. .rows goes to ops.tokens_to_histories / score_histories with
        group_size = keep; host.spread_scores takes the kept rows' scores back to the input rows. diversity: a host.Diversity (keep,
        weight, dim_scale, decay, gripper_penalty, cover_dist; none has a recommended value). One launch; the policy is not run. Off by
        default: nothing calls this."""
        if not isinstance(diversity, host.Diversity):
            raise L.CoverError("OpenVLA.diverse_subset: diversity must be a host.Diversity")
        return ops.diverse_subset_tokens(tokens, group_rows, diversity.keep, self.bin_centers(), self.c["tok_vocab"], steps=steps,
                                         quality=quality, **diversity.kwargs(tokens.device, steps))

    def proposal_prior(self, tokens: torch.Tensor, group_rows: int, n_fit: int, *, sigma, sd_floor, log_share=None):
        """The proposal log-density prior of action-token chunks (ops.proposal_prior_tokens with this model's tok_vocab, bin centres and
        steps = n_gen // 7): tokens int64 [P * group_rows, n_gen] -> fp32 [P * group_rows], per row the unnormalised log-density of the
        diagonal Gaussian fitted to the first n_fit rows of its prompt (the fit augment draws from) plus, with log_share
        (host.vote_log_shares on the device), the log share of the row's gripper class. After augment(tokens, n, K, ...) pass
        group_rows = n + K and n_fit = n; on sampled tokens alone group_rows = n_fit = n. The result is the [N] prior ops.prior_select
        and score_histories(prior=, prior_beta=) take with group_size = group_rows. sigma and sd_floor must be > 0; none is
        recommended. One launch; the policy is not run. Off by default: nothing calls this."""
        return ops.proposal_prior_tokens(tokens, group_rows, n_fit, self.bin_centers(), self.c["tok_vocab"], steps=self.n_gen // 7,
                                         sigma=sigma, sd_floor=sd_floor, log_share=log_share)
