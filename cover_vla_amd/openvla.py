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

from typing import Dict, Optional

import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .host import TopLogprobs
from .ops import RowParam
from .models import BF, Decoder, KvGeometry, VitTower, _f32

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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
        self._cap = None
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
            st = dict(frame=torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev),
                      d=self.dino.static_bufs(n, H, W), s=self.siglip.static_bufs(n, H, W),
                      fused=torch.empty(n * P, self.fused, dtype=BF, device=dev),
                      h=[torch.empty(n * P, lin.n_out, dtype=BF, device=dev) for lin in self.proj],
                      ws=[ops.gemm_workspace(n * P, lin.N, lin.K, dev) for lin in self.proj], graph=None)
            self._vis[key] = st
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
        gen = (self.dino.ws_gen, self.siglip.ws_gen)
        if st["graph"] is not None and st.get("ws_gen") != gen:
            st["graph"] = None                                           # a tower workspace moved (a larger frame batch ran since): re-capture
        if st["graph"] is not None and self.vision_graph:
            st["graph"].launch()
            return st["h"][2]
        out = self._encode_static(st)                                    # eager (also sizes the towers' workspaces)
        if self.vision_graph and st["graph"] is None:
            cur = torch.cuda.current_stream()
            if self._cap is None:
                self._cap = torch.cuda.Stream(device=self.dev)
            self._cap.wait_stream(cur)
            with torch.cuda.stream(self._cap):
                with ops.Graph() as g:
                    self._encode_static(st)
            st["graph"] = g
            st["ws_gen"] = (self.dino.ws_gen, self.siglip.ws_gen)
            cur.wait_stream(self._cap)
        return out

    # ---------------------------------------------------------------------------------------------- sampler
    def sample(self, frame_u8: torch.Tensor, prompt_tokens: torch.Tensor, prompt_lens: torch.Tensor, n_samples: int,
               uniforms: Optional[torch.Tensor] = None, temperature: RowParam = 1.0, trace: Optional[dict] = None,
               force_tokens: Optional[torch.Tensor] = None, on_prefill_enqueued=None, on_vision_enqueued=None,
               top_k: RowParam = 0, top_p: RowParam = 1.0, return_logprobs: bool = False, top_logprobs: int = 0,
               prior_temperature: Optional[float] = None):
        """frame_u8 [n_cams,H,W,3] uint8; prompt_tokens int64 [P, Lt] right padded, prompt_lens int32 [P] (device);
        n_samples candidates per prompt (N = P*n_samples, candidate i belongs to prompt i // n_samples);
        uniforms fp32 [N, n_gen] in [0,1) for inverse-CDF sampling over the 256 action tokens, None = greedy over the
        tokenizer vocabulary; top_k / top_p filter the sampled distribution after the temperature, in the order and with the
        meaning of Hugging Face's `generate(do_sample=True, top_k, top_p)` (ops.token_sample; 0 / 1.0 = off, the unfiltered
        ops.token_select path; greedy ignores them). force_tokens int64 [N, n_gen] (tests): teacher-force the fed-back tokens while still
        returning this path's own picks. on_prefill_enqueued: optional callable invoked once the prefill launches are
        queued -- the point where a caller should queue independent side-stream work (the verifier towers): the
        HBM-bound decode passes that follow tolerate concurrent kernels, the MFMA-bound prefill does not. Returns (tokens int64 [N, n_gen], selected-logit fp32 [N, n_gen]).
        return_logprobs: a third tensor fp32 [N, n_gen], the log-probability of each pick under the distribution it was drawn from
        (sampled: temperature, top_k, top_p over the action bins, cover_token_sample_scored / cover_token_logprob; greedy: temperature 1,
        no filters, over the tokenizer vocabulary the arg-max runs over). With force_tokens it is still this path's own picks that are
        scored. The default launches exactly what it launched without the argument.
        top_logprobs = n in 1..64: appends host.TopLogprobs(tokens int64 [N, n_gen, n], logprobs fp32 [N, n_gen, n], entropy fp32
        [N, n_gen]) to the return: per step the n most probable tokens of the distribution return_logprobs documents (descending logit,
        equal logits by ascending id; -1 / -inf where it keeps fewer than n), their log-probabilities (cover_token_logprob's, bit for
        bit) and its entropy in nats -- one ops.token_topn launch per step on the logits the pick used. 0: today's launches.
        Parameters per candidate: temperature, top_k and top_p each accept a scalar or a length-N sequence / tensor (host.sampling_ladder
        builds them). All scalars is the path above, untouched. As soon as one of the three is per candidate, all three are validated on
        the host (temperature >= 0, top_k >= 0, top_p > 0, all finite, else CoverError; a device tensor of any numeric dtype is read back
        once for it, so no pick is ever the -1 of an invalid row), broadcast to fp32 / int32 / fp32 [N] device tensors and every step's pick is ONE ops.token_sample_rows launch (ops.pick_token(row_params=)); uniforms is then
        required, return_logprobs is that launch's log-probability and top_logprobs is ops.token_topn_rows. In this mode EVERY row picks
        over the action bins [action_lo, action_hi), the launch's range: a candidate with temperature 0 is greedy and takes the arg-max
        over the 256 action bins (its log-probability: temperature 1, unfiltered, over those bins), whereas an all-greedy call
        (uniforms=None) keeps its arg-max over the tokenizer vocabulary. The decode graph is keyed on the fact "per-row parameters", not
        on their values: the three tensors are static buffers filled before each replay, so a new ladder is not a new capture.
        prior_temperature = T_ref (> 0, finite): the return gains a fp32 [N, n_gen] tensor (after the return_logprobs tensor if that is
        present, before TopLogprobs): the log-probability of each pick under ONE reference distribution for every candidate -- temperature
        T_ref, unfiltered, over the action bins -- written by the pick's own launch (cover_token_sample_rows_ref; ops.token_logprob_rows at
        (T_ref, 0, 1) on the pick, bit for bit). It is the prior that compares across the rungs of a ladder: return_logprobs scores every
        candidate under its own rung. Scalar parameters are broadcast and the per-row path is taken (the only one that carries the
        reference); uniforms is required: a greedy candidate is a row with temperature 0. The decode graph's key carries the value of
        T_ref, which travels by value in the launch. None launches exactly what it launched before."""
        c, dev = self.c, self.dev
        n_top = int(top_logprobs)
        if not 0 <= n_top <= 64:
            raise ValueError("top_logprobs must be in 0..64")
        t_ref = None
        if prior_temperature is not None:
            t_ref = ops.ref_temperature_value("sample: prior_temperature", prior_temperature)
            if uniforms is None:
                raise ValueError("prior_temperature needs uniforms: the reference score comes from the per-row sampler, in which a greedy "
                                 "candidate is a row with temperature=0 (pass uniforms and temperature=0 rows instead of uniforms=None)")
        P, Lt = prompt_tokens.shape
        N = P * n_samples

        def mark(name):   # optional phase timing (tools/phases.py): trace["events"] collects (name, event) pairs
            if trace is not None and "events" in trace:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                trace["events"].append((name, ev))

        if P > self.max_prompts or N > self.max_candidates or Lt > self.max_text:
            raise ValueError("prompts/candidates/text length exceed the sizes this model was built for")
        D, T0 = c["llm_dim"], self.T0
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
        # ---- first action token: last valid text position of each candidate's prompt
        prompt_of_cand = (torch.arange(N, device=dev) // n_samples).to(torch.int32)
        cand_len = prompt_lens.to(torch.int32)[prompt_of_cand.long()].contiguous()
        last_row = (Tp + prompt_of_cand * Lt + cand_len - 1).to(torch.int32)
        pos_all = ((T0 + cand_len)[None, :] + torch.arange(self.n_gen, dtype=torch.int32, device=dev)[:, None]).contiguous()
        u_t = None if uniforms is None else uniforms.to(torch.float32).t().contiguous()
        rp = None
        if t_ref is not None or any(ops.is_per_row(v) for v in (temperature, top_k, top_p)):
            if uniforms is None:
                raise ValueError("per-candidate temperature / top_k / top_p need uniforms (a greedy candidate is a temperature of 0)")
            rp = ops.row_param_tensors(N, temperature, top_k, top_p, dev)
            temperature, filt = None, None
        else:
            filt = None if uniforms is None or (top_k <= 0 and top_p >= 1.0) else (int(top_k), float(top_p))
        if self.decode_graph and trace is None and force_tokens is None and not self.slice_action_head:
            # static buffers per batch shape; the per-decision values (prompt lengths -> rows / positions, uniforms) are copied in
            # per-row parameters: the key carries the fact, the values live in static buffers (st["rp"]) like the uniforms
            key = (P, n_samples, Lt, uniforms is None, "rows" if rp is not None else float(temperature), self.slice_action_head, filt) + ((True,) if return_logprobs else ()) + ((("top", n_top),) if n_top else ()) + ((("prior", t_ref),) if t_ref is not None else ())
            st = self._dec.get(key)
            if st is None:
                st = dict(graph=None, prompt_of_cand=prompt_of_cand.clone(), cand_len=torch.empty_like(cand_len), last_row=torch.empty_like(last_row),
                          pos_all=torch.empty_like(pos_all), tokens=torch.empty(self.n_gen, N, dtype=torch.int64, device=dev),
                          sel=torch.empty(self.n_gen, N, dtype=torch.float32, device=dev),
                          u=None if u_t is None else torch.empty_like(u_t),
                          lps=torch.empty(self.n_gen, N, dtype=torch.float32, device=dev) if return_logprobs else None,
                          prior=torch.empty(self.n_gen, N, dtype=torch.float32, device=dev) if t_ref is not None else None,
                          top=self._top_bufs(N, n_top), rp=None if rp is None else tuple(torch.empty_like(t) for t in rp),
                          prompt_slots=torch.arange(P, dtype=torch.int32, device=dev), prompt_lens=torch.empty(P, dtype=torch.int32, device=dev))
                self._dec[key] = st
            st["cand_len"].copy_(cand_len); st["last_row"].copy_(last_row); st["pos_all"].copy_(pos_all)
            st["prompt_lens"].copy_(prompt_lens.to(torch.int32))
            if u_t is not None:
                st["u"].copy_(u_t)
            if rp is not None:
                for dst, src in zip(st["rp"], rp):
                    dst.copy_(src)
            body = lambda: self._decode_body(x, N, n_samples, Lt, st["prompt_of_cand"], st["cand_len"], st["last_row"], st["pos_all"], st["u"], temperature,
                                             st["tokens"], st["sel"], st["tokens"], None, st["prompt_slots"], st["prompt_lens"], filt=filt, lps=st["lps"], top=st["top"], rp=st["rp"],
                                             prior=None if t_ref is None else (t_ref, st["prior"]))
            if st["graph"] is not None and st.get("ws_gen") != self.llm.ws_gen:
                st["graph"] = None                                      # the decoder workspace moved under the captured pointer: re-capture
            if st["graph"] is None:
                body()                                                  # eager once (also sizes every workspace), then recorded
                cur = torch.cuda.current_stream()
                if self._cap is None:
                    self._cap = torch.cuda.Stream(device=self.dev)
                self._cap.wait_stream(cur)
                with torch.cuda.stream(self._cap):
                    with ops.Graph() as g:
                        body()
                st["graph"] = g
                st["ws_gen"] = self.llm.ws_gen
                cur.wait_stream(self._cap)
            else:
                st["graph"].launch()
            # the eager pass before a capture has filled the same buffers
            return self._sample_result(st["tokens"], st["sel"], st["lps"], st["top"], st["prior"])
        # step-major buffers: row i of each is contiguous, so the kernels of step i read / write them in place (no per-step slice copies)
        tokens = torch.empty(self.n_gen, N, dtype=torch.int64, device=dev)
        sel = torch.empty(self.n_gen, N, dtype=torch.float32, device=dev)
        lps = torch.empty(self.n_gen, N, dtype=torch.float32, device=dev) if return_logprobs else None
        top = self._top_bufs(N, n_top)
        prior = torch.empty(self.n_gen, N, dtype=torch.float32, device=dev) if t_ref is not None else None
        fed = tokens if force_tokens is None else force_tokens.t().contiguous()
        self._decode_body(x, N, n_samples, Lt, prompt_of_cand, cand_len, last_row, pos_all, u_t, temperature, tokens, sel, fed, trace,
                          torch.arange(P, dtype=torch.int32, device=dev), prompt_lens.to(torch.int32).contiguous(), mark, filt=filt, lps=lps, top=top, rp=rp,
                          prior=None if t_ref is None else (t_ref, prior))
        return self._sample_result(tokens, sel, lps, top, prior)

    def _top_bufs(self, N, n_top):
        """Step-major buffers of sample(top_logprobs=n): (tokens [n_gen, N, n], logprobs [n_gen, N, n], entropy [n_gen, N]), None for n = 0."""
        if not n_top:
            return None
        return (torch.empty(self.n_gen, N, n_top, dtype=torch.int64, device=self.dev),
                torch.empty(self.n_gen, N, n_top, dtype=torch.float32, device=self.dev),
                torch.empty(self.n_gen, N, dtype=torch.float32, device=self.dev))

    @staticmethod
    def _sample_result(tokens, sel, lps, top, prior=None):
        """Candidate-major copies of the step-major buffers: what sample returns."""
        out = (tokens.t().contiguous(), sel.t().contiguous())
        if lps is not None:
            out += (lps.t().contiguous(),)
        if prior is not None:
            out += (prior.t().contiguous(),)
        if top is not None:
            out += (TopLogprobs(top[0].transpose(0, 1).contiguous(), top[1].transpose(0, 1).contiguous(), top[2].t().contiguous()),)
        return out

    def _decode_body(self, x, N, n_samples, Lt, prompt_of_cand, cand_len, last_row, pos_all, uniforms, temperature, tokens, sel, fed, trace,
                     prompt_slots, prompt_lens_i32, mark=lambda name: None, filt=None, lps=None, top=None, rp=None, prior=None):
        """Head on the last prompt rows, then n_gen - 1 decode passes + heads. Launches only (no allocation, no host read): recordable."""
        D, T0 = self.c["llm_dim"], self.T0
        ops.copy_rows(x, self.h_sel, N, D, last_row, None)
        self._head_select(self.h_sel[:N], uniforms, 0, temperature, tokens, sel, trace, filt, lps, top, rp, prior)
        xd = self.x_dec[:N]
        own = {}
        if self.own_kv is not None:   # regular structure of the batch: the n_samples candidates of prompt p are rows [p S, (p + 1) S)
            own = dict(own_kv=self.own_kv, seg1_group=n_samples, seg1_slot_of_group=prompt_slots, seg1_len_of_group=prompt_lens_i32)
        for i in range(1, self.n_gen):
            ops.embed_gather(self.embed, fed[i - 1], out=xd)
            g = self.llm.group(N, 1, pos_all[i - 1],
                               [dict(region=0, length=T0, slot_of_batch=self.zero_slots),
                                dict(region=1, length=Lt, len_of_batch=cand_len, slot_of_batch=prompt_of_cand),
                                dict(region=2, length=i)], 2, write_t_off=i - 1, seg0_shared=True, **own)
            self.llm.forward(xd, [g], final_norm=False)
            self._head_select(xd, uniforms, i, temperature, tokens, sel, trace, filt, lps, top, rp, prior)
            mark(f"decode{i}")

    def _head_select(self, h, uniforms, i, temperature, tokens, sel, trace, filt=None, lps=None, top=None, rp=None, prior=None):
        """Norm, head GEMM, one ops.pick_token. filt: None = the unfiltered ops.token_select pick; (top_k, top_p) = ops.token_sample over
        the same columns. lps fp32 [n_gen, N] or None: row i receives the log-probability of step i's picks.
        top (tokens, logprobs, entropy) or None: slab i receives ops.token_topn of the distribution the pick came from.
        rp (temperature, top_k, top_p) device tensors [N] or None: the pick is ops.token_sample_rows, the top-n ops.token_topn_rows.
        prior (T_ref, fp32 [n_gen, N]) or None (rp is then set): row i receives the picks' log-probability at temperature T_ref, unfiltered."""
        N = h.shape[0]
        u = None if uniforms is None else uniforms[i]
        # out_kept: written by the filtered pick (ops.token_sample) only
        out = dict(out_logit=sel[i], out_kept=self.kept_sel[:N], out_logprob=None if lps is None else lps[i])
        if rp is not None:
            out["row_params"] = rp
        if prior is not None:
            out["ref"] = (prior[0], prior[1][i])
        hn = ops.rmsnorm(h, self.llm.final_norm, 1e-5, w_offset=0.0, style=1, out=self.hn[:N])
        if uniforms is not None and (trace is None or "events" in trace) and self.slice_action_head:
            lg = ops.gemm(hn, self.lm_head_actions, out=self.logits_actions[:N], ws=self.head_ws_actions)
            t, _, _ = ops.pick_token(lg, 0, self.c["n_bins"], u, temperature, filt, **out)
            torch.add(t, self.action_lo, out=tokens[i])
            if top is not None:
                self._head_topn(lg, 0, self.c["n_bins"], uniforms is None, temperature, filt, top, i, rp)
                top[0][i].add_((top[0][i] >= 0) * self.action_lo)          # ids as the tokens are; the -1 padding stays
            return
        lg = ops.gemm(hn, self.lm_head, out=self.logits[:N], ws=self.head_ws)
        if trace is not None and "events" not in trace:
            trace.setdefault("logits", []).append(lg.clone())
        lo, hi = (0, self.c["tok_vocab"]) if uniforms is None else (self.action_lo, self.action_hi)   # greedy: the tokenizer vocabulary
        ops.pick_token(lg, lo, hi, u, temperature, filt, out_tok=tokens[i], **out)
        if top is not None:
            self._head_topn(lg, lo, hi, uniforms is None, temperature, filt, top, i, rp)

    @staticmethod
    def _head_topn(lg, lo, hi, greedy, temperature, filt, top, i, rp=None):
        """One ops.token_topn launch on step i's logits; greedy: temperature 1, unfiltered (what return_logprobs scores a greedy pick under).
        rp: ops.token_topn_rows with the parameters of every row its own."""
        if rp is not None:
            ops.token_topn_rows(lg, lo, hi, top[0].shape[2], rp[0], rp[1], rp[2], out_tok=top[0][i], out_logprob=top[1][i], out_entropy=top[2][i])
            return
        k, p = (0, 1.0) if greedy or filt is None else filt
        ops.token_topn(lg, lo, hi, top[0].shape[2], 1.0 if greedy else temperature, k, p, out_tok=top[0][i], out_logprob=top[1][i],
                       out_entropy=top[2][i])

    # ---------------------------------------------------------------------------------------------- de-tokeniser
    def tokens_to_actions(self, tokens: np.ndarray) -> np.ndarray:
        """256-bin de-tokeniser (policy_wrapper.py:259-266 arithmetic): discretized = vocab - token, clip(d-1, 0, 254),
        bin centres of linspace(-1, 1, 256). Host numpy on N x 7 integers."""
        bins = np.linspace(-1, 1, self.c["n_bins"])
        centers = (bins[:-1] + bins[1:]) / 2.0
        d = self.c["tok_vocab"] - np.asarray(tokens)
        d = np.clip(d - 1, a_min=0, a_max=centers.shape[0] - 1)
        return centers[d]
