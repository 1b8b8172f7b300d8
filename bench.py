#!/usr/bin/env python3
"""bench.py — candidates sampled AND scored per second, OpenVLA-7B shapes, 224^2 RGB, on MI355X.

One step = one DECISION of the hot path on one observation:
    frame -> DINOv2-L + SigLIP-So400m + projector -> Llama-2-7B prefill (shared image prefix + 8 prompts) ->
    6 decode passes (7 action tokens for each of N=32 candidates = 8 prompts x 4 samples) -> de-tokenise ->
    CoVer verifier (SigLIP2-L/16-384 image+text towers, 3-member head ensemble, trajectory encoder per candidate) ->
    grouped arg-max.
Weights are synthetic (seeded N(0,0.02), random-init of the named architectures: there is no network for
checkpoints), inputs synthetic and resident in HBM before the timed region.

Multi-GPU (one process per GPU, RCCL; candidates are independent given the observation, so the path shards by prompt group
with ONE all-gather of [score | tokens] records and the same grouped arg-max on every rank):
  --scaling weak   (default) per-GPU work fixed at the headline's: ONE observation with 8 x W DISTINCT rephrased prompts x 4
                   samples, N = 32 x W candidates with their own uniforms; rank r owns prompt groups r, r + W, ...
                   (batch construction: run_simpler_eval_with_openpi.py:296-319 -- `lang_rephrase_num` prompts, each repeated
                   `policy_batch_inference_size` times). value = all ranks' candidates / max-over-ranks time. At W = 1 this is
                   exactly the headline line.
  --config 3       BASELINE config 3 as SURVEY 8(d) defines it: W prompt groups of 32 samples, rank r owns group r (N = 256 at 8 GPUs).
  --scaling strong the headline N = 32 itself sharded: rank r takes prompts r, r+W, ... (8/W prompts x 4 samples). Every rank
                   still streams all the decoder weights per decode pass (M = 32/W rows), so the expected gain is small.

Prints ONE JSON line (rank 0). A plain run sets up, warms up, times --steps decisions and prints the line (metric, value, unit,
higher_is_better, dtype, ms_per_step = milliseconds of one timed decision, config); --dump-outputs DIR also writes what the last timed
decision returned as DIR/<name>.npy (float32 / float64; the inputs and weights are seeded, so two builds compare output for output).
Everything else runs only with --full, which adds these objects (and, with --dtype fp8, "fp8_vs_bf16"):
  "roofline"       dominant kernel = the weight-streaming GEMM of the decode passes (HBM-bound), timed live per launch
                   with the kernels' own start/stop stamps (hipExtLaunchKernelGGL event pairs on their stream);
  "roofline_mfma"  every LDS-tiled MFMA GEMM of the decision (LLM prefill + all ViT towers + projector):
                   sum 2MNK / (their kernel time + their split-K reductions) against the dense bf16 peak;
  "end_to_end"     (HBM floor + MFMA floor) / measured step time;
  "cpu_baseline"   the CPU oracle executing FULL candidates (all 32 layers, every tower block) on the host cores: one cold run
                   (config 1, N = 1 greedy) + the median of 3 timed candidates, the de-duplicated variant composed beside it.
The profiled decision runs single-threaded on one stream without hipGraph replay, so that kernels neither overlap
(inflated durations) nor hide from the timer; any roofline fraction > 1 is refused (the timer did not time the work).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_PROMPTS, N_SAMPLES, LT = 8, 4, 24
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_PEAK_TF = 2500.0      # bf16 dense
FP8_PEAK_TF = 5000.0       # MX-scaled fp8 dense (MI355X_MICROARCH.md chip table; measured 4.65 PF)
SIDE_GRAPH_DEFAULT = "2"   # verifier towers: "0" eager launches from a second host thread, "1" one hipGraph launched by the main thread, "2" by the second thread
N_PROF = 10                # include/cover_hip.h COVER_PROF_CLASSES: 6 / 8 / 9 = the split-K reductions behind the ViT-sized / LLM-sized / fp8 tiled GEMMs
BASE_METRIC = "candidate actions scored/sec (whole node), OpenVLA-7B N=32, 224^2 RGB"


def build_inputs(dev, cfg, n_prompts, n_samples, n_cams=1, seed=0, n_gen=7):
    """All ranks build the SAME global inputs (one observation, n_prompts rephrases). Prompt p and the uniforms of candidate n are
    functions of (seed, p) / (7, n) alone -- not of how many prompts there are -- so the first 8 prompts of a W-rank weak-scaling run
    are the headline's prompts and every rank slices its own rows out of identical global tensors."""
    g = torch.Generator().manual_seed(seed)
    frame = torch.randint(0, 256, (n_cams, cfg["image"], cfg["image"], 3), generator=g, dtype=torch.uint8)
    img384 = torch.randn(1, 3, 384, 384, generator=g)
    text = torch.randint(0, 32000, (1, 64), generator=g)
    past = torch.randn(6, 7, generator=g) * 0.02
    past[:, 6] = (torch.rand(6, generator=g) > 0.5).float()
    lens = torch.tensor([16 + (i % 8) for i in range(n_prompts)], dtype=torch.int32)
    toks = torch.zeros(n_prompts, LT, dtype=torch.long)
    for p in range(n_prompts):
        gp = torch.Generator().manual_seed(1000 * (seed + 1) + p)
        toks[p, : lens[p]] = torch.randint(3, cfg["tok_vocab"] - cfg["n_bins"], (int(lens[p]),), generator=gp)
    u = torch.rand(n_prompts * n_samples, n_gen, generator=torch.Generator().manual_seed(7))   # row-major: row n is the same for any total
    return dict(frame=frame.to(dev), toks=toks.to(dev), lens=lens.to(dev), u=u.to(dev), img384=img384.to(dev), text=text.to(dev),
                past=past.double().numpy())


class Pipeline:
    def __init__(self, dev, small=False, n_prompts=N_PROMPTS, n_samples=N_SAMPLES, n_cams=1, members=3, prompt_ids=None,
                 weight_dtype="bf16", horizon=1, own_kv="auto", peaked=True):
        """prompt_ids: the global prompt indices this rank owns (strong scaling); None = all n_prompts.
        peaked: the synthetic checkpoint with decision margins (synth.openvla_state(peaked=True): depth-scaled residual projections, unit-scale
        embeddings, log-normal gains on the action rows of the head) -- same shapes, same bytes, same launches as the flat i.i.d. one."""
        from cover_vla_amd import synth
        from cover_vla_amd.openvla import OpenVLA
        from cover_vla_amd.verifier import EfficientEnsembleMerged, SigLIP2Encoder
        self.dev = dev
        c = dict(synth.OPENVLA_SMALL if small else synth.OPENVLA_7B)
        sc = dict(synth.SIGLIP2_SMALL if small else synth.SIGLIP2_L)
        self.c, self.sc = c, sc
        self.n_prompts_global, self.n_samples, self.n_cams = n_prompts, n_samples, n_cams
        self.prompt_ids = list(range(n_prompts)) if prompt_ids is None else list(prompt_ids)
        P = len(self.prompt_ids)
        wd = torch.bfloat16
        sd = synth.openvla_state(c, seed=1234, nontrivial=False, device=dev, wdtype=wd, peaked=peaked)
        self.peaked = peaked
        self.horizon, self.weight_dtype = horizon, weight_dtype
        if own_kv == "auto":   # more decode rows than the 16-candidate fused kernel is built for (config 5): head-major own-token cache,
            own_kv = (("fp8" if weight_dtype == "fp8" else "bf16") if P * n_samples > 64 else None)   # e4m3 in the fp8 profile (fp8 KV)
        self.own_kv = own_kv
        self.policy = OpenVLA(sd, c, device=str(dev), max_prompts=P, max_candidates=P * n_samples, max_text=LT, n_cams=n_cams,
                              horizon=horizon, weight_dtype=weight_dtype, own_kv=own_kv)
        del sd
        ssd = synth.siglip2_state(sc, seed=4321, nontrivial=False, device=dev, wdtype=wd)
        if small:
            self.enc = SigLIP2Encoder(ssd, dim=sc["dim"], layers=sc["layers"], heads=sc["heads"], mlp=sc["mlp"], patch=sc["patch"],
                                      image=sc["image"], context_length=sc["context_length"], device=str(dev))
        else:
            self.enc = SigLIP2Encoder(ssd, device=str(dev))
        del ssd
        torch.cuda.empty_cache()
        ck = synth.verifier_checkpoint(members, seed=1234, num_patches=self.enc.num_patches, vision_dim=sc["dim"], text_dim=sc["dim"])
        self.ver = EfficientEnsembleMerged(ck, device=str(dev), encoder=self.enc)
        g = build_inputs(dev, c, n_prompts, n_samples, n_cams, n_gen=7 * horizon)
        ids = torch.tensor(self.prompt_ids, device=dev)
        cand = (ids[:, None] * n_samples + torch.arange(n_samples, device=dev)[None]).reshape(-1)
        self.inp = dict(g, toks=g["toks"][ids].contiguous(), lens=g["lens"][ids].contiguous(), u=g["u"][cand].contiguous())
        self.side = None
        self.pool = None
        bins = np.linspace(-1, 1, c["n_bins"])
        self.centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=dev)   # float64 -> fp32 table
        self.past_dev = torch.tensor(self.inp["past"], dtype=torch.float32, device=dev)
        if small:
            g = torch.Generator().manual_seed(1)
            self.inp["img384"] = torch.randn(1, 3, sc["image"], sc["image"], generator=g).to(dev)
            self.inp["text"] = torch.randint(0, sc["vocab"], (1, sc["context_length"]), generator=g).to(dev)

    def decision(self, world=1, rank=0, cpu_gather=False, serial=False):
        """One decision. Returns (global winner index, local tokens, selection dict | None)."""
        i = self.inp
        S = self.n_samples
        # The verifier's frozen towers and image-text heads depend only on the observation and the instruction: they run on
        # a side stream while the policy samples. Who queues them matters as much as where they run: queued by this
        # thread before the policy they cost ~2.6 ms of host launch time with the main stream idle; queued from the
        # sampler's after-prefill hook they run underneath the decode passes, whose one-block-per-CU weight-streaming
        # grids lose ~1.4 ms to the co-tenants. A second host thread queues them from t = 0 instead (ctypes releases
        # the GIL inside the library's composites): they overlap the launch-bound vision phase and the start of the
        # prefill, and the decode passes run alone (42.2 -> 41.8 ms). COVER_SIDE_THREAD=0 selects the hook.
        # serial=True (the profiled decision): everything on the main stream from this thread, no hipGraph replay.
        main = torch.cuda.current_stream()
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.dev)
        out = {}

        def side_work():
            pf, tf = self.ver.extract_shared_features(i["img384"], i["text"])
            return self.ver.image_text_embeddings(pf, tf)

        if serial:
            keep = (self.policy.vision_graph, self.policy.vision_overlap, self.policy.decode_graph)
            self.policy.vision_graph, self.policy.vision_overlap, self.policy.decode_graph = False, False, False
            try:
                its = side_work()
                tokens, _ = self.policy.sample(i["frame"], i["toks"], i["lens"], S, i["u"], 1.0)
            finally:
                self.policy.vision_graph, self.policy.vision_overlap, self.policy.decode_graph = keep
        elif os.environ.get("COVER_SIDE_GRAPH", SIDE_GRAPH_DEFAULT) == "1":
            # round 6 experiment: the verifier's two towers + image-text heads as ONE replayed hipGraph (image tower and text tower as parallel
            # branches) launched on the side stream by THIS thread before the policy. Measured SLOWER (35.1-35.3 vs 34.45 ms): launching a
            # ~600-node graph costs this thread 1.6 ms before the policy's first launch (profiles/r06_side_graph_ab.txt). "2" = the same graph
            # launched by the second host thread (below).
            ev = torch.cuda.Event()
            ev.record(main)
            self.side.wait_event(ev)
            with torch.cuda.stream(self.side):
                its = self.ver.shared_embeddings_graph(i["img384"], i["text"])
            tokens, _ = self.policy.sample(i["frame"], i["toks"], i["lens"], S, i["u"], 1.0)
        elif os.environ.get("COVER_SIDE_THREAD", "1") != "0":
            if self.pool is None:
                import concurrent.futures
                self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
            ev = torch.cuda.Event()
            ev.record(main)
            after_vision = os.environ.get("COVER_SIDE_AFTER_VISION", "0") == "1"   # experiment: towers under the prefill instead of the vision phase
            import threading
            gate = threading.Event()

            def threaded():
                torch.cuda.set_device(self.dev)
                if after_vision:
                    gate.wait()
                self.side.wait_event(ev)
                with torch.cuda.stream(self.side):
                    if os.environ.get("COVER_SIDE_GRAPH", SIDE_GRAPH_DEFAULT) == "2":
                        return self.ver.shared_embeddings_graph(i["img384"], i["text"])
                    return side_work()

            def vision_hook():
                ev.record(main)
                gate.set()

            fut = self.pool.submit(threaded)
            tokens, _ = self.policy.sample(i["frame"], i["toks"], i["lens"], S, i["u"], 1.0, on_vision_enqueued=vision_hook if after_vision else None)
            its = fut.result()
        else:
            def hook():
                ev = torch.cuda.Event()
                ev.record(main)
                self.side.wait_event(ev)
                with torch.cuda.stream(self.side):
                    out["its"] = side_work()

            tokens, _ = self.policy.sample(i["frame"], i["toks"], i["lens"], S, i["u"], 1.0, on_prefill_enqueued=hook)
            its = out["its"]
        # de-tokenise + assemble the verifier histories on the device: no host sync between sampler and verifier
        from cover_vla_amd import ops
        hb, pad = ops.tokens_to_histories(tokens, self.c["tok_vocab"], self.centers, self.past_dev, n_use=min(self.horizon, 4))
        if not serial:
            main.wait_stream(self.side)
        r = self.ver.score_histories(its, hb, S, pad=pad)
        self.last_scores = r["scores"]
        if world > 1:
            # ONE collective: all-gather of [score | 7 tokens] records (RCCL over xGMI; gloo only in plumbing tests), then the
            # same deterministic grouped arg-max on every rank, which thereby also holds the winner's tokens and its prompt
            # group's tokens (cover_vla_amd/sharding.py)
            from cover_vla_amd.sharding import gather_records_and_select
            sc = r["scores"].cpu() if cpu_gather else r["scores"]
            tk = tokens.cpu() if cpu_gather else tokens
            sel = gather_records_and_select(sc, S, rank, world, n_prompts_total=self.n_prompts_global, local_payload=tk)
            return sel["global_idx"], tokens, sel
        return int(r["result"][0]), tokens, None


class Pi0Pipeline:
    """Profile P1 -- what the reference ships and evaluates: pi0 = SigLIP-So400m + PaliGemma-3B prefix + 300 M
    action expert, 10 Euler steps, chunk 4; B = 40 candidates = 8 rephrased prompts x 5 samples on ONE 224^2 observation
    (run_simpler_eval_with_openpi.py:296-319), then the CoVer verifier (SigLIP2-L/16-384 + 3-member ensemble) on the 40 chunks and
    the grouped arg-max. Batch construction as the reference's harness shapes it (lerobot_custom/.../pi0/conversion_scripts/
    benchmark.py:52-77 times select_action on such a batch); tokenizer max_length 72 (prompts of 16..23 real tokens, right padded)."""

    def __init__(self, dev, B=40, P=8, L=72, members=3, max_prompts=None, seed=1234):
        from cover_vla_amd import host, synth
        from cover_vla_amd.pi0 import PI0FlowMatching
        from cover_vla_amd.verifier import EfficientEnsembleMerged, SigLIP2Encoder
        self.dev, self.B, self.P, self.L, self.S = dev, B, P, L, B // P
        self.c = dict(synth.PI0_FULL)
        sd = synth.pi0_state(self.c, seed=seed, nontrivial=False, std=0.02, device=dev, wdtype=torch.bfloat16)
        self.model = PI0FlowMatching(sd, self.c, device=str(dev), max_batch=B, max_prompts=max_prompts or P, max_lang=L)
        del sd
        torch.cuda.empty_cache()
        self.sc = dict(synth.SIGLIP2_L)
        ssd = synth.siglip2_state(self.sc, seed=4321, nontrivial=False, device=dev, wdtype=torch.bfloat16)
        self.enc = SigLIP2Encoder(ssd, device=str(dev))
        del ssd
        torch.cuda.empty_cache()
        self.ver = EfficientEnsembleMerged(synth.verifier_checkpoint(members, seed=1234), device=str(dev), encoder=self.enc)
        gen = torch.Generator().manual_seed(0)
        img = (torch.rand(1, 3, 224, 224, generator=gen) * 2 - 1).repeat(B, 1, 1, 1)
        toks, masks = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.bool)
        for p in range(P):
            n = 16 + (p % 8)
            row = torch.randint(1, 257000, (n,), generator=gen)
            toks[p * self.S:(p + 1) * self.S, :n] = row
            masks[p * self.S:(p + 1) * self.S, :n] = True
        state = torch.zeros(B, 32)
        state[:, :7] = torch.rand(1, 7, generator=gen) * 2 - 1
        noise = torch.randn(B, self.c["chunk"], 32, generator=gen)
        img384 = torch.randn(1, 3, 384, 384, generator=gen)
        text = torch.randint(0, 32000, (1, 64), generator=gen)
        past = (torch.randn(6, 7, generator=gen) * 0.02).double().numpy()
        self.inp = dict(img=img.to(dev), toks=toks.to(dev), masks=masks.to(dev), state=state.to(dev), noise=noise.to(dev),
                        img384=img384.to(dev), text=text.to(dev), past=past)
        st = host.bridge_statistics()["action"]
        self.lo_hi = torch.tensor(list(st["p01"][:6]) + list(st["p99"][:6]), dtype=torch.float32, device=dev)
        self.past_dev = torch.tensor(past, dtype=torch.float32, device=dev)
        self.all_valid = torch.ones(B, dtype=torch.bool, device=dev)
        self.side, self.pool = None, None

    def _side_work(self):
        pf, tf = self.ver.extract_shared_features(self.inp["img384"], self.inp["text"])
        return self.ver.image_text_embeddings(pf, tf)

    def decision(self, serial=False, on_phase=None, noise=None):
        """One decision -> (winner index, actions [B, chunk, 32]). serial: everything on the main stream from this thread (the profiled
        decision); on_phase(name) is then called after the verifier towers, after the prefix pass and after the Euler loop."""
        from cover_vla_amd import ops
        i = self.inp
        main = torch.cuda.current_stream()
        if self.side is None:
            self.side = torch.cuda.Stream(device=self.dev)
        noise = i["noise"] if noise is None else noise
        if serial:
            its = self._side_work()
            if on_phase:
                on_phase("verifier_towers")
            keep = (self.model.n_chains, self.model.denoise_graph)
            self.model.n_chains, self.model.denoise_graph = 1, False     # ONE eager chain: launches replayed from a graph carry no timers
            try:
                x = self.model.sample_actions([i["img"]], [self.all_valid], i["toks"], i["masks"], i["state"], noise=noise,
                                              on_prefix_enqueued=(lambda: on_phase("prefix")) if on_phase else None)
            finally:
                self.model.n_chains, self.model.denoise_graph = keep
            if on_phase:
                on_phase("denoise")
        else:
            if self.pool is None:
                import concurrent.futures
                self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
            ev = torch.cuda.Event()
            ev.record(main)

            def threaded():   # the verifier's frozen towers: queued by a second host thread from t = 0 (see Pipeline.decision)
                torch.cuda.set_device(self.dev)
                self.side.wait_event(ev)
                with torch.cuda.stream(self.side):
                    if os.environ.get("COVER_SIDE_GRAPH", SIDE_GRAPH_DEFAULT) == "2":
                        return self.ver.shared_embeddings_graph(i["img384"], i["text"])
                    return self._side_work()

            if os.environ.get("COVER_SIDE_GRAPH", SIDE_GRAPH_DEFAULT) == "1":   # (see Pipeline.decision)
                self.side.wait_event(ev)
                with torch.cuda.stream(self.side):
                    its = self.ver.shared_embeddings_graph(i["img384"], i["text"])
                x = self.model.sample_actions([i["img"]], [self.all_valid], i["toks"], i["masks"], i["state"], noise=noise)
            else:
                fut = self.pool.submit(threaded)
                x = self.model.sample_actions([i["img"]], [self.all_valid], i["toks"], i["masks"], i["state"], noise=noise)
                its = fut.result()
            main.wait_stream(self.side)
        hists, pad = ops.actions_to_histories(x, self.c["chunk"], self.past_dev, self.lo_hi)
        r = self.ver.score_histories(its, hists, self.S, pad=pad)
        self.last_scores = r["scores"]
        return int(r["result"][0]), x


def _profile_phases(pipe):
    """One serialised pi0 decision with the in-library kernel timers read out at every phase boundary."""
    import ctypes as C
    from cover_vla_amd import _lib as L
    h = L.lib()
    n = N_PROF
    out = {}

    def begin():
        L.check(h.cover_profile_begin(32768), "profile_begin")

    def end(name):
        ms, cnt, work = (C.c_double * n)(), (C.c_longlong * n)(), (C.c_double * n)()
        L.check(h.cover_profile_end_n(ms, cnt, work, n), "profile_end")
        out[name] = (list(ms), list(cnt), list(work))

    def on_phase(name):
        end(name)
        begin()

    begin()
    try:
        pipe.decision(serial=True, on_phase=on_phase)
    finally:
        end("verifier_heads")
    return out


def pi0_cpu_baseline(pipe, batch):
    """The CPU oracle (oracle/cover_ref/pi0.py + verifier.py, PyTorch-CPU eager, bf16 PaliGemma / fp32 projections as the reference casts
    them) executing the decision AS THE REFERENCE EXECUTES IT: ONE sample_actions call on the whole batch of `batch` rows -- the vision
    tower and the 18-layer prefix run on every row, no dedup (modeling_pi0.py:672-715; run_simpler_eval_with_openpi.py:305-326) --
    then the verifier. Beside it the de-duplicated schedule this repo runs (tower once, prefix once per distinct prompt), timed, not
    composed: the oracle's prefix pass on the 8 distinct rows + its Euler loop on all rows."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from cover_ref import blocks as Bk, pi0 as PR, openvla as OR, verifier as V
    from cover_vla_amd import host, synth
    t_all = time.time()
    c, dev = pipe.c, pipe.dev
    sd = PR.cast_like_reference({k: v.cpu() for k, v in synth.pi0_state(c, seed=1234, nontrivial=False, std=0.02, device=dev, wdtype=torch.bfloat16).items()})
    ssd = Bk.to_bf16({k: v.cpu() for k, v in synth.siglip2_state(pipe.sc, seed=4321, nontrivial=False, device=dev, wdtype=torch.bfloat16).items()})
    torch.cuda.empty_cache()
    vit = Bk.VitCfg(c["vit_dim"], c["vit_layers"], c["vit_heads"], c["vit_mlp"], c["patch"], "gelu_tanh", 1e-6)
    lm = Bk.DecoderCfg(c["lm_dim"], c["layers"], c["Hq"], c["Hkv"], c["D"], c["lm_mlp"], "gelu_tanh", "gemma", 1e-6, "pi0")
    ex = Bk.DecoderCfg(c["ex_dim"], c["layers"], c["Hq"], c["Hkv"], c["D"], c["ex_mlp"], "gelu_tanh", "gemma", 1e-6, "pi0")
    cfg = PR.Pi0Cfg(vit, lm, ex, proj_width=c["ex_dim"], chunk_size=c["chunk"], n_img_tokens=(c["image"] // c["patch"]) ** 2)
    i = pipe.inp
    B = min(batch, pipe.B)
    rows = list(range(B))
    img, toks, masks, state, noise = (i[k][rows].cpu() for k in ("img", "toks", "masks", "state", "noise"))
    ck = synth.verifier_checkpoint(3, seed=1234)
    stt = host.bridge_statistics()["action"]
    ph = {}
    with torch.no_grad():
        t0 = time.perf_counter()
        x = PR.sample_actions(cfg, sd, [img], [torch.ones(B, dtype=torch.bool)], toks, masks, state, noise)
        ph["policy_as_executed"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        pf, tf = OR.siglip2_features(pipe.sc, ssd, i["img384"].cpu(), i["text"].cpu())
        ph["verifier_towers"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        xa = x[:, : c["chunk"], :7].double().numpy()
        hists = host.process_inputs([xa[:, t] for t in range(c["chunk"])], True, [i["past"][k] for k in range(6)], c["chunk"])
        V.compute_max_similarity_scores(ck["ensemble_components"], pf, tf, hists, max(1, B // pipe.P))
        ph["verifier_heads"] = time.perf_counter() - t0
        # the de-duplicated schedule, timed: prefix (vision + 18 layers) on ONE row per distinct prompt, Euler loop on all rows
        first = [p * pipe.S for p in range(pipe.P) if p * pipe.S < B]
        t0 = time.perf_counter()
        tr = {}
        PR.sample_actions(cfg, sd, [img[first]], [torch.ones(len(first), dtype=torch.bool)], toks[first], masks[first], state[first], noise[first], trace=tr)
        ph["policy_on_distinct_prompts_only"] = time.perf_counter() - t0
    as_exec = ph["policy_as_executed"] + ph["verifier_towers"] + ph["verifier_heads"]
    # dedup: distinct-prompt run covers the prefix; its Euler loop ran on len(first) rows, the remaining rows' loop scales by rows
    model, isa = _cpu_info()
    r2 = lambda v: round(float(v), 2)
    return {"value": round(B / as_exec, 4), "unit": "candidates/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"ONE decision, batch of {B} rows in one sample_actions call exactly as the reference executes it (vision tower + 18-layer prefix on every row, "
                      f"10 Euler steps) + verifier towers + 3-member heads; cold (first call in the process), one run",
            "decision_seconds_as_executed": r2(as_exec), "phase_seconds": {k: round(v, 3) for k, v in ph.items()},
            "dedup_variant": {"note": "sample_actions on the distinct prompts only (the prefix work this repo's schedule does) -- a lower bound of the "
                                      "de-duplicated CPU decision: the other rows add their Euler loops only",
                              "rows": len(first), "seconds": r2(ph["policy_on_distinct_prompts_only"] + ph["verifier_towers"] + ph["verifier_heads"])},
            "total_cpu_leg_seconds": r2(time.time() - t_all), "cpu_model": model, "isa": isa,
            "dtype": "bf16 PaliGemma + expert layers, fp32 projections (to_bfloat16_like_physical_intelligence), eager PyTorch-CPU"}


def main_pi0(a):
    """`--profile pi0`: the contractual line for P1 (same JSON schema as the headline)."""
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: bench.py measures the HIP path only (no CPU fallback)"}))
        sys.exit(2)
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    pipe = Pi0Pipeline(dev)
    for _ in range(a.warmup):
        pipe.decision()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        idx, x = pipe.decision()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {"actions": x, "scores": pipe.last_scores, "winner_index": [idx]})
    assert torch.isfinite(x).all()
    ms_per_step = 1e3 * dt / a.steps
    B, c = pipe.B, pipe.c
    out = {"metric": "candidate actions scored/sec (whole node), pi0 (PaliGemma-3B + 300M action expert) B=40, 224^2 RGB",
           "value": round(B * a.steps / dt, 3), "unit": "candidates/s", "n_gpus": 1, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
           "data": "synthetic",
           "config": {"workload": f"pi0 (SigLIP-So400m + Gemma-2B prefix + 300M expert) B={B} = {pipe.P} prompts x {pipe.S} samples, chunk {c['chunk']}, 10 Euler steps, "
                                  f"tokenizer max_length {pipe.L}, one 224x224 RGB frame; CoVer verifier SigLIP2-L/16-384 + 3-member ensemble; random-init weights",
                      "candidates_total": B, "parallelism": "one GPU", "lib_sha16": lib_hash(), "selected": idx,
                      "denoise_chains": pipe.model.n_chains, "denoise_graph": pipe.model.denoise_graph}}
    if a.full and not a.no_profile:
        ph = _profile_phases(pipe)
        M_exp = B * (1 + c["chunk"])
        ms_d, cnt_d, work_d = ph["denoise"]
        ms_p, cnt_p, work_p = ph["prefix"]
        ms_v, cnt_v, work_v = ph["verifier_towers"]
        exp_bytes = work_d[1] / M_exp            # tiled-GEMM work is 2 M N K FLOP; the weight bytes of the same launches are 2 N K
        ach = exp_bytes / (ms_d[1] * 1e-3) / 1e9 if ms_d[1] > 0 else 0.0
        out["roofline"] = {"bound": "hbm", "kernel": f"gemm_tiled at M = {M_exp} rows (the action expert's 4 projections x 18 layers x 10 Euler steps): bound by weight bytes "
                                                     "on paper, by the latency of a 5-15 us launch in practice (latency-bound: see launches / avg_launch_us)",
                           "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None,
                           "launches": int(cnt_d[1]), "avg_launch_us": round(1e3 * ms_d[1] / max(cnt_d[1], 1), 2),
                           "algorithmic_bytes_per_launch": round(exp_bytes / max(cnt_d[1], 1)), "algorithmic_bytes_per_decision": exp_bytes,
                           "kernel_ms_per_decision": round(ms_d[1], 3), "splitk_reduce_ms_per_decision": round(ms_d[6], 3),
                           "attention_ms_per_decision": round(ms_d[2], 3), "attention_launches": int(cnt_d[2])}
        tp = ms_p[1] + ms_p[4] + ms_p[6] + ms_p[8]
        fp = work_p[1] + work_p[4]
        if tp > 0:
            tf = fp / (tp * 1e-3) / 1e12
            out["roofline_mfma"] = {"bound": "mfma", "kernel": "gemm_tiled_v3 (self-loading, prefix pass) / gemm_tiled: SigLIP-So400m tower + projector + the 18-layer Gemma-2B prefix pass "
                                                               f"(M = {pipe.P} x (256 + longest real prompt) rows), split-K reductions included",
                                    "achieved": round(tf, 1), "peak": MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": round(tf / MFMA_PEAK_TF, 4),
                                    "launches": int(cnt_p[1] + cnt_p[4]), "kernel_ms_per_decision": round(tp, 3), "flop_per_decision": fp}
            if ms_p[4] > 0:   # the LLM-sized GEMMs of the prefix pass WITH the split-K reductions that complete them (profiler class 8)
                t4 = work_p[4] / ((ms_p[4] + ms_p[8]) * 1e-3) / 1e12
                out["roofline_mfma"]["prefix_mlp"] = {"achieved": round(t4, 1), "frac": round(t4 / MFMA_PEAK_TF, 4), "launches": int(cnt_p[4]),
                                                      "kernel_ms_per_decision": round(ms_p[4] + ms_p[8], 3), "splitk_reduce_ms": round(ms_p[8], 3),
                                                      "gemm_kernels_only_frac": round(work_p[4] / (ms_p[4] * 1e-3) / 1e12 / MFMA_PEAK_TF, 4)}
        fv = work_v[1] + work_v[4]
        floor_ms = 1e3 * (exp_bytes / (HBM_PEAK_GBS * 1e9) + (fp + fv) / (MFMA_PEAK_TF * 1e12))
        out["end_to_end"] = {"floor_ms": round(floor_ms, 3), "measured_ms": round(ms_per_step, 3), "frac": round(floor_ms / ms_per_step, 4),
                             "floor": "expert weight bytes (10 steps) / 8 TB/s + (tower + prefix + verifier-tower tiled FLOPs) / 2.5 PFLOP/s (attention, norms, fp32 heads: 0)"}
        out["phase_kernel_ms"] = {k: {"gemm_tiled_small": round(v[0][1], 3), "gemm_tiled_llm": round(v[0][4], 3), "splitk_reduce": round(v[0][6] + v[0][5] + v[0][8], 3),
                                      "attention": round(v[0][2], 3), "weight_streaming": round(v[0][0] + v[0][3], 3),
                                      "launches": int(sum(v[1]))} for k, v in ph.items()}
        for k in ("roofline", "roofline_mfma"):
            if k in out and out[k]["frac"] > 1.0:
                out[k] = {"invalid": f"frac {out[k]['frac']} > 1: refused"}
    if a.full and not a.no_cpu_baseline:
        out["cpu_baseline"] = pi0_cpu_baseline(pipe, a.cpu_batch)
    print(json.dumps(out), flush=True)


def _cpu_info():
    model, flags = "unknown", set()
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name") and model == "unknown":
                    model = line.split(":", 1)[1].strip()
                elif line.startswith("flags") and not flags:
                    flags = set(line.split(":", 1)[1].split())
    except OSError:
        pass
    return model, {"amx_bf16": "amx_bf16" in flags, "avx512_bf16": "avx512_bf16" in flags, "avx512f": "avx512f" in flags}


def sampled_pick_decided(logits, t, u, err, temperature=1.0, eps=1e-4):
    """Is the inverse-CDF pick of bin t on uniform u DATA-DECIDED against logit perturbations of magnitude <= err? logits [..., bins] (float64),
    t [...] int64 (the picked bin: first j with cumsum_j > u * total), u, err [...]. Exact worst case: with p_j = exp(l_j / T) and c = the
    normalised mass up to an edge, the perturbation that moves the edge furthest up multiplies every p_j below it by e^(err/T) and every p_j
    above it by e^(-err/T): c -> c e^a / (c e^a + (1 - c) e^-a), a = err / T (and down with the signs swapped). The pick survives every
    perturbation iff the lower edge of bin t cannot reach u and the upper edge cannot fall to u (eps = 1e-4 of the total mass: the sequential fp32
    cumsum of 256 terms in both selectors is good to ~2e-5 relative)."""
    l = logits.double()
    p = torch.exp((l - l.amax(dim=-1, keepdim=True)) / temperature)
    cs = torch.cumsum(p, -1) / p.sum(-1, keepdim=True)
    nb = l.shape[-1]
    hi_edge = torch.gather(cs, -1, t[..., None])[..., 0]
    lo_edge = torch.where(t > 0, torch.gather(cs, -1, (t - 1).clamp(min=0)[..., None])[..., 0], torch.zeros_like(hi_edge))
    ea = torch.exp(err.double() / temperature)
    up = lambda c: (c * ea) / (c * ea + (1 - c) / ea)
    down = lambda c: (c / ea) / (c / ea + (1 - c) * ea)
    return (up(lo_edge) < u - eps) & ((down(hi_edge) > u + eps) | (t == nb - 1))


def oracle_agreement(pipe, tok_o, logits_o, sel_o, n_prompts, free=None):
    """Full-size agreement of the HIP path with the CPU oracle on the SAME decision (checkpoint, frame, prompts, uniforms): what
    run_simpler_eval_with_openpi.py:305-326 (one batched policy call) and :346-365 (verifier scores -> grouped arg-max) produce.
      tokens : the HIP sampler TEACHER-FORCED on the oracle's tokens (every step then compares like with like; the returned tokens are the
               HIP path's own picks), per (row, step): err = max |logit difference| over the action bins; the oracle's inverse-CDF pick
               of bin t on uniform u is DATA-DECIDED when no logit perturbation of magnitude <= err can move either CDF edge of bin t
               across u -- exactly: an edge at cumulative mass c moves at most to c e^(a) / (c e^(a) + (1 - c) e^(-a)), a = err / T
               (the mass below the edge up-weighted, the rest down-weighted). This is the worst case the relative bound
               exp(4 err / T) - 1 of tests/test_openvla_gpu.py over-estimates; a pick that is decided must be equal bit for bit.
      scores : the HIP verifier on the ORACLE's tokens (same histories) against the oracle's scores; the winner must be the same
               whenever the oracle's own margins (best group mean vs runner-up, best candidate in that group vs runner-up) exceed
               twice the largest score difference.
    free = (winner index, tokens) of the free-running HIP decision: reported (token agreement, same winner), not asserted -- after
    the first undecided pick two free-running histories are different sequences."""
    from cover_vla_amd import ops
    i, S, dev, c = pipe.inp, pipe.n_samples, pipe.dev, pipe.c
    N_ = n_prompts * S
    lo, hi = c["tok_vocab"] - c["n_bins"], c["tok_vocab"]
    n_gen = tok_o.shape[1]
    tr = {}
    tok_g, _ = pipe.policy.sample(i["frame"], i["toks"][:n_prompts].contiguous(), i["lens"][:n_prompts].contiguous(), S,
                                  i["u"][:N_].contiguous(), 1.0, trace=tr, force_tokens=tok_o.to(dev))
    tok_g = tok_g.cpu()
    lg = torch.stack([l[:N_, lo:hi].float().cpu() for l in tr["logits"][:n_gen]], 1).double()      # [N, n_gen, bins]
    lo_ = logits_o[:, :n_gen, lo:hi].double()
    u = i["u"][:N_, :n_gen].cpu().double()
    err = (lg - lo_).abs().amax(dim=2)                                                                # [N, n_gen]
    t = (tok_o[:, :n_gen] - lo).clamp(0, hi - lo - 1)
    decided = sampled_pick_decided(lo_, t, u, err)
    same = tok_g[:, :n_gen] == tok_o[:, :n_gen]
    n_dec = int(decided.sum())
    rel = ((lg - lo_).flatten(1).norm(dim=1) / lo_.flatten(1).norm(dim=1))
    # verifier on the oracle's tokens
    hb, pad = ops.tokens_to_histories(tok_o.to(dev), c["tok_vocab"], pipe.centers, pipe.past_dev, n_use=1)
    pf, tf = pipe.ver.extract_shared_features(i["img384"], i["text"])
    r = pipe.ver.score_histories(pipe.ver.image_text_embeddings(pf, tf), hb, S, pad=pad)
    sc_g, sc_o = r["scores"].float().cpu().double(), torch.as_tensor(np.asarray(sel_o["scores"])).double().flatten()
    s_err = float((sc_g - sc_o).abs().max())
    gm = sc_o.view(n_prompts, S).mean(1)
    g_best = int(sel_o["group"])
    m_group = float(gm[g_best] - gm[torch.arange(n_prompts) != g_best].max()) if n_prompts > 1 else float("inf")
    in_g = sc_o.view(n_prompts, S)[g_best]
    m_cand = float(in_g.max() - in_g[torch.arange(S) != int(in_g.argmax())].max()) if S > 1 else float("inf")
    w_decided = min(m_group, m_cand) > 2 * s_err
    out = {"rows": N_, "steps": n_gen, "decided": n_dec, "of": int(decided.numel()),
           "agree_on_decided": round(float(same[decided].double().mean()), 6) if n_dec else None,
           "agree_all_teacher_forced": round(float(same.double().mean()), 4),
           "logit_max_abs": round(float(err.max()), 4), "logit_rel_l2_max": round(float(rel.max()), 4),
           "score_max_abs": round(s_err, 6), "winner_same": bool(int(r["result"][0]) == int(sel_o["global_idx"])), "winner_decided": bool(w_decided),
           "oracle_winner": int(sel_o["global_idx"]), "oracle_margins": {"group_mean": round(m_group, 5), "within_group": round(m_cand, 5)},
           "criterion": "HIP sampler teacher-forced on the oracle's tokens; a pick is decided when no logit perturbation <= the measured max |logit difference| of that "
                        "(row, step) can move a CDF edge of the picked bin across the uniform (exact worst case); HIP verifier on the oracle's tokens vs the oracle's scores"}
    if free is not None:
        gi_f, tok_f = free
        tok_f = tok_f[:N_, :n_gen].cpu()
        first = (tok_f != tok_o[:, :n_gen]).int().argmax(1)
        out["free_running"] = {"token_agreement": round(float((tok_f == tok_o[:, :n_gen]).double().mean()), 4), "winner_same": bool(int(gi_f) == int(sel_o["global_idx"])),
                               "rows_identical": int((tok_f == tok_o[:, :n_gen]).all(1).sum())}
    return out


def oracle_state(pipe):
    """The CPU oracle's copy of the SAME synthetic checkpoints the pipeline holds (drawn on the device with the same seeds, copied to the host)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from cover_ref import blocks as Bk
    from cover_vla_amd import synth
    c, sc, dev = pipe.c, pipe.sc, pipe.dev
    sd = {k: v.cpu() for k, v in synth.openvla_state(c, seed=1234, nontrivial=False, device=dev, wdtype=torch.bfloat16, peaked=pipe.peaked).items()}
    sd = Bk.to_bf16(sd)
    ssd = Bk.to_bf16({k: v.cpu() for k, v in synth.siglip2_state(sc, seed=4321, nontrivial=False, device=dev, wdtype=torch.bfloat16).items()})
    torch.cuda.empty_cache()
    ck = synth.verifier_checkpoint(len(pipe.ver.trainable_models), seed=1234, num_patches=(sc["image"] // sc["patch"]) ** 2, vision_dim=sc["dim"], text_dim=sc["dim"])
    return sd, ssd, ck


def oracle_batched_decision(pipe, sd, ssd, ck, n_prompts):
    """ONE decision of the CPU oracle on the pipeline's first n_prompts prompt groups, executed the way the reference executes it
    (oracle/cover_ref/openvla.py::sample_batched + the verifier). Returns (tokens, trace with logits / seconds, selection, policy s, towers s, heads s)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from cover_ref import openvla as OR, verifier as V
    c, sc, i, S = pipe.c, pipe.sc, pipe.inp, pipe.n_samples
    N_ = n_prompts * S
    trb = {"seconds": {}}
    with torch.no_grad():
        t0 = time.perf_counter()
        tok_b = OR.sample_batched(c, sd, i["frame"][:1].cpu(), i["toks"][:n_prompts].cpu(), i["lens"][:n_prompts].cpu(), S, i["u"][:N_].cpu(), 1.0, trace=trb)
        t_pol = time.perf_counter() - t0
        t0 = time.perf_counter()
        pf, tf = OR.siglip2_features(sc, ssd, i["img384"].cpu(), i["text"].cpu())
        t_tow = time.perf_counter() - t0
        t0 = time.perf_counter()
        acts = OR.tokens_to_actions(c, tok_b.numpy())                            # [N, 7]
        hists = [np.concatenate([i["past"], acts[n:n + 1].astype(np.float64)], 0) for n in range(N_)]
        sel_b = V.compute_max_similarity_scores(ck["ensemble_components"], pf, tf, hists, S)
        t_heads = time.perf_counter() - t0
    return tok_b, trb, sel_b, t_pol, t_tow, t_heads


def cpu_baseline(pipe, timed=1, batched=True, free=None):
    """BASELINE.md 4 protocol, bounded: the CPU oracle (oracle/cover_ref, PyTorch-CPU eager bf16) executes FULL candidates exactly as
    an eager, un-deduplicated implementation does -- both vision towers at full depth, the 3-layer projector, all 32 Llama layers for
    the T ~ 280 prefill and six single-token decode steps with a concatenated KV cache, lm_head x 7, then the verifier (SigLIP2-L
    image + text towers at full depth, 3-member heads, trajectory encoder, score) -- on the SAME synthetic 7B checkpoint the GPU path
    uses (drawn in HBM, copied to the host). CANDIDATES are timed, not decisions (a 32-candidate decision is ~10 minutes of CPU):
      run 0  = BASELINE config 1 (N = 1, greedy) and the warm-up (cold: oneDNN primitive creation, page-in) -- reported on its own;
      runs 1..timed = sampled candidates (another prompt / uniform row each), `value` = 1 / median.
    N = 32 as the reference executes it (no dedup; a batch of N full forwards does N x the FLOPs of one -- the path is compute-bound
    on a CPU) = 32 x the median. The de-duplicated variant is COMPOSED from the medians of the measured phases: vision once + verifier
    towers once + 8 prefills + 32 x (decode + heads) -- what a CPU run of this repo's schedule would cost; reported beside it so
    the part of the GPU/CPU ratio that is dedup rather than kernels is visible."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from cover_ref import openvla as OR, verifier as V
    c, sc = pipe.c, pipe.sc
    t_all = time.time()
    sd, ssd, ck = oracle_state(pipe)
    i = pipe.inp
    frame, img384, text = i["frame"][:1].cpu(), i["img384"].cpu(), i["text"].cpu()
    S = pipe.n_samples

    n_local = len(pipe.prompt_ids)

    def one_candidate(p, greedy):
        p = p % n_local                                        # (--config 3 on one GPU: a single local prompt group)
        toks, lens = i["toks"][p:p + 1].cpu(), i["lens"][p:p + 1].cpu()
        u = None if greedy else i["u"][p * S:p * S + 1].cpu()
        tr = {"seconds": {}}
        with torch.no_grad():
            tok = OR.sample(c, sd, frame, toks, lens, 1, u, 1.0, trace=tr)
            ph = dict(tr["seconds"])
            t0 = time.perf_counter()
            pf, tf = OR.siglip2_features(sc, ssd, img384, text)
            ph["verifier_towers"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            acts = OR.tokens_to_actions(c, tok.numpy())                              # [1, 7]
            hist = [np.concatenate([i["past"], acts.astype(np.float64)], 0)]
            V.compute_max_similarity_scores(ck["ensemble_components"], pf, tf, hist, 1)
            ph["verifier_heads"] = time.perf_counter() - t0
        ph["total"] = sum(ph.values())
        return ph

    cold = one_candidate(0, True)                          # config 1: N = 1 greedy (and the warm-up)
    runs = [one_candidate(1 + r, False) for r in range(timed)]
    # ---- the decision AS THE REFERENCE EXECUTES IT, measured (not multiplied): ONE batched policy call on the N un-deduplicated rows
    # (run_simpler_eval_with_openpi.py:296-326: the frame repeated for every row, one call) -- vision towers on N frames, one left-padded
    # batched prefill, six batched decode steps, lm_head on N rows x 7 -- then the verifier on one image + P instructions and N histories
    asx = None
    if batched:
        P_, N_ = n_local, n_local * S
        tok_b, trb, sel_b, t_pol, t_tow, t_heads = oracle_batched_decision(pipe, sd, ssd, ck, P_)
        dec_s = t_pol + t_tow + t_heads
        # the oracle's decision is the CHECKER of the GPU decision on the same checkpoint, frame, prompts and uniforms (never the other way round)
        # (bf16 profile only: the fp8 profile's oracle runs on the de-quantised weights, tests/test_openvla_gpu.py)
        agreement = oracle_agreement(pipe, tok_b, trb["logits"], sel_b, P_, free=free) if (pipe.weight_dtype == "bf16" and pipe.horizon == 1) else None
        asx = {"decision_seconds": round(dec_s, 2), "candidates_per_s": round(N_ / dec_s, 4), "rows": N_, "measured": True,
               "phase_seconds": {**{k: round(v, 3) for k, v in trb["seconds"].items()}, "verifier_towers": round(t_tow, 3), "verifier_heads": round(t_heads, 3)},
               "agreement": agreement,
               "note": "ONE decision: policy = one batched forward over the N un-deduplicated rows (both vision towers + projector on N copies of the frame, "
                       "left-padded batched prefill of N full sequences, 6 batched decode steps over a concatenated KV cache, lm_head on N rows x 7: "
                       "oracle/cover_ref/openvla.py::sample_batched), verifier = SigLIP2 towers on one image + P instructions, 3-member heads on N histories; "
                       "warm (fourth policy evaluation of the process), one run"}
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    per_cand = med["total"]
    P, N = len(pipe.prompt_ids), len(pipe.prompt_ids) * S
    dedup = med["vision"] + med["verifier_towers"] + P * med["prefill"] + N * (med["decode"] + med["verifier_heads"])
    model, isa = _cpu_info()
    r2 = lambda x: round(float(x), 2)
    return {"value": asx["candidates_per_s"] if asx else round(1.0 / per_cand, 4), "unit": "candidates/s", "cores": torch.get_num_threads(), "kind": "port",
            "value_is": ("as_executed_batched: N / the measured seconds of ONE batched, un-deduplicated N-row decision (the way the reference executes a decision)" if asx
                         else "per_candidate_unbatched: 1 / the median seconds of one batch-1 candidate (pessimistic: see extrapolation)"),
            "as_executed_batched": asx, "agreement": asx["agreement"] if asx else None,
            "per_candidate_unbatched": {"candidates_per_s": round(1.0 / per_cand, 4), "seconds_per_candidate": r2(per_cand),
                                        "note": "secondary figure: one full candidate at batch 1 (no weight re-use across rows); N x this is an upper bound of the decision time"},
            "extrapolation": f"per_candidate_unbatched only: N={N} x ONE timed single-candidate forward (batch 1) = {N * per_cand:.0f} s would be a pessimistic bound of the "
                             "decision; the reference runs the N candidates as ONE batch (run_simpler_eval_with_openpi.py:305-326), which as_executed_batched measures",
            "sample": f"1 cold run (config 1: N=1 greedy) + {timed} timed FULL candidate(s) at batch 1 + ONE batched N={N} decision. One candidate = "
                      f"an eager un-deduplicated forward (all layers of every tower, 32 Llama layers prefill T~{1 + 256 + int(i['lens'][1 % n_local])} + 6 decode "
                      f"steps, lm_head x7, verifier towers + 3-member heads)",
            "seconds_per_candidate": r2(per_cand), "seconds_per_candidate_runs": [r2(r["total"]) for r in runs],
            "phase_seconds_median": {k: round(v, 3) for k, v in med.items()},
            "config1_n1_greedy": {"seconds": r2(cold["total"]), "candidates_per_s": round(1.0 / cold["total"], 4), "note": "cold (first run in the process); warm it equals a timed candidate: the arithmetic differs only in the pick rule"},
            "as_executed_decision_seconds": r2(N * per_cand),
            "dedup_variant": {"decision_seconds": r2(dedup), "candidates_per_s": round(N / dedup, 4),
                              "composition": f"vision + verifier towers once + {P} prefills + {N} x (decode + heads), from the phase medians"},
            "total_cpu_leg_seconds": r2(time.time() - t_all), "cpu_model": model, "isa": isa, "dtype": "bf16 weights, eager PyTorch-CPU"}


def fp8_agreement(pipe, dev, a, n_prompts_global, prompt_ids):
    """What quantisation changes ("report arg-max agreement rate and score RMSE"), per decode step and per source:
    the SAME decision (frame, prompts, uniforms) through a bf16 pipeline of the same synthetic checkpoint, then -- TEACHER-FORCED on
    the bf16 run's tokens, so that step t compares like with like instead of two diverged histories -- through (a) this fp8 pipeline
    as it runs (e4m3 weights; e4m3 activations in every pass with more than 64 rows: the 448-row prefill at N = 32, every pass at
    N = 512) and (b) the same pipeline with COVER_FP8_MFMA=0 (e4m3 WEIGHTS only, bf16 activations everywhere). Per step: rel-L2 of
    the action-bin logits against bf16, top-1 agreement over the action bins, and the agreement among the rows whose bf16 top-1 / top-2
    margin exceeds twice the row's max logit error (the picks the data decide). Random-init weights have no margin to spare
    (top-1 / top-2 gaps of ~0.3 logits against quantisation noise of the same size), so raw agreement on them is a noise-to-margin
    ratio, not a verdict on the kernels: the decided-row agreement and the logit errors are the numbers that transfer."""
    gi8, tok8, _ = pipe.decision()
    sc8 = pipe.last_scores.clone()
    ref = Pipeline(dev, small=a.small, n_prompts=n_prompts_global, n_samples=a.samples, n_cams=a.cams, members=a.members,
                   prompt_ids=prompt_ids, weight_dtype="bf16", horizon=a.horizon, own_kv=pipe.own_kv if pipe.own_kv != "fp8" else "bf16", peaked=pipe.peaked)
    gi16, tok16, _ = ref.decision()
    sc16 = ref.last_scores
    i, S = pipe.inp, pipe.n_samples
    lo, hi = pipe.c["tok_vocab"] - pipe.c["n_bins"], pipe.c["tok_vocab"]
    n_steps = min(tok16.shape[1], 7)           # (config 5 decodes 56 tokens: the first chunk's seven carry the comparison)

    def forced_logits(p):
        tr = {}
        p.policy.sample(i["frame"], i["toks"], i["lens"], S, i["u"], 1.0, trace=tr, force_tokens=tok16)
        return [lg[:, lo:hi].float() for lg in tr["logits"][:n_steps]]

    l16 = forced_logits(ref)
    l8 = forced_logits(pipe)
    os.environ["COVER_FP8_MFMA"] = "0"
    try:
        l8w = forced_logits(pipe)
    finally:
        os.environ.pop("COVER_FP8_MFMA", None)

    def per_step(lq):
        rows = []
        for t in range(n_steps):
            b, q = l16[t], lq[t]
            err = (q - b).abs().amax(dim=1)
            top2 = b.topk(2, dim=1).values
            decided = (top2[:, 0] - top2[:, 1]) > 2 * err
            same = q.argmax(1) == b.argmax(1)
            rows.append({"logit_rel_l2": round(float((q - b).norm() / b.norm()), 4), "top1_agreement": round(float(same.float().mean()), 4),
                         "decided_rows": int(decided.sum()), "decided_agreement": (round(float(same[decided].float().mean()), 4) if bool(decided.any()) else None)})
        return rows

    dbin = (tok8 - tok16).abs().float()
    res = {"token_agreement_free_running": round(float((tok8 == tok16).float().mean()), 4), "mean_bin_distance": round(float(dbin.mean()), 3),
           "first_token_agreement": round(float((tok8[:, 0] == tok16[:, 0]).float().mean()), 4),
           "score_rmse": round(float((sc8 - sc16).pow(2).mean().sqrt()), 5), "winner_same": bool(gi8 == gi16),
           "teacher_forced_per_step": {"weights_and_activations_e4m3 (as run)": per_step(l8), "weights_only_e4m3 (COVER_FP8_MFMA=0)": per_step(l8w)},
           "logit_spread": round(float(l16[0].std()), 3),
           "note": "free-running numbers compare two diverged token histories after the first disagreement; the teacher-forced table isolates each step. "
                   "e4m3 weights: per-channel 2^e scales (the e4m3 stream is bit-identical to a bf16 GEMM on the de-quantised weights, tests/test_fp8_gpu.py); "
                   "e4m3 activations: per-row 2^e scales in every pass with more than 64 rows (error bound: tests/test_fp8_gpu.py::test_fp8_activation_error_bound_with_outliers)"}
    del ref
    torch.cuda.empty_cache()
    return res


def dump_outputs(out_dir, arrays):
    """--dump-outputs: what the last timed decision returned, one DIR/<name>.npy per array (float32 scores / actions, float64 indices and
    tokens: exact as integers). The arrays are small (a decision returns N scores and N x 7 x horizon tokens or N x chunk x 32 actions)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, x in arrays.items():
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu()
            x = (x.double() if x.dtype == torch.float64 or not x.is_floating_point() else x.float()).numpy()
        else:
            x = np.asarray(x, dtype=np.float64)
        np.save(os.path.join(out_dir, f"{name}.npy"), np.ascontiguousarray(x))


def lib_hash():
    from cover_vla_amd import _lib as L
    h = hashlib.sha256()
    with open(L.LIB_PATH, "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def profile_decision(pipe, world, rank, cpu_gather):
    import ctypes as C
    from cover_vla_amd import _lib as L
    h = L.lib()
    n = N_PROF
    ms, cnt, work = (C.c_double * n)(), (C.c_longlong * n)(), (C.c_double * n)()
    L.check(h.cover_profile_begin(32768), "profile_begin")
    try:
        pipe.decision(world, rank, cpu_gather, serial=True)
    finally:   # an exception in between must not leave the profiler armed (the next begin would return COVER_EINVAL)
        rc = h.cover_profile_end_n(ms, cnt, work, n)
    L.check(rc, "profile_end (event pool overflow = incomplete sums)")
    return list(ms), list(cnt), list(work)


def roofline_objects(ms, cnt, work, ms_per_step, lib_sha):
    out = {}

    def guard(name, obj):
        if obj["frac"] > 1.0:   # a fraction above the peak means the timer did not time the work: not evidence
            out[name] = {"invalid": f"frac {obj['frac']} > 1: refused", "launches": obj.get("launches")}
        else:
            out[name] = obj

    if cnt[0] > 0 and ms[0] > 0:
        # the split-K reduce (+ residual + RMSNorm) launches that COMPLETE o_proj / down / qkv belong to the streaming GEMMs they finish: their
        # time is part of the denominator (as roofline_mfma counts its reductions); the kernels alone are quoted beside it
        ach = work[0] / ((ms[0] + ms[5]) * 1e-3) / 1e9
        ach_k = work[0] / (ms[0] * 1e-3) / 1e9
        traffic, tnote = None, "no PMC pass recorded for this build"
        try:  # HBM bytes per launch from the PMC pass of the SAME build (rocprofv3 --pmc FETCH_SIZE, x2 gfx950 correction): newest matching file
            import glob
            for fn in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic.json")), reverse=True):
                with open(fn) as f:
                    t = json.load(f)
                rel = os.path.relpath(fn, ROOT)
                if t.get("lib_sha16") == lib_sha:
                    traffic, tnote = round(t["hbm_fetch_bytes_per_launch"]), f"{rel} (lib {lib_sha})"
                    break
                tnote = f"{rel} is from lib {t.get('lib_sha16')}, this run is {lib_sha}: not quoted"
        except Exception:
            pass
        guard("roofline", {"bound": "hbm", "kernel": "gemm_skinny2 / gemm_skinny3 (weight-streaming GEMMs of the 7B decode passes and lm_head, M = 32, >= 16 MB of weights each) "
                                                     "+ the splitk_reduce_norm launches that complete them",
                           "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                           "traffic": traffic, "traffic_source": tnote, "algorithmic_bytes_per_launch": round(work[0] / cnt[0]), "launches": int(cnt[0]),
                           "avg_launch_us": round(1e3 * ms[0] / cnt[0], 2), "algorithmic_bytes_per_decision": work[0],
                           "kernel_ms_per_decision": round(ms[0] + ms[5], 3), "streaming_kernels_only": {"ms": round(ms[0], 3), "achieved": round(ach_k, 1),
                                                                                                         "frac": round(ach_k / HBM_PEAK_GBS, 4)},
                           "splitk_reduce_ms_per_decision": round(ms[5], 3)})
    t_mfma = ms[1] + ms[4] + ms[6] + ms[8]
    if cnt[1] + cnt[4] > 0 and t_mfma > 0:
        tf_all = (work[1] + work[4]) / (t_mfma * 1e-3) / 1e12
        obj = {"bound": "mfma", "kernel": "gemm_tiled_v3 (self-loading 224-row tiles: LLM prefill) / gemm_tiled (64-row tiles: towers) (LLM prefill + DINOv2 / SigLIP / SigLIP2 towers + projector), split-K reductions included",
               "achieved": round(tf_all, 1), "peak": MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": round(tf_all / MFMA_PEAK_TF, 4),
               "launches": int(cnt[1] + cnt[4]), "kernel_ms_per_decision": round(t_mfma, 3), "flop_per_decision": work[1] + work[4]}
        if cnt[4] > 0 and ms[4] > 0:   # every sub-object carries the split-K reductions of ITS OWN GEMMs (profiler classes 8 / 6)
            tf_p = work[4] / ((ms[4] + ms[8]) * 1e-3) / 1e12
            obj["prefill"] = {"achieved": round(tf_p, 1), "frac": round(tf_p / MFMA_PEAK_TF, 4), "launches": int(cnt[4]),
                              "kernel_ms_per_decision": round(ms[4] + ms[8], 3), "splitk_reduce_ms": round(ms[8], 3), "splitk_reduce_launches": int(cnt[8]),
                              "gemm_kernels_only_frac": round(work[4] / (ms[4] * 1e-3) / 1e12 / MFMA_PEAK_TF, 4)}
        if cnt[1] > 0 and ms[1] > 0:
            tf_v = work[1] / ((ms[1] + ms[6]) * 1e-3) / 1e12
            obj["vit"] = {"achieved": round(tf_v, 1), "frac": round(tf_v / MFMA_PEAK_TF, 4), "launches": int(cnt[1]),
                          "kernel_ms_per_decision": round(ms[1] + ms[6], 3), "splitk_reduce_ms": round(ms[6], 3)}
        if any(o.get("frac", 0) > 1.0 for o in (obj, obj.get("prefill", {}), obj.get("vit", {}))):
            out["roofline_mfma"] = {"invalid": "a fraction > 1: refused"}
        else:
            out["roofline_mfma"] = obj
    if len(cnt) > 7 and cnt[7] > 0 and ms[7] > 0:
        # config 5: the decoder's projections on the MX-scaled fp8 matrix instruction -- priced against the 5 PFLOP/s fp8 peak
        tf8 = work[7] / ((ms[7] + ms[9]) * 1e-3) / 1e12     # with the split-K reductions behind the fp8 GEMMs (class 9)
        obj = {"bound": "mfma", "kernel": "gemm_tiled_v3_f8 / gemm_tiled_pc_f8 (v_mfma_scale_f32_16x16x128_f8f6f4: e4m3 activations per row x e4m3 weights per channel; the decoder's "
                                          "projections in every pass with more than 64 rows)",
               "achieved": round(tf8, 1), "peak": FP8_PEAK_TF, "unit": "TFLOP/s", "frac": round(tf8 / FP8_PEAK_TF, 4), "traffic": None,
               "launches": int(cnt[7]), "avg_launch_us": round(1e3 * ms[7] / cnt[7], 2), "kernel_ms_per_decision": round(ms[7] + ms[9], 3),
               "splitk_reduce_ms": round(ms[9], 3), "gemm_kernels_only_frac": round(work[7] / (ms[7] * 1e-3) / 1e12 / FP8_PEAK_TF, 4), "flop_per_decision": work[7]}
        guard("roofline_fp8_mfma", obj)
        if "roofline" not in out and "frac" in out.get("roofline_fp8_mfma", {}):
            out["roofline"] = dict(out["roofline_fp8_mfma"])
    if "roofline" not in out and isinstance(out.get("roofline_mfma"), dict) and "frac" in out["roofline_mfma"]:
        # no weight-streaming launch of >= 16 MB in this configuration (M > 64 decode rows, e.g. config 5: N = 512): the dominant
        # kernel class is the tiled GEMM, bounded by the matrix pipes
        m = out["roofline_mfma"]
        out["roofline"] = {"bound": "mfma", "kernel": m["kernel"], "achieved": m["achieved"], "peak": m["peak"], "unit": m["unit"], "frac": m["frac"],
                           "traffic": None, "launches": m["launches"], "kernel_ms_per_decision": m["kernel_ms_per_decision"]}
    if cnt[3] > 0:
        out["small_streaming_gemms"] = {"kernel": "weight-streaming launches with < 16 MB of weights (verifier text tower etc.): latency-bound",
                                        "launches": int(cnt[3]), "kernel_ms_per_decision": round(ms[3], 3)}
    if cnt[2] > 0:
        out["attention_kernels"] = {"launches": int(cnt[2]), "kernel_ms_per_decision": round(ms[2], 3)}
    floor_ms = 1e3 * (work[0] / (HBM_PEAK_GBS * 1e9) + (work[1] + work[4]) / (MFMA_PEAK_TF * 1e12) + (work[7] if len(work) > 7 else 0.0) / (FP8_PEAK_TF * 1e12))
    if floor_ms > 0 and ms_per_step > 0:
        e2e = floor_ms / ms_per_step
        out["end_to_end"] = ({"floor_ms": round(floor_ms, 3), "measured_ms": round(ms_per_step, 3), "frac": round(e2e, 4),
                              "floor": "decode weight bytes / 8 TB/s + bf16 tiled-GEMM FLOPs / 2.5 PFLOP/s + fp8 tiled-GEMM FLOPs / 5 PFLOP/s (attention, norms, heads: 0)"}
                             if e2e <= 1.0 else {"invalid": f"frac {e2e:.3f} > 1: refused"})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="tiny config (plumbing check, not a valid bench line)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--flat-weights", action="store_true", help="the flat i.i.d. N(0, 0.02) checkpoint of rounds 1-4 instead of the one with decision margins (synth.openvla_state(peaked=True))")
    ap.add_argument("--no-cpu-batched", action="store_true", help="cpu_baseline: skip the batched N-row decision (minutes of CPU), keep the per-candidate figure")
    ap.add_argument("--no-profile", action="store_true", help="skip the profiled decision (plumbing tests)")
    ap.add_argument("--backend", default="nccl", help="nccl (= RCCL) for real runs; gloo only to test the N>1 plumbing")
    ap.add_argument("--share-gpu", action="store_true", help="plumbing test: every rank uses cuda:0")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--config", type=int, default=0, choices=[0, 3], help="3 = BASELINE config 3: one prompt group of 32 samples per GPU (N = 256 at 8 GPUs)")
    ap.add_argument("--samples", type=int, default=N_SAMPLES, help="samples per prompt (4 = headline N=32; 2 = config 2, N=16)")
    ap.add_argument("--cams", type=int, default=1, help="cameras (2 = config 4)")
    ap.add_argument("--members", type=int, default=3, help="verifier ensemble members (2 = config 4)")
    ap.add_argument("--no-agreement", action="store_true", help="fp8: skip the comparison run through a bf16 pipeline")
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16", help="fp8 = e4m3 decoder + lm_head weights (config 5)")
    ap.add_argument("--own-kv", choices=["auto", "none", "bf16", "fp8"], default="auto",
                    help="own-token KV cache of the decode passes: auto = head-major (e4m3 with --dtype fp8) above 64 candidates per GPU, legacy below")
    ap.add_argument("--horizon", type=int, default=1, help="action-chunk horizon: 7 x horizon action tokens per candidate (config 5: 8)")
    ap.add_argument("--check-out", default=None, help="write this rank's selection (winner index / tokens) as JSON (plumbing tests)")
    ap.add_argument("--profile", choices=["openvla", "pi0"], default="openvla",
                    help="pi0 = profile P1 (what the reference ships: pi0 sampler B = 40 + verifier), one GPU; the default is the BASELINE.json metric (OpenVLA-7B shapes)")
    ap.add_argument("--cpu-batch", type=int, default=40, help="--profile pi0: rows of the CPU-baseline decision (40 = as the reference executes it)")
    ap.add_argument("--full", action="store_true",
                    help="everything besides the headline: the profiled decision (roofline objects), the fp8-vs-bf16 comparison and the CPU baseline "
                         "with its agreement check (each still switched off by its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed decision returned as DIR/<name>.npy (rank 0)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if a.profile == "pi0":
        if a.gpus != 1:
            raise SystemExit("--profile pi0 is a one-GPU line")
        return main_pi0(a)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start one rank per GPU as CHILD processes (torch.distributed.run) before
        # anything here touches the GPU, and leave with their exit code (never exec from a process that may have initialised HIP)
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if a.gpus != world and "WORLD_SIZE" in os.environ and a.gpus != 1:
        raise SystemExit(f"--gpus {a.gpus} but the launcher started {world} rank(s)")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: bench.py measures the HIP path only (no CPU fallback)"}))
        sys.exit(2)
    if a.share_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device(f"cuda:{local}")
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(a.backend, rank=rank, world_size=world)
    strong = a.scaling == "strong" and world > 1 and a.config != 3
    if strong and world > N_PROMPTS:
        raise SystemExit(f"--scaling strong shards the {N_PROMPTS} prompt groups: at most {N_PROMPTS} ranks")
    if a.config == 3:       # W prompt groups x 32 samples, rank r owns group r
        a.samples = 32
        n_prompts_global = world
    else:                   # strong: the headline's 8 groups shared out; weak: 8 DISTINCT groups per rank (8 W in total)
        n_prompts_global = N_PROMPTS if strong else N_PROMPTS * world
    prompt_ids = list(range(rank, n_prompts_global, world))
    pipe = Pipeline(dev, small=a.small, n_prompts=n_prompts_global, n_samples=a.samples, n_cams=a.cams, members=a.members,
                    prompt_ids=prompt_ids, weight_dtype=a.dtype, horizon=a.horizon, own_kv=None if a.own_kv == "none" else a.own_kv, peaked=not a.flat_weights)

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()

    cpu_gather = a.backend != "nccl"
    for _ in range(a.warmup):
        pipe.decision(world, rank, cpu_gather)
    sync()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        last = pipe.decision(world, rank, cpu_gather)
    sync()
    dt = time.perf_counter() - t0
    from cover_vla_amd import ops as _ops
    if world > 1:
        t = torch.tensor([dt], device=dev if a.backend == "nccl" else "cpu")
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t[0])
    if a.dump_outputs and rank == 0:
        gi, toks, sel = last
        arrays = {"winner_index": [gi], "tokens": toks, "scores": pipe.last_scores}
        if sel is not None:   # world > 1: what every rank receives from the all-gather (rank 0's own tokens above)
            arrays.update(scores=sel["scores"], winner_tokens=sel["winner_payload"], group_tokens=sel["group_payload"])
        dump_outputs(a.dump_outputs, arrays)
    if a.check_out:
        gi, toks, sel = last
        rec = {"rank": rank, "global_idx": int(gi), "local_tokens": toks.cpu().tolist(), "prompt_ids": pipe.prompt_ids}
        if sel is not None:
            rec.update(winner_tokens=sel["winner_payload"].cpu().tolist(), group_tokens=sel["group_payload"].cpu().tolist(),
                       scores=[float(x) for x in sel["scores"].cpu()])
        with open(f"{a.check_out}.rank{rank}.json", "w") as f:
            json.dump(rec, f)

    n_local = len(pipe.prompt_ids) * a.samples
    n_total = n_prompts_global * a.samples
    ms_per_step = 1000.0 * dt / a.steps
    headline = (a.samples == N_SAMPLES and a.cams == 1 and a.members == 3 and not a.small and a.dtype == "bf16" and a.horizon == 1 and a.config == 0)
    metric = BASE_METRIC
    if world > 1 and not strong:
        metric += f" [weak scaling: N=32 per GPU = 8 distinct prompt groups x 4 samples per rank, N={n_total} in total at {world} GPUs]"
    if not headline:
        metric = (f"candidate actions scored/sec (whole node), OpenVLA-7B N={n_total}, 224^2 RGB x {a.cams} camera(s), verifier ensemble={a.members}, "
                  f"{a.dtype} weights, action-chunk horizon {a.horizon}")
    out = {
        "metric": metric,
        "value": round(n_total * a.steps / dt, 3), "unit": "candidates/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
        "dtype": "bf16" if a.dtype == "bf16" else ("fp8 (e4m3 decoder + lm_head weights with per-channel 2^e scales; passes with more than 64 rows run on the MX-scaled fp8 "
                                                   "matrix instruction with per-row e4m3 activations; own-token KV cache " + ("e4m3 with per-row scales" if pipe.own_kv == "fp8" else "bf16") +
                                                   "; bf16 vision towers, shared-prefix / text KV)"),
        "data": "synthetic",
        "config": {"workload": ("SMALL-PLUMBING-CONFIG (invalid as a bench line)" if a.small else
                                f"OpenVLA-7B (DINOv2-L+SigLIP-So400m+Llama-2-7B) N={n_local} = {len(pipe.prompt_ids)} prompts x {a.samples} samples per GPU, "
                                f"{7 * a.horizon} action tokens, {a.cams} 224x224 RGB frame(s); CoVer verifier SigLIP2-L/16-384 + {a.members}-member ensemble; "
                                "random-init weights" + (" with decision margins (depth-scaled residual projections, unit-scale embeddings, log-normal gains on the action rows of the head: synth.openvla_state(peaked=True))" if pipe.peaked else " (flat i.i.d.)")),
                   "candidates_total": n_total, "candidates_per_gpu": n_local, "prompts_per_gpu": len(pipe.prompt_ids),
                   "parallelism": f"candidate-sharded x{world} ({'strong' if strong else 'weak'})", "own_kv": pipe.own_kv or "legacy", "lib_sha16": lib_hash()},
    }
    if a.full and not a.no_profile:
        # ---- rooflines: kernel start/stop stamps of every GEMM / attention launch of one extra (serialised) decision
        ms, cnt, work = profile_decision(pipe, world, rank, cpu_gather)
        out.update(roofline_objects(ms, cnt, work, ms_per_step, out["config"]["lib_sha16"]))
        try:   # context for roofline_mfma (never its denominator): the clock the prefill tiles really run at, read inside the kernel
            pr = _ops.gemm_probe()
            if isinstance(out.get("roofline_mfma"), dict) and pr["k_tiles"] > 0:
                out["roofline_mfma"]["in_kernel_clock"] = {
                    "ghz": round(pr["clock_ghz"], 3), "cycles_per_k_tile": round(pr["cycles_per_k_tile"], 1), "k_tiles": pr["k_tiles"],
                    "prologue_us": round(pr["prologue_us"], 2), "loop_us": round(pr["loop_us"], 2), "epilogue_us": round(pr["epilogue_us"], 2),
                    "kernel": "last self-loading tiled GEMM launch of the profiled decision (gemm_v3.hip, workgroup 0: the prefill pass's last down projection, 224 x 128 "
                              "tile): shader cycle counter over the 100 MHz wall clock across its k-loop",
                    "note": "context only: the fractions above stay priced against 2.5 PFLOP/s = the matrix peak at 2.4 GHz; under MFMA + LDS + HBM load the chip "
                            "sustains the clock reported here (power limit), so the same kernel time is a larger share of the peak actually available"}
        except Exception as e:   # noqa: BLE001 -- a measurement hook must never take the bench line down
            out.setdefault("notes", []).append(f"in-kernel clock probe unavailable: {e}")
    if a.full and a.dtype == "fp8" and world == 1 and not a.no_agreement:
        out["fp8_vs_bf16"] = fp8_agreement(pipe, dev, a, n_prompts_global, prompt_ids)
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline and not a.small:
        out["cpu_baseline"] = cpu_baseline(pipe, batched=not a.no_cpu_batched, free=(last[0], last[1]))
        ag = out["cpu_baseline"].get("agreement")
        if ag is not None and ag["decided"] > 0 and ag["agree_on_decided"] < 1.0:
            # a data-decided pick that differs from the oracle's is a wrong result, not a slow one: no bench line
            print(json.dumps({"error": "HIP path disagrees with the CPU oracle on a data-decided pick: bench line refused", "agreement": ag}), flush=True)
            sys.exit(3)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
