"""Gaussian proposal augmentation, timed: (1) the median launch time of cover_augment_tokens / cover_augment_actions at two shapes and
of cover_proposal_prior_tokens / cover_proposal_prior_actions over their output (G = 8 groups of S = 64 rows, 4 of them fitted),
(2) one OpenVLA + CoVer decision with P = 8 prompts, n = 4 policy samples and K = 60 augmented candidates per prompt (512 verifier
candidates) beside bench.py's N = 32 decision (the same Pipeline object, the same process, decisions of the two kinds interleaved).
Reuses bench.py's pipeline classes; bench.py itself is untouched. Usage: python tools/augment_timing.py [--launch-only] [--small] [--steps 20] [--warmup 3]"""
import argparse
import concurrent.futures
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from cover_vla_amd import host, ops


def launch_times(dev, reps=30, per_rep=20):
    """hipEvent pairs around per_rep back-to-back launches, the median over reps, per launch, in microseconds."""
    bins = np.linspace(-1, 1, 256)
    centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=dev)
    out = {}
    for G, n, K, h in ((8, 4, 60, 1), (8, 4, 60, 8)):
        g = torch.Generator().manual_seed(0)
        tok = (32000 - 1 - torch.randint(0, 255, (G * n, 7 * h), generator=g)).to(dev)
        act = (torch.rand(G * n, h, 7, generator=g) * 2 - 1).to(dev)
        z = host.augmentation_normals(G, K, h, seed=1).to(dev)
        o_tok = torch.empty(G * (n + K), 7 * h, dtype=torch.int64, device=dev)
        o_act = torch.empty(G * (n + K), h, 7, dtype=torch.float32, device=dev)
        S = n + K
        ls = torch.from_numpy(host.vote_log_shares(n, 1.0)).to(dev)
        o_pt, o_pa = torch.empty(G * S, device=dev), torch.empty(G * S, device=dev)
        forms = {"tokens": lambda: ops.augment_tokens(tok, n, K, z, centers, 32000, steps=h, out=o_tok),
                 "actions": lambda: ops.augment_actions(act, n, K, z, out=o_act),
                 # the prior of the rows the two launches above left in o_tok / o_act (the warm-up fills them before these are timed)
                 "prior_tokens": lambda: ops.proposal_prior_tokens(o_tok, S, n, centers, 32000, steps=h, sigma=1.0, sd_floor=1e-3, log_share=ls,
                                                                   out=o_pt),
                 "prior_actions": lambda: ops.proposal_prior_actions(o_act, S, n, sigma=1.0, sd_floor=1e-3, log_share=ls, out=o_pa)}
        for name, fn in forms.items():
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            t, ms = ops.Timer(), []
            for _ in range(reps):
                t.start()
                for _ in range(per_rep):
                    fn()
                ms.append(t.stop() / per_rep)
            out[f"{name}_{G}x{n}x{K}x{h}_us"] = round(float(np.median(ms)) * 1e3, 2)
            out[f"{name}_{G}x{n}x{K}x{h}_us_min_max"] = [round(min(ms) * 1e3, 2), round(max(ms) * 1e3, 2)]
    return out


def decision_augmented(pipe, K, z):
    """Pipeline.decision's default schedule (verifier towers as one graph from a second host thread) with K augmented candidates per
    prompt between the sampler and the history builder."""
    i, n = pipe.inp, pipe.n_samples
    main = torch.cuda.current_stream()
    if pipe.side is None:
        pipe.side = torch.cuda.Stream(device=pipe.dev)
    if pipe.pool is None:
        pipe.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    ev = torch.cuda.Event()
    ev.record(main)

    def threaded():
        torch.cuda.set_device(pipe.dev)
        pipe.side.wait_event(ev)
        with torch.cuda.stream(pipe.side):
            return pipe.ver.shared_embeddings_graph(i["img384"], i["text"])

    fut = pipe.pool.submit(threaded)
    tokens, _ = pipe.policy.sample(i["frame"], i["toks"], i["lens"], n, i["u"], 1.0)
    its = fut.result()
    aug = pipe.policy.augment(tokens, n, K, z)
    hb, pad = ops.tokens_to_histories(aug, pipe.c["tok_vocab"], pipe.centers, pipe.past_dev)
    main.wait_stream(pipe.side)
    r = pipe.ver.score_histories(its, hb, n + K, pad=pad)
    return int(r["result"][0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="tiny config (plumbing check, not a measurement)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--augmented", type=int, default=60, help="K per prompt (60: 8 x (4 + 60) = 512 verifier candidates)")
    ap.add_argument("--launch-only", action="store_true", help="part (1) only: no pipeline is built")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {"launch": launch_times(dev)}
    if a.launch_only:
        print(json.dumps(res))
        return
    pipe = bench.Pipeline(dev, small=a.small)
    P, n, K = len(pipe.prompt_ids), pipe.n_samples, a.augmented
    z = host.augmentation_normals(P, K, 1, seed=0).to(dev)
    for _ in range(a.warmup):
        pipe.decision()
        decision_augmented(pipe, K, z)
    torch.cuda.synchronize()
    base, aug = [], []
    for _ in range(a.steps):                       # interleaved: both kinds see the same clocks and the same box
        for ts, fn in ((base, pipe.decision), (aug, lambda: decision_augmented(pipe, K, z))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                   # ends with the winner index on the host
            ts.append((time.perf_counter() - t0) * 1e3)
    res["decision"] = {"P": P, "n": n, "K": K, "verifier_candidates": P * (n + K), "steps": a.steps, "small": a.small,
                       "policy_only_N%d_ms_median" % (P * n): round(float(np.median(base)), 3),
                       "policy_only_N%d_ms_min_max" % (P * n): [round(min(base), 3), round(max(base), 3)],
                       "augmented_ms_median": round(float(np.median(aug)), 3), "augmented_ms_min_max": [round(min(aug), 3), round(max(aug), 3)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
