"""Verifier-guided refinement, timed: the median launch time of cover_refine_tokens / cover_refine_actions at (G, S, m, K, h) =
(8, 64, 8, 56, 1) and (8, 512, 16, 496, 4) and, beside each, of cover_augment_tokens / cover_augment_actions at the same G, K and h with
n = m, in the same process (the forms of one shape interleaved rep by rep, so each pair sees the same clocks). What refine adds to augment
is the sort (21 or 45 compare-exchange stages at these two shapes) and the gather. Usage: python tools/refine_timing.py [--reps 30]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cover_vla_amd import host, ops

SHAPES = ((8, 64, 8, 56, 1), (8, 512, 16, 496, 4))


def launch_times(dev, reps=30, per_rep=20):
    """hipEvent pairs around per_rep back-to-back launches, the median over reps, per launch, in microseconds."""
    bins = np.linspace(-1, 1, 256)
    centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=dev)
    out = {}
    for G, S, m, K, h in SHAPES:
        g = torch.Generator().manual_seed(0)
        tok = (32000 - 1 - torch.randint(0, 255, (G * S, 7 * h), generator=g)).to(dev)
        act = (torch.rand(G * S, h, 7, generator=g) * 2 - 1).to(dev)
        scores = torch.randn(G * S, generator=g).to(dev)
        z = host.augmentation_normals(G, K, h, seed=1).to(dev)
        o_tok = torch.empty(G * (m + K), 7 * h, dtype=torch.int64, device=dev)
        o_act = torch.empty(G * (m + K), h, 7, dtype=torch.float32, device=dev)
        a_tok, a_act = tok[:G * m].contiguous(), act[:G * m].contiguous()       # augment's input: m rows per group
        forms = {"refine_tokens": lambda: ops.refine_tokens(tok, scores, S, m, K, z, centers, 32000, steps=h, out=o_tok),
                 "augment_tokens": lambda: ops.augment_tokens(a_tok, m, K, z, centers, 32000, steps=h, out=o_tok),
                 "refine_actions": lambda: ops.refine_actions(act, scores, S, m, K, z, out=o_act),
                 "augment_actions": lambda: ops.augment_actions(a_act, m, K, z, out=o_act)}
        for fn in forms.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        t, ms = ops.Timer(), {name: [] for name in forms}
        for _ in range(reps):
            for name, fn in forms.items():
                t.start()
                for _ in range(per_rep):
                    fn()
                ms[name].append(t.stop() / per_rep)
        n2 = 1 << max(1, (S - 1).bit_length())
        key = f"{G}x{S}x{m}x{K}x{h}"
        out[key] = {"sort_stages": n2.bit_length() * (n2.bit_length() - 1) // 2}
        for name, v in ms.items():
            out[key][f"{name}_us"] = round(float(np.median(v)) * 1e3, 2)
            out[key][f"{name}_us_min_max"] = [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(json.dumps({"launch": launch_times(dev, reps=a.reps)}))


if __name__ == "__main__":
    main()
