"""The chunk-coherence prior, timed: the median time per graph replay of the cover_coherence_prior_tokens launch at (G, S, R, h) =
(8, 4, 1, 4) (backward coherence: one committed chunk), (8, 64, 64, 8), (1, 512, 512, 8) and (1, 4096, 4096, 8) (forward contrast: as many
references as rows), hr = h, shift 0, one reference set per group and, beside each, of cover_score_select at the same N = G * S (2
members, dim 512, group_size S) and of cover_smooth_scores_tokens at the same (G, S, h). Each launch is captured once; a replay is timed
with hipEvent pairs around per_rep back-to-back replays, the launches of one shape interleaved rep by rep.
Usage: python tools/coherence_timing.py [--reps 30]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import graphs, host, ops

SHAPES = ((8, 4, 1, 4), (8, 64, 64, 8), (1, 512, 512, 8), (1, 4096, 4096, 8))
DIM_SCALE = [1.0, 1.0, 1.0, 0.5, 0.5, 0.5]


def replay_times(dev, reps=30, per_rep=20):
    """-> {shape: {name_us: the median over reps of the time per replay, name_us_min_max, pair_dims}}, microseconds."""
    bins = np.linspace(-1, 1, 256)
    centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=dev)
    scale = torch.tensor(DIM_SCALE, dtype=torch.float32, device=dev)
    out = {}
    for G, S, R, h in SHAPES:
        N = G * S
        g = torch.Generator().manual_seed(0)
        tok = (32000 - 1 - torch.randint(0, 255, (N, 7 * h), generator=g)).to(dev)
        ref = (torch.rand(G, R, h, 7, generator=g) * 2 - 1).to(dev)
        w = torch.cat([torch.full((G, R - R // 2), 1.0 / (R - R // 2)), torch.full((G, R // 2), -1.0 / max(R // 2, 1))], dim=1).to(dev)
        sw = torch.from_numpy(host.coherence_step_weights(h, 0.9)).to(dev)
        prior = torch.empty(N, dtype=torch.float32, device=dev)
        coherence = lambda: ops.coherence_prior_tokens(tok, S, ref, w, centers, 32000, steps=h, step_weight=sw, dim_scale=scale,
                                                       gripper_penalty=0.25, out=prior)
        scores = torch.randn(N, generator=g).to(dev)
        smoothed = torch.empty(N, dtype=torch.float32, device=dev)
        smooth = lambda: ops.smooth_scores_tokens(tok, scores, S, centers, 32000, steps=h, radius=0.5 * float(np.sqrt(h)), dim_scale=scale,
                                                  shrink=1.0, out=smoothed)
        its = torch.randn(2, 512, generator=g).to(dev)
        acts = torch.randn(2, N, 512, generator=g).to(dev)
        f32 = dict(dtype=torch.float32, device=dev)
        sel = [torch.empty(N, **f32), torch.empty(4, dtype=torch.int32, device=dev), torch.empty(2, **f32), torch.empty(512, **f32),
               torch.empty(N, 512, **f32)]                    # cover_score_select over caller-owned outputs: nothing allocates under capture
        sa = L.ScoreSelectArgs()
        sa.it, sa.act, sa.n_members, sa.N, sa.dim, sa.group_size = its.data_ptr(), acts.data_ptr(), 2, N, 512, S
        sa.scores_out, sa.result_out, sa.best_out, sa.fused_it_out, sa.fused_act_out = (t.data_ptr() for t in sel)
        select = lambda: L.check(L.lib().cover_score_select(C.byref(sa), torch.cuda.current_stream().cuda_stream), "score_select")
        forms = {}
        for name, fn in (("coherence_prior", coherence), ("score_select", select), ("smooth_scores", smooth)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            forms[name] = graphs.capture(fn, dev)[0]
        for gr in forms.values():
            for _ in range(10):
                gr.launch()
        torch.cuda.synchronize()
        t, ms = ops.Timer(), {name: [] for name in forms}
        for _ in range(reps):
            for name, gr in forms.items():
                t.start()
                for _ in range(per_rep):
                    gr.launch()
                ms[name].append(t.stop() / per_rep)
        key = f"{G}x{S}x{R}x{h}"
        out[key] = {"pair_dims": G * S * R * 6 * h}
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
    print(json.dumps({"replay": replay_times(dev, reps=a.reps)}))


if __name__ == "__main__":
    main()
