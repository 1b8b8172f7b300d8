"""Diverse candidate subsets, timed: the median time per graph replay of the cover_diverse_subset_tokens launch at (G, S, m, h) =
(8, 64, 16, 1), (8, 37, 8, 50), (1, 512, 64, 8) and (1, 4096, 256, 8) (quality given, weight 0.5, cover_dist 0, every output asked
for) and, beside each, what the launch buys: the time of EfficientEnsembleMerged.score_histories (the existing code path: trajectory
encoder, fusion, scoring, grouped arg-max; 2 synthetic members) on G * S rows and on G * m rows. break_even_keep_fraction is the m / S
below which pruning pays for itself if the verifier's time were linear in its rows between the two measured points:
1 - diverse / (score(G * S) - score(G * m)) * (1 - m / S), clamped to [0, 1]; 0 means the launch costs more than the rows it saves.
The launch is captured once; a replay is timed with hipEvent pairs around per_rep back-to-back replays. score_histories allocates, so it
is timed eagerly, warm, with the same event pairs.
Usage: python tools/diverse_timing.py [--reps 30]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cover_vla_amd import graphs, host, ops, synth

SHAPES = ((8, 64, 16, 1), (8, 37, 8, 50), (1, 512, 64, 8), (1, 4096, 256, 8))
DIM_SCALE = [1.0, 1.0, 1.0, 0.5, 0.5, 0.5]
TOK_VOCAB = 32000


def _median_us(fn, reps, per_rep):
    t, ms = ops.Timer(), []
    for _ in range(reps):
        t.start()
        for _ in range(per_rep):
            fn()
        ms.append(t.stop() / per_rep)
    return round(float(np.median(ms)) * 1e3, 2), [round(min(ms) * 1e3, 2), round(max(ms) * 1e3, 2)]


def times(dev, reps=30, per_rep=10):
    """-> {shape: {diverse_us, score_all_us, score_kept_us (medians, microseconds), their _min_max, count, break_even_keep_fraction}}."""
    from cover_vla_amd.verifier import EfficientEnsembleMerged
    bins = np.linspace(-1, 1, 256)
    centers = torch.tensor((bins[:-1] + bins[1:]) / 2.0, dtype=torch.float32, device=dev)
    ver = EfficientEnsembleMerged(synth.verifier_checkpoint(2, seed=9), device=str(dev))
    pf, tf, _ = synth.verifier_inputs(1, seed=9)
    its = ver.image_text_embeddings(pf.to(dev), tf.to(dev))
    past = torch.from_numpy((np.random.default_rng(0).normal(size=(6, 7)) * 0.02).astype(np.float32)).to(dev)
    out = {}
    for G, S, m, h in SHAPES:
        N = G * S
        g = torch.Generator().manual_seed(0)
        tok = (TOK_VOCAB - 1 - torch.randint(0, 255, (N, 7 * h), generator=g)).to(dev)
        quality = torch.randn(N, generator=g).to(dev)
        div = host.Diversity(m, 0.5, DIM_SCALE, 0.9, 0.25, cover_dist=0.0)
        kw = div.kwargs(dev, h)
        launch = lambda: ops.diverse_subset_tokens(tok, S, m, centers, TOK_VOCAB, steps=h, quality=quality, **kw)
        for _ in range(3):
            sub = launch()
        torch.cuda.synchronize()
        pg = graphs.PooledGraph(launch, dev)                               # the wrapper allocates its outputs: call 1 eager, call 2 captures
        pg()
        torch.cuda.synchronize()
        held = pg()
        gr = pg.graph
        for _ in range(10):
            gr.launch()
        torch.cuda.synchronize()
        assert torch.equal(held.picked, sub.picked)
        key = f"{G}x{S}x{m}x{h}"
        out[key] = {"count": sub.count.cpu().tolist()}
        out[key]["diverse_us"], out[key]["diverse_us_min_max"] = _median_us(gr.launch, reps, per_rep)
        for name, rows, gs in (("score_all", tok, S), ("score_kept", sub.rows, m)):
            try:
                hb, pad = ops.tokens_to_histories(rows[:, :7].contiguous(), TOK_VOCAB, centers, past)
                score = lambda: ver.score_histories(its, hb, gs, pad=pad)
                for _ in range(3):
                    score()
                torch.cuda.synchronize()
                out[key][f"{name}_us"], out[key][f"{name}_us_min_max"] = _median_us(score, max(reps // 3, 5), 3)
            except Exception as e:                                         # a row count the verifier does not take: say so
                out[key][f"{name}_us"], out[key][f"{name}_error"] = None, f"{type(e).__name__}: {e}"[:200]
        a, k = out[key].get("score_all_us"), out[key].get("score_kept_us")
        if a is not None and k is not None and a > k:
            out[key]["break_even_keep_fraction"] = round(min(1.0, max(0.0, 1.0 - out[key]["diverse_us"] / (a - k) * (1.0 - m / S))), 3)
        else:
            out[key]["break_even_keep_fraction"] = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(json.dumps({"diverse": times(dev, reps=a.reps)}))


if __name__ == "__main__":
    main()
