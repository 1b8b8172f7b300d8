"""Per-member verifier scores, timed: what turning member_kappa on adds to the tail of a decision. At N = 32 and N = 512 candidates
(M = 3 members, dim = 512) two launch sequences over static buffers are captured as graphs -- cover_score_select alone (the tail as it
is with the option off) and cover_score_select + cover_member_scores -- and replayed: hipEvent pairs around per_rep back-to-back
replays, the two sequences alternating inside every repetition so that both see the same clocks, the median over the repetitions, per
replay, in microseconds. No threshold: the option is off by default. Needs a GPU (there is no CPU path).
Usage: python tools/member_scores_timing.py [--reps 50] [--per-rep 200]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cover_vla_amd import _lib as L
from cover_vla_amd import graphs, ops


def _unit_rows(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1)


def sequences(dev, M, N, dim, gs, kappa):
    """-> (score_select alone, score_select + member_scores): two closures that launch on the current stream, over static buffers."""
    it, act = _unit_rows(M, dim, seed=1).to(dev), _unit_rows(M, N, dim, seed=2).to(dev)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    keep = dict(it=it, act=act, scores=torch.empty(N, **f32), result=torch.empty(4, **i32), best=torch.empty(2, **f32),
                fit=torch.empty(dim, **f32), fact=torch.empty(N, dim, **f32))
    s = L.ScoreSelectArgs()
    s.it, s.act, s.n_members, s.N, s.dim, s.group_size = it.data_ptr(), act.data_ptr(), M, N, dim, gs
    s.scores_out, s.result_out, s.best_out = keep["scores"].data_ptr(), keep["result"].data_ptr(), keep["best"].data_ptr()
    s.fused_it_out, s.fused_act_out = keep["fit"].data_ptr(), keep["fact"].data_ptr()
    outs = {"member_scores": torch.empty(M, N, **f32), "mean": torch.empty(N, **f32), "spread": torch.empty(N, **f32),
            "min": torch.empty(N, **f32), "min_member": torch.empty(N, **i32), "robust": torch.empty(N, **f32),
            "result": torch.empty(4, **i32), "best": torch.empty(2, **f32), "member_result": torch.empty(M, 4, **i32),
            "member_best": torch.empty(M, 2, **f32)}
    m = L.MemberScoresArgs()
    m.it, m.act, m.scores = it.data_ptr(), act.data_ptr(), keep["scores"].data_ptr()
    m.n_members, m.N, m.dim, m.group_size, m.kappa, m.mode = M, N, dim, gs, kappa, ops.MEMBER_MODES["lcb"]
    for k, t in outs.items():
        setattr(m, k + "_out", t.data_ptr())
    keep.update(outs=outs, s=s, m=m)

    def stream():
        return torch.cuda.current_stream().cuda_stream

    def alone():
        L.check(L.lib().cover_score_select(C.byref(s), stream()), "score_select")

    def both():
        alone()
        L.check(L.lib().cover_member_scores(C.byref(m), stream()), "member_scores")

    return alone, both, keep


def measure(dev, N, gs, reps, per_rep, M=3, dim=512, kappa=0.5):
    alone, both, keep = sequences(dev, M, N, dim, gs, kappa)
    both()                                                           # eager once: loads the code objects
    torch.cuda.synchronize()
    g_alone, _ = graphs.capture(alone, dev)
    g_both, _ = graphs.capture(both, dev)
    for g in (g_alone, g_both):
        for _ in range(per_rep):
            g.launch()
    torch.cuda.synchronize()
    t, us = ops.Timer(), {"alone": [], "both": []}
    for _ in range(reps):
        for name, g in (("alone", g_alone), ("both", g_both)):
            t.start()
            for _ in range(per_rep):
                g.launch()
            us[name].append(t.stop() / per_rep * 1e3)
    a, b = float(np.median(us["alone"])), float(np.median(us["both"]))
    return {"M": M, "N": N, "dim": dim, "group_size": gs, "reps": reps, "per_rep": per_rep,
            "score_select_us": round(a, 2), "score_select_us_min_max": [round(min(us["alone"]), 2), round(max(us["alone"]), 2)],
            "score_select_plus_member_scores_us": round(b, 2),
            "score_select_plus_member_scores_us_min_max": [round(min(us["both"]), 2), round(max(us["both"]), 2)],
            "added_us": round(b - a, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--per-rep", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("member_scores_timing: needs a GPU, nothing was measured")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(json.dumps({"member_scores": [measure(dev, N, gs, a.reps, a.per_rep) for N, gs in ((32, 4), (512, 64))]}))


if __name__ == "__main__":
    main()
