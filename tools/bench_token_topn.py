"""Cost of ops.token_topn next to ops.token_logprob on the same inputs on one MI355X (n = 8, top_k = 50, top_p = 0.9): 32 rows x 256
action bins (the OpenVLA head) and 64 rows x 257 152 columns (the pi0-FAST head), rows shaped like a language model's (randn plus 40
boosted columns). Event-timed with ops.Timer: per figure REPS launches after WARM warm-up launches, ROUNDS figures per call,
the two calls alternating. `GREEDY=1` adds the unfiltered wide row (temperature 1, what a greedy step reports).
    python tools/bench_token_topn.py          one JSON line, microseconds per launch (min - max of the rounds)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, REPS, ROUNDS, N = 5, 40, 4, 8


def main():
    import torch
    from cover_vla_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    timer = ops.Timer()

    def rows_like_lm(rows, ld, lo, hi):
        x = torch.randn(rows, ld, generator=g)
        for r in range(rows):
            cols = lo + torch.randperm(hi - lo, generator=g)[:40]
            x[r, cols] += 10.0 + 8.0 * torch.rand(40, generator=g)
        return x.to(dev)

    def timed(fn):
        for _ in range(WARM):
            fn()
        timer.start()
        for _ in range(REPS):
            fn()
        return timer.stop() / REPS * 1e3

    res = {}
    shapes = [("32 x 256 bins", 32, 32064, 31744, 32000, 1.0, 50, 0.9), ("64 x 257152", 64, 257152, 0, 257152, 1.0, 50, 0.9)]
    if os.environ.get("GREEDY", "0") == "1":
        shapes.append(("64 x 257152 unfiltered", 64, 257152, 0, 257152, 1.0, 0, 1.0))
    for name, rows, ld, lo, hi, t, k, p in shapes:
        x = rows_like_lm(rows, ld, lo, hi)
        tok = torch.empty(rows, N, dtype=torch.int64, device=dev)
        lp = torch.empty(rows, N, dtype=torch.float32, device=dev)
        ent = torch.empty(rows, dtype=torch.float32, device=dev)
        kept = torch.empty(rows, dtype=torch.int32, device=dev)
        one = torch.empty(rows, dtype=torch.float32, device=dev)
        ops.token_topn(x, lo, hi, N, temperature=t, top_k=k, top_p=p, out_tok=tok, out_logprob=lp, out_entropy=ent, out_kept=kept)
        best = tok[:, 0].contiguous()
        a, b = [], []
        for _ in range(ROUNDS):
            a.append(timed(lambda: ops.token_logprob(x, lo, hi, best, temperature=t, top_k=k, top_p=p, out=one, out_kept=kept)))
            b.append(timed(lambda: ops.token_topn(x, lo, hi, N, temperature=t, top_k=k, top_p=p, out_tok=tok, out_logprob=lp,
                                                  out_entropy=ent, out_kept=kept)))
        res[name] = {"token_logprob": [round(min(a), 2), round(max(a), 2)], "token_topn": [round(min(b), 2), round(max(b), 2)],
                     "median kept": int(kept.median())}
    print(json.dumps({"n": N, "launches_per_figure": REPS, "rounds": ROUNDS, "us_per_launch_min_max": res}))


if __name__ == "__main__":
    main()
