"""Cost of the filtered sampler at the pi0-FAST head's shape on one MI355X: ops.token_sample over 40 rows x 257 152 fp32 logits for the
five (temperature, top_k, top_p) settings of tests/sampling_ref.py, next to the greedy pick (token_argmax_wide_k) and the lm_head GEMM
of the same decode step (40 x 2048 bf16 times the 257 152 x 2048 tied embedding). Rows are shaped like a language model's (randn
plus 40 boosted columns); FLAT=1 adds i.i.d. Gaussian rows, where the top-p cut falls into the tail and the kernel takes one
pass over the row per digit. Every setting is timed three ways: the plain sampler, the scored sampler (out_logprob: the same launch with
one logarithm and one store per row more) and ops.token_logprob on the picks just made (the same passes without the pick).
    python tools/bench_token_sample.py                  event-timed microseconds per launch, one JSON line
    rocprofv3 --kernel-trace --stats -d D -o ts -- python tools/bench_token_sample.py
    python tools/bench_token_sample.py --from-db D/.../ts_results.db      per-setting averages from that trace (dispatch order)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = [(1.0, 0, 1.0), (1.0, 50, 1.0), (1.0, 0, 0.9), (0.7, 64, 0.95), (1.5, 8, 1.0)]
REPS = 20
ROWS, V, K = 40, 257152, 2048


def from_db(path):
    import sqlite3
    cur = sqlite3.connect(path).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)")]
    ncol = "name" if "name" in cols else "kernel_name"
    rows = cur.execute(f"select {ncol}, start, end from kernels order by start").fetchall()
    # dispatch order: per setting REPS plain (token_sample_k<false>), REPS scored (token_sample_k<true>), REPS token_logprob_k
    smp = [(e - s) / 1e3 for n, s, e in rows if "token_sample_k" in n or "token_logprob_k" in n]
    out = {}
    labels = [f"{tag}T={t} k={k} p={p}{col}" for tag in ("", "flat ") for t, k, p in SETTINGS for col in ("", " scored", " logprob")]
    for i in range(0, len(smp) - REPS + 1, REPS):
        grp = smp[i:i + REPS][2:]                                       # the first two launches of a setting warm it up
        out[labels[i // REPS]] = round(sum(grp) / len(grp), 2)
    for key in ("token_argmax_wide_k", "gemm"):
        d = [(e - s) / 1e3 for n, s, e in rows if key in n]
        if d:
            d = d[-(REPS - 2):]
            out[key + " (last launches)"] = round(sum(d) / len(d), 2)
    print(json.dumps({"us_per_launch_from_trace": out}))


def main():
    import torch
    from cover_vla_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(ROWS, V, generator=g)
    for r in range(ROWS):
        cols = torch.randperm(V, generator=g)[:40]
        x[r, cols] += 10.0 + 8.0 * torch.rand(40, generator=g)
    u = torch.rand(ROWS, generator=g).to(dev)
    inputs = [("", x.to(dev))]
    if os.environ.get("FLAT", "0") == "1":
        inputs.append(("flat ", (4 * torch.randn(ROWS, V, generator=g)).to(dev)))
    tok = torch.empty(ROWS, dtype=torch.int64, device=dev)
    lg = torch.empty(ROWS, dtype=torch.float32, device=dev)
    kept = torch.empty(ROWS, dtype=torch.int32, device=dev)
    lp = torch.empty(ROWS, dtype=torch.float32, device=dev)

    def timed(fn):
        for _ in range(2):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS - 2):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) / (REPS - 2) * 1e3, 2)

    res = {}
    for tag, xd in inputs:
        for t, k, p in SETTINGS:
            res[f"{tag}T={t} k={k} p={p}"] = timed(lambda: ops.token_sample(xd, 0, V, u, temperature=t, top_k=k, top_p=p, out_tok=tok,
                                                                              out_logit=lg, out_kept=kept))
            res[f"{tag}T={t} k={k} p={p} scored"] = timed(lambda: ops.token_sample(xd, 0, V, u, temperature=t, top_k=k, top_p=p, out_tok=tok,
                                                                                     out_logit=lg, out_kept=kept, out_logprob=lp))
            res[f"{tag}T={t} k={k} p={p} logprob"] = timed(lambda: ops.token_logprob(xd, 0, V, tok, temperature=t, top_k=k, top_p=p, out=lp,
                                                                                       out_kept=kept))
            res[f"{tag}T={t} k={k} p={p} median kept"] = int(kept.median())
    res["greedy token_select (token_argmax_wide_k)"] = timed(lambda: ops.token_select(inputs[0][1], 0, V, out_tok=tok, out_logit=lg))
    w = (0.02 * torch.randn(V, K, generator=g)).to(torch.bfloat16).to(dev)
    head = ops.pack_linear(w)
    del w
    h = torch.randn(ROWS, K, generator=g).to(torch.bfloat16).to(dev)
    logits = torch.empty(ROWS, V, dtype=torch.float32, device=dev)
    ws = ops.gemm_workspace(ROWS, V, K, dev)
    res["lm_head gemm 40 x 257152 x 2048"] = timed(lambda: ops.gemm(h, head, out=logits, ws=ws))
    print(json.dumps({"rows": ROWS, "width": V, "us_per_launch": res}))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--from-db":
        from_db(sys.argv[2])
    else:
        main()
