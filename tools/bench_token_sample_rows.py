"""Cost of one ops.token_sample_rows launch next to the scalar launches it stands for, on one MI355X.
  uniform parameters (0.7, 64, 0.95) on every row: token_sample_rows against cover_token_sample_scored on the same rows, 32 x 257 147
  columns (tests/sample_rows_ref's wide range) and 32 x 256 action bins;
  the mixed ladder of tests/sample_rows_ref.LADDER on 32 rows: ONE token_sample_rows launch against the 7 scalar launches (one per
  sampled parameter set, each over its 4 rows) it replaces -- the greedy rows' token_select + token_logprob are left out of the 7.
Every launch is event-timed on its own (ops.Timer) as a bare C call with a prepared argument struct (a Python wrapper's time between the
two events would count against it), the contenders alternate, and the figure is the median of LAUNCHES launches with the 10th and 90th
percentile next to it. PARENT_LIB=<path of another build's libcover_hip.so>: the scalar side of the first comparison
is that library's cover_token_sample_scored (an A/B against an older build); unset: this build's.
    python tools/bench_token_sample_rows.py          one JSON line, microseconds per launch [median, p10, p90]"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, LAUNCHES = 10, 60


def main():
    import numpy as np
    import torch
    from cover_vla_amd import _lib as L, ops
    from tests import sample_rows_ref as RR
    from tests import sampling_ref as R
    dev = torch.device("cuda:0")
    timer = ops.Timer()
    parent = None
    if os.environ.get("PARENT_LIB"):
        parent = C.CDLL(os.environ["PARENT_LIB"])
        parent.cover_token_sample_scored.restype = C.c_int
        parent.cover_token_sample_scored.argtypes = [C.POINTER(L.TokenSampleScoredArgs), C.c_void_p]

    st = torch.cuda.current_stream().cuda_stream
    keep = []                                                               # the argument structs outlive their closures' calls

    def scored(x, lo, hi, u, T, k, p, tok, lg, kept, lp, lib=None):
        """cover_token_sample_scored of the parent build (or of this one) as a bare C call: no wrapper time between the two events."""
        a = L.TokenSampleScoredArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi = x.data_ptr(), x.stride(0), x.shape[0], lo, hi
        a.uniform, a.temperature, a.top_k, a.top_p = u.data_ptr(), T, k, p
        a.token_out, a.logit_out, a.kept_out, a.logprob_out = tok.data_ptr(), lg.data_ptr(), kept.data_ptr(), lp.data_ptr()
        keep.append(a)
        fn = (lib or L.lib()).cover_token_sample_scored

        def call():
            assert fn(C.byref(a), st) == 0
        return call

    def rows_call(x, lo, hi, u, Td, kd, pd, tok, lg, kept, lp):
        """cover_token_sample_rows as a bare C call."""
        a = L.TokenSampleRowsArgs()
        a.logits, a.ld, a.rows, a.lo, a.hi = x.data_ptr(), x.stride(0), x.shape[0], lo, hi
        a.uniform, a.temperature, a.top_k, a.top_p = u.data_ptr(), Td.data_ptr(), kd.data_ptr(), pd.data_ptr()
        a.token_out, a.logit_out, a.kept_out, a.logprob_out = tok.data_ptr(), lg.data_ptr(), kept.data_ptr(), lp.data_ptr()
        keep.append(a)
        fn = L.lib().cover_token_sample_rows

        def call():
            assert fn(C.byref(a), st) == 0
        return call

    def race(fns):
        """Alternating, one event pair per call of a contender -> [median, p10, p90] in microseconds each."""
        for _ in range(WARM):
            for fn in fns:
                fn()
        t = [[] for _ in fns]
        for _ in range(LAUNCHES):
            for i, fn in enumerate(fns):
                timer.start()
                fn()
                t[i].append(timer.stop() * 1e3)
        return [[round(float(np.percentile(v, q)), 2) for q in (50, 10, 90)] for v in t]

    def outs(rows):
        return (torch.empty(rows, dtype=torch.int64, device=dev), torch.empty(rows, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                torch.empty(rows, device=dev))

    res = {}
    rows = 32
    T, k, p = 0.7, 64, 0.95
    for name, (ld, lo, hi, _, seed) in (("wide x 32", RR.CASES["wide"]), ("narrow x 32", RR.CASES["narrow"])):
        x, u = R.lm_like_rows(seed, rows, ld, lo, hi)
        x, u = x.to(dev), u.to(dev)
        Td, kd, pd = torch.full((rows,), T, device=dev), torch.full((rows,), k, dtype=torch.int32, device=dev), torch.full((rows,), p, device=dev)
        o_a, o_b = outs(rows), outs(rows)
        a = scored(x, lo, hi, u, T, k, p, *o_a, lib=parent)
        b = rows_call(x, lo, hi, u, Td, kd, pd, *o_b)
        ta, tb = race([a, b])
        torch.cuda.synchronize()
        assert all(torch.equal(i, j) for i, j in zip(o_a, o_b))
        res[name] = {"token_sample_scored" + (" (PARENT_LIB)" if parent else ""): ta, "token_sample_rows": tb}
        if name.startswith("wide"):                                         # the mixed ladder on the same rows
            Tl, kl, pl = (torch.from_numpy(v).to(dev) for v in RR.ladder_params(rows))
            o_m = outs(rows)
            mixed = rows_call(x, lo, hi, u, Tl, kl, pl, *o_m)
            subs = []
            for j, (Tj, kj, pj) in enumerate(RR.LADDER):
                if Tj == 0:
                    continue
                idx = torch.arange(j, rows, len(RR.LADDER), device=dev)
                xs, us, o_s = x[idx].contiguous(), u[idx].contiguous(), outs(idx.numel())
                keep.extend((xs, us, o_s))
                subs.append(scored(xs, lo, hi, us, Tj, kj, pj, *o_s))                 # more than 4096 columns: token_sample_k for every set

            def seven():
                for fn in subs:
                    fn()
            tm, ts = race([mixed, seven])
            res["mixed ladder, wide x 32"] = {"one token_sample_rows launch": tm, "7 scalar token_sample_scored launches (4 rows each, rows gathered beforehand)": ts}
    print(json.dumps({"launches_per_figure": LAUNCHES, "us_per_launch_median_p10_p90": res}))


if __name__ == "__main__":
    main()
