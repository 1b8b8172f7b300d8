"""The pi0-FAST de-tokeniser, timed: the median time per graph replay of the cover_fast_decode launch at B = 32 and B = 512 rows of
L = 256 generated ids, H = 50, D = 32 (a synthetic BPE of 1024 pieces of 1..12 symbols, so that a row fills most of its 1600
coefficients), the same launch as an eager ops.fast_decode call ending in a synchronise, and beside them the host path on the same
tokens: PI0FASTPolicy.extract_actions(tokens.cpu(), H, D) moved back to the device, copies included (a host clock around work that ends
in a synchronise). The launch is captured once; a replay is timed with hipEvent pairs around per_rep back-to-back replays.
Usage: python tools/fast_decode_timing.py [--reps 30] [--host-reps 5]"""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cover_vla_amd import graphs, ops, synth
from cover_vla_amd.pi0fast import PI0FASTConfig, PI0FASTPolicy

BATCHES = (32, 512)
L, H, D = 256, 50, 32
VOCAB, FAST_VOCAB, SKIP = 2048, 1024, 128
MIN_TOKEN, SCALE = -300, 10.0


def make_policy(dev):
    """A policy over the character-level stand-in tokenizer and a synthetic BPE; the token generator is not used here."""
    rng = np.random.default_rng(0)
    strs = ["".join(chr(int(c)) for c in rng.integers(1, 600, size=1 + f % 12)) for f in range(FAST_VOCAB)]
    # (an id outside the table decodes to nothing: extract_actions' re-encoding prepends BOS, whose mirrored id is one)
    decode = lambda ids: "".join(strs[i] if 0 <= i < FAST_VOCAB else "" for i in ids)
    tok = synth.CharTokenizer(vocab_size=VOCAB)
    fast = types.SimpleNamespace(bpe_tokenizer=types.SimpleNamespace(decode=decode), min_token=MIN_TOKEN, scale=SCALE)
    cfg = PI0FASTConfig(action_dim=D, chunk_size=H, n_action_steps=H, fast_skip_tokens=SKIP, device_detokenize=True, fast_vocab_size=FAST_VOCAB,
                        action_end_token_id=3 + ord("|"), action_format_token_ids=tuple(3 + ord(ch) for ch in "Action:"))
    return PI0FASTPolicy(cfg, types.SimpleNamespace(dev=dev, c={"vocab": VOCAB}), tok, fast), tok


def make_tokens(B, tok, dev):
    """"Action:" + band ids + "|" + EOS + pad, the band part of a random length in [L / 2, L - 12]."""
    rng = np.random.default_rng(B)
    out = np.full((B, L), tok.pad_token_id, dtype=np.int64)
    head = [3 + ord(ch) for ch in "Action:"]
    for b in range(B):
        n = int(rng.integers(L // 2, L - 12))
        row = head + list(VOCAB - SKIP - 1 - rng.integers(0, FAST_VOCAB, size=n)) + [3 + ord("|"), tok.eos_token_id]
        out[b, :len(row)] = row
    return torch.from_numpy(out).to(dev)


def timings(dev, reps=30, per_rep=20, host_reps=5):
    """-> {B: {launch_us, launch_us_min_max, eager_call_us, host_path_us, host_over_launch, host_over_eager, max_abs_diff}}."""
    pol, tok = make_policy(dev)
    d = pol._detok
    out = {}
    for B in BATCHES:
        toks = make_tokens(B, tok, dev)
        chunk = torch.empty(B, H, D, dtype=torch.float32, device=dev)
        launch = lambda: ops.fast_decode(toks, d.pieces, d.basis, band=d.band, stop_ids=d.stop_ids, skip_ids=d.skip_ids, min_token=MIN_TOKEN,
                                         scale=SCALE, horizon=H, action_dim=D, relaxed=True, out=chunk)
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        g = graphs.capture(launch, dev)[0]
        for _ in range(10):
            g.launch()
        torch.cuda.synchronize()
        t, ms = ops.Timer(), []
        for _ in range(reps):
            t.start()
            for _ in range(per_rep):
                g.launch()
            ms.append(t.stop() / per_rep)
        eager = []
        for _ in range(reps):
            t0 = time.perf_counter()
            launch()
            torch.cuda.synchronize()
            eager.append(time.perf_counter() - t0)
        host_s, ref = [], None
        for _ in range(1 + host_reps):                                     # the first pass warms the host path up and is dropped
            t0 = time.perf_counter()
            ref = pol.extract_actions(toks.cpu(), H, D).to(device=dev, dtype=torch.float32)
            torch.cuda.synchronize()
            host_s.append(time.perf_counter() - t0)
        host_s = host_s[1:]
        launch_us, eager_us, host_us = float(np.median(ms)) * 1e3, float(np.median(eager)) * 1e6, float(np.median(host_s)) * 1e6
        out[str(B)] = {"launch_us": round(launch_us, 2), "launch_us_min_max": [round(min(ms) * 1e3, 2), round(max(ms) * 1e3, 2)],
                       "eager_call_us": round(eager_us, 1), "host_path_us": round(host_us, 1),
                       "host_over_launch": round(host_us / launch_us, 1), "host_over_eager": round(host_us / eager_us, 1),
                       "max_abs_diff": float((chunk - ref).abs().max())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--host-reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(json.dumps({"L": L, "H": H, "D": D, "fast_decode": timings(dev, reps=a.reps, host_reps=a.host_reps)}))


if __name__ == "__main__":
    main()
