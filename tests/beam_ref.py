"""CPU references of the beam-search launches (cover_beam_merge, cover_kv_gather_slots, cover_beam_backtrack; include/cover_hip.h) and
a whole beam search over a callable, shared by tests/test_beam_cpu.py and tests/test_beam_gpu.py.

The merge has no tolerance: a candidate's score is ONE fp32 add (np.float32 + np.float32), the order is (higher score, lower beam,
lower rank), so every output is a fixed bit pattern. The per-row top-B lists of the whole search come from tests/topn_ref.py on
tests/logprob_ref.py (imported, not copied): float64 log-probabilities rounded to fp32 once."""
import numpy as np

from tests import topn_ref as TR

NINF = np.float32(-np.inf)


def merge(cum, cand_tok, cand_lp, B, feed_pad):
    """cum fp32 [G * B], cand_tok int64 / cand_lp fp32 [G * B, >= B] -> (parent int32, token int64, feed int64, cum_out fp32, step_lp fp32)."""
    cum = np.asarray(cum, dtype=np.float32)
    cand_tok, cand_lp = np.asarray(cand_tok, dtype=np.int64), np.asarray(cand_lp, dtype=np.float32)
    rows = cum.shape[0]
    assert rows % B == 0
    parent, token = np.full(rows, -1, np.int32), np.full(rows, -1, np.int64)
    feed = np.full(rows, feed_pad, np.int64)
    cum_out, step_lp = np.full(rows, NINF, np.float32), np.full(rows, NINF, np.float32)
    for g in range(rows // B):
        live = []
        for b in range(B):
            for j in range(B):
                c, lp, t = cum[g * B + b], cand_lp[g * B + b, j], cand_tok[g * B + b, j]
                if np.isfinite(c) and np.isfinite(lp) and t >= 0:
                    with np.errstate(over="ignore"):
                        live.append((np.float32(c + lp), b, j))
        live.sort(key=lambda e: (-float(e[0]), e[1], e[2]))       # -0.0 == +0.0 under the float comparison; the sort is stable anyway
        for r, (s, b, j) in enumerate(live[:B]):
            o = g * B + r
            parent[o], token[o], feed[o] = b, cand_tok[g * B + b, j], cand_tok[g * B + b, j]
            cum_out[o], step_lp[o] = s, cand_lp[g * B + b, j]
    return parent, token, feed, cum_out, step_lp


def gather(k_layers, vt_layers, src_slot, dst_slot, n_t, n_slots):
    """k_layers: list of arrays [n_slots, cap, Hkv, D]; vt_layers: list of [n_slots, Hkv, D, cap]. Returns copies with K rows / V^T
    columns t < n_t of slot dst_slot[i] set to slot src_slot[i]'s, rows with a slot outside [0, n_slots) skipped. Reads the ORIGINAL
    arrays (the contract: no destination is a source)."""
    ko, vo = [k.copy() for k in k_layers], [v.copy() for v in vt_layers]
    for s, d in zip(src_slot, dst_slot):
        if not (0 <= s < n_slots and 0 <= d < n_slots):
            continue
        for l in range(len(k_layers)):
            ko[l][d, :n_t] = k_layers[l][s, :n_t]
            vo[l][d, :, :, :n_t] = vt_layers[l][s, :, :, :n_t]
    return ko, vo


def backtrack(parent, token, step_lp, B):
    """Step-major [S, R] -> candidate-major (tokens int64 [R, S], logprobs fp32 [R, S])."""
    parent, token, step_lp = np.asarray(parent), np.asarray(token), np.asarray(step_lp, dtype=np.float32)
    S, R = parent.shape
    tokens, lps = np.full((R, S), -1, np.int64), np.full((R, S), NINF, np.float32)
    for r in range(R):
        g, cur = r // B, r % B
        for s in range(S - 1, -1, -1):
            if cur < 0:
                break
            i = g * B + cur
            tokens[r, s], lps[r, s] = token[s, i], step_lp[s, i]
            cur = int(parent[s, i]) if 0 <= parent[s, i] < B else -1
    return tokens, lps


def topn_lists(logits, lo, hi, B):
    """Per-row top-B lists of fp32 logits [rows, V] over [lo, hi) at temperature 1, unfiltered: (tok int64 [rows, B] absolute ids, -1
    padded; lp fp32 [rows, B], -inf padded), from tests/topn_ref.py."""
    refs = TR.reference_topn_rows(np.asarray(logits, dtype=np.float32), lo, hi, B, 1.0, 0, 1.0)
    tok = np.stack([np.where(r["top_tok"] >= 0, r["top_tok"] + lo, -1) for r in refs]).astype(np.int64)
    lp = np.stack([r["top_lp"] for r in refs]).astype(np.float32)
    return tok, lp


def search(step_logits, G, B, S, lo, hi, feed_pad=0):
    """Whole beam search. step_logits(prefixes) -> fp32 logits [G * B, V] for the int64 prefixes [G * B, i] (row g * B + b is beam b of
    group g; a dead beam's prefix holds -1). Returns (tokens [G * B, S], logprobs [G * B, S], scores [G * B], parents [S, G * B])."""
    rows = G * B
    cum = np.full(rows, NINF, np.float32)
    cum[::B] = 0.0
    prefixes = np.zeros((rows, 0), np.int64)
    parents, toks, lps = [], [], []
    for i in range(S):
        ct, cl = topn_lists(step_logits(prefixes), lo, hi, B)
        parent, token, _, cum, step_lp = merge(cum, ct, cl, B, feed_pad)
        src = (np.arange(rows) // B) * B + np.maximum(parent, 0)
        prefixes = np.concatenate([np.where((parent >= 0)[:, None], prefixes[src], -1), token[:, None]], 1)
        parents.append(parent), toks.append(token), lps.append(step_lp)
    tokens, logprobs = backtrack(np.stack(parents), np.stack(toks), np.stack(lps), B)
    return tokens, logprobs, cum, np.stack(parents)
