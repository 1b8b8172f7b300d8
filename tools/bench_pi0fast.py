"""pi0-FAST token path at full size on one MI355X (secondary measurement; bench.py is the contractual line): PaliGemma-3B geometry
(SigLIP-So400m 224^2 + Gemma-2B, vocabulary 257152), B = 40 candidates = 8 rephrased prompts x 5 samples, prompt 48 tokens, NEW
action tokens per candidate (default 32), synthetic weights.
  default        greedy: decoding is a function of the prompt, 8 distinct generations are decoded and broadcast
  SAMPLE=1       sampled (TEMPERATURE, TOP_K, TOP_P; defaults 1.0 / 50 / 0.95): max_batch = B, every candidate decodes on its own
                 with uniforms from a seeded generator; the line also counts the distinct token rows among the B candidates
  SAMPLE=both    greedy and sampled alternating, ROUNDS (default 3) lines of each: the spread of repeated runs in one process
  SHARE=1        generate_tokens(share_prefix=True) on a model with max_prompts = 8: the 8 distinct prefixes are prefilled once, all B
                 candidates decode (greedy too); COVER_FAST_FEEDBACK=0 keeps the torch bookkeeping between the steps of that path,
                 FEEDBACK=both measures every line with the fused kernel and with the torch bookkeeping, alternating in one process
The line carries share_prefix and prefill_rows (rows through the prefill: distinct prefixes x prefix length with SHARE=1, decoded
rows x prefix length without)."""
import os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cover_vla_amd import synth
from cover_vla_amd.pi0fast import PI0FASTTokens

dev = torch.device("cuda:0")
NEW = int(os.environ.get("NEW", "32"))
c = dict(synth.PI0_FULL)
g = synth._G(1234, False, 0.02, dev, torch.bfloat16)
sd = {}
n_patches = (c["image"] // c["patch"]) ** 2
for k, v in synth.vit_state(g, dim=c["vit_dim"], layers=c["vit_layers"], heads=c["vit_heads"], mlp=c["vit_mlp"], patch=c["patch"], n_pos=n_patches).items():
    sd["vision." + k] = v
sd["projector.weight"] = g.w(c["lm_dim"], c["vit_dim"]); sd["projector.bias"] = g.b(c["lm_dim"])
for k, v in synth.decoder_state(g, dim=c["lm_dim"], layers=c["layers"], Hq=c["Hq"], Hkv=c["Hkv"], D=c["D"], mlp=c["lm_mlp"], rms_base=0.0, vocab=c["vocab"]).items():
    sd["lm." + k] = v
B, P, L = 40, 8, 48
SAMPLE = os.environ.get("SAMPLE", "0")
TEMPERATURE, TOP_K, TOP_P = float(os.environ.get("TEMPERATURE", "1.0")), int(os.environ.get("TOP_K", "50")), float(os.environ.get("TOP_P", "0.95"))
SHARE = os.environ.get("SHARE", "0") != "0"
if SHARE:
    model = PI0FASTTokens(sd, c, device="cuda:0", max_batch=B, max_prompts=P, max_prompt=L, max_new_tokens=max(NEW, 8))
else:
    model = PI0FASTTokens(sd, c, device="cuda:0", max_batch=P if SAMPLE == "0" else B, max_prompt=L, max_new_tokens=max(NEW, 8))
del sd; torch.cuda.empty_cache()
gen = torch.Generator().manual_seed(0)
img = (torch.rand(1, 3, 224, 224, generator=gen) * 2 - 1).repeat(B, 1, 1, 1).to(dev)
toks = torch.zeros(B, L, dtype=torch.long); pad = torch.zeros(B, L, dtype=torch.long)
for p in range(P):
    n = 30 + p
    row = torch.randint(2, 257000, (n,), generator=gen)
    for s in range(B // P):
        toks[p * (B // P) + s, :n] = row; pad[p * (B // P) + s, :n] = 1
toks, pad = toks.to(dev), pad.to(dev)
ones = [torch.ones(B, dtype=torch.bool, device=dev)]
uni = torch.rand(B, NEW, generator=torch.Generator().manual_seed(1)).to(dev)
def step(sampled):
    kw = dict(uniforms=uni, temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P) if sampled else {}
    if SHARE:
        kw.update(share_prefix=True)
    return model.generate_tokens([img], ones, toks, pad, NEW, eos_token_id=-1, **kw)      # no early stop: NEW tokens for every row
wbytes = 2.0 * (c["layers"] * (c["lm_dim"] * (c["Hq"] + 2 * c["Hkv"]) * c["D"] + c["Hq"] * c["D"] * c["lm_dim"] + 3 * c["lm_dim"] * c["lm_mlp"]) + c["vocab"] * c["lm_dim"])
def measure(sampled, n=5):
    for _ in range(2): out = step(sampled)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n): out = step(sampled)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    assert out.shape == (B, NEW)
    rec = {"profile": "pi0-FAST tokens", "B": B, "distinct_prompts": P, "new_tokens": NEW, "ms_per_decision": round(dt * 1e3, 2),
           "candidates_per_s": round(B / dt, 1), "decode_weight_GB_per_step": round(wbytes / 1e9, 2),
           "hbm_floor_ms_decode": round((NEW - 1) * wbytes / 8e12 * 1e3, 2), "mode": "sampled" if sampled else "greedy",
           "share_prefix": SHARE, "prefill_rows": (P if SHARE or not sampled else B) * (n_patches + L)}
    if SHARE:
        rec["fused_feedback"] = os.environ.get("COVER_FAST_FEEDBACK", "1") != "0"
    if sampled:
        rec.update(temperature=TEMPERATURE, top_k=TOP_K, top_p=TOP_P, distinct_token_rows=len({tuple(r) for r in out.cpu().tolist()}))
    print(json.dumps(rec), flush=True)
def measure_ab(sampled):
    if SHARE and os.environ.get("FEEDBACK") == "both":
        for v in ("1", "0"):
            os.environ["COVER_FAST_FEEDBACK"] = v
            measure(sampled)
    else:
        measure(sampled)
if SAMPLE == "both":
    for _ in range(int(os.environ.get("ROUNDS", "3"))):
        measure_ab(False); measure_ab(True)
else:
    measure_ab(SAMPLE != "0")
