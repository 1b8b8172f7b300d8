"""The oracle (oracle/cover_ref) against golden vectors produced by the REFERENCE's own modules
(oracle/gen_golden.py, run in the build container). CPU only. Tolerances: fp32 heads/scores atol 1e-5,
indices exact."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
GOLD = os.path.join(ROOT, "tests", "golden")

from cover_ref import verifier as V  # noqa: E402
from cover_vla_amd import synth  # noqa: E402

# The goldens were written on one CPU with one thread count. The same eager graph on another CPU (another ISA: AMX vs AVX-512 BF16
# vs AVX2 kernels) or another thread split sums its GEMMs in another order: fp32 results move by about an ulp, a few bf16 results
# land one bf16 ulp away and a layer carries those on. Measured for one eager bf16 layer of the SAME graph on other kernel paths:
# <= 4.3e-3 rel-L2 from its golden; the nearest DIFFERENT graph (G3 (b): fp32 attention scores) sits >= 7.1e-3 from the same golden.
# XCPU_REL lies between the two: it accepts the rounding of other kernels and still rejects a different graph.
XCPU_REL = 5e-3


def _kernel_rounding_equal(a, b, rel_l2, max_frac=1.0):
    """a equals the golden b up to the summation order of the CPU's kernels: same shape, rel-L2 <= rel_l2 (orders of magnitude below
    what a structural difference produces) and at most max_frac of the elements different at all."""
    a, b = (x.double() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float64)) for x in (a, b))
    if a.shape != b.shape:
        return False
    return ((a - b).norm() / b.norm()).item() <= rel_l2 and (a != b).double().mean().item() <= max_frac


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "verifier_m*.npz"))))
def test_verifier_oracle_matches_reference(path):
    z = np.load(path)
    members, N, group = int(z["members"]), int(z["N"]), int(z["group"])
    ckpt = synth.verifier_checkpoint(members, seed=int(z["ckpt_seed"]))
    pf, tf, hists = synth.verifier_inputs(N, seed=int(z["input_seed"]))
    assert [len(h) for h in hists] == z["hist_lens"].tolist()
    with torch.no_grad():
        r = V.compute_max_similarity_scores(ckpt["ensemble_components"], pf, tf, hists, group)
    assert np.allclose(r["its"].numpy(), z["its"], atol=1e-5)
    assert np.allclose(r["acts"].numpy(), z["acts"], atol=1e-5)
    assert np.allclose(r["scores"].numpy(), z["scores"], atol=1e-5)
    assert r["global_idx"] == int(z["global_idx"])
    assert abs(r["max_score"] - float(z["max_score"])) < 1e-5


def test_verifier_oracle_mlp_action_encoder_matches_reference():
    """use_transformer = False variant (complex_action_encoder, efficient_ensemble_merged.py:148-184, 241-243)."""
    from cover_ref import verifier as V
    z = np.load(os.path.join(GOLD, "verifier_cae_m2_n8_g2.npz"))
    ckpt = synth.verifier_checkpoint(2, seed=int(z["ckpt_seed"]), use_transformer=False)
    pf, tf, hists = synth.verifier_inputs(8, seed=int(z["input_seed"]))
    with torch.no_grad():
        o = V.compute_max_similarity_scores(ckpt["ensemble_components"], pf, tf, hists, 2)
    assert np.allclose(o["acts"].numpy(), z["acts"], atol=1e-5)
    assert o["global_idx"] == int(z["global_idx"]) and abs(o["max_score"] - float(z["max_score"])) < 1e-5


@pytest.mark.parametrize("name", ["verifier_train_fwd_tr_b12", "verifier_train_fwd_mlp_b6"])
def test_verifier_oracle_contrastive_forward_matches_reference(name):
    """Validation forward of one verifier model + InfoNCE loss + top-k accuracies (finetune_trajectory_bridge_ddp.py:357-421,
    :446-469, :895-899), against the reference's own VLA_SigLIP2_Bridge.forward (oracle/gen_golden.py gen_verifier_training)."""
    from cover_ref import verifier as V
    z = np.load(os.path.join(GOLD, name + ".npz"))
    ckpt = synth.verifier_checkpoint(1, seed=int(z["ckpt_seed"]), use_transformer=bool(z["use_transformer"]))
    pf, tf, hist = synth.verifier_batch_inputs(int(z["B"]), seed=int(z["input_seed"]))
    assert np.array_equal(hist.numpy(), z["hist"])          # the seeded batch is the generator's batch
    with torch.no_grad():
        li, la = V.contrastive_forward(ckpt["ensemble_components"][0], float(z["logit_scale"]), pf, tf, hist)
    assert np.allclose(li.numpy(), z["image_logits"], atol=2e-5) and np.allclose(la.numpy(), z["action_logits"], atol=2e-5)
    m = V.contrastive_metrics(li, la)
    assert abs(m["loss"] - float(z["loss"])) < 1e-5 and abs(m["image_loss"] - float(z["image_loss"])) < 1e-5
    for k, v in zip(z["acc_names"], z["acc_values"]):
        assert abs(m[str(k)] - float(v)) < 1e-7, k


def test_verifier_oracle_public_api_golden():
    """The reference's public 4-tuple (distinct instructions per group), restated at the feature level."""
    from cover_ref import verifier as V
    z = np.load(os.path.join(GOLD, "verifier_api_m2_n12_g3.npz"))
    ckpt = synth.verifier_checkpoint(2, seed=int(z["ckpt_seed"]))
    pf, tf, hists = synth.verifier_inputs(12, seed=int(z["input_seed"]))
    with torch.no_grad():
        o = V.compute_max_similarity_scores(ckpt["ensemble_components"], pf, tf, hists, 3)
        _, _, h10 = synth.verifier_inputs(6, seed=32, min_hist=10)
        p = V.compute_max_similarity_scores(ckpt["ensemble_components"], pf, tf, h10, 1)
    assert o["global_idx"] == int(z["global_idx"]) and o["group"] == int(z["instr_index"]) // 3
    assert abs(o["max_score"] - float(z["max_score"])) < 1e-5
    assert np.allclose(p["scores"].numpy(), z["predict_scores"], atol=1e-5) and int(p["scores"].argmax()) == int(z["predict_index"])
    assert np.allclose(p["fused_act"].numpy(), z["fused_act"], atol=1e-5)
    assert np.allclose(p["fused_it"].numpy().repeat(6, 0), z["fused_it"], atol=1e-5)


def test_verifier_ties_first_index_wins():
    z = np.load(os.path.join(GOLD, "verifier_ties.npz"))
    ckpt = synth.verifier_checkpoint(2, seed=99)
    pf, tf, _ = synth.verifier_inputs(12, seed=99)
    with torch.no_grad():
        r = V.compute_max_similarity_scores(ckpt["ensemble_components"], pf, tf, [z["hist"]] * 12, 3)
    assert r["global_idx"] == int(z["global_idx"]) == 0
    assert abs(r["max_score"] - float(z["max_score"])) < 1e-5


# ------------------------------------------------------------------------------------------------ pi0 sampler
from tests.helpers import _pi0_cfg, pi0_case  # noqa: E402


@pytest.mark.parametrize("name", ["pi0_tiny_b6", "pi0_tiny_b1", "pi0_tiny_b40"])
def test_pi0_oracle_matches_reference(name):
    from cover_ref import pi0 as P
    z, tiny, sd, (images, img_masks, toks, masks, state, noise) = pi0_case(os.path.join(GOLD, name + ".npz"))
    cfg = _pi0_cfg(tiny)
    sdr = P.cast_like_reference(sd)
    with torch.no_grad():
        pe, _, _ = P.embed_prefix(cfg, sdr, images, img_masks, toks, masks)
        se, _, _ = P.embed_suffix(cfg, sdr, state, noise, torch.ones(state.shape[0]))
        x = P.sample_actions(cfg, sdr, images, img_masks, toks, masks, state, noise)
        x_iso = P.sample_actions(cfg, sdr, images, img_masks, toks, masks, state, noise,
                                 prefix_embs=torch.from_numpy(z["prefix_embs"]).to(torch.bfloat16))
    nimg = cfg.n_img_tokens
    a, b = pe.float().numpy(), z["prefix_embs"]
    # language tokens: same eager op sequence -> bit-identical; suffix embedding (fp32 projections): bit-identical on the CPU that
    # wrote the golden, elsewhere equal up to the summation order of the CPU's GEMM kernels
    assert np.array_equal(a[:, nimg:], b[:, nimg:])
    assert _kernel_rounding_equal(se.float(), z["suffix_embs_t1"], rel_l2=1e-6)
    # image tokens go through the un-vendored HF SigLIP tower whose attention rounds differently (sdpa, bf16 scores):
    # bf16-ulp level agreement only
    assert np.linalg.norm(a[:, :nimg] - b[:, :nimg]) / np.linalg.norm(b[:, :nimg]) < 1e-2
    # decoder + flow matching, isolated from the tower by feeding the reference's own prefix embeddings: bit-identical on the CPU
    # that wrote the golden; on another CPU the bf16 GEMM kernels' rounding runs through 10 Euler steps (measured on other kernel
    # paths: rel-L2 <= 5.2e-3 of the update, max-abs <= 1.5e-2), judged on the UPDATE like the end-to-end check below but half as
    # wide in both measures (that one also carries the tower's rounding)
    upd = z["actions"] - noise.numpy()
    d_iso = x_iso.numpy() - z["actions"]
    assert np.linalg.norm(d_iso) / np.linalg.norm(upd) < 1e-2 and np.abs(d_iso).max() < 2e-2, np.abs(d_iso).max()
    # end to end (tower included): bf16-ulp differences of the tower propagate through randomly initialised layers;
    # judged on the flow-matching UPDATE (actions - noise): relative L2 <= 2e-2, and max-abs within 2x the loosest
    # rung the reference itself accepted against JAX (atol 3e-2, compare_with_jax.py:131-133)
    assert np.linalg.norm(x.numpy() - z["actions"]) / np.linalg.norm(upd) < 2e-2
    assert np.abs(x.numpy() - z["actions"]).max() < 6e-2


# ------------------------------------------------------------------------------------------------ P2 blocks vs HF modules
class _fp32_blocks:
    """Evaluate the oracle's blocks in fp32 (module-level BF switched) to pin STRUCTURE against HF's fp32 modules."""

    def __enter__(self):
        from cover_ref import blocks as Bk
        self.Bk, self.old = Bk, Bk.BF
        Bk.BF = torch.float32
        return Bk

    def __exit__(self, *a):
        self.Bk.BF = self.old


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files if z[k].dtype.kind == "f" and k not in ("logits", "pixels", "last_hidden", "hidden_1", "hidden_2")}
    return z, sd


def test_blocks_match_hf_llama():
    z, sd = _load("hf_llama_tiny")
    with _fp32_blocks() as Bk, torch.no_grad():
        cfg = Bk.DecoderCfg(64, 2, 4, 4, 16, 128, "silu", "llama", 1e-5, "hf")
        ids = torch.from_numpy(z["ids"])
        x = torch.nn.functional.embedding(ids, sd["llm.embed_tokens.weight"])
        T = ids.shape[1]
        mask = torch.tril(torch.ones(T, T, dtype=torch.bool))[None].expand(2, -1, -1)
        lsd = {k[4:]: v for k, v in sd.items() if k.startswith("llm.")}
        h, _ = Bk.decoder_forward(cfg, lsd, x, torch.arange(T)[None].expand(2, -1), mask, final_norm=True, n_pos=64)
        logits = torch.nn.functional.linear(h, sd["lm_head.weight"])
    assert np.allclose(logits.numpy(), z["logits"], atol=2e-4, rtol=1e-4), np.abs(logits.numpy() - z["logits"]).max()


def test_blocks_match_hf_siglip():
    z, sd = _load("hf_siglip_tiny")
    with _fp32_blocks() as Bk, torch.no_grad():
        cfg = Bk.VitCfg(48, 2, 4, 80, 14, "gelu_tanh", 1e-6)
        x = Bk.vit_embed(cfg, sd, torch.from_numpy(z["pixels"]))
        h1 = Bk.vit_encode(cfg, sd, x.clone(), n_blocks=1)
        out = Bk.vit_encode(cfg, sd, x, post_ln=True)
    assert np.allclose(h1.numpy(), z["hidden_1"], atol=2e-4, rtol=1e-4)
    assert np.allclose(out.numpy(), z["last_hidden"], atol=2e-4, rtol=1e-4)


def test_blocks_match_hf_dinov2_with_registers():
    z, sd = _load("hf_dinov2_tiny")
    with _fp32_blocks() as Bk, torch.no_grad():
        cfg = Bk.VitCfg(48, 2, 4, 96, 14, "gelu_erf", 1e-6, layerscale=True, prefix_tokens=5)
        x = Bk.vit_embed(cfg, sd, torch.from_numpy(z["pixels"]))
        h1 = Bk.vit_encode(cfg, sd, x.clone(), n_blocks=1)
        h2 = Bk.vit_encode(cfg, sd, x, n_blocks=2)
    assert np.allclose(h1.numpy(), z["hidden_1"], atol=2e-4, rtol=1e-4)
    assert np.allclose(h2.numpy(), z["hidden_2"], atol=2e-4, rtol=1e-4)


def _g2_case():
    from gen_golden_g2 import G2, SEED, g2_inputs
    z = np.load(os.path.join(GOLD, "pi0_g2_fullwidth.npz"))
    assert int(z["seed"]) == SEED and all(int(z["g2_" + k]) == v for k, v in G2.items())
    unbits = lambda a: torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).float()
    gold = dict(pre_b0=unbits(z["prefix_out_b0"]), pre_b1=unbits(z["prefix_out_b1_every4"]), k_b0=unbits(z["k_b0"]), v_b0=unbits(z["v_b0"]),
                suffix=torch.from_numpy(z["suffix_out"]))
    return dict(G2), SEED, g2_inputs(), gold


def test_oracle_full_width_gemma_layers_match_reference_g2():
    """one full-width Gemma-2B layer (T = 328, head_dim 256, MQA 8:1, MLP 16384) and one expert layer (5 suffix
    tokens over the cached prefix) through the reference's PaliGemmaWithExpertModel.forward vs the oracle's decoder_forward."""
    from cover_ref import blocks as Bk, pi0 as P
    g2, seed, (prefix, pad, att, suffix, s_pad, s_att), gold = _g2_case()
    sd = P.cast_like_reference(synth.pi0_state(g2, seed=seed))
    lm = Bk.DecoderCfg(g2["lm_dim"], 1, g2["Hq"], g2["Hkv"], g2["D"], g2["lm_mlp"], "gelu_tanh", "gemma", 1e-6, "pi0")
    ex = Bk.DecoderCfg(g2["ex_dim"], 1, g2["Hq"], g2["Hkv"], g2["D"], g2["ex_mlp"], "gelu_tanh", "gemma", 1e-6, "pi0")
    B = prefix.shape[0]
    with torch.no_grad():
        pmask = P.make_att_2d_masks(pad, att)
        ppos = torch.cumsum(pad, dim=1) - 1
        pre, kv = Bk.decoder_forward(lm, P.sub(sd, "lm."), prefix, ppos.clamp(min=0), pmask, past=None, keep_kv=True, final_norm=True)
        S, T = s_pad.shape[1], pad.shape[1]
        full = torch.cat([pad[:, None, :].expand(B, S, T), P.make_att_2d_masks(s_pad, s_att)], dim=2)
        spos = torch.sum(pad, dim=-1)[:, None] + torch.cumsum(s_pad, dim=1) - 1
        suf, _ = Bk.decoder_forward(ex, P.sub(sd, "expert."), suffix, spos, full, past=kv, keep_kv=False, final_norm=True)
    n0, n1 = int(pad[0].sum()), int(pad[1].sum())
    rel = lambda a, b: ((a.float() - b).norm() / b.norm()).item()
    assert rel(pre[0, :n0], gold["pre_b0"][:n0]) < XCPU_REL                   # two eager bf16 evaluations of the same graph
    assert rel(pre[1, ::4][: (n1 + 3) // 4], gold["pre_b1"][: (n1 + 3) // 4]) < XCPU_REL
    assert rel(kv[0][0][0, :n0, 0], gold["k_b0"][:n0]) < XCPU_REL and rel(kv[0][1][0, :n0, 0], gold["v_b0"][:n0]) < XCPU_REL
    assert rel(suf, gold["suffix"]) < XCPU_REL


def _g3_case():
    """hf_llama7b_layer.npz: one full-width Llama-2-7B layer through HF LlamaModel (oracle/gen_golden_llama7b.py)."""
    from gen_golden_llama7b import HEADS, L7, LT, N_PATCH, P, S, SEED, llama7b_inputs, llama7b_weights
    z = np.load(os.path.join(GOLD, "hf_llama7b_layer.npz"))
    assert int(z["seed"]) == SEED and all(int(z["l7_" + k]) == v for k, v in L7.items())
    assert (int(z["n_patch"]), int(z["P"]), int(z["LT"]), int(z["S"])) == (N_PATCH, P, LT, S) and tuple(z["heads"].tolist()) == HEADS
    unbits = lambda a: torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).float()
    gold = {k: unbits(z[k]) for k in ("prefix_every4", "k_prefix_every4", "v_prefix_every4", "text_p0", "text_p5", "k_text_p5", "v_text_p5",
                                       "last_text_rows", "decode_rows")}
    gold.update({k: torch.from_numpy(z[k]) for k in ("f32_prefix_every16", "f32_text_p5", "f32_last_text_rows", "f32_decode_rows")})
    return dict(L7), llama7b_weights(), llama7b_inputs(), gold


def test_oracle_full_width_llama7b_layer_matches_hf_g3():
    """G3: one full-width Llama-2-7B layer (4096 wide, 32 x 128 MHA, MLP 11008) on [BOS | 256 patches | text] and one decode row per
    sample over the cache -- HF LlamaModel (bf16, eager) vs the oracle's decoder_forward. Prompts 0 and 5 (CPU time).
    (a) with HF's bf16 attention scores restated (scores_bf16) the oracle IS HF's graph: rel-L2 < XCPU_REL, post-RoPE K / V bit-exact
        up to the rounding of the CPU's GEMM kernels;
    (b) in its default form (fp32 scores, what the HIP kernels compute) it sits no further from HF's fp32 evaluation of the same
        bf16 parameters than HF's own bf16 path does (HF-bf16: ~0.8e-2)."""
    from cover_ref import blocks as Bk
    from gen_golden_llama7b import HEADS, N_PATCH, S
    l7, sd, i, gold = _g3_case()
    sdb = Bk.to_bf16(sd)
    T0 = 1 + N_PATCH
    rel = lambda a, b: ((a.float() - b).norm() / b.norm()).item()
    # one projection + RoPE: bit-exact but for the odd element whose fp32 sum sits on a bf16 rounding boundary (another CPU's kernel)
    kv_equal = lambda a, b: _kernel_rounding_equal(a, b, rel_l2=1e-4, max_frac=1e-3)
    hf_own = {"text": rel(gold["text_p5"], gold["f32_text_p5"]), "dec": rel(gold["decode_rows"], gold["f32_decode_rows"]),
              "last": rel(gold["last_text_rows"], gold["f32_last_text_rows"]), "prefix": rel(gold["prefix_every4"][::4], gold["f32_prefix_every16"])}
    assert all(5e-3 < v < 1.2e-2 for v in hf_own.values()), hf_own
    for hf_scores in (True, False):
        cfg = Bk.DecoderCfg(l7["dim"], 1, l7["Hq"], l7["Hkv"], l7["D"], l7["mlp"], "silu", "llama", 1e-5, "hf", scores_bf16=hf_scores)
        with torch.no_grad():
            for p in (0, 5):
                n = int(i["lens"][p])
                x = torch.cat([i["bos"], i["patches"], i["text"][p, :n]], 0)[None]
                T = x.shape[1]
                pos = torch.arange(T)[None]
                mask = torch.tril(torch.ones(T, T, dtype=torch.bool))[None]
                h, kv = Bk.decoder_forward(cfg, sdb, x, pos, mask, past=None, keep_kv=True, final_norm=True, n_pos=512)
                dec = []
                for s in range(S):
                    xd = i["dec"][p * S + s][None, None]
                    m1 = torch.ones(1, 1, T + 1, dtype=torch.bool)
                    hd, _ = Bk.decoder_forward(cfg, sdb, xd, torch.tensor([[T]]), m1, past=kv, keep_kv=False, final_norm=True, n_pos=512)
                    dec.append(hd[0, 0])
                dec = torch.stack(dec)
                if hf_scores:
                    if p == 0:
                        assert rel(h[0, 1:T0][::4], gold["prefix_every4"]) < XCPU_REL
                        assert kv_equal(kv[0][0][0, 1:T0][::4][:, list(HEADS)].transpose(0, 1).float(), gold["k_prefix_every4"])
                        assert kv_equal(kv[0][1][0, 1:T0][::4][:, list(HEADS)].transpose(0, 1).float(), gold["v_prefix_every4"])
                    else:
                        assert kv_equal(kv[0][0][0, T0:][:, list(HEADS)].transpose(0, 1).float(), gold["k_text_p5"])
                    assert rel(h[0, T0:], gold["text_p0" if p == 0 else "text_p5"]) < XCPU_REL
                    assert rel(h[0, -1], gold["last_text_rows"][p]) < XCPU_REL
                    assert rel(dec, gold["decode_rows"][p * S:(p + 1) * S]) < XCPU_REL
                else:
                    if p == 0:
                        assert rel(h[0, 1:T0][::16], gold["f32_prefix_every16"]) <= 1.1 * hf_own["prefix"]
                    else:
                        assert rel(h[0, T0:], gold["f32_text_p5"]) <= 1.1 * hf_own["text"]
                    assert rel(h[0, -1], gold["f32_last_text_rows"][p]) <= 1.25 * hf_own["last"]      # one row: noisier
                    assert rel(dec, gold["f32_decode_rows"][p * S:(p + 1) * S]) <= 1.1 * hf_own["dec"]


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def test_oracle_siglip2_bridge_matches_hf_text_and_image_towers():
    """the verifier backbone restatement (cover_ref.openvla.siglip2_features) against HF SiglipVisionModel +
    SiglipTextModel with the bridge's hook semantics: patch features = the LAST block's attention-module output, text
    features = transformer -> final_layer_norm -> head on every position (fixture: oracle/gen_golden_hf.py)."""
    from cover_ref import openvla as OR
    from gen_golden_hf import siglip2_bridge_weights
    z = np.load(os.path.join(GOLD, "hf_siglip2_bridge_tiny.npz"))
    c, sd = siglip2_bridge_weights(int(z["weight_seed"]))
    with torch.no_grad():
        pf, tf = OR.siglip2_features(c, sd, torch.from_numpy(z["pixels"]), torch.from_numpy(z["ids"]))      # fp32 weights: fp32 math
    assert torch.allclose(pf, torch.from_numpy(z["patch_features"]), atol=2e-5)
    assert torch.allclose(tf, torch.from_numpy(z["text_features"]), atol=2e-5)
    # HF's own pooled output = head(last position): the same projection the restatement applies to every position
    pooled = torch.from_numpy(z["text_pooled"])
    assert torch.allclose(tf[:, -1], pooled / pooled.norm(dim=-1, keepdim=True), atol=2e-5)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_oracle_openvla_end_to_end_matches_hf_composition(prec):
    """END-TO-END P2 pin: the oracle's sampler (vision towers -> projector -> [BOS | patches | prompt] -> Llama -> 7 greedy
    tokens) against the same pipeline composed from HF modules (Dinov2WithRegisters + SiglipVision + LlamaForCausalLM), per-step
    logits and token ids. fp32: logits atol 2e-3, tokens exact. bf16 (two different eager bf16 evaluations: HF rounds scores to
    bf16 before the softmax, the reference repo's convention keeps them fp32): logits rel-L2 <= 3e-2, tokens exact wherever the
    HF top-1 / top-2 margin exceeds twice the logit error."""
    from cover_ref import blocks as Bk, openvla as OR
    from gen_golden_hf import openvla_e2e_weights
    z = np.load(os.path.join(GOLD, "hf_openvla_e2e_tiny.npz"))
    c, sd = openvla_e2e_weights(int(z["weight_seed"]))
    frame, toks, lens = torch.from_numpy(z["frame"]), torch.from_numpy(z["toks"]), torch.from_numpy(z["lens"])
    ref_l, ref_t = torch.from_numpy(z["logits_" + prec]), torch.from_numpy(z["tokens_" + prec])
    tr = {}
    if prec == "bf16":
        with torch.no_grad():
            tok = OR.sample(c, Bk.to_bf16(sd), frame, toks, lens, 1, None, trace=tr)
    else:
        with _fp32_blocks(), torch.no_grad():          # the same graph evaluated in fp32 (structure pin)
            tok = OR.sample(c, sd, frame, toks, lens, 1, None, trace=tr)
    lg = tr["logits"]
    if prec == "fp32":
        assert torch.allclose(lg, ref_l, atol=2e-3), (lg - ref_l).abs().max()
        assert torch.equal(tok, ref_t)
        return
    n_dec = 0
    for n in range(tok.shape[0]):
        agree_so_far = True
        for i in range(7):
            if not agree_so_far:
                break                                # free-running: after the first differing pick the contexts differ
            err = (lg[n, i] - ref_l[n, i]).abs().max().item()
            assert _rel(lg[n, i], ref_l[n, i]) < 3e-2, (n, i, _rel(lg[n, i], ref_l[n, i]))
            top2 = torch.topk(ref_l[n, i, : c["tok_vocab"]], 2).values
            if (top2[0] - top2[1]).item() > 2 * err:
                n_dec += 1
                assert tok[n, i] == ref_t[n, i], (n, i)
            agree_so_far = bool(tok[n, i] == ref_t[n, i])
    assert n_dec >= 10


def test_oracle_openvla_batched_execution_equals_per_candidate():
    """OR.sample_batched (ONE left-padded batched forward over N un-deduplicated rows, the way the reference executes a policy call --
    what bench.py times as `cpu_baseline.as_executed_batched`) is the same function as OR.sample (one candidate at a time): in fp32 the
    per-step logits agree to 2e-3 and every token is identical, greedy and sampled, with ragged prompt lengths and samples > 1; the same
    structure through HF's fixture: tokens of the HF composition reproduced exactly."""
    from cover_ref import openvla as OR
    from gen_golden_hf import openvla_e2e_weights
    z = np.load(os.path.join(GOLD, "hf_openvla_e2e_tiny.npz"))
    c, sd = openvla_e2e_weights(int(z["weight_seed"]))
    frame, toks, lens = torch.from_numpy(z["frame"]), torch.from_numpy(z["toks"]), torch.from_numpy(z["lens"])
    with _fp32_blocks(), torch.no_grad():
        tr = {}
        tb = OR.sample_batched(c, sd, frame, toks, lens, 1, None, trace=tr)
        assert torch.equal(tb, torch.from_numpy(z["tokens_fp32"]))
        assert torch.allclose(tr["logits"], torch.from_numpy(z["logits_fp32"]), atol=2e-3)
        g = torch.Generator().manual_seed(5)
        u = torch.rand(toks.shape[0] * 2, 7, generator=g)
        ta, tbb = {}, {}
        a = OR.sample(c, sd, frame, toks, lens, 2, u, 1.0, trace=ta)
        b = OR.sample_batched(c, sd, frame, toks, lens, 2, u, 1.0, trace=tbb)
        assert torch.equal(a, b)
        assert torch.allclose(ta["logits"], tbb["logits"], atol=2e-3)


# ------------------------------------------------------------------------------------------------ pi0-FAST token path
def _fast_case(name):
    from gen_golden_pi0fast import fast_inputs
    z = np.load(os.path.join(GOLD, name + ".npz"))
    tiny = {k[5:]: int(z[k]) for k in z.files if k.startswith("tiny_")}
    sd = synth.pi0_state(tiny, seed=int(z["seed"]))
    return z, tiny, sd, fast_inputs(tiny, int(z["B"]), int(z["Lp"]), int(z["seed"]))


@pytest.mark.parametrize("name", ["pi0fast_tiny_b6_f32", "pi0fast_tiny_b1_f32"])
def test_oracle_pi0fast_tokens_match_reference(name):
    """Greedy pi0-FAST token generation (embed_inputs + block-causal mask + PaliGemma forward of the REFERENCE, imported by
    oracle/gen_golden_pi0fast.py) vs the restatement, fp32: logits of every step, the picked tokens, the teacher-forced
    continuation and the pad-after-EOS rule."""
    from cover_ref import pi0fast as PF
    z, tiny, sd, (img, toks, pad) = _fast_case(name)
    n_new = int(z["n_new"])
    with _fp32_blocks() as Bk, torch.no_grad():
        vit = Bk.VitCfg(tiny["vit_dim"], tiny["vit_layers"], tiny["vit_heads"], tiny["vit_mlp"], tiny["patch"], "gelu_tanh", 1e-6)
        lm = Bk.DecoderCfg(tiny["lm_dim"], tiny["layers"], tiny["Hq"], tiny["Hkv"], tiny["D"], tiny["lm_mlp"], "gelu_tanh", "gemma", 1e-6, "hf")
        gen, lg = PF.generate(vit, lm, sd, img, toks, pad, n_new)
        _, lgf = PF.generate(vit, lm, sd, img, toks, pad, n_new, force=torch.from_numpy(z["force"]))
        gen_e, lge = PF.generate(vit, lm, sd, img, toks, pad, n_new, eos=int(z["eos2"]))
    assert np.allclose(lg.numpy(), z["logits"], atol=3e-4), np.abs(lg.numpy() - z["logits"]).max()
    assert np.array_equal(gen.numpy(), z["tokens"])
    assert np.allclose(lgf.numpy(), z["logits_forced"], atol=3e-4), np.abs(lgf.numpy() - z["logits_forced"]).max()
    assert np.array_equal(gen_e.numpy(), z["tokens_eos2"]) and (z["tokens_eos2"][0, 1:] == 0).all()
    # the embedded prefix of the reference (left padded) holds the same rows as the restatement's (right padded)
    with _fp32_blocks() as Bk, torch.no_grad():
        pe, pm = PF.embed_inputs(vit, lm, sd, img, toks, pad)
    ref_e, ref_m = z["prefix_embs_leftpad"], z["pad_masks_leftpad"]
    for b in range(pe.shape[0]):
        assert np.allclose(pe[b][pm[b].bool()].numpy(), ref_e[b][ref_m[b].astype(bool)], atol=2e-5)


def test_oracle_pi0fast_bf16_matches_reference():
    """The same path with the language model / tower / projector in bf16 (PI0FAST.__init__ :466-473), teacher-forced: logits
    within bf16 noise of the reference's bf16 run, arg-max equal wherever the reference's margin exceeds the error."""
    from cover_ref import blocks as Bk, pi0fast as PF
    z, tiny, sd, (img, toks, pad) = _fast_case("pi0fast_tiny_b6_bf16")
    sdb = {k: (v.to(torch.bfloat16) if k.startswith(("lm.", "vision.", "projector.")) else v) for k, v in sd.items()}
    vit = Bk.VitCfg(tiny["vit_dim"], tiny["vit_layers"], tiny["vit_heads"], tiny["vit_mlp"], tiny["patch"], "gelu_tanh", 1e-6)
    lm = Bk.DecoderCfg(tiny["lm_dim"], tiny["layers"], tiny["Hq"], tiny["Hkv"], tiny["D"], tiny["lm_mlp"], "gelu_tanh", "gemma", 1e-6, "hf")
    with torch.no_grad():
        _, lgf = PF.generate(vit, lm, sdb, img, toks, pad, int(z["n_new"]), force=torch.from_numpy(z["force"]))
    ref = torch.from_numpy(z["logits_forced"])
    assert _rel(lgf, ref) < 2e-2, _rel(lgf, ref)
    err = (lgf - ref).abs().amax(-1)
    top2 = torch.topk(ref, 2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 2 * err
    assert decided.sum() >= 30 and torch.equal(lgf.argmax(-1)[decided], ref.argmax(-1)[decided])


def test_oracle_pi0fast_dct_decode_matches_reference():
    from cover_ref import pi0fast as PF
    z = np.load(os.path.join(GOLD, "pi0fast_dct_decode.npz"))
    seqs = [z["seq0"].tolist(), z["seq1"].tolist(), z["seq2"].tolist()]
    out = PF.decode_actions_with_fast(seqs, lambda t: "".join(chr(i) for i in t), int(z["min_token"]), float(z["scale"]), 4, 7)
    assert np.allclose(out, z["actions"], atol=1e-12)
