"""CoVer verifier on MI355X behind the reference's API (bridge_verifier/ensemble_eval/efficient_ensemble_merged.py).

  EfficientEnsembleMerged(merged_checkpoint, device=...)                      :25-186
      .extract_shared_features(img_tensor, text_tokens) -> (patch_features, text_features)      :188-192
      .get_embeddings_from_model_batch(model_idx, pf, tf, histories)                            :194-247
      .fuse_embeddings / .predict                                                               :249-307
      .compute_max_similarity_scores_batch(images, instructions, histories, group) ->
            (max_score: float, max_instruction: str, max_action_history: ndarray, global_action_idx: 0-dim int64) :309-454

Same results, different schedule: the reference repeats the (image, text) heads N times on identical inputs
(:213-214) and loops members sequentially; here the image-text embedding of a member is computed once per distinct
(image, text) pair and only the trajectory encoder runs per candidate. Heads, fusion and scoring stay fp32 as in
the reference; the frozen SigLIP2 towers run in bf16 through the shared ViT kernels.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import host, ops
from .models import BF, VitTower, _f32


def _dev_sd(sd, dev):
    return {k: (_f32(v, dev) if torch.is_tensor(v) else v) for k, v in sd.items()}


def _member_batch() -> bool:
    """COVER_MEMBER_BATCH=0 (A/B runs): every member runs as a stack of one instead of all members per launch."""
    return os.environ.get("COVER_MEMBER_BATCH", "1") != "0"


def _pad_mask(hist: torch.Tensor, pad_value: float, dev) -> torch.Tensor:
    """hist [N, T, A] -> uint8 [N, T] on dev, 1 where the step is padding (efficient_ensemble_merged.py:229: a comparison where `hist`
    lives, no arithmetic)."""
    return (hist[:, :, 0] == pad_value).to(torch.uint8).to(dev).contiguous()


def _stack(ts: List[torch.Tensor]) -> torch.Tensor:
    """[G, ...] of G same-shaped contiguous tensors; a lone tensor is viewed, not copied."""
    return ts[0].unsqueeze(0) if len(ts) == 1 else torch.stack(ts).contiguous()


def _stackable(sds: List[Optional[dict]]) -> bool:
    """The state dicts (None = the member has no such module) have the same keys and tensor shapes."""
    sig = lambda sd: None if sd is None else {k: (tuple(v.shape) if torch.is_tensor(v) else None) for k, v in sd.items()}
    return all(sig(sd) == sig(sds[0]) for sd in sds)


class _Pooling:
    """Weights of one AttentionPooling (model.py:76-112) with num_readouts = 1; `_PoolingStack` runs them."""

    def __init__(self, sd, dev, heads=8):
        self.sd = _dev_sd(sd, dev)
        self.heads = heads
        self.n_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        self.dim = sd["query"].shape[-1]
        # K and V projections of all blocks read the same kv tokens: one stacked weight -> one GEMM per pooling
        ws, bs = [], []
        for i in range(self.n_layers):
            p = f"blocks.{i}.attention."
            b_in = self.sd[p + "in_proj_bias"]
            ws += [self.sd[p + "k_proj_weight"], self.sd[p + "v_proj_weight"]]
            bs += [b_in[self.dim:2 * self.dim], b_in[2 * self.dim:]]
        self.w_kv = torch.cat(ws, 0).contiguous()
        self.b_kv = torch.cat(bs, 0).contiguous()


class _Member:
    """One ensemble member's weights, softmax temperature, padding value and trajectory depth; the stacks below run them."""

    def __init__(self, comp: dict, dev):
        self.dev = dev
        ta = comp["text_aware_visual_extraction"]
        self.inv_temp = 1.0 / float(torch.as_tensor(ta["temperature"]).clamp(0, 100))
        self.pos_emb = _f32(ta["pos_emb"], dev)
        self.vision = _Pooling(comp["vision_poolings"], dev)
        self.text = _Pooling(comp["text_pooling"], dev)
        self.ip = _dev_sd(comp["input_projection"], dev)
        self.mlp = None
        if comp.get("trajectory_encoder") is not None:
            self.se = _dev_sd(comp["single_step_action_encoder"], dev)
            self.traj = _dev_sd(comp["trajectory_encoder"], dev)
            self.traj_layers = 1 + max(int(k.split(".")[1]) for k in comp["trajectory_encoder"])
        else:
            # MLP action encoder (use_transformer = False): Sequential(Linear(h*a, 512), LayerNorm, ReLU, Dropout, Linear)
            # -> state-dict keys 0.*, 1.*, 4.* (efficient_ensemble_merged.py:148-184)
            self.mlp = _dev_sd(comp["complex_action_encoder"], dev)
            self.se, self.traj, self.traj_layers = None, None, 0
        self.pad_value = float(comp["action_padding_value"])


class _PoolingStack:
    """AttentionPooling of G members (member = batch index): one learned query per member cross-attends that member's kv tokens."""

    def __init__(self, pools: List[_Pooling]):
        p0 = pools[0]
        self.G, self.L, self.E, self.H = len(pools), p0.n_layers, p0.dim, p0.heads
        self.sd = {k: _stack([pp.sd[k] for pp in pools]) for k in p0.sd if torch.is_tensor(p0.sd[k])}
        self.w_kv, self.b_kv = _stack([pp.w_kv for pp in pools]), _stack([pp.b_kv for pp in pools])
        self.q_b = [_stack([pp.sd[f"blocks.{i}.attention.in_proj_bias"][:p0.dim] for pp in pools]) for i in range(p0.n_layers)]

    def __call__(self, x: torch.Tensor, shared: bool) -> torch.Tensor:
        """x fp32 [T, Din] (shared by every member) or [G, T, Din] -> [G, E]."""
        sd, G, E, H = self.sd, self.G, self.E, self.H
        T, Din = x.shape[-2], x.shape[-1]
        ld = self.w_kv.shape[1]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        kv = ops.gemm_f32(x, self.w_kv, bias=self.b_kv, batch=G, a_bs=0 if shared else T * Din, b_bs=ld * Din, c_bs=T * ld,
                          bias_bs=ld, M=T, N=ld, K=Din, out=new(G, T, ld))               # [G, T, L*2E]
        q = sd["query"].reshape(G, E)
        # member g's row of a [G, K] operand times its [N, K] weight (row stride K = batch stride: no [G, 1, K] views on the host path)
        bg = lambda a_, w_, b_, N_, K_, **kw: ops.gemm_f32(a_, w_, bias=b_, batch=G, a_bs=K_, b_bs=N_ * K_, c_bs=N_, bias_bs=N_,
                                                           M=1, N=N_, K=K_, out=new(G, N_), **kw)
        for i in range(self.L):
            p = f"blocks.{i}."
            q = ops.layernorm_f32_grouped(q, sd[p + "q_layer_norm.weight"], sd[p + "q_layer_norm.bias"], 1)
            qp = bg(q, sd[p + "attention.q_proj_weight"], self.q_b[i], E, E)
            k = kv[:, :, (2 * i) * E:(2 * i + 1) * E]
            v = kv[:, :, (2 * i + 1) * E:(2 * i + 2) * E]
            a = ops.mha_f32(qp, k, v, G, 1, T, H, E // H, (E, E), (T * ld, ld), (T * ld, ld))        # [G, 1, E]
            q = bg(a, sd[p + "attention.out_proj.weight"], sd[p + "attention.out_proj.bias"], E, E, residual=q)
            q = ops.layernorm_f32_grouped(q, sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1)
            F = sd[p + "mlp.fc1.weight"].shape[1]
            h = bg(q, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], F, E, act="gelu_erf")
            q = bg(h, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"], E, F, residual=q)
        return ops.layernorm_f32_grouped(q, sd["layer_norm.weight"], sd["layer_norm.bias"], 1)


class _Stack:
    """A trainable head of G >= 1 ensemble members as ONE chain of fp32 launches with the member index as the batch dimension
    of every GEMM / attention / norm: 1/G of the ~150 tiny launches of a member loop (a third at the headline's three members; the
    chains are latency-bound, ~10 us per launch, so this is ~3x off the verifier tail), same per-element arithmetic, bit-identical
    results. A lone member is a stack of one: the same launches as an unbatched chain (batch strides are not read at batch 1, save
    by the GEMM's plan, see tests/test_verifier_cpu.py). Members that cannot be stacked (`ok` False: other shapes, depths or
    encoder kinds) and COVER_MEMBER_BATCH=0 run `singles`, one stack of one per member, each into its member's slice of `out`."""

    def __init__(self, members: List[_Member]):
        self.G, self.dev = len(members), members[0].dev
        self.ok = self.G == 1 or self.stackable(members)
        if self.ok:
            self.build(members)
        self.singles = [self] if self.G == 1 else [type(self)([m]) for m in members]

    def __call__(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """run(a, b, out) of the subclass; out's leading dimension is the member."""
        if self.G == 1 or (self.ok and _member_batch()):
            self.run(a, b, out)
        else:
            for i, single in enumerate(self.singles):
                single.run(a, b, out[i:i + 1])
        return out


class _ImageTextStack(_Stack):
    """TextAwareVisualExtraction, the vision and text poolings and the input projection (efficient_ensemble_merged.py:216-223)."""

    @staticmethod
    def stackable(ms: List[_Member]) -> bool:
        return (_stackable([m.vision.sd for m in ms]) and _stackable([m.text.sd for m in ms]) and _stackable([m.ip for m in ms]) and
                len({(m.pos_emb.shape, m.vision.heads, m.text.heads) for m in ms}) == 1)

    def build(self, ms: List[_Member]):
        self.inv_temp = [m.inv_temp for m in ms]
        self.pos = _stack([m.pos_emb.reshape(-1, m.pos_emb.shape[-1]) for m in ms]).flatten(0, 1)                # [G*P, D]
        self.vision, self.text = _PoolingStack([m.vision for m in ms]), _PoolingStack([m.text for m in ms])
        self.ip_w, self.ip_b = _stack([m.ip["weight"] for m in ms]), _stack([m.ip["bias"] for m in ms])

    def run(self, pf: torch.Tensor, tf: torch.Tensor, out: torch.Tensor):
        """pf fp32 [P, D], tf fp32 [T, D] unit rows -> out fp32 [G, 512] unit rows."""
        G = self.G
        P, D = pf.shape
        T = tf.shape[0]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.dev)
        sim = ops.gemm_f32(tf, pf, batch=G, a_bs=0, b_bs=0, c_bs=T * P, M=T, N=P, K=D, out=new(G, T, P))   # the same product, one copy per member
        for gi in range(G):
            ops.softmax_rows_f32(sim[gi], self.inv_temp[gi])
        pfpe = ops.add_f32(self.pos, pf)                                                 # [G*P, D]: pos_emb[g] + pf (b rows cycle)
        taf = ops.gemm_f32(sim, pfpe, b_is_kn=True, batch=G, a_bs=T * P, b_bs=P * D, c_bs=T * D, M=T, N=D, K=P, out=new(G, T, D))
        vt = self.vision(taf, shared=False)
        tt = self.text(tf, shared=True)
        E1, E2 = tt.shape[1], vt.shape[1]
        comb = new(G, E1 + E2)
        comb[:, :E1].copy_(tt)     # cat([text_token, vision_token]) (device copies, no arithmetic)
        comb[:, E1:].copy_(vt)
        No = self.ip_w.shape[1]
        y = ops.gemm_f32(comb, self.ip_w, bias=self.ip_b, batch=G, a_bs=E1 + E2, b_bs=No * (E1 + E2), c_bs=No, bias_bs=No,
                         M=1, N=No, K=E1 + E2, out=new(G, No))
        ops.l2norm_rows_f32(y, out=out)


class _TrajectoryStack(_Stack):
    """The action encoder (efficient_ensemble_merged.py:226-245): per-step Linear + TransformerEncoder + masked mean, or the MLP
    `complex_action_encoder` over the flattened history (use_transformer = False), then the L2 norm."""

    @staticmethod
    def stackable(ms: List[_Member]) -> bool:
        return _stackable([m.se for m in ms]) and _stackable([m.traj for m in ms]) and _stackable([m.mlp for m in ms])

    def build(self, ms: List[_Member]):
        st = lambda sds: None if sds[0] is None else {k: _stack([sd[k] for sd in sds]) for k in sds[0]}
        self.se, self.w, self.mlp = st([m.se for m in ms]), st([m.traj for m in ms]), st([m.mlp for m in ms])
        self.layers = ms[0].traj_layers

    def run(self, hist: torch.Tensor, pad: torch.Tensor, out: torch.Tensor):
        """hist fp32 [N, 10, 7], pad uint8 [N, 10] -> out fp32 [G, N, 512] unit rows."""
        (self._transformer if self.mlp is None else self._mlp)(hist, pad, out)

    def _mlp(self, hist, pad, out):
        """Linear -> LayerNorm -> ReLU -> (Dropout) -> Linear -> L2 norm (:241-245); padding rows are plain inputs."""
        G, m = self.G, self.mlp
        N, K = hist.shape[0], hist.shape[1] * hist.shape[2]
        Hd, No = m["0.weight"].shape[1], m["4.weight"].shape[1]
        new = lambda cols: torch.empty(G * N, cols, dtype=torch.float32, device=self.dev)      # member g: rows g*N .. (g+1)*N - 1
        h = ops.gemm_f32(hist.view(N, K), m["0.weight"], bias=m["0.bias"], batch=G, a_bs=0, b_bs=Hd * K, c_bs=N * Hd, bias_bs=Hd,
                         M=N, N=Hd, K=K, out=new(Hd))
        h = ops.act_f32(ops.layernorm_f32_grouped(h, m["1.weight"], m["1.bias"], N), "relu")
        y = ops.gemm_f32(h, m["4.weight"], bias=m["4.bias"], batch=G, a_bs=N * Hd, b_bs=No * Hd, c_bs=N * No, bias_bs=No,
                         M=N, N=No, K=Hd, out=new(No))
        ops.l2norm_rows_f32(y, out=out.view(G * N, No))

    def _transformer(self, hist, pad, out):
        G, w, H = self.G, self.w, 8
        N, T, A = hist.shape
        E, R = self.se["weight"].shape[1], N * T
        new = lambda cols: torch.empty(G * R, cols, dtype=torch.float32, device=self.dev)      # member g: rows g*R .. (g+1)*R - 1
        x = ops.gemm_f32(hist.view(R, A), self.se["weight"], bias=self.se["bias"], batch=G, a_bs=0, b_bs=E * A, c_bs=R * E, bias_bs=E,
                         M=R, N=E, K=A, out=new(E))
        pad_g = pad if G == 1 else pad.repeat(G, 1).contiguous()
        for i in range(self.layers):
            p = f"layers.{i}."
            qkv = ops.gemm_f32(x, w[p + "self_attn.in_proj_weight"], bias=w[p + "self_attn.in_proj_bias"], batch=G,
                               a_bs=R * E, b_bs=3 * E * E, c_bs=R * 3 * E, bias_bs=3 * E, M=R, N=3 * E, K=E, out=new(3 * E))
            a = ops.mha_f32(qkv, qkv[:, E:], qkv[:, 2 * E:], G * N, T, T, H, E // H, (T * 3 * E, 3 * E), (T * 3 * E, 3 * E),
                            (T * 3 * E, 3 * E), key_pad=pad_g)                                                  # [G*N, T, E]
            y = ops.gemm_f32(a, w[p + "self_attn.out_proj.weight"], bias=w[p + "self_attn.out_proj.bias"],
                             residual=x, batch=G, a_bs=R * E, b_bs=E * E, c_bs=R * E, bias_bs=E, M=R, N=E, K=E, out=new(E))
            x = ops.layernorm_f32_grouped(y, w[p + "norm1.weight"], w[p + "norm1.bias"], R)
            F = w[p + "linear1.weight"].shape[1]
            h = ops.gemm_f32(x, w[p + "linear1.weight"], bias=w[p + "linear1.bias"], act="relu", batch=G, a_bs=R * E,
                             b_bs=F * E, c_bs=R * F, bias_bs=F, M=R, N=F, K=E, out=new(F))
            y = ops.gemm_f32(h, w[p + "linear2.weight"], bias=w[p + "linear2.bias"], residual=x, batch=G, a_bs=R * F,
                             b_bs=E * F, c_bs=R * E, bias_bs=E, M=R, N=E, K=F, out=new(E))
            x = ops.layernorm_f32_grouped(y, w[p + "norm2.weight"], w[p + "norm2.bias"], R)
        m = ops.masked_mean_f32(x, pad_g, G * N, T, E)
        ops.l2norm_rows_f32(m, out=out.view(G * N, E))


class VLASigLIP2Bridge:
    """One verifier model as it is trained and validated (bridge_verifier/ensemble_eval/finetune_trajectory_bridge_ddp.py:182-421):
    forward(image, text, action_histories) -> (image_logits, action_logits), both [B, B], for B DISTINCT (image, text, history)
    triples, and the symmetric InfoNCE loss + retrieval accuracies of its validation loop (:446-469, :1081-1090). Inference
    (eval) mode only: dropout is the identity, no gradients -- the optimiser side of training is outside the hot path.

    `component` is one entry of the merged checkpoint's `ensemble_components` (the trainable heads, merge_ensemble_checkpoints
    layout); `logit_scale` is the model's learned log-temperature (init 2.6592, :210)."""

    def __init__(self, component: dict, logit_scale: float = 2.6592, device="cuda:0", encoder: Optional["SigLIP2Encoder"] = None):
        L.lib()
        self.device = torch.device(device)
        self.member = _Member(component, self.device)
        self.image_text, self.trajectory = _ImageTextStack([self.member]), _TrajectoryStack([self.member])
        self.logit_scale = float(logit_scale)
        self.encoder = encoder
        self.history_length, self.action_dim = 10, 7

    def forward_features(self, patch_features, text_features, action_histories):
        """patch_features [B, P, D], text_features [B, T, D] (unit rows, what extract_features returns :297-355),
        action_histories [B, H, A] padded with the member's padding value -> (image_logits, action_logits) fp32 [B, B]."""
        pf = _f32(patch_features, self.device)
        tf = _f32(text_features, self.device)
        hist = _f32(torch.as_tensor(np.asarray(action_histories.cpu() if torch.is_tensor(action_histories) else action_histories)), self.device)
        B = pf.shape[0]
        if tf.shape[0] != B or hist.shape[0] != B:
            raise ValueError(f"batch sizes differ: images {B}, texts {tf.shape[0]}, histories {hist.shape[0]}")
        it = torch.empty(B, 512, dtype=torch.float32, device=self.device)
        for b in range(B):                                   # per-sample text-aware heads (:368-377)
            self.image_text(pf[b], tf[b], it[b:b + 1])
        pad = _pad_mask(hist, self.member.pad_value, self.device)                      # :384
        act = self.trajectory(hist.contiguous(), pad, torch.empty(1, B, 512, dtype=torch.float32, device=self.device))[0]   # :380-412
        scale = float(np.exp(np.float32(self.logit_scale)))                            # :414
        image_logits = ops.gemm_f32(it, act, alpha=scale)                              # :416
        action_logits = ops.gemm_f32(act, it, alpha=scale)                             # :417
        return image_logits, action_logits

    def forward(self, image, text, action_histories):
        if self.encoder is None:
            raise RuntimeError("VLASigLIP2Bridge.forward needs a SigLIP2Encoder; call forward_features with extracted features instead")
        pf, tf = self.encoder.extract_features(image, text)
        return self.forward_features(pf, tf, action_histories)

    __call__ = forward

    @staticmethod
    def contrastive_metrics(image_logits, action_logits, k_values=(1, 5)) -> Dict[str, float]:
        """loss = (CE(image_logits, arange) + CE(action_logits, arange)) / 2 (:895-899) and the top-k retrieval accuracies of
        calculate_accuracy_metrics (:446-469). Row statistics come from one kernel per direction; only the B-element means run on
        the host. Ties at the k-th place are broken towards the lower column (torch.topk leaves the order of equal values open)."""
        B = image_logits.shape[0]
        li, ri = ops.xent_diag_f32(image_logits)
        la, ra = ops.xent_diag_f32(action_logits)
        li, ri, la, ra = (t.cpu().numpy() for t in (li, ri, la, ra))
        out = {"image_loss": float(li.astype(np.float64).mean()), "action_loss": float(la.astype(np.float64).mean())}
        out["loss"] = 0.5 * (out["image_loss"] + out["action_loss"])
        for k in k_values:
            if k <= B:
                out[f"img2act_top{k}_acc"] = float((ri < k).mean())
                out[f"act2img_top{k}_acc"] = float((ra < k).mean())
        return out


class SigLIP2Encoder:
    """The frozen shared encoder: SigLIP2 ViT-L/16-384 image tower (patch features = the LAST block's attention-module
    output, forward hook at finetune_trajectory_bridge_ddp.py:272-274) and text tower (transformer output -> ln_final
    -> text_projection on all 64 positions, :318-330), both bf16, features cast to fp32 and L2-normalised per token.
    State dict: image.* / text.* in synth.vit_state layout; text.tok_emb [vocab, dim]; text.proj.{weight,bias}."""

    def __init__(self, sd: Dict[str, torch.Tensor], *, dim=1024, layers=24, heads=16, mlp=4096, patch=16, image=384,
                 context_length=64, device="cuda:0"):
        dev = torch.device(device)
        self.dev, self.dim, self.context_length, self.image_size = dev, dim, context_length, image
        self.num_patches = (image // patch) ** 2
        sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
        self.layers = layers
        self.image = VitTower(sub("image."), dim=dim, layers=layers, heads=heads, mlp=mlp, patch=patch, act="gelu_tanh",
                              eps=1e-6, device=device)
        tsd = sub("text.")
        tsd.setdefault("patch.weight", torch.zeros(dim, 3 * patch * patch))  # text tower has no patch embedding
        tsd.setdefault("patch.bias", torch.zeros(dim))
        self.text = VitTower(tsd, dim=dim, layers=layers, heads=heads, mlp=mlp, patch=patch, act="gelu_tanh", eps=1e-6,
                             device=device)
        self.tok_emb = sd["text.tok_emb"].to(BF).contiguous().to(dev)
        self.text_pos = sd["text.pos"].to(BF).contiguous().to(dev)
        self.text_proj = ops.pack_linear(sd["text.proj.weight"].to(dev), sd["text.proj.bias"])

    def extract_features(self, images: torch.Tensor, text: torch.Tensor, text_stream: Optional[torch.cuda.Stream] = None):
        """images fp32 [B,3,384,384] (open_clip-preprocessed), text int64 [B,64] -> (pf fp32 [B,P,D], tf fp32 [B,64,D]).
        text_stream: run the text tower there, beside the image tower on the current stream (the two towers are independent chains of
        launches that each fill a fraction of the chip); joined before returning."""
        B = images.shape[0]
        cur = torch.cuda.current_stream()
        ts = text_stream if text_stream is not None else cur
        if ts is not cur:
            ts.wait_stream(cur)
        with torch.cuda.stream(ts):
            T = text.shape[1]
            t = ops.embed_gather(self.tok_emb, text.reshape(-1).contiguous())
            ops.add_rows(t, self.text_pos[:T])
            t = self.text.forward(t.view(B, T, self.dim), post_ln=True)      # transformer -> ln_final
            tp = ops.gemm(t.view(B * T, self.dim), self.text_proj)           # text_projection (Linear)
            tf = ops.l2norm_rows_f32(ops.cast_bf16_to_f32(tp)).view(B, T, self.dim)
        x = self.image.embed(images.float().contiguous())
        a = self.image.forward(x, n_layers=self.layers, last_attn_only=True)
        pf = ops.cast_bf16_to_f32(a.view(B * self.num_patches, self.dim))
        pf = ops.l2norm_rows_f32(pf).view(B, self.num_patches, self.dim)
        if ts is not cur:
            cur.wait_stream(ts)
        return pf, tf


class EfficientEnsembleMerged:
    def __init__(self, merged_checkpoint, device="cuda:0", encoder: Optional[SigLIP2Encoder] = None,
                 preprocess: Optional[Callable] = None, tokenizer: Optional[Callable] = None):
        """merged_checkpoint: the already-loaded dict, or a path -- the directory written once by loaders.verifier_pt_to_safetensors, or the
        merged .pt itself, read with torch.load(weights_only=True) (efficient_ensemble_merged.py:37-53 unpickles it; this side never does). encoder/preprocess/tokenizer: the SigLIP2 towers and the open_clip
        CPU transforms are injected (they are un-vendored pip dependencies of the reference, :57,69)."""
        self.device = device
        self.last_member_stats = None            # the dict of the latest score_histories call that was given member_kappa
        self.last_smooth_stats = None            # the dict of the latest compute_max_similarity_scores_batch call that was given smooth
        dev = torch.device(device)
        if isinstance(merged_checkpoint, str):   # a converted directory (safetensors + JSON) or a .pt read WITHOUT arbitrary unpickling
            from .loaders import load_verifier_checkpoint
            ck = load_verifier_checkpoint(merged_checkpoint)
        else:
            ck = merged_checkpoint
        if "ensemble_components" in ck and "backbone" not in ck:
            self.backbone, self.use_transformer, self.history_length, self.action_dim = \
                "hf-hub:timm/ViT-L-16-SigLIP2-384", True, 10, 7
            self.num_models = len(ck["ensemble_components"])
        else:
            self.backbone, self.use_transformer = ck["backbone"], ck["use_transformer"]
            self.history_length, self.action_dim, self.num_models = ck["history_length"], ck["action_dim"], ck["num_models"]
        self.trainable_models = [_Member(c, dev) for c in ck["ensemble_components"]]
        self._traj_stack, self._it_stack = _TrajectoryStack(self.trainable_models), _ImageTextStack(self.trainable_models)
        self._shared_graphs = {}                 # shared_embeddings_graph's captured graphs by input shapes
        if preprocess is None:
            # open_clip's transform for the SigLIP2 checkpoints (:69) restated: Resize(BICUBIC, squash) + ToTensor + Normalize(.5)
            from .imaging import siglip_preprocess
            size = encoder.image_size if encoder is not None else 384
            preprocess = lambda im: siglip_preprocess(im, size)
        self.encoder, self.preprocess, self.tokenizer = encoder, preprocess, tokenizer
        self._dev = dev

    # ---- feature-level API (what the parity tests drive: tokenisation / resampling are inputs)
    def extract_shared_features(self, img_tensor, text_tokens):
        return self.encoder.extract_features(img_tensor.to(self._dev), text_tokens.to(self._dev))

    def _pad_histories(self, all_action_histories):
        """efficient_ensemble_merged.py:378-390: front pad with -5 to length 10 -> host fp32 [N, 10, 7] (`_pad_mask` makes the mask of :229)."""
        max_len = 10
        out = []
        for ah in all_action_histories:
            ah = np.array(ah)
            if len(ah) < max_len:
                ah = np.vstack([np.ones((max_len - len(ah), ah.shape[1])) * -5, ah])
            out.append(ah)
        hb = torch.tensor(np.array(out), dtype=torch.float32)
        return hb

    def get_embeddings_from_model_batch(self, model_idx, patch_features, text_features, action_histories_batch):
        m = self.trainable_models[model_idx]
        hb = action_histories_batch.float().to(self._dev).contiguous()
        pad = _pad_mask(action_histories_batch.cpu(), m.pad_value, self._dev)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=self._dev)
        it = self._it_stack.singles[model_idx](patch_features[0].contiguous(), text_features[0].contiguous(), new(1, 512))
        act = self._traj_stack.singles[model_idx](hb, pad, new(1, hb.shape[0], 512))[0]
        return it.expand(hb.shape[0], -1), act

    def shared_embeddings_graph(self, img_tensor: torch.Tensor, text_tokens: torch.Tensor) -> torch.Tensor:
        """image_text_embeddings(*extract_shared_features(img, text)) for ONE (image, instruction) pair, replayed as one hipGraph from the
        third call on, with the SigLIP2 image tower and text tower as parallel branches (ops.PooledGraph): ~600 launches become one host
        call, and the two towers -- 576 and 64 rows, a fraction of the chip each -- overlap. Same kernels, same results as the eager pair of
        calls. Returns the per-member embeddings [M, 512] (a static tensor, overwritten by the next call)."""
        key = (tuple(img_tensor.shape), tuple(text_tokens.shape))
        st = self._shared_graphs.get(key)
        if st is None:
            img = torch.empty_like(img_tensor, device=self._dev)
            txt = torch.empty_like(text_tokens, device=self._dev)
            side = torch.cuda.Stream(device=self._dev)

            def fn():
                pf, tf = self.encoder.extract_features(img, txt, text_stream=side)
                return self.image_text_embeddings(pf, tf)

            st = dict(img=img, txt=txt, g=ops.PooledGraph(fn, self._dev))
            self._shared_graphs[key] = st
        st["img"].copy_(img_tensor)
        st["txt"].copy_(text_tokens)
        return st["g"]()

    def image_text_embeddings(self, patch_features, text_features) -> torch.Tensor:
        """Per-member image-text embeddings [M, 512] of ONE (image, text) pair. Independent of the candidates, so a caller
        may run it (and extract_shared_features) on a side stream while the policy is still sampling."""
        pf = patch_features[0].to(self._dev).contiguous()
        tf = text_features[0].to(self._dev).contiguous()
        its = torch.empty(self.num_models, 512, dtype=torch.float32, device=self._dev)
        return self._it_stack(pf, tf, its)

    def score_histories(self, its: torch.Tensor, all_action_histories, group_size=1, pad: Optional[torch.Tensor] = None, *,
                        prior: Optional[torch.Tensor] = None, prior_beta: float = 0.0, length_normalize: bool = False,
                        prior_tokens: Optional[torch.Tensor] = None, pad_token_id: Optional[int] = None, top_m: int = 0,
                        member_kappa: Optional[float] = None, member_mode: str = "lcb", smooth: Optional[host.Smooth] = None):
        """Trajectory encoder per candidate + fusion + scoring + grouped arg-max against precomputed image-text embeddings.
        all_action_histories: list of [h<=10, 7] host arrays (reference format), OR an already padded DEVICE tensor
        fp32 [N,10,7] together with its padding mask `pad` uint8 [N,10] (ops.tokens_to_histories): no host round trip.
        prior (device fp32 [N] or [N, steps]: the candidates' log-probabilities under the policy, see ops.prior_select for the layouts,
        prior_tokens / pad_token_id and length_normalize) makes the decision the grouped arg-max of scores + prior_beta * prior: one
        ops.prior_select launch behind ops.score_select then supplies `result` / `best` (best[0] is the winner's COMBINED score) and the
        dict gains prior, combined, group_mean and ranked (the best top_m of the winning group). top_m > 0 without a prior ranks by the
        verifier score alone (beta 0). With prior None and top_m == 0 (the default) nothing else is launched or returned.
        member_kappa (finite, >= 0; None, the default, launches and returns nothing more) makes the decision disagreement-aware: one
        ops.member_scores call behind ops.score_select scores every candidate under every member on its own and the dict gains
        member_scores, mean, spread, min, min_member, robust, member_result and member_best. `result` / `best` are then the grouped
        arg-max of `robust` -- member_mode "lcb": scores - member_kappa * spread (the scores' own bits at member_kappa 0), "min": the
        worst member's score, member_kappa 0 -- while `scores` stays the fused score. With a prior or top_m as well, ops.prior_select
        is fed `robust` in place of `scores`: combined = robust + prior_beta * prior, and `result` / `best` come from it as above.
        The dict of the latest such call is kept as self.last_member_stats.
        smooth (a host.Smooth; None, the default, launches and returns nothing more) makes the decision neighbourhood-aware: one
        ops.smooth_scores_actions launch replaces every candidate's value -- `robust` with member_kappa, else `scores` -- by the
        kernel-weighted mean of its group's values over the history tensor itself (steps = its 10 rows; past rows and pads are equal
        within a group and contribute exact zeros, so the distance is that of the candidates' own steps in the verifier's input space),
        shrunk towards the group's mean. The dict gains smoothed, density, neighbours and smooth_group_mean; `result` / `best` are the
        grouped arg-max of `smoothed` while `scores` (and `robust`) stay what they were. With a prior or top_m as well, ops.prior_select
        is fed `smoothed`: combined = smoothed + prior_beta * prior. No radius, scale or shrink is recommended."""
        if smooth is not None and not isinstance(smooth, host.Smooth):
            raise L.CoverError("score_histories: smooth must be a host.Smooth or None")
        if torch.is_tensor(all_action_histories) and all_action_histories.is_cuda:
            hb = all_action_histories.contiguous()
        else:
            hb = self._pad_histories(all_action_histories)
            pad = _pad_mask(hb, self.trainable_models[0].pad_value, self._dev)
            hb = hb.to(self._dev).contiguous()
        N = hb.shape[0]
        # (members on separate HIP streams were tried: the tail shrinks 1.95 -> 1.47 ms but every decode pass of the policy
        # slows by ~0.17 ms with the extra queues alive -- a net loss, so the members share one chain of launches)
        acts = self._traj_stack(hb, pad, torch.empty(self.num_models, N, 512, dtype=torch.float32, device=self._dev))
        scores, result, best, fit, fact = ops.score_select(its, acts, group_size)
        out = {"scores": scores, "result": result, "best": best, "its": its, "acts": acts, "fused_it": fit, "fused_act": fact}
        base = scores                   # what the prior is added to and the ranking is made on
        if member_kappa is not None:
            out.update(ops.member_scores(its.contiguous(), acts, scores, group_size, member_kappa, member_mode))   # result / best: the robust decision
            base = out["robust"]
        if smooth is not None:
            base, st = ops.smooth_scores_actions(hb, base, group_size, stats=True, **smooth.kwargs(self._dev))
            out.update(smoothed=base, density=st.density, neighbours=st.neighbours, smooth_group_mean=st.group_mean)
            if prior is None and not top_m:
                out["result"], out["best"] = ops.group_argmax(base, group_size)
        if prior is not None or top_m:
            if prior is None:           # rank by the verifier score alone: beta 0 never reads the (summed) prior into the decision
                sel = ops.prior_select(base, base, group_size, 0.0, top_m=top_m)
                del sel["prior"]        # (the scores stood in for the unread log-probabilities)
            else:
                sel = ops.prior_select(base, prior, group_size, prior_beta, tokens=prior_tokens, pad_token_id=pad_token_id,
                                       length_normalize=length_normalize, top_m=top_m)
            out.update(sel)
        if member_kappa is not None:
            self.last_member_stats = out
        return out

    def score_refined(self, its: torch.Tensor, candidates, group_rows: int, *, to_histories, refine, normals, n_elite: int, prior_fn=None,
                      **score_kw):
        """Verifier-guided refinement, the loop: score, then per entry of `normals` one round of the cross-entropy method -- keep every
        prompt's n_elite best rows, refit the proposal on them, draw new rows, score again. Nothing but the composition of existing calls;
        the policy is not run. candidates: the rows in the policy's own form (OpenVLA: int64 tokens [P * group_rows, n_gen]), group_rows
        per prompt. to_histories(cands) -> (hb, pad), what score_histories takes (ops.tokens_to_histories with the model's table and the
        past actions). refine(cands, values, group_rows, n_elite, z) -> the n_elite + z.shape[1] rows per prompt, elites first
        (OpenVLA.refine), or (rows, elites) with elites.rows their indices in cands (OpenVLA.refine(elites=True)). normals: a sequence of R
        device tensors fp32 [P, K_r, steps, 6], one per round (host.augmentation_normals with a fresh seed each). prior_fn(cands,
        group_rows, n_fit) -> the [N] prior of that round's rows (OpenVLA.proposal_prior; n_fit is None in round 0, where the caller
        knows how its candidates were made, and n_elite later); None = no prior (a `prior` among score_kw is for the given candidates, so
        it is accepted only with an empty `normals`). score_kw goes to every score_histories call (member_kappa, member_mode, prior_beta,
        top_m, ...).
        Round 0 scores the given candidates. Each later round refines on the per-candidate value the previous decision was made on --
        `combined` if that dict has it, else `smoothed`, else `robust`, else `scores` -- and scores the new rows with group_size = n_elite + K_r. Returns the
        LAST score_histories dict plus `candidates` (the final rows, which `result` indexes) and `rounds` (per round, round 0 included, a
        dict of that round's `best`, `result` and `elite_rows`: None in round 0 and when refine returns no elites). The elites are
        carried verbatim, so a row-wise scorer's best value per prompt never decreases; no n_elite, K, round count or sigma is
        recommended. With an empty `normals` this is one score_histories call and nothing else is launched."""
        normals = list(normals)
        if "prior" in score_kw and (prior_fn is not None or normals):
            raise L.CoverError("score_refined: prior= belongs to the given candidates only; pass prior_fn to score refined rows under a prior")
        cands, S, n_fit, elite_rows, rounds = candidates, int(group_rows), None, None, []
        for r in range(len(normals) + 1):
            if r > 0:
                values = next(out[k] for k in ("combined", "smoothed", "robust", "scores") if k in out)
                z = normals[r - 1]
                got = refine(cands, values, S, n_elite, z)
                cands, elite_rows = (got[0], getattr(got[1], "rows", got[1])) if isinstance(got, tuple) else (got, None)
                S, n_fit = int(n_elite) + int(z.shape[1]), int(n_elite)
            hb, pad = to_histories(cands)
            kw = dict(score_kw)
            if prior_fn is not None:
                kw["prior"] = prior_fn(cands, S, n_fit)
            out = self.score_histories(its, hb, S, pad=pad, **kw)
            rounds.append({"best": out["best"], "result": out["result"], "elite_rows": elite_rows})
        out = dict(out)
        out["candidates"], out["rounds"] = cands, rounds
        return out

    def score_features(self, patch_features, text_features, all_action_histories, group_size=1, candidate_prior=None, prior_beta=0.0,
                       member_kappa=None, member_mode="lcb", smooth=None):
        """Scores every candidate history against ONE (image, text) pair given its features. Returns a dict with the
        device tensors (scores [N], result int32[4], best f32[2]) plus per-member embeddings. candidate_prior ([N] or [N, steps]
        log-probabilities, host or device) with prior_beta: the decision is made on scores + prior_beta * prior (score_histories).
        member_kappa / member_mode: the decision is made on the disagreement-aware robust score (score_histories). smooth (a
        host.Smooth): the decision is made on the neighbourhood-smoothed score (score_histories)."""
        if candidate_prior is not None:
            candidate_prior = torch.as_tensor(candidate_prior, dtype=torch.float32).to(self._dev)
        return self.score_histories(self.image_text_embeddings(patch_features, text_features), all_action_histories, group_size,
                                    prior=candidate_prior, prior_beta=prior_beta, member_kappa=member_kappa, member_mode=member_mode,
                                    smooth=smooth)

    def fuse_embeddings(self, image, instruction, action_histories):
        """efficient_ensemble_merged.py:249-293 -> (fused_image_text [N,512] (the one pair's embedding, a row per history),
        fused_action [N,512]). The reference stacks the histories with np.array (equal lengths, :267); shorter histories are
        front-padded here, which gives the same valid rows."""
        pf, tf = self._encode_pair(image, instruction)
        r = self.score_features(pf, tf, action_histories, 1)
        return r["fused_it"].view(1, -1).expand(r["fused_act"].shape[0], -1), r["fused_act"]

    def predict(self, image, instruction, possible_action_histories):
        """efficient_ensemble_merged.py:295-307."""
        pf, tf = self._encode_pair(image, instruction)
        scores = self.score_features(pf, tf, possible_action_histories, 1)["scores"].cpu().numpy()
        idx = scores.argmax()
        return possible_action_histories[idx], {str(i): float(scores[i]) for i in range(len(scores))}

    def _encode_pair(self, image, instruction):
        if self.encoder is None:
            raise L.CoverError("EfficientEnsembleMerged needs the SigLIP2 encoder for image/text inputs")
        if isinstance(image, np.ndarray):                      # efficient_ensemble_merged.py:252-253, 334-337
            from PIL import Image
            image = Image.fromarray(image.astype("uint8"))
        img_tensor = self.preprocess(image).unsqueeze(0)
        if isinstance(instruction, str):
            if self.tokenizer is None:
                raise L.CoverError("EfficientEnsembleMerged needs a tokenizer for string instructions (open_clip's is un-vendored)")
            toks = self.tokenizer([instruction], context_length=self.encoder.context_length)
        else:
            toks = instruction if instruction.ndim > 1 else instruction.unsqueeze(0)
        return self.extract_shared_features(img_tensor, toks)

    def compute_max_similarity_scores_batch(self, images, instructions, all_action_histories,
                                            cfg_repeat_language_instructions=1, candidate_prior=None, prior_beta=0.0,
                                            member_kappa=None, member_mode="lcb", smooth=None):
        """efficient_ensemble_merged.py:309-454. The reference scores candidates against the FIRST (image, text) pair only
        (reference_scores = similarity_matrix[0], :421-425), on both of its encode paths, so one pair is encoded here.
        candidate_prior ([N] or [N, steps] policy log-probabilities) with prior_beta selects on score + prior_beta * prior; the
        returned max_score is then the winner's COMBINED score, not its cosine score. member_kappa (None = off) with member_mode
        selects on the disagreement-aware robust score (score_histories); the returned max_score is then the winner's ROBUST score --
        or, with a prior as well, its combined score robust + prior_beta * prior -- and the per-member figures are in
        self.last_member_stats. smooth (a host.Smooth; None = off) selects on the neighbourhood-smoothed score (score_histories); the
        returned max_score is then the winner's SMOOTHED score, or its combined score with a prior; the dict of that call is kept as
        self.last_smooth_stats."""
        group_size = cfg_repeat_language_instructions
        pf, tf = self._encode_pair(images[0], instructions[0])
        r = self.score_features(pf, tf, all_action_histories, group_size, candidate_prior=candidate_prior, prior_beta=prior_beta,
                                member_kappa=member_kappa, member_mode=member_mode, smooth=smooth)
        if smooth is not None:
            self.last_smooth_stats = r
        result = r["result"].cpu()
        best = r["best"].cpu()
        gidx, gbest = int(result[0]), int(result[1])
        all_same = len(set(instructions)) == 1 if isinstance(instructions[0], str) else False
        if all_same and len(images) > 1:
            max_instruction = instructions[0]
        else:
            max_instruction = instructions[min(gbest * group_size, len(instructions) - 1)]
        return float(best[0]), max_instruction, all_action_histories[gidx], torch.tensor(gidx, dtype=torch.int64)
