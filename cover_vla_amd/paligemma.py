"""The PaliGemma prefix that pi0 (pi0.py) and pi0-FAST (pi0fast.py) share: SigLIP tower -> projector -> image tokens, the token
embedding table, where both go in a [P, Tp, D] prefix buffer, the rule by which equal rows form a group, and the policies'
Normalize / Unnormalize pair. torch here allocates buffers and does index bookkeeping only; the arithmetic is libcover_hip.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from .models import BF, VitTower


def sub_state(sd: Dict[str, torch.Tensor], prefix: str) -> Dict[str, torch.Tensor]:
    """The entries of a neutral state dict under `prefix`, with the prefix removed."""
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def frames_shared(im: torch.Tensor) -> bool:
    """Is this camera's frame the same for every row (the evaluation driver's case: one observation, B candidates)?"""
    return bool(torch.equal(im[:1].expand_as(im), im))


def row_groups(*int_columns) -> Tuple[np.ndarray, np.ndarray]:
    """Rows that are equal in every column form a group; groups are numbered in order of first occurrence. Columns are integers
    [B] or [B, k] (tensors or arrays). Returns (first int64 [P]: the first row of each group, slot int64 [B]: the group of each row),
    so column[first][slot] == column. Host index bookkeeping on a few tens of KB: the ordering rule of pi0-FAST's greedy
    de-duplication and shared prefill and of pi0's (frames, prompt) de-duplication."""
    cols = [(c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)).astype(np.int64) for c in int_columns]
    cols = [c[:, None] if c.ndim == 1 else c for c in cols]
    if any(c.ndim != 2 or c.shape[0] != cols[0].shape[0] for c in cols):
        raise ValueError("row_groups: every column must be [B] or [B, k] over the same B rows")
    _, first, inv = np.unique(np.concatenate(cols, axis=1), axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)                             # distinct rows in order of first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(order.shape[0])
    return first[order].astype(np.int64), rank[inv.reshape(-1)].astype(np.int64)


class PaliGemmaPrefix:
    """SigLIP tower, projector and embedding table of one PaliGemma checkpoint, and the assembly of its prefix."""

    def __init__(self, sd: Dict[str, torch.Tensor], c: dict, *, device, n_cams: int):
        """sd: neutral state dict with vision.*, projector.*, lm.embed_tokens.weight; c: size dict."""
        self.dev = dev = torch.device(device)
        self.D = c["lm_dim"]
        self.n_img = (c["image"] // c["patch"]) ** 2
        self.n_cams = n_cams
        self.vit = VitTower(sub_state(sd, "vision."), dim=c["vit_dim"], layers=c["vit_layers"], heads=c["vit_heads"], mlp=c["vit_mlp"],
                            patch=c["patch"], act="gelu_tanh", eps=1e-6, device=device)
        self.projector = ops.pack_linear(sd["projector.weight"].to(dev), sd["projector.bias"])
        self.embed = sd["lm.embed_tokens.weight"].to(BF).contiguous().to(dev)
        self.emb_scale = float(torch.tensor(self.D ** 0.5, dtype=BF))     # GemmaModel: normalizer in the embedding dtype

    def image_tokens(self, img: torch.Tensor) -> torch.Tensor:
        """img fp32 [n,3,H,W] in [-1,1] -> bf16 [n, n_img, lm_dim]: tower -> projector -> / sqrt(D) (get_image_features, HF 4.48.3),
        then GemmaModel's * bf16(sqrt(D)) on the embedded sequence -- two bf16 roundings, as the reference's dtype flow has them
        (pi0: modeling_pi0.py:529-538, Appendix A.3 double rounding; pi0-FAST: modeling_pi0fast.py:888-946 embed_inputs)."""
        x = self.vit.embed(img.float().contiguous())
        x = self.vit.forward(x, post_ln=True)
        n, T, _ = x.shape
        y = ops.gemm(x.view(n * T, -1), self.projector)
        ops.scale_bf16(y, self.D ** 0.5, self.emb_scale)
        return y.view(n, T, self.D)

    def place(self, prefix: torch.Tensor, col: int, rows: torch.Tensor, *, by_index: bool = False,
              src_of_slot: Optional[torch.Tensor] = None) -> None:
        """Write rows bf16 [n, T, D] into columns [col, col + T) of every slot of prefix bf16 [P, Tp, D]: camera ci's image tokens at
        col = ci * n_img, the language embeddings behind the last camera. A device copy, no arithmetic. Two forms behind the one
        signature, because each model keeps the launches it has always issued (one cannot replace the other without changing a kernel):
          by_index False (pi0-FAST): one strided copy_; n == 1 is broadcast to the P slots, otherwise n == P.
          by_index True (pi0): ONE ops.copy_rows launch over index tensors; slot p takes rows[src_of_slot[p]] (int64 [P] on the
          device; None: n == P and slot p takes rows[p])."""
        P, Tp, D = prefix.shape
        T = rows.shape[1]
        if not by_index:
            prefix[:, col:col + T].copy_(rows.expand(P, -1, -1))
            return
        dev = prefix.device
        t = torch.arange(T, device=dev)
        sidx = None if src_of_slot is None else (t[None] + src_of_slot[:, None] * T).reshape(-1).to(torch.int32)
        didx = (torch.arange(P, device=dev)[:, None] * Tp + col + t[None]).reshape(-1)
        ops.copy_rows(rows.view(-1, D), prefix.view(-1, D), P * T, D, sidx, didx.to(torch.int32))


# ------------------------------------------------------------------------------ Normalize / Unnormalize (normalize.py:152-254)
IDENTITY = ("IDENTITY", None, None)


def _stats(x, triple):
    mode, a, b = triple
    if mode == "IDENTITY":
        return mode, None, None
    if mode not in ("MEAN_STD", "MIN_MAX"):
        raise ValueError(f"unknown normalization mode {mode!r}")
    return mode, a.to(x.device), b.to(x.device)


def normalize_state(x: torch.Tensor, triple) -> torch.Tensor:
    """triple = (mode, a, b): IDENTITY, MEAN_STD (a, b = mean, std) or MIN_MAX (a, b = min, max)."""
    mode, a, b = _stats(x, triple)
    if mode == "MEAN_STD":
        return (x - a) / (b + 1e-8)                       # normalize.py:169
    if mode == "MIN_MAX":
        return (x - a) / (b - a + 1e-8) * 2 - 1           # :177-179
    return x


def unnormalize_action(x: torch.Tensor, triple) -> torch.Tensor:
    mode, a, b = _stats(x, triple)
    if mode == "MEAN_STD":
        return x * b + a                                  # :243
    if mode == "MIN_MAX":
        return (x + 1) / 2 * (b - a) + a                  # :250-251
    return x
