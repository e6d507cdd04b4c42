"""CPU reference of patch dropout for the ViT path, built from the oracle's own pieces
(oracle/vit_ref.py: embed, dropout_hash, layer_norm) and tests/ref_droppath.py's block, without
editing the oracle.  TEST INFRASTRUCTURE ONLY.

Semantics (include/vitmi.h, "Patch dropout"): key(b, p) = dropout_hash(seed, PATCH_SITE, b, p);
sample b keeps the K = max(1, int(np * (1 - rate))) patches with the smallest (key, p) pairs, listed
in ascending patch order; the token tensor is the class token plus those patches' rows of the full
embedding (position embedding included), nothing rescaled, and everything downstream sees a model
with N = K + 1 (dropout and drop path hash by the rows of the shortened sequence).  Gradients come
from torch autograd."""
import numpy as np
import torch
import torch.nn.functional as F

import ref_droppath
from oracle import vit_ref

PATCH_SITE = 0x20000000


def kept(np_: int, rate: float) -> int:
    """K of timm's PatchDropout."""
    return max(1, int(np_ * (1.0 - rate)))


def keys(seed: int, B: int, np_: int) -> np.ndarray:
    """uint [B, np_]: the hash key of every (sample, patch)."""
    return vit_ref.dropout_hash(seed, PATCH_SITE, np.arange(B), np.arange(np_))


def keep_indices(seed: int, B: int, np_: int, K: int) -> np.ndarray:
    """int64 [B, K]: each sample's kept patch numbers, ascending (a stable argsort orders equal keys
    by the smaller patch number)."""
    return np.sort(np.argsort(keys(seed, B, np_), axis=1, kind="stable")[:, :K], axis=1)


def slot_indices(keep: np.ndarray, np_: int) -> np.ndarray:
    """int64 [B, np_]: the position of each patch in its sample's keep row, -1 when dropped."""
    B, K = keep.shape
    slot = np.full((B, np_), -1, dtype=np.int64)
    slot[np.arange(B)[:, None], keep] = np.arange(K)[None, :]
    return slot


def gather_tokens(x: torch.Tensor, keep: np.ndarray) -> torch.Tensor:
    """x [B, 1 + np, D] -> [B, 1 + K, D]: the class token and the kept patches' rows."""
    B = x.shape[0]
    rows = torch.from_numpy(np.concatenate([np.zeros((B, 1), dtype=np.int64), 1 + keep], axis=1))
    return x[torch.arange(B)[:, None], rows]


def forward(img, p, cfg, seed=None):
    """Logits of a training-mode forward with patch dropout at cfg.patch_drop_rate (``seed`` None:
    inference, nothing drops)."""
    x = vit_ref.embed(img, p, cfg)
    np_ = x.shape[1] - 1
    K = kept(np_, cfg.patch_drop_rate)
    if seed is not None and K < np_:
        x = gather_tokens(x, keep_indices(seed, x.shape[0], np_, K))
    for i in range(cfg.depth):
        x = ref_droppath.block(x, p, i, cfg, seed)
    cls = x[:, 0] if cfg.with_cls_token else x.mean(dim=1)
    cls = vit_ref.layer_norm(cls, p["norm.weight"], p["norm.bias"], cfg.ln_eps)
    return F.linear(cls, p["head.weight"], p["head.bias"])


def forward_backward(img, target, p, cfg, seed=None):
    """(logits, loss, {name: grad}) of one CPU step, like vit_ref.forward_backward."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits = forward(img, leaves, cfg, seed)
    loss = vit_ref.loss_fn(logits, target, cfg.num_classes)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad.detach() for k, v in leaves.items()}
