"""CPU reference of stochastic depth (drop path) for the ViT path, built from the oracle's own
pieces (oracle/vit_ref.py: layer_norm, attention, mlp, embed, dropout_hash) without editing the
oracle.  TEST INFRASTRUCTURE ONLY.

Semantics (include/vitmi.h, "Stochastic depth"): sample b of drop-path site ``site`` is kept iff
dropout_hash(seed, site, b, 0) >= thresh, thresh = round(p * 2^32) as for dropout; its factor is
1/(1-p) if kept, else 0.  Block i uses site PATH_SITE0 + 2i for the attention branch and
PATH_SITE0 + 2i + 1 for the MLP branch, at rate linspace(0, drop_path_rate, depth)[i]; each branch
(after its element dropout, if any) is scaled by its sample's factor before the residual add.
Gradients come from torch autograd."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit_ref

PATH_SITE0 = 0x40000000


def rates(drop_path_rate: float, depth: int):
    """linspace(0, drop_path_rate, depth), as MS_CvT / timm build it."""
    return [float(r) for r in np.linspace(0.0, drop_path_rate, depth)]


def keep_mask(seed: int, site: int, B: int, p: float) -> np.ndarray:
    """bool [B]: which samples of the site are kept."""
    thresh, _ = vit_ref.dropout_params(p)
    return vit_ref.dropout_hash(seed, site, np.arange(B), np.array([0]))[:, 0] >= thresh


def sample_factor(seed: int, site: int, B: int, p: float) -> torch.Tensor:
    """float32 [B]: 1/(1-p) for kept samples, 0 for dropped ones."""
    _, scale = vit_ref.dropout_params(p)
    return torch.from_numpy(keep_mask(seed, site, B, p).astype(np.float32)) * scale


def mask_string(seed: int, site: int, B: int, p: float) -> str:
    return "".join("1" if k else "0" for k in keep_mask(seed, site, B, p))


def block(x, p, i, cfg, seed=None):
    """vit_ref.block with each branch scaled by its drop-path factor (``seed`` None: inference)."""
    pre = f"blocks.{i}."
    n2 = "norm1" if cfg.tie_norms else "norm2"
    drate = getattr(cfg, "drop_rate", 0.0)
    prate = rates(cfg.drop_path_rate, cfg.depth)[i]
    don = seed is not None and drate > 0
    da = (seed, 3 * i, drate) if don else None
    dm = (seed, 3 * i + 1, drate) if don else None
    B = x.shape[0]
    f1 = f2 = None
    if seed is not None and prate > 0:
        f1 = sample_factor(seed, PATH_SITE0 + 2 * i, B, prate).view(B, 1, 1)
        f2 = sample_factor(seed, PATH_SITE0 + 2 * i + 1, B, prate).view(B, 1, 1)
    a = vit_ref.attention(vit_ref.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], cfg.ln_eps),
                          p, pre, cfg, da)
    x = x + (a if f1 is None else a * f1)
    m = vit_ref.mlp(vit_ref.layer_norm(x, p[pre + n2 + ".weight"], p[pre + n2 + ".bias"], cfg.ln_eps), p, pre, dm)
    return x + (m if f2 is None else m * f2)


def forward(img, p, cfg, seed=None):
    """Logits; the head as vit_ref.forward does it."""
    x = vit_ref.embed(img, p, cfg)
    for i in range(cfg.depth):
        x = block(x, p, i, cfg, seed)
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
