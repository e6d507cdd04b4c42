"""CPU reference of LayerScale for the ViT path, built from the oracle's own pieces (oracle/vit_ref.py:
layer_norm, attention, mlp, embed) and tests/ref_droppath.py's sample factors, without editing the
oracle.  TEST INFRASTRUCTURE ONLY.

Semantics (include/vitmi.h, "LayerScale"): block i with parameters ``blocks.i.ls1.gamma`` /
``blocks.i.ls2.gamma`` (fp32 [D]) computes

    x1  = x  + f1[b] * (gamma1 * attention(norm1(x)))      attention / mlp: vit_ref's, their element
    out = x1 + f2[b] * (gamma2 * mlp(norm2(x1)))           dropout included

so the order is dropout -> gamma -> drop-path sample factor; with no dropout and f = 1 this is timm's
``x + drop_path(ls(branch))``.  LayerScale acts the same with ``seed`` None (inference).  Gradients come
from torch autograd."""
import torch
import torch.nn.functional as F

import ref_droppath
from oracle import vit_ref

ZERO_CHANNEL = 3


def gamma_names(cfg):
    return [f"blocks.{i}.ls{j}.gamma" for i in range(cfg.depth) for j in (1, 2)]


def gammas(cfg, seed: int):
    """{name: gamma [D]}: magnitudes uniform in [0.25, 1.5], each negative with probability 1/4,
    channel 3 of every gamma exactly 0."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in gamma_names(cfg):
        mag = 0.25 + 1.25 * torch.rand(cfg.embed_dim, generator=g)
        sign = torch.where(torch.rand(cfg.embed_dim, generator=g) < 0.25, -1.0, 1.0)
        t = (mag * sign).float()
        t[ZERO_CHANNEL] = 0.0
        out[name] = t.contiguous()
    return out


def ones(cfg):
    return {name: torch.ones(cfg.embed_dim) for name in gamma_names(cfg)}


def block(x, p, i, cfg, seed=None):
    """ref_droppath.block with each branch scaled by its gamma before the drop-path factor."""
    pre = f"blocks.{i}."
    n2 = "norm1" if cfg.tie_norms else "norm2"
    drate = getattr(cfg, "drop_rate", 0.0)
    prate = ref_droppath.rates(cfg.drop_path_rate, cfg.depth)[i]
    don = seed is not None and drate > 0
    da = (seed, 3 * i, drate) if don else None
    dm = (seed, 3 * i + 1, drate) if don else None
    B = x.shape[0]
    f1 = f2 = None
    if seed is not None and prate > 0:
        f1 = ref_droppath.sample_factor(seed, ref_droppath.PATH_SITE0 + 2 * i, B, prate).view(B, 1, 1)
        f2 = ref_droppath.sample_factor(seed, ref_droppath.PATH_SITE0 + 2 * i + 1, B, prate).view(B, 1, 1)
    a = vit_ref.attention(vit_ref.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], cfg.ln_eps),
                          p, pre, cfg, da)
    a = a * p[pre + "ls1.gamma"]
    x = x + (a if f1 is None else a * f1)
    m = vit_ref.mlp(vit_ref.layer_norm(x, p[pre + n2 + ".weight"], p[pre + n2 + ".bias"], cfg.ln_eps), p, pre, dm)
    m = m * p[pre + "ls2.gamma"]
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
    """(logits, loss, {name: grad}) of one CPU step, like vit_ref.forward_backward; ``p`` holds the
    model's parameters and the gammas."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits = forward(img, leaves, cfg, seed)
    loss = vit_ref.loss_fn(logits, target, cfg.num_classes)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad.detach() for k, v in leaves.items()}
