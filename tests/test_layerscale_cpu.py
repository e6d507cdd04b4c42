"""LayerScale without a GPU: config validation, the CPU reference tests/ref_layerscale.py against the
oracle, and the algebra the backward kernel relies on (include/vitmi.h, "LayerScale")."""
import functools

import pytest
import torch

import ref_layerscale as ref
from oracle import vit_ref
from vitmi.config import ViTConfig

CFG = dict(img_size=32, patch_size=8, embed_dim=128, depth=3, num_heads=2, num_classes=2)
MB = 6


@functools.lru_cache(maxsize=None)
def case():
    cfg = ViTConfig(**CFG, dtype="fp32")
    params = vit_ref.init_params(cfg, seed=0)
    img, tgt = vit_ref.synthetic_batch(cfg, MB)
    return cfg, params, img, tgt, vit_ref.forward_backward(img, tgt, params, cfg)


def test_config_validation():
    assert ViTConfig().init_values is None
    for v in (1e-5, 1e-4, 1.0, 0.0, -0.5):          # any finite float; 0.0 is a scale, not "off"
        assert ViTConfig(init_values=v).init_values == v
    assert ViTConfig(init_values=0.0).init_values is not None
    for v in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="init_values"):
            ViTConfig(init_values=v)
    a, b = ViTConfig(), ViTConfig(init_values=1e-4)
    assert a.flops_per_image_fwd() == b.flops_per_image_fwd()
    assert b.replace(dtype="fp32").init_values == 1e-4


def test_gammas_are_what_the_tests_need():
    cfg = ViTConfig(**CFG)
    g = ref.gammas(cfg, 5)
    assert list(g) == [f"blocks.{i}.ls{j}.gamma" for i in range(3) for j in (1, 2)]
    for t in g.values():
        assert t.shape == (128,) and t.dtype == torch.float32 and t[ref.ZERO_CHANNEL] == 0
        nz = torch.cat([t[:ref.ZERO_CHANNEL], t[ref.ZERO_CHANNEL + 1:]])
        assert (nz.abs() >= 0.25).all() and (nz.abs() <= 1.5).all()
    allg = torch.cat(list(g.values()))
    assert 0.15 < (allg < 0).float().mean().item() < 0.35
    assert all(torch.equal(a, b) for a, b in zip(g.values(), ref.gammas(cfg, 5).values()))


def test_gamma_one_is_the_oracle_bitwise():
    cfg, params, img, tgt, (l0, loss0, g0) = case()
    l1, loss1, g1 = ref.forward_backward(img, tgt, {**params, **ref.ones(cfg)}, cfg)
    assert torch.equal(l0, l1) and torch.equal(loss0, loss1)
    assert set(g1) == set(g0) | set(ref.gamma_names(cfg))
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


def test_gammas_move_the_logits():
    cfg, params, img, tgt, (l0, _, _) = case()
    l1, _, g1 = ref.forward_backward(img, tgt, {**params, **ref.gammas(cfg, 5)}, cfg)
    moved = (l1 - l0).abs().max().item()
    print(f"gammas move the logits by {moved:.3e}")
    assert moved > 1e-3
    # the zero channel has a gradient all the same
    assert all(g1[k][ref.ZERO_CHANNEL] != 0 for k in ref.gamma_names(cfg))


def test_dgamma_identity_float64():
    """dgamma[n] = rowdot(dW_eff[n], W[n]) + db_eff[n] * b[n], with dW_eff = g^T a and db_eff =
    colsum(g): equal to autograd's gradient of gamma in y = gamma * (a W^T + b), zero channel included;
    and dW = gamma o dW_eff, db = gamma o db_eff."""
    gen = torch.Generator().manual_seed(3)
    M, K, N = 37, 24, 16
    f64 = torch.float64
    a = torch.randn(M, K, generator=gen, dtype=f64)
    W = torch.randn(N, K, generator=gen, dtype=f64).requires_grad_()
    b = torch.randn(N, generator=gen, dtype=f64).requires_grad_()
    gamma = (0.25 + 1.25 * torch.rand(N, generator=gen, dtype=f64))
    gamma[::4] *= -1
    gamma[ref.ZERO_CHANNEL] = 0.0
    gamma.requires_grad_()
    g = torch.randn(M, N, generator=gen, dtype=f64)
    (gamma * (a @ W.t() + b)).backward(g)
    dW_eff, db_eff = g.t() @ a, g.sum(0)
    dgamma = (dW_eff * W.detach()).sum(1) + db_eff * b.detach()
    assert (dgamma - gamma.grad).abs().max().item() <= 1e-12
    assert gamma.grad[ref.ZERO_CHANNEL] != 0
    assert (gamma.detach()[:, None] * dW_eff - W.grad).abs().max().item() <= 1e-12
    assert (gamma.detach() * db_eff - b.grad).abs().max().item() <= 1e-12
    # the forward operand: (a W_eff^T + b_eff) is the scaled branch
    y_fold = a @ (gamma.detach()[:, None] * W.detach()).t() + gamma.detach() * b.detach()
    assert (y_fold - (gamma * (a @ W.t() + b)).detach()).abs().max().item() <= 1e-12
