"""CPU checks of stochastic depth (no GPU): the per-block schedule, ViTConfig validation, and that the
reference masks of the GPU tests' cases (tests/test_gpu_droppath.py) both keep and drop."""
import numpy as np
import pytest

import ref_droppath as ref
from oracle import vit_ref
from vitmi.config import ViTConfig


@pytest.mark.parametrize("depth,rate", [(12, 0.1), (3, 0.5), (24, 0.3), (2, 0.2)])
def test_schedule_is_linspace_with_block_0_at_zero(depth, rate):
    got = ViTConfig(depth=depth, drop_path_rate=rate).drop_path_rates()
    assert len(got) == depth and got[0] == 0.0
    np.testing.assert_allclose(got, np.linspace(0.0, rate, depth), rtol=1e-15, atol=0)
    assert got[-1] == pytest.approx(rate, rel=1e-15)


def test_schedule_edge_cases():
    assert ViTConfig(depth=1, drop_path_rate=0.3).drop_path_rates() == [0.0]      # linspace(0, r, 1) = [0]
    assert ViTConfig(depth=4).drop_path_rates() == [0.0] * 4
    assert ViTConfig().drop_path_rate == 0.0


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_config_refuses_rates_outside_0_1(bad):
    with pytest.raises(ValueError, match="drop_path_rate"):
        ViTConfig(drop_path_rate=bad)
    with pytest.raises(ValueError, match="drop_path_rate"):
        ViTConfig().replace(drop_path_rate=bad)


def test_config_accepts_the_range():
    for ok in (0.0, 0.1, 0.999):
        assert ViTConfig(drop_path_rate=ok).drop_path_rate == ok


def test_sites_are_disjoint_from_the_dropout_sites():
    depth = 48
    drop = {3 * i + j for i in range(depth) for j in range(3)}
    path = {ref.PATH_SITE0 + 2 * i + j for i in range(depth) for j in range(2)}
    assert len(path) == 2 * depth and not (drop & path)


def test_epilogue_case_mask_is_mixed():
    """seed 7, site 0x40000003, p = 0.25, the first 11 samples."""
    assert ref.mask_string(7, 0x40000003, 11, 0.25) == "11001010111"
    f = ref.sample_factor(7, 0x40000003, 11, 0.25)
    assert sorted(set(f.tolist())) == [0.0, pytest.approx(1 / 0.75)]


def test_model_case_masks_are_mixed():
    """depth 3, drop_path_rate 0.5, B = 6, seed 11: blocks 1 and 2 are active (rates 0.25, 0.5)."""
    r = ref.rates(0.5, 3)
    assert r == [0.0, 0.25, 0.5]
    got = [ref.mask_string(11, ref.PATH_SITE0 + 2 * i + j, 6, r[i]) for i in (1, 2) for j in (0, 1)]
    assert got == ["011110", "111010", "101000", "011100"]
    assert all("0" in m and "1" in m for m in got)


def test_statistics_case():
    """B = 4096, p = 0.1, seed 5, site 0x40000000: the kept share."""
    share = ref.keep_mask(5, ref.PATH_SITE0, 4096, 0.1).mean()
    assert abs(share - 0.9) < 0.01
    assert share == pytest.approx(0.9006, abs=5e-5)


def test_reference_at_rate_zero_is_the_oracle():
    import torch
    cfg = ViTConfig(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2, num_classes=2, dtype="fp32")
    params = vit_ref.init_params(cfg, seed=0)
    img, tgt = vit_ref.synthetic_batch(cfg, 3)
    l0, _, g0 = vit_ref.forward_backward(img, tgt, params, cfg)
    l1, _, g1 = ref.forward_backward(img, tgt, params, cfg, seed=11)
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
