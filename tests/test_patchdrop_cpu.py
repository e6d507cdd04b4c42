"""CPU checks of patch dropout (no GPU, no library): the reference's subset selection pinned to
values computed from the oracle's hash, the number kept, the uniformity of the reference, and
ViTConfig's field, validation and FLOP count."""
import numpy as np
import pytest

import ref_patchdrop as ref
from vitmi.config import ViTConfig


def test_keep_indices_are_pinned():
    assert ref.keep_indices(11, 6, 16, 8).tolist() == [
        [8, 9, 10, 11, 12, 13, 14, 15],
        [1, 3, 4, 8, 10, 11, 12, 14],
        [0, 3, 4, 6, 9, 10, 12, 15],
        [0, 1, 6, 7, 11, 12, 14, 15],
        [1, 2, 3, 6, 8, 9, 11, 14],
        [0, 1, 3, 5, 7, 8, 9, 15]]
    assert ref.keep_indices(7, 5, 9, 6).tolist() == [
        [0, 1, 4, 5, 7, 8],
        [0, 2, 4, 5, 6, 8],
        [2, 3, 4, 5, 6, 8],
        [1, 3, 4, 5, 6, 7],
        [0, 1, 2, 4, 7, 8]]


def test_slot_is_the_inverse_of_keep():
    keep = ref.keep_indices(11, 6, 16, 8)
    slot = ref.slot_indices(keep, 16)
    assert ((slot >= 0).sum(axis=1) == 8).all()
    for b in range(6):
        assert slot[b, keep[b]].tolist() == list(range(8))


@pytest.mark.parametrize("np_,rate,K", [(9, 0.3, 6), (196, 0.25, 147), (196, 0.5, 98), (576, 0.75, 144),
                                        (16, 0.999, 1), (16, 0.01, 15)])
def test_number_kept(np_, rate, K):
    assert ref.kept(np_, rate) == K
    g = int(round(np_ ** 0.5))
    assert ViTConfig(img_size=g * 16, patch_size=16, patch_drop_rate=rate).kept_patches == K


@pytest.mark.parametrize("seed", [5, 11])
def test_reference_is_uniform(seed):
    B, np_, K = 4096, 196, 98
    k = ref.keys(seed, B, np_)
    assert all(len(np.unique(row)) == np_ for row in k)            # no sample has tied keys
    keep = ref.keep_indices(seed, B, np_, K)
    assert len({row.tobytes() for row in keep}) == B               # no two samples share an index row
    share = (ref.slot_indices(keep, np_) >= 0).mean(axis=0)
    print(f"seed {seed}: kept share per patch {share.min():.4f} .. {share.max():.4f}, sigma {share.std():.4f}")
    assert (np.abs(share - 0.5) <= 0.04).all()


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_config_refuses_rates_outside_0_1(bad):
    with pytest.raises(ValueError, match="patch_drop_rate"):
        ViTConfig(patch_drop_rate=bad)
    with pytest.raises(ValueError, match="patch_drop_rate"):
        ViTConfig().replace(patch_drop_rate=bad)


def test_config_field_and_flops():
    cfg = ViTConfig()
    assert cfg.patch_drop_rate == 0.0 and cfg.kept_patches == cfg.num_patches == 196
    for ok in (0.0, 0.25, 0.999):
        assert ViTConfig(patch_drop_rate=ok).patch_drop_rate == ok
    # the no-argument value is unchanged: ViT-B/16 224, 2 classes, restated from its definition
    D, N, F, L = 768, 197, 3072, 12
    full = 2.0 * (196 * 768 * D + L * (N * D * 3 * D + 2 * N * N * D + N * D * D + 2 * N * D * F) + D * 2)
    assert cfg.flops_per_image_fwd() == full
    assert cfg.flops_per_image_fwd(kept_patches=196) == full
    assert ViTConfig(patch_drop_rate=0.5).flops_per_image_fwd() == full    # the default counts the full sequence
    N = 99
    half = 2.0 * (98 * 768 * D + L * (N * D * 3 * D + 2 * N * N * D + N * D * D + 2 * N * D * F) + D * 2)
    assert cfg.flops_per_image_fwd(kept_patches=98) == half
    assert cfg.flops_per_image_fwd_bwd() == 3.0 * full
    assert 0.49 < half / full < 0.51
