"""CPU checks of the mixup / cutmix parameter draw (vitmi.augment.draw): pure NumPy on the host."""
import numpy as np
import pytest

from ref_loss import mix as mix_ref
from vitmi.augment import draw

f32 = np.float32


def tables(seed, B=16, H=32, W=48, **kw):
    return draw(B, H, W, np.random.default_rng(seed), **kw)


def test_same_seed_same_tables():
    for kw in ({}, {"per_sample": True}):
        a, b = tables(7, **kw), tables(7, **kw)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)
        c = tables(8, **kw)
        assert any(not np.array_equal(x, y) for x, y in zip(a, c))


def test_dtypes_shapes_and_permutation():
    perm, lam_mix, box, lam_t = tables(0, per_sample=True)
    assert perm.dtype == np.int32 and lam_mix.dtype == f32 and box.dtype == np.int32 and lam_t.dtype == f32
    assert perm.shape == (16,) and lam_mix.shape == (16,) and box.shape == (16, 4) and lam_t.shape == (16,)
    assert sorted(perm.tolist()) == list(range(16))


@pytest.mark.parametrize("H,W", [(32, 48), (7, 9), (224, 224)])
def test_boxes_inside_the_image_and_target_lam(H, W):
    n_cut = n_mix = 0
    for seed in range(20):
        perm, lam_mix, box, lam_t = draw(16, H, W, np.random.default_rng(seed), per_sample=True)
        y0, y1, x0, x1 = box.T
        assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
        assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
        assert ((0 <= lam_t) & (lam_t <= 1)).all() and ((0 <= lam_mix) & (lam_mix <= 1)).all()
        area = (y1 - y0) * (x1 - x0)
        for b in range(16):
            if area[b] > 0:        # cutmix: the image keeps lam 1 outside the box
                n_cut += 1
                assert lam_mix[b] == 1
                assert lam_t[b] == f32(1.0 - int(area[b]) / float(H * W))
            else:                  # mixup (or a cutmix whose box came out empty: lam 1 both ways)
                n_mix += 1
                assert lam_t[b] == lam_mix[b]
    assert n_cut > 40 and n_mix > 40       # switch_prob 0.5 over 320 draws


def test_alpha_switches():
    for seed in range(5):
        _, lam_mix, box, lam_t = tables(seed, cutmix_alpha=0.0, per_sample=True)     # mixup only
        assert not box.any() and np.array_equal(lam_mix, lam_t) and (lam_mix < 1).any()
        _, lam_mix, box, lam_t = tables(seed, mixup_alpha=0.0, per_sample=True)      # cutmix only
        assert (lam_mix == 1).all() and box.any()
        _, lam_mix, box, lam_t = tables(seed, mixup_alpha=0.0, cutmix_alpha=0.0)
        assert (lam_mix == 1).all() and (lam_t == 1).all() and not box.any()


def test_prob_zero_is_the_identity():
    for kw in ({}, {"per_sample": True}):
        perm, lam_mix, box, lam_t = tables(3, B=4, H=6, W=10, prob=0.0, **kw)
        assert (lam_mix == 1).all() and (lam_t == 1).all() and not box.any()
        img = np.random.default_rng(0).standard_normal((4, 3, 6, 10)).astype(f32)
        assert np.array_equal(mix_ref(img, perm, lam_mix, box), img)


def test_batch_mode_shares_one_draw_and_per_sample_differs():
    _, lam_mix, box, lam_t = tables(11)
    assert (lam_t == lam_t[0]).all() and (box == box[0]).all() and (lam_mix == lam_mix[0]).all()
    _, lam_mix, box, lam_t = tables(11, per_sample=True)
    assert len(set(lam_t.tolist())) > 8
