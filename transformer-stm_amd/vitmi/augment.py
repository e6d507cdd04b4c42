"""Mixup and cutmix batch augmentation (timm's ``Mixup`` rules) on the vitmi mix kernel
(vitmi_mix_batch, csrc/loss.hip).

The random parameters are drawn on the HOST with a seeded ``numpy.random.Generator`` and uploaded
(three small H2D copies; no device data is read back); the 154 MB image pass is one kernel.  The
labels are not mixed into a dense [B, C] target: ``losses.cross_entropy(logits, label_a,
target_b=label_b, lam=lam)`` takes the pair.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor

__all__ = ["Mixup", "draw"]


def _rand_box(H: int, W: int, lam: float, rng: np.random.Generator) -> Tuple[int, int, int, int]:
    """timm's rand_bbox: a box of side ratio sqrt(1 - lam), centred uniformly, clipped to the image."""
    ratio = np.sqrt(1.0 - lam)
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
    y0, y1 = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
    x0, x1 = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
    return int(y0), int(y1), int(x0), int(x1)


def draw(B: int, H: int, W: int, rng: np.random.Generator, *, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0,
         prob: float = 1.0, switch_prob: float = 0.5, per_sample: bool = False):
    """The per-sample tables of one batch, on the host:

    ``perm`` int32 [B] (a random permutation: sample b is mixed with sample perm[b]), ``lam_mix``
    fp32 [B] and ``box`` int32 [B, 4] = (y0, y1, x0, x1) for the image kernel, and ``lam_target`` fp32
    [B], the weight of the sample's own label.

    One draw for the whole batch, or one per sample with ``per_sample``.  With probability ``prob`` a
    draw mixes at all; it is cutmix with probability ``switch_prob`` when both alphas are positive.
    mixup: lam ~ Beta(a, a), empty box, lam_target = lam_mix = lam.  cutmix: lam ~ Beta(a, a) sizes
    the box, the image keeps lam_mix = 1 outside it, and lam_target = 1 - box_area / (H W) after
    clipping.  Not mixed: lam = 1 and an empty box (the kernel copies)."""
    perm = rng.permutation(B).astype(np.int32)
    lam_mix = np.ones(B, np.float32)
    lam_target = np.ones(B, np.float32)
    box = np.zeros((B, 4), np.int32)

    def one():
        if not (mixup_alpha > 0.0 or cutmix_alpha > 0.0) or rng.random() >= prob:
            return 1.0, 1.0, (0, 0, 0, 0)
        if mixup_alpha > 0.0 and cutmix_alpha > 0.0:
            cut = rng.random() < switch_prob
        else:
            cut = cutmix_alpha > 0.0
        a = cutmix_alpha if cut else mixup_alpha
        lam = float(rng.beta(a, a))
        if not cut:
            return lam, lam, (0, 0, 0, 0)
        y0, y1, x0, x1 = _rand_box(H, W, lam, rng)
        return 1.0, 1.0 - (y1 - y0) * (x1 - x0) / float(H * W), (y0, y1, x0, x1)

    if per_sample:
        for b in range(B):
            lam_mix[b], lam_target[b], box[b] = one()
    else:
        lam_mix[:], lam_target[:], box[:] = one()
    return perm, lam_mix, box, lam_target


class Mixup:
    """``mixed, label_a, label_b, lam = Mixup(...)(images, labels)``: images fp32 [B, C, H, W] and labels
    [B] on the device; ``label_a = labels``, ``label_b = labels[perm]`` and ``lam`` (fp32 [B]) the
    weight of ``label_a``, all on the device.  The generator is seeded once: successive calls give
    successive draws."""

    def __init__(self, mixup_alpha: float = 0.8, cutmix_alpha: float = 1.0, prob: float = 1.0,
                 switch_prob: float = 0.5, per_sample: bool = False, seed: int = 0):
        self.kw = dict(mixup_alpha=float(mixup_alpha), cutmix_alpha=float(cutmix_alpha), prob=float(prob),
                       switch_prob=float(switch_prob), per_sample=bool(per_sample))
        self.rng = np.random.default_rng(seed)

    def __call__(self, images: Tensor, labels: Tensor):
        B, _, H, W = images.shape
        perm, lam_mix, box, lam_target = draw(B, H, W, self.rng, **self.kw)
        dev = images.device
        perm_d = torch.from_numpy(perm).to(dev)
        mixed = ops.mix_batch(images.contiguous(), perm_d, torch.from_numpy(lam_mix).to(dev),
                              torch.from_numpy(box).to(dev))
        label_b = labels[perm_d.long()]          # B indices: not worth a kernel of its own
        return mixed, labels, label_b, torch.from_numpy(lam_target).to(dev)
