"""Classification losses and metrics on the vitmi loss kernel (vitmi_softmax_xent, csrc/loss.hip).

``cross_entropy`` is softmax cross-entropy on class indices, on the mixed pair of mixup / cutmix
(``target``, ``target_b``, ``lam``) or on a dense soft target, with torch's ``label_smoothing``
rule: what ``tf.keras.losses.CategoricalCrossentropy(label_smoothing=)`` and timm's
``Mixup`` + ``SoftTargetCrossEntropy`` compute.  The loss and d loss / d logits come from one
launch; nothing is read back to the host.

``ClassMetrics`` owns the device record the same launch adds each batch to (loss sum, rows, top-1
and top-k hits); ``read()`` is the one host read, once per epoch.  ``accuracy`` scores a batch
without a loss (evaluation under ``no_grad``).

``modules.cross_entropy`` is the older, plain-label entry point and keeps its own kernel.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor

__all__ = ["cross_entropy", "accuracy", "ClassMetrics"]


class ClassMetrics:
    """The 32-byte device record ``struct { double loss_sum; uint64 rows, top1, topk; }`` of
    include/vitmi.h, zeroed.  Every ``cross_entropy(..., metrics=m)`` / ``accuracy(..., metrics=m)``
    call adds its batch on the device."""

    def __init__(self, device="cuda", topk: int = 5):
        if topk < 1:
            raise ValueError("ClassMetrics: topk must be >= 1")
        self.topk = int(topk)
        self.record = torch.zeros(4, dtype=torch.float64, device=device)   # 32 bytes, allocator-aligned

    def reset(self) -> None:
        self.record.zero_()

    def read(self) -> Dict[str, float]:
        """One host read: mean loss, top-1 and top-k accuracy over the rows seen since the last reset."""
        rec = self.record.cpu().numpy()
        rows, top1, topk = (int(x) for x in rec.view(np.uint64)[1:])
        if rows == 0:
            return {"loss": 0.0, "top1": 0.0, "topk": 0.0, "rows": 0}
        return {"loss": float(rec[0]) / rows, "top1": top1 / rows, "topk": topk / rows, "rows": rows}


def _metric_args(metrics: Optional[ClassMetrics], topk: int, C: int):
    if metrics is None:
        return None, 0
    return metrics.record, min(metrics.topk if topk is None else int(topk), C)


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label_a, label_b, lam, soft, smoothing, rec, topk):
        _, loss, dl = ops.softmax_xent(logits.float(), label_a, label_b, lam, soft, smoothing, topk, rec,
                                       want_row_loss=False)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl * g,) + (None,) * 7


def cross_entropy(logits: Tensor, target: Tensor, *, target_b: Optional[Tensor] = None,
                  lam: Optional[Tensor] = None, label_smoothing: float = 0.0,
                  metrics: Optional[ClassMetrics] = None, topk: Optional[int] = None) -> Tensor:
    """Mean softmax cross-entropy of ``logits`` [B, C].

    ``target``: class indices [B] (any integer dtype), or a dense float target [B, C] that need not
    sum to 1.  ``target_b`` with ``lam`` (fp32 [B], a float, or a 0-d tensor): the mixed pair, row b's
    target is ``lam[b] onehot(target[b]) + (1 - lam[b]) onehot(target_b[b])``.  ``label_smoothing`` in
    [0, 1) mixes the target with the uniform distribution (torch's rule).  ``metrics``: a
    ``ClassMetrics`` this batch is added to, scored against ``target`` (``topk`` defaults to the
    record's own k, capped at C); with a dense target the metrics need class indices, so they are not
    taken there."""
    if logits.dim() != 2:
        raise ValueError("cross_entropy: logits must be [B, C]")
    B, C = logits.shape
    dense = target.is_floating_point()
    if (target_b is None) != (lam is None):
        raise ValueError("cross_entropy: target_b and lam go together")
    if dense:
        if target_b is not None:
            raise ValueError("cross_entropy: a dense target takes no target_b / lam")
        if metrics is not None:
            raise ValueError("cross_entropy: metrics are scored against class indices; use accuracy()")
        if target.shape != logits.shape:
            raise ValueError("cross_entropy: a dense target must be [B, C]")
        return _XentFn.apply(logits, None, None, None, target, float(label_smoothing), None, 0)
    if target.shape != (B,):
        raise ValueError("cross_entropy: class indices must be [B]")
    if lam is not None:
        if not torch.is_tensor(lam):
            lam = torch.full((B,), float(lam), dtype=torch.float32, device=logits.device)
        elif lam.dim() == 0:
            lam = lam.to(device=logits.device, dtype=torch.float32).expand(B)
        if lam.shape != (B,) or target_b.shape != (B,):
            raise ValueError("cross_entropy: lam and target_b must be [B]")
    rec, k = _metric_args(metrics, topk, C)
    return _XentFn.apply(logits, target, target_b, lam, None, float(label_smoothing), rec, k)


def accuracy(logits: Tensor, labels: Tensor, topk: Optional[int] = None,
             metrics: Optional[ClassMetrics] = None) -> ClassMetrics:
    """Score ``logits`` [B, C] against ``labels`` [B] without a loss gradient: the same launch with
    no dlogits.  Adds the batch to ``metrics`` (a fresh record if None) and returns it; nothing is
    read back here."""
    if metrics is None:
        metrics = ClassMetrics(logits.device, topk=5 if topk is None else topk)
    rec, k = _metric_args(metrics, topk, logits.shape[1])
    ops.softmax_xent(logits.detach().float(), labels, topk=k, metrics=rec, want_row_loss=False, want_loss=False,
                     want_grad=False)
    return metrics
