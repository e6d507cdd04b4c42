"""The reference's optimizer and learning-rate schedule on the fused vitmi kernel.

``model.compile(optimizer=keras.optimizers.Adam(learning_rate=1e-3), loss='mean_squared_error')``
(``models/CvT(Par).py:458-460``) and ``lr_scheduler`` (``:357-360``: x0.8 every 50 epochs).

``Adam`` runs Keras' update (include/vitmi.h ``vitmi_adam_step``): ONE launch over a model's
ParamArena (every parameter, gradient and moment at the same flat offsets), which also writes
the bf16 operand shadow the next forward's GEMMs read; models without an arena (the CvT) get
one launch per parameter tensor.

``global_clipnorm``, ``weight_decay`` and ``skip_nonfinite`` (all off by default) are decided on
the device: a fixed-order fp64 sum of squares of the gradients (``vitmi_grad_sumsq``), one
finalize launch that writes a 16-byte record (``vitmi_clip_finalize``), and the step reading it
(``vitmi_adam_step_ctl``).  No host read, no torch reduction kernel.

``use_ema`` keeps Keras' exponential moving average of the weights inside the same launch
(``vitmi_adam_step_ema``: the updated parameter is in a register, the average costs one 4-byte
read and one 4-byte write per parameter) and ``vitmi_ema_apply`` exchanges or copies it into the
parameters, bf16 shadow included, for evaluation.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from ._lib import check, lib

Tensor = torch.Tensor


def keras_alpha(lr: float, beta_1: float, beta_2: float, step: int) -> float:
    """alpha = lr sqrt(1 - b2^t) / (1 - b1^t), in float32 like Keras' update_step."""
    f = np.float32
    b1p = np.power(f(beta_1), f(step), dtype=np.float32)
    b2p = np.power(f(beta_2), f(step), dtype=np.float32)
    return float(f(lr) * np.sqrt(f(1) - b2p, dtype=np.float32) / (f(1) - b1p))


def ema_momentum_at(t: int, ema_momentum: Union[float, Callable[[int], float]]) -> float:
    """The momentum of the weight average at step ``t`` (1-based, ``Adam.iterations``): 0 at the
    first step (Keras' ``not_first_step``: the first average is the first updated weights),
    otherwise the value, or ``ema_momentum(t)`` for a callable, rounded once to float32.
    ``ValueError`` unless the rounded value is in [0, 1)."""
    x = ema_momentum(t) if callable(ema_momentum) else ema_momentum
    x = float(np.float32(x))
    if not 0.0 <= x < 1.0:
        raise ValueError(f"vitmi Adam: ema_momentum must be in [0, 1) as float32, got {x!r} at step {t}")
    return 0.0 if t == 1 else x


class Adam:
    """keras.optimizers.Adam(learning_rate, beta_1=0.9, beta_2=0.999, epsilon=1e-7,
    global_clipnorm=None, weight_decay=None, use_ema=False, ema_momentum=0.99,
    ema_overwrite_frequency=None).

    ``target``: a model with ``arena()`` (VisionTransformer: single fused launch + bf16 shadow
    refresh) or an iterable of parameters.  ``grad_scale`` multiplies the gradients as they are
    read (e.g. 1/world for a sum all-reduce).

    ``global_clipnorm``: the gradients of the parameters being stepped, times ``grad_scale``, are
    scaled by ``clipnorm / norm`` when their global L2 norm exceeds it (Keras' ``global_clipnorm``,
    torch's ``clip_grad_norm_``); the gradient buffers themselves are not modified.  Under data
    parallelism call ``step()`` after the reducer's ``finish()``: the norm is then over the reduced
    gradients and every rank decides alike.

    ``weight_decay``: decoupled, ``p -= p * weight_decay * lr`` before the Adam update, as Keras
    applies it.  It acts on the decay set: by default every parameter with ``ndim >= 2`` except a
    model's class token and position embedding; ``decay_filter(name, param) -> bool`` overrides
    that (the name is ``""`` for a plain parameter list).

    ``skip_nonfinite``: a step whose gradient norm is not finite leaves parameters and moments
    bit for bit as they were.  ``iterations`` still counts it, as Keras' own counter counts
    ``step()`` calls, and ``alpha`` follows ``iterations``: after a skipped step the bias
    correction runs slightly ahead of the moments, which errs towards a smaller step and vanishes
    as ``t`` grows.  ``skipped_steps`` reads the device counter (the only accessor that
    synchronises); ``last_clip()`` returns the last step's ``(norm, coef)`` as device tensors.

    ``use_ema``: an fp32 average of the parameters, ``e = momentum * e + (1 - momentum) * p`` after
    every update, three rounded fp32 operations inside the step's own launch.  It starts as a copy of
    the parameters; the momentum of step ``t`` is ``ema_momentum_at(t, ema_momentum)`` (a float in
    [0, 1) or a host callable ``t -> float``, e.g. a warm-up).  Parameters that are not stepped
    (frozen, or without a gradient) keep their average as it is, and so does every parameter across a
    step skipped by ``skip_nonfinite``.  ``ema_overwrite_frequency=k`` copies the average into the
    stepped parameters after every k-th step; ``finalize_variable_values()`` does so for all of them
    (``train.fit`` calls it after the last epoch, Keras' ``on_train_end``).  ``swap_ema()`` exchanges
    parameters and average in place and ``with opt.ema_weights():`` does so around a block (an
    evaluation), swapping back even when the block raises; inside the block ``step()``,
    ``state_dict()``, ``load_state_dict()``, ``swap_ema()`` and a nested ``ema_weights()`` raise.
    Only parameters are averaged and swapped: buffers such as BatchNorm moving statistics are not.
    ``state_dict()`` carries the average as ``"ema"``; a state without it loaded into a
    ``use_ema`` optimizer resets the average to the current parameters, so load the weights first,
    then the optimizer state."""

    def __init__(self, target, learning_rate: float = 1e-3, beta_1: float = 0.9, beta_2: float = 0.999,
                 epsilon: float = 1e-7, grad_scale: float = 1.0, global_clipnorm: Optional[float] = None,
                 weight_decay: float = 0.0, decay_filter: Optional[Callable[[str, Tensor], bool]] = None,
                 skip_nonfinite: bool = False, use_ema: bool = False,
                 ema_momentum: Union[float, Callable[[int], float]] = 0.99,
                 ema_overwrite_frequency: Optional[int] = None):
        self.learning_rate = float(learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self.grad_scale = float(grad_scale)
        if global_clipnorm is not None and not float(global_clipnorm) > 0.0:
            raise ValueError("vitmi Adam: global_clipnorm must be > 0 (None = off)")
        if not float(weight_decay) >= 0.0:
            raise ValueError("vitmi Adam: weight_decay must be >= 0")
        self.global_clipnorm = None if global_clipnorm is None else float(global_clipnorm)
        self.weight_decay = float(weight_decay)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.use_ema = bool(use_ema)
        if not callable(ema_momentum):
            ema_momentum_at(2, ema_momentum)        # validates
        self.ema_momentum = ema_momentum
        if ema_overwrite_frequency is not None:
            if isinstance(ema_overwrite_frequency, bool) or not isinstance(ema_overwrite_frequency, int) \
                    or ema_overwrite_frequency < 1:
                raise ValueError("vitmi Adam: ema_overwrite_frequency must be an int >= 1 (None = never)")
        self.ema_overwrite_frequency = ema_overwrite_frequency
        self.iterations = 0
        self._model = target if hasattr(target, "arena") else None
        if self._model is not None:
            arena = self._model.arena()
            self._arena = arena
            self.params: List[Tensor] = list(arena.params)
            self._m = torch.zeros_like(arena.flat)
            self._v = torch.zeros_like(arena.flat)
            names = {id(p): k for k, p in self._model.named_parameters()}
            no_decay = {id(getattr(self._model, k, None)) for k in ("cls_token", "pos_embed")}
        else:
            self._arena = None
            self.params = [p for p in target if p.requires_grad]
            self._m = [torch.zeros_like(p) for p in self.params]
            self._v = [torch.zeros_like(p) for p in self.params]
            names, no_decay = {}, set()
        if decay_filter is not None:
            self._decays = [bool(decay_filter(names.get(id(p), ""), p)) for p in self.params]
        else:
            self._decays = [p.ndim >= 2 and id(p) not in no_decay for p in self.params]
        # the average: a flat fp32 buffer at the arena's offsets, or one tensor per parameter
        self._ema = None
        if self.use_ema:
            self._ema = arena.flat.clone() if self._arena is not None else [p.detach().clone() for p in self.params]
        self._in_ema_weights = False
        self._mask: Optional[Tensor] = None       # arena: one byte per 64 elements, built once
        self._ctl: Optional[Tensor] = None        # the 16-byte device record (coef, norm, skip, skipped_total)
        self._partials: Optional[Tensor] = None   # fp64 chunk sums of every stepped run / tensor
        self._ov = None   # overlap_with state

    def overlap_with(self, red) -> None:
        """Step each gradient bucket of ``red`` (``vitmi.dp.attach``'s reducer) as soon as the
        backward has finished it (world 1) or its all-reduce has (the vitmi comm leg): the update
        of the blocks behind the backward runs on a side stream beside it, and ``step()`` only
        launches the rest and joins.  The update is the same launch over the same elements, in
        another order of ranges (elementwise, so bitwise the same result).  Needs one backward per
        ``step()`` (no gradient accumulation across backwards) and every arena parameter
        trainable; otherwise that step runs the plain single launch.  The learning rate is read
        when the backward finishes its first bucket."""
        if self._arena is None:
            raise ValueError("vitmi Adam.overlap_with: needs a model with a parameter arena")
        if self._use_ctl():
            raise ValueError("vitmi Adam.overlap_with: global_clipnorm / skip_nonfinite need the whole gradient "
                             "before the first update; the overlapped per-bucket update cannot use them")
        if red.flat.data_ptr() != self._arena.grad.data_ptr() or red.flat.numel() != self._arena.grad.numel():
            raise ValueError("vitmi Adam.overlap_with: the reducer is not over this model's gradient arena")
        self._ov = {"stream": torch.cuda.Stream(device=self._arena.flat.device), "done": 0, "alpha": None,
                    "lr": None, "mom": None, "skip": False}
        red.listeners.append(self._on_bucket)

    # -- clipping / decay / skipping state
    def _use_ctl(self) -> bool:
        return self.global_clipnorm is not None or self.skip_nonfinite

    def _ctl_record(self) -> Tensor:
        if self._ctl is None:
            dev = self._arena.flat.device if self._arena is not None else self.params[0].device
            self._ctl = torch.zeros(4, dtype=torch.float32, device=dev)
            if self._arena is not None:
                n_part = lib().vitmi_grad_sumsq_partials(self._arena.numel) + len(self.params)
            else:
                n_part = sum(lib().vitmi_grad_sumsq_partials(p.numel()) for p in self.params)
            self._partials = torch.zeros(max(1, n_part), dtype=torch.float64, device=dev)
        return self._ctl

    def _decay_mask(self) -> Tensor:
        if self._mask is None:
            arena = self._arena
            mask = torch.zeros(arena.numel // arena.ALIGN, dtype=torch.uint8)
            for p, dec in zip(arena.params, self._decays):
                if dec:
                    o = arena.offsets[id(p)] // arena.ALIGN
                    mask[o:o + (p.numel() + arena.ALIGN - 1) // arena.ALIGN] = 1
            self._mask = mask.to(arena.flat.device)
        return self._mask

    def _clip(self, grads: List[Tuple[Tensor, int]]) -> Tensor:
        """Sum of squares of every (flat gradient, n) into its slice of the partials buffer, then
        the finalize launch; returns the record the step launches read."""
        ctl = self._ctl_record()
        part, k = self._partials, 0
        for g, n in grads:
            check(lib().vitmi_grad_sumsq(n, ops._p(g), ops._p(part[k:]), ops._s()), "grad_sumsq")
            k += lib().vitmi_grad_sumsq_partials(n)
        check(lib().vitmi_clip_finalize(k, ops._p(part), self.grad_scale, self.global_clipnorm or 0.0,
                                        int(self.skip_nonfinite), ops._p(ctl), ops._s()), "clip_finalize")
        return ctl

    @property
    def skipped_steps(self) -> int:
        """Steps skipped so far on a non-finite gradient norm (reads the device: synchronises)."""
        if self._ctl is None:
            return 0
        return int(self._ctl.view(torch.int32)[3].item())

    def last_clip(self) -> Tuple[Tensor, Tensor]:
        """(norm, coef) of the last clipped step: device tensors, views of the record (no sync)."""
        ctl = self._ctl_record()
        return ctl[1], ctl[0]

    def _step_call(self, n: int, p, g, m, v, lp, alpha: float, lr: float, wd: float, mask, ctl, ema, mom) -> None:
        """One step launch over n elements; every buffer is a raw pointer or None.  The plain step
        when the optimizer has no average, no record and no weight decay, else the step with the
        average when there is one, else the step with the record, the decay or both."""
        head = (n, p, g, m, v, lp, alpha, self.beta_1, self.beta_2, self.epsilon, self.grad_scale)
        if ema is None and ctl is None and self.weight_decay == 0.0:
            check(lib().vitmi_adam_step(*head, ops._s()), "adam_step")
        elif ema is not None:
            check(lib().vitmi_adam_step_ema(*head, wd, lr, mask, ctl, ema, mom, ops._s()), "adam_step_ema")
        else:
            check(lib().vitmi_adam_step_ctl(*head, wd, lr, mask, ctl, ops._s()), "adam_step_ctl")

    def _launch(self, s0: int, e0: int, alpha: float, lr: Optional[float] = None,
                ctl: Optional[Tensor] = None, mom: Optional[float] = None) -> None:
        arena, lp = self._arena, self._arena.flat_lp
        mask = None
        if self.weight_decay != 0.0:
            if s0 % arena.ALIGN:
                raise RuntimeError("vitmi Adam: weight decay needs step ranges on 64-element boundaries")
            mask = ops._p(self._decay_mask()[s0 // arena.ALIGN:])
        self._step_call(e0 - s0, ops._p(arena.flat[s0:]), ops._p(arena.grad[s0:]), ops._p(self._m[s0:]),
                        ops._p(self._v[s0:]), ops._p(lp[s0:]) if lp is not None else None, alpha,
                        self.learning_rate if lr is None else lr, self.weight_decay, mask, ops._p(ctl),
                        ops._p(self._ema[s0:]) if self._ema is not None else None, mom)

    @torch.no_grad()
    def _on_bucket(self, s0: int, e0: int, stream) -> None:
        ov = self._ov
        if ov["skip"]:
            return
        if ov["alpha"] is None:
            # the first bucket of this backward
            if not all(p.requires_grad for p in self._arena.params) or s0 != 0:
                ov["skip"] = True
                return
            ov["alpha"] = keras_alpha(self.learning_rate, self.beta_1, self.beta_2, self.iterations + 1)
            ov["lr"] = self.learning_rate
            if self._ema is not None:
                ov["mom"] = ema_momentum_at(self.iterations + 1, self.ema_momentum)
        if s0 != ov["done"]:
            raise RuntimeError("vitmi Adam: gradient buckets finished out of order")
        side = ov["stream"]
        ready = torch.cuda.Event()
        ready.record(stream if stream is not None else torch.cuda.current_stream(self._arena.flat.device))
        side.wait_event(ready)
        with torch.cuda.stream(side):
            self._launch(s0, e0, ov["alpha"], ov["lr"], None, ov["mom"])
        ov["done"] = e0

    # -- keras-style schedule hook
    @property
    def lr(self) -> float:
        return self.learning_rate

    @lr.setter
    def lr(self, v: float) -> None:
        self.learning_rate = float(v)

    def zero_grad(self, set_to_none: bool = True) -> None:
        """torch's convention: drop the gradients (the next forward of an arena model zeroes the
        flat buffer once and the backward writes into it again), or zero them in place."""
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.zero_()

    @torch.no_grad()
    def step(self) -> None:
        self._not_in_ema_weights("step")
        # (a callable momentum out of range raises here, before the step is counted)
        mom = ema_momentum_at(self.iterations + 1, self.ema_momentum) if self._ema is not None else None
        self.iterations += 1
        alpha = keras_alpha(self.learning_rate, self.beta_1, self.beta_2, self.iterations)
        k = self.ema_overwrite_frequency
        overwrite = self._ema is not None and k is not None and self.iterations % k == 0
        if self._arena is not None:
            arena = self._model.arena()
            if arena is not self._arena:
                raise RuntimeError("vitmi Adam: the model's parameter arena was rebuilt after the optimizer "
                                   "was created (model moved?); create the optimizer after placing the model")
            # the launch reads the flat gradient buffer: every .grad must be its arena view (they
            # are after a backward from an arena forward; a gradient set elsewhere is copied in).
            # Parameters with no gradient (frozen, or zero_grad(set_to_none) and no backward) are
            # not stepped, as in torch / Keras: the launch covers the runs of the arena between them
            stepping = [p.requires_grad and p.grad is not None for p in arena.params]
            ov, done, lr = self._ov, 0, self.learning_rate
            if ov is not None:
                if self._use_ctl():
                    raise ValueError("vitmi Adam: global_clipnorm / skip_nonfinite cannot be used with overlap_with")
                done, ov_alpha, ov_lr, ov_mom = ov["done"], ov["alpha"], ov["lr"], ov["mom"]
                ov["done"], ov["alpha"], ov["lr"], ov["mom"], ov["skip"] = 0, None, None, None, False
                if done:
                    # the buckets the backward finished were stepped on the side stream
                    torch.cuda.current_stream(arena.flat.device).wait_stream(ov["stream"])
                    alpha, lr, mom = ov_alpha, ov_lr, ov_mom
            if not any(stepping):
                return
            lp = arena.flat_lp
            if not all(stepping):
                arena.refresh_lp()          # the skipped parameters' shadow must be current too
            arena.bind_grads(fill_missing=all(stepping))
            stepped = arena.runs(stepping)
            runs = [(max(s0, done), e0) for s0, e0 in stepped if e0 > max(s0, done)]
            # the norm is over the gradients of the parameters being stepped, and only those
            ctl = self._clip([(arena.grad[s0:], e0 - s0) for s0, e0 in runs]) if self._use_ctl() else None
            for s0, e0 in runs:
                self._launch(s0, e0, alpha, lr, ctl, mom)
            if overwrite:
                self._ema_apply(1, stepped)
            arena.mark_lp_fresh()
            return
        todo = [(p, m, v, dec) for p, m, v, dec in zip(self.params, self._m, self._v, self._decays)
                if p.grad is not None]
        for p, _, _, _ in todo:
            if not (p.is_contiguous() and p.grad.is_contiguous()):
                raise RuntimeError("vitmi Adam: parameters and gradients must be contiguous")
        if not todo:
            return
        ctl = self._clip([(p.grad, p.numel()) for p, _, _, _ in todo]) if self._use_ctl() else None
        emas = {id(p): e for p, e in zip(self.params, self._ema)} if self._ema is not None else {}
        for p, m, v, dec in todo:
            # a decaying tensor decays whole (NULL mask); one that does not gets weight_decay 0
            e = ops._p(emas[id(p)]) if self._ema is not None else None
            self._step_call(p.numel(), ops._p(p), ops._p(p.grad), ops._p(m), ops._p(v), None, alpha,
                            self.learning_rate, self.weight_decay if dec else 0.0, None, ops._p(ctl), e, mom)
            if overwrite:
                check(lib().vitmi_ema_apply(p.numel(), ops._p(p), e, None, 1, ops._s()), "ema_apply")
            # the kernel wrote through a raw pointer: bump the version counter, so a ParamArena
            # that owns p (its bf16 operand shadow is keyed on these counters) re-casts it
            torch.autograd.graph.increment_version(p)

    # -- the average of the weights
    def _need_ema(self, what: str) -> None:
        if self._ema is None:
            raise RuntimeError(f"vitmi Adam.{what}: the optimizer was created with use_ema=False")

    def _not_in_ema_weights(self, what: str) -> None:
        if self._in_ema_weights:
            raise RuntimeError(f"vitmi Adam.{what}: not inside ema_weights(): the parameters hold the average")

    def _ema_apply(self, mode: int, ranges: Optional[List[Tuple[int, int]]] = None) -> None:
        """vitmi_ema_apply (0: exchange, 1: p <- ema) over arena ranges (default: the whole arena),
        shadow included, or over every tensor of a parameter list."""
        if self._arena is not None:
            arena, lp = self._arena, self._arena.flat_lp
            if self._model.arena() is not arena:
                raise RuntimeError("vitmi Adam: the model's parameter arena was rebuilt after the optimizer "
                                   "was created (model moved?); create the optimizer after placing the model")
            for s0, e0 in ([(0, arena.numel)] if ranges is None else ranges):
                check(lib().vitmi_ema_apply(e0 - s0, ops._p(arena.flat[s0:]), ops._p(self._ema[s0:]),
                                            ops._p(lp[s0:]) if lp is not None else None, mode, ops._s()),
                      "ema_apply")
            if ranges is None:
                arena.mark_lp_fresh()
            return
        for p, e in zip(self.params, self._ema):
            if not p.is_contiguous():
                raise RuntimeError("vitmi Adam: parameters must be contiguous")
            check(lib().vitmi_ema_apply(p.numel(), ops._p(p), ops._p(e), None, mode, ops._s()), "ema_apply")
            torch.autograd.graph.increment_version(p)

    @torch.no_grad()
    def swap_ema(self) -> None:
        """Exchange parameters and average in place (one launch over the arena, bf16 shadow
        included; one per tensor for a parameter list).  Twice restores both."""
        self._need_ema("swap_ema")
        self._not_in_ema_weights("swap_ema")
        self._ema_apply(0)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with opt.ema_weights():`` the model computes with the averaged weights; the training
        weights come back on leaving, also when the block raises."""
        self._need_ema("ema_weights")
        self._not_in_ema_weights("ema_weights")
        with torch.no_grad():
            self._ema_apply(0)
        self._in_ema_weights = True
        try:
            yield self
        finally:
            self._in_ema_weights = False
            with torch.no_grad():
                self._ema_apply(0)

    @torch.no_grad()
    def finalize_variable_values(self) -> None:
        """Keras' name: every parameter becomes its average (the average stays)."""
        self._need_ema("finalize_variable_values")
        self._not_in_ema_weights("finalize_variable_values")
        self._ema_apply(1)

    @torch.no_grad()
    def reset_ema(self) -> None:
        """The average becomes a copy of the current parameters."""
        self._need_ema("reset_ema")
        self._not_in_ema_weights("reset_ema")
        if self._arena is not None:
            self._ema.copy_(self._arena.flat)
        else:
            for e, p in zip(self._ema, self.params):
                e.copy_(p.detach())

    def ema_parameters(self):
        """The average, as views: ``{name: tensor}`` for an arena model, a list aligned with
        ``params`` for a parameter list."""
        self._need_ema("ema_parameters")
        if self._arena is not None:
            return {k: self._arena.view(self._ema, p) for k, p in self._model.named_parameters()}
        return list(self._ema)

    # -- checkpointing (Keras saves the optimizer variables with the model weights)
    def state_dict(self) -> Dict:
        self._not_in_ema_weights("state_dict")
        if self._arena is not None:
            sd = {"iterations": self.iterations, "learning_rate": self.learning_rate, "m": self._m.clone(),
                  "v": self._v.clone()}
            if self._ema is not None:
                sd["ema"] = self._ema.clone()
            return sd
        sd = {"iterations": self.iterations, "learning_rate": self.learning_rate,
              "m": [t.clone() for t in self._m], "v": [t.clone() for t in self._v]}
        if self._ema is not None:
            sd["ema"] = [t.clone() for t in self._ema]
        return sd

    def load_state_dict(self, sd: Dict) -> None:
        self._not_in_ema_weights("load_state_dict")
        self.iterations = int(sd["iterations"])
        self.learning_rate = float(sd["learning_rate"])
        with torch.no_grad():
            if self._arena is not None:
                self._m.copy_(sd["m"])
                self._v.copy_(sd["v"])
            else:
                for dst, src in zip(self._m, sd["m"]):
                    dst.copy_(src)
                for dst, src in zip(self._v, sd["v"]):
                    dst.copy_(src)
            if self._ema is not None:
                if sd.get("ema") is None:
                    self.reset_ema()
                elif self._arena is not None:
                    self._ema.copy_(sd["ema"])
                else:
                    for dst, src in zip(self._ema, sd["ema"]):
                        dst.copy_(src)


def keras_step_decay(epoch: int, lr: float, every: int = 50, factor: float = 0.8) -> float:
    """lr_scheduler (models/CvT(Par).py:357-360): x0.8 at every 50th epoch (epoch > 0)."""
    if epoch > 0 and epoch % every == 0:
        return lr * factor
    return lr


__all__ = ["Adam", "ema_momentum_at", "keras_alpha", "keras_step_decay"]

