"""Numpy float32 reference of the Adam step with the weight average (include/vitmi.h
vitmi_adam_step_ema; TEST INFRASTRUCTURE ONLY): oracle/optim_ref.adam_step, fed a gradient already
multiplied by the clip coefficient and parameters already decayed (as tests/test_gpu_optim_clip.py
does), followed by the three rounded operations of the average

    e = (mom * e) + (one_m * p_new),      one_m = float32(1) - float32(mom)

and Keras' momentum rule (0 at the first step, ``not_first_step``)."""
import numpy as np

from oracle.optim_ref import adam_step

f32 = np.float32


def momentum_at(t, ema_momentum):
    """float32 momentum of step t (1-based): 0 at t == 1, else the value (a callable: of t)."""
    x = f32(ema_momentum(t) if callable(ema_momentum) else ema_momentum)
    if not f32(0) <= x < f32(1):
        raise ValueError(f"ema momentum {x!r} outside [0, 1)")
    return f32(0) if t == 1 else x


def ema_update(e, p_new, mom):
    """Two products and one sum, each rounded to float32."""
    mom = f32(mom)
    one_m = f32(1) - mom
    e, p_new = np.asarray(e, f32), np.asarray(p_new, f32)
    return ((mom * e).astype(f32) + (one_m * p_new).astype(f32)).astype(f32)


def decayed(p, wd, lr, sel):
    """The three rounded fp32 ops of the decoupled decay, where sel."""
    p = np.asarray(p, f32)
    return np.where(sel, p - (p * f32(wd)) * f32(lr), p).astype(f32)


def adam_ema_step(p, g, m, v, e, lr, t, mom, grad_scale=1.0, coef=None, wd=0.0, sel=None):
    """One step: -> new (p, m, v, e).  ``mom`` is the momentum of this step as the kernel gets it
    (momentum_at's value).  coef: the clip coefficient (None: 1); sel: the decay set (None with
    wd != 0: every element)."""
    g = np.asarray(g, f32)
    if grad_scale != 1.0:
        g = g * f32(grad_scale)
    if coef is not None and f32(coef) != f32(1):
        g = g * f32(coef)
    if wd != 0.0:
        p = decayed(p, wd, lr, np.ones(g.shape, bool) if sel is None else sel)
    p, m, v = adam_step(p, g, m, v, lr, t)
    return p, m, v, ema_update(e, p, mom)
