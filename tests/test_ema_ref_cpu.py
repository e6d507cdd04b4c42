"""The reference of the weight average (tests/ref_ema.py) judged on its own: the float32 recurrence
against the same recurrence in float64, and the momentum rule (the product's
vitmi.optim.ema_momentum_at against the reference's)."""
import numpy as np
import pytest

import ref_ema
from vitmi import optim

f32 = np.float32


@pytest.mark.parametrize("mom", [0.0, 0.9, 0.99, 0.9999])
def test_fp32_recurrence_against_fp64(mom):
    """Each step rounds three times (two products, one sum), each by at most 2^-24 of a magnitude
    <= M, and an error made at step j is damped by mom^(k - j): at step k the distance is at most
    3 * 2^-24 * M * min(k, 1 / one_m).  Worst ratio to that bound on these inputs: 0, 0.28, 0.50
    and 0.35 for the four momenta."""
    rng = np.random.default_rng(int(mom * 10000))
    n, steps = 4096, 400
    m32 = f32(mom)
    one_m = f32(1) - m32
    e32 = rng.standard_normal(n).astype(f32)
    e64 = e32.astype(np.float64)
    M = float(np.abs(e32).max())
    worst = 0.0
    for k in range(1, steps + 1):
        p = rng.standard_normal(n).astype(f32)
        M = max(M, float(np.abs(p).max()))
        e32 = ref_ema.ema_update(e32, p, m32)
        assert e32.dtype == f32
        e64 = float(m32) * e64 + float(one_m) * p.astype(np.float64)
        bound = 3 * 2.0 ** -24 * M * min(k, 1.0 / float(one_m))
        err = float(np.abs(e32.astype(np.float64) - e64).max())
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
    print(f"momentum {mom}: worst ratio to the bound {worst:.3f}")


def test_momentum_zero_gives_the_new_weights():
    rng = np.random.default_rng(1)
    e, p = rng.standard_normal(1000).astype(f32), rng.standard_normal(1000).astype(f32)
    assert np.array_equal(ref_ema.ema_update(e, p, 0.0), p)


@pytest.mark.parametrize("fn", [ref_ema.momentum_at, optim.ema_momentum_at], ids=["reference", "vitmi.optim"])
def test_momentum_rule(fn):
    for x in (0.0, 0.5, 0.99, 0.9999, 1.0 / 3.0):
        assert fn(1, x) == 0
        for t in (2, 3, 1000):
            assert fn(t, x) == f32(x)
            assert f32(fn(t, x)) == f32(x)
    warm = lambda t: min(0.9999, (1 + t) / (10 + t))            # noqa: E731  (timm's warm-up)
    assert fn(1, warm) == 0
    for t in (2, 10, 100000):
        assert fn(t, warm) == f32(warm(t))
    for bad in (1.0, 1.5, -0.1, float("nan"), 1.0 - 1e-9):        # the last rounds to float32 1
        with pytest.raises(ValueError):
            fn(2, bad)
        with pytest.raises(ValueError):
            fn(5, lambda t: bad)


def test_product_and_reference_agree():
    for t in (1, 2, 7):
        for x in (0.0, 0.9, 0.99, 0.9999):
            assert f32(optim.ema_momentum_at(t, x)) == ref_ema.momentum_at(t, x)
    assert isinstance(optim.ema_momentum_at(2, 0.99), float)
