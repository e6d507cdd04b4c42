"""CPU-side checks of the weight-average entry points (include/vitmi.h: vitmi_adam_step_ema,
vitmi_ema_apply): host validation rejects bad arguments before any launch, and n == 0 is OK."""
from vitmi import _lib

OK_PTR = 4096          # never dereferenced: every call below fails validation first


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def test_adam_step_ema_rejects_bad_arguments():
    lib = _lib.lib()

    def call(p=OK_PTR, g=OK_PTR, m=OK_PTR, v=OK_PTR, ema=OK_PTR, lp=None, wd=0.0, mask=None, ctl=None, n=100,
             b1=0.9, b2=0.999, eps=1e-7, mom=0.99):
        return lib.vitmi_adam_step_ema(n, p, g, m, v, lp, 1e-3, b1, b2, eps, 1.0, wd, 1e-3, mask, ctl, ema, mom, None)

    for name in ("p", "g", "m", "v", "ema"):
        rejected(call(**{name: None}), b"null")
        rejected(call(**{name: OK_PTR + 8}), b"16-byte")
    rejected(call(lp=OK_PTR + 2), b"8-byte")
    rejected(call(ctl=OK_PTR + 8), b"16-byte")
    rejected(call(n=-1), b"n < 0")
    for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(eps=-1e-7)):
        rejected(call(**kw), b"hyper-parameters")
    rejected(call(wd=-0.1), b"weight_decay")
    rejected(call(wd=float("nan")), b"weight_decay")
    for mom in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        rejected(call(mom=mom), b"ema_momentum")
    assert call(n=0) == 0                      # nothing to do
    assert call(n=0, mom=0.0) == 0


def test_ema_apply_rejects_bad_arguments():
    lib = _lib.lib()

    def call(p=OK_PTR, ema=OK_PTR, lp=None, mode=0, n=100):
        return lib.vitmi_ema_apply(n, p, ema, lp, mode, None)

    for name in ("p", "ema"):
        rejected(call(**{name: None}), b"null")
        rejected(call(**{name: OK_PTR + 8}), b"16-byte")
    rejected(call(lp=OK_PTR + 2), b"8-byte")
    rejected(call(n=-1), b"n < 0")
    for mode in (-1, 2, 3):
        rejected(call(mode=mode), b"mode")
    assert call(n=0) == 0
    assert call(n=0, mode=1) == 0


def test_signatures_are_in_the_table():
    assert {"vitmi_adam_step_ema", "vitmi_ema_apply"} <= set(_lib.exported_symbols())
