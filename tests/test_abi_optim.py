"""CPU-side checks of the clipping / weight-decay entry points of the optimizer
(include/vitmi.h: vitmi_grad_sumsq, vitmi_clip_finalize, vitmi_adam_step_ctl) and of the plain
vitmi_adam_step, which shares its validation with the other two step entry points: host validation
rejects bad arguments before any launch, and the partials count is ceil(n / CHUNK)."""
import os
import re

from vitmi import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitmi.h")

OK_PTR = 4096          # never dereferenced: every call below fails validation first


def chunk() -> int:
    m = re.search(r"#define\s+VITMI_GRAD_SUMSQ_CHUNK\s+(\d+)", open(HEADER).read())
    assert m, "include/vitmi.h states the chunk size"
    return int(m.group(1))


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def test_chunk_is_a_power_of_two_multiple_of_64():
    c = chunk()
    assert c >= 64 and c % 64 == 0 and c & (c - 1) == 0


def test_partials_count():
    lib, c = _lib.lib(), chunk()
    assert lib.vitmi_grad_sumsq_partials(1) == 1
    assert lib.vitmi_grad_sumsq_partials(c) == 1
    assert lib.vitmi_grad_sumsq_partials(c + 1) == 2
    assert lib.vitmi_grad_sumsq_partials(0) == 0
    assert lib.vitmi_grad_sumsq_partials(10 * c - 1) == 10


def test_grad_sumsq_rejects_bad_arguments():
    lib = _lib.lib()
    rejected(lib.vitmi_grad_sumsq(100, None, OK_PTR, None), b"null")
    rejected(lib.vitmi_grad_sumsq(100, OK_PTR, None, None), b"null")
    rejected(lib.vitmi_grad_sumsq(100, OK_PTR + 4, OK_PTR, None), b"16-byte")
    rejected(lib.vitmi_grad_sumsq(100, OK_PTR, OK_PTR + 4, None), b"8-byte")
    rejected(lib.vitmi_grad_sumsq(-1, OK_PTR, OK_PTR, None), b"n < 0")


def test_clip_finalize_rejects_bad_arguments():
    lib = _lib.lib()
    rejected(lib.vitmi_clip_finalize(4, None, 1.0, 1.0, 0, OK_PTR, None), b"null")
    rejected(lib.vitmi_clip_finalize(4, OK_PTR, 1.0, 1.0, 0, None, None), b"null")
    rejected(lib.vitmi_clip_finalize(4, OK_PTR + 4, 1.0, 1.0, 0, OK_PTR, None), b"8-byte")
    rejected(lib.vitmi_clip_finalize(4, OK_PTR, 1.0, 1.0, 0, OK_PTR + 8, None), b"16-byte")
    rejected(lib.vitmi_clip_finalize(4, OK_PTR, 1.0, -1.0, 0, OK_PTR, None), b"clip_norm")
    rejected(lib.vitmi_clip_finalize(4, OK_PTR, 1.0, float("nan"), 0, OK_PTR, None), b"clip_norm")


def test_adam_step_ctl_rejects_bad_arguments():
    lib = _lib.lib()

    def call(p=OK_PTR, g=OK_PTR, m=OK_PTR, v=OK_PTR, lp=None, wd=0.0, mask=None, ctl=None, n=100):
        return lib.vitmi_adam_step_ctl(n, p, g, m, v, lp, 1e-3, 0.9, 0.999, 1e-7, 1.0, wd, 1e-3, mask, ctl, None)

    for name in ("p", "g", "m", "v"):
        rejected(call(**{name: None}), b"null")
        rejected(call(**{name: OK_PTR + 8}), b"16-byte")
    rejected(call(lp=OK_PTR + 2), b"8-byte")
    rejected(call(ctl=OK_PTR + 8), b"16-byte")
    rejected(call(wd=-0.1), b"weight_decay")
    rejected(call(wd=float("nan")), b"weight_decay")
    rejected(call(n=-1), b"n < 0")
    assert call(n=0) == 0                      # nothing to do


BAD_HYPER = (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan")), dict(eps=-1e-7))


def test_adam_step_rejects_bad_arguments():
    lib = _lib.lib()

    def call(p=OK_PTR, g=OK_PTR, m=OK_PTR, v=OK_PTR, lp=None, n=100, b1=0.9, b2=0.999, eps=1e-7):
        return lib.vitmi_adam_step(n, p, g, m, v, lp, 1e-3, b1, b2, eps, 1.0, None)

    def refused(rc, word):
        rejected(rc, word)
        assert lib.vitmi_last_error().startswith(b"adam_step: ")      # its own name, not a sibling's

    for name in ("p", "g", "m", "v"):
        refused(call(**{name: None}), b"null")
        refused(call(**{name: OK_PTR + 8}), b"16-byte")
    refused(call(lp=OK_PTR + 2), b"8-byte")
    refused(call(n=-1), b"n < 0")
    for kw in BAD_HYPER:
        refused(call(**kw), b"hyper-parameters")
    assert call(n=0) == 0                      # nothing to do


def test_adam_steps_judge_values_before_an_empty_range_and_pointers_after():
    """All three step entry points alike: n == 0 with a bad value argument is refused, under the
    entry point's own name; n == 0 with null pointers is OK."""
    lib = _lib.lib()
    hyper = dict(b1=0.9, b2=0.999, eps=1e-7)

    def plain(n, ptr, wd=0.0, mom=0.5, **kw):
        h = {**hyper, **kw}
        return lib.vitmi_adam_step(n, ptr, ptr, ptr, ptr, None, 1e-3, h["b1"], h["b2"], h["eps"], 1.0, None)

    def ctl(n, ptr, wd=0.0, mom=0.5, **kw):
        h = {**hyper, **kw}
        return lib.vitmi_adam_step_ctl(n, ptr, ptr, ptr, ptr, None, 1e-3, h["b1"], h["b2"], h["eps"], 1.0, wd, 1e-3,
                                       None, None, None)

    def ema(n, ptr, wd=0.0, mom=0.5, **kw):
        h = {**hyper, **kw}
        return lib.vitmi_adam_step_ema(n, ptr, ptr, ptr, ptr, None, 1e-3, h["b1"], h["b2"], h["eps"], 1.0, wd, 1e-3,
                                       None, None, ptr, mom, None)

    for name, call in (("adam_step", plain), ("adam_step_ctl", ctl), ("adam_step_ema", ema)):
        for kw in BAD_HYPER:
            rejected(call(0, OK_PTR, **kw), b"hyper-parameters")
            assert lib.vitmi_last_error().startswith(name.encode() + b": ")
        assert call(0, None) == 0
        assert call(0, OK_PTR + 8) == 0        # nor is alignment judged for an empty range
    for name, call in (("adam_step_ctl", ctl), ("adam_step_ema", ema)):
        rejected(call(0, OK_PTR, wd=-0.1), b"weight_decay")
        assert lib.vitmi_last_error().startswith(name.encode() + b": ")
    rejected(ema(0, OK_PTR, mom=1.0), b"ema_momentum")
    assert lib.vitmi_last_error().startswith(b"adam_step_ema: ")
