"""CPU-side checks of the LayerScale entry points (include/vitmi.h: vitmi_layerscale_fold, _bwd, _apply,
_dgamma): host validation rejects bad arguments with a message before any launch."""
from vitmi import _lib

OK_PTR = 4096          # never dereferenced: every call below fails validation first
F32, BF16 = 0, 1


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def fold(N=768, K=768, w=OK_PTR, gamma=OK_PTR, bias=OK_PTR, w_eff=OK_PTR, w_dtype=BF16, bias_eff=OK_PTR):
    return _lib.lib().vitmi_layerscale_fold(N, K, w, gamma, bias, w_eff, w_dtype, bias_eff, None)


def bwd(N=768, K=768, w=OK_PTR, bias=OK_PTR, gamma=OK_PTR, dw=OK_PTR, db=OK_PTR, dgamma=OK_PTR, scale=1):
    return _lib.lib().vitmi_layerscale_bwd(N, K, w, bias, gamma, dw, db, dgamma, scale, None)


def apply(M=64, N=128, x=OK_PTR, ldx=None, gamma=OK_PTR, y=OK_PTR, y_dtype=F32, ldy=None):
    return _lib.lib().vitmi_layerscale_apply(M, N, x, N if ldx is None else ldx, gamma, y, y_dtype,
                                             N if ldy is None else ldy, None)


def dgamma(M=64, N=128, dy=OK_PTR, lddy=None, x=OK_PTR, ldx=None, dg=OK_PTR, ws=OK_PTR, ws_bytes=1 << 30):
    return _lib.lib().vitmi_layerscale_dgamma(M, N, dy, N if lddy is None else lddy, x, N if ldx is None else ldx,
                                              dg, ws, ws_bytes, None)


def test_fold_rejects_null_pointers():
    for name in ("w", "gamma", "w_eff"):
        rejected(fold(**{name: None}), b"null")
    rejected(fold(bias=None), b"together")            # bias without bias_eff, and the reverse
    rejected(fold(bias_eff=None), b"together")


def test_fold_rejects_bad_shapes_and_dtypes():
    rejected(fold(N=0), b"N must be >= 1")
    rejected(fold(N=-3), b"N must be >= 1")
    for K in (0, -8, 4, 100, 770):
        rejected(fold(K=K), b"K must be")
    for dtype in (2, 3, 4, 5, -1):
        rejected(fold(w_dtype=dtype), b"w_dtype")
    rejected(fold(N=1 << 20, K=1 << 20), b"2^31")
    rejected(fold(w=OK_PTR + 4), b"aligned")
    rejected(fold(w_eff=OK_PTR + 8), b"aligned")


def test_bwd_rejects_bad_arguments():
    rejected(bwd(dw=None, db=None, dgamma=None), b"null")
    rejected(bwd(dw=None), b"null")                   # dgamma needs dw ...
    rejected(bwd(w=None), b"null")                    # ... and w
    rejected(bwd(bias=None), b"null")                 # dgamma with db needs the bias
    rejected(bwd(gamma=None), b"null")                # scaling needs gamma
    rejected(bwd(scale=2), b"scale_grads")
    rejected(bwd(N=0), b"N must be >= 1")
    for K in (0, 4, 100):
        rejected(bwd(K=K), b"K must be")
    rejected(bwd(dw=OK_PTR + 4), b"aligned")
    rejected(bwd(w=OK_PTR + 8), b"aligned")


def test_bwd_with_nothing_to_do_is_ok_without_a_launch():
    assert bwd(dgamma=None, scale=0) == 0             # frozen gamma, gradients in temporaries


def test_apply_rejects_bad_arguments():
    for name in ("x", "gamma", "y"):
        rejected(apply(**{name: None}), b"null")
    rejected(apply(y_dtype=3), b"dtype")
    rejected(apply(N=126), b"multiples of 4")
    rejected(apply(ldx=130), b"multiples of 4")
    rejected(apply(ldx=124), b"multiples of 4")       # ldx < N
    rejected(apply(ldy=64), b"multiples of 4")
    rejected(apply(x=OK_PTR + 4), b"alignment")
    rejected(apply(gamma=OK_PTR + 4), b"alignment")
    rejected(apply(y=OK_PTR + 4), b"alignment")
    rejected(apply(M=-1), b"negative")
    assert apply(M=0) == 0 and apply(N=0) == 0


def test_dgamma_rejects_bad_arguments():
    for name in ("dy", "x", "dg"):
        rejected(dgamma(**{name: None}), b"null")
    rejected(dgamma(N=126), b"multiples of 4")
    rejected(dgamma(lddy=124), b"multiples of 4")
    rejected(dgamma(ldx=130), b"multiples of 4")
    rejected(dgamma(dy=OK_PTR + 4), b"alignment")
    rejected(dgamma(M=-1), b"negative")
    need = _lib.lib().vitmi_layerscale_dgamma_workspace_size(2167, 320)
    assert need > 0 and need % (320 * 4) == 0
    rejected(dgamma(M=2167, N=320, ws_bytes=need - 1), b"workspace")
    rejected(dgamma(M=2167, N=320, ws=None), b"workspace")
    assert dgamma(M=0) == 0 and dgamma(N=0) == 0
    assert _lib.lib().vitmi_layerscale_dgamma_workspace_size(0, 320) == 0
