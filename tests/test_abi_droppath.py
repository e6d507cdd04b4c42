"""CPU-side checks of the stochastic-depth entry points (include/vitmi.h: vitmi_linear_fwd_droppath,
vitmi_droppath_apply): host validation rejects bad arguments with a message before any launch."""
from vitmi import _lib

OK_PTR = 4096          # never dereferenced: every call below fails validation first
F32, BF16, BF16F8 = 0, 1, 4
EPI_STORE, EPI_BIAS_GELU, EPI_RESIDUAL, EPI_AUX_TILED = 0, 1, 2, 0x100
THRESH = 1 << 30       # p = 0.25
SCALE = 1 / 0.75


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def fwd(dtype=BF16, M=197 * 4, N=128, K=128, x=OK_PTR, w=OK_PTR, bias=OK_PTR, y=OK_PTR, y_dtype=F32,
        epilogue=EPI_RESIDUAL, residual=OK_PTR, drop_thresh=0, rows_per_sample=197):
    return _lib.lib().vitmi_linear_fwd_droppath(dtype, M, N, K, x, w, bias, y, y_dtype, epilogue, residual, None, 0,
                                                7, 2, drop_thresh, 1.0, rows_per_sample, 0x40000001, THRESH, SCALE,
                                                None)


def apply(M=197 * 4, N=128, x=OK_PTR, ldx=None, y=OK_PTR, y_dtype=F32, ldy=None, rows_per_sample=197,
          drop_thresh=0):
    return _lib.lib().vitmi_droppath_apply(M, N, x, N if ldx is None else ldx, y, y_dtype, N if ldy is None else ldy,
                                           rows_per_sample, 7, 0x40000001, THRESH, SCALE, 2, drop_thresh, 1.0, None)


def test_linear_fwd_droppath_rejects_null_pointers():
    for name in ("x", "w", "y", "residual"):
        rejected(fwd(**{name: None}), b"null")


def test_linear_fwd_droppath_rejects_bad_sample_geometry():
    rejected(fwd(rows_per_sample=0), b"rows_per_sample must be >= 1")
    rejected(fwd(rows_per_sample=-197), b"rows_per_sample must be >= 1")
    rejected(fwd(M=197 * 4 + 1), b"not a multiple")
    rejected(fwd(M=200, rows_per_sample=197), b"not a multiple")
    # the multiply-high row -> sample mapping is exact only for M * rows_per_sample <= 2^32
    rejected(fwd(M=1 << 20, rows_per_sample=1 << 13), b"2^32")
    rejected(fwd(M=-197), b"negative")


def test_linear_fwd_droppath_takes_the_residual_epilogue_only():
    for epi in (EPI_STORE, EPI_BIAS_GELU, EPI_RESIDUAL | EPI_AUX_TILED, 3, 4):
        rejected(fwd(epilogue=epi), b"RESIDUAL")


def test_linear_fwd_droppath_follows_its_siblings_rules():
    rejected(fwd(dtype=BF16F8), b"dtype")                     # bf16 / fp32 operands only
    rejected(fwd(dtype=7), b"dtype")
    rejected(fwd(y_dtype=BF16), b"fp32")                      # the residual epilogue writes fp32
    rejected(fwd(K=100), b"K ")                               # k-major operands: K % 64 (bf16)
    rejected(fwd(dtype=F32, K=48), b"K ")                     # ... K % 32 (fp32)
    rejected(fwd(x=OK_PTR + 8), b"aligned")
    rejected(fwd(drop_thresh=THRESH, x=None), b"null")        # the combined form validates the same way


def test_droppath_apply_rejects_bad_arguments():
    rejected(apply(x=None), b"null")
    rejected(apply(y=None), b"null")
    rejected(apply(y_dtype=3), b"dtype")
    rejected(apply(N=126), b"multiples of 4")
    rejected(apply(ldx=130), b"multiples of 4")
    rejected(apply(ldx=124), b"multiples of 4")               # ldx < N
    rejected(apply(ldy=64), b"multiples of 4")
    rejected(apply(x=OK_PTR + 4), b"alignment")
    rejected(apply(y=OK_PTR + 4), b"alignment")
    rejected(apply(rows_per_sample=0), b"rows_per_sample must be >= 1")
    rejected(apply(M=197 * 4 + 3), b"not a multiple")
    rejected(apply(M=1 << 20, rows_per_sample=1 << 13), b"2^32")
    rejected(apply(M=-4, rows_per_sample=1), b"negative")
    rejected(apply(drop_thresh=THRESH, y_dtype=9), b"dtype")


def test_nothing_to_do_is_ok_without_a_launch():
    assert apply(M=0) == 0
    assert apply(N=0) == 0
    assert fwd(M=0) == 0
