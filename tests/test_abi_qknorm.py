"""CPU-side checks of the QK-norm entry points (include/vitmi.h: vitmi_qknorm_fwd, _bwd): host validation
rejects every bad argument with a message before any launch, and M == 0 is a no-op."""
import pytest

import ref_qknorm as ref
from vitmi import _lib

A, B, C = 4096, 8192, 12288          # never dereferenced: every call below fails validation first or has M == 0
F32, BF16 = 0, 1
H, W = 12, 3 * 12 * 64


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def fwd(dtype=BF16, M=394, H=H, dh=64, qkv=A, ld=W, gq=C, bq=C, gk=C, bk=C, out=B, ldo=W, mean=C, rstd=C):
    return _lib.lib().vitmi_qknorm_fwd(dtype, M, H, dh, qkv, ld, gq, bq, gk, bk, 1e-6, out, ldo, mean, rstd, None)


def bwd(dtype=BF16, M=394, H=H, dh=64, qkv=A, ld=W, mean=C, rstd=C, gq=C, gk=C, dqkv=B, ldd=W, dgq=C, dbq=C, dgk=C,
        dbk=C, dbias=C, ws=C, ws_bytes=1 << 30):
    return _lib.lib().vitmi_qknorm_bwd(dtype, M, H, dh, qkv, ld, mean, rstd, gq, gk, dqkv, ldd, dgq, dbq, dgk, dbk,
                                       dbias, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [fwd, bwd], ids=["fwd", "bwd"])
def test_rejects_bad_shapes_and_dtypes(call):
    for dtype in (2, 3, 4, 5, -1):
        rejected(call(dtype=dtype), b"dtype must be")
    for dh in (32, 128, 0, 63):
        rejected(call(dh=dh), b"dh must be 64")
    for h in (0, -1, 33, 64):
        rejected(call(H=h), b"H must be in [1, 32]")
    rejected(call(M=-1), b"negative")
    strides = ("ld", "ldo") if call is fwd else ("ld", "ldd")
    for name in strides:
        rejected(call(**{name: W - 8}), b"row strides")               # below 3*H*dh
        rejected(call(**{name: W + 4}), b"row strides")               # bf16: not a multiple of 8
        rejected(call(dtype=F32, **{name: W + 2}), b"row strides")    # fp32: not a multiple of 4
    assert call(dtype=F32, M=0, **{strides[1]: W + 4}) == 0           # fp32: a multiple of 4 is enough


def test_fwd_rejects_bad_pointers():
    for name in ("qkv", "gq", "bq", "gk", "bk", "out", "mean", "rstd"):
        rejected(fwd(**{name: None}), b"null")
    for name in ("qkv", "out", "gq", "bq", "gk", "bk"):
        rejected(fwd(**{name: A + 8}), b"16-byte aligned")
    rejected(fwd(out=A), b"alias")
    rejected(fwd(qkv=B), b"alias")


def test_bwd_rejects_bad_pointers_and_workspaces():
    for name in ("qkv", "mean", "rstd", "gq", "gk", "dqkv"):
        rejected(bwd(**{name: None}), b"null")
    for name in ("qkv", "dqkv", "gq", "gk", "ws"):
        rejected(bwd(**{name: A + 8}), b"16-byte aligned")
    rejected(bwd(dqkv=A), b"alias")
    need = _lib.lib().vitmi_qknorm_bwd_workspace_size(394, H)
    assert need == ref.workspace_bytes(394, H) > 0
    rejected(bwd(ws_bytes=need - 1), b"workspace too small")
    rejected(bwd(ws=None), b"workspace too small")


def test_workspace_size_follows_the_launch_geometry():
    for M in (1, 3, 64, 394, 905, 50432):
        for h in (1, 2, 3, 5, 12, 16, 20, 31, 32):
            assert _lib.lib().vitmi_qknorm_bwd_workspace_size(M, h) == ref.workspace_bytes(M, h), (M, h)
    assert _lib.lib().vitmi_qknorm_bwd_workspace_size(394, 0) == 0
    assert _lib.lib().vitmi_qknorm_bwd_workspace_size(394, 33) == 0


def test_m_zero_is_ok_and_launches_nothing():
    # no pointer is looked at: NULL everywhere, no workspace
    none = dict(qkv=None, gq=None, gk=None, mean=None, rstd=None)
    assert fwd(M=0, bq=None, bk=None, out=None, **none) == 0
    assert bwd(M=0, dqkv=None, dgq=None, dbq=None, dgk=None, dbk=None, dbias=None, ws=None, ws_bytes=0, **none) == 0
    # the shape is still validated
    rejected(fwd(M=0, dh=32), b"dh must be 64")
    rejected(bwd(M=0, H=40), b"H must be in [1, 32]")
