"""CPU-side checks of the token-path, head, cast and loss entry points (include/vitmi.h: vitmi_patch_im2col,
vitmi_patch_embed_*, vitmi_tokens_assemble(_bwd), vitmi_head_fwd / _bwd, the casts, vitmi_dropout_apply):
host validation refuses a bad argument with VITMI_ERR_INVALID (1) and a message that names it, before any
launch.

Every refusal is paired with its valid neighbour, which must NOT return 1.  Where the neighbour can be a
call that does no work (B == 0, n == 0, M == 0) it is one, and runs everywhere.  The others would launch:
they are made only on a machine without a device, where the launch itself fails with VITMI_ERR_HIP (2),
which shows that validation let the call through; with a device present the same valid calls are made on
real buffers by tests/test_gpu_tokens_conformance.py."""
import torch

from vitmi import _lib

OK_PTR = 4096          # 16-byte aligned, never dereferenced
F32, BF16, X3, F8 = 0, 1, 3, 4
BIG = 1 << 30
NO_DEVICE = not torch.cuda.is_available()


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def served(call):
    """A valid call that would launch: made only where there is no device to launch on."""
    if NO_DEVICE:
        rc = call()
        assert rc != 1, (rc, _lib.lib().vitmi_last_error())


def no_work(rc):
    """A valid call of zero size: accepted, nothing launched."""
    assert rc == 0, (rc, _lib.lib().vitmi_last_error())


def im2col(dtype=BF16, B=2, C=3, S=32, P=8, img=OK_PTR, patches=OK_PTR):
    return _lib.lib().vitmi_patch_im2col(dtype, B, C, S, P, img, patches, None)


def embed_fwd(dtype=BF16, B=2, C=3, S=32, P=8, D=128):
    return _lib.lib().vitmi_patch_embed_fwd(dtype, B, C, S, P, D, OK_PTR, OK_PTR, None, None, None, OK_PTR, OK_PTR,
                                            OK_PTR, BIG, None)


def embed_bwd(dtype=BF16, B=2, C=3, S=32, P=8, D=128):
    return _lib.lib().vitmi_patch_embed_bwd(dtype, B, C, S, P, D, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR,
                                            OK_PTR, BIG, None)


def assemble(B=2, np_=16, D=128, tok=OK_PTR, cls=OK_PTR, pos=OK_PTR, x=OK_PTR):
    return _lib.lib().vitmi_tokens_assemble(B, np_, D, tok, cls, pos, x, None)


def assemble_bwd(B=2, np_=16, D=128, dx=OK_PTR, dtok=OK_PTR, dtok_lp=OK_PTR, dcls=OK_PTR, dpos=OK_PTR):
    return _lib.lib().vitmi_tokens_assemble_bwd(B, np_, D, dx, dtok, dtok_lp, dcls, dpos, None)


def head_fwd(B=4, D=64, C=3, ldy=None):
    return _lib.lib().vitmi_head_fwd(B, D, C, OK_PTR, D if ldy is None else ldy, OK_PTR, OK_PTR, OK_PTR, None)


def head_bwd(B=4, D=64, C=3, ldy=None):
    return _lib.lib().vitmi_head_bwd(B, D, C, OK_PTR, OK_PTR, D if ldy is None else ldy, OK_PTR, OK_PTR, OK_PTR,
                                     OK_PTR, None)


def dropout(M=4, N=8, dtype=F32):
    return _lib.lib().vitmi_dropout_apply(M, N, OK_PTR, 8, OK_PTR, dtype, 8, 1, 2, 3, 1.0, None)


def test_im2col_dtype_must_be_f32_or_bf16():
    for dtype in (7, 3, F8, 5, 2, -1):
        rejected(im2col(dtype=dtype), b"dtype")
    for dtype in (F32, BF16):
        no_work(im2col(dtype=dtype, B=0))
        served(lambda: im2col(dtype=dtype))


def test_im2col_sizes():
    rejected(im2col(B=-1), b"B >= 0")
    rejected(im2col(C=0), b"C > 0")
    rejected(im2col(C=-3), b"C > 0")
    rejected(im2col(S=0), b"S > 0")
    rejected(im2col(S=-32), b"S > 0")
    rejected(im2col(C=17, S=64, P=16), b"4096")
    no_work(im2col(B=0, C=1, S=4, P=4))
    served(lambda: im2col(B=1, C=1, S=4, P=4))
    served(lambda: im2col(C=16, S=64, P=16))


def test_im2col_alignment():
    rejected(im2col(img=OK_PTR + 4), b"aligned")
    rejected(im2col(img=OK_PTR + 8), b"aligned")
    rejected(im2col(patches=OK_PTR + 2), b"aligned")
    rejected(im2col(patches=OK_PTR + 4), b"aligned")
    rejected(im2col(dtype=F32, patches=OK_PTR + 8), b"aligned")
    no_work(im2col(B=0, patches=OK_PTR + 8))          # bf16 rows need 8 bytes only
    no_work(im2col(B=0, dtype=F32, patches=OK_PTR + 16))
    served(lambda: im2col(patches=OK_PTR + 8))


def test_patch_embed_dtype_must_be_f32_or_bf16():
    lib = _lib.lib()
    for dtype in (3, 7, F8, 5):
        rejected(embed_fwd(dtype=dtype), b"dtype")
        rejected(embed_bwd(dtype=dtype), b"dtype")
        assert lib.vitmi_patch_embed_fwd_workspace_size(dtype, 2, 3, 32, 8, 128) == 0
        assert lib.vitmi_patch_embed_bwd_workspace_size(dtype, 2, 3, 32, 8, 128) == 0
        assert lib.vitmi_patch_embed_keep_fwd_workspace_size(dtype, 2, 3, 32, 8, 128, 8) == 0
        rejected(lib.vitmi_patch_embed_keep_fwd(dtype, 2, 3, 32, 8, 128, 8, OK_PTR, OK_PTR, OK_PTR, None, None, None,
                                                OK_PTR, OK_PTR, OK_PTR, BIG, None), b"dtype")
        rejected(lib.vitmi_patch_embed_keep_bwd(dtype, 2, 3, 32, 8, 128, 8, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR,
                                                OK_PTR, OK_PTR, OK_PTR, BIG, None), b"dtype")
    for dtype in (F32, BF16):
        assert lib.vitmi_patch_embed_fwd_workspace_size(dtype, 2, 3, 32, 8, 128) > 0
        assert lib.vitmi_patch_embed_bwd_workspace_size(dtype, 2, 3, 32, 8, 128) > 0
        served(lambda: embed_fwd(dtype=dtype))


def test_tokens_assemble_sizes_and_alignment():
    rejected(assemble(B=-1), b"B >= 0")
    rejected(assemble(np_=-1), b"np >= 0")
    rejected(assemble(D=0), b"D > 0")
    rejected(assemble(D=-4), b"D > 0")
    rejected(assemble(D=126), b"D % 4")
    for name in ("tok", "cls", "pos", "x"):
        for off in (4, 8):
            rejected(assemble(**{name: OK_PTR + off}), b"aligned")
    rejected(assemble(tok=None), b"null")
    no_work(assemble(B=0))
    no_work(assemble(B=0, cls=None, pos=None, tok=OK_PTR + 16, x=OK_PTR + 32))
    served(lambda: assemble(B=1, np_=1, D=4))
    served(lambda: assemble(np_=0))


def test_tokens_assemble_bwd_sizes_and_alignment():
    rejected(assemble_bwd(B=-1), b"B >= 0")
    rejected(assemble_bwd(np_=-1), b"np >= 0")
    rejected(assemble_bwd(D=0), b"D > 0")
    rejected(assemble_bwd(D=126), b"D % 4")
    for name in ("dx", "dtok", "dcls", "dpos"):
        for off in (4, 8):
            rejected(assemble_bwd(**{name: OK_PTR + off}), b"aligned")
    rejected(assemble_bwd(dtok_lp=OK_PTR + 2), b"aligned")
    rejected(assemble_bwd(dtok_lp=OK_PTR + 4), b"aligned")
    rejected(assemble_bwd(dx=None), b"null")
    no_work(assemble_bwd(B=0))
    no_work(assemble_bwd(B=0, dtok_lp=OK_PTR + 8))     # the bf16 copy needs 8 bytes only
    no_work(assemble_bwd(B=0, dtok=None, dtok_lp=None, dcls=None, dpos=None))
    served(lambda: assemble_bwd(dtok_lp=OK_PTR + 8))
    served(lambda: assemble_bwd(B=1, np_=1, D=4))


def test_head_sizes():
    for call, name in ((head_fwd, b"head_fwd"), (head_bwd, b"head_bwd")):
        rejected(call(ldy=63), b"ldy >= D")
        rejected(call(ldy=0), b"ldy >= D")
        rejected(call(D=0, ldy=0), b"D > 0")
        rejected(call(D=-1), b"D > 0")
        rejected(call(B=0), name)
        rejected(call(B=-1), name)
        rejected(call(C=0), name)
        served(lambda: call())                          # ldy == D
        served(lambda: call(ldy=65))
        served(lambda: call(B=1, D=1, C=1))
    rejected(head_bwd(B=0), b"B > 0")
    rejected(head_bwd(C=0), b"C > 0")
    rejected(head_bwd(C=65536), b"65535")


def test_casts_refuse_a_negative_count():
    lib = _lib.lib()
    for call in (lib.vitmi_cast_f32_bf16, lib.vitmi_cast_bf16_f32):
        rejected(call(-8, OK_PTR, OK_PTR, None), b"n must be >= 0")
        rejected(call(-1, OK_PTR, OK_PTR, None), b"n must be >= 0")
        rejected(call(8, OK_PTR + 8, OK_PTR, None), b"alignment")
        rejected(call(8, None, OK_PTR, None), b"null")
        no_work(call(0, OK_PTR, OK_PTR, None))
        served(lambda: call(1, OK_PTR, OK_PTR, None))
        served(lambda: call(8, OK_PTR, OK_PTR, None))


def test_dropout_apply_refuses_negative_sizes():
    rejected(dropout(M=-1), b"negative size")
    rejected(dropout(N=-4), b"negative size")
    rejected(dropout(dtype=3), b"dtype")
    rejected(dropout(N=6), b"multiples of 4")
    no_work(dropout(M=0))
    no_work(dropout(N=0))
    served(lambda: dropout())
    served(lambda: dropout(M=1, N=4, dtype=BF16))


def test_loss_arguments():
    lib = _lib.lib()
    rejected(lib.vitmi_loss_fwd_bwd(2, 4, 3, OK_PTR, OK_PTR, OK_PTR, OK_PTR, None), b"bad kind")
    rejected(lib.vitmi_loss_fwd_bwd(0, 0, 3, OK_PTR, OK_PTR, OK_PTR, OK_PTR, None), b"bad arguments")
    rejected(lib.vitmi_loss_fwd_bwd(0, 4, 0, OK_PTR, OK_PTR, OK_PTR, OK_PTR, None), b"bad arguments")
    rejected(lib.vitmi_loss_fwd_bwd(0, 4, 3, OK_PTR, OK_PTR, None, None, None), b"bad arguments")
    rejected(lib.vitmi_xent_fwd(4, 3, OK_PTR, OK_PTR, None, None), b"null loss")
    rejected(lib.vitmi_xent_bwd(4, 3, OK_PTR, OK_PTR, None, None), b"null dlogits")
    rejected(lib.vitmi_mse_fwd(4, 3, OK_PTR, OK_PTR, None, None), b"null loss")
    rejected(lib.vitmi_mse_bwd(4, 3, OK_PTR, OK_PTR, None, None), b"null dpred")
    served(lambda: lib.vitmi_loss_fwd_bwd(0, 4, 3, OK_PTR, OK_PTR, OK_PTR, None, None))
