"""CPU-side checks of the patch-dropout entry points (include/vitmi.h, "Patch dropout"): host
validation rejects bad arguments with the invalid-argument code before any launch."""
from vitmi import _lib

OK_PTR = 4096          # never dereferenced: every call below fails validation first
F32, BF16 = 0, 1
SEED, SITE = 7, 0x20000000
BIG = 1 << 30          # a workspace size no call below gets to use


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def keep(B=4, np_=16, K=8, keep=OK_PTR, slot=OK_PTR):
    return _lib.lib().vitmi_patch_keep(B, np_, K, SEED, SITE, keep, slot, None)


def im2col(dtype=BF16, B=4, C=3, S=32, P=8, K=8, keep=OK_PTR, img=OK_PTR, patches=OK_PTR):
    return _lib.lib().vitmi_patch_im2col_keep(dtype, B, C, S, P, K, keep, img, patches, None)


def assemble(B=4, np_=16, K=8, D=128, tok=OK_PTR, keep=OK_PTR, x=OK_PTR):
    return _lib.lib().vitmi_tokens_assemble_keep(B, np_, K, D, tok, OK_PTR, OK_PTR, keep, x, None)


def assemble_bwd(B=4, np_=16, K=8, D=128, dx=OK_PTR, slot=OK_PTR):
    return _lib.lib().vitmi_tokens_assemble_keep_bwd(B, np_, K, D, dx, OK_PTR, None, OK_PTR, OK_PTR, slot, None)


def embed_fwd(dtype=BF16, B=4, C=3, S=32, P=8, D=128, K=8, keep=OK_PTR, img=OK_PTR, w=OK_PTR, patches=OK_PTR,
              x=OK_PTR, ws=OK_PTR, ws_bytes=BIG):
    return _lib.lib().vitmi_patch_embed_keep_fwd(dtype, B, C, S, P, D, K, keep, img, w, None, None, None, patches, x,
                                                 ws, ws_bytes, None)


def embed_bwd(dtype=BF16, B=4, C=3, S=32, P=8, D=128, K=8, slot=OK_PTR, dx=OK_PTR, patches=OK_PTR, ws=OK_PTR,
              ws_bytes=BIG):
    return _lib.lib().vitmi_patch_embed_keep_bwd(dtype, B, C, S, P, D, K, slot, dx, patches, OK_PTR, OK_PTR, OK_PTR,
                                                 OK_PTR, ws, ws_bytes, None)


def test_null_pointers_are_rejected():
    for name in ("keep", "slot"):
        rejected(keep(**{name: None}), b"null")
    for name in ("keep", "img", "patches"):
        rejected(im2col(**{name: None}), b"null")
    for name in ("tok", "keep", "x"):
        rejected(assemble(**{name: None}), b"null")
    for name in ("dx", "slot"):
        rejected(assemble_bwd(**{name: None}), b"null")
    for name in ("keep", "img", "w", "patches", "x"):
        rejected(embed_fwd(**{name: None}), b"null")
    for name in ("slot", "dx", "patches"):
        rejected(embed_bwd(**{name: None}), b"null")


def test_number_kept_must_be_in_1_np():
    for K in (0, -1, 17):
        rejected(keep(K=K), b"1 <= K <= np")
        rejected(im2col(K=K), b"1 <= K <= np")
        rejected(assemble(K=K), b"1 <= K <= np")
        rejected(assemble_bwd(K=K), b"1 <= K <= np")
        rejected(embed_fwd(K=K), b"1 <= K <= np")
        rejected(embed_bwd(K=K), b"1 <= K <= np")
        assert _lib.lib().vitmi_patch_embed_keep_fwd_workspace_size(BF16, 4, 3, 32, 8, 128, K) == 0
        assert _lib.lib().vitmi_patch_embed_keep_bwd_workspace_size(BF16, 4, 3, 32, 8, 128, K) == 0


def test_more_than_4096_patches_are_rejected():
    rejected(keep(np_=4097, K=8), b"4096")
    rejected(assemble(np_=4097), b"4096")
    rejected(assemble_bwd(np_=4097), b"4096")
    # a 65 x 65 grid of 4 x 4 patches: np = 4225
    rejected(im2col(S=260, P=4), b"4096")
    rejected(embed_fwd(S=260, P=4), b"4096")
    rejected(embed_bwd(S=260, P=4), b"4096")
    assert keep(B=0) == 1                                      # nothing to select is a caller's mistake too


def test_embedding_width_must_be_a_multiple_of_4():
    rejected(assemble(D=126), b"D % 4")
    rejected(assemble_bwd(D=126), b"D % 4")
    rejected(embed_fwd(D=126), b"D % 4")
    rejected(embed_bwd(D=126), b"D % 4")


def test_geometry_and_dtype():
    rejected(im2col(S=30), b"S % P")
    rejected(im2col(P=6, S=36), b"P % 4")
    rejected(im2col(dtype=4), b"dtype")
    rejected(embed_fwd(S=30), b"shape")


def test_workspace_queries_and_small_workspaces():
    lib = _lib.lib()
    # rows = B*K: the conv output (fp32) / its gradient (dtype) of the kept rows, plus the GEMMs' own
    assert lib.vitmi_patch_embed_keep_fwd_workspace_size(BF16, 256, 3, 224, 16, 768, 98) >= 256 * 98 * 768 * 4
    assert lib.vitmi_patch_embed_keep_bwd_workspace_size(BF16, 256, 3, 224, 16, 768, 98) >= 256 * 98 * 768 * 2
    assert (lib.vitmi_patch_embed_keep_fwd_workspace_size(BF16, 256, 3, 224, 16, 768, 98)
            < lib.vitmi_patch_embed_fwd_workspace_size(BF16, 256, 3, 224, 16, 768))
    rejected(embed_fwd(ws_bytes=8), b"workspace")
    rejected(embed_bwd(ws_bytes=8), b"workspace")
    rejected(embed_fwd(ws=None), b"workspace")
