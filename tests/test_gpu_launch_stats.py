"""Which kernel each dtype / template switch of the host launch layer selects, on the MI355X, and the
work it records: one small call per branch of csrc/{layernorm,elementwise,layerscale,optim,split}.hip
and of the single-pass attention backward's NKB table.

Every case asserts, from the library's own statistics (vitmi_stats_*),
  (a) that exactly the expected kernel instance recorded exactly one call and no other kernel did,
  (b) its flops and bytes against the closed forms written out here from the shapes (the formulas of
      the csrc comments: operands read and written once, 2 flops per multiply-add),
  (c) that an entry point that records no work records none.
The shapes are the smallest at which each branch is selected."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from kstats import kernel_stats  # noqa: E402
from vitmi import ops  # noqa: E402
from vitmi._lib import check, lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
VF32, VBF16, VX3, VF8, VF8W = 0, 1, 3, 4, 5            # include/vitmi.h dtypes
p, s = ops._p, ops._s

# template argument -> (Itanium mangling, demangled spelling)
TYPES = {"float": ("f", "float"), "bf16": ("DF16b", "__bf16"), "SplitX3": ("NS_7SplitX3E", "vitmi::SplitX3"),
         "SplitF8": ("NS_7SplitF8E", "vitmi::SplitF8"), "SplitF8W": ("NS_8SplitF8WE", "vitmi::SplitF8W")}


def kname(base, *targs):
    """The kernel's name as recorded: mangled (base I <args> E) or demangled (base<args>)."""
    if not targs:
        return (base,)
    m, d = [], []
    for a in targs:
        if isinstance(a, bool):
            m.append(f"Lb{int(a)}E"), d.append("true" if a else "false")
        elif isinstance(a, int):
            m.append(f"Li{a}E"), d.append(str(a))
        else:
            m.append(TYPES[a][0]), d.append(TYPES[a][1])
    return (base + "I" + "".join(m) + "E", base + "<" + ", ".join(d) + ">")


def assert_recorded(st, exp, what):
    """exp: {name forms: (calls, flops, bytes)}; nothing else may have been recorded."""
    got = dict(st.work)
    print(f"{what}: {got}")
    for forms, w in exp.items():
        hits = [n for n in got if any(f in n for f in forms)]
        assert len(hits) == 1, (what, forms, got)
        assert got.pop(hits[0]) == w, (what, forms, w)
    assert not got, (what, "not expected", got)


def rnd(*shape, dtype=F32, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


def tname(t):
    return "bf16" if t == BF else "float"


# ---------------------------------------------------------------- LayerNorm
LN_M = 5                                                # a partial 4-row block
LN_DS = (64, 128, 256, 768, 2048)
LN_Y = {VF32: ("float", 4, 1.0), VBF16: ("bf16", 2, 1.0), VX3: ("SplitX3", 6, 3.0), VF8: ("SplitF8", 4, 2.0),
        VF8W: ("SplitF8W", 3, 1.5)}                     # template tag, y bytes per element, ldy / D (bf16 units)


def ln_nv(D):
    nv = (D + 255) // 256
    return nv if nv <= 4 else 8


def ln_y_dtypes(D):
    return [y for y in LN_Y if not (y == VF8 and D % 64) and not (y == VF8W and D % 128)]


@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_fwd(D):
    M = LN_M
    x, g, b = rnd(M, D), rnd(D, seed=2), rnd(D, seed=3)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    for ydt in ln_y_dtypes(D):
        tag, ysz, ldf = LN_Y[ydt]
        y = torch.empty(M, 3 * D, dtype=F32 if ydt == VF32 else BF, device=DEV)
        with kernel_stats() as st:
            check(lib().vitmi_layernorm_fwd(M, D, p(x), D, p(g), p(b), 1e-6, p(y), ydt, int(ldf * D), p(mean), p(rstd),
                                            s()), "layernorm_fwd")
        torch.cuda.synchronize()
        small = D in (64, 128) and ydt in (VF32, VBF16)
        name = kname("ln_fwd_small_kernel", D // 4, tag) if small else kname("ln_fwd_kernel", ln_nv(D), tag)
        # x (fp32) read, y written, mean / rstd written
        assert_recorded(st, {name: (1, 0.0, float(M * D * (4 + ysz) + 8 * M))}, f"ln fwd D {D} y {tag}")


@pytest.mark.parametrize("D", LN_DS)
def test_layernorm_bwd(D):
    M = LN_M
    x, g, res = rnd(M, D), rnd(D, seed=2), rnd(M, D, seed=4)
    mean, rstd = x.mean(1), (x.var(1, unbiased=False) + 1e-6).rsqrt()
    dx, dx_lp = torch.empty(M, D, device=DEV), torch.empty(M, D, dtype=BF, device=DEV)
    ws = torch.empty(lib().vitmi_layernorm_bwd_workspace_size(M, D), dtype=torch.uint8, device=DEV)
    for T in (BF, F32):
        dy = rnd(M, D, dtype=T, seed=5)
        for lp in (False, True):
            for dres in (False, True):
                with kernel_stats() as st:      # no dgamma / dbeta / dxsum: the partials are not folded
                    check(lib().vitmi_layernorm_bwd(M, D, p(dy), VBF16 if T == BF else VF32, D, p(x), D, p(mean),
                                                    p(rstd), p(g), p(res) if dres else None, D, p(dx), D,
                                                    p(dx_lp) if lp else None, D, None, None, None, p(ws), ws.numel(),
                                                    s()), "layernorm_bwd")
                torch.cuda.synchronize()
                name = (kname("ln_bwd_small_kernel", D // 4, tname(T), lp) if D in (64, 128)
                        else kname("ln_bwd_kernel", ln_nv(D), tname(T), lp))
                # dy + x (+ dres) read, dx (+ its bf16 copy) written, mean / rstd read
                by = M * D * ((2 if T == BF else 4) + 4 + (4 if dres else 0) + 4 + (2 if lp else 0)) + 8 * M
                assert_recorded(st, {name: (1, 0.0, float(by))}, f"ln bwd D {D} dy {tname(T)} lp {lp} dres {dres}")


# ---------------------------------------------------------------- elementwise.hip
@pytest.mark.parametrize("N", [8, 12], ids=["vector", "column"])
@pytest.mark.parametrize("T", [BF, F32], ids=["bf16", "f32"])
def test_bias_grad(T, N):
    M = 37
    dy, db = rnd(M, N, dtype=T), torch.zeros(N, device=DEV)
    Z = 2                                               # row chunks of >= 32 rows: ceil(37 / 32)
    assert lib().vitmi_bias_grad_workspace_size(M, N) == Z * N * 4
    ws = torch.empty(Z * N * 4, dtype=torch.uint8, device=DEV)
    with kernel_stats() as st:
        check(lib().vitmi_bias_grad(VBF16 if T == BF else VF32, M, N, p(dy), N, p(db), p(ws), ws.numel(), s()),
              "bias_grad")
    torch.cuda.synchronize()
    base = "colsum8_kernel" if N == 8 else "colsum_kernel"
    assert_recorded(st, {kname(base, tname(T)): (1, 0.0, float(M * N * (2 if T == BF else 4))),    # dy read once
                         kname("fold_kernel"): (1, 0.0, 4.0 * (Z + 2) * N)},    # Z partial rows, db read and written
                    f"bias_grad {tname(T)} N {N}")
    assert torch.allclose(db.cpu(), dy.float().sum(0).cpu(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("thresh", [0, 1 << 31], ids=["path", "path+dropout"])
@pytest.mark.parametrize("T", [BF, F32], ids=["bf16", "f32"])
def test_droppath_apply(T, thresh):
    M, S, N = 6, 3, 8
    x, y = rnd(M, N), torch.empty(M, N, dtype=T, device=DEV)
    with kernel_stats() as st:
        check(lib().vitmi_droppath_apply(M, N, p(x), N, p(y), VBF16 if T == BF else VF32, N, S, 7, 1, 1 << 30, 1.25, 2,
                                         thresh, 2.0, s()), "droppath_apply")
    torch.cuda.synchronize()
    # x read, y written
    assert_recorded(st, {kname("droppath_apply_kernel", tname(T), thresh != 0):
                         (1, 0.0, float(M * N * (4 + (2 if T == BF else 4))))}, f"droppath {tname(T)} {thresh}")


@pytest.mark.parametrize("T", [BF, F32], ids=["bf16", "f32"])
def test_dropout_apply_records_nothing(T):
    M, N = 6, 8
    x, y = rnd(M, N), torch.empty(M, N, dtype=T, device=DEV)
    with kernel_stats() as st:
        check(lib().vitmi_dropout_apply(M, N, p(x), N, p(y), VBF16 if T == BF else VF32, N, 7, 1, 1 << 31, 2.0, s()),
              "dropout_apply")
    torch.cuda.synchronize()
    assert not st.work, st.work


# ---------------------------------------------------------------- layerscale.hip
@pytest.mark.parametrize("T", [BF, F32], ids=["bf16", "f32"])
def test_layerscale_fold_and_apply(T):
    N, K, M = 5, 8, 3
    es = 2 if T == BF else 4
    w, g, b = rnd(N, K), rnd(N, seed=2), rnd(N, seed=3)
    w_eff, b_eff = torch.empty(N, K, dtype=T, device=DEV), torch.empty(N, device=DEV)
    with kernel_stats() as st:
        check(lib().vitmi_layerscale_fold(N, K, p(w), p(g), p(b), p(w_eff), VBF16 if T == BF else VF32, p(b_eff), s()),
              "layerscale_fold")
    torch.cuda.synchronize()
    # w read, w_eff written
    assert_recorded(st, {kname("layerscale_fold_kernel", tname(T)): (1, 0.0, float((4 + es) * N * K))},
                    f"layerscale_fold {tname(T)}")
    x, gk, y = rnd(M, K), rnd(K, seed=4), torch.empty(M, K, dtype=T, device=DEV)
    with kernel_stats() as st:
        check(lib().vitmi_layerscale_apply(M, K, p(x), K, p(gk), p(y), VBF16 if T == BF else VF32, K, s()),
              "layerscale_apply")
    torch.cuda.synchronize()
    # x read, y written
    assert_recorded(st, {kname("layerscale_apply_kernel", tname(T)): (1, 0.0, float((4 + es) * M * K))},
                    f"layerscale_apply {tname(T)}")


@pytest.mark.parametrize("K", [8, 1032], ids=["wave-per-row", "block-per-row"])
@pytest.mark.parametrize("dot,scale", [(True, True), (True, False), (False, True)])
def test_layerscale_bwd(dot, scale, K):
    N = 5
    w, b, g = rnd(N, K), rnd(N, seed=2), rnd(N, seed=3)
    dw, db, dg = rnd(N, K, seed=4), rnd(N, seed=5), torch.zeros(N, device=DEV)
    with kernel_stats() as st:
        check(lib().vitmi_layerscale_bwd(N, K, p(w), p(b), p(g), p(dw), p(db), p(dg) if dot else None, int(scale), s()),
              "layerscale_bwd")
    torch.cuda.synchronize()
    # dw read (+ w read for the dot) (+ dw written when scaled); the dot is one multiply-add per element
    work = (1, 2.0 * N * K if dot else 0.0, 4.0 * N * K * ((2 if dot else 1) + (1 if scale else 0)))
    assert_recorded(st, {kname("layerscale_bwd_kernel", 4 if K > 1024 else 1, dot, scale): work},
                    f"layerscale_bwd K {K} dot {dot} scale {scale}")


# ---------------------------------------------------------------- optim.hip
@pytest.mark.parametrize("lp", [False, True], ids=["fp32", "shadow"])
def test_adam_steps(lp):
    n = 1000
    prm, g, m, v = rnd(n), rnd(n, seed=2), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    shadow = torch.empty(n, dtype=BF, device=DEV) if lp else None
    with kernel_stats() as st:
        check(lib().vitmi_adam_step(n, p(prm), p(g), p(m), p(v), p(shadow), 1e-3, 0.9, 0.999, 1e-7, 1.0, s()),
              "adam_step")
    torch.cuda.synchronize()
    # p, g, m, v read; p, m, v (+ the bf16 shadow) written
    # adam_kernel<LP, CTL, EMA>: each entry point records its own instance
    assert_recorded(st, {kname("adam_kernel", lp, False, False): (1, 0.0, float(n * (30 if lp else 28)))},
                    f"adam lp {lp}")
    ctl = torch.zeros(4, device=DEV)
    check(lib().vitmi_clip_finalize(0, None, 1.0, 0.0, 0, p(ctl), s()), "clip_finalize")
    with kernel_stats() as st:
        check(lib().vitmi_adam_step_ctl(n, p(prm), p(g), p(m), p(v), p(shadow), 1e-3, 0.9, 0.999, 1e-7, 1.0, 0.0, 1e-3,
                                        None, p(ctl), s()), "adam_step_ctl")
    torch.cuda.synchronize()
    # as adam_step, plus the 16-byte clip record (no decay mask)
    assert_recorded(st, {kname("adam_kernel", lp, True, False): (1, 0.0, float(n * (30 if lp else 28) + 16))},
                    f"adam ctl lp {lp}")
    # and the ctl instance it stays with no record and no decay: the argument values select nothing
    with kernel_stats() as st:
        check(lib().vitmi_adam_step_ctl(n, p(prm), p(g), p(m), p(v), p(shadow), 1e-3, 0.9, 0.999, 1e-7, 1.0, 0.0, 1e-3,
                                        None, None, s()), "adam_step_ctl")
    torch.cuda.synchronize()
    assert_recorded(st, {kname("adam_kernel", lp, True, False): (1, 0.0, float(n * (30 if lp else 28)))},
                    f"adam ctl, no record, lp {lp}")


# ---------------------------------------------------------------- split.hip
@pytest.mark.parametrize("copy", [False, True], ids=["split", "split+hi"])
def test_split(copy):
    rows, K = 3, 64
    x = rnd(rows, K)
    hi = torch.empty(rows, K, dtype=BF, device=DEV) if copy else None
    for fn, kern, parts in (("vitmi_split_bf16x3", "split3_kernel", 3), ("vitmi_split_bf16f8", "split_f8_kernel", 2)):
        dst = torch.empty(rows, parts * K, dtype=BF, device=DEV)
        with kernel_stats() as st:
            check(getattr(lib(), fn)(rows, K, p(x), K, p(dst), parts * K, 0, p(hi), K, s()), fn)
        torch.cuda.synchronize()
        # src (fp32) read, the parts (bf16 units) (+ the bf16 copy of hi) written
        assert_recorded(st, {kname(kern): (1, 0.0, float(rows * K * (4 + 2 * parts + (2 if copy else 0))))},
                        f"{fn} copy {copy}")


# ---------------------------------------------------------------- attention.hip: the single-pass backward's NKB
@pytest.mark.parametrize("N", [1, 33, 197])
def test_attention_bwd_single_pass(N):
    B, H, DH = 1, 2, 64
    scale = DH ** -0.5
    qkv, do = rnd(B * N, 3 * H * DH, dtype=BF, seed=22), rnd(B * N, H * DH, dtype=BF, seed=23)
    o, lse = ops.attention_fwd(qkv, B, N, H, scale)
    with kernel_stats() as st:
        ops.attention_bwd(qkv, o, do, lse, B, N, H, scale)
    torch.cuda.synchronize()
    bh, t = B * H, B * H * N * DH
    # dP, dQ, dV, dK: 8 N^2 dh flops per head; q, k, v, o, dO read and dq, dk, dv written (bf16), lse read, delta written
    assert_recorded(st, {kname("attn_bwd_fused_seq_bf16", (N + 31) // 32):
                         (1, 8.0 * bh * N * N * DH, float(t * 8 * 2 + bh * N * 8))}, f"attention bwd N {N}")
