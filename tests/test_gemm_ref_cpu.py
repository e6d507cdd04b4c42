"""The GEMM conformance bound (tests/ref_gemm.py) judged on the CPU: an emulation of the kernels'
arithmetic (fp32 matmul of the rounded operands, fp32 epilogue, round-to-nearest-even bf16 store)
must pass at every shape of tests/test_gpu_gemm_matrix.py, and each of a set of subtly wrong
results must fail.  No GPU."""
import pytest
import torch

import ref_gemm as rg

BF = torch.bfloat16

# the shapes of the GPU matrix: edges (k-major / m-major / fp32), tail, small, split-K
SHAPES = [(261, 264, 128), (261, 264, 100), (261, 264, 96), (515, 520, 1024), (515, 520, 1000), (515, 776, 1024),
          (645, 648, 1024), (645, 648, 1000), (131, 133, 64),
          (5, 8, 128), (1, 13, 64), (1, 1, 64), (130, 136, 64), (136, 136, 4000), (1, 136, 4000)]


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def operands(M, N, K, T, layout):
    ak, bk = rg.LAYOUTS[layout]
    a = rnd(M, K, dtype=T, seed=1) if ak else rnd(K, M, dtype=T, seed=1)
    b = rnd(N, K, dtype=T, seed=2, scale=0.05) if bk else rnd(K, N, dtype=T, seed=2, scale=0.05)
    return a, b


def sides(M, N, T):
    return dict(bias=rnd(N, seed=3), aux=rg.gelu_grad(rnd(M, N, seed=4)).to(T), residual=rnd(M, N, seed=5),
                prev=rnd(M, N, seed=6))


def layout_for(K):
    return "KK" if K % 64 == 0 else "NN"


CASES = [("store", False), ("store", True), ("gelu", True), ("residual", False), ("dgelu", False), ("dgelu", True),
         ("accum", False)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_emulation_is_within_the_bound(M, N, K):
    """Accept: worst |err| / tol <= 1 for every epilogue family, bf16 and fp32 operands, plus the
    dropping epilogues.  (Measured: fp32 outputs <= 0.03 of the bound, bf16 outputs 0.85-0.99 at the
    shapes with more than a few elements: the bound is tight where it matters, the bf16 rounding.)"""
    lay = layout_for(K)
    for T in (BF, torch.float32):
        if T == torch.float32 and K % 32 and lay == "KK":
            continue
        a, b = operands(M, N, K, T, lay)
        s = sides(M, N, T)
        for base, out_bf16 in CASES:
            if T == torch.float32 and out_bf16 and base == "gelu":
                out_bf16 = False
            kw = dict(bias=None if base in ("dgelu", "accum") else s["bias"], aux=s["aux"], residual=s["residual"],
                      prev=s["prev"], out_bf16=out_bf16)
            ref = rg.reference(a, b, lay, base, **kw)
            got = rg.emulate(a, b, lay, base, **kw)
            for name, (r, tol) in ref.items():
                w = rg.worst_ratio(got[name], r, tol)
                print(f"{M}x{N}x{K} {lay} {'bf16' if T == BF else 'fp32'} {base} out_bf16={out_bf16} {name}: {w:.3f}")
                assert w <= 1.0, (base, name, w)
        rps = M if M < 5 else 1
        for base, drop, path in (("gelu", (7, 4, 0.25), None), ("residual", (7, 5, 0.25), None),
                                 ("residual", None, (7, 0x40000001, 0.5, rps)),
                                 ("residual", (7, 5, 0.25), (7, 0x40000001, 0.5, rps))):
            kw = dict(bias=s["bias"], residual=s["residual"], out_bf16=(base == "gelu" and T == BF), drop=drop, path=path)
            ref = rg.reference(a, b, lay, base, **kw)
            got = rg.emulate(a, b, lay, base, **kw)
            for name, (r, tol) in ref.items():
                assert rg.worst_ratio(got[name], r, tol) <= 1.0, (base, drop, path, name)


# ------------------------------------------------------------------ mutants
@pytest.fixture(scope="module")
def edge():
    """The edges case, bf16 STORE with bias: operands, reference and the faithful result."""
    M, N, K = 261, 264, 128
    a, b = operands(M, N, K, BF, "KK")
    bias = rnd(N, seed=3)
    out = {}
    for out_bf16 in (False, True):
        r, tol = rg.reference(a, b, "KK", "store", bias=bias, out_bf16=out_bf16)["C"]
        out[out_bf16] = (r, tol, rg.emulate(a, b, "KK", "store", bias=bias, out_bf16=out_bf16)["C"])
    return a, b, bias, out


def test_rejects_truncating_bf16_store(edge):
    """A bf16 store that drops the low bits instead of rounding to nearest (measured 1.3-2.0 x
    the bound)."""
    a, b, bias, out = edge
    r, tol, good = out[True]
    assert rg.worst_ratio(good, r, tol) <= 1.0
    bad = rg.emulate(a, b, "KK", "store", bias=bias, out_bf16=True, store=rg.bf16_trunc)["C"]
    w = rg.worst_ratio(bad, r, tol)
    print(f"truncating store: {w:.2f} x the bound")
    assert w > 1.0
    a32, b32 = operands(261, 264, 128, BF, "KK")
    for base in ("gelu", "dgelu"):
        kw = dict(bias=bias if base == "gelu" else None, aux=rg.gelu_grad(rnd(261, 264, seed=4)).to(BF), out_bf16=True)
        ref = rg.reference(a32, b32, "KK", base, **kw)
        bad = rg.emulate(a32, b32, "KK", base, store=rg.bf16_trunc, **kw)
        for name, (r2, t2) in ref.items():
            assert rg.worst_ratio(bad[name], r2, t2) > 1.0, (base, name)


@pytest.mark.parametrize("out_bf16", [False, True])
def test_rejects_a_dropped_k(edge, out_bf16):
    """One k of the reduction left out (measured: > 89 % of the elements out of bound)."""
    a, b, bias, out = edge
    r, tol, _ = out[out_bf16]
    bad = rg.emulate(a[:, :-1], b[:, :-1], "KK", "store", bias=bias, out_bf16=out_bf16)["C"]
    frac = ((bad.double() - r).abs() > tol).double().mean().item()
    print(f"dropped k, out_bf16={out_bf16}: {100 * frac:.1f} % of the elements out of bound")
    assert frac > 0.5
    assert rg.worst_ratio(bad, r, tol) > 1.0


@pytest.mark.parametrize("out_bf16", [False, True])
def test_rejects_local_mutants(edge, out_bf16):
    """Errors a whole-output norm averages away: one row shifted by one, the bias one column off,
    one transposed 16x16 sub-block, one 4-column group of the last ragged row left unwritten."""
    a, b, bias, out = edge
    r, tol, good = out[out_bf16]
    M, N = good.shape
    assert rg.worst_ratio(good, r, tol) <= 1.0
    # one output row holds its neighbour's values
    bad = good.clone()
    bad[200] = good[201]
    assert rg.worst_ratio(bad, r, tol) > 1.0
    # bias applied one column off
    bad = rg.emulate(a, b, "KK", "store", bias=torch.roll(bias, 1), out_bf16=out_bf16)["C"]
    assert rg.worst_ratio(bad, r, tol) > 1.0
    # one transposed 16x16 sub-block
    bad = good.clone()
    bad[128:144, 64:80] = good[128:144, 64:80].t()
    assert rg.worst_ratio(bad, r, tol) > 1.0
    # the last ragged row's last 4-column group keeps what the buffer held before
    buf = rg.padded(M, N, N + 8, good.dtype, "guard")
    buf.set(good)
    assert rg.guards_intact(buf) and rg.worst_ratio(buf.view, r, tol) <= 1.0
    fresh = rg.padded(M, N, N + 8, good.dtype, "guard")
    buf.view[M - 1, N - 4:] = fresh.view[M - 1, N - 4:]
    assert rg.worst_ratio(buf.view, r, tol) > 1.0
    # and one wrong element among 68904 is enough
    bad = good.clone()
    bad[M - 1, N - 1] = good[M - 1, N - 2]
    assert rg.worst_ratio(bad, r, tol) > 1.0


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("fill", ["guard", "nan"])
def test_guard_bytes(dtype, fill):
    """guards_intact is bitwise: writing the window leaves it true; one changed guard byte, before,
    after or in the pitch columns, makes it false (NaN fills included: compared as bits)."""
    p = rg.padded(5, 13, 16, dtype, fill, offset=1)
    assert p.view.shape == (5, 13) and p.view.stride() == (16, 1)
    assert rg.guards_intact(p)
    p.set(torch.arange(65.0).view(5, 13))
    assert rg.guards_intact(p)
    assert torch.equal(p.view.float(), torch.arange(65.0).view(5, 13))
    nbytes = p.buf.numel() * p.buf.element_size()
    es = p.buf.element_size()
    for byte in (0, (p.start - 1) * es, (p.start + 13) * es, (p.start + 4 * 16 + 13) * es + 1, nbytes - 1):
        q = p.clone()
        q.buf.view(torch.uint8)[byte] ^= 1
        assert not rg.guards_intact(q), byte
    q = p.clone()
    q.buf.view(torch.uint8)[(p.start + 2 * 16 + 5) * es] ^= 1     # inside the window: not a guard
    assert rg.guards_intact(q)


def test_f8_rows_decode():
    """f8_rows: the decoded float64 rows multiply to hi.hi + (hi8.lo8 + lo8.hi8) / 2^9, the product
    tests/test_gpu_f8.py emulates, and the stored rows have the documented widths."""
    x, w = rnd(7, 128, seed=11), rnd(16, 128, seed=12, scale=0.05)
    xs, xd = rg.f8_rows(x, weight=False)
    ws, wd = rg.f8_rows(w, weight=True)
    assert xs.shape == (7, 256) and ws.shape == (16, 256) and xs.dtype == BF
    hi = lambda t: t.to(BF).double()                                      # noqa: E731
    e8 = lambda t: t.clamp(-448, 448).to(rg.E4).double()                  # noqa: E731
    lo = lambda t: e8((t - t.to(BF).float()) * 512.0)                     # noqa: E731
    want = hi(x) @ hi(w).t() + (e8(hi(x).float()) @ lo(w).t() + lo(x) @ e8(hi(w).float()).t()) / 512.0
    assert torch.equal(xd @ wd.t(), want)
    assert torch.equal(xs[:, :128], x.to(BF))
    xs2, xd2 = rg.f8_rows(x, weight=False, wform=True)
    ws2, wd2 = rg.f8_rows(w, weight=True, wform=True)
    assert xs2.shape == (7, 192) and ws2.shape == (16, 192)
    assert torch.equal(xd2 @ wd2.t(), hi(x) @ hi(w).t() + e8(hi(x).float()) @ lo(w).t() / 512.0)
