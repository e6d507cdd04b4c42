"""tests/ref_tokens.py judged on the CPU (no GPU): the float64 reference agrees with torch's own operators
and autograd; the float32 restatements of the kernels' arithmetic sit inside the derived bounds for every
family and every case of the GPU matrix (the bounds are not vacuous, nothing is excluded, nothing skipped);
and every mutated restatement is REJECTED, by the bound or by the bit comparison, in every family where the
mutation applies."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_tokens as rt

BF = torch.bfloat16
CAP = 1.0                        # fixed: an emulation conforms iff every element's |err| / tol <= 1


def head_inputs(fam, B, D, C):
    y = rt.family(fam, B, D, "y")
    w = rt.family("randn" if fam == "rows" else fam, C, D, "w")
    b = rt.family("randn" if fam == "rows" else fam, 1, C, "b")[0]
    dl = rt.family(fam, B, C, "dl")
    pw, pb = rt.family("int" if fam == "int" else "randn", C, D, "pw"), rt.family("int" if fam == "int" else "randn", 1, C, "pb")[0]
    return y, w, b, dl, pw, pb


def token_inputs(fam, B, np_, D, K=None):
    K = np_ if K is None else K
    dx = rt.family(fam, B, (K + 1) * D, "dx")
    pf = "int" if fam == "int" else "randn"
    return dx, rt.family(pf, np_ + 1, D, "ppos"), rt.family(pf, 1, D, "pcls")[0]


# ------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("C,S,P", rt.IM2COL_SHAPES)
def test_im2col_is_unfold_and_conv2d(C, S, P):
    B, D = 3, 5
    g = rt.gen("im2col", C, S, P)
    img = torch.randn(B, C, S, S, generator=g)
    got = rt.im2col(img, P)
    unf = F.unfold(img, P, stride=P).transpose(1, 2).reshape(-1, C * P * P)
    assert torch.equal(got, unf)
    w = torch.randn(D, C, P, P, generator=g).double()
    conv = F.conv2d(img.double(), w, stride=P).flatten(2).transpose(1, 2).reshape(-1, D)
    assert torch.allclose(got.double() @ w.view(D, -1).t(), conv, rtol=1e-12, atol=1e-12)
    np_ = (S // P) ** 2
    for K in sorted({1, max(np_ // 2, 1), np_}):
        keep = rt.keep_lists(B, np_, K, bad=K == max(np_ // 2, 1) and K > 1)
        gk = rt.im2col(img, P, keep).view(B, K, -1)
        for b in range(B):
            for j in range(K):
                p = keep[b, j]
                want = unf.view(B, np_, -1)[b, p] if 0 <= p < np_ else torch.zeros(C * P * P)
                assert torch.equal(gk[b, j], want), (K, b, j)
    assert torch.equal(rt.im2col_expected(img, P, True), unf.to(BF))


@pytest.mark.parametrize("D,np_,B", [(4, 1, 1), (64, 16, 9), (260, 49, 7)])
def test_assemble_is_cat_plus_add_and_its_autograd(D, np_, B):
    tok, cls, pos = rt.family("rows", B * np_, D, "tok"), rt.family("randn", 1, D, "cls")[0], rt.family("randn", np_ + 1, D, "pos")
    for c, p in itertools.product((cls, None), (pos, None)):
        got = rt.assemble(tok, c, p, B, np_, D)
        ref = rt.assemble_ref(tok, c, p, B, np_, D)
        assert torch.equal(got, ref.float()) if (c is None or p is None) else (got.double() - ref).abs().max() <= 2.0 ** -24 * ref.abs().max()
        assert torch.equal(got, (torch.cat([(torch.zeros(D) if c is None else c).expand(B, 1, D), tok.view(B, np_, D)], 1)
                                 + (0 if p is None else p)).float())
    # the backward: autograd of cat + add in float64
    dx, ppos, pcls = token_inputs("rows", B, np_, D)
    leaves = [t.double().requires_grad_() for t in (tok, cls, pos)]
    x = torch.cat([leaves[1].expand(B, 1, D), leaves[0].view(B, np_, D)], 1) + leaves[2]
    x.backward(dx.view(B, np_ + 1, D).double())
    out = rt.pos_bwd(dx, ppos, pcls, B, np_, D)
    assert torch.allclose(out["dpos"][1], ppos.double() + leaves[2].grad, rtol=1e-13, atol=1e-13)
    assert torch.allclose(out["dcls"][1][0], pcls.double() + leaves[1].grad, rtol=1e-13, atol=1e-13)
    dtok, dtok_lp = rt.split_bwd(dx, B, np_, D)
    assert torch.equal(dtok.double(), leaves[0].grad) and torch.equal(dtok_lp, dtok.to(BF))
    # the gathered form: autograd through an index_select of the position rows
    K = max(np_ // 2, 1)
    keep = rt.keep_lists(B, np_, K)
    slot = rt.slot_lists(keep, np_)
    tokk = rt.family("rows", B * K, D, "tokk")
    dxk, _, _ = token_inputs("rows", B, np_, D, K)
    lv = [t.double().requires_grad_() for t in (tokk, cls, pos)]
    rows = torch.from_numpy(np.concatenate([np.zeros((B, 1), dtype=np.int64), 1 + keep.astype(np.int64)], 1))
    xk = torch.cat([lv[1].expand(B, 1, D), lv[0].view(B, K, D)], 1) + lv[2][rows]
    assert torch.equal(rt.assemble(tokk, cls, pos, B, np_, D, keep), xk.detach().float()) or \
        (rt.assemble(tokk, cls, pos, B, np_, D, keep).double() - xk.detach()).abs().max() <= 2.0 ** -24 * xk.detach().abs().max()
    xk.backward(dxk.view(B, K + 1, D).double())
    outk = rt.pos_bwd(dxk, ppos, pcls, B, np_, D, slot)
    assert torch.allclose(outk["dpos"][1], ppos.double() + lv[2].grad, rtol=1e-13, atol=1e-13)
    assert torch.allclose(outk["dcls"][1][0], pcls.double() + lv[1].grad, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("B,D,C", [(1, 1, 1), (17, 65, 3), (37, 192, 10)])
def test_head_is_linear_and_its_autograd(B, D, C):
    y, w, b, dl, pw, pb = head_inputs("rows", B, D, C)
    lv = [t.double().requires_grad_() for t in (y, w, b)]
    out = F.linear(*lv)
    assert torch.allclose(rt.head_fwd(y, w, b)[0], out.detach(), rtol=1e-13, atol=1e-13)
    assert torch.allclose(rt.head_fwd(y, w, None)[0], F.linear(y.double(), w.double()), rtol=1e-13, atol=1e-13)
    out.backward(dl.double())
    r = rt.head_bwd(dl, y, w, pw, pb)
    for k, g, p in (("dy", lv[0].grad, 0), ("dw", lv[1].grad, pw.double()), ("db", lv[2].grad, pb.double())):
        assert torch.allclose(r[k][0], p + g, rtol=1e-12, atol=1e-12), k


@pytest.mark.parametrize("M,N,K", rt.DENSE_SHAPES)
@pytest.mark.parametrize("act", (0, 1))
def test_dense_is_linear_relu_and_its_autograd(M, N, K, act):
    x, w, b = rt.family("rows", M, K, "x"), rt.family("randn", N, K, "w"), rt.family("randn", 1, N, "b")[0]
    dy, pw, pb = rt.family("rows", M, N, "dy"), rt.family("randn", N, K, "pw"), rt.family("randn", 1, N, "pb")[0]
    lv = [t.double().requires_grad_() for t in (x, w, b)]
    out = F.linear(*lv)
    out = F.relu(out) if act else out
    ref, tol = rt.dense_fwd(x, w, b, act)
    assert torch.allclose(ref, out.detach(), rtol=1e-13, atol=1e-13)
    out.backward(dy.double())
    r = rt.dense_bwd(dy, ref.float(), x, w, pw, pb, act)       # y as the float32 the kernel is handed
    for k, g, p in (("dx", lv[0].grad, 0), ("dw", lv[1].grad, pw.double()), ("db", lv[2].grad, pb.double())):
        assert torch.allclose(r[k][0], p + g, rtol=1e-12, atol=1e-12), k
    y32 = rt.emulate_dense_fwd(x, w, b, act)
    assert rt.worst_ratio(y32, ref, tol) <= CAP
    e = rt.emulate_dense_bwd(dy, y32, x, w, pw, pb, act)
    r = rt.dense_bwd(dy, y32, x, w, pw, pb, act)
    for k in r:
        assert rt.worst_ratio(e[k], *r[k]) <= CAP, k


@pytest.mark.parametrize("B,C", [(1, 1), (37, 3), (257, 10)])
def test_losses_are_torch_losses_and_their_autograd(B, C):
    z, t = rt.loss_inputs("ce", "rows", B, C)
    zz = z.double().requires_grad_()
    L = F.cross_entropy(zz, t)
    L.backward()
    r = rt.ce(z, t)
    assert torch.allclose(r["loss"][0], L.detach().view(1), rtol=1e-12) and torch.allclose(r["dl"][0], zz.grad, rtol=1e-11, atol=1e-15)
    z, t = rt.loss_inputs("mse", "rows", B, C)
    zz = z.double().requires_grad_()
    L = F.mse_loss(zz, t.double())
    L.backward()
    r = rt.mse(z, t)
    assert torch.allclose(r["loss"][0], L.detach().view(1), rtol=1e-12) and torch.allclose(r["dl"][0], zz.grad, rtol=1e-12, atol=1e-18)
    # a label outside [0, C): the row's loss is its log-sum-exp, its gradient softmax / B
    z, t = rt.loss_inputs("ce", "rows", B, C)
    t = t.clone()
    t[0], t[-1] = -1, C
    r = rt.ce(z, t)
    lse = torch.logsumexp(z.double(), 1)
    inside = (t >= 0) & (t < C)
    want = (F.cross_entropy(z.double()[inside], t[inside], reduction="sum") if inside.any() else 0) + lse[~inside].sum()
    assert torch.allclose(r["loss"][0], (want / B).view(1), rtol=1e-12)
    assert torch.allclose(r["dl"][0][0], torch.softmax(z.double()[0], 0) / B, rtol=1e-11, atol=1e-300)


# ------------------------------------------------------------------------------------------- emulations conform
@pytest.mark.parametrize("D", rt.HEAD_DS)
def test_head_emulation_is_inside_the_bound(D):
    worst = {}
    for C, B, fam in itertools.product(rt.HEAD_CS, rt.HEAD_BS, rt.FAMILIES):
        y, w, b, dl, pw, pb = head_inputs(fam, B, D, C)
        for bias in (b, None):
            worst["logits"] = max(worst.get("logits", 0), rt.worst_ratio(rt.emulate_head_fwd(y, w, bias), *rt.head_fwd(y, w, bias)))
        r, e = rt.head_bwd(dl, y, w, pw, pb), rt.emulate_head_bwd(dl, y, w, pw, pb)
        for k in r:
            worst[k] = max(worst.get(k, 0), rt.worst_ratio(e[k], *r[k]))
        if fam == "int":
            assert torch.equal(e["db"].double(), r["db"][0]) and torch.equal(e["dw"].double(), r["dw"][0])
    assert all(v <= CAP for v in worst.values()), worst


@pytest.mark.parametrize("D", rt.TOKEN_DS)
def test_position_gradient_emulation_is_inside_the_bound(D):
    for np_, B, fam in itertools.product(rt.TOKEN_NPS, rt.TOKEN_BS, rt.FAMILIES):
        dx, ppos, pcls = token_inputs(fam, B, np_, D)
        for name, (exact, ref, tol) in rt.pos_bwd(dx, ppos, pcls, B, np_, D).items():
            assert rt.worst_ratio(exact, ref, tol) <= CAP, (name, np_, B, fam)
            if fam == "int":
                assert torch.equal(exact.double(), ref)
        K = max(np_ // 2, 1)
        slot = rt.slot_lists(rt.keep_lists(B, np_, K), np_, bad=np_ > 1)
        dxk, _, _ = token_inputs(fam, B, np_, D, K)
        for name, (exact, ref, tol) in rt.pos_bwd(dxk, ppos, pcls, B, np_, D, slot).items():
            assert rt.worst_ratio(exact, ref, tol) <= CAP, (name, np_, B, fam, "keep")


@pytest.mark.parametrize("kind", ("ce", "mse"))
def test_loss_emulation_is_inside_the_bound(kind):
    worst = {}
    for B, C, fam in itertools.product(rt.LOSS_BS, rt.LOSS_CS, ("rows", "spike")):
        z, t = rt.loss_inputs(kind, fam, B, C)
        r, e = (rt.ce if kind == "ce" else rt.mse)(z, t), rt.emulate_loss(kind, z, t)
        for k in r:
            worst[k] = max(worst.get(k, 0), rt.worst_ratio(e[k], *r[k]))
        if kind == "ce":
            t = t.clone()
            t[0], t[-1] = -1, C
            r, e = rt.ce(z, t), rt.emulate_loss(kind, z, t)
            for k in r:
                worst[k] = max(worst.get(k, 0), rt.worst_ratio(e[k], *r[k]))
    assert all(v <= CAP for v in worst.values()), worst


# ------------------------------------------------------------------------------------------- mutations fail
def differs(a, b):
    return not rt.same_bits(a, b)


def test_every_mutation_is_named():
    assert set(rt.MUTATIONS) == {"khkw", "rowshift", "pos_prev", "cls_tok", "drop_b", "last_wave", "d_lt_D", "trunc",
                                 "pattern", "f8_off", "one_trip", "no_invB"}


@pytest.mark.parametrize("C,S,P", rt.IM2COL_SHAPES)
def test_im2col_mutations_fail(C, S, P):
    img = torch.randn(2, C, S, S, generator=rt.gen("mut", C, S, P))
    np_ = (S // P) ** 2
    for bf in (False, True):
        good = rt.im2col_expected(img, P, bf)
        assert differs(rt.im2col_expected(img, P, bf, mut="khkw"), good)
        if np_ > 1:
            assert differs(rt.im2col_expected(img, P, bf, mut="rowshift"), good)
            keep = rt.keep_lists(2, np_, max(np_ // 2, 1))
            assert differs(rt.im2col_expected(img, P, bf, keep, "rowshift"), rt.im2col_expected(img, P, bf, keep))
    assert differs(rt.im2col_expected(img, P, True, mut="trunc"), rt.im2col_expected(img, P, True))


@pytest.mark.parametrize("fam", rt.FAMILIES)
def test_token_mutations_fail(fam):
    B, np_, D = 9, 16, 64
    tok, cls, pos = rt.family(fam, B * np_, D, "tok"), rt.family("randn", 1, D, "cls")[0], rt.family("randn", np_ + 1, D, "pos")
    good = rt.assemble(tok, cls, pos, B, np_, D)
    for mut in ("pos_prev", "cls_tok"):
        assert differs(rt.assemble(tok, cls, pos, B, np_, D, mut=mut), good), mut
    K = 8
    keep = rt.keep_lists(B, np_, K)
    tokk = rt.family(fam, B * K, D, "tokk")
    goodk = rt.assemble(tokk, cls, pos, B, np_, D, keep)
    for mut in ("pos_prev", "cls_tok"):
        assert differs(rt.assemble(tokk, cls, pos, B, np_, D, keep, mut), goodk), mut
    dx, ppos, pcls = token_inputs(fam, B, np_, D)
    bad = rt.pos_bwd(dx, ppos, pcls, B, np_, D, mut="drop_b")
    for name, (exact, ref, tol) in rt.pos_bwd(dx, ppos, pcls, B, np_, D).items():
        assert differs(bad[name][0], exact), name
        assert rt.worst_ratio(bad[name][0], ref, tol) > CAP, (name, "the bound accepts a dropped batch row")
    d, lp = rt.split_bwd(dx, B, np_, D)
    if fam != "int":               # small integers are bf16 numbers: nothing to truncate
        assert differs(rt.split_bwd(dx, B, np_, D, mut="trunc")[1], lp)


@pytest.mark.parametrize("fam", rt.FAMILIES)
def test_head_mutations_fail(fam):
    for B, D, C in ((37, 65, 3), (16, 192, 10)):
        y, w, b, dl, pw, pb = head_inputs(fam, B, D, C)
        assert rt.worst_ratio(rt.emulate_head_fwd(y, w, b, "d_lt_D"), *rt.head_fwd(y, w, b)) > CAP
        r = rt.head_bwd(dl, y, w, pw, pb)
        e = rt.emulate_head_bwd(dl, y, w, pw, pb, "d_lt_D")
        assert rt.worst_ratio(e["dy"], *r["dy"]) > CAP and rt.worst_ratio(e["dw"], *r["dw"]) > CAP
        e = rt.emulate_head_bwd(dl, y, w, pw, pb, "last_wave")
        assert rt.worst_ratio(e["dw"], *r["dw"]) > CAP and rt.worst_ratio(e["db"], *r["db"]) > CAP


def test_cast_and_split_mutations_fail():
    for x in (rt.family("rows", 37, 128, "cast"), rt.special(rt.CAST_SPECIAL_N).view(1, -1)):
        assert differs(rt.cast_down(x.reshape(-1), "trunc"), rt.cast_down(x.reshape(-1)))
    x = rt.family("rows", 37, 128, "split")
    for pattern in (0, 1):
        good = rt.split_x3(x, pattern)
        assert differs(rt.split_x3(x, pattern, "pattern")[0], good[0])
        assert differs(rt.split_x3(x, pattern, "trunc")[0], good[0]) and differs(rt.split_x3(x, pattern, "trunc")[1], good[1])
    for pattern in (0, 1, 2, 3):
        good = rt.split_f8(x, pattern)
        assert good[0].shape == (37, rt.f8_width(128, pattern))
        assert differs(rt.split_f8(x, pattern, "trunc")[0], good[0])
        if pattern >= 2:
            assert differs(rt.split_f8(x, pattern, "f8_off")[0], good[0])
    # the second trip of a capped grid: only sizes past one trip can show it
    n = rt.GRID_ITEMS * 8 + 8 * 300 + 5
    x = torch.randn(n, generator=rt.gen("walk")) + 3
    assert differs(rt.cast_down(x, "one_trip"), rt.cast_down(x))
    assert differs(rt.cast_up(x.to(BF), "one_trip"), rt.cast_up(x.to(BF)))
    assert not differs(rt.cast_down(x[:2047], "one_trip"), rt.cast_down(x[:2047]))
    rows, K = rt.SPLIT_WALK_X3
    x = torch.randn(rows, K, generator=rt.gen("walk3")) + 3
    assert differs(rt.split_x3(x, 0, "one_trip")[0], rt.split_x3(x, 0)[0])
    rows, K = rt.SPLIT_WALK_F8
    assert differs(rt.split_f8(x[:, :K], 3, "one_trip")[0], rt.split_f8(x[:, :K], 3)[0])
    M, N = rt.DROP_WALK
    assert differs(rt.dropout_apply(x, 5, 9, 1 << 30, 4 / 3, False, "one_trip"), rt.dropout_apply(x, 5, 9, 1 << 30, 4 / 3, False))
    assert differs(rt.dropout_apply(x[:37], 5, 9, 1 << 31, 2.0, True, "trunc"), rt.dropout_apply(x[:37], 5, 9, 1 << 31, 2.0, True))


def test_special_family_holds_what_it_names():
    x = rt.special(rt.CAST_SPECIAL_N)
    b = rt.bits_of(x)
    assert torch.isnan(x).any() and torch.isinf(x).any() and (b == 0).any() and (b == -2 ** 31).any()
    assert ((x != 0) & (x.abs() < 2.0 ** -126)).any() and (x == torch.finfo(torch.float32).max).any()
    low = b & 0xFFFF
    assert ((low == 0x8000) & ((b >> 16) & 1 == 0)).any() and ((low == 0x8000) & ((b >> 16) & 1 == 1)).any()
    f = rt.special(rt.CAST_SPECIAL_N, f8=True)
    assert torch.isfinite(f).all() and (f == 448.0).any() and (f == 224.0).any() and (f.abs() > 448).any()
    # round-to-nearest-even on the ties, and the up-cast is exact
    assert rt.same_bits(rt.cast_up(rt.cast_down(x)), x.to(BF).float())


@pytest.mark.parametrize("kind", ("ce", "mse"))
def test_loss_mutation_fails(kind):
    for fam in ("rows", "spike"):
        for B, C in ((37, 3), (257, 1000), (2, 1) if kind == "mse" else (2, 2)):
            z, t = rt.loss_inputs(kind, fam, B, C)
            r = (rt.ce if kind == "ce" else rt.mse)(z, t)
            assert rt.worst_ratio(rt.emulate_loss(kind, z, t, "no_invB")["dl"], *r["dl"]) > CAP, (fam, B, C)
