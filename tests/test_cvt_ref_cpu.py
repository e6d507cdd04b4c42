"""The CvT convolution conformance bound (tests/ref_cvt.py) judged on the CPU: an fp32 emulation of the
kernels' arithmetic must pass it at every listed case of the GPU suite, each of a set of subtly wrong
results (one plausible bug each) must leave the bound at the case and on the output named, the conditioning
condition must hold at every listed case, the reference must agree with oracle/cvt_ref.py, and what the
families pin bitwise must hold for the emulation.  No GPU."""
from functools import lru_cache

import pytest
import torch
import torch.nn.functional as F

import ref_cvt as rc
from oracle import cvt_ref

FWD = ("z", "mean", "rstd", "y", "y_bf16", "run_mean", "run_var")
BWD = ("dx", "dw9", "dgamma", "dbeta")


def show(tag, w):
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in w.items()))
    return w


def merge(into, w):
    for k, v in w.items():
        into[k] = max(into.get(k, 0.0), v)


# ------------------------------------------------------------------ layouts: the GPU suite's, in rows
def layout(H, W):
    """{buffer: (img, off)}: x, y and dy differ in image stride and offset."""
    hw = H * W
    return {"x": (hw + 3, 1), "y": (hw + 4, 2), "dy": (hw + 1, 0)}


def laid(v, ref, tol, H, W, buf, mut):
    """The ratio of an output written through the row layout of ``buf``: 'imgstride' writes it with x's image
    stride, 'nocls' without its offset; the rows in between must stay untouched."""
    L = layout(H, W)
    img, off = L[buf]
    B = v.shape[0]
    total = B * max(a for a, _ in L.values()) + 4
    wimg, woff = (L["x"][0] if mut == "imgstride" else img), (0 if mut == "nocls" else off)
    return rc.worst_rows(rc.rows(v, wimg, woff, total), ref, tol, img, off)


# ------------------------------------------------------------------ dw_bn
@lru_cache(maxsize=4)
def dw_case(family, B, H, W, C):
    inp = rc.dw_inputs(family, B, H, W, C)
    fwd = rc.dwconv_bn_forward(inp["x"], inp["w9"], inp["gamma"], inp["beta"], run_mean=inp["run_mean"],
                               run_var=inp["run_var"], chain=rc.chain_rows(B, H, W, C))
    bwd = rc.dwconv_bn_backward(inp["dy"], inp["x"], inp["w9"], inp["gamma"], fwd["z_in"], fwd["mean_in"], fwd["rstd_in"],
                                inp["prev"], rc.chain_pixels(B, H, W, C), rc.chain_rows(B, H, W, C))
    return inp, fwd, bwd


def dw_fwd_ratios(case, mut=None):
    inp, fwd, _ = dw_case(*case)
    _, B, H, W, C = case
    kw = dict(run_mean=inp["run_mean"], run_var=inp["run_var"], mut=mut)
    a = rc.emulate_dw_fwd(inp["x"], inp["w9"], inp["gamma"], inp["beta"], **kw)
    b = rc.emulate_dw_fwd(inp["x"], inp["w9"], inp["gamma"], inp["beta"], bf16=True, **kw)
    w = {k: rc.worst_ratio(a[k], *fwd[k]) for k in ("z", "mean", "rstd", "run_mean", "run_var")}
    w["y"] = laid(a["y"].double(), *fwd["y"], H, W, "y", mut)
    w["y_bf16"] = laid(b["y"].double(), *fwd["y_bf16"], H, W, "y", mut)
    return w


def dw_bwd_ratios(case, mut=None):
    inp, fwd, bwd = dw_case(*case)
    got = rc.emulate_dw_bwd(inp["dy"], inp["x"], inp["w9"], inp["gamma"], fwd["z_in"], fwd["mean_in"], fwd["rstd_in"],
                            inp["prev"], mut=mut)
    return {k: rc.worst_ratio(got[k], *bwd[k]) for k in BWD}


def pool_ratios(case, count_pad, mut=None):
    family, B, H, W, C = case
    inp = rc.dw_inputs(family, B, H, W, C)
    f = rc.avgpool_fwd(inp["x"], count_pad)
    ref, tol = rc.avgpool_bwd(inp["dy"], inp["prev"]["dx"], count_pad)
    w = {"y": laid(rc.emulate_avgpool_fwd(inp["x"], count_pad, mut=mut).double(), *f["y"], H, W, "y", mut),
         "y_bf16": laid(rc.emulate_avgpool_fwd(inp["x"], count_pad, bf16=True, mut=mut).double(), *f["y_bf16"], H, W, "y", mut),
         "dx": laid(rc.emulate_avgpool_bwd(inp["dy"], inp["prev"]["dx"], count_pad, mut=mut).double(), ref, tol, H, W, "x", mut)}
    return w


ALL_DW = [c for C in rc.DW_CHANNELS for c in rc.dw_matrix(C)]
WALK_CASES = [(f, B, H, W, C) for B, H, W, C, _ in rc.WALKS for f in rc.FAMILIES]
SWEEP_CASES = [("chan", 2, H, W, 64) for H, W in rc.SWEEP]
CAP_CASES = [("randn", *c) for c in rc.CAPS]


@pytest.mark.parametrize("C", rc.DW_CHANNELS)
def test_emulation_conforms_matrix(C):
    """Accept: worst |err| / tol < 1 on every output at every case of the C x (H, W) x B matrix, and the
    conditioning condition holds there (dwconv_bn_forward raises otherwise)."""
    w, rho = {}, 0.0
    for case in rc.dw_matrix(C):
        merge(w, dw_fwd_ratios(case))
        merge(w, dw_bwd_ratios(case))
        for cp in (0, 1):
            merge(w, {f"pool{cp}.{k}": v for k, v in pool_ratios(case, cp).items()})
        rho = max(rho, dw_case(*case)[1]["rho"].max().item())
    show(f"C {C} ({len(rc.dw_matrix(C))} cases, worst rho {rho:.3g})", w)
    assert max(w.values()) < 1.0 and rho <= rc.RHO_MAX, w


@pytest.mark.parametrize("case", WALK_CASES + CAP_CASES + SWEEP_CASES[::9] + SWEEP_CASES[4::9],
                         ids=lambda c: "-".join(map(str, c)))
def test_emulation_conforms_walks_caps_sweep(case):
    w = {**dw_fwd_ratios(case), **dw_bwd_ratios(case)}
    for cp in (0, 1):
        w.update({f"pool{cp}.{k}": v for k, v in pool_ratios(case, cp).items()})
    show(str(case), w)
    assert max(w.values()) < 1.0, w


def test_sweep_is_conditioned():
    for case in SWEEP_CASES:
        assert dw_case(*case)[1]["rho"].max().item() <= rc.RHO_MAX


def test_walk_cases_walk():
    """The host formulas give the multiplicities the issue names (the GPU suite asserts the same formulas
    against the library's workspace size)."""
    for B, H, W, C, least in rc.WALKS:
        G, lanes, per = rc.rows_grid(B, H, W, C)
        assert rc.cdiv(B * H * (C // 4), 256) > rc.dw_blocks(B * H * W, C) and W < 8 and per >= least, (B, H, W, C, per)
    (B, H, W, C), (B2, H2, W2, C2) = rc.CAPS
    cap = rc.CVT_BLOCKS * 256
    assert B * H * (C // 4) > cap and (B * H * (C // 4)) % cap and B * H * W * (C // 4) % cap
    assert rc.cdiv(B2 * H2 * W2, 8 * (256 // (C2 // 4))) > 1024 and B2 * H2 * W2 * (C2 // 4) > cap
    for _, g, Kp in rc.CONV_CAPS:
        assert max(g.B * g.Ho * g.Wo * Kp // 4, g.B * g.H * g.W * g.C // 4) > cap


# ------------------------------------------------------------------ reject: dw_bn forward
SMALL, LANES4, WALK3 = ("chan", 2, 3, 5, 64), ("chan", 3, 5, 3, 256), ("chan", 8, 64, 3, 64)
FWD_REJECT = {      # mutant: (cases, outputs that must leave the bound, outputs that must stay inside)
    "ij": ((SMALL, ("ramp", 2, 3, 5, 64)), ("z", "y"), ()),
    "noleft": ((SMALL,), ("z",), ()),
    "noright": ((SMALL,), ("z",), ()),
    "nobottom": ((SMALL,), ("z",), ()),
    "biasedrv": ((SMALL, LANES4), ("run_var",), ("z", "mean", "rstd", "y", "run_mean")),
    "besselrstd": ((SMALL, LANES4), ("rstd", "y"), ("z", "mean", "run_var")),
    "neighmean": ((SMALL, ("chan", 2, 7, 7, 8)), ("y", "y_bf16"), ("z", "mean", "rstd")),
    "trunc": ((SMALL, LANES4), ("y_bf16",), ("z", "mean", "rstd", "y")),
    "droplast": ((LANES4, WALK3, ("chan", 4, 100, 1, 1024)), ("mean", "rstd"), ("z",)),
    "firsttwice": ((LANES4, WALK3, ("chan", 16, 33, 2, 256)), ("mean", "rstd"), ("z",)),
    "imgstride": ((SMALL,), ("y", "y_bf16"), ("z", "mean", "rstd")),
    "nocls": ((SMALL, ("chan", 1, 1, 1, 64)), ("y", "y_bf16"), ("z", "mean", "rstd")),
}


@pytest.mark.parametrize("mut", sorted(FWD_REJECT))
def test_rejects_forward_mutant(mut):
    cases, bad, good = FWD_REJECT[mut]
    for case in cases:
        assert max(dw_fwd_ratios(case).values()) < 1.0
        w = show(f"{mut} {case}", dw_fwd_ratios(case, mut))
        assert all(w[k] > 1.0 for k in bad) and all(w[k] < 1.0 for k in good), (mut, case, w)


@pytest.mark.parametrize("case", [("ramp", 8, 64, 3, 64), ("ramp", 16, 33, 2, 256)], ids=lambda c: "-".join(map(str, c)))
def test_rejects_fp32_variance_by_the_ramp_pin(case):
    """One fp32 running sum over the channel's n pixels for both moments, fp32 finish: inside the bound on every
    output (measured rstd 0.14 at the worst, see ref_cvt), and off the exact mean the ``ramp`` family pins."""
    inp, fwd, _ = dw_case(*case)
    assert fwd["chain_exact"]
    kw = dict(run_mean=inp["run_mean"], run_var=inp["run_var"])
    good = rc.emulate_dw_fwd(inp["x"], inp["w9"], inp["gamma"], inp["beta"], **kw)
    bad = rc.emulate_dw_fwd(inp["x"], inp["w9"], inp["gamma"], inp["beta"], mut="fp32var", **kw)
    assert torch.equal(good["mean"], fwd["mean_exact"]) and torch.equal(good["z"].double(), fwd["z"][0])
    assert not torch.equal(bad["mean"], fwd["mean_exact"])


def test_ramp_and_int_pins_hold_for_the_emulation():
    """z of ``ramp`` bitwise (and a swapped or unmasked tap moves it by whole multiples of 2^-8), its mean where
    the chain is exact; dbeta of ``int`` the exact sum; the pooling of ``int`` fl(S fl(1 / t))."""
    exact = 0
    for case in [c for c in ALL_DW if c[0] == "ramp"][::3] + [("ramp", *w[:4]) for w in rc.WALKS]:
        inp, fwd, _ = dw_case(*case)
        got = rc.emulate_dw_fwd(inp["x"], inp["w9"], inp["gamma"], inp["beta"])
        assert torch.equal(got["z"].double(), fwd["z"][0]), case
        exact += fwd["chain_exact"]
        assert not fwd["chain_exact"] or torch.equal(got["mean"], fwd["mean_exact"]), case
    assert exact > 20
    for case in [c for c in ALL_DW if c[0] == "int"][::7] + [("int", *w[:4]) for w in rc.WALKS]:
        inp, fwd, bwd = dw_case(*case)
        got = rc.emulate_dw_bwd(inp["dy"], inp["x"], inp["w9"], inp["gamma"], fwd["z_in"], fwd["mean_in"], fwd["rstd_in"],
                                inp["prev"])
        assert torch.equal(got["dbeta"].double(), bwd["dbeta"][0]), case
        for cp in (0, 1):
            y = rc.emulate_avgpool_fwd(inp["x"], cp)
            assert torch.equal(y, rc.avgpool_int_pin(inp["x"], cp)), (case, cp)


# ------------------------------------------------------------------ reject: dw_bn backward
BWD_REJECT = {
    "mirror": ((SMALL, LANES4), ("dx",), ("dw9", "dgamma", "dbeta")),
    "lookahead": ((SMALL,), ("dx",), ("dw9", "dgamma", "dbeta")),
    "k2non": ((SMALL, LANES4), ("dx", "dw9"), ("dgamma", "dbeta")),
    "dxover": ((SMALL,), ("dx",), ("dw9", "dgamma", "dbeta")),
    "dw9over": ((SMALL,), ("dw9",), ("dx", "dgamma", "dbeta")),
    "dgammaover": ((SMALL,), ("dgamma",), ("dx", "dw9", "dbeta")),
    "droplast": ((SMALL, WALK3, ("int", 4, 100, 1, 1024)), ("dgamma", "dbeta", "dw9"), ()),
    "firsttwice": ((SMALL, WALK3, ("int", 16, 33, 2, 256)), ("dgamma", "dbeta", "dw9"), ()),
    "neighmean": ((SMALL, ("chan", 2, 7, 7, 8)), ("dx", "dgamma"), ("dbeta",)),
}


@pytest.mark.parametrize("mut", sorted(BWD_REJECT))
def test_rejects_backward_mutant(mut):
    cases, bad, good = BWD_REJECT[mut]
    for case in cases:
        assert max(dw_bwd_ratios(case).values()) < 1.0
        w = show(f"{mut} {case}", dw_bwd_ratios(case, mut))
        assert all(w[k] > 1.0 for k in bad) and all(w[k] < 1.0 for k in good), (mut, case, w)


# ------------------------------------------------------------------ reject: pooling
POOL_REJECT = {     # mutant: (cases, count_pad, outputs that must fail)
    "hwswap": ((SMALL, ("chan", 1, 5, 3, 4)), 0, ("y", "dx")),
    "nocountpad": ((SMALL, ("chan", 1, 1, 1, 64)), 1, ("y", "dx")),
    "trunc": ((SMALL,), 0, ("y_bf16",)),
    "imgstride": ((SMALL,), 1, ("y", "y_bf16")),
    "nocls": ((SMALL,), 0, ("y", "dx")),
    "droplast": ((CAP_CASES[0],), 0, ("y", "dx")),
    "firsttwice": ((CAP_CASES[0],), 1, ("dx",)),
}


@pytest.mark.parametrize("mut", sorted(POOL_REJECT))
def test_rejects_pooling_mutant(mut):
    cases, cp, bad = POOL_REJECT[mut]
    for case in cases:
        w = show(f"{mut} {case}", pool_ratios(case, cp, mut))
        assert all(w[k] > 1.0 for k in bad), (mut, case, w)
        assert mut != "trunc" or max(w["y"], w["dx"]) < 1.0, (mut, case, w)
    w = pool_ratios(SMALL, 0, "nocountpad")       # count_pad = 0 never looks at the flag
    assert max(w.values()) < 1.0


# ------------------------------------------------------------------ conv
CONV = {name: (g, Kp) for name, g, Kp in rc.conv_cases() + list(rc.CONV_CAPS)}


def conv_layout(g):
    return g.H * g.W + 2, 1          # img_stride, row_off (stage 3: the cls row first; one more row of gap)


def conv_ratios(name, family="randn", mut=None):
    """{im2col f32 / bf16: 0 iff bitwise, col2im with and without accumulate, f32 and bf16 dpatches}."""
    g, Kp = CONV[name]
    inp = rc.conv_inputs(family, g, Kp)
    ref = rc.im2col(inp["x"], g, Kp)
    gm = rc.same_geo(g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, mut) if mut == "padceil" else g
    w = {}
    for bf in (False, True):
        got = rc.emulate_im2col(inp["x"], gm, Kp, bf16=bf, mut=mut, vec=4 if g.C % 4 == 0 and Kp % 4 == 0 else 1)
        want = rc.bf16_rne(ref.float()).double() if bf else ref
        w["im2col.bf16" if bf else "im2col"] = rc.worst_ratio(got, want, torch.zeros_like(want))
    if g.C % 4:
        return w
    img, off = conv_layout(g)
    for bf in (False, True):
        dp = rc.bf16_rne(inp["dp"]).float() if bf else inp["dp"]
        for acc in (False, True):
            prev = inp["prev"] if acc else None
            ref, tol, _ = rc.col2im(dp, g, prev)
            got = rc.emulate_col2im(dp, gm, prev, mut=mut).double()
            wimg, woff = (img + 1 if mut == "imgstride" else img), (0 if mut == "nocls" else off)
            got = rc.rows(got, wimg, woff, g.B * (img + 1) + 2)
            w[f"col2im{'.bf16' if bf else ''}{'.acc' if acc else ''}"] = rc.worst_rows(got, ref, tol, img, off)
    return w


@pytest.mark.parametrize("name", sorted(CONV))
def test_conv_emulation_conforms(name):
    for family in ("randn", "int") if "cap" not in name else ("randn",):
        w = show(f"{name} {family}", conv_ratios(name, family))
        assert max(w.values()) < 1.0, (name, family, w)
    g, Kp = CONV[name]
    if g.C % 4 == 0 and "cap" not in name:      # ``int``: the exact sum, bitwise
        inp = rc.conv_inputs("int", g, Kp)
        ref, _, t = rc.col2im(inp["dp"], g, inp["prev"])
        assert torch.equal(rc.emulate_col2im(inp["dp"], g, inp["prev"]).double(), ref)
        assert (t == 0).any() or not name.endswith("unread"), (name, "no pixel without a window")


CONV_REJECT = {     # mutant: (cases, outputs that must fail)
    "padceil": (("k3s2-odd-total", "k2s3-unread"), ("im2col", "col2im")),
    "ij": (("k3x7s2", "k3s1"), ("im2col", "im2col.bf16")),
    "nopadcols": (("k7s4", "C3-scalar"), ("im2col", "im2col.bf16")),
    "trunc": (("k7s4", "C1-scalar"), ("im2col.bf16",)),
    "nooh": (("k3s1", "k3s2p1"), ("col2im", "col2im.acc")),
    "nomod": (("k3s2-odd-total", "k2s3-unread"), ("col2im", "col2im.bf16")),
    "overwrite": (("k3s1", "k2s3-unread"), ("col2im.acc", "col2im.bf16.acc")),
    "imgstride": (("k3s1",), ("col2im", "col2im.acc")),
    "nocls": (("k3s1", "k1s4-unread"), ("col2im", "col2im.acc")),
    "droplast": (("im2col-cap", "col2im-cap"), ()),
    "firsttwice": (("col2im-cap",), ("col2im.acc",)),
}


@pytest.mark.parametrize("mut", sorted(CONV_REJECT))
def test_rejects_conv_mutant(mut):
    cases, bad = CONV_REJECT[mut]
    for name in cases:
        w = show(f"{mut} {name}", conv_ratios(name, mut=mut))
        assert all(w[k] > 1.0 for k in bad if k in w), (mut, name, w)
        assert max(w.values()) > 1.0, (mut, name, w)


def test_same_geometry_closed_form_and_oracle():
    """same_pad against the oracle's conv_geometry and the definition (the windows cover the input, the
    padding splits floor / ceil) over H x k x s = 1..40 x 1..7 x 1..4; 'padceil' differs iff the total is odd."""
    odd = 0
    for H in range(1, 41):
        for k in range(1, 8):
            for s in range(1, 5):
                Ho, pt = rc.same_pad(H, k, s)
                assert (Ho, pt) == cvt_ref.conv_geometry(H, k, s, None)[:2]
                tot = max((Ho - 1) * s + k - H, 0)
                assert Ho == -(-H // s) and pt == tot // 2 and (rc.same_pad(H, k, s, "padceil")[1] != pt) == bool(tot % 2)
                odd += tot % 2
    assert odd > 100


# ------------------------------------------------------------------ the reference against the oracle
@pytest.mark.parametrize("case", [("chan", 2, 3, 5, 64), ("randn", 3, 8, 9, 4), ("chan", 1, 1, 2, 8)], ids=str)
def test_reference_agrees_with_the_oracle(case):
    """dwconv_bn_forward / _backward against oracle/cvt_ref.dw_bn with autograd in float64, the poolings against
    F.avg_pool2d, im2col against F.unfold with the oracle's geometry."""
    inp, fwd, _ = dw_case(*case)
    _, B, H, W, C = case
    x = inp["x"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    w = inp["w9"].double().t().reshape(C, 1, 3, 3).clone().requires_grad_(True)
    g, b = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
    y = cvt_ref.dw_bn(x, w, g, b, rc.f32(rc.EPS))
    assert torch.allclose(y.permute(0, 2, 3, 1), fwd["y"][0], rtol=1e-12, atol=1e-12)
    dy = inp["dy"].double()
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    zero = {k: torch.zeros_like(v) for k, v in inp["prev"].items()}
    ex = rc.dwconv_bn_backward(dy, inp["x"], inp["w9"], inp["gamma"], fwd["z"][0], fwd["mean"][0], fwd["rstd"][0], zero)
    close = lambda a, r: torch.allclose(a, r, rtol=1e-9, atol=1e-10)  # noqa: E731
    assert close(ex["dx"][0], x.grad.permute(0, 2, 3, 1)) and close(ex["dw9"][0], w.grad.reshape(C, 9).t())
    assert close(ex["dgamma"][0], g.grad) and close(ex["dbeta"][0], b.grad)
    zr = F.conv2d(x.detach(), w.detach(), None, padding=1, groups=C)
    n = B * H * W
    if n > 1:
        omm = float(torch.tensor(1.0) - torch.tensor(rc.f32(rc.MOMENTUM)))
        assert close(fwd["run_var"][0], rc.f32(rc.MOMENTUM) * inp["run_var"].double() + omm * zr.var(dim=(0, 2, 3), unbiased=True))
    for cp in (False, True):
        xs = inp["x"].double().permute(0, 3, 1, 2).clone().requires_grad_(True)
        p = F.avg_pool2d(xs, 3, 1, 1, count_include_pad=cp)
        assert close(rc.avgpool_fwd(inp["x"], cp)["y"][0], p.permute(0, 2, 3, 1))
        (p * dy.permute(0, 3, 1, 2)).sum().backward()
        assert close(rc.avgpool_bwd(inp["dy"], torch.zeros_like(inp["dy"]), cp)[0], xs.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("name", ("k7s4", "k3s2-odd-total", "k3x7s2", "k2s3-unread", "k3s2p1", "k2s2p1-hang"))
def test_conv_reference_agrees_with_unfold(name):
    g, Kp = CONV[name]
    inp = rc.conv_inputs("randn", g, Kp)
    K = g.kh * g.kw * g.C
    pb = max((g.Ho - 1) * g.s + g.kh - g.H - g.pt, 0)
    pr = max((g.Wo - 1) * g.s + g.kw - g.W - g.pl, 0)
    xp = F.pad(inp["x"].double().permute(0, 3, 1, 2), (g.pl, pr, g.pt, pb))
    u = F.unfold(xp, (g.kh, g.kw), stride=g.s)
    grid = ((xp.shape[2] - g.kh) // g.s + 1, (xp.shape[3] - g.kw) // g.s + 1)
    u = u.view(g.B, g.C, g.kh * g.kw, *grid)[:, :, :, :g.Ho, :g.Wo].permute(0, 3, 4, 2, 1).reshape(-1, K)
    ref = rc.im2col(inp["x"], g, Kp)
    assert torch.equal(ref[:, :K], u) and not ref[:, K:].any()
    # the adjoint identity <im2col(x), P> == <x, col2im(P)> in float64
    dx, _, _ = rc.col2im(inp["dp"], g)
    lhs, rhs = (ref[:, :K] * inp["dp"][:, :K].double()).sum(), (inp["x"].double() * dx).sum()
    assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs))


def test_ill_conditioned_channels_are_refused():
    """A channel of two nearly equal large values raises; every listed case does not (the matrix tests above)."""
    x = torch.full((1, 1, 2, 4), 300.0)
    x[0, 0, 1] += 0.001
    w9 = torch.zeros(9, 4)
    w9[4] = 1.0
    with pytest.raises(ValueError, match="ill-conditioned"):
        rc.dwconv_bn_forward(x, w9, torch.ones(4), torch.zeros(4), chain=2)
    for case in WALK_CASES:
        assert dw_case(*case)[1]["rho"].max().item() <= rc.RHO_MAX
