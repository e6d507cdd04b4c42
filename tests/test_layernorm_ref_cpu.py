"""The LayerNorm / column-sum conformance bound (tests/ref_layernorm.py) judged on the CPU: an fp32
emulation of the kernels' arithmetic must pass it for every input family and size, and each of a set
of subtly wrong results must leave the bound on the output named, at the size named.  Measured worst
|err| / tol are in the docstrings.  No GPU."""
from functools import lru_cache

import pytest
import torch

import ref_layernorm as rl

BF = rl.BF
DS, MS = (4, 64, 128, 260, 768, 2048), (67, 2052)
FWD, BWD = ("y", "y_bf16", "mean", "rstd"), ("dx", "dx_lp", "dgamma", "dbeta", "dxsum")


@lru_cache(maxsize=8)
def case(family, M, D):
    return rl.reference(family, M, D)


def fwd_ratios(family, M, D, mut=None):
    inp, fwd, _, _ = case(family, M, D)
    a = rl.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], mut=mut)
    b = rl.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], bf16=True, mut=mut)
    got = {"y": a["y"], "y_bf16": b["y"], "mean": a["mean"], "rstd": a["rstd"]}
    return {k: rl.worst_ratio(got[k], *fwd[k]) for k in FWD}


def bwd_ratios(family, M, D, mut=None, dres=True):
    inp, fwd, bwd, bwd0 = case(family, M, D)
    got = rl.emulate_bwd(inp["x"], fwd["mean_in"], fwd["rstd_in"], inp["gamma"], inp["dy"],
                         inp["dres"] if dres else None, inp["prev"], mut=mut)
    ref = bwd if dres else bwd0
    return {k: rl.worst_ratio(got[k], *ref[k]) for k in BWD}


def show(tag, w):
    print(f"{tag}: " + " ".join(f"{k} {v:.3g}" for k, v in w.items()))
    return w


# ------------------------------------------------------------------ accept
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("D", DS)
def test_emulation_is_within_the_bound(D, M):
    """Accept: worst |err| / tol < 1 for every output and family, with and without dres.  (Measured:
    fp32 outputs <= 0.35, bf16 stores <= 0.996 -- a round-to-nearest store uses the whole half ulp.)"""
    for family in rl.FAMILIES:
        w = show(f"D {D} M {M} {family}", {**fwd_ratios(family, M, D), **bwd_ratios(family, M, D)})
        w0 = bwd_ratios(family, M, D, dres=False)
        assert max(w.values()) < 1.0 and max(w0.values()) < 1.0, (family, w, w0)


def test_const_rows_and_int_sums_are_exact():
    """What the GPU suite asserts bitwise holds in the emulation: a constant row has mean == c and
    y == beta (bf16: bf16(beta)) exactly; integer dy gives dbeta == the exact sum exactly."""
    for D in DS:
        inp, fwd, _, _ = case("const", 67, D)
        rows = rl.const_rows(67)
        for bf in (False, True):
            got = rl.emulate_fwd(inp["x"], inp["gamma"], inp["beta"], bf16=bf)
            assert (got["mean"][rows] == rl.CONST_VALUE).all()
            want = inp["beta"].to(BF) if bf else inp["beta"]
            assert torch.equal(got["y"][rows], want.expand(len(rows), D))
        inp, fwd, bwd, _ = case("int", 2052, D)
        got = rl.emulate_bwd(inp["x"], fwd["mean_in"], fwd["rstd_in"], inp["gamma"], inp["dy"], inp["dres"], inp["prev"])
        assert torch.equal(got["dbeta"].double(), bwd["dbeta"][0])


# ------------------------------------------------------------------ reject: the forward
@pytest.mark.parametrize("D", (64, 192))
def test_rejects_one_pass_variance(D):
    """var = E[x^2] - mu^2 on rows of +-64 + randn: the cancellation costs about 64^2 u = 2.4e-4
    absolute of a variance of 1.  Measured rstd 162 (D = 64), 104 (D = 192), y 5.3 and 2.8; the bound's
    (D + 4) u term grows with D while the cancellation does not, so it is claimed at these two sizes only."""
    assert max(fwd_ratios("offset", 67, D).values()) < 1.0
    w = show(f"onepass D {D}", fwd_ratios("offset", 67, D, "onepass"))
    assert w["rstd"] > 1.0


@pytest.mark.parametrize("D", (4, 64, 260))
def test_rejects_padded_divisor_forward(D):
    """Sums divided by the padded width 256 ceil(D / 256).  Measured mean > 4e3 at every size."""
    w = show(f"paddiv D {D}", fwd_ratios("rows", 67, D, "paddiv"))
    assert w["mean"] > 1.0 and w["rstd"] > 1.0 and w["y"] > 1.0


@pytest.mark.parametrize("D", (64, 768))
def test_rejects_truncating_bf16_store(D):
    """bf16 by dropping the low 16 bits: up to a whole ulp, the bound allows half.  Measured 1.98."""
    w = show(f"trunc D {D}", fwd_ratios("rows", 67, D, "trunc"))
    assert w["y_bf16"] > 1.0 and w["y"] < 1.0


@pytest.mark.parametrize("D", (4, 260))
def test_rejects_shifted_gamma_beta(D):
    w = show(f"shiftgb D {D}", fwd_ratios("rows", 67, D, "shiftgb"))
    assert w["y"] > 1.0 and w["y_bf16"] > 1.0 and w["mean"] < 1.0


@pytest.mark.parametrize("family", ("rows", "randn"))
def test_rejects_statistics_of_the_neighbouring_row(family):
    """mean / rstd written to row + 1.  Measured > 4e3 on ``rows``; ``randn`` rows differ by the sampling
    noise of a 64-term mean alone and still fail."""
    w = show(f"rowplus1 {family}", fwd_ratios(family, 67, 64, "rowplus1"))
    assert w["mean"] > 1.0 and w["rstd"] > 1.0 and w["y"] < 1.0


# ------------------------------------------------------------------ reject: the backward
@pytest.mark.parametrize("D", (64, 260))
def test_rejects_mean_of_the_previous_row(D):
    w = show(f"prevmean D {D}", bwd_ratios("rows", 67, D, "prevmean"))
    assert w["dx"] > 1.0 and w["dgamma"] > 1.0 and w["dbeta"] < 1.0


@pytest.mark.parametrize("D", (4, 64, 260))
def test_rejects_padded_divisor_backward(D):
    w = show(f"paddiv bwd D {D}", bwd_ratios("rows", 67, D, "paddiv"))
    assert w["dx"] > 1.0 and w["dx_lp"] > 1.0 and w["dgamma"] < 1.0


@pytest.mark.parametrize("family", ("rows", "int"))
@pytest.mark.parametrize("M", MS)
def test_rejects_dropped_last_row(M, family):
    """The last row left out of dgamma, dbeta and dxsum.  Measured at M = 67 > 1e3 each; at M = 2052
    dgamma > 35, dxsum > 10 (the (M + 1) u sum|terms| bound grows with M, one row does not)."""
    for D in (64, 260):
        assert max(bwd_ratios(family, M, D).values()) < 1.0
        w = show(f"droplast M {M} D {D} {family}", bwd_ratios(family, M, D, "droplast"))
        assert w["dgamma"] > 1.0 and w["dbeta"] > 1.0 and w["dxsum"] > 1.0 and w["dx"] < 1.0


def test_rejects_dres_of_the_next_row():
    """Every row takes the dres of the row after it (the last one the first row's): dx fails; the column
    sums of dx hold the same terms and pass, which is why dx is judged per element."""
    w = show("dresplus1", bwd_ratios("rows", 67, 128, "dresplus1"))
    assert w["dx"] > 1.0 and w["dx_lp"] > 1.0 and w["dgamma"] < 1.0


def test_rejects_dxsum_before_dres():
    w = show("sumfirst", bwd_ratios("rows", 67, 128, "sumfirst"))
    assert w["dxsum"] > 1.0 and w["dx"] < 1.0


@pytest.mark.parametrize("M", (67, 16))
def test_rejects_neighbouring_sub_row_in_the_row_sum(M):
    """D = 64 (16 lanes per row, four rows per wave): the xor-shuffle reduction carried one step too
    far (offset L = 16) adds the neighbouring sub-row's s1 and s2."""
    w = show(f"xorl M {M}", bwd_ratios("rows", M, 64, "xorl"))
    assert w["dx"] > 1.0 and w["dgamma"] < 1.0


# ------------------------------------------------------------------ reject: the column sums
@pytest.mark.parametrize("mut", ("twice", "dropped"))
@pytest.mark.parametrize("family,M", (("int", 100), ("int", 8193), ("randn", 100)))
def test_rejects_a_row_counted_twice_or_not_at_all(family, M, mut):
    """``int``: the faithful emulation equals the exact sum bitwise (tol is not needed), the mutant does
    not, at any M up to 8209; ``randn`` at M = 100 by the bound."""
    dy, prev = rl.colsum_inputs(family, M, 72)
    ref, tol = rl.colsum(dy, prev)
    good, bad = rl.emulate_colsum(dy, prev), rl.emulate_colsum(dy, prev, mut=mut)
    w = rl.worst_ratio(bad, ref, tol)
    print(f"colsum {family} M {M} {mut}: {w:.3g} (faithful {rl.worst_ratio(good, ref, tol):.3g})")
    assert rl.worst_ratio(good, ref, tol) < 1.0
    if family == "int":
        assert torch.equal(good.double(), ref) and not torch.equal(bad.double(), ref)
    else:
        assert w > 1.0


# ------------------------------------------------------------------ the helpers
def test_split_forms_round_trip():
    """split_x3 / split_f8 / f8_unpack agree with ref_gemm.f8_rows (the layout the GEMM reads) and hi + lo
    and hi + lo8 / 512 are within their bounds of the fp32 value."""
    inp, fwd, _, _ = case("rows", 67, 128)
    y = rl.emulate_fwd(inp["x"], inp["gamma"], inp["beta"])["y"]
    x3 = rl.split_x3(y)
    assert torch.equal(x3[:, :128], x3[:, 128:256])
    assert rl.worst_ratio(x3[:, :128].double() + x3[:, 256:].double(), *fwd["hi+lo"]) < 1.0
    assert rl.worst_ratio(x3[:, :128].double(), *fwd["hi+lo"]) > 1.0          # hi alone is not enough
    hi, hi8, lo8 = rl.split_f8(y)
    for wform in (False, True):
        stored, _ = rl.rg.f8_rows(y, weight=False, wform=wform)
        h, a, b = rl.f8_unpack(stored, 128, wform)
        assert torch.equal(h, hi) and torch.equal(a, hi8) and (wform or torch.equal(b, lo8))
    assert rl.worst_ratio(hi.double() + rl.e4m3_value(lo8) / 512.0, *fwd["hi+lo8"]) < 1.0


def test_guards_detect_a_stray_store():
    p = rl.padded(5, 8, 12, torch.float32, "guard", offset=4)
    p.set(torch.zeros(5, 8))
    assert rl.guards_intact(p)
    for idx in (0, 3, 4 + 3 * 12 - 1, p.start + 8, p.buf.numel() - 1):
        q = p.clone()
        q.buf[idx] = 1.0
        assert not rl.guards_intact(q), idx
    q = p.clone()
    q.view[4, 7] = 1.0
    assert rl.guards_intact(q)


def test_ill_conditioned_rows_are_refused():
    """mean|x| rstd > 2^10 on a row that is not constant raises; a constant row, and every family at
    every size of this file, does not (the families stay under 2^7)."""
    x = torch.full((3, 64), 4096.0)
    x[1, 0] += 1.0
    with pytest.raises(ValueError, match="ill-conditioned"):
        rl.forward(x, torch.ones(64), torch.zeros(64))
    x[1, 0] = 4096.0
    rl.forward(x, torch.ones(64), torch.zeros(64))
    for family in rl.FAMILIES:
        for D in DS:
            A, _, var, rs, _, _ = rl.stats(rl.inputs(family, 67, D)["x"])
            assert (torch.where(var > 0, A * rs, torch.zeros_like(A)) < 2.0 ** 7).all(), (family, D)
