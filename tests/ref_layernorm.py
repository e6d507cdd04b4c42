"""Float64 reference of the LayerNorm entry points (include/vitmi.h vitmi_layernorm_fwd, _bwd) and of
the column sums (vitmi_bias_grad, the dgamma / dbeta / dxsum reductions) with a per-element error
bound DERIVED from the arithmetic, input families and a CPU emulation of the kernels' arithmetic
with its mutants.  Plain torch on the CPU, no GPU.  TEST INFRASTRUCTURE ONLY (the counterpart of
tests/ref_gemm.py and tests/ref_attention.py, whose guarded buffers and constants it reuses).

Inputs are taken as stored and as exact (``eps`` as the float32 the API receives).  Every output
comes back as ``(ref, tol)`` in float64: a result conforms iff |got - ref| <= tol for EVERY element.

Notation.  u = 2^-24 (U32), ubf = 2^-8 (UBF).  Per row, in float64: A = mean|x|, mu, var,
rs = (var + eps)^-1/2.  "Any order" is the (n + 1) u sum|terms| rule of the GEMM suite for an n-term
fp32 sum: the kernels sum 4 columns per lane, then lanes by xor shuffles, then waves, blocks and the
fold, and no particular order is assumed.

Forward (csrc/layernorm.hip ln_fwd_kernel, ln_fwd_small_kernel).
  mean   e_mu = (D + 1) u A                    the row sum in any order;
         tol = e_mu + u |mu|                   the division
  rstd   the variance is taken about the COMPUTED mean: sum (x - mu')^2 / D = var + (mu' - mu)^2, so
         a shift e_mu enters only squared.
         rho = ((D + 4) u + e_mu^2 / (var + eps)) / 2 + T_FN_ULPS u
                                               D-term sum of squares (each square carries 2u from
                                               the rounded difference and 1u of its own, inside the
                                               + 4), / D, + eps; half of it through the power
                                               -1/2; rsqrtf
         tol = rs rho
  xhat   t_xh = rs (e_mu + u (|x| + |mu|)) + |xhat| (rho + 2u)
                                               the difference (the mean's error and its rounding),
                                               rstd's relative error, the two products
  y      |gamma| t_xh + 2u (|y| + |beta|)      times gamma (or one fma), plus beta
         bf16 store: + ubf |y| (half a bf16 ulp at the least: a truncating store fails)
  x3     rows [hi | hi | lo]: hi within the bf16 bound, hi + lo within the fp32 bound + ubf^2 |y|
  f8     rows [hi | hi8 | lo8] (f8w: [hi | hi8]): hi within the bf16 bound, hi + lo8 / 512 within the
         fp32 bound + 2^-4 ubf |y| + 2^-19 (lo = y - hi is below ubf |y|, e4m3 rounds it to 2^-4
         relative; ADDED to the starting derivation: below 2^-6 the scaled low part 512 lo is an e4m3
         subnormal with spacing 2^-9, so its rounding is absolute, 2^-10 / 512 = 2^-19, and that exceeds
         the relative term for |y| < 2^-7.  Seen with the exact CPU split at D = 512, ratio 4.3 without
         it.  The saturation at 512 |lo| > 448 needs |y| > 224: not reached by any family)

Backward (ln_bwd_kernel, ln_bwd_small_kernel).  A function of the GIVEN mean and rstd (the reference's,
rounded to fp32), exactly as the API defines it: judged alone.
  gy = dy gamma, c1 = mean(gy), c2 = mean(gy xhat), dxn = rs (gy - c1 - xhat c2), dx = dxn + dres
  t_xh  = u (|x| + |mu|) rs + 2u |xhat|        mean and rstd are exact inputs here
  e1    = (D + 2) u mean|gy|                   any order, gy's own rounding, the division
  e2    = (D + 4) u mean|gy xhat| + mean(|gy| t_xh)
  t_in  = e1 + |xhat| e2 + t_xh |c2| + 4u (|gy| + |c1| + |xhat c2|)
  dx    rs t_in + 2u |dxn| + u (|dres| + |dx|);  the bf16 copy: + ubf |dx|
  dgamma  (M + 3) u sum_m |dy xhat| + sum_m |dy| t_xh + u (|prev| + |ref|)
  dbeta   (M + 1) u sum_m |dy| + u (|prev| + |ref|)
  dxsum   (M + 1) u sum_m |dx| + sum_m tol_dx + u (|prev| + |ref|)     the kernel sums what it stored
The three reductions accumulate (+=) onto ``prev``.

Bias gradient (colsum8_kernel / colsum_kernel + fold_kernel): (M + 1) u sum_m |dy| + u (|prev| + |ref|).

The e4m3 floor above is the one term added to the starting derivation, and it came from the CPU split,
not from a kernel; the MI355X kernels needed none (DESIGN.md has the measured ratios: fp32 outputs
<= 0.49 of the bound, bf16 stores <= 0.996).

Conditioning.  ``forward`` refuses (raises) a non-constant row with A rs > 2^10: there xhat is a
difference of nearly equal numbers and no fp32 LayerNorm is accurate.  A condition on the inputs, not
a tolerance; the families below stay under 2^7.

Input families (``inputs``), all seeded:
  randn   x = 2 randn + 0.5
  rows    x_m = (1 + m % 5) randn + 0.5 (m % 7), dy_m *= 1 + m % 3: neighbouring rows differ in mean,
          rstd, c1 and c2, so a row that reads its neighbour's statistics shows
  offset  x_m = +-64 + randn (the sign alternates by row): the one-pass variance's cancellation.  The
          randn part is standardised per row: four samples (D = 4) can lie within 0.05 of each other,
          and 64 + such a row is past the conditioning limit (seen at D = 4, M = 2052: A rs = 1.2e3)
  const   rows 1, M // 2 and M - 1 hold the single value 3.25 (D x 3.25 and every partial sum of it
          are exact in fp32): mean == 3.25 and y == beta BITWISE, rstd within rho of eps^-1/2
  int     dy (and the bias-gradient input) are integers in [-8, 8] and prev small integers: with
          M <= 8209 every fp32 partial sum is exact in any order, so dbeta and the bias gradient
          equal the exact sum BITWISE and no order can hide a row counted twice or not at all
"""
from __future__ import annotations

import numpy as np
import torch

import ref_gemm as rg
from ref_gemm import BF, T_FN_ULPS, U32, UBF, Padded, guards_intact, padded, worst_ratio  # noqa: F401

F32 = torch.float32
EPS = 1e-6
FAMILIES = ("randn", "rows", "offset", "const", "int")
CONST_VALUE = 3.25
COND_MAX = 2.0 ** 10
INT_ROWS_MAX = 8209
E4_REL = 2.0 ** -4          # e4m3: 3 mantissa bits, half an ulp relative
E4_LO_FLOOR = 2.0 ** -19    # half the e4m3 subnormal spacing 2^-9 of the low part, which is scaled by 2^9


def f32_eps(eps=EPS) -> float:
    """eps as the API receives it: a float32."""
    return float(np.float32(eps))


def const_rows(M):
    return sorted({r for r in (1, M // 2, M - 1) if 0 <= r < M})


# --------------------------------------------------------------------------- inputs
def inputs(family, M, D, seed=11):
    """{x, gamma, beta, dy, dres [fp32], prev [3, D]: what dgamma, dbeta, dxsum hold before the call}."""
    assert family in FAMILIES, family
    g = torch.Generator().manual_seed(seed * 1000003 + M * 4099 + D)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    m = torch.arange(M).view(M, 1)
    x = 2 * rn(M, D) + 0.5
    dy = rn(M, D)
    if family == "rows":
        x = rn(M, D) * (1 + m % 5).float() + 0.5 * (m % 7).float()
        dy = dy * (1 + m % 3).float()
    elif family == "offset":
        z = rn(M, D)
        z = (z - z.mean(1, keepdim=True)) / z.std(1, unbiased=False, keepdim=True)
        x = z + 64.0 * (1 - 2 * (m % 2)).float()
    elif family == "const":
        x[const_rows(M)] = CONST_VALUE
    prev = 0.5 * rn(3, D)
    if family == "int":
        assert M <= INT_ROWS_MAX
        dy = torch.randint(-8, 9, (M, D), generator=g).float()
        prev = torch.randint(-4, 5, (3, D), generator=g).float()
    return dict(x=x, gamma=1 + 0.3 * rn(D), beta=0.2 * rn(D), dy=dy, dres=rn(M, D), prev=prev)


def colsum_inputs(family, M, N, seed=5):
    """(dy [M, N] fp32 holding bf16-exact values, prev [N]) of the bias gradient."""
    g = torch.Generator().manual_seed(seed * 1000003 + M * 4099 + N)
    if family == "int":
        assert M <= INT_ROWS_MAX
        return torch.randint(-8, 9, (M, N), generator=g).float(), torch.randint(-4, 5, (N,), generator=g).float()
    assert family == "randn", family
    m = torch.arange(M).view(M, 1)
    dy = torch.randn(M, N, generator=g) * (1 + m % 3).float() + 0.25
    return dy.to(BF).float(), 0.5 * torch.randn(N, generator=g)


# --------------------------------------------------------------------------- float64 reference
def stats(x, eps=EPS):
    """(A, mu, var, rs, e_mu, rho) per row, float64 [M, 1]."""
    X = x.double()
    D = X.shape[1]
    A = X.abs().mean(1, keepdim=True)
    mu = X.mean(1, keepdim=True)
    var = ((X - mu) ** 2).mean(1, keepdim=True)
    ve = var + f32_eps(eps)
    rs = ve ** -0.5
    e_mu = (D + 1) * U32 * A
    rho = ((D + 4) * U32 + e_mu ** 2 / ve) / 2 + T_FN_ULPS * U32
    return A, mu, var, rs, e_mu, rho


def forward(x, gamma, beta, eps=EPS):
    """{mean, rstd, y, y_bf16, hi+lo, hi+lo8: (ref, tol)} plus mean_in / rstd_in, the statistics rounded
    to fp32 that the backward is fed.  Raises ValueError on an ill-conditioned row."""
    X, g, b = x.double(), gamma.double(), beta.double()
    A, mu, var, rs, e_mu, rho = stats(x, eps)
    cond = torch.where(var > 0, A * rs, torch.zeros_like(A))
    if (cond > COND_MAX).any():
        raise ValueError(f"layernorm reference: ill-conditioned row, mean|x| rstd = {cond.max().item():.3g} > 2^10")
    xhat = (X - mu) * rs
    t_xh = rs * (e_mu + U32 * (X.abs() + mu.abs())) + xhat.abs() * (rho + 2 * U32)
    y = xhat * g + b
    tol = g.abs() * t_xh + 2 * U32 * (y.abs() + b.abs())
    return {"mean": (mu[:, 0], (e_mu + U32 * mu.abs())[:, 0]), "rstd": (rs[:, 0], (rs * rho)[:, 0]),
            "y": (y, tol), "y_bf16": (y, tol + UBF * y.abs()),
            "hi+lo": (y, tol + UBF * UBF * y.abs()), "hi+lo8": (y, tol + E4_REL * UBF * y.abs() + E4_LO_FLOOR),
            "mean_in": mu[:, 0].float(), "rstd_in": rs[:, 0].float()}


def backward(x, mean, rstd, gamma, dy, dres, prev):
    """{dx, dx_lp, dgamma, dbeta, dxsum: (ref, tol)} from the GIVEN fp32 mean / rstd; dres may be None;
    prev [3, D] is what dgamma, dbeta, dxsum held."""
    X, g, DY = x.double(), gamma.double(), dy.double()
    M, D = X.shape
    mu, rs = mean.double().view(M, 1), rstd.double().view(M, 1)
    R = torch.zeros_like(X) if dres is None else dres.double()
    P = prev.double()
    xhat = (X - mu) * rs
    t_xh = U32 * (X.abs() + mu.abs()) * rs + 2 * U32 * xhat.abs()
    gy = DY * g
    c1 = gy.mean(1, keepdim=True)
    c2 = (gy * xhat).mean(1, keepdim=True)
    e1 = (D + 2) * U32 * gy.abs().mean(1, keepdim=True)
    e2 = (D + 4) * U32 * (gy * xhat).abs().mean(1, keepdim=True) + (gy.abs() * t_xh).mean(1, keepdim=True)
    t_in = e1 + xhat.abs() * e2 + t_xh * c2.abs() + 4 * U32 * (gy.abs() + c1.abs() + (xhat * c2).abs())
    dxn = rs * (gy - c1 - xhat * c2)
    dx = dxn + R
    t_dx = rs * t_in + 2 * U32 * dxn.abs() + U32 * (R.abs() + dx.abs())
    out = {"dx": (dx, t_dx), "dx_lp": (dx, t_dx + UBF * dx.abs())}

    def acc(i, terms, t):
        ref = P[i] + terms.sum(0)
        return ref, t + U32 * (P[i].abs() + ref.abs())

    out["dgamma"] = acc(0, DY * xhat, (M + 3) * U32 * (DY * xhat).abs().sum(0) + (DY.abs() * t_xh).sum(0))
    out["dbeta"] = acc(1, DY, (M + 1) * U32 * DY.abs().sum(0))
    out["dxsum"] = acc(2, dx, (M + 1) * U32 * dx.abs().sum(0) + t_dx.sum(0))
    return out


def reference(family, M, D, eps=EPS, seed=11):
    """The inputs of a family with the forward and the backward references: (inp, fwd, bwd, bwd without
    dres).  The backward is fed fwd['mean_in'] / fwd['rstd_in']."""
    inp = inputs(family, M, D, seed)
    fwd = forward(inp["x"], inp["gamma"], inp["beta"], eps)
    args = (inp["x"], fwd["mean_in"], fwd["rstd_in"], inp["gamma"], inp["dy"])
    return inp, fwd, backward(*args, inp["dres"], inp["prev"]), backward(*args, None, inp["prev"])


def colsum(dy, prev):
    """(ref, tol) of the bias gradient db = prev + sum_m dy."""
    DY, P = dy.double(), prev.double()
    ref = P + DY.sum(0)
    return ref, (DY.shape[0] + 1) * U32 * DY.abs().sum(0) + U32 * (P.abs() + ref.abs())


# --------------------------------------------------------------------------- the split row forms
def e4m3(v):
    """fp32 -> e4m3 bytes (OCP, round to nearest even, saturating at +-448 as the kernels do)."""
    return rg._e4m3(v).view(torch.uint8)


def split_x3(y):
    """fp32 y [M, D] -> bf16 [M, 3D] rows [hi | hi | lo] (csrc/layernorm.hip SplitX3)."""
    y = y.float()
    hi = y.to(BF)
    return torch.cat([hi, hi, (y - hi.float()).to(BF)], 1)


def split_f8(y):
    """fp32 y -> (hi bf16, hi8 bytes, lo8 bytes) on the CPU (tests/test_gpu_f8.py's reference too)."""
    y = y.float().cpu()
    hi = y.to(BF)
    return hi, e4m3(hi.float()), e4m3((y - hi.float()) * 512.0)


def f8_unpack(rows, D, wform=False):
    """bf16-unit rows [M, 2D] ([M, 1.5D] for the weight-side form) -> (hi bf16 [M, D], hi8 bytes, lo8
    bytes or None): the e4m3 part in 64-column blocks [hi8 | lo8] (common.h f8_off), one byte per
    column for the weight-side form."""
    rows = rows.contiguous().cpu()
    M = rows.shape[0]
    by = rows.view(torch.uint8)[:, 2 * D:]
    if wform:
        return rows[:, :D], by[:, :D], None
    b = by.reshape(M, D // 64, 2, 64)
    return rows[:, :D], b[:, :, 0].reshape(M, D), b[:, :, 1].reshape(M, D)


def e4m3_value(b):
    return b.contiguous().view(rg.E4).double()


# --------------------------------------------------------------------------- CPU emulation
def padded_divisor(D):
    return 256 * -(-D // 256)


def emulate_fwd(x, gamma, beta, eps=EPS, bf16=False, mut=None):
    """The forward kernels' arithmetic in float32: two-pass variance, (x - mu) * rs * g + b, a
    round-to-nearest bf16 store.  Returns {y, mean, rstd}.  Mutants: 'onepass' (E[x^2] - mu^2),
    'paddiv' (the divisor rounded up to the vector width), 'trunc' (a truncating bf16 store),
    'shiftgb' (gamma / beta of the next column), 'rowplus1' (mean / rstd written to row + 1)."""
    x, g, b = x.float(), gamma.float(), beta.float()
    M, D = x.shape
    div = float(padded_divisor(D) if mut == "paddiv" else D)
    e = torch.tensor(f32_eps(eps), dtype=F32)
    mu = x.sum(1, keepdim=True) / div
    if mut == "onepass":
        var = (x * x).sum(1, keepdim=True) / div - mu * mu
    else:
        d = x - mu
        var = (d * d).sum(1, keepdim=True) / div
    rs = torch.rsqrt(var + e)
    if mut == "shiftgb":
        g, b = g.roll(-1), b.roll(-1)
    y = (x - mu) * rs * g + b
    if bf16:
        y = rg.bf16_trunc(y) if mut == "trunc" else rg.bf16_rne(y)
    mean, rstd = mu[:, 0].clone(), rs[:, 0].clone()
    if mut == "rowplus1":
        mean, rstd = mean.roll(1), rstd.roll(1)
    return {"y": y, "mean": mean, "rstd": rstd}


def emulate_bwd(x, mean, rstd, gamma, dy, dres, prev, mut=None):
    """The backward as written in ln_bwd_kernel, in float32, the reductions in 4-row groups (a block's
    four waves) and then over the groups.  Returns {dx, dx_lp, dgamma, dbeta, dxsum}.  Mutants:
    'prevmean' (mean of the previous row), 'paddiv' (c1, c2 over the padded width), 'droplast' (the last
    row left out of the three reductions), 'dresplus1' (dres of row + 1), 'sumfirst' (dxsum summed before
    dres is added), 'xorl' (D = 64: the row sums take in the neighbouring sub-row's lanes)."""
    x, g, dy = x.float(), gamma.float(), dy.float()
    M, D = x.shape
    mu, rs = mean.float().view(M, 1), rstd.float().view(M, 1)
    r = torch.zeros_like(x) if dres is None else dres.float()
    if mut == "prevmean":
        mu = mu.roll(1, 0)
    if mut == "dresplus1":
        r = r.roll(-1, 0)
    div = float(padded_divisor(D) if mut == "paddiv" else D)
    xh = (x - mu) * rs
    gy = dy * g
    s1, s2 = gy.sum(1, keepdim=True), (gy * xh).sum(1, keepdim=True)
    if mut == "xorl":
        partner = torch.arange(M) ^ 1
        live = (partner < M).float().view(M, 1)
        partner = partner.clamp_max(M - 1)
        s1, s2 = s1 + s1[partner] * live, s2 + s2[partner] * live
    c1, c2 = s1 / div, s2 / div
    core = (gy - c1 - xh * c2) * rs
    dx = core + r
    n = M - 1 if mut == "droplast" else M

    def red(t, i):
        t = t[:n]
        pad = (-t.shape[0]) % 4
        t = torch.cat([t, torch.zeros(pad, D)], 0).view(-1, 4, D).sum(1).sum(0)
        return prev[i].float() + t

    return {"dx": dx, "dx_lp": rg.bf16_rne(dx), "dgamma": red(dy * xh, 0), "dbeta": red(dy, 1),
            "dxsum": red(core if mut == "sumfirst" else dx, 2)}


def emulate_colsum(dy, prev, chunk=32, mut=None):
    """The bias gradient in float32: per-chunk partial rows, then their fold.  Mutants: 'twice' (one row
    added twice), 'dropped' (one row left out)."""
    dy = dy.float()
    M = dy.shape[0]
    if mut == "twice":
        dy = torch.cat([dy, dy[M // 2:M // 2 + 1]], 0)
    elif mut == "dropped":
        dy = torch.cat([dy[:M // 2], dy[M // 2 + 1:]], 0)
    parts = torch.stack([c.sum(0) for c in dy.split(chunk, 0)], 0) if dy.shape[0] else torch.zeros(1, dy.shape[1])
    return prev.float() + parts.sum(0)
