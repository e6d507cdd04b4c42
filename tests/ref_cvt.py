"""Float64 reference of the CvT convolution entry points (include/vitmi.h: vitmi_conv_same_geometry,
vitmi_conv_im2col, _col2im, vitmi_dwconv_bn_fwd, _bwd, vitmi_avgpool3_fwd, _bwd; csrc/cvt.hip) with a
per-element error bound DERIVED from the arithmetic, input families, and a CPU emulation of the kernels'
arithmetic with its mutants.  Plain torch on the CPU, no GPU.  TEST INFRASTRUCTURE ONLY (the counterpart
of tests/ref_layernorm.py, whose guarded buffers and constants it reuses through tests/ref_gemm.py).

Tensors are logical NHWC [B, H, W, C]; ``rows`` lays one out as the token rows the library reads (image b
pixel p at row b * img + off + p).  Inputs are taken as stored (a bf16 input rounded first) and as exact,
``eps`` and ``momentum`` as the float32 the API receives.  Every output comes back as ``(ref, tol)`` in
float64: a result conforms iff |got - ref| <= tol for EVERY element.

Notation.  u = 2^-24 (U32), ubf = 2^-8 (UBF).  "Any order" is the (m + 1) u sum|terms| rule of the GEMM
suite for an m-term fp32 sum: no particular order is assumed.  n = B H W, the pixels per channel.

im2col      a copy: fp32 BITWISE the value, bf16 BITWISE its round-to-nearest-even (tol = 0: a truncating
            store fails); columns K..Kp-1 and every out-of-image tap are +0.
col2im      dx = sum over the t windows (oh, ow, i, j) that read the pixel, t <= ceil(kh/s) ceil(kw/s):
            (t + 1) u sum|terms|; with ``accumulate`` + u (|prev| + |ref|).  A pixel no window reads
            (k < s) is exactly 0, or ``prev`` BITWISE with accumulate (tol = 0).
avgpool fwd y = r sum x over the t in-image taps, r = 1/t (1/9 with count_pad):
            (t + 1) u r sum|x| + 2u |y|   (the rounded reciprocal and the product); bf16 store + ubf |y|.
avgpool bwd dx = prev + sum_q dy[q] r[q]: every term carries its own rounded reciprocal and product (2u),
            the sum follows the (t + 1) u rule, the += onto prev adds u (|prev| + |ref|):
            (t + 3) u sum|terms| + u (|prev| + |ref|).

dw_bn forward (dw_fwd_stats_rows_kernel, bn_finalize_kernel, bn_apply_kernel).
  z      tol_z = 10 u sum|w x| over the in-image taps (<= 9 products, <= 9 adds).
  mean   an m-term fp32 sum of z AS COMPUTED has m - 1 additions (the first lands on an exact 0) and the
         division is fp64: e_s = (m - 1) u mean|z|, e_mu = e_s + mean(tol_z);
         tol = e_mu + u |mu| (the rounding to fp32).
  rstd   the one-pass variance mean(z'^2) - mu'^2, BOTH moments of the same computed z' = z + d, |d| <= tol_z.
         Its exact value is var(z'), and var(z + d) = var + 2 cov(z, d) + var(d) with |cov| <= sigma rms(d):
         a common shift of z cancels.  On top of that come the two sums' own roundings:
           e_var = m u mean(z^2)                    m - 1 additions and each square's one rounding
                 + 2 sigma rms(tol_z) + mean(tol_z^2)  var(z') for var(z)
                 + 2 |mu| e_s + e_s^2               the sum's rounding in mu'^2
                 + 2u mu^2                          the fp64 finish, generously
           d = e_var / (var + eps);  rho = d (1 + d) / 2 + 4u
         This is SHARPER than the starting derivation ((n + 3) u mean(z^2) + 2 mean(|z| tol_z) + 2 |mu| e_mu
         + e_mu^2 + 2u mu^2, e_mu with its (n + 1) u): that one charges a one-pixel channel (n = 1: var' =
         fl(z^2) - z^2, within u z^2) 50 u z^2 and so calls every family ill-conditioned at B = H = W = 1,
         eps = 1e-3 (rho up to 0.14 at C = 1024).  Counting the roundings that exist keeps those cases in.
         (1 + x)^-1/2 - 1 is within |x| (1 + |x|) / 2 of 0 for |x| <= 2^-5: the first-order d / 2 of the
         starting derivation with its remainder (ADDED: at rho = 2^-6 the remainder is 3% of it); 4u: the
         rounding of rstd to fp32, sqrt and the division in fp64.  tol = rstd rho.
         The clamp var' >= 0 only moves var' towards var >= 0.
  y      as LayerNorm's: t_zh = rs (tol_z + tol_mean + u (|z| + |mu|)) + |zh| (rho + 2u);
         tol = |gamma| t_zh + 2u (|y| + |beta|); bf16 store + ubf |y|.
  moving statistics  ref = m old + (1 - m) stat with (1 - m) as the fp32 difference the kernel forms:
         tol = |1 - m| tol_stat + 2u (|m old| + |(1 - m) stat|); stat = mu, or the unbiased variance
         var n / (n - 1) (n = 1: var) with tol_stat = e_var n / (n - 1) + u var_u (its rounding to fp32).
  inference (training = 0)  mean == run_mean BITWISE, rstd = (run_var + eps)^-1/2 within 4u, the moving
         statistics untouched; y by the same formula with e_mu = 0, rho = 4u.
  m is n, the any-order rule over every pixel of the channel, unless ``chain`` is given (see below).

dw_bn backward (bn_bwd_stats_kernel, bn_bwd_finalize_kernel, dw_bwd_dz_rows_kernel, dw_wgrad_finalize_kernel,
dw_bwd_dx_rows_kernel).  A function of the GIVEN z, mean and rstd (the reference's, rounded to fp32): judged
alone.  zh = (z - mu) rs, k1 = mean(dy), k2 = mean(dy zh), dz = gamma rs (dy - k1 - zh k2).
  t_zh   = u (|z| + |mu|) rs + 2u |zh|
  dbeta  = prev + sum dy:     (m + 1) u sum|dy| + u (|prev| + |ref|)
  dgamma = prev + sum dy zh:  (m + 3) u sum|dy zh| + sum|dy| t_zh + u (|prev| + |ref|)
  e1 = (m + 1) u mean|dy| + u |k1|;  e2 = (m + 3) u mean|dy zh| + mean(|dy| t_zh) + u |k2|
  t_in   = e1 + |zh| e2 + t_zh |k2| + 4u (|dy| + |k1| + |zh k2|)
  tol_dz = |gamma rs| t_in + 3u |dz|            (gamma rs is rounded, then the product)
  dx     = prev + sum_taps w dz (the flipped window): sum|w| tol_dz + 10u sum|w dz| + u (|prev| + |ref|)
  dw9    = prev + sum_p dz[p] x[p + tap]:  (m + 3) u sum|dz x| + sum tol_dz |x| + u (|prev| + |ref|)

The chain.  With m = n the rule allows ANY fp32 summation of the n terms, so a variance accumulated
ENTIRELY in fp32 (the mutant 'fp32var') conforms by construction and no case can reject it.  m is
therefore the longest fp32 chain csrc/cvt.hip's header documents: a thread's own partial (the image rows
it walks x W pixels for the *_rows kernels, the pixels it walks for bn_bwd_stats_kernel), then the other
``lanes`` - 1 partials of its block; everything after that is fp64.
``chain_rows`` / ``chain_pixels`` compute it from the host formulas (``dw_blocks``), and the GPU suite
asserts those formulas against the library's workspace size.  m <= n always, so this bound is the tighter.
Even so the BOUND does not reject 'fp32var' at any size a test can afford: on ``offset`` the bound allows
about 3 m u mean(z^2) + 2 sigma rms(tol_z), 29 u mean(z^2) at m = 8, and one fp32 running sum over n
terms measures 4 u mean(z^2) at n = 400 (0.14 of the bound on rstd), growing like sqrt(n): it would
need n > 20000 at C = 1024.  What rejects it is the ``ramp`` pin on the mean: the kernel's partial sums are
exact there and a running sum over the whole channel is not (test_cvt_ref_cpu.py names the cases).

Conditioning.  A condition on the inputs, not a tolerance: ``dwconv_bn_forward`` raises if any channel's
rho exceeds 2^-6 (there rstd itself is not determined by fp32 arithmetic).  No listed case triggers it:
with eps = 1e-3 the worst rho of a listed case is 0.0106 (``offset`` at n = 2, where two pixels of a
channel lie close together around |z| = 12 and var + eps is little more than eps).  ``offset`` is listed
for n <= 2048 only (``offset_ok``), the limit the n-term rule's estimate gave it; with the chain the
condition holds with room to spare there (rho 1.4e-4 at n = 1536) and no larger ``offset`` case is listed.

Input families (``dw_inputs`` / ``conv_inputs``), all seeded per shape:
  randn   x = randn, w = 0.3 randn, gamma = 1 + 0.3 randn, beta = 0.2 randn, dy = randn, prev = 0.5 randn
  chan    channel c has x scaled by 1 + c % 5 and shifted by 0.5 (c % 7), dy scaled by 1 + c % 3; image b
          is shifted by 0.25 b: neighbouring channels, lanes and images differ in mu, rstd, k1 and k2
  offset  x = +-8 + randn (the sign alternates by channel): the one-pass variance's cancellation
  ramp    x[b, h, w, c] = ((1 + c % 4) p + c % 4) % 251 with p the pixel's index in (b, h, w): small distinct
          integers; w a 3x3 of the nine powers of two 2^-8 .. 1 (tap k of channel c holds 2^((k + c) % 9 - 8)).
          PINS: every z BITWISE equal to the reference (all partial sums are integers / 256 below 2^24), and
          mean BITWISE fl32(sum z / n) wherever the chain's partial sums stay below 2^24 / 256 (``chain_exact``)
  int     dy, dpatches and x are integers in [-8, 8], prev small integers.
          PINS: dbeta BITWISE the exact sum (n <= 2^20); col2im BITWISE the exact sum; avgpool forward
          BITWISE fl(S fl(1 / t)) with S the exact integer tap sum (count_pad: t = 9), fp32 output
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from ref_gemm import BF, U32, UBF, Padded, guards_intact, padded, worst_ratio, bf16_rne, bf16_trunc  # noqa: F401

F32, F64 = torch.float32, torch.float64
EPS, MOMENTUM = 1e-3, 0.99
RHO_MAX = 2.0 ** -6
FAMILIES = ("randn", "chan", "offset", "ramp", "int")
DW_CHANNELS = (4, 8, 16, 32, 64, 128, 256, 512, 1024)
CVT_BLOCKS = 4096           # csrc/cvt.hip: the cap of the grid-stride kernels' grids (256 threads each)
NAN = float("nan")


def offset_ok(n) -> bool:
    """The sizes at which the ``offset`` family is listed (see Conditioning)."""
    return n <= 2048


def f32(v) -> float:
    """A Python float as the API receives it: a float32."""
    return float(np.float32(v))


def cdiv(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------- host formulas of csrc/cvt.hip
def dw_channels_ok(C):
    return C >= 4 and C % 4 == 0 and 1024 % C == 0


def dw_blocks(n, C):
    lanes = 256 // (C // 4)
    return max(1, min(1024, cdiv(n, lanes * 8)))


def dw_workspace_size(B, H, W, C):
    n = B * H * W
    return dw_blocks(n, C) * 9 * C * 4 + n * C * 4 + 2 * C * 4


def rows_grid(B, H, W, C):
    """(G, lanes, most image rows one thread walks) of the *_rows kernels."""
    lanes = 256 // (C // 4)
    G = min(cdiv(B * H * (C // 4), 256), dw_blocks(B * H * W, C))
    return G, lanes, cdiv(B * H, G * lanes)


def chain_rows(B, H, W, C):
    """The terms of the longest fp32 chain of the row-walking statistics: a thread's rows x W, then its
    block's other ``lanes`` - 1 partials."""
    G, lanes, per = rows_grid(B, H, W, C)
    return min(B * H * W, per * W + lanes - 1)


def chain_pixels(B, H, W, C):
    """The same for bn_bwd_stats_kernel: the pixels one thread walks, then ``lanes``."""
    n, lanes = B * H * W, 256 // (C // 4)
    return min(n, cdiv(n, dw_blocks(n, C) * lanes) + lanes - 1)


# --------------------------------------------------------------------------- conv geometry
Geo = namedtuple("Geo", "B H W C kh kw s pt pl Ho Wo")


def same_pad(H, k, s, mut=None):
    """TF 'same': (Ho, pad_before) = (ceil(H / s), floor(max((Ho - 1) s + k - H, 0) / 2)).  Mutant
    'padceil': pad_before = ceil of the total."""
    Ho = cdiv(H, s)
    tot = max((Ho - 1) * s + k - H, 0)
    return Ho, (cdiv(tot, 2) if mut == "padceil" else tot // 2)


def same_geo(B, H, W, C, kh, kw, s, mut=None):
    (Ho, pt), (Wo, pl) = same_pad(H, kh, s, mut), same_pad(W, kw, s, mut)
    return Geo(B, H, W, C, kh, kw, s, pt, pl, Ho, Wo)


def geo_ok(g):
    """What make_geo of csrc/cvt.hip accepts."""
    return (min(g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, g.Ho, g.Wo) > 0 and 0 <= g.pt < g.kh and 0 <= g.pl < g.kw
            and (g.Ho - 1) * g.s - g.pt < g.H and (g.Wo - 1) * g.s - g.pl < g.W)


def _padded_hw(g):
    return max(g.pt + g.H, (g.Ho - 1) * g.s + g.kh), max(g.pl + g.W, (g.Wo - 1) * g.s + g.kw)


def _win(g, i, j):
    return (slice(None), slice(i, i + (g.Ho - 1) * g.s + 1, g.s), slice(j, j + (g.Wo - 1) * g.s + 1, g.s))


def im2col(x, g, Kp):
    """patches [B Ho Wo, Kp] float64 of x [B, H, W, C]: column (i, j, c) of row (b, oh, ow) is
    x[b, oh s - pt + i, ow s - pl + j, c], 0 outside the image and in columns K..Kp-1.  The value is exact:
    compare bitwise (a bf16 output with its round-to-nearest-even)."""
    K = g.kh * g.kw * g.C
    Hp, Wp = _padded_hw(g)
    xp = torch.zeros(g.B, Hp, Wp, g.C, dtype=F64)
    xp[:, g.pt:g.pt + g.H, g.pl:g.pl + g.W] = x.double()
    cols = [xp[_win(g, i, j)] for i in range(g.kh) for j in range(g.kw)]
    out = torch.zeros(g.B * g.Ho * g.Wo, Kp, dtype=F64)
    out[:, :K] = torch.stack(cols, 3).reshape(-1, K)
    return out


def col2im(dp, g, prev=None):
    """(ref, tol, t) of dx [B, H, W, C] = (prev +) the adjoint of im2col applied to dp [rows, >= K] as stored;
    t [H, W] is the number of windows that read the pixel."""
    K = g.kh * g.kw * g.C
    D = dp[:, :K].double().reshape(g.B, g.Ho, g.Wo, g.kh, g.kw, g.C)
    Hp, Wp = _padded_hw(g)
    acc, ab = torch.zeros(g.B, Hp, Wp, g.C, dtype=F64), torch.zeros(g.B, Hp, Wp, g.C, dtype=F64)
    cnt = torch.zeros(1, Hp, Wp, 1, dtype=F64)
    for i in range(g.kh):
        for j in range(g.kw):
            acc[_win(g, i, j)] += D[:, :, :, i, j]
            ab[_win(g, i, j)] += D[:, :, :, i, j].abs()
            cnt[_win(g, i, j)] += 1
    crop = (slice(None), slice(g.pt, g.pt + g.H), slice(g.pl, g.pl + g.W))
    acc, ab, cnt = acc[crop], ab[crop], cnt[crop]
    assert cnt.max() <= cdiv(g.kh, g.s) * cdiv(g.kw, g.s)
    tol = (cnt + 1) * U32 * ab
    ref = acc
    if prev is not None:
        ref = prev.double() + acc
        tol = tol + U32 * (prev.double().abs() + ref.abs())
    tol = torch.where(cnt > 0, tol, torch.zeros_like(tol))
    return ref, tol, cnt[0, :, :, 0]


# --------------------------------------------------------------------------- 3x3 windows
def shift(x, di, dj, relax=None):
    """t[b, h, w] = x[b, h + di, w + dj], 0 outside the image.  ``relax`` (emulation mutants) drops one
    border test -- 'left', 'right', 'bottom' -- so the tap reads the pixel at that distance in the flat
    [B H W] row order instead (the previous row's end, the next row's start, the next image; NaN past
    either end of the buffer)."""
    B, H, W, C = x.shape
    if relax is None:
        return F.pad(x, (0, 0, 1, 1, 1, 1))[:, 1 + di:1 + di + H, 1 + dj:1 + dj + W]
    n = B * H * W
    guard = torch.full((W + 1, C), NAN, dtype=x.dtype)
    flat = torch.cat([guard, x.reshape(n, C), guard])
    p = torch.arange(n)
    h, w = (p // W) % H, p % W
    okh = (h + di >= 0) & ((h + di < H) | (relax == "bottom"))
    okw = ((w + dj >= 0) | (relax == "left")) & ((w + dj < W) | (relax == "right"))
    v = flat[p + di * W + dj + W + 1]
    return torch.where((okh & okw).view(n, 1), v, torch.zeros_like(v)).view(B, H, W, C)


def taps_in(H, W):
    """[H, W] float64: the number of in-image taps of the 3x3 window centred on each pixel."""
    one = torch.ones(1, H, W, 1, dtype=F64)
    return sum(shift(one, di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1))[0, :, :, 0]


def avgpool_fwd(x, count_pad):
    """{y, y_bf16: (ref, tol)} of the 3x3 stride-1 'same' average; S: the tap sum."""
    X = x.double()
    B, H, W, C = X.shape
    t = taps_in(H, W).view(1, H, W, 1)
    r = torch.full_like(t, 1 / 9) if count_pad else 1 / t
    S = sum(shift(X, di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1))
    A = sum(shift(X.abs(), di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1))
    y = S * r
    tol = (t + 1) * U32 * r * A + 2 * U32 * y.abs()
    return {"y": (y, tol), "y_bf16": (y, tol + UBF * y.abs()), "S": S, "t": t}


def avgpool_int_pin(x, count_pad):
    """``int`` family: the tap sum S is an exact small integer in any order, so an fp32 y is fl(S fl(1 / t))
    BITWISE (t = 9 with count_pad)."""
    f = avgpool_fwd(x, count_pad)
    t = torch.full_like(f["t"], 9.0) if count_pad else f["t"]
    return f["S"].float() * (torch.ones(1) / t.float())


def avgpool_bwd(dy, prev, count_pad):
    """(ref, tol) of dx = prev + sum over the windows q containing the pixel of dy[q] / count(q)."""
    DY, P = dy.double(), prev.double()
    B, H, W, C = DY.shape
    t = taps_in(H, W).view(1, H, W, 1)
    r = torch.full_like(t, 1 / 9) if count_pad else 1 / t
    term = DY * r
    s = sum(shift(term, di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1))
    a = sum(shift(term.abs(), di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1))
    ref = P + s
    return ref, (t + 3) * U32 * a + U32 * (P.abs() + ref.abs())


def _tap(k):
    return k // 3 - 1, k % 3 - 1


def dwconv(x, w9):
    """(z, sum|w x|) float64: z[p] = sum_k w9[k] x[p + tap k], w9 [9, C] = [3][3][C]."""
    X, Wt = x.double(), w9.double()
    z = sum(Wt[k] * shift(X, *_tap(k)) for k in range(9))
    a = sum(Wt[k].abs() * shift(X.abs(), *_tap(k)) for k in range(9))
    return z, a


def dwconv_bn_forward(x, w9, gamma, beta, eps=EPS, momentum=MOMENTUM, run_mean=None, run_var=None, training=True,
                      chain=None):
    """{z, mean, rstd, y, y_bf16, run_mean, run_var: (ref, tol)}, rho [C], and z_in / mean_in / rstd_in: what
    the backward is fed (rounded to fp32).  ``chain``: the m of the sums (default n).  Raises ValueError when
    a channel's rho exceeds 2^-6."""
    eps, mom = f32(eps), f32(momentum)
    g, b = gamma.double(), beta.double()
    z, a = dwconv(x, w9)
    B, H, W, C = z.shape
    n = B * H * W
    m = n if chain is None else chain
    tol_z = 10 * U32 * a
    dims = (0, 1, 2)
    if training:
        mu = z.mean(dims)
        var = ((z - mu) ** 2).mean(dims)
        e_s = (m - 1) * U32 * z.abs().mean(dims)
        e_mu = e_s + tol_z.mean(dims)
        tol_mean = e_mu + U32 * mu.abs()
        t2 = (tol_z ** 2).mean(dims)
        e_var = (m * U32 * (z * z).mean(dims) + 2 * (var * t2).sqrt() + t2 + 2 * mu.abs() * e_s + e_s ** 2
                 + 2 * U32 * mu * mu)
        d = e_var / (var + eps)
        rho = d * (1 + d) / 2 + 4 * U32
        if (rho > RHO_MAX).any():
            raise ValueError(f"dw_bn reference: ill-conditioned channel, rho = {rho.max().item():.3g} > 2^-6")
    else:
        mu, var = run_mean.double(), run_var.double()
        tol_mean, e_var = torch.zeros_like(mu), torch.zeros_like(mu)
        rho = torch.full_like(mu, 4 * U32)
    rs = (var + eps) ** -0.5
    zh = (z - mu) * rs
    t_zh = rs * (tol_z + tol_mean + U32 * (z.abs() + mu.abs())) + zh.abs() * (rho + 2 * U32)
    y = zh * g + b
    tol = g.abs() * t_zh + 2 * U32 * (y.abs() + b.abs())
    out = {"z": (z, tol_z), "mean": (mu, tol_mean), "rstd": (rs, rs * rho), "y": (y, tol),
           "y_bf16": (y, tol + UBF * y.abs()), "rho": rho, "var": var,
           # ramp: z is a multiple of 2^-8; while m |z| 2^8 < 2^24 every fp32 partial sum of the chain is exact,
           # the fp64 fold too, and mean is the correctly rounded sum / n (the same fp64 division) BITWISE
           "mean_exact": (z.sum(dims) / n).float() if training else None,
           "chain_exact": bool(((z * 256) == (z * 256).round()).all() and m * z.abs().max() * 256 < 2 ** 24),
           "z_in": z.float(), "mean_in": mu.float(), "rstd_in": rs.float()}
    if training:
        omm = float(np.float32(1.0) - np.float32(mom))
        var_u = var * n / (n - 1) if n > 1 else var
        t_vu = (e_var * n / (n - 1) if n > 1 else e_var) + U32 * var_u
        for key, old, stat, t_stat in (("run_mean", run_mean, mu, tol_mean), ("run_var", run_var, var_u, t_vu)):
            if old is not None:
                p, q = mom * old.double(), omm * stat
                out[key] = (p + q, abs(omm) * t_stat + 2 * U32 * (p.abs() + q.abs()))
    return out


def dwconv_bn_backward(dy, x, w9, gamma, z, mean, rstd, prev, chain_px=None, chain_rw=None):
    """{dx, dw9, dgamma, dbeta: (ref, tol)} from the GIVEN fp32 z / mean / rstd; prev: what the four held."""
    DY, X, Wt, g = dy.double(), x.double(), w9.double(), gamma.double()
    Z, mu, rs = z.double(), mean.double(), rstd.double()
    B, H, W, C = Z.shape
    n = B * H * W
    mp = n if chain_px is None else chain_px
    mr = n if chain_rw is None else chain_rw
    dims = (0, 1, 2)
    P = {k: v.double() for k, v in prev.items()}
    zh = (Z - mu) * rs
    t_zh = U32 * (Z.abs() + mu.abs()) * rs + 2 * U32 * zh.abs()

    def acc(key, terms, t):
        ref = P[key] + terms
        return ref, t + U32 * (P[key].abs() + ref.abs())

    out = {"dbeta": acc("dbeta", DY.sum(dims), (mp + 1) * U32 * DY.abs().sum(dims)),
           "dgamma": acc("dgamma", (DY * zh).sum(dims),
                         (mp + 3) * U32 * (DY * zh).abs().sum(dims) + (DY.abs() * t_zh).sum(dims))}
    k1, k2 = DY.mean(dims), (DY * zh).mean(dims)
    e1 = (mp + 1) * U32 * DY.abs().mean(dims) + U32 * k1.abs()
    e2 = (mp + 3) * U32 * (DY * zh).abs().mean(dims) + (DY.abs() * t_zh).mean(dims) + U32 * k2.abs()
    t_in = e1 + zh.abs() * e2 + t_zh * k2.abs() + 4 * U32 * (DY.abs() + k1.abs() + (zh * k2).abs())
    dz = g * rs * (DY - k1 - zh * k2)
    tol_dz = (g * rs).abs() * t_in + 3 * U32 * dz.abs()
    # dx[p] = sum_k w[k] dz[p - tap k]
    s = sum(Wt[k] * shift(dz, -_tap(k)[0], -_tap(k)[1]) for k in range(9))
    sa = sum(Wt[k].abs() * shift(dz.abs(), -_tap(k)[0], -_tap(k)[1]) for k in range(9))
    st = sum(Wt[k].abs() * shift(tol_dz, -_tap(k)[0], -_tap(k)[1]) for k in range(9))
    out["dx"] = acc("dx", s, st + 10 * U32 * sa)
    xs = [shift(X, *_tap(k)) for k in range(9)]
    dw = torch.stack([(dz * xs[k]).sum(dims) for k in range(9)])
    dwa = torch.stack([(dz * xs[k]).abs().sum(dims) for k in range(9)])
    dwt = torch.stack([(tol_dz * xs[k].abs()).sum(dims) for k in range(9)])
    out["dw9"] = acc("dw9", dw, (mr + 3) * U32 * dwa + dwt)
    out["dz"] = (dz, tol_dz)
    return out


# --------------------------------------------------------------------------- row layout
def rows(t, img, off, total=None, fill=NAN):
    """Logical [B, H, W, C] -> token rows [total, C]: image b pixel p at row b img + off + p, every other
    row ``fill`` (what a guard holds)."""
    B, H, W, C = t.shape
    total = B * img if total is None else total
    out = torch.full((total, C), fill, dtype=t.dtype)
    idx = (torch.arange(B).view(B, 1) * img + off + torch.arange(H * W).view(1, -1)).reshape(-1)
    out[idx] = t.reshape(B * H * W, C)
    return out


def worst_rows(got, ref, tol, img, off):
    """worst_ratio of a row buffer against a logical reference; every row outside the images must be NaN
    (untouched) in ``got``."""
    total = got.shape[0]
    r, t = rows(ref, img, off, total), rows(tol, img, off, total, 0.0)
    inside = ~torch.isnan(r)
    if not torch.isnan(got[~inside]).all() or got.shape != r.shape:
        return float("inf")
    return worst_ratio(got[inside], r[inside], t[inside])


# --------------------------------------------------------------------------- inputs
def _gen(seed, *shape):
    s = seed * 1000003
    for v in shape:
        s = (s * 4099 + v) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def dw_inputs(family, B, H, W, C, seed=7):
    """{x, dy [B, H, W, C], w9 [9, C], gamma, beta, run_mean, run_var [C], prev {dx, dw9, dgamma, dbeta}}."""
    assert family in FAMILIES, family
    g = _gen(seed, B, H, W, C)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
    c = torch.arange(C)
    b = torch.arange(B).view(B, 1, 1, 1)
    x, dy, w9 = rn(B, H, W, C), rn(B, H, W, C), 0.3 * rn(9, C)
    prev = {"dx": 0.5 * rn(B, H, W, C), "dw9": 0.5 * rn(9, C), "dgamma": 0.5 * rn(C), "dbeta": 0.5 * rn(C)}
    if family == "chan":
        x = x * (1 + c % 5).float() + 0.5 * (c % 7).float() + 0.25 * b.float()
        dy = dy * (1 + c % 3).float()
    elif family == "offset":
        x = x + 8.0 * (1 - 2 * (c % 2)).float()
    elif family == "ramp":
        p = torch.arange(B * H * W).view(B, H, W, 1)
        x = (((1 + c % 4) * p + c % 4) % 251).float()
        k = torch.arange(9).view(9, 1)
        w9 = torch.pow(2.0, ((k + c) % 9 - 8).float())
    elif family == "int":
        x, dy = ri(-8, 8, B, H, W, C), ri(-8, 8, B, H, W, C)
        prev = {"dx": ri(-4, 4, B, H, W, C), "dw9": ri(-4, 4, 9, C), "dgamma": ri(-4, 4, C), "dbeta": ri(-4, 4, C)}
    return dict(x=x, dy=dy, w9=w9, gamma=1 + 0.3 * rn(C), beta=0.2 * rn(C), run_mean=0.1 * rn(C),
                run_var=0.5 + torch.rand(C, generator=g), prev=prev)


def conv_inputs(family, g: Geo, Kp, seed=9):
    """{x, prev [B, H, W, C], dp [B Ho Wo, Kp] (columns K.. hold NaN: the adjoint never reads them)}."""
    gen = _gen(seed, g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, g.pt, g.pl, Kp)
    K, R = g.kh * g.kw * g.C, g.B * g.Ho * g.Wo
    if family == "int":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()  # noqa: E731
        x, prev, dp = ri(-8, 8, g.B, g.H, g.W, g.C), ri(-4, 4, g.B, g.H, g.W, g.C), ri(-8, 8, R, Kp)
    else:
        assert family == "randn", family
        x = torch.randn(g.B, g.H, g.W, g.C, generator=gen)
        prev, dp = 0.5 * torch.randn(g.B, g.H, g.W, g.C, generator=gen), torch.randn(R, Kp, generator=gen)
    dp[:, K:] = NAN
    return dict(x=x, prev=prev, dp=dp)


# --------------------------------------------------------------------------- CPU emulation
CONV_MUTANTS = ("padceil", "ij", "nopadcols", "trunc", "nooh", "nomod", "overwrite", "imgstride", "nocls",
                "droplast", "firsttwice")
POOL_MUTANTS = ("hwswap", "nocountpad", "trunc", "imgstride", "nocls", "droplast", "firsttwice")
FWD_MUTANTS = ("ij", "noleft", "noright", "nobottom", "biasedrv", "besselrstd", "fp32var", "neighmean", "trunc",
               "droplast", "firsttwice", "imgstride", "nocls")
BWD_MUTANTS = ("mirror", "lookahead", "k2non", "dxover", "dw9over", "dgammaover", "droplast", "firsttwice",
               "neighmean")


def _store(v, bf16, mut):
    if not bf16:
        return v
    return (bf16_trunc(v) if mut == "trunc" else bf16_rne(v)).float()


def _walk(new, old, mut, accumulate=False):
    """A flat grid-stride kernel of at most CVT_BLOCKS x 256 threads over the leading dimension's work
    items (one per 4 channels): 'droplast' leaves the items of the last, partial trip as they were,
    'firsttwice' visits the items of the first trip twice (visible where the kernel accumulates)."""
    flat_n, flat_o = new.reshape(-1, 4), old.reshape(-1, 4)
    cap, total = CVT_BLOCKS * 256, flat_n.shape[0]
    if total <= cap or mut not in ("droplast", "firsttwice"):
        return new
    out = flat_n.clone()
    if mut == "droplast":
        out[total - total % cap:] = flat_o[total - total % cap:]
    elif accumulate:
        out[:cap] = flat_n[:cap] + (flat_n[:cap] - flat_o[:cap])
    return out.view(new.shape)


def emulate_im2col(x, g, Kp, bf16=False, mut=None, vec=4):
    """The patch rows in fp32 (bf16 values as fp32), NaN where nothing was written.  Mutants: 'ij' (the tap
    index splits as (j, i)), 'nopadcols' (columns K.. unwritten), 'trunc', 'droplast'."""
    K = g.kh * g.kw * g.C
    Hp, Wp = _padded_hw(g)
    xp = torch.zeros(g.B, Hp, Wp, g.C)
    xp[:, g.pt:g.pt + g.H, g.pl:g.pl + g.W] = x.float()
    order = [(i, j) for i in range(g.kh) for j in range(g.kw)]
    if mut == "ij":
        order = [(t % g.kh, t // g.kh) for t in range(g.kh * g.kw)]
    out = torch.full((g.B * g.Ho * g.Wo, Kp), NAN if mut == "nopadcols" else 0.0)
    out[:, :K] = torch.stack([xp[_win(g, i, j)] for i, j in order], 3).reshape(-1, K)
    out = _store(out, bf16, mut)
    if mut == "droplast" and out.numel() // vec > CVT_BLOCKS * 256:
        flat = out.view(-1, vec)
        flat[flat.shape[0] - flat.shape[0] % (CVT_BLOCKS * 256):] = NAN
    return out


def emulate_col2im(dp, g, prev=None, mut=None):
    """conv_col2im_kernel in fp32: the gather over (i, j) in order.  Mutants: 'nooh' (no oh < Ho / ow < Wo
    bound: the row index runs into the next image's, NaN past the end), 'nomod' (no th % s test), 'overwrite'
    (accumulate ignored), 'droplast', 'firsttwice'."""
    B, H, W, C, Ho, Wo, s = g.B, g.H, g.W, g.C, g.Ho, g.Wo, g.s
    K, R = g.kh * g.kw * C, g.B * g.Ho * g.Wo
    ext = torch.cat([dp[:, :K].float(), torch.full((Ho * Wo + Wo + 1, K), NAN)])
    b = torch.arange(B).view(B, 1, 1)
    acc = torch.zeros(B, H, W, C)
    for i in range(g.kh):
        th = torch.arange(H) + g.pt - i
        okh = (th >= 0) & ((th % s == 0) | (mut == "nomod")) & ((th // s < Ho) | (mut == "nooh"))
        for j in range(g.kw):
            tw = torch.arange(W) + g.pl - j
            okw = (tw >= 0) & ((tw % s == 0) | (mut == "nomod")) & ((tw // s < Wo) | (mut == "nooh"))
            ok = okh.view(1, H, 1) & okw.view(1, 1, W)
            r = ((b * Ho + (th // s).view(1, H, 1)) * Wo + (tw // s).view(1, 1, W)).clamp(0, ext.shape[0] - 1)
            v = ext[r.reshape(-1), (i * g.kw + j) * C:(i * g.kw + j + 1) * C].view(B, H, W, C)
            acc = acc + torch.where(ok.expand(B, H, W).unsqueeze(-1), v, torch.zeros_like(v))
    old = torch.zeros(B, H, W, C) if prev is None else prev.float()
    new = acc if prev is None or mut == "overwrite" else old + acc
    if prev is None:      # an overwriting kernel: a dropped item keeps the guard it held
        return _walk(new, torch.full_like(new, NAN), mut)
    return _walk(new, old, mut, accumulate=True)


def _count(H, W, mut):
    def inb(n):
        i = torch.arange(n)
        return 3.0 - (i == 0).float() - (i == n - 1).float()
    ch, cw = inb(H), inb(W)
    if mut == "hwswap":
        i, j = torch.arange(H), torch.arange(W)
        ch = 3.0 - (i == 0).float() - (i == W - 1).float()
        cw = 3.0 - (j == 0).float() - (j == H - 1).float()
    return (ch.view(H, 1) * cw.view(1, W)).view(1, H, W, 1)


def _recip(H, W, count_pad, mut):
    if count_pad and mut != "nocountpad":
        return torch.full((1, H, W, 1), 1.0) / 9.0
    return 1.0 / _count(H, W, mut)


def emulate_avgpool_fwd(x, count_pad, bf16=False, mut=None):
    """avgpool3_fwd_kernel in fp32: the in-image taps in (i, j) order times the fp32 reciprocal.  Mutants:
    'hwswap' (H and W swapped in the count), 'nocountpad', 'trunc', 'droplast'."""
    x = x.float()
    B, H, W, C = x.shape
    acc = torch.zeros_like(x)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            acc = acc + shift(x, di, dj)
    y = _store(acc * _recip(H, W, count_pad, mut), bf16, mut)
    return _walk(y, torch.full_like(y, NAN), mut)


def emulate_avgpool_bwd(dy, prev, count_pad, mut=None):
    dy, prev = dy.float(), prev.float()
    B, H, W, C = dy.shape
    term = dy * _recip(H, W, count_pad, mut)
    acc = torch.zeros_like(dy)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            acc = acc + shift(term, di, dj)
    return _walk(prev + acc, prev, mut, accumulate=True)


def _stencil(x, w9, flip=False, swap=False, relax=None):
    """sum over (i, j) in order of w[i][j] x[p + (i - 1, j - 1)] (flip: p - (i - 1, j - 1)) in fp32."""
    acc = torch.zeros_like(x)
    for i in range(3):
        for j in range(3):
            k = j * 3 + i if swap else i * 3 + j
            di, dj = (1 - i, 1 - j) if flip else (i - 1, j - 1)
            acc = acc + w9[k] * shift(x, di, dj, relax)
    return acc


def _partials(terms, T, lanes, mut=None, all32=False):
    """Per-channel sums of terms [R, ..., C] the way the statistics kernels form them: work item r belongs
    to thread r % T (T = G x lanes threads per channel group, thread = block * lanes + lane); a thread's
    own sum and its block's ``lanes`` partials in fp32, the G block partials in fp64 (all32: fp32 too).
    Mutants: 'droplast' (the last trip of the walk left out), 'firsttwice' (the first trip twice)."""
    R, C = terms.shape[0], terms.shape[-1]
    t = terms.float().reshape(R, -1, C)
    trips = cdiv(R, T)
    t = torch.cat([t, torch.zeros(trips * T - R, t.shape[1], C)]).view(trips, T, -1, C)
    if mut == "droplast" and trips > 1:
        t = t[:-1]
    if mut == "firsttwice" and trips > 1:
        t = torch.cat([t[:1], t])
    per_thread = t.sum((0, 2))                              # [T, C] fp32
    per_block = per_thread.view(T // lanes, lanes, C).sum(1)
    return per_block.sum(0).double() if all32 else per_block.double().sum(0)


def emulate_dw_fwd(x, w9, gamma, beta, eps=EPS, momentum=MOMENTUM, run_mean=None, run_var=None, training=True,
                   bf16=False, mut=None):
    """The three forward kernels: z by the sliding window's (i, j) order in fp32, fp32 partials of sum z and
    sum z^2 per thread and block, the fp64 finish with the one-pass variance, (z - mean) rstd gamma + beta,
    a round-to-nearest bf16 store.  Returns {z, mean, rstd, y, run_mean, run_var}.  Mutants: FWD_MUTANTS."""
    x, w9, g, b = x.float(), w9.float(), gamma.float(), beta.float()
    B, H, W, C = x.shape
    n = B * H * W
    eps32, m32 = np.float32(eps), np.float32(momentum)
    relax = {"noleft": "left", "noright": "right", "nobottom": "bottom"}.get(mut)
    z = _stencil(x, w9, swap=mut == "ij", relax=relax)
    out = {"z": z}
    if training:
        G, lanes, _ = rows_grid(B, H, W, C)
        zr = z.view(B * H, W, C)
        s1 = _partials(zr, G * lanes, lanes, mut)
        s2 = _partials(zr * zr, G * lanes, lanes, mut)
        if mut == "fp32var":        # one fp32 running sum over the channel's n pixels, and an fp32 finish
            s1 = z.reshape(n, C).cumsum(0)[-1].double()
            s2 = (z * z).reshape(n, C).cumsum(0)[-1].double()
            mu = (s1.float() / np.float32(n)).double()
            var = (s2.float() / np.float32(n) - mu.float() * mu.float()).double()
        else:
            mu = s1 / n
            var = s2 / n - mu * mu
        var = var.clamp_min(0.0)
        var_u = var * n / (n - 1) if n > 1 else var
        mean = mu.float()
        rstd = (1.0 / torch.sqrt((var_u if mut == "besselrstd" else var) + float(eps32))).float()
        omm = np.float32(1.0) - m32
        if run_mean is not None:
            out["run_mean"] = float(m32) * run_mean.float() + float(omm) * mean
        if run_var is not None:
            out["run_var"] = float(m32) * run_var.float() + float(omm) * (var if mut == "biasedrv" else var_u).float()
    else:
        mean = run_mean.float().clone()
        rstd = (1.0 / torch.sqrt(run_var.double() + float(eps32))).float()
    out["mean"], out["rstd"] = mean, rstd
    ma, ra = (mean.roll(-4), rstd.roll(-4)) if mut == "neighmean" else (mean, rstd)
    out["y"] = _store((z - ma) * ra * g + b, bf16, mut)
    return out


def emulate_dw_bwd(dy, x, w9, gamma, z, mean, rstd, prev, mut=None):
    """The five backward kernels in fp32 with their fp32 partials and fp64 folds.  Returns {dx, dw9, dgamma,
    dbeta}.  Mutants: BWD_MUTANTS."""
    dy, x, w9, g, z = dy.float(), x.float(), w9.float(), gamma.float(), z.float()
    mu, rs = mean.float(), rstd.float()
    B, H, W, C = z.shape
    n = B * H * W
    lanes = 256 // (C // 4)
    G = dw_blocks(n, C)
    if mut == "neighmean":
        mu = mu.roll(-4)
    zh = (z - mu) * rs
    wm = mut if mut in ("droplast", "firsttwice") else None
    s1 = _partials(dy.reshape(n, C), G * lanes, lanes, wm)
    s2 = _partials((dy * zh).reshape(n, C), G * lanes, lanes, wm)
    out = {"dbeta": prev["dbeta"].float() + s1.float(),
           "dgamma": s2.float() if mut == "dgammaover" else prev["dgamma"].float() + s2.float()}
    k1, k2 = (s1 / n).float(), (s2 if mut == "k2non" else s2 / n).float()
    dz = (g * rs) * (dy - k1 - zh * k2)
    Gw, _, _ = rows_grid(B, H, W, C)
    Gw = min(Gw, G)
    dw = torch.stack([_partials((dz * shift(x, *_tap(k))).view(B * H, W, C), Gw * lanes, lanes, wm)
                      for k in range(9)]).float()
    out["dw9"] = dw if mut == "dw9over" else prev["dw9"].float() + dw
    acc = _stencil(dz, w9, flip=mut != "mirror", relax="right" if mut == "lookahead" else None)
    out["dx"] = acc if mut == "dxover" else prev["dx"].float() + acc
    return out


# --------------------------------------------------------------------------- the listed cases
HW = ((1, 1), (1, 2), (2, 1), (1, 5), (5, 1), (2, 2), (3, 3), (3, 5), (5, 3), (7, 7), (8, 9), (16, 5))
BS = (1, 2, 3)
FAMILY_CS = (4, 64, 256, 1024)
# (B, H, W, C, rows per thread at the least); the last adds a ragged tail at eight rows
WALKS = ((8, 64, 3, 64, 2), (16, 33, 2, 256, 4), (4, 100, 1, 1024, 8), (4, 101, 1, 1024, 8))
# past the 4096 x 256 work items of every flat and row-walking grid (with a remainder), and past dw_blocks' 1024
CAPS = ((4, 1025, 1, 1024), (3, 53, 53, 1024))
SWEEP = tuple((h, w) for h in range(1, 10) for w in range(1, 10))


def dw_matrix(C):
    """[(family, B, H, W, C)] of the C x (H, W) x B matrix: ``chan`` everywhere, every family at FAMILY_CS."""
    fams = FAMILIES if C in FAMILY_CS else ("chan",)
    return [(f, B, H, W, C) for f in fams for H, W in HW for B in BS if f != "offset" or offset_ok(B * H * W)]


def conv_cases():
    """[(name, Geo, Kp)]: kh, kw in {1, 2, 3, 4, 7} with kh != kw, s in {1..4} with k < s, H != W, H or W below
    k, TF 'same' with an odd padding total, explicit padding whose last window hangs over the bottom and the
    right, Kp in {K, K up to 64, K + 1}, C in {1, 3, 4, 6, 64}."""
    out = []

    def same(name, B, H, W, C, kh, kw, s, kp):
        g = same_geo(B, H, W, C, kh, kw, s)
        K = kh * kw * C
        out.append((name, g, {"K": K, "64": cdiv(K, 64) * 64, "+1": K + 1}[kp]))

    same("k7s4", 2, 13, 9, 4, 7, 7, 4, "64")
    same("k3s2-odd-total", 3, 8, 6, 64, 3, 3, 2, "K")          # total 1: pad_before 0, pad_after 1
    same("k3s1", 2, 5, 7, 4, 3, 3, 1, "64")
    same("k1s1", 2, 3, 4, 64, 1, 1, 1, "K")
    same("k2s3-unread", 2, 7, 8, 4, 2, 2, 3, "64")             # k < s: pixels no window reads
    same("k1s4-unread", 1, 9, 6, 4, 1, 1, 4, "K")
    same("k3x7s2", 2, 6, 11, 4, 3, 7, 2, "64")
    same("k4x2s3", 2, 10, 5, 4, 4, 2, 3, "K")
    same("k7-H-below-k", 2, 3, 5, 4, 7, 7, 4, "64")
    same("k4s4", 1, 8, 12, 64, 4, 4, 4, "K")
    same("C1-scalar", 2, 9, 7, 1, 7, 7, 4, "64")
    same("C3-scalar", 2, 5, 6, 3, 3, 3, 2, "+1")
    same("C6-scalar", 1, 4, 5, 6, 2, 3, 1, "64")
    same("C4-Kp+1-scalar", 2, 5, 4, 4, 3, 3, 2, "+1")
    # explicit geometry (torch's symmetric padding): (H + 2p - k) // s + 1 windows, the last over the edge
    out.append(("k3s2p1", Geo(2, 8, 6, 64, 3, 3, 2, 1, 1, 4, 3), 9 * 64))
    out.append(("k7s4p2", Geo(2, 11, 14, 4, 7, 7, 4, 2, 2, 3, 3), 256))
    out.append(("k3s2-hang", Geo(1, 4, 4, 4, 3, 3, 2, 0, 0, 2, 2), 64))      # rows 2..4, columns 2..4: one over
    out.append(("k2s2p1-hang", Geo(2, 5, 3, 4, 2, 2, 2, 1, 1, 3, 2), 16))
    assert all(geo_ok(g) for _, g, _ in out)
    return out


CONV_CAPS = (("im2col-cap", Geo(2, 65, 65, 64, 3, 3, 1, 1, 1, 65, 65), 576),
             ("col2im-cap", Geo(2, 65, 65, 512, 1, 1, 1, 0, 0, 65, 65), 512))
