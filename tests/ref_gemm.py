"""Float64 reference of the GEMM entry points (include/vitmi.h vitmi_gemm and the vitmi_linear_*
calls built on it) with a per-element error bound DERIVED from the arithmetic, plus guarded
buffers.  Plain torch / numpy on the CPU, no GPU.  TEST INFRASTRUCTURE ONLY.

``reference`` takes the operands as the kernel sees them (already rounded to their storage type, in
their stored layout) and returns, for every output the epilogue writes, ``(ref, tol)`` in float64:
a got value conforms iff |got - ref| <= tol for every element.  With S = |A| |B| + |bias| (float64),
u32 = 2^-24, ubf = 2^-8 and K the reduction length,

  t_acc = 2 (K + 1) u32 S                     any summation order of fp32 partial sums; the factor 2
                                              because MFMA's internal block sum is not documented
                                              as one IEEE rounding per product
  STORE fp32        t_acc + u32 |ref|
  STORE bf16        1.01 t_acc + ubf |ref|     (ubf |ref| >= half a bf16 ulp: a truncating store fails)
  RESIDUAL family   f t_acc + 4 u32 (|res| + |branch|), f the dropout x drop-path factor; an element
                    whose factor is 0 is the residual bit for bit (tol 0)
  BIAS_GELU C, aux  1.13 f t_acc + t_fn + (bf16 ? ubf : u32) |ref|, 1.13 >= max |gelu'| (and 0.8 >=
                    max |gelu''|), t_fn = T_FN_ULPS u32 max(|ref|, 1) for erff / exp
  DGELU             |aux| t_acc + (bf16 ? ubf : u32) |ref|
  ACCUM             t_acc + u32 (|prev| + |ref|)
  SPLIT_X3          C columns [N, 2N) bitwise equal to [0, N); hi + lo within the GELU bound with
                    ubf^2 in place of ubf
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import vit_ref

import ref_droppath

U32 = 2.0 ** -24
UBF = 2.0 ** -8
T_FN_ULPS = 16.0          # t_fn = T_FN_ULPS * u32 * max(|ref|, 1): not fitted to any kernel
GELU_LIP = 1.13           # >= max |gelu'| (1.129 at u = sqrt 2) and >= max |gelu''| (0.798 at 0)
BF = torch.bfloat16
E4 = torch.float8_e4m3fn

LAYOUTS = {"KK": (True, True), "KN": (True, False), "NN": (False, False), "NK": (False, True)}


# --------------------------------------------------------------------------- float64 pieces
def gelu(u: torch.Tensor) -> torch.Tensor:
    """Exact-erf GELU in the dtype of u (float64 for the reference)."""
    return 0.5 * u * (1 + torch.erf(u / 2 ** 0.5))


def gelu_grad(u: torch.Tensor) -> torch.Tensor:
    """d/du of the exact-erf GELU: Phi(u) + u phi(u) (tests/test_gpu_ops.py gelu_grad)."""
    return 0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * math.pi) ** 0.5


def logical(a: torch.Tensor, b: torch.Tensor, layout: str):
    """(A [M, K], B [K, N]) in float64 from the stored operands: A is stored [M][K] when k-major,
    [K][M] otherwise; B is stored [N][K] when k-major, [K][N] otherwise."""
    ak, bk = LAYOUTS[layout]
    A = a.double() if ak else a.double().t()
    B = b.double().t() if bk else b.double()
    assert A.shape[1] == B.shape[0], (A.shape, B.shape)
    return A, B


def drop_factor(seed: int, site: int, rate: float, M: int, N: int) -> torch.Tensor:
    """float64 [M, N]: 1/(1-p) where element (row, col) of the dropout site is kept, else 0."""
    thresh, scale = vit_ref.dropout_params(rate)
    keep = vit_ref.dropout_hash(seed, site, np.arange(M), np.arange(N)) >= thresh
    return torch.from_numpy(keep.astype(np.float64)) * float(np.float32(scale))


def path_factor(seed: int, site: int, rate: float, M: int, rows_per_sample: int) -> torch.Tensor:
    """float64 [M, 1]: the drop-path factor of the sample that owns each row."""
    _, scale = vit_ref.dropout_params(rate)
    keep = ref_droppath.keep_mask(seed, site, M // rows_per_sample, rate)
    f = torch.from_numpy(keep.astype(np.float64)) * float(np.float32(scale))
    return f.repeat_interleave(rows_per_sample).view(M, 1)


def reference(a, b, layout, base, *, bias=None, aux=None, residual=None, prev=None, out_bf16=False,
              aux_bf16=None, drop=None, path=None, split_x3=False, k_acc=None):
    """The outputs of one GEMM call as {name: (ref, tol)}, float64.

    a, b       the stored operands (see ``logical``); any float dtype, taken as exact
    base       "store" | "gelu" | "residual" | "dgelu" | "accum"
    bias       fp32 [N] or None;  aux: gelu' [M, N] read by "dgelu";  residual: fp32 [M, N];
    prev       what C holds before an "accum"
    out_bf16   C is stored as bf16;  aux_bf16: the gelu' written by "gelu" is bf16 (default: the
               operands are)
    drop       (seed, site, rate) element dropout;  path: (seed, site, rate, rows_per_sample)
    split_x3   "gelu" with C as [hi | hi | lo]: adds "hi+lo" (C itself is the bound of hi)
    k_acc      reduction length of the accumulation when it is not A.shape[1]
    """
    A, B = logical(a, b, layout)
    M, K = A.shape
    N = B.shape[1]
    if k_acc is None:
        k_acc = K
    acc = A @ B
    S = A.abs() @ B.abs()
    bv = torch.zeros(N, dtype=torch.float64) if bias is None else bias.double()
    S = S + bv.abs()
    t_acc = 2.0 * (k_acc + 1) * U32 * S
    u = acc + bv
    f = torch.ones(M, N, dtype=torch.float64)
    if drop is not None:
        f = f * drop_factor(drop[0], drop[1], drop[2], M, N)
    if path is not None:
        f = f * path_factor(path[0], path[1], path[2], M, path[3])
    uo = UBF if out_bf16 else U32
    if aux_bf16 is None:
        aux_bf16 = a.dtype == BF
    out = {}
    if base == "store":
        ref = u
        out["C"] = (ref, (1.01 * t_acc + UBF * ref.abs()) if out_bf16 else (t_acc + U32 * ref.abs()))
    elif base == "residual":
        r = residual.double()
        branch = f * u
        tol = f * t_acc + 4 * U32 * (r.abs() + branch.abs())
        out["C"] = (r + branch, torch.where(f == 0, torch.zeros_like(tol), tol))
    elif base == "gelu":
        for name, fn, ub in (("C", gelu, uo), ("aux", gelu_grad, UBF if aux_bf16 else U32)):
            ref = fn(u) * f
            t_fn = T_FN_ULPS * U32 * ref.abs().clamp_min(1.0)
            out[name] = (ref, GELU_LIP * f * t_acc + t_fn + ub * ref.abs())
            if name == "C" and split_x3:
                out["hi+lo"] = (ref, GELU_LIP * f * t_acc + t_fn + UBF * UBF * ref.abs())
    elif base == "dgelu":
        g = aux.double()
        ref = acc * g
        out["C"] = (ref, g.abs() * t_acc + uo * ref.abs())
    elif base == "accum":
        p = prev.double()
        ref = p + acc
        out["C"] = (ref, t_acc + U32 * (p.abs() + ref.abs()))
    else:
        raise ValueError(base)
    return out


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """max over every element of |got - ref| / tol; an element with tol == 0 counts 0 when it is
    exact and inf otherwise, a NaN anywhere gives inf."""
    err = (got.double() - ref).abs()
    if torch.isnan(err).any():
        return float("inf")
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    return ratio.max().item() if ratio.numel() else 0.0


# --------------------------------------------------------------------------- VITMI_BF16F8 rows
def _e4m3(x: torch.Tensor) -> torch.Tensor:
    return x.clamp(-448.0, 448.0).to(E4)


def f8_rows(x: torch.Tensor, weight: bool, wform: bool = False):
    """VITMI_BF16F8 (wform: VITMI_BF16F8W) rows of fp32 x [rows, K] as (stored, decoded): ``stored``
    is the bf16-unit tensor [rows, 2K] ([rows, 1.5K]) the GEMM reads -- [hi | e4m3 part], the e4m3
    part in 64-k blocks [hi8 | lo8] for an A operand and [lo8 | hi8] for a weight (wform: one byte
    per k, hi8 for A and lo8 for a weight) -- and ``decoded`` the float64 [rows, 2K] ([rows, 1.5K])
    whose plain product A_dec B_dec^T is what the GEMM computes (the 2^-9 scale of every lo8 folded
    in), as tests/test_gpu_f8.py builds it."""
    x = x.float()
    rows, K = x.shape
    hi = x.to(BF)
    hi8 = _e4m3(hi.float())
    lo8 = _e4m3((x - hi.float()) * 512.0)
    hb = hi.view(torch.uint8).reshape(rows, 2 * K)
    if wform:
        assert K % 128 == 0
        part = (lo8 if weight else hi8).view(torch.uint8)
        dec = torch.cat([hi.double(), (lo8.double() / 512.0) if weight else hi8.double()], 1)
    else:
        assert K % 64 == 0
        first, second = (lo8, hi8) if weight else (hi8, lo8)
        part = torch.stack([first.view(torch.uint8).reshape(rows, K // 64, 64),
                            second.view(torch.uint8).reshape(rows, K // 64, 64)], 2).reshape(rows, 2 * K)
        dec = torch.cat([hi.double(), first.double() / (512.0 if weight else 1.0),
                         second.double() / (1.0 if weight else 512.0)], 1)
    stored = torch.cat([hb, part], 1).contiguous().view(BF)
    return stored, dec


# --------------------------------------------------------------------------- guarded buffers
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
GUARD_BITS = {torch.float32: 0x4B4B4B4B, torch.bfloat16: 0x4B4B}     # finite, fixed
NAN_BITS = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0}
GUARD_ROWS = 3


class Padded:
    """A rows x cols window (row pitch ``pitch`` elements) inside a larger allocation: GUARD_ROWS
    whole guard rows before and after, guard columns [cols, pitch) in every row and ``offset``
    guard elements in front (a window whose base is not vector aligned).  ``buf`` is the flat
    allocation, ``view`` the strided window into it."""

    def __init__(self, rows, cols, pitch, dtype, fill, offset=0, _buf=None):
        assert pitch >= cols and rows >= 0
        self.rows, self.cols, self.pitch, self.dtype, self.offset = rows, cols, pitch, dtype, offset
        self.bits = {"guard": GUARD_BITS, "nan": NAN_BITS}[fill][dtype] if isinstance(fill, str) else int(fill)
        self.fill = fill
        n = offset + (rows + 2 * GUARD_ROWS) * pitch
        if _buf is None:
            _buf = torch.full((n,), self._signed(), dtype=_INT[dtype]).view(dtype)
        self.buf = _buf
        self.start = offset + GUARD_ROWS * pitch
        self.view = self.buf.as_strided((rows, cols), (pitch, 1), self.start)

    def _signed(self):
        w = 16 if self.dtype == BF else 32
        return self.bits - (1 << w) if self.bits >= 1 << (w - 1) else self.bits

    def set(self, values):
        self.view.copy_(values.to(self.dtype))
        return self

    def to(self, device):
        return Padded(self.rows, self.cols, self.pitch, self.dtype, self.bits, self.offset, self.buf.to(device))

    def clone(self):
        return Padded(self.rows, self.cols, self.pitch, self.dtype, self.bits, self.offset, self.buf.clone())

    def ptr(self):
        return self.buf.data_ptr() + self.start * self.buf.element_size()


def padded(rows, cols, pitch, dtype, fill, offset=0) -> Padded:
    return Padded(rows, cols, pitch, dtype, fill, offset)


def guards_intact(p: Padded) -> bool:
    """Every element of the allocation outside the window still holds the fill bit pattern."""
    ints = p.buf.view(_INT[p.dtype]).clone()
    ints.as_strided((p.rows, p.cols), (p.pitch, 1), p.start).fill_(p._signed())
    return bool((ints == p._signed()).all().item())


# --------------------------------------------------------------------------- CPU emulation
def bf16_rne(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(BF)


def bf16_trunc(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (the mutant a half-ulp bound must reject)."""
    bits = x.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(BF)


def emulate(a, b, layout, base, *, bias=None, aux=None, residual=None, prev=None, out_bf16=False,
            drop=None, path=None, store=bf16_rne):
    """The kernels' arithmetic on the CPU: fp32 matmul of the rounded operands, the epilogue in
    fp32, the bf16 outputs through ``store``.  Returns {name: tensor}."""
    ak, bk = LAYOUTS[layout]
    A = a.float() if ak else a.float().t()
    B = b.float().t() if bk else b.float()
    acc = A @ B
    M, N = acc.shape
    u = acc + bias.float() if bias is not None else acc
    f = torch.ones(M, N)
    if drop is not None:
        f = f * drop_factor(drop[0], drop[1], drop[2], M, N).float()
    if path is not None:
        f = f * path_factor(path[0], path[1], path[2], M, path[3]).float()
    fin = (lambda t: store(t)) if out_bf16 else (lambda t: t)
    if base == "store":
        return {"C": fin(u)}
    if base == "residual":
        return {"C": residual.float() + u * f}
    if base == "gelu":
        g = gelu_grad(u) * f
        return {"C": fin(gelu(u) * f), "aux": store(g) if a.dtype == BF else g}
    if base == "dgelu":
        return {"C": fin(acc * aux.float())}
    if base == "accum":
        return {"C": prev.float() + acc}
    raise ValueError(base)
