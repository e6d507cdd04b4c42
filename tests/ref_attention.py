"""Float64 reference of the attention entry points (include/vitmi.h vitmi_attention_fwd, _fwd_x3,
_fwd_f8, _bwd, _bwd_bias) with a per-element error bound DERIVED from the arithmetic, input
families, guarded buffers and a CPU emulation of the kernels' arithmetic.  Plain torch on the CPU,
no GPU.  TEST INFRASTRUCTURE ONLY (the counterpart of tests/ref_gemm.py).

``forward`` / ``backward`` / ``reference`` take the operands as stored (bf16 or fp32 values count as
exact, ``scale`` as the float32 the API receives) and return ``{name: (ref, tol)}`` in float64, in the
API's layouts (o, dq, dk, dv [B*N, H*64]; lse [B*H, N]): a result conforms iff |got - ref| <= tol for
EVERY element.

Notation.  u32 = 2^-24, ubf = 2^-8, d = 64, T_FN_ULPS from ref_gemm; up = ubf for the bf16 kernels
(P and dS are rounded to bf16 before their MFMA: csrc/attention.hip pack8), 0 for fp32; uo = ubf or
u32, the store rounding.  Per (batch, head) pair, a = scale Q K^T, Sb = scale |Q| |K|^T.

Exponent (absolute error of the natural-log argument of every exp)
  ex_ij = 2 (d+1) u32 Sb_ij                      the QK^T sum in any order of fp32 partial sums (as
                                                 ref_gemm's t_acc; it also covers the fp32 kernels'
                                                 rounding of scale q_d / scale k_d before the sum)
        + 4 u32 (|a_ij| + max_j |a_ij|)          c2 = scale log2(e) rounded, the row maximum times
                                                 c2 rounded, the fma s c2 - m rounded
        + T_FN_ULPS u32                          v_exp_f32
  Every forward kernel is an online softmax over key tiles (64 keys in the bf16 kernels and the
  streamed fp32 one, 32 in attn_fwd_seq_f32): when the running maximum moves, the row sum and the
  output are rescaled by alpha = exp(m_old - m_new).  The same alpha multiplies numerator and
  denominator, so its error is an error of the weight of the EARLIER keys and belongs in ex.  No new
  term is needed for the sizes run here: the arguments m_old - m_new telescope to at most
  2 max|a|, whose roundings (half an ulp each) fit beside the 1.5 (|a| + max|a|) u32 that the three
  roundings named above use of the 4; and each rescale costs one exp (1 ulp, v_exp_f32 / expf) and
  one product, so a row's first keys carry 1 + 2 (tiles - 1) ulps, 15 of the T_FN_ULPS = 16 at the
  most tiles any case has (8: attn_fwd_seq_f32 at N = 256; 7 at N = 385 streamed).  A longer
  sequence needs T_FN_ULPS replaced by 1 + 2 (tiles - 1) there.

Forward.  L = logsumexp(a), P = exp(a - L), o = P V.
  tol_o   = ((up + ex) o P) |V|                  each weight: bf16 rounding and exponent error
          + 2 (N+1) u32 P |V|                    the PV sum in any order
          + ((N+2) u32 + max_j ex) |o|           the row sum l (N additions, 1 / l, the product) and
                                                 the exponent error of l
          + uo |o|                               the store
          + floor_o
  tol_lse = max_j ex + (N+2) u32 + T_FN_ULPS u32 + 2 u32 |L|
                                                 l, v_log_f32, and (m + log2 l) ln 2 rounded twice

Backward.  A function of the GIVEN o and lse, exactly as the API defines it:
  P = exp(a - lse), delta = rowsum(dO o o), dP = dO V^T, G = P o (dP - delta),
  dV = P^T dO, dK = scale G^T Q, dQ = scale G K.
  eps    = ex + 2 u32 |lse|                      lse log2(e) rounded, and inside the fma
  e_dp   = 2 (d+1) u32 (|dO| |V|^T + rowsum |dO o o|)
                                                 dP - delta is one chain of 2 d fp32 terms (the MFMA
                                                 accumulator starts at -delta)
  g      = P o ((up + eps + u32) |dP - delta| + e_dp)
                                                 dS: the product rounded (u32), then to bf16 (up)
  tol_dV = ((up + eps) o P)^T |dO| + 2 (N+1) u32 P^T |dO| + uo |dV| + floor
  tol_dK = scale (g^T |Q| + 2 (N+1) u32 |G|^T |Q|) + (uo + u32) |dK| + floor
                                                 scale is applied to the fp32 sum at the store (u32)
  tol_dQ   the same with |K|: scale (g |K| + 2 (N+1) u32 |G| |K|) + (uo + u32) |dQ| + floor

Flushed denormals.  The kernels call v_exp_f32 directly: a result below 2^-126 is flushed to 0, and
the MFMA flushes denormal operands and results.  In the forward the weights are relative to the row
maximum, so l >= 1 and a flushed weight changes P_ij by less than 2^-126; each of the N products
P_ij V_jc, and each partial sum, can lose less than 2^-126 again.  Hence
  floor_o = 4 * 2^-126 (sum_j |V_jc| + N)   (<= 2^-120 sum|V| for N <= 16 sum|V|),
and the same with |dO| for dV and with scale (|dP - delta| |Q|) resp. |K| for dK and dQ.  It matters
only where reference and bound are both next to 0.

Conditioning.  The bound is first order in ex.  ``forward`` and ``backward`` assert max ex < 2^-10 and
max |a| < 80 (exp(a - L) is a normal fp32 number only down to about a - L = -87): inputs that
break either are refused, not judged.

x3.  o3 rows are [hi | hi | lo] of the fp32 output: hi is o; hi + lo is held to tol_o with ubf^2 in
place of uo (lo = bf16(v - hi) leaves a relative 2^-9 of a value below 2^-8 |v|).  The P-rounding
term stays: the weights are bf16 in that kernel too.

Bias gradient (the bound of tests/test_gpu_attn_dispatch.py, word for word).  Every column c of dbias against the
column sums of the RETURNED g = dqkv: |dbias_c - sum_r g[r,c]| <= (2^-8 + n 2^-24) sum_r |g[r,c]|,
n = B N.  For bf16 the 2^-8 is twice the half-ulp with which each summand was rounded to bf16 (the
kernels may sum the fp32 values before that rounding); n 2^-24 bounds the fp32 summation.  fp32
drops the 2^-8.  A wrong count of partial rows misses or adds whole rows: orders above this bound.

Input families (``inputs``), different data per batch and head, rounded to the storage type:
  randn  the baseline, unit normal q, k, v, dO
  rows   q_i *= 2^((i%5)-2), k_j *= 2^((3j%4)-2), V += 3 (-1)^col, dO_i = dO_i 2^((i%3)-1) + 1: lse
         and delta differ strongly between neighbouring rows, and the dP - delta cancellation is
         large.  Here q and k start from N(0, 1/2): with unit variance the largest |q_i| |k_j|
         pairs (x 8) reach Sb ~ 0.3 * 8 * 64 * 0.64 = 98 +- 15 at scale 0.3, over the 2^-10 limit of
         ex (Sb < 126) in a few percent of them; halving the products leaves Sb < 80, |a| < 45
  edge   k_{N-1} = 6 mean(q over the last 20 rows), k_0 = 6 mean(q over the rest): softmax mass on
         the last valid key and on key 0; the row after a batch's last one is the next batch's
         large k_0, so a read across the batch boundary shows.  A mean over fewer than 20 rows
         divides by 20 all the same (N = 1: k_0 = 0.3 q_0), or a = 6 scale |q_0|^2 ~ 115 leaves
         the conditioning limit
  flat   K = 0: lse = log N, o = the column mean of V, P exact in bf16: pins the count of masked keys
"""
from __future__ import annotations

import math

import numpy as np
import torch

import ref_gemm as rg
from ref_gemm import BF, T_FN_ULPS, U32, UBF, guards_intact, padded, worst_ratio  # noqa: F401

DH = 64
F32 = torch.float32
TINY = 2.0 ** -126
EX_MAX, A_MAX = 2.0 ** -10, 80.0
FAMILIES = ("randn", "rows", "edge", "flat")
LOG2E = float(np.float32(1.4426950408889634))
LN2 = float(np.float32(0.6931471805599453))
CHUNK = 16          # (batch, head) pairs per float64 step


def f32_scale(scale) -> float:
    """The scale as the API receives it: a float32."""
    return float(np.float32(scale))


# --------------------------------------------------------------------------- layouts
def heads(x: torch.Tensor, B, N, H) -> torch.Tensor:
    """[B*N, H*64] -> [B*H, N, 64] (a copy, dtype kept)."""
    return x.reshape(B, N, H, DH).permute(0, 2, 1, 3).reshape(B * H, N, DH)


def tokens(x: torch.Tensor, B, N, H) -> torch.Tensor:
    """[B*H, N, 64] -> [B*N, H*64]."""
    return x.reshape(B, H, N, DH).permute(0, 2, 1, 3).reshape(B * N, H * DH)


def split_qkv(qkv: torch.Tensor, B, N, H):
    """qkv [B*N, 3*H*64] -> q, k, v, each [B*H, N, 64]."""
    D = H * DH
    return tuple(heads(qkv[:, i * D:(i + 1) * D], B, N, H) for i in range(3))


# --------------------------------------------------------------------------- inputs
def inputs(family, B, N, H, dtype, seed=0):
    """(qkv [B*N, 3*H*64], dO [B*N, H*64]) of ``dtype`` (see the module docstring)."""
    assert family in FAMILIES, family
    g = torch.Generator().manual_seed(1000 * seed + FAMILIES.index(family))
    q, k, v, do = (torch.randn(B * H, N, DH, generator=g, dtype=torch.float64) for _ in range(4))
    i = torch.arange(N)
    if family == "rows":
        q = q * (0.5 ** 0.5) * (2.0 ** ((i % 5) - 2)).view(1, N, 1)
        k = k * (0.5 ** 0.5) * (2.0 ** (((3 * i) % 4) - 2)).view(1, N, 1)
        v = v + 3.0 * (1 - 2 * (torch.arange(DH) % 2)).view(1, 1, DH)
        do = do * (2.0 ** ((i % 3) - 1)).view(1, N, 1) + 1.0
    elif family == "edge":
        k = k.clone()
        if N > 20:
            k[:, 0] = 6.0 * q[:, :N - 20].sum(1) / max(N - 20, 20)
        k[:, N - 1] = 6.0 * q[:, max(0, N - 20):].sum(1) / 20
    elif family == "flat":
        k = torch.zeros_like(k)
    qkv = torch.cat([tokens(t, B, N, H) for t in (q, k, v)], 1)
    return qkv.to(dtype).contiguous(), tokens(do, B, N, H).to(dtype).contiguous()


# --------------------------------------------------------------------------- float64 reference
def _units(dtype):
    bf = dtype == BF
    return (UBF if bf else 0.0), (UBF if bf else U32)


def _exponent(q, k, scale):
    """a, ex of a chunk of pairs (q, k float64 [P, N, 64]); refuses ill-conditioned inputs."""
    a = scale * (q @ k.transpose(1, 2))
    sb = scale * (q.abs() @ k.abs().transpose(1, 2))
    amax = a.abs().amax(-1, keepdim=True)
    ex = 2 * (DH + 1) * U32 * sb + 4 * U32 * (a.abs() + amax) + T_FN_ULPS * U32
    assert ex.max().item() < EX_MAX, f"ill-conditioned: max ex {ex.max().item():.3g} >= 2^-10"
    assert a.abs().max().item() < A_MAX, f"ill-conditioned: max |a| {a.abs().max().item():.3g} >= 80"
    return a, ex


def _chunks(P):
    return [slice(s, min(s + CHUNK, P)) for s in range(0, P, CHUNK)]


def forward(qkv, B, N, H, scale, dtype):
    """{"o": (ref, tol) [B*N, H*64], "lse": (ref, tol) [B*H, N]}."""
    scale = f32_scale(scale)
    up, uo = _units(dtype)
    q, k, v = (t.double() for t in split_qkv(qkv, B, N, H))
    o, to, lse, tl = [], [], [], []
    for c in _chunks(B * H):
        a, ex = _exponent(q[c], k[c], scale)
        L = torch.logsumexp(a, -1)
        P = torch.exp(a - L.unsqueeze(-1))
        av = v[c].abs()
        oc = P @ v[c]
        exm = ex.amax(-1)
        floor = 4 * TINY * (av.sum(1, keepdim=True) + N)
        o.append(oc)
        to.append(((up + ex) * P) @ av + 2 * (N + 1) * U32 * (P @ av)
                  + ((N + 2) * U32 + exm + uo).unsqueeze(-1) * oc.abs() + floor)
        lse.append(L)
        tl.append(exm + (N + 2) * U32 + T_FN_ULPS * U32 + 2 * U32 * L.abs())
    cat = torch.cat
    return {"o": (tokens(cat(o), B, N, H), tokens(cat(to), B, N, H)), "lse": (cat(lse), cat(tl))}


def backward(qkv, o, do, lse, B, N, H, scale, dtype):
    """{"dq" | "dk" | "dv": (ref, tol) [B*N, H*64]} of the given o (storage type) and lse (fp32)."""
    scale = f32_scale(scale)
    up, uo = _units(dtype)
    q, k, v = (t.double() for t in split_qkv(qkv, B, N, H))
    oh, dh = heads(o.double(), B, N, H), heads(do.double(), B, N, H)
    ls = lse.double().reshape(B * H, N)
    out = {n: ([], []) for n in ("dq", "dk", "dv")}
    for c in _chunks(B * H):
        a, ex = _exponent(q[c], k[c], scale)
        lc = ls[c].unsqueeze(-1)
        P = torch.exp(a - lc)
        d_o, aq, ak = dh[c], q[c].abs(), k[c].abs()
        delta = (d_o * oh[c]).sum(-1, keepdim=True)
        dpd = d_o @ v[c].transpose(1, 2) - delta
        G = P * dpd
        eps = ex + 2 * U32 * lc.abs()
        e_dp = 2 * (DH + 1) * U32 * (d_o.abs() @ v[c].abs().transpose(1, 2) + (d_o * oh[c]).abs().sum(-1, keepdim=True))
        g = P * ((up + eps + U32) * dpd.abs() + e_dp)
        Pt, Gt, gt = P.transpose(1, 2), G.transpose(1, 2), g.transpose(1, 2)
        dv = Pt @ d_o
        tdv = (((up + eps) * P).transpose(1, 2) @ d_o.abs() + 2 * (N + 1) * U32 * (Pt @ d_o.abs()) + uo * dv.abs()
               + 4 * TINY * (d_o.abs().sum(1, keepdim=True) + N))
        dk = scale * (Gt @ q[c])
        tdk = (scale * (gt @ aq + 2 * (N + 1) * U32 * (Gt.abs() @ aq)) + (uo + U32) * dk.abs()
               + 4 * TINY * scale * (dpd.abs().transpose(1, 2) @ aq + N))
        dq = scale * (G @ k[c])
        tdq = (scale * (g @ ak + 2 * (N + 1) * U32 * (G.abs() @ ak)) + (uo + U32) * dq.abs()
               + 4 * TINY * scale * (dpd.abs() @ ak + N))
        for n, r, t in (("dq", dq, tdq), ("dk", dk, tdk), ("dv", dv, tdv)):
            out[n][0].append(r)
            out[n][1].append(t)
    return {n: (tokens(torch.cat(r), B, N, H), tokens(torch.cat(t), B, N, H)) for n, (r, t) in out.items()}


def reference(qkv, do, B, N, H, scale, dtype):
    """One forward and the backward of ITS o (rounded to ``dtype``) and lse (fp32):
    {"o", "lse", "hi+lo", "dq", "dk", "dv": (ref, tol); "o_in", "lse_in": what the backward is fed}."""
    out = forward(qkv, B, N, H, scale, dtype)
    if dtype == BF:         # tol_o with ubf^2 in place of uo
        r, t = out["o"]
        out["hi+lo"] = (r, t - (UBF - UBF * UBF) * r.abs())
    o_in, lse_in = out["o"][0].to(dtype), out["lse"][0].float()
    out.update(backward(qkv, o_in, do, lse_in, B, N, H, scale, dtype))
    out["o_in"], out["lse_in"] = o_in, lse_in
    return out


def bias_bound(dqkv: torch.Tensor, n: int, bf16: bool):
    """(ref, tol) float64 [3*H*64] of the bias gradient from the RETURNED dqkv [n, 3*H*64]."""
    g = dqkv.double()
    return g.sum(0), ((UBF if bf16 else 0.0) + n * U32) * g.abs().sum(0)


# --------------------------------------------------------------------------- guarded buffers
def aligned(rows, cols, dtype, fill) -> rg.Padded:
    """rg.padded with a dense pitch and as many leading guard elements as put the window on a 256-byte
    boundary of the allocation (the entry points take device allocations: whole-line stores)."""
    es = 2 if dtype == BF else 4
    per = 256 // es
    return rg.padded(rows, cols, cols, dtype, fill, offset=(-rg.GUARD_ROWS * cols) % per)


# --------------------------------------------------------------------------- CPU emulation
def emulate(qkv, do, B, N, H, scale, dtype, o=None, lse=None, mut=None):
    """The kernels' arithmetic on the CPU in float32, keys and queries summed in 32-row blocks (an
    order other than the reference's): P and dS rounded to bf16 before their products and a bf16
    store for ``dtype`` bf16.  The backward reads ``o`` / ``lse`` when given, else its own forward's.
    ``mut`` switches on the deliberately wrong variants tests/test_attention_ref_cpu.py rejects:
      drop_last_key   True (every query) | (q0, q1) (those query rows only)
      extra_zero_key  a zero K / V row is admitted by the key mask
      scale_exp       the scale used in the exponent;  scale_dk: ... at the dK store
      swap_lse        (i, j) of pair 1: the backward reads each other's lse
      delta_shift     delta of row i + 1 is used for row i
      dkv_skip_last_q the last query row is missing from dK / dV
      ds_transpose    (q0, k0): that 32x32 block of dS is transposed
      v_next_head     the forward of head hd reads the V of head hd + 1 (pair p + 1)
    Returns {"o", "lse", "dq", "dk", "dv"} in the API's layouts (o, dq, dk, dv of ``dtype``)."""
    mut = mut or {}
    bf = dtype == BF
    rb = (lambda t: t.to(BF).float()) if bf else (lambda t: t)
    scale = np.float32(scale)
    c2 = float(np.float32(mut.get("scale_exp", scale)) * np.float32(LOG2E))
    scale = float(scale)
    sdk = float(np.float32(mut.get("scale_dk", scale)))
    q, k, v = (t.float() for t in split_qkv(qkv, B, N, H))
    dh = heads(do.float(), B, N, H)
    P_ = B * H

    def blocked(x, y):          # x @ y in fp32, the reduction in 32-wide blocks
        acc = torch.zeros(x.shape[0], y.shape[1])
        for s in range(0, x.shape[1], 32):
            acc = acc + x[:, s:s + 32] @ y[s:s + 32]
        return acc

    o_f, lse_f = torch.empty(P_, N, DH), torch.empty(P_, N)
    for p in range(P_):
        kk, vv = k[p], v[(p + 1) % P_] if mut.get("v_next_head") else v[p]
        if mut.get("extra_zero_key"):
            kk, vv = torch.cat([kk, torch.zeros(1, DH)]), torch.cat([vv, torch.zeros(1, DH)])
        s = blocked(q[p], kk.t().contiguous())
        drop = mut.get("drop_last_key")
        if drop:
            r0, r1 = (0, N) if drop is True else drop
            s[r0:r1, N - 1] = -math.inf
        m = s.amax(-1, keepdim=True) * c2
        pw = torch.exp2(s * c2 - m)
        l = pw.sum(-1, keepdim=True)
        o_f[p] = blocked(rb(pw), vv) * (1.0 / l)
        lse_f[p] = ((m + torch.log2(l)) * LN2).squeeze(-1)
    o_out = tokens(o_f, B, N, H).to(dtype)
    out = {"o": o_out, "lse": lse_f}
    o_in = heads((o_out if o is None else o).float(), B, N, H)
    ls = (lse_f if lse is None else lse.float().reshape(P_, N)).clone()
    if mut.get("swap_lse"):
        i, j = mut["swap_lse"]
        ls[1, [i, j]] = ls[1, [j, i]]
    dq, dk, dv = (torch.empty(P_, N, DH) for _ in range(3))
    for p in range(P_):
        s = blocked(q[p], k[p].t().contiguous())
        pw = torch.exp2(s * c2 - (ls[p] * LOG2E).unsqueeze(-1))
        delta = (dh[p] * o_in[p]).sum(-1, keepdim=True)
        if mut.get("delta_shift"):
            delta = torch.roll(delta, -1, 0)
        ds = pw * (blocked(dh[p], v[p].t().contiguous()) - delta)
        if mut.get("ds_transpose"):
            q0, k0 = mut["ds_transpose"]
            ds[q0:q0 + 32, k0:k0 + 32] = ds[q0:q0 + 32, k0:k0 + 32].t().clone()
        pb, sb = rb(pw), rb(ds)
        dq[p] = blocked(sb, k[p]) * scale
        if mut.get("dkv_skip_last_q"):
            pb, sb = pb.clone(), sb.clone()
            pb[N - 1], sb[N - 1] = 0.0, 0.0
        dv[p] = blocked(pb.t().contiguous(), dh[p])
        dk[p] = blocked(sb.t().contiguous(), q[p]) * sdk
    for n, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        out[n] = tokens(t, B, N, H).to(dtype)
    return out
