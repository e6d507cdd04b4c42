"""Float64 reference of the kernels that move data into and out of the transformer stack -- patch
im2col, token assembly and its backward (full and gathered), the classifier head, the loss, the casts,
the operand splits, the backward's dropout mask and the small fp32 Dense layers (csrc/elementwise.hip,
split.hip, dense.hip and the gathered kernels of patchdrop.hip) -- with a per-element bound DERIVED from
the arithmetic, a bit-exact restatement wherever the arithmetic pins the bits, and mutated restatements
that the bounds must reject.  Plain torch / numpy on the CPU.  TEST INFRASTRUCTURE ONLY.

u = 2^-24.  A sum of n fp32 terms in ANY order, each term one rounded product (or one fused one), carries
at most n roundings per term: |got - ref| <= n u sum|terms| to first order; every bound below is
multiplied by SLACK = 1 + 2^-10 for the neglected products of errors (every relative error here is below
2^-12).  Adding a zero is exact, so a tree over lanes that hold nothing costs no rounding.

Bitwise (tol 0):
  im2col(_keep), dtok, dtok_lp, the casts   a move, or one round-to-nearest-even conversion (torch CPU)
  split_bf16x3 / split_bf16f8 / weights      hi = bf16(x), lo = bf16(x - hi); hi8 = e4m3(hi), lo8 =
                                             e4m3((x - hi) 2^9), saturating at +-448 (ref_layernorm.split_f8,
                                             ref_gemm.f8_rows).  The e4m3 bytes of a NaN / of inf - inf
                                             are not pinned by the header: the f8 ``special`` family holds
                                             no NaN and no infinity.
  tokens_assemble(_keep)                     one fp32 add
  dropout_apply                              kept: one fp32 product (then RNE to bf16); dropped: +0
  dpos, dcls                                 s = 0; s += dx[b] for b = 0, 1, ...; out = prev + s  (float32
                                             numpy loop: plain adds, no fast-math in the build)
Bounded (float64 reference):
  head_fwd      (D + 2) u (sum|y||w| + |b|)          D products, at most D - 1 inexact adds, the bias add
  head_bwd dy   (C + 1) u sum|dl||w|
           dw   (B + 2) u (sum_b|dl||y| + |prev|)    db  (B + 2) u (sum_b|dl| + |prev|)
  dpos, dcls    (B + 1) u (sum_b|dx| + |prev|)       (besides the bitwise restatement)
  dense_f32_fwd (K + 2) u (sum|x||w| + |b|)          ReLU is 1-Lipschitz: the same bound
  dense_f32_bwd g = dy [y > 0] exactly (y is an input);  dx (N + 1) u sum|g||w|;
                dw (M + 2) u (sum_m|g||x| + |prev|);  db (M + 2) u (sum_m|g| + |prev|)
  loss, MSE     term = (z - t)^2 / C: three roundings; a thread adds ceil(B/256) C terms (the first add is to
                zero), the tree adds 8 times, 1/B and the product round once each:
                  loss  (ceil(B/256) C + 12) u L          (every term is >= 0, so sum|terms| / B = L)
                  dl = 2 (z - t) (1/B) / C: four roundings, 4 u |ref|
  loss, CE      lse = mx + logf(sum_c expf(z_c - mx)), T = T_FN_ULPS (ref_gemm: the project's figure for device
                expf / logf, t_fn = T u max(|value|, 1); for expf, whose value is <= 1 here, T u value + TINY
                with TINY = 2^-126, below which a result may be flushed to zero).  With e_c = exp(z_c - mx),
                s = sum e_c >= 1:
                  expf(fl(z_c - mx)) = e_c (1 + r_c),  |r_c| <= (|z_c - mx| + T) u
                  the sum: C roundings               rho = sum_c e_c |r_c| / s + C u + C TINY
                  E_lse = rho + T u max(log s, 1) + u |lse|          (log(s (1 + rho)) <= log s + rho)
                  row loss lse - z_t:                E_row = E_lse + u |lse - z_t|   (label outside [0, C):
                                                     the row loss is lse, E_row = E_lse)
                  loss  sum_b E_row / B + (ceil(B/256) + 9) u sum_b|row| / B
                        (ceil(B/256) - 1 adds per thread, 8 of the tree, 1/B and the product)
                  dl_c = (expf(fl(z_c - lse)) - [c == t]) (1/B),  p_c = exp(z_c - lse):
                        (p_c (E_lse + u |z_c - lse| + T u) + TINY + 3 u |p_c - [c == t]|) / B
The one number taken on trust is T_FN_ULPS.

Mutations (``mut=``): each restatement can be made subtly wrong in the ways listed in MUTATIONS; the CPU
tests require every bound / bit comparison to reject each of them."""
from __future__ import annotations

import numpy as np
import torch

import ref_gemm as rg
import ref_layernorm as rl
from oracle import vit_ref

U = 2.0 ** -24
T_FN = rg.T_FN_ULPS
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
BF = torch.bfloat16
F64 = torch.float64
GRID_ITEMS = 8192 * 256          # items one trip of a capped grid-stride launch covers (common.h grid_cap)

FAMILIES = ("rows", "int", "cancel")
MUTATIONS = ("khkw", "rowshift", "pos_prev", "cls_tok", "drop_b", "last_wave", "d_lt_D", "trunc", "pattern",
             "f8_off", "one_trip", "no_invB")

# ------------------------------------------------------------------------------------------- the matrix
IM2COL_SHAPES = ((1, 4, 4), (3, 8, 4), (3, 16, 8), (1, 32, 8), (5, 16, 8), (3, 32, 16), (16, 32, 16), (1, 64, 64))
IM2COL_BS = (1, 3)
TOKEN_DS = (4, 64, 192, 260)
TOKEN_NPS = (1, 16, 49)
TOKEN_BS = (1, 7, 8, 9, 16, 19)
TOKEN_WALK_FWD = (646, 49, 260)           # B, np, D: B (np + 1) D / 4 just past 2^21 + 300, an odd last trip
TOKEN_WALK_BWD = (659, 49, 260)           # the same for B np D / 4
CAST_NS = (1, 7, 8, 9, 2047, 2 ** 24 + 8 * 300 + 5)
CAST_SPECIAL_N = 4099
SPLIT_SHAPES = ((1, 4), (5, 64), (37, 128), (3, 192), (197, 768))
SPLIT_WALK_F8 = (2051, 4096)
SPLIT_WALK_X3 = (2051, 4100)
# (rows, K, pattern) per weight; the 8-weight set holds more than 2^21 items
BATCH_SETS = (((300, 128, 3),), ((5, 64, 1), (37, 128, 3), (3, 192, 1)),
              ((5, 64, 1), (37, 128, 3), (3, 192, 1), (197, 768, 1), (64, 256, 3), (1, 64, 1), (2, 128, 1),
               (10930, 768, 3)))
DROP_SHAPES = ((1, 4), (37, 132), (197, 768))
DROP_WALK = (2051, 4100)
HEAD_DS = (1, 63, 64, 65, 192, 769)
HEAD_CS = (1, 3, 10, 1000)
HEAD_BS = (1, 15, 16, 17, 37)
LOSS_BS = (1, 37, 255, 256, 257, 513)
LOSS_CS = (1, 2, 3, 1000)
DENSE_SHAPES = ((1, 1, 1), (3, 256, 5), (37, 256, 256), (5, 7, 3))


def cdiv(a, b):
    return -(-a // b)


def f8_patterns(K):
    return ([0, 1] if K % 64 == 0 else []) + ([2, 3] if K % 128 == 0 else [])


# ------------------------------------------------------------------------------------------- inputs
def gen(*key):
    """A generator seeded by the key (strings and integers), the same in every process."""
    seed = 0
    for k in key:
        v = sum(ord(c) * 131 ** i for i, c in enumerate(k)) if isinstance(k, str) else int(k)
        seed = (seed * 1000003 + v) % (2 ** 61 - 1)
    return torch.Generator().manual_seed(seed)


def family(name, rows, cols, *key):
    """fp32 [rows, cols] of a named family; sums along axis 0 (the batch) are what ``cancel`` cancels."""
    g = gen(name, rows, cols, *key)
    if name == "int":
        return torch.randint(-8, 9, (rows, cols), generator=g).float()
    x = torch.randn(rows, cols, generator=g)
    if name == "rows":
        e = torch.randint(-6, 7, (rows, 1), generator=g).float()
        return x * torch.pow(torch.tensor(2.0), e)
    if name == "cancel":
        h = rows // 2
        v = x[:h]
        out = 1e-6 * x.clone()
        out[:h] = v
        out[h:2 * h] = -v * (1 + 1e-6 * torch.randn(h, cols, generator=g))
        return out[torch.randperm(rows, generator=g)] if rows > 1 else out
    assert name == "randn", name
    return x


def special(n, f8=False):
    """fp32 [n]: +-0, subnormals, bf16 ties of both parities, the largest finite fp32, |x| around 224 and 448
    (the e4m3 saturation and its last binade), +-inf and NaN (not for the f8 splits), among ordinary values."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,          # zeros, subnormals
            0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,  # ties: even, odd; near ties
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x00800000]                      # largest finite, smallest normal
    vals = [223.9, 224.0, 224.1, 232.0, 240.0, 447.9, 448.0, 448.1, 464.0, 480.0, 1000.0, -224.0, -448.0, -449.0,
            -3e4, 0.0625, 2.0 ** -9, 2.0 ** -10, 1.0 + 2.0 ** -9, 447.0 + 2.0 ** -9]
    if not f8:
        bits += [0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    sp = torch.cat([torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy()), torch.tensor(vals)])
    x = torch.randn(n, generator=gen("special", n)) * 3
    idx = torch.arange(n)
    k = sp.numel()
    sel = idx % 3 == 0
    x[sel] = sp[(idx[sel] // 3) % k]
    return x


def bits_of(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def same_bits(got, exp):
    """Bitwise equal, a NaN in ``exp`` matching any NaN (the payload is not pinned)."""
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False
    if not exp.is_floating_point():
        return bool(torch.equal(got, exp))
    nan = torch.isnan(exp.float())
    return bool((torch.isnan(got.float()) == nan).all() and torch.equal(bits_of(got)[~nan], bits_of(exp)[~nan]))


def store_bf16(x, mut=None):
    return rg.bf16_trunc(x) if mut == "trunc" else x.float().to(BF)


def one_trip(out, items, per_item, mut, fill):
    """mut 'one_trip': what a launch leaves when only the first GRID_ITEMS items are served: the flat output
    past them keeps ``fill`` (per_item consecutive elements per item)."""
    if mut == "one_trip" and items > GRID_ITEMS:
        flat = out.reshape(-1)
        flat[GRID_ITEMS * per_item:items * per_item] = fill
    return out


# ------------------------------------------------------------------------------------------- im2col
def im2col(img, P, keep=None, mut=None):
    """fp32 [rows, C P P] by explicit indices: row b np + ph G + pw (keep: row b K + j reads patch keep[b][j],
    an index outside [0, np) gives a zero row), column c P P + kh P + kw."""
    B, C, S, _ = img.shape
    G = S // P
    np_ = G * G
    if keep is None:
        keep = np.tile(np.arange(np_), (B, 1))
    keep = np.asarray(keep).reshape(B, -1)
    if mut == "rowshift":
        keep = np.where((keep >= 0) & (keep < np_), (keep + 1) % np_, keep)
    valid = (keep >= 0) & (keep < np_)
    pid = np.where(valid, keep, 0)
    b = np.arange(B)[:, None, None]
    ph, pw = (pid // G)[:, :, None], (pid % G)[:, :, None]
    col = np.arange(C * P * P)[None, None, :]
    c, kh, kw = col // (P * P), (col % (P * P)) // P, col % P
    if mut == "khkw":
        kh, kw = kw, kh
    out = np.where(valid[:, :, None], img.numpy()[b, c, ph * P + kh, pw * P + kw], np.float32(0))
    return torch.from_numpy(np.ascontiguousarray(out.reshape(-1, C * P * P)).astype(np.float32))


def im2col_expected(img, P, bf16, keep=None, mut=None):
    out = im2col(img, P, keep, mut)
    return store_bf16(out, mut) if bf16 else out


def keep_lists(B, np_, K, bad=False):
    """int32 [B, K] ascending kept patch numbers (the hashed selection of ref_patchdrop); ``bad``: one -1 and one
    np among them (documented: no patch, a zero row)."""
    import ref_patchdrop
    keep = ref_patchdrop.keep_indices(7, B, np_, K).astype(np.int32)
    if bad:
        keep[0, 0] = -1
        keep[B - 1, K - 1] = np_
    return keep


def slot_lists(keep, np_, bad=False):
    """int32 [B, np]: the inverse of keep (-1: dropped); ``bad``: one entry equal to K and one below -1."""
    B, K = keep.shape
    slot = np.full((B, np_), -1, dtype=np.int32)
    for b in range(B):
        for j, p in enumerate(keep[b]):
            if 0 <= p < np_:
                slot[b, p] = j
    if bad:
        slot[0, np_ - 1] = K
        slot[B - 1, 0] = -7
    return slot


# ------------------------------------------------------------------------------------------- token assembly
def assemble(tok, cls, pos, B, np_, D, keep=None, mut=None):
    """fp32 [B, N, D], N = 1 + np (1 + K with keep): x[b][0] = cls + pos[0], x[b][1 + j] = tok[b K + j] +
    pos[1 + keep[b][j]] (a zero row for an index outside [0, np)); one float32 add."""
    K = np_ if keep is None else keep.shape[1]
    kp = np.tile(np.arange(np_), (B, 1)) if keep is None else np.asarray(keep)
    t = tok.numpy().reshape(B, K, D)
    x = np.zeros((B, K + 1, D), dtype=np.float32)
    z = np.zeros(D, dtype=np.float32)
    c = z if cls is None else cls.numpy()
    p = None if pos is None else pos.numpy().reshape(np_ + 1, D)
    for b in range(B):
        x[b, 0] = t[b, 0] if mut == "cls_tok" else c
        if p is not None:
            x[b, 0] = x[b, 0] + p[0]
        valid = (kp[b] >= 0) & (kp[b] < np_)
        rows = np.where(valid, kp[b], 0)
        v = t[b].copy()
        if p is not None:
            v = v + p[(rows if mut == "pos_prev" else 1 + rows)]
        x[b, 1:] = np.where(valid[:, None], v, np.float32(0))
    return torch.from_numpy(x)


def assemble_ref(tok, cls, pos, B, np_, D):
    """The float64 statement with torch.cat (full form): what the CPU tests compare ``assemble`` with."""
    c = torch.zeros(D, dtype=F64) if cls is None else cls.double()
    x = torch.cat([c.expand(B, 1, D), tok.double().view(B, np_, D)], 1)
    return x if pos is None else x + pos.double().view(np_ + 1, D)


def split_bwd(dx, B, K, D, mut=None):
    """(dtok fp32 [B K, D], dtok_lp bf16): dx[:, 1:]."""
    d = dx.view(B, K + 1, D)[:, 1:].reshape(B * K, D).contiguous()
    return d, store_bf16(d, mut)


def pos_bwd(dx, prev_pos, prev_cls, B, np_, D, slot=None, mut=None):
    """{'dpos': (exact fp32 restatement, ref, tol), 'dcls': ...}: s = sum over b in order of dx[b][n] (gathered:
    dx[b][1 + slot[b][p]] over the samples whose slot is in [0, K)), out = prev + s."""
    K = np_ if slot is None else dx.numel() // (B * D) - 1
    d = dx.numpy().reshape(B, K + 1, D)
    sl = np.tile(np.arange(np_), (B, 1)) if slot is None else np.asarray(slot)
    s32 = np.zeros((np_ + 1, D), dtype=np.float32)
    s64 = np.zeros((np_ + 1, D))
    a64 = np.zeros((np_ + 1, D))
    for b in range(B):
        valid = (sl[b] >= 0) & (sl[b] < K)
        rows = np.concatenate([[0], 1 + np.where(valid, sl[b], 0)])
        m = np.concatenate([[True], valid])[:, None]
        v = np.where(m, d[b][rows], np.float32(0))
        v64 = v.astype(np.float64)
        s64 += v64
        a64 += np.abs(v64)
        if mut == "drop_b" and b == B // 2:
            v = v.copy()
            v[np_ // 2, D // 3] = 0
            v[0, D // 3] = 0
        s32 = s32 + v
    out = {}
    for name, prev, sel in (("dpos", prev_pos, slice(None)), ("dcls", prev_cls, slice(0, 1))):
        if prev is None:
            continue
        p = prev.numpy().reshape(-1, D)
        exact = torch.from_numpy((p + s32[sel]).astype(np.float32))
        ref = torch.from_numpy(p.astype(np.float64) + s64[sel])
        tol = torch.from_numpy(SLACK * (B + 1) * U * (a64[sel] + np.abs(p.astype(np.float64))))
        out[name] = (exact, ref, tol)
    return out


# ------------------------------------------------------------------------------------------- casts and splits
def cast_down(x, mut=None):
    return one_trip(store_bf16(x, mut), x.numel() // 8, 8, mut, torch.tensor(0.0, dtype=BF))


def cast_up(x, mut=None):
    return one_trip(x.float(), x.numel() // 8, 8, mut, 0.0)


def split_x3(x, pattern, mut=None):
    """bf16 [rows, 3K] ([hi | hi | lo] pattern 0, [hi | lo | hi] pattern 1) and the hi copy."""
    x = x.float()
    hi = store_bf16(x, mut)
    lo = store_bf16(x - hi.float(), mut)
    if mut == "pattern":
        pattern = 1 - pattern
    out = torch.cat([hi, hi, lo] if pattern == 0 else [hi, lo, hi], 1)
    if mut == "one_trip" and x.numel() // 4 > GRID_ITEMS:
        r = GRID_ITEMS * 4 // x.shape[1] + 1
        out[r:] = 0
    return out, hi


def split_f8(x, pattern, mut=None):
    """The bf16-unit rows of vitmi_split_bf16f8: patterns 0 / 1 [rows, 2K] (ref_gemm.f8_rows), 2 / 3 [rows, 1.5K]
    (one e4m3 byte per k: hi8 / lo8), and the hi copy."""
    x = x.float()
    wform = pattern >= 2
    weight = pattern in (1, 3)
    if mut == "f8_off" and wform:
        rows, K = x.shape
        hi, hi8, lo8 = rl.split_f8(x)
        part = torch.zeros(rows, 2 * K, dtype=torch.uint8)
        c = torch.arange(K)
        part[:, (c // 64) * 128 + c % 64] = lo8 if weight else hi8
        stored = torch.cat([hi.view(torch.uint8).reshape(rows, 2 * K), part[:, :K]], 1).contiguous().view(BF)
    else:
        stored, _ = rg.f8_rows(x, weight=weight, wform=wform)
    hi = store_bf16(x, mut)
    if mut == "trunc":
        stored = stored.clone()
        stored[:, :x.shape[1]] = hi
    if mut == "one_trip" and x.numel() // 4 > GRID_ITEMS:
        stored = stored.clone()
        stored[GRID_ITEMS * 4 // x.shape[1] + 1:] = 0
    return stored, hi


def f8_width(K, pattern):
    return K + K // 2 if pattern >= 2 else 2 * K


# ------------------------------------------------------------------------------------------- dropout mask
def dropout_apply(x, seed, site, thresh, scale, bf16, mut=None):
    """kept: fl(x * scale), dropped: +0; then RNE to bf16."""
    M, N = x.shape
    keep = vit_ref.dropout_hash(seed, site, np.arange(M), np.arange(N)) >= np.uint64(thresh)
    y = np.where(keep, x.numpy() * np.float32(scale), np.float32(0)).astype(np.float32)
    out = torch.from_numpy(y)
    out = store_bf16(out, mut) if bf16 else out
    return one_trip(out, M * N // 4, 4, mut, 0.0) if M * N // 4 > GRID_ITEMS else out


# ------------------------------------------------------------------------------------------- head
def head_fwd(y, w, b):
    Y, W = y.double(), w.double()
    bv = torch.zeros(w.shape[0], dtype=F64) if b is None else b.double()
    D = y.shape[1]
    return Y @ W.t() + bv, SLACK * (D + 2) * U * (Y.abs() @ W.abs().t() + bv.abs())


def head_bwd(dl, y, w, prev_w, prev_b):
    DL, Y, W = dl.double(), y.double(), w.double()
    B, C = dl.shape
    out = {"dy": (DL @ W, SLACK * (C + 1) * U * (DL.abs() @ W.abs())),
           "dw": (prev_w.double() + DL.t() @ Y, SLACK * (B + 2) * U * (DL.abs().t() @ Y.abs() + prev_w.double().abs()))}
    if prev_b is not None:
        out["db"] = (prev_b.double() + DL.sum(0), SLACK * (B + 2) * U * (DL.abs().sum(0) + prev_b.double().abs()))
    return out


def emulate_head_fwd(y, w, b, mut=None):
    y, w = y.float(), w.float()
    if mut == "d_lt_D":
        y, w = y[:, :-1], w[:, :-1]
    out = y @ w.t()
    return out if b is None else out + b.float()


def emulate_head_bwd(dl, y, w, prev_w, prev_b, mut=None):
    dl, y, w = dl.float(), y.float(), w.float()
    B = dl.shape[0]
    rows = torch.arange(B)
    if mut == "last_wave":
        rows = rows[rows % 16 != 15]
    dw = dl[rows].t() @ y[rows]
    dy = dl @ w
    if mut == "d_lt_D":
        dw[:, -1] = 0
        dy[:, -1] = 0
    out = {"dy": dy, "dw": prev_w.float() + dw}
    if prev_b is not None:
        out["db"] = prev_b.float() + dl[rows].sum(0)
    return out


# ------------------------------------------------------------------------------------------- dense
def dense_fwd(x, w, b, act):
    X, W = x.double(), w.double()
    bv = torch.zeros(w.shape[0], dtype=F64) if b is None else b.double()
    ref = X @ W.t() + bv
    return (ref.clamp_min(0) if act else ref), SLACK * (x.shape[1] + 2) * U * (X.abs() @ W.abs().t() + bv.abs())


def dense_bwd(dy, y, x, w, prev_w, prev_b, act):
    G = dy.double() * ((y > 0).double() if act else 1.0)
    X, W = x.double(), w.double()
    M, N = dy.shape
    out = {"dx": (G @ W, SLACK * (N + 1) * U * (G.abs() @ W.abs())),
           "dw": (prev_w.double() + G.t() @ X, SLACK * (M + 2) * U * (G.abs().t() @ X.abs() + prev_w.double().abs()))}
    if prev_b is not None:
        out["db"] = (prev_b.double() + G.sum(0), SLACK * (M + 2) * U * (G.abs().sum(0) + prev_b.double().abs()))
    return out


def emulate_dense_fwd(x, w, b, act):
    out = x.float() @ w.float().t()
    if b is not None:
        out = out + b.float()
    return out.clamp_min(0) if act else out


def emulate_dense_bwd(dy, y, x, w, prev_w, prev_b, act):
    g = dy.float() * ((y > 0).float() if act else 1.0)
    out = {"dx": g @ w.float(), "dw": prev_w.float() + g.t() @ x.float()}
    if prev_b is not None:
        out["db"] = prev_b.float() + g.sum(0)
    return out


# ------------------------------------------------------------------------------------------- loss
def loss_inputs(kind, fam, B, C):
    """(logits fp32 [B, C], target): int64 labels in [0, C) for CE, fp32 [B, C] for MSE.  ``spike``: one +80 logit
    per row over a -80 tail (finite; exp(-160) is below fp32)."""
    g = gen("loss", kind, fam, B, C)
    if fam == "spike":
        z = torch.full((B, C), -80.0) + torch.randn(B, C, generator=g)
        pos = torch.randint(0, C, (B,), generator=g)
        z[torch.arange(B), pos] = 80.0
    else:
        z = family("rows", B, C, "loss")
    if kind == "ce":
        t = torch.randint(0, C, (B,), generator=g)
        if fam == "spike" and B > 1:
            t[::2] = pos[::2]            # half the rows are confident and right: p_t - 1 cancels
        return z, t
    return z, z + torch.randn(B, C, generator=g)


def loss_tail(B):
    return cdiv(B, 256)


def mse(z, t):
    Z, T = z.double(), t.double()
    B, C = z.shape
    L = ((Z - T) ** 2).sum() / (B * C)
    dl = 2 * (Z - T) / (B * C)
    return {"loss": (L.view(1), SLACK * (loss_tail(B) * C + 12) * U * L.view(1)), "dl": (dl, SLACK * 4 * U * dl.abs())}


def ce(z, t):
    """Labels outside [0, C) match no class: row loss lse, gradient softmax / B."""
    Z = z.double()
    B, C = z.shape
    mx = Z.max(1, keepdim=True).values
    a = Z - mx
    e = a.exp()
    s = e.sum(1, keepdim=True)
    logs = s.log()
    lse = mx + logs
    hit = (t >= 0) & (t < C)
    y = torch.zeros(B, C, dtype=F64)
    y[hit, t[hit]] = 1.0
    zt = (Z * y).sum(1, keepdim=True)
    row = torch.where(hit.view(B, 1), lse - zt, lse)
    rho = (e * (a.abs() + T_FN) * U).sum(1, keepdim=True) / s + C * U + C * TINY
    e_lse = rho + T_FN * U * logs.clamp_min(1.0) + U * lse.abs()
    e_row = e_lse + torch.where(hit.view(B, 1), U * row.abs(), torch.zeros_like(row))
    L = row.sum() / B
    t_loss = e_row.sum() / B + (loss_tail(B) + 9) * U * row.abs().sum() / B
    p = (Z - lse).exp()
    dl = (p - y) / B
    t_dl = (p * (e_lse + U * (Z - lse).abs() + T_FN * U) + TINY + 3 * U * (p - y).abs()) / B
    return {"loss": (L.view(1), SLACK * t_loss.view(1)), "dl": (dl, SLACK * t_dl)}


def emulate_loss(kind, z, t, mut=None):
    """The kernel's arithmetic in float32 (torch's expf / logf): {'loss': [1], 'dl': [B, C]}."""
    z = z.float()
    B, C = z.shape
    inv = torch.tensor(1.0) if mut == "no_invB" else torch.tensor(1.0) / B
    if kind == "mse":
        d = z - t.float()
        return {"loss": ((d * d / C).sum() * (torch.tensor(1.0) / B)).view(1), "dl": 2.0 * d * inv / C}
    mx = z.max(1, keepdim=True).values
    lse = mx + (z - mx).exp().sum(1, keepdim=True).log()
    hit = (t >= 0) & (t < C)
    y = torch.zeros(B, C)
    y[hit, t[hit]] = 1.0
    row = lse - (z * y).sum(1, keepdim=True)
    return {"loss": (row.sum() * (torch.tensor(1.0) / B)).view(1), "dl": ((z - lse).exp() - y) * inv}


def worst_ratio(got, ref, tol):
    return rg.worst_ratio(got, ref, tol)
