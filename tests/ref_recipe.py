"""Float64 reference of the kernels that make up a training recipe around the model -- the soft-target
cross-entropy with its fold and metrics record and the mixup / cutmix image pass (csrc/loss.hip), the SLS
preprocessing and the row gather (csrc/sls.hip), and the patch selection (csrc/patchdrop.hip) -- with a
per-element bound DERIVED from the arithmetic, a bit-exact restatement wherever the arithmetic pins the bits,
float32 emulations of each kernel's own arithmetic, and mutated emulations that the bounds and the bit
comparisons must reject.  Plain numpy on the CPU.  TEST INFRASTRUCTURE ONLY.

u = 2^-24, T = ref_gemm.T_FN_ULPS (device expf / logf: t_fn = T u max(|value|, 1); for expf, whose value is
<= 1 here, T u value + TINY with TINY = 2^-126, below which a result may be flushed to zero).  Every bound is
first order and multiplied by SLACK = 1 + 2^-10 for the neglected products of errors, as in ref_tokens.
A result conforms iff every element's |err| / tol <= 1; an element whose reference is NaN (or infinite)
conforms iff the result is NaN (that infinity).  Nothing is excluded.

softmax_xent (one wave64 per row; a lane takes the groups of W elements g = lane, lane + 64, ...; W = 4 on
the 16-byte path, 1 on the scalar one; n = ceil(C / 64 W) steps per lane).  M = max z, a_c = z_c - M,
e_c = exp(a_c), s = sum e_c >= 1, p_c = e_c / s:
  the online (max, sum)   an element enters as expf(fl(z_c - m)) under the lane's running max m and is
                          rescaled by expf(fl(m - m')) each time the max rises to m', at last by
                          expf(fl(m_lane - M)) in the lane combine.  The rounded arguments telescope:
                          (m - z_c) + (m' - m) + ... + (M - m_lane) = |a_c|, so together they cost |a_c| u;
                          the first expf costs T u, every rescale (T + 1) u (its expf and its product).  The
                          maxima are exact, so the number of raises of every lane is known from the data:
                          R = the largest count over the row's lanes.
                            e_c as summed = e_c (1 + r_c),  |r_c| <= (|a_c| + T + (T + 1)(R + 1)) u
  the sum                 n W sequential additions per lane, six butterfly steps, all terms >= 0:
                            rho = sum_c e_c |r_c| / s + (n W + 6) u + C TINY
  lse = M + logf(se)      E_lse = rho + T u max(log s, 1) + u |lse|
  the target sums         labels: S = 1, dot = z_a exactly.  pair: wb = fl(1 - lam), S = fl(lam + wb),
                          dot = fl(fl(lam z_a) + fl(wb z_b)):  E_S = u (|wb| + |S|),
                          E_dot = 3 u (|lam z_a| + |wb z_b|).  dense: S = sum t, dot = sum t z (t != 0),
                          each n W + 6 additions, the products one more:  E_S = (n W + 6) u sum|t|,
                          E_dot = (n W + 7) u sum|t z|.  sum z (smoothing): E_sz = (n W + 6) u sum|z|
  the final products      keep = fl(1 - eps), unif = fl(fl(eps S) / C), qz = fl(fl(keep dot) + fl(unif sz)):
                            E_unif = 2 u |unif| + eps E_S / C
                            E_qz = 2 u |keep dot| + keep E_dot + 2 u |unif sz| + |sz| E_unif + unif E_sz + u |qz|
                          (eps = 0: keep = 1 and qz = dot, the product is exact: E_qz = E_dot)
                          row = fl(fl(lse S) - qz):
                            E_row = |S| E_lse + |lse| E_S + u |lse S| + E_qz + u |row|
  loss                    the fp64 fold of the fp32 rows and one rounding to fp32:
                            E_loss = sum_b E_row / B + u |loss| + (B + 10) 2^-53 sum_b |row| / B
                          (besides: bitwise the emulated fold of the rows the kernel wrote, ``fold``)
  dlogits                 g = fl(fl(fl(fl(expf(fl(z_c - M)) inv) S) - q) invB), inv = fl(1 / se):
                            E_p = |S| p_c ((|a_c| + T) u + rho + 3 u) + p_c E_S + 2 TINY (|S| + 1)
                            q_c: pair t_c = fl([c = a] lam + [c = b] wb): E_t = 2 u |t_c|; else E_t = 0;
                                 smoothing: q = fl(fl(keep t) + unif): E_q = keep E_t + 2 u |keep t| + E_unif + u |q|
                            E_g = (E_p + E_q + u |p S - q|) / B + 2 u |g|
                          A class at -inf has e = p = 0 exactly: with q = 0 its gradient is an exact zero (tol 0).
The one number taken on trust is T_FN_ULPS.

Bitwise (tol 0):
  hits            the rule of include/vitmi.h on the fp32 logits (integers)
  loss, loss_sum  ``fold``: thread t adds rows t, t + 256, ... ascending in fp64, the xor butterfly 32 .. 1 inside
                  each wave, then ((w0 + w1) + w2) + w3
  mix_batch       1 - lam once, two rounded products, one addition (ref_loss.mix); a NaN matches any NaN (the sign
                  of 0 * inf differs between host and device)
  sls_preprocess  OpenCV's 8-bit fixed point as oracle/sls_ref.py restates it, here on the flat (pitched) bytes
  gather_rows     a move; an index outside [0, n_src) gives a zero row
  patch_keep      keep / slot of ref_patchdrop.  The (key, p) tie branch is unreachable from real seeds: a search
                  over 2,560 rows of 4096 keys and 192,000 rows of 1024 keys found no two equal keys in a row
                  (a random 32-bit hash would have shown about 5 and about 20), so the hash looks injective in
                  the patch index and the tie order is stated here, not tested.

Mutations (``mut=``): MUTATIONS lists, per kernel family, the ways each emulation can be made subtly wrong; the
CPU tests require the bounds / bit comparisons to reject every one of them, but the one EQUIVALENT names: a mutation
that changes an address and no value, which the tests show to be equal instead."""
from __future__ import annotations

import numpy as np

import ref_gemm as rg
import ref_loss
import ref_patchdrop
from oracle import sls_ref, vit_ref

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
T_FN = rg.T_FN_ULPS
TINY = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -10
NEG = f32(-np.inf)
SLS_GRID_ITEMS = 16384 * 256        # items one trip of the capped sls / gather launches covers

MUTATIONS = {
    "xent": ("no_rescale", "nan_drop", "sumq_one", "unif_noS", "wb_lam", "no_invB", "tie_le"),
    "mix": ("fma", "box_off1", "box_unclamped", "plane_chunk", "u0_only"),
    "sls": ("no_round", "no_shift4", "swap_br", "x1_unclamped", "one_trip"),
    "gather": ("no_zero_row", "one_trip"),
    "keep": ("pad_zero", "chunk_base"),
}

# ------------------------------------------------------------------------------------------- the matrix
XENT_CS = (1, 2, 3, 4, 5, 63, 64, 65, 67, 68, 252, 256, 260, 1020, 1023, 1024, 1025, 1028, 1088, 2052, 4099, 65535)
XENT_BS = (1, 3, 5)
XENT_BIG_BS = (255, 256, 257, 513, 2047, 2048, 2051)
XENT_BIG_CS = (5, 8)
XENT_FORMS = ("labels", "pair", "dense")
XENT_SMOOTHINGS = (0.0, 0.1)
# how the scalar path is reached: "auto" is the 16-byte path when C % 4 == 0 and the scalar one otherwise; the
# others force the scalar path at C % 4 == 0 through one misalignment alone
XENT_WAYS = ("auto", "base", "ldl", "lds", "lddl")
XENT_SUBSETS = (("row",), ("loss",), ("dl",), ("metrics",), ("row", "loss", "dl", "metrics"))
XENT_FAMILIES = ("randn4", "spike", "equal", "halfint", "masked", "outside")
XENT_FAMILY_CS = (5, 65, 68, 1028, 4099)        # both paths, inside and past the register file
XENT_ROW_H = 2                                  # the row compared alone, inside B = 5 and inside B = 2051
XENT_NAN_CS = (64, 65, 1028, 1029)
XENT_KS = (1, 5, "C")

MIX_VEC = ((1, 4), (3, 8), (255, 4), (256, 4), (257, 4), (1025, 4), (1, 4100), (33, 128), (65, 128))
MIX_SCALAR = ((1, 1), (3, 1), (7, 9), (41, 25))
MIX_OFFSET = ((32, 32), (33, 32))               # scalar through img or out one float off, W % 4 == 0
MIX_B, MIX_C = 3, 3
MIX_LAMS = (0.0, 0.3, 1.0)
MIX_PERMS = ("identity", "roll", "outside")
MIX_BOXES = ("empty", "full", "clamped", "inverted", "pixel", "unaligned", "second_chunk", "across_chunks", "outside")
MIX_GROUPS_PER_CHUNK = 1024

SLS_SHAPES = ((1, 1, 3, 5), (1, 7, 4, 4), (7, 1, 4, 4), (2, 2, 1, 1), (13, 7, 40, 23), (64, 64, 64, 64),
              (100, 90, 33, 47), (345, 340, 128, 128))         # H, W, Ho, Wo
SLS_FRAMES = ("zeros", "full", "checker", "random")
SLS_WALK = (258, 9, 5, 128, 128)                               # n, H, W, Ho, Wo

GATHER_ROW_BYTES = (1, 4, 12, 16, 20, 48, 4100, 65536)
GATHER_N_SRC = 8
GATHER_WALKS = ((1030, 65536), (1030, 4100))                   # n, row_bytes: the 16-byte and the byte path
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1

KEEP_NPS = (1, 2, 3, 4, 5, 255, 256, 257, 259, 1023, 1025, 4093, 4094, 4095, 4096)
KEEP_B = 3
KEEP_SEED = 20240607


# Listed because a kernel could be written that way, but no output value can tell: the clamp of sx1 (and sy1)
# acts only where the source index was clamped to the last pixel, and there the table's second weight is 0.
# The clamp keeps the ADDRESS inside the row; the CPU tests show the values equal at every case.
EQUIVALENT = {"sls": ("x1_unclamped",)}


def cdiv(a, b):
    return -(-a // b)


def xent_shape_cases():
    """(B, C, way) of the shape matrix: every C at B in {1, 3, 5}; every forced way to the scalar path at each
    C % 4 == 0 and the same B; the large batches at C in {5, 8}."""
    out = [(B, C, "auto") for C in XENT_CS for B in XENT_BS]
    out += [(B, C, way) for C in XENT_CS if C % 4 == 0 for B in XENT_BS for way in XENT_WAYS[1:]]
    out += [(B, C, "auto") for C in XENT_BIG_CS for B in XENT_BIG_BS]
    return out


def xent_ways(C, form):
    """The ways that exist at this C and form: forcing needs C % 4 == 0, and lds a dense target."""
    if C % 4:
        return ("auto",)
    return tuple(w for w in XENT_WAYS if w != "lds" or form == "dense")


def keep_ks(np_):
    return sorted({1, max(np_ // 2, 1), max(np_ - 1, 1), np_})


def rng_of(*key):
    """A numpy generator seeded by the key (strings and integers), the same in every process."""
    seed = 0
    for k in key:
        v = sum(ord(c) * 131 ** i for i, c in enumerate(k)) if isinstance(k, str) else int(k)
        seed = (seed * 1000003 + v) % (2 ** 61 - 1)
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------- judging
def ratio(got, ref, tol):
    """max |got - ref| / tol over every element.  tol == 0: 0 when exact, else inf.  A NaN (infinite) reference
    element is met by a NaN (that infinity) only; a NaN where the reference has a number gives inf."""
    got, ref, tol = np.asarray(got, f64), np.asarray(ref, f64), np.asarray(tol, f64)
    got, ref, tol = np.broadcast_arrays(got.reshape(ref.shape), ref, tol)
    if got.size == 0:
        return 0.0
    nan = np.isnan(ref)
    if (np.isnan(got) != nan).any():
        return float("inf")
    inf = np.isinf(ref)
    if (got[inf] != ref[inf]).any() or np.isinf(got[~inf & ~nan]).any():
        return float("inf")
    ok = ~nan & ~inf
    err = np.abs(got[ok] - ref[ok])
    t = tol[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(t > 0, err / np.where(t > 0, t, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def same_bits_nan(got, exp):
    """Bitwise equal numpy arrays, a NaN in ``exp`` matching any NaN (the payload and the sign are not pinned)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False
    if exp.dtype.kind != "f":
        return bool(np.array_equal(got, exp))
    nan = np.isnan(exp)
    iv = {4: np.uint32, 8: np.uint64}[exp.dtype.itemsize]
    return bool((np.isnan(got) == nan).all() and np.array_equal(got.view(iv)[~nan], exp.view(iv)[~nan]))


# ------------------------------------------------------------------------------------------- xent: inputs
def xent_batch(fam, B, C):
    """dict(z, la, lb, lam, soft) of a named family.  Pairs carry lam 0, lam 1 and a pair that names one class
    twice; the dense target does not sum to 1 and has zeros.
      randn4   4 randn                          spike    +-80 among them
      equal    row 0 all 3.25                   halfint  half-integers: ties everywhere
      masked   -inf at classes of zero weight (smoothing 0 only)
      outside  labels -1 and C"""
    g = rng_of("xent", fam, B, C)
    z = (4.0 * g.standard_normal((B, C))).astype(f32)
    la, lb = g.integers(0, C, B), g.integers(0, C, B)
    lam = g.random(B).astype(f32)
    lam[0] = 1.0
    if B > 1:
        lam[1] = 0.0
    if B > 2:
        lb[2] = la[2]
    soft = (g.random((B, C)) * g.random((B, 1)) * 1.7 / C).astype(f32)
    soft[g.random((B, C)) < 0.2] = 0.0
    if fam == "spike":
        k = min(C, 6)
        for b in range(B):
            z[b, g.choice(C, k, replace=False)] = np.array([80, -80, 80, -80, 79.5, -80], f32)[:k]
    elif fam == "equal":
        z[0, :] = 3.25
    elif fam == "halfint":
        z = (np.round(z) / 2).astype(f32)
    elif fam == "masked":
        m = g.random((B, C)) < 0.4
        m[np.arange(B), la] = False
        m[np.arange(B), lb] = False
        z[m] = -np.inf
        soft[m] = 0.0
        if C > 2:                                     # lam 1: a partner of zero weight at a -inf logit
            free = [c for c in range(C) if c != la[0]]
            lb[0] = free[0]
            z[0, lb[0]] = -np.inf
            soft[0, lb[0]] = 0.0
    elif fam == "outside":
        la[0], la[-1] = -1, C
        lb[-1] = -1
    else:
        assert fam == "randn4", fam
    return dict(z=z, la=la.astype(np.int64), lb=lb.astype(np.int64), lam=lam, soft=soft)


def form_args(batch, form):
    if form == "labels":
        return dict(label_a=batch["la"])
    if form == "pair":
        return dict(label_a=batch["la"], label_b=batch["lb"], lam=batch["lam"])
    assert form == "dense", form
    return dict(soft=batch["soft"])


def width(C, way="auto"):
    """Elements per load of the path the entry point selects."""
    return 4 if C % 4 == 0 and way == "auto" else 1


def nan_columns(C):
    """(name, columns) of the non-finite cases: one NaN at column 0, 5, 63, 64, C - 1, and one whole aligned group
    of four (the first of its lane on the 16-byte path)."""
    cols = sorted({c for c in (0, 5, 63, 64, C - 1) if c < C})
    return [(f"col{c}", (c,)) for c in cols] + [("group", (8, 9, 10, 11))]


def nan_batch(C, cols):
    """B = 3 randn rows, NaN at ``cols`` of row 1, every label elsewhere."""
    b = xent_batch("randn4", 3, C)
    free = [c for c in range(C) if c not in cols]
    g = rng_of("nan", C, *cols)
    b["la"] = np.asarray(g.choice(free, 3), np.int64)
    b["lb"] = np.asarray(g.choice(free, 3), np.int64)
    b["soft"][:, list(cols)] = 0.0
    b["z"][1, list(cols)] = np.nan
    return b


# ------------------------------------------------------------------------------------------- xent: reference
def _lanes(x, C, W, fill):
    """[B, C] -> [B, n, 64, W]: step, lane, element of the wave's walk over a row."""
    B = x.shape[0]
    n = cdiv(C, 64 * W)
    p = np.full((B, n * 64 * W), fill, x.dtype)
    p[:, :C] = x
    return p.reshape(B, n, 64, W)


def raises(z, W):
    """int [B]: the most times any lane's running max rises (exact: a maximum rounds nothing)."""
    B, C = z.shape
    with np.errstate(invalid="ignore"):
        gm = np.fmax.reduce(_lanes(np.asarray(z, f32), C, W, NEG), axis=3)          # [B, n, 64]
        run = np.fmax.accumulate(gm, axis=1)
        prev = np.concatenate([np.full((B, 1, 64), NEG), run[:, :-1]], 1)
        return (gm > prev).sum(1).max(1)


def xent(z32, label_a=None, label_b=None, lam=None, soft=None, smoothing=0.0, W=1):
    """{'row': (ref [B], tol), 'loss': (ref [1], tol), 'dl': (ref [B, C], tol)} in float64, by the header's
    formulas (ref_loss.xent) and the derivation above.  ``smoothing`` is the fp32 value the entry point receives.
    A row holding a NaN logit is NaN throughout, and so is the loss."""
    z32 = np.asarray(z32, f32)
    B, C = z32.shape
    eps = float(f32(smoothing))
    row, loss, dl = ref_loss.xent(z32, label_a, label_b, lam, soft, eps)
    z = z32.astype(f64)
    t, S = ref_loss.target_dist(B, C, label_a, label_b, lam, soft)
    nW = cdiv(C, 64 * W) * W
    R = raises(z32, W).astype(f64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        M = z.max(1, keepdims=True)
        a = z - M
        e = np.exp(a)
        s = e.sum(1, keepdims=True)
        absa = np.where(e > 0, np.abs(a), 0.0)
        absa = np.where(np.isfinite(absa), absa, 0.0)
        r = (absa + T_FN + (T_FN + 1) * (R[:, None] + 1)) * U
        rho = (e * r).sum(1, keepdims=True) / s + (nW + 6) * U + C * TINY
        logs = np.log(s)
        lse = M + logs
        e_lse = (rho + T_FN * U * np.maximum(logs, 1.0) + U * np.abs(lse))[:, 0]
        lse, rho = lse[:, 0], rho[:, 0]
        zf = np.where(np.isfinite(z), z, 0.0)
        if soft is not None:
            tz = np.where(t != 0, np.abs(t * zf), 0.0).sum(1)
            e_S, e_dot = (nW + 6) * U * np.abs(t).sum(1), (nW + 7) * U * tz
            dot = np.where(t != 0, t * zf, 0.0).sum(1)
            e_t = np.zeros_like(t)
        elif lam is not None:
            wa = np.asarray(lam, f32).astype(f64)
            wb = 1.0 - wa
            za = np.array([zf[b, label_a[b]] if 0 <= label_a[b] < C else 0.0 for b in range(B)])
            zb = np.array([zf[b, label_b[b]] if 0 <= label_b[b] < C else 0.0 for b in range(B)])
            e_S, e_dot = U * (np.abs(wb) + np.abs(S)), 3 * U * (np.abs(wa * za) + np.abs(wb * zb))
            dot = wa * za + wb * zb
            e_t = 2 * U * np.abs(t)
        else:
            e_S, e_dot, e_t = np.zeros(B), np.zeros(B), np.zeros_like(t)
            dot = np.array([zf[b, label_a[b]] if 0 <= label_a[b] < C else 0.0 for b in range(B)])
        keep = 1.0 - eps
        if eps > 0:
            unif = eps * S / C
            sz, e_sz = z.sum(1), (nW + 6) * U * np.abs(z).sum(1)
            e_unif = 2 * U * np.abs(unif) + eps * e_S / C
            qz = keep * dot + unif * sz
            e_qz = (2 * U * np.abs(keep * dot) + keep * e_dot + 2 * U * np.abs(unif * sz) + np.abs(sz) * e_unif +
                    np.abs(unif) * e_sz + U * np.abs(qz))
            q = keep * t + unif[:, None]
            e_q = keep * e_t + 2 * U * np.abs(keep * t) + e_unif[:, None] + U * np.abs(q)
        else:
            e_qz = e_dot                                          # keep = 1: the product is exact
            q, e_q = t, e_t
        t_row = np.abs(S) * e_lse + np.abs(lse) * e_S + U * np.abs(lse * S) + e_qz + U * np.abs(row)
        t_loss = t_row.sum() / B + U * abs(loss) + (B + 10) * 2.0 ** -53 * np.abs(row).sum() / B
        p = e / s
        Sc = S[:, None]
        e_p = np.abs(Sc) * p * ((absa + T_FN) * U + rho[:, None] + 3 * U) + p * e_S[:, None] + 2 * TINY * (np.abs(Sc) + 1)
        t_dl = (e_p + e_q + U * np.abs(p * Sc - q)) / B + 2 * U * np.abs(dl)
        t_dl = np.where((p == 0) & (q == 0), 0.0, t_dl)           # a masked class: an exact zero
    return {"row": (row, SLACK * t_row), "loss": (np.array([loss]), SLACK * np.array([t_loss])), "dl": (dl, SLACK * t_dl)}


def hits(z32, labels, k, mut=None):
    """bool [B]: the exact top-k rule of include/vitmi.h (ref_loss.hits); mut 'tie_le' ranks an equal logit of the
    label's own or a lower index in front."""
    if mut != "tie_le":
        return ref_loss.hits(z32, labels, k)
    z = np.asarray(z32, f32)
    B, C = z.shape
    out = np.zeros(B, bool)
    for b in range(B):
        y = int(labels[b])
        if 0 <= y < C and not np.isnan(z[b, y]):
            with np.errstate(invalid="ignore"):
                out[b] = int(((z[b] > z[b, y]) | ((z[b] == z[b, y]) & (np.arange(C) <= y))).sum()) < k
    return out


def tie_cases():
    """[(name, z [B, C], labels)]: the row maximum 9.5 tied across a lane boundary (columns 63 | 64 on the scalar
    path, 255 | 256 on the 16-byte one; the label at the lower index wins, at the higher one loses), inside one
    16-byte group (label first: a hit; label last: three in front), and the all-equal row of 65535 classes with
    the last label (a hit at k = C alone)."""
    z = np.minimum(xent_batch("halfint", 4, 260)["z"], f32(9.0))
    z[0, 63] = z[0, 64] = z[1, 255] = z[1, 256] = 9.5
    z[2, 8:12] = z[3, 8:12] = 9.5
    return [("lanes", z, np.array([63, 256, 8, 11], np.int64)),
            ("equal", np.full((1, 65535), 3.25, f32), np.array([65534], np.int64))]


def fold(rows):
    """The fp64 total of the fp32 rows in the promised order: thread t of 256 adds rows t, t + 256, ... ascending,
    the xor butterfly 32 .. 1 inside each wave of 64, then ((w0 + w1) + w2) + w3.  Bit-exact."""
    rows = np.asarray(rows, f32).astype(f64)
    B = rows.size
    acc = np.zeros(256, f64)
    with np.errstate(invalid="ignore"):
        for i in range(0, B, 256):
            part = rows[i:i + 256]
            acc[:part.size] = acc[:part.size] + part
        lane = np.arange(256)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lane ^ o]
        return float(((acc[0] + acc[64]) + acc[128]) + acc[192])


def fold_loss(rows):
    total = fold(rows)
    return f32(total / float(np.asarray(rows).size))


def record_after(calls):
    """(loss_sum, rows, top1, topk) of a zeroed record after the calls [(rows fp32 [B], hit1 [B], hitk [B]), ...]."""
    ls, n, h1, hk = 0.0, 0, 0, 0
    for rows, a, b in calls:
        with np.errstate(invalid="ignore"):
            ls = ls + fold(rows)
        n += int(np.asarray(rows).size)
        h1 += int(np.sum(a))
        hk += int(np.sum(b))
    return ls, n, h1, hk


# ------------------------------------------------------------------------------------------- xent: emulation
def _butterfly(x):
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lane ^ o]
    return x[:, 0]


def emulate_xent(z32, label_a=None, label_b=None, lam=None, soft=None, smoothing=0.0, W=1, mut=None):
    """The kernel's arithmetic in float32 (numpy's expf / logf): {'row': [B], 'loss': [1], 'dl': [B, C]}.
    mut: no_rescale (the sum is not rescaled when a lane's max rises), nan_drop (a NaN met before the lane's first
    finite element is dropped, and so is a lane that met none), sumq_one (sum(q) taken as 1), unif_noS (the uniform
    part without S), wb_lam (wb = lam), no_invB."""
    z = np.asarray(z32, f32)
    B, C = z.shape
    one, eps = f32(1), f32(smoothing)
    n = cdiv(C, 64 * W)
    zl = _lanes(z, C, W, NEG)
    present = (np.arange(n * 64 * W) < C).reshape(n, 64, W)
    dense = soft is not None
    if dense:
        tl = _lanes(np.asarray(soft, f32), C, W, f32(0))
    m = np.full((B, 64), NEG)
    s = np.zeros((B, 64), f32)
    sz, st, stz = np.zeros((B, 64), f32), np.zeros((B, 64), f32), np.zeros((B, 64), f32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for i in range(n):
            v = zl[:, i]                                              # [B, 64, W]
            act = present[i, :, 0][None, :]
            vm = np.fmax.reduce(v, axis=2)
            up = (vm > m) & act
            if mut != "no_rescale":
                s = np.where(up, s * np.exp(m - vm), s)
            m = np.where(up, vm, m)
            fin = (m != NEG) & act
            for j in range(W):
                x = v[:, :, j]
                s = np.where(fin, s + np.exp(x - m), s)
                if mut != "nan_drop":
                    s = np.where(~fin & act & np.isnan(x), x, s)
                pj = present[i, :, j][None, :]
                sz = np.where(pj, sz + x, sz)
                if dense:
                    t = tl[:, i, :, j]
                    st = np.where(pj, st + t, st)
                    stz = np.where(pj & (t != 0), stz + t * x, stz)
        M = m.max(1)
        part = s * np.exp(m - M[:, None])
        empty = np.zeros_like(s) if mut == "nan_drop" else s
        se = _butterfly(np.where(m == NEG, empty, part).astype(f32))
        lse = (M + np.log(se)).astype(f32)
        ia = np.full(B, -1) if label_a is None else np.where((label_a >= 0) & (label_a < C), label_a, -1)
        ib = np.full(B, -1)
        rows = np.arange(B)
        cls = np.arange(C)[None, :]
        if dense:
            S = one + f32(0) * _butterfly(st) if mut == "sumq_one" else _butterfly(st)
            dot = _butterfly(stz)
            t = np.asarray(soft, f32)
        else:
            wa = np.ones(B, f32) if lam is None else np.asarray(lam, f32)
            wb = np.zeros(B, f32)
            if lam is not None:
                wb = wa.copy() if mut == "wb_lam" else (one - wa).astype(f32)
                ib = np.where((label_b >= 0) & (label_b < C), label_b, -1)
            S = (wa + wb).astype(f32) if lam is not None else np.ones(B, f32)
            if mut == "sumq_one":
                S = np.ones(B, f32)
            za = np.where(ia >= 0, z[rows, np.maximum(ia, 0)], f32(0))
            zb = np.where(ib >= 0, z[rows, np.maximum(ib, 0)], f32(0))
            dot = np.zeros(B, f32)
            dot = np.where((ia >= 0) & (wa != 0), dot + wa * za, dot).astype(f32)
            dot = np.where((ib >= 0) & (wb != 0), dot + wb * zb, dot).astype(f32)
            t = (np.where(cls == ia[:, None], wa[:, None], f32(0)) + np.where(cls == ib[:, None], wb[:, None], f32(0))).astype(f32)
        S = S.astype(f32)
        keep = one - eps
        unif = np.zeros(B, f32)
        if eps > 0:
            unif = (eps / f32(C) + f32(0) * S if mut == "unif_noS" else eps * S / f32(C)).astype(f32)
        qz = (keep * dot).astype(f32)
        if eps > 0:
            qz = (qz + unif * _butterfly(sz)).astype(f32)
        row = ((lse * S).astype(f32) - qz).astype(f32)
        inv = (one / se).astype(f32)
        q = ((keep * t).astype(f32) + unif[:, None]).astype(f32) if eps > 0 else t
        invB = one if mut == "no_invB" else one / f32(B)
        pS = ((np.exp(z - M[:, None]) * inv[:, None]).astype(f32) * S[:, None]).astype(f32)
        dl = ((pS - q).astype(f32) * invB).astype(f32)
    return {"row": row, "loss": np.array([fold_loss(row)], f32), "dl": dl}


# ------------------------------------------------------------------------------------------- mix
def mix_tables(H, W, B=MIX_B):
    """[(name, perm int32 [B], lam fp32 [B], box int32 [B, 4])]: every box kind crossed with the lams and perms so
    that each sample of a table differs.  Boxes are (y0, y1, x0, x1)."""
    gw = W // 4 if W % 4 == 0 else W                     # groups per row of the path W selects
    rows_per_chunk = max(MIX_GROUPS_PER_CHUNK // gw, 1)
    boxes = {
        "empty": (2, 2, 0, W), "full": (0, H, 0, W), "clamped": (-5, H + 9, -3, W + 7), "inverted": (H, 0, W, 0),
        "pixel": (H // 2, H // 2 + 1, W // 2, W // 2 + 1), "unaligned": (0, H, 1, max(W - 1, 2)),
        "second_chunk": (rows_per_chunk, min(2 * rows_per_chunk, H), 0, W),
        "across_chunks": (max(rows_per_chunk - 1, 0), rows_per_chunk + 2, 1, W),
        "outside": (-7, 0, -4, 0),
    }
    if H == 1:                                           # a one-row plane: the chunks split the row itself
        per = MIX_GROUPS_PER_CHUNK * (4 if W % 4 == 0 else 1)
        boxes["second_chunk"] = (0, 1, per + 3, min(2 * per - 5, W))
        boxes["across_chunks"] = (0, 1, max(per - 6, 0), per + 6)
    out = []
    names = list(MIX_BOXES)
    for k in range(0, len(names), B):
        for pk, pname in enumerate(MIX_PERMS):
            grp = [names[(k + j) % len(names)] for j in range(B)]
            perm = {"identity": np.arange(B), "roll": np.roll(np.arange(B), 1), "outside": np.array([B, -1, B + 5][:B])}[pname]
            lam = np.array([MIX_LAMS[(j + pk + k) % 3] for j in range(B)], f32)
            box = np.array([boxes[g] for g in grp], np.int32)
            out.append((f"{'+'.join(grp)} {pname}", perm.astype(np.int32), lam, box))
    return out


def mix_copy_table(B=MIX_B):
    """lam 1 with an empty box, one box wholly outside the image (it clamps to empty): copies whose partner, a NaN
    plane, is not read."""
    perm = np.roll(np.arange(B), 1).astype(np.int32)
    lam = np.ones(B, f32)
    box = np.array([(2, 2, 0, 9), (-7, 0, -4, 0), (5, 1, 0, 9)][:B], np.int32)
    return perm, lam, box


def mix_image(B, C, H, W, nan_sample=None):
    img = rng_of("mix", B, C, H, W).standard_normal((B, C, H, W)).astype(f32) * 3
    if nan_sample is not None:
        img[nan_sample] = np.nan
    return img


def mix(img, perm, lam, box):
    return ref_loss.mix(img, perm, lam, box)


def emulate_mix(img, perm, lam, box, vec, fill, mut=None):
    """The kernel block by block: blockIdx -> (plane, chunk), 1024 groups of W4 elements per chunk, four per thread.
    ``fill`` is what the output held before.  mut: fma (one rounding), box_off1 (y <= y1), box_unclamped,
    plane_chunk (the split swapped), u0_only (each thread serves its first group alone)."""
    img = np.asarray(img, f32)
    B, C, H, W = img.shape
    W4 = 4 if vec else 1
    hw = H * W
    groups = hw // W4
    chunks = cdiv(groups, MIX_GROUPS_PER_CHUNK)
    planes = B * C
    flat = img.reshape(planes, hw)
    out = np.full((planes, hw), fill, f32)
    for bid in range(planes * chunks):
        plane, chunk = divmod(bid, chunks)
        if mut == "plane_chunk":
            chunk, plane = divmod(bid, chunks)
            if plane >= planes:
                continue
        b = plane // C
        pb = int(perm[b]) if 0 <= int(perm[b]) < B else b
        l = f32(lam[b])
        oml = f32(1) - l
        clip = (lambda v, hi: int(v)) if mut == "box_unclamped" else (lambda v, hi: int(min(max(int(v), 0), hi)))
        y0, y1, x0, x1 = clip(box[b][0], H), clip(box[b][1], H), clip(box[b][2], W), clip(box[b][3], W)
        empty = y0 >= y1 or x0 >= x1
        copy = empty and l == f32(1)
        g_lo = chunk * MIX_GROUPS_PER_CHUNK
        g_hi = min(g_lo + (256 if mut == "u0_only" else MIX_GROUPS_PER_CHUNK), groups)
        if g_lo >= g_hi:
            continue
        e = np.arange(g_lo * W4, g_hi * W4)
        a = flat[plane, e]
        if copy:
            out[plane, e] = a
            continue
        q = flat[pb * C + (plane - b * C), e]
        y, x = e // W, e % W
        inside = (not empty) & (y >= y0) & ((y <= y1) if mut == "box_off1" else (y < y1)) & (x >= x0) & (x < x1)
        with np.errstate(invalid="ignore", over="ignore"):
            if mut == "fma":
                mixed = (l.astype(f64) * a.astype(f64) + (oml * q).astype(f32).astype(f64)).astype(f32)
            else:
                mixed = ((l * a).astype(f32) + (oml * q).astype(f32)).astype(f32)
        out[plane, e] = np.where(inside, q, mixed)
    return out.reshape(B, C, H, W)


# ------------------------------------------------------------------------------------------- sls
def sls_frames(kind, n, H, W, seed=0):
    """uint8 [n, H, W, 3]."""
    if kind == "zeros":
        return np.zeros((n, H, W, 3), np.uint8)
    if kind == "full":
        return np.full((n, H, W, 3), 255, np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        c = (((yy + xx) % 2) * 255).astype(np.uint8)
        f = np.stack([c, 255 - c, c], -1)
        return np.stack([f if i % 2 == 0 else 255 - f for i in range(n)])
    assert kind == "random", kind
    return rng_of("sls", n, H, W, seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def sls_walk_frames(n, H, W):
    """Frame i = base[i % 7] + i (mod 256): a wrong frame index shows."""
    base = sls_frames("random", 7, H, W, 1)
    return np.stack([(base[i % 7].astype(np.int64) + i).astype(np.uint8) for i in range(n)])


def sls_pack(frames, pitched):
    """(flat uint8 buffer, img_bytes, row_bytes): dense, or pitched with row_bytes = 3 W + 5 and img_bytes =
    row_bytes H + 11, 0xFF in every gap (and 16 bytes of it behind the last frame)."""
    n, H, W, _ = frames.shape
    rb = 3 * W + (5 if pitched else 0)
    ib = rb * H + (11 if pitched else 0)
    buf = np.full(n * ib + 16, 0xFF, np.uint8)
    for i in range(n):
        for y in range(H):
            o = i * ib + y * rb
            buf[o:o + 3 * W] = frames[i, y].reshape(-1)
    return buf, ib, rb


def sls_image(buf, n, H, W, img_bytes, row_bytes, bgr, Ho, Wo, mut=None, first=0):
    """fp32 [n, Ho, Wo] from the flat bytes: oracle/sls_ref.py's resize -> gray -> / 255.0, indexed through
    img_bytes / row_bytes as the kernel does.  mut: no_round (without the + 2), no_shift4 (without >> 4),
    swap_br, x1_unclamped."""
    xo, xw = sls_ref.resize_coeffs(W, Wo)
    yo, yw = sls_ref.resize_coeffs(H, Ho)
    x1 = xo + 1 if mut == "x1_unclamped" else np.minimum(xo + 1, W - 1)
    y1 = np.minimum(yo + 1, H - 1)
    src = np.asarray(buf, np.uint8).astype(np.int64)
    c = np.arange(3)[None, None, :]
    out = np.empty((n, Ho, Wo), f32)
    for i in range(n):
        base = (first + i) * img_bytes
        r0 = (base + yo * row_bytes)[:, None, None]
        r1 = (base + y1 * row_bytes)[:, None, None]
        a0, a1 = xw[None, :, 0, None], xw[None, :, 1, None]
        px0, px1 = (xo * 3)[None, :, None] + c, (x1 * 3)[None, :, None] + c
        h0 = src[r0 + px0] * a0 + src[r0 + px1] * a1
        h1 = src[r1 + px0] * a0 + src[r1 + px1] * a1
        b0, b1 = yw[:, 0, None, None], yw[:, 1, None, None]
        if mut == "no_shift4":
            v = ((h0 * b0) >> 16) + ((h1 * b1) >> 16)
        else:
            v = (((h0 >> 4) * b0) >> 16) + (((h1 >> 4) * b1) >> 16)
        ch = np.clip((v + (0 if mut == "no_round" else 2)) >> 2, 0, 255)
        blue, red = (ch[..., 0], ch[..., 2]) if bool(bgr) != (mut == "swap_br") else (ch[..., 2], ch[..., 0])
        gray = (blue * 1868 + ch[..., 1] * 9617 + red * 4899 + (1 << 13)) >> 14
        out[i] = (gray / 255.0).astype(f32)
    return out


def one_trip(out, fill, items, mut):
    """mut 'one_trip': what a launch leaves when only the first trip of its capped grid is served."""
    if mut == "one_trip" and items > SLS_GRID_ITEMS:
        out.reshape(-1)[SLS_GRID_ITEMS * (out.size // items):] = fill
    return out


# ------------------------------------------------------------------------------------------- gather
def gather_src(n_src, row_bytes):
    return rng_of("gather", n_src, row_bytes).integers(1, 256, (n_src, row_bytes), dtype=np.uint8)   # no zero byte


def gather_idx(n, n_src, bad=True):
    """int64 [n]: repeats, and (bad) -1, n_src, INT64_MIN, INT64_MAX among them: those give zero rows."""
    idx = rng_of("gidx", n, n_src).integers(0, n_src, n).astype(np.int64)
    if n > 1:
        idx[1] = idx[0]
    if bad:
        for k, v in zip(range(2, n, max(n // 5, 1)), (-1, n_src, I64_MIN, I64_MAX)):
            idx[k] = v
    return idx


def gather_rows(src, idx, mut=None):
    """uint8 [n, row_bytes].  mut no_zero_row: a bad index is clamped into the table instead."""
    n_src = src.shape[0]
    ok = (idx >= 0) & (idx < n_src)
    out = src[np.clip(idx, 0, n_src - 1)]
    if mut != "no_zero_row":
        out = np.where(ok[:, None], out, np.uint8(0))
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------- patch_keep
def keep_slot(seed, site, B, np_, K, mut=None):
    """(keep int32 [B, K] ascending, slot int32 [B, np]): the K smallest (key, p) pairs of each sample (a stable
    argsort: see the header for why the tie order is stated and not tested).  mut: pad_zero (the padding keys up to
    a multiple of 4 rank in front of every patch), chunk_base (the position restarts in every chunk of 256)."""
    keys = vit_ref.dropout_hash(seed, site, np.arange(B), np.arange(np_))
    rank = np.argsort(np.argsort(keys, axis=1, kind="stable"), axis=1, kind="stable")
    if mut == "pad_zero":
        rank = rank + (-np_) % 4
    kept = rank < K
    keep = np.full((B, K), -1, np.int32)
    slot = np.full((B, np_), -1, np.int32)
    for b in range(B):
        p = np.flatnonzero(kept[b])
        j = np.arange(p.size)
        if mut == "chunk_base":
            j = np.array([int(kept[b, (q // 256) * 256:q].sum()) for q in p], dtype=np.int64)
        slot[b, p] = j
        keep[b, j] = p
    return keep, slot


def keep_slot_ref(seed, B, np_, K):
    """The same through tests/ref_patchdrop.py (site PATCH_SITE)."""
    keep = ref_patchdrop.keep_indices(seed, B, np_, K)
    return keep.astype(np.int32), ref_patchdrop.slot_indices(keep, np_).astype(np.int32)
