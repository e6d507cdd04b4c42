"""NumPy restatement of the classification recipe's formulas (include/vitmi.h, the
vitmi_softmax_xent / vitmi_mix_batch block): the loss and its gradient in fp64, the exact top-k
rule on the fp32 logits, and the float32 evaluation of the image mix.  A helper of the tests, not
a test module."""
import numpy as np

f32, f64 = np.float32, np.float64


def target_dist(B, C, label_a=None, label_b=None, lam=None, soft=None):
    """(t [B, C] fp64, S [B] fp64 = sum(t)).  A label outside [0, C) matches no class but keeps its
    weight in S."""
    if soft is not None:
        t = np.asarray(soft, f32).astype(f64)
        return t, t.sum(1)
    t = np.zeros((B, C), f64)
    la = np.asarray(label_a, np.int64)
    wa = np.ones(B, f64) if lam is None else np.asarray(lam, f32).astype(f64)
    wb = np.zeros(B, f64) if lam is None else 1.0 - wa
    for b in range(B):
        if 0 <= la[b] < C:
            t[b, la[b]] += wa[b]
        if lam is not None and 0 <= int(label_b[b]) < C:
            t[b, int(label_b[b])] += wb[b]
    return t, wa + wb


def xent(z32, label_a=None, label_b=None, lam=None, soft=None, smoothing=0.0):
    """(row_loss [B], loss, dlogits [B, C]) in fp64 from the fp32 logits."""
    z = np.asarray(z32, f32).astype(f64)
    B, C = z.shape
    t, S = target_dist(B, C, label_a, label_b, lam, soft)
    q = (1.0 - smoothing) * t + smoothing * S[:, None] / C if smoothing > 0 else t
    m = z.max(1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = np.exp(z - m)
        se = e.sum(1, keepdims=True)
        lse = (m + np.log(se))[:, 0]
        qz = np.where(q != 0, q * np.where(q != 0, z, 0.0), 0.0).sum(1)
        row = lse * S - qz
        dl = (e / se * S[:, None] - q) / B
    return row, row.sum() / B, dl


def hits(z32, labels, k):
    """bool [B]: row b is a top-k hit iff #{c : z_c > z_y or (z_c == z_y and c < y)} < k; a NaN at
    the label or a label outside [0, C) is a miss."""
    z = np.asarray(z32, f32)
    B, C = z.shape
    out = np.zeros(B, bool)
    cls = np.arange(C)
    for b in range(B):
        y = int(labels[b])
        if not 0 <= y < C or np.isnan(z[b, y]):
            continue
        with np.errstate(invalid="ignore"):
            ahead = (z[b] > z[b, y]) | ((z[b] == z[b, y]) & (cls < y))
        out[b] = int(ahead.sum()) < k
    return out


def mix(img, perm, lam, box):
    """float32 evaluation of vitmi_mix_batch: 1 - lam once, two rounded products, one addition."""
    img = np.asarray(img, f32)
    B, C, H, W = img.shape
    out = np.empty_like(img)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    for b in range(B):
        pb = int(perm[b]) if 0 <= int(perm[b]) < B else b
        y0, y1 = (int(np.clip(v, 0, H)) for v in box[b][:2])
        x0, x1 = (int(np.clip(v, 0, W)) for v in box[b][2:])
        inside = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
        l = f32(lam[b])
        if l == f32(1) and not inside.any():
            out[b] = img[b]                      # a copy: the partner is not read
            continue
        oml = f32(1) - l
        with np.errstate(invalid="ignore"):
            mixed = (l * img[b]).astype(f32) + (oml * img[pb]).astype(f32)
        out[b] = np.where(inside[None], img[pb], mixed.astype(f32))
    return out
