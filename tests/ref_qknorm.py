"""Float64 reference of QK-norm (include/vitmi.h, "QK-norm": vitmi_qknorm_fwd, _bwd) with per-element
bounds, its input families, a CPU emulation of the kernels' arithmetic with mutants, and the model-level
reference (oracle/vit_ref.py's pieces with the norm inserted, gradients by autograd) with a bf16
emulation of it.  Plain torch on the CPU, no GPU.  TEST INFRASTRUCTURE ONLY.

Kernel level.  The q and k blocks of qkv [M, 3*H*64] are viewed as [M*H, 64] rows (row m*H + h is head h
of token m) and given to tests/ref_layernorm.py's ``forward`` / ``backward``, whose derived bounds then
hold as they stand: the D = 64 row sums in any order, the bf16 store term for a bf16 buffer (``y_bf16``,
``dx_lp``: the kernels round once to the buffer's dtype), dgamma / dbeta over M*H rows.  The qkv bias
gradient is a column sum over the M token rows of what the backward STORED, so its bound is
ref_layernorm's dxsum bound with M rows per column: (M + 1) u sum_m |dx| + sum_m tol_dx + u (|prev| +
|ref|); the v columns are plain column sums of the given gradient (ref_layernorm.colsum).  Inputs are
taken as stored: for a bf16 buffer they are rounded to bf16 first and are exact from there on.

Families (ref_layernorm's, per [M*H, 64] view, so neighbouring HEADS differ in the 'rows' family):
randn, rows, offset, const (rows 1, M*H // 2, M*H - 1 of the view hold 3.25: out == beta BITWISE) and
int (dy, dv and every prev are small integers: dbeta and the v columns of dbias are exact sums in any
order, compared BITWISE; the q and k columns of dbias sum rounded non-integers and keep their bound).

Norm parameters of the tests (``norm_params``): weight magnitudes uniform in [0.5, 1.5], a quarter of
them negative, channel 3 exactly 0; bias = 0.2 randn.

Model level.  ``block`` / ``forward`` / ``forward_backward`` restate vit_ref's block with timm's QK-norm
(``blocks.i.attn.q_norm`` / ``k_norm``, LayerNorm over each head's 64 columns, epsilon cfg.ln_eps)
between the qkv projection and QK^T, and take LayerScale gammas, dropout and drop path as
tests/ref_layerscale.py does.  With cfg.qk_norm False the operations are vit_ref's own, bit for bit.
``emulate=True`` is the bf16 device path in emulation: the GEMM operands (activations, weights and, in
the backward, the incoming gradients), the qkv output, the normalised q and k, the softmax P and the
attention output o are rounded to bf16, forward and backward (round-to-nearest; a gradient is rounded
where the device path holds it in bf16), everything else fp32.  The attention core's backward is
restated as csrc/attention.hip computes it (``_AttnCore``): delta = rowsum(dO o) from the STORED bf16 o,
dP - delta in fp32, dS rounded to bf16.  That term is the largest one in dq and dk, and with them in the
norm parameters' gradients; rounding values and gradients alone misses it (1.0e-2 instead of 1.9e-2 for
blocks.0.attn.k_norm.weight on the GPU test's model).  The emulation's distance from the fp32 reference
is what a bf16 path costs on these inputs; the GPU test derives its low-precision bound from it."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

import ref_droppath
import ref_gemm as rg
import ref_layernorm as rl
from oracle import vit_ref
from ref_gemm import BF, U32, UBF, guards_intact, padded, worst_ratio  # noqa: F401

F32 = torch.float32
DH = 64
ZERO_CHANNEL = 3
FAMILIES = rl.FAMILIES
EPS = rl.EPS
GRID_CAP = 1024          # csrc/qknorm.hip QK_BLOCKS


# --------------------------------------------------------------------------- launch geometry
def rows_per_pass(M, H, bf16):
    """R of csrc/qknorm.hip's qk_geom: the rows one pass of the grid covers (a thread walks rows r,
    r + R, ...).  M > R makes every grid-stride loop walk."""
    import math
    S = 3 * H * (8 if bf16 else 16)
    unit = S // math.gcd(S, 256)
    need = -(-M * S // 256)                     # blocks that cover every row once
    k = min(max(-(-need // unit), 1), max(GRID_CAP // unit, 1))
    return unit * k * 256 // S


def workspace_bytes(M, H):
    """vitmi_qknorm_bwd_workspace_size: the larger of the two dtypes' partial sets."""
    def one(bf16):
        R = rows_per_pass(M, H, bf16)
        G = R * 3 * H * (8 if bf16 else 16) // 256
        return 4 * (R * 3 * H * DH + 4 * G * DH)
    return max(one(True), one(False))


# --------------------------------------------------------------------------- inputs
def norm_vec(seed):
    g = torch.Generator().manual_seed(seed)
    w = (0.5 + torch.rand(DH, generator=g)) * torch.where(torch.rand(DH, generator=g) < 0.25, -1.0, 1.0)
    w[ZERO_CHANNEL] = 0.0
    return w.float().contiguous(), (0.2 * torch.randn(DH, generator=g)).float().contiguous()


def norm_params(seed=3):
    """(gamma_q, beta_q, gamma_k, beta_k), fp32 [64]."""
    return norm_vec(seed) + norm_vec(seed + 1)


def model_norm_params(cfg, seed=3):
    """{blocks.i.attn.q_norm.weight, .bias, k_norm.weight, .bias} of every block."""
    out = {}
    for i in range(cfg.depth):
        for j, n in enumerate(("q_norm", "k_norm")):
            w, b = norm_vec(seed + 2 * i + j)
            out[f"blocks.{i}.attn.{n}.weight"], out[f"blocks.{i}.attn.{n}.bias"] = w, b
    return out


def norm_names(cfg):
    return [f"blocks.{i}.attn.{n}.{leaf}" for i in range(cfg.depth) for n in ("q_norm", "k_norm")
            for leaf in ("weight", "bias")]


@functools.lru_cache(maxsize=None)
def inputs(family, M, H, bf16, seed=11):
    """{qkv, dqkv [M, 3D] fp32 holding values exact in the buffer dtype, gq, bq, gk, bk, prev: {dgq, dbq,
    dgk, dbk [64], dbias [3D]}}."""
    assert family in FAMILIES
    D = H * DH
    fam = "randn" if family == "int" else family
    iq, ik = rl.inputs(fam, M * H, DH, seed), rl.inputs(fam, M * H, DH, seed + 1)
    g = torch.Generator().manual_seed(seed * 7919 + M * 31 + H)
    v, dv = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    dq, dk = iq["dy"].view(M, D), ik["dy"].view(M, D)
    prev = {k: 0.5 * torch.randn(n, generator=g) for k, n in
            (("dgq", DH), ("dbq", DH), ("dgk", DH), ("dbk", DH), ("dbias", 3 * D))}
    if family == "int":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
        dq, dk, dv = ri(-8, 8, M, D), ri(-8, 8, M, D), ri(-8, 8, M, D)
        prev = {k: ri(-4, 4, p.numel()) for k, p in prev.items()}
    qkv = torch.cat([iq["x"].view(M, D), ik["x"].view(M, D), v], 1)
    dqkv = torch.cat([dq, dk, dv], 1)
    if bf16:
        qkv, dqkv = qkv.to(BF).float(), dqkv.to(BF).float()
    gq, bq, gk, bk = norm_params(seed)
    return dict(qkv=qkv.contiguous(), dqkv=dqkv.contiguous(), gq=gq, bq=bq, gk=gk, bk=bk, prev=prev)


def const_heads(M, H):
    """(row of the [M*H, 64] view) of the const family's constant heads."""
    return rl.const_rows(M * H)


# --------------------------------------------------------------------------- float64 reference
@functools.lru_cache(maxsize=None)
def reference(family, M, H, bf16, eps=EPS, seed=11):
    """(inp, ref): ref maps out [M, 2D] (the q | k blocks), mean, rstd [M, 2H], dqk [M, 2D], dgq, dbq, dgk,
    dbk [64], dbias [3D] to (ref, tol) in float64, and mean_in / rstd_in to the fp32 statistics [M, 2H]
    the backward is fed."""
    inp = inputs(family, M, H, bf16, seed)
    D = H * DH
    ref, halves = {}, []
    for blk, (g, b, kg, kb) in enumerate((("gq", "bq", "dgq", "dbq"), ("gk", "bk", "dgk", "dbk"))):
        x = inp["qkv"][:, blk * D:(blk + 1) * D].reshape(M * H, DH)
        dy = inp["dqkv"][:, blk * D:(blk + 1) * D].reshape(M * H, DH)
        fwd = rl.forward(x, inp[g], inp[b], eps)
        prev = torch.stack([inp["prev"][kg], inp["prev"][kb], torch.zeros(DH)])
        bwd = rl.backward(x, fwd["mean_in"], fwd["rstd_in"], inp[g], dy, None, prev)
        ref[kg], ref[kb] = bwd["dgamma"], bwd["dbeta"]
        halves.append((fwd, bwd))

    def cat(pick, shape):
        parts = [pick(f, b) for f, b in halves]
        return tuple(torch.cat([p[i].reshape(M, shape) for p in parts], 1) for i in (0, 1))
    ref["out"] = cat(lambda f, b: f["y_bf16" if bf16 else "y"], D)
    ref["mean"] = cat(lambda f, b: f["mean"], H)
    ref["rstd"] = cat(lambda f, b: f["rstd"], H)
    ref["dqk"] = cat(lambda f, b: b["dx_lp" if bf16 else "dx"], D)
    ref["mean_in"] = torch.cat([f["mean_in"].view(M, H) for f, _ in halves], 1).contiguous()
    ref["rstd_in"] = torch.cat([f["rstd_in"].view(M, H) for f, _ in halves], 1).contiguous()
    # the bias gradient: column sums over the M token rows of the stored q / k gradient, and of v as given
    dx, t_dx = ref["dqk"]
    P = inp["prev"]["dbias"].double()
    qk_ref = P[:2 * D] + dx.sum(0)
    qk_tol = (M + 1) * U32 * dx.abs().sum(0) + t_dx.sum(0) + U32 * (P[:2 * D].abs() + qk_ref.abs())
    v_ref, v_tol = rl.colsum(inp["dqkv"][:, 2 * D:], inp["prev"]["dbias"][2 * D:])
    ref["dbias"] = (torch.cat([qk_ref, v_ref]), torch.cat([qk_tol, v_tol]))
    return inp, ref


# --------------------------------------------------------------------------- CPU emulation
def _store(t, bf16, trunc=False):
    if not bf16:
        return t.float()
    return (rg.bf16_trunc(t) if trunc else rg.bf16_rne(t)).float()


def emulate_fwd(inp, H, bf16, eps=EPS, mut=None):
    """The forward kernel's arithmetic in float32 (two-pass variance, (x - mu) * rs * g + b, one rounding
    to the buffer dtype, v copied).  Returns {out [M, 3D], mean, rstd [M, 2H]}.  Mutants: 'nbrstats' (a
    head normalised with the statistics of the next head), 'trunc' (a truncating bf16 store), 'vnocopy' (the
    v block left as the output buffer's fill, zero), 'kgammaq' (k normalised with q's gamma)."""
    qkv = inp["qkv"].float()
    M, D = qkv.shape[0], H * DH
    e = torch.tensor(rl.f32_eps(eps), dtype=F32)
    outs, means, rstds = [], [], []
    for blk, (g, b) in enumerate((("gq", "bq"), ("gk", "bk"))):
        x = qkv[:, blk * D:(blk + 1) * D].reshape(M * H, DH)
        gam = inp["gq" if mut == "kgammaq" else g].float()
        mu = x.sum(1, keepdim=True) / DH
        d = x - mu
        rs = torch.rsqrt((d * d).sum(1, keepdim=True) / DH + e)
        mu_u, rs_u = (mu.roll(-1, 0), rs.roll(-1, 0)) if mut == "nbrstats" else (mu, rs)
        y = (x - mu_u) * rs_u * gam + inp[b].float()
        outs.append(_store(y, bf16, mut == "trunc").view(M, D))
        means.append(mu.view(M, H))
        rstds.append(rs.view(M, H))
    v = torch.zeros(M, D) if mut == "vnocopy" else qkv[:, 2 * D:]
    return {"out": torch.cat(outs + [v], 1), "mean": torch.cat(means, 1), "rstd": torch.cat(rstds, 1)}


def emulate_bwd(inp, mean, rstd, H, bf16, mut=None, chunk=32):
    """The backward kernel in float32 from the given statistics [M, 2H]: the row reductions per head,
    the parameter and bias sums in ``chunk``-row partials and then over the partials.  Returns {dqkv
    [M, 3D], dgq, dbq, dgk, dbk, dbias}.  Mutants: 'nbrstats', 'trunc', 'kgammaq' as above, 'droplast' (the
    last token row left out of every sum and not written)."""
    qkv, dqkv = inp["qkv"].float(), inp["dqkv"].float()
    M, D = qkv.shape[0], H * DH
    n = M - 1 if mut == "droplast" else M

    def red(t, prev):
        t = t[:n]
        parts = torch.stack([c.sum(0) for c in t.split(chunk, 0)], 0) if t.shape[0] else torch.zeros(1, t.shape[1])
        return prev.float() + parts.sum(0)
    out, res = [], {}
    for blk, (g, kg, kb) in enumerate((("gq", "dgq", "dbq"), ("gk", "dgk", "dbk"))):
        x = qkv[:, blk * D:(blk + 1) * D].reshape(M * H, DH)
        dy = dqkv[:, blk * D:(blk + 1) * D].reshape(M * H, DH)
        gam = inp["gq" if mut == "kgammaq" else g].float()
        mu = mean[:, blk * H:(blk + 1) * H].float().reshape(M * H, 1)
        rs = rstd[:, blk * H:(blk + 1) * H].float().reshape(M * H, 1)
        if mut == "nbrstats":
            mu, rs = mu.roll(-1, 0), rs.roll(-1, 0)
        xh = (x - mu) * rs
        gy = dy * gam
        c1, c2 = gy.sum(1, keepdim=True) / DH, (gy * xh).sum(1, keepdim=True) / DH
        dx = _store((gy - c1 - xh * c2) * rs, bf16, mut == "trunc")
        dxm = dx.view(M, D).clone()
        if mut == "droplast":
            dxm[M - 1] = dqkv[M - 1, blk * D:(blk + 1) * D]
        out.append(dxm)
        # sums over (row, head): a token row's heads, then the rows
        res[kg] = red((dy * xh).view(M, H, DH).sum(1), inp["prev"][kg])
        res[kb] = red(dy.view(M, H, DH).sum(1), inp["prev"][kb])
    out.append(dqkv[:, 2 * D:])
    res["dqkv"] = torch.cat(out, 1)
    res["dbias"] = red(res["dqkv"], inp["prev"]["dbias"])
    return res


# --------------------------------------------------------------------------- the model reference
class _Round(torch.autograd.Function):
    """bf16 rounding of the value (``fwd``) and / or of the gradient (``bwd``)."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return x.to(BF).to(x.dtype) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.to(BF).to(g.dtype) if ctx.bwd else g), None, None


def _q(x, on):       # a bf16 activation: the value and its gradient are held in bf16
    return _Round.apply(x, True, True) if on else x


def _qf(x, on):      # a bf16 operand copy of an fp32 master (weights): the gradient stays fp32
    return _Round.apply(x, True, False) if on else x


def _qb(x, on):      # an fp32 value whose gradient enters a GEMM as a bf16 operand
    return _Round.apply(x, False, True) if on else x


def _bf(x):
    return x.to(BF).to(x.dtype)


class _AttnCore(torch.autograd.Function):
    """softmax(q k^T scale) v on bf16 q, k, v as the device's attention kernels round it
    (csrc/attention.hip): forward P in fp32, bf16 P into P V, o stored in bf16; backward from the bf16
    dO and the STORED bf16 o: delta = rowsum(dO o), dP - delta in fp32 (the MFMA accumulator), dS = P (dP -
    delta) rounded to bf16 as the operand of dQ = dS K and dK = dS^T Q, dV = bf16(P)^T dO."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1)
        o = _bf(torch.matmul(_bf(p), v))
        ctx.save_for_backward(q, k, v, p, o)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, o = ctx.saved_tensors
        do = _bf(do)
        delta = (do * o).sum(-1, keepdim=True)
        ds = _bf(p * (torch.matmul(do, v.transpose(-1, -2)) - delta))
        dq = torch.matmul(ds, k) * ctx.scale
        dk = torch.matmul(ds.transpose(-1, -2), q) * ctx.scale
        dv = torch.matmul(_bf(p).transpose(-1, -2), do)
        return dq, dk, dv, None


def attention(x, p, pre, cfg, drop=None, emulate=False):
    """vit_ref.attention with QK-norm between the projection and QK^T when cfg.qk_norm."""
    B, N, D = x.shape
    H = cfg.num_heads
    dh = D // H
    e = emulate
    qkv = _q(F.linear(x, _qf(p[pre + "attn.qkv.weight"], e), p.get(pre + "attn.qkv.bias")), e)
    q, k, v = qkv.split(D, dim=-1)
    q = q.reshape(B, N, H, dh).transpose(1, 2)
    k = k.reshape(B, N, H, dh).transpose(1, 2)
    v = v.reshape(B, N, H, dh).transpose(1, 2)
    if getattr(cfg, "qk_norm", False):
        q = _q(F.layer_norm(q, (dh,), p[pre + "attn.q_norm.weight"], p[pre + "attn.q_norm.bias"], cfg.ln_eps), e)
        k = _q(F.layer_norm(k, (dh,), p[pre + "attn.k_norm.weight"], p[pre + "attn.k_norm.bias"], cfg.ln_eps), e)
    scale = cfg.head_dim ** -0.5 if cfg.attn_scale == "head" else cfg.embed_dim ** -0.5
    if e:
        o = _AttnCore.apply(q, k, v, scale).transpose(1, 2).reshape(B, N, D)
    else:
        s = torch.matmul(q, k.transpose(-1, -2)) * scale
        a = torch.softmax(s, dim=-1)
        o = torch.matmul(a, v).transpose(1, 2).reshape(B, N, D)
    out = _qb(F.linear(o, _qf(p[pre + "attn.proj.weight"], e), p[pre + "attn.proj.bias"]), e)
    if drop is not None:
        out = vit_ref.dropout(out, drop[0], drop[1], drop[2])
    return out


def mlp(x, p, pre, drop=None, emulate=False):
    if not emulate:
        return vit_ref.mlp(x, p, pre, drop)
    h = _qb(F.linear(x, _qf(p[pre + "mlp.fc1.weight"], True), p[pre + "mlp.fc1.bias"]), True)
    h = _q(F.gelu(h), True)
    if drop is not None:
        h = vit_ref.dropout(h, drop[0], drop[1], drop[2])
    y = _qb(F.linear(h, _qf(p[pre + "mlp.fc2.weight"], True), p[pre + "mlp.fc2.bias"]), True)
    if drop is not None:
        y = vit_ref.dropout(y, drop[0], drop[1] + 1, drop[2])
    return y


def block(x, p, i, cfg, seed=None, emulate=False):
    """vit_ref.block with QK-norm; LayerScale where p holds the block's gammas, dropout and drop path
    at ``seed`` (tests/ref_layerscale.py's order: dropout -> gamma -> sample factor)."""
    pre = f"blocks.{i}."
    n2 = "norm1" if cfg.tie_norms else "norm2"
    drate = getattr(cfg, "drop_rate", 0.0)
    prate = ref_droppath.rates(getattr(cfg, "drop_path_rate", 0.0), cfg.depth)[i]
    don = seed is not None and drate > 0
    da = (seed, 3 * i, drate) if don else None
    dm = (seed, 3 * i + 1, drate) if don else None
    B = x.shape[0]
    f1 = f2 = None
    if seed is not None and prate > 0:
        f1 = ref_droppath.sample_factor(seed, ref_droppath.PATH_SITE0 + 2 * i, B, prate).view(B, 1, 1)
        f2 = ref_droppath.sample_factor(seed, ref_droppath.PATH_SITE0 + 2 * i + 1, B, prate).view(B, 1, 1)
    a = attention(_q(vit_ref.layer_norm(x, p[pre + "norm1.weight"], p[pre + "norm1.bias"], cfg.ln_eps), emulate),
                  p, pre, cfg, da, emulate)
    if pre + "ls1.gamma" in p:
        a = a * p[pre + "ls1.gamma"]
    x = x + (a if f1 is None else a * f1)
    m = mlp(_q(vit_ref.layer_norm(x, p[pre + n2 + ".weight"], p[pre + n2 + ".bias"], cfg.ln_eps), emulate),
            p, pre, dm, emulate)
    if pre + "ls2.gamma" in p:
        m = m * p[pre + "ls2.gamma"]
    return x + (m if f2 is None else m * f2)


def forward(img, p, cfg, seed=None, emulate=False):
    """Logits; the embedding and the head as vit_ref.forward does them (with ``emulate`` the patch
    embedding's operands are rounded too; the head stays fp32 as on the device)."""
    if emulate:
        p = dict(p)
        p["patch_embed.proj.weight"] = _qf(p["patch_embed.proj.weight"], True)
        img = img.to(BF).to(img.dtype)
    x = _qb(vit_ref.embed(img, p, cfg), emulate)
    for i in range(cfg.depth):
        x = block(x, p, i, cfg, seed, emulate)
    cls = x[:, 0] if cfg.with_cls_token else x.mean(dim=1)
    cls = vit_ref.layer_norm(cls, p["norm.weight"], p["norm.bias"], cfg.ln_eps)
    return F.linear(cls, p["head.weight"], p["head.bias"])


def forward_backward(img, target, p, cfg, seed=None, emulate=False):
    """(logits, loss, {name: grad}) of one CPU step, like vit_ref.forward_backward."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    logits = forward(img, leaves, cfg, seed, emulate)
    loss = vit_ref.loss_fn(logits, target, cfg.num_classes)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad.detach() for k, v in leaves.items()}
