"""Which launches one forward + backward of Block / Mlp / Attention / a 2-block VisionTransformer /
the CvT makes, against a table written out here from reading the autograd Functions (vitmi/modules.py
_BlockFn, _MlpFn, _AttentionFn, _EmbedFn, _HeadFn; vitmi/cvt.py _CvTBlockFn, _ConvEmbedFn).  A change
that drops, doubles or moves a launch into another family fails here even where the numbers still
agree with the oracle (a gradient accumulated twice into a zeroed buffer, a cast the handover was
meant to save).

Two counts per case, both exact:

``OPS``: calls of the vitmi.ops wrappers, counted by wrapping them for the run.  ``wgrad_group`` is the
tuple of item counts of the linear_wgrad_group calls; ``linear_wgrad`` / ``gemm`` include the calls
those wrappers make themselves (a row-strided x of linear_wgrad goes through ops.gemm: the precision
knobs' hi parts).

``KERNELS``: launches per kernel family from the library's own statistics (tests/kstats.py), by
substring of the recorded kernel name:
  gemm                 gemm_kernel + gemm256_kernel: every GEMM call is one of them, split or not
  splitk_reduce        splitk_reduce_kernel + splitk_reduce_small_kernel (a split-K weight gradient)
  splitk_reduce_group  the grouped weight gradient's reduction (its GEMM instance is a gemm256_kernel)
  ln_fwd / ln_bwd      ln_fwd_kernel / ln_bwd_kernel
  ln_fwd_small / ln_bwd_small   the D = 64 / 128 kernels (ln_fwd_small_kernel / ln_bwd_small_kernel): every
                       LayerNorm here but the knobs' split-output forward and the CvT's D = 256 ones
  attn_fwd / attn_bwd  bf16 at N = 17: one single-pass backward kernel; fp32: dQ then dK/dV
  cast, droppath_apply, layerscale_fold, layerscale_bwd, fold (fold_kernel, not layerscale_fold_kernel)
What the statistics do not record, and OPS therefore carries: vitmi_dropout_apply.  (The column-sum
kernels of bias_grad are recorded and not tabled here: OPS carries the bias_grad calls.)
At these shapes (M = B N = 51 rows) the library runs a grouped weight gradient one problem at a time
(vitmi_linear_wgrad_group groups from 256 rows on) and no weight gradient splits K (fewer than 4
K-steps), so both reduce families are 0 for the ViT cases and the grouping shows in OPS alone; the
CvT's first stage (768 rows: 12 K-steps, 3 slabs) splits its 6 block weight gradients and its
conv-embed one.

Shapes: tests/test_gpu_modules.py (D = 128, H = 2, N = 17, B = 3); the CvT is the model of
tests/test_gpu_cvt_model.py::test_cvt_dropout_matches_oracle."""
import pytest
import torch

from kstats import kernel_stats
from vitmi import cvt, ops
from vitmi.config import ViTConfig
from vitmi.modules import LP_STATS, Attention, Block, Mlp, VisionTransformer, cross_entropy, mse_loss

pytestmark = pytest.mark.gpu

D, H, N, B = 128, 2, 17, 3

FAMILIES = {
    "gemm": ("gemm_kernel", "gemm256_kernel"),
    "splitk_reduce": ("splitk_reduce_kernel", "splitk_reduce_small_kernel"),
    "splitk_reduce_group": ("splitk_reduce_group_kernel",),
    "ln_fwd": ("ln_fwd_kernel",),
    "ln_bwd": ("ln_bwd_kernel",),
    "ln_fwd_small": ("ln_fwd_small_kernel",),
    "ln_bwd_small": ("ln_bwd_small_kernel",),
    "attn_fwd": ("attn_fwd",),
    "attn_bwd": ("attn_bwd",),
    "cast": ("cast_kernel",),
    "droppath_apply": ("droppath_apply_kernel",),
    "layerscale_fold": ("layerscale_fold_kernel",),
    "layerscale_bwd": ("layerscale_bwd_kernel",),
}
COUNTED_OPS = ("linear_fwd", "linear_dgrad", "linear_wgrad", "bias_grad", "gemm", "layernorm_fwd", "layernorm_bwd",
               "attention_fwd", "attention_fwd_x3", "attention_fwd_f8", "attention_bwd", "cast_bf16", "dropout_apply",
               "droppath_apply", "layerscale_fold", "layerscale_bwd")


class op_calls:
    """Counts the calls of the vitmi.ops wrappers named in COUNTED_OPS (and the item counts of
    linear_wgrad_group) while active."""

    def __enter__(self):
        self.n = {k: 0 for k in COUNTED_OPS}
        self.groups = []
        self._orig = {k: getattr(ops, k) for k in COUNTED_OPS + ("linear_wgrad_group",)}

        def counted(name, fn):
            def call(*a, **kw):
                self.n[name] += 1
                return fn(*a, **kw)
            return call

        def group(items):
            self.groups.append(len([t for t in items if t is not None]))
            return self._orig["linear_wgrad_group"](items)

        for k in COUNTED_OPS:
            setattr(ops, k, counted(k, self._orig[k]))
        ops.linear_wgrad_group = group
        return self

    def __exit__(self, *exc):
        for k, fn in self._orig.items():
            setattr(ops, k, fn)
        return False

    def table(self):
        t = dict(self.n)
        t["attention_fwd"] += t.pop("attention_fwd_x3") + t.pop("attention_fwd_f8")
        t["wgrad_group"] = tuple(self.groups)
        return t


def _kernels(st):
    t = {fam: sum(st.calls(s) for s in subs) for fam, subs in FAMILIES.items()}
    t["fold"] = st.calls("fold_kernel") - st.calls("layerscale_fold_kernel")
    return t


# ----------------------------------------------------------------------------- the cases
def _x(seed=7):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, D, generator=g).cuda().requires_grad_(True), torch.randn(B, N, D, generator=g).cuda()


def _init(mod, seed=5):
    """Seeded values for every parameter (LayerNorm weights near 1, LayerScale gammas kept)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.endswith("gamma"):
                continue
            t = torch.randn(p.shape, generator=g) * 0.05
            p.copy_(t + 1.0 if "norm" in k and k.endswith("weight") else t)
    return mod


def _module_step(mod, *extra):
    """One forward + backward of a standalone module from an upstream torch gradient: the output, the
    input gradient and every parameter gradient."""
    x, gy = _x()
    y = mod(x, *extra)
    y.backward(gy)
    torch.cuda.synchronize()
    out = {"out": y.detach(), "dx": x.grad}
    out.update({k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
    return out


def _block(dtype="bf16", tie=False, drop_rate=0.0, drop_path=0.0, init_values=None, freeze_fc2=False):
    def run():
        blk = _init(Block(D, H, tie_norms=tie, dtype=dtype, init_values=init_values).cuda())
        blk.drop_rate, blk.drop_path, blk.drop_seed = drop_rate, drop_path, 4242
        if freeze_fc2:
            blk.mlp.fc2.weight.requires_grad_(False)
            blk.mlp.fc2.bias.requires_grad_(False)
        return _module_step(blk, 4, 4)
    return run


def _vit():
    cfg = ViTConfig(img_size=32, patch_size=8, embed_dim=D, depth=2, num_heads=H, num_classes=2, dtype="bf16")
    model = VisionTransformer(cfg).cuda()
    model.reset_parameters(seed=1)
    g = torch.Generator().manual_seed(3)
    img = torch.randn(B, cfg.in_chans, 32, 32, generator=g).cuda()
    tgt = torch.randint(0, 2, (B,), generator=g).cuda()
    LP_STATS.update(hit=0, miss=0)
    logits = model(img)
    cross_entropy(logits, tgt).backward()
    torch.cuda.synchronize()
    # the handover: each block's backward took the bf16 gradient copy its consumer wrote
    assert LP_STATS == {"hit": cfg.depth, "miss": 0}, LP_STATS
    out = {"out": logits.detach()}
    out.update({k: p.grad for k, p in model.named_parameters()})
    return out


def _mlp(dtype):
    return lambda: _module_step(_init(Mlp(D, 4 * D, dtype).cuda()))


def _attention(dtype):
    return lambda: _module_step(_init(Attention(D, H, dtype=dtype).cuda()), 4, 4)


def _cvt(drop_rate):
    def run():
        cfg = cvt.CvTConfig(img_size=64, num_classes=1, dtype="bf16", drop_rate=drop_rate, proc_dim=5)
        model = cvt.CvT(cfg).cuda()
        model.reset_parameters(seed=6)
        model.train()
        model.drop_seed = 4242
        g = torch.Generator().manual_seed(8)
        img = torch.randn(B, 1, 64, 64, generator=g).cuda()
        proc, tgt = torch.randn(B, 5, generator=g).cuda(), torch.randn(B, 1, generator=g).cuda()
        logits = model(img, proc)
        mse_loss(logits, tgt).backward()
        torch.cuda.synchronize()
        out = {"out": logits.detach()}
        out.update({k: p.grad for k, p in model.named_parameters()})
        return out
    return run


# ----------------------------------------------------------------------------- the table
def _with(base, **kw):
    return {**base, **kw}


# Block, bf16, standalone (no arena: 4 weight casts; the incoming gradient comes from torch: 1 cast).
# Forward: LN1, qkv, attention, out-proj + residual, LN2, fc1 + GELU, fc2 + residual.  Backward: DGELU
# dgrad (+ fc1 bias sums), fc2 bias column sum, fc2 and fc1 weight gradients (one linear_wgrad each),
# fc1 dgrad, LN2 backward (+ out-proj bias sums), out-proj dgrad, attention backward (+ qkv bias sums),
# qkv dgrad, out-proj + qkv weight gradients (one group of 2), LN1 backward; one fold launch at the end.
BLOCK_OPS = dict(linear_fwd=4, linear_dgrad=4, linear_wgrad=2, wgrad_group=(2,), bias_grad=1, gemm=0,
                 layernorm_fwd=2, layernorm_bwd=2, attention_fwd=1, attention_bwd=1, cast_bf16=5, dropout_apply=0,
                 droppath_apply=0, layerscale_fold=0, layerscale_bwd=0)
BLOCK_K = dict(gemm=12, splitk_reduce=0, splitk_reduce_group=0, ln_fwd=0, ln_bwd=0, ln_fwd_small=2, ln_bwd_small=2,
               attn_fwd=1, attn_bwd=1, cast=5, droppath_apply=0, layerscale_fold=0, layerscale_bwd=0, fold=1)
# masked branches: no cast of the incoming gradient (the mask pass writes the compute dtype), one mask
# pass per branch, and the out-projection's bias sums from a column-sum pass over the masked gradient
MASKED_OPS = _with(BLOCK_OPS, cast_bf16=4, bias_grad=2)
# LayerScale: W_eff / b_eff of the out-projection and fc2 folded in the forward (no cast of those two
# weights), vitmi_layerscale_bwd on each in the backward, after the folds queued so far
LS_OPS = _with(BLOCK_OPS, cast_bf16=3, layerscale_fold=2, layerscale_bwd=2)
LS_K = _with(BLOCK_K, cast=3, layerscale_fold=2, layerscale_bwd=2)
# the precision knobs: split-output LayerNorm forwards (recorded), the bf16 backward on row-strided hi
# parts (the MLP pair's linear_wgrad goes through ops.gemm)
KNOB_OPS = _with(BLOCK_OPS, gemm=2)
KNOB_K = _with(BLOCK_K, ln_fwd=2, ln_fwd_small=0)
# 2-block VisionTransformer: the arena's bf16 shadow is the one cast (no weight casts, and both blocks
# take the handed-over bf16 gradient); the patch GEMM and its weight gradient run inside the
# patch-embedding entry points; head LayerNorm; no bias_grad (each fc2 bias gradient comes out of its
# consumer's LayerNorm backward); one fold launch per backward (head, 2 blocks, patch embedding)
VIT_OPS = dict(linear_fwd=8, linear_dgrad=8, linear_wgrad=4, wgrad_group=(2, 2), bias_grad=0, gemm=0,
               layernorm_fwd=5, layernorm_bwd=5, attention_fwd=2, attention_bwd=2, cast_bf16=1, dropout_apply=0,
               droppath_apply=0, layerscale_fold=0, layerscale_bwd=0)
VIT_K = _with(BLOCK_K, gemm=26, ln_fwd_small=5, ln_bwd_small=5, attn_fwd=2, attn_bwd=2, cast=1, fold=4)
MLP_OPS = dict(linear_fwd=2, linear_dgrad=2, linear_wgrad=2, wgrad_group=(), bias_grad=1, gemm=0, layernorm_fwd=0,
               layernorm_bwd=0, attention_fwd=0, attention_bwd=0, cast_bf16=4, dropout_apply=0, droppath_apply=0,
               layerscale_fold=0, layerscale_bwd=0)
MLP_K = _with(BLOCK_K, gemm=6, ln_fwd_small=0, ln_bwd_small=0, attn_fwd=0, attn_bwd=0, cast=4)
ATTN_OPS = _with(MLP_OPS, attention_fwd=1, attention_bwd=1)
ATTN_K = _with(MLP_K, attn_fwd=1, attn_bwd=1)
# CvT, 3 stages of one block, bf16.  Per stage: conv embed (forward GEMM; backward: cast, weight
# gradient, bias sums, and the dgrad of stages 1 and 2) and the block: LN1, 3 x (dw_bn, weight cast, q/k/v
# ops.gemm), attention, 3 weight casts, out-proj, LN2, fc1, fc2; backward: cast (none under dropout: 2 mask
# passes), DGELU dgrad, fc2 / fc1 / out-proj weight gradients and bias sums (fc1's fused), 2 dgrads, LN2,
# attention, 3 x (dgrad, weight gradient, bias sums), LN1.  Then the LayerNorm before the head.  The block
# backward does not defer its folds: 10 fold launches per block, 1 per conv embed, 1 for the final norm.
# Recorded LayerNorms: the D = 256 ones (stage 2's LN1, LN2 and the final norm).  Attention backward: the
# single-pass kernel holds N <= 224, so stage 0 (N = 256) runs dQ then dK/dV, stages 1 and 2 one kernel.
CVT_OPS = dict(linear_fwd=12, linear_dgrad=20, linear_wgrad=21, wgrad_group=(), bias_grad=18, gemm=9,
               layernorm_fwd=7, layernorm_bwd=7, attention_fwd=3, attention_bwd=3, cast_bf16=24, dropout_apply=0,
               droppath_apply=0, layerscale_fold=0, layerscale_bwd=0)
CVT_K = _with(BLOCK_K, gemm=62, splitk_reduce=7, ln_fwd=3, ln_bwd=3, ln_fwd_small=4, ln_bwd_small=4, attn_fwd=3, attn_bwd=4,
              cast=24, fold=34)

CASES = {
    "block-bf16": (_block(), BLOCK_OPS, BLOCK_K),
    "block-fp32": (_block("fp32"), _with(BLOCK_OPS, cast_bf16=0), _with(BLOCK_K, cast=0, attn_bwd=2)),
    # tied norms: LN1's dgamma / dbeta folds land on LN2's destinations, so the queue is launched between
    "block-tied": (_block(tie=True), BLOCK_OPS, _with(BLOCK_K, fold=2)),
    "block-dropout": (_block(drop_rate=0.1), _with(MASKED_OPS, dropout_apply=2), _with(BLOCK_K, cast=4)),
    "block-droppath": (_block(drop_path=0.1), _with(MASKED_OPS, droppath_apply=2),
                       _with(BLOCK_K, cast=4, droppath_apply=2)),
    "block-dropout-droppath": (_block(drop_rate=0.1, drop_path=0.1), _with(MASKED_OPS, droppath_apply=2),
                               _with(BLOCK_K, cast=4, droppath_apply=2)),
    "block-layerscale": (_block(init_values=1e-4), LS_OPS, LS_K),
    # frozen fc2 under a trainable gamma: dW_eff / db_eff still formed (zeroed temporaries), same launches
    "block-layerscale-frozen-fc2": (_block(init_values=1e-4, freeze_fc2=True), LS_OPS, LS_K),
    "block-bf16x3": (_block("bf16x3"), KNOB_OPS, KNOB_K),
    "block-bf16f8": (_block("bf16f8"), KNOB_OPS, KNOB_K),     # D = 128: the "weight" qkv form
    "vit-2-blocks-bf16": (_vit, VIT_OPS, VIT_K),
    "mlp-bf16": (_mlp("bf16"), MLP_OPS, MLP_K),
    "mlp-fp32": (_mlp("fp32"), _with(MLP_OPS, cast_bf16=0), _with(MLP_K, cast=0)),
    "attention-bf16": (_attention("bf16"), ATTN_OPS, ATTN_K),
    "attention-fp32": (_attention("fp32"), _with(ATTN_OPS, cast_bf16=0), _with(ATTN_K, cast=0, attn_bwd=2)),
    "cvt": (_cvt(0.0), CVT_OPS, CVT_K),
    "cvt-dropout": (_cvt(0.1), _with(CVT_OPS, cast_bf16=21, dropout_apply=6), _with(CVT_K, cast=21)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_block_step_launches(case):
    run, want_ops, want_kernels = CASES[case]
    with kernel_stats() as st, op_calls() as oc:
        run()
    got_ops, got_kernels = oc.table(), _kernels(st)
    print(f"{case}: ops {got_ops}\n{case}: kernels {got_kernels}")
    assert got_ops == want_ops, {k: (got_ops[k], want_ops[k]) for k in want_ops if got_ops[k] != want_ops[k]}
    assert got_kernels == want_kernels, {k: (got_kernels[k], want_kernels[k]) for k in want_kernels
                                         if got_kernels[k] != want_kernels[k]}
