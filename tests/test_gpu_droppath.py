"""Stochastic depth (drop path) on the device against the CPU reference tests/ref_droppath.py: the
fused residual-GEMM epilogues on all three GEMM paths, vitmi_droppath_apply, the model's forward
and backward, the identity / hygiene properties, vitmi.DropPath and the keep statistics."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_droppath as ref  # noqa: E402
import vitmi  # noqa: E402
from oracle import vit_ref  # noqa: E402
from vitmi import ops  # noqa: E402
from vitmi._lib import lib  # noqa: E402
from vitmi.config import ViTConfig  # noqa: E402
from vitmi.modules import Block, VisionTransformer, cross_entropy  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
EPS32 = float(np.finfo(np.float32).eps)

# ------------------------------------------------------------------ the epilogue, all three GEMM paths
S, B, N = 197, 11, 320            # M = 2167: 128- and 256-row tiles straddle sample boundaries
M = S * B
SEED, SITE, P = 7, 0x40000003, 0.25
DSITE, DP = 2, 0.1                # the element dropout of the combined epilogue


def rnd(*shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


@functools.lru_cache(maxsize=None)
def epilogue_masks():
    """(row keep [M] bool, element factor [M, N] float64) of the reference, computed once."""
    keep = ref.keep_mask(SEED, SITE, B, P)
    thresh, dscale = vit_ref.dropout_params(DP)
    ekeep = vit_ref.dropout_hash(SEED, DSITE, np.arange(M), np.arange(N)) >= thresh
    return torch.from_numpy(np.repeat(keep, S)), torch.from_numpy(ekeep.astype(np.float64) * dscale)


def check_epilogue(dtype, policy, K, expect_ws):
    assert ref.mask_string(SEED, SITE, B, P) == "11001010111"
    rows, efac = epilogue_masks()
    pscale = 1.0 / (1.0 - P)
    x = rnd(M, K, seed=1, dtype=dtype).to(DEV)
    w = rnd(N, K, seed=2, scale=0.05, dtype=dtype).to(DEV)
    b, res = rnd(N, seed=3).to(DEV), rnd(M, N, seed=4).to(DEV)
    lib().vitmi_gemm_set_policy(policy)
    try:
        if expect_ws:   # the tail-split fix-up is planned for this shape (8-block persistent grid)
            assert lib().vitmi_linear_fwd_workspace_size(ops.dt(dtype), M, N, K) > 0
        t = ops.linear_fwd(x, w, b, F32)                                        # acc + bias, fp32
        y = ops.linear_fwd(x, w, b, F32, ops.EPI_RESIDUAL, residual=res, droppath=(SEED, SITE, P, S))
        yd = ops.linear_fwd(x, w, b, F32, ops.EPI_RESIDUAL, residual=res, dropout=(SEED, DSITE, DP),
                            droppath=(SEED, SITE, P, S))
        y0 = ops.linear_fwd(x, w, b, F32, ops.EPI_RESIDUAL, residual=res, droppath=(SEED, SITE, 0.0, S))
        plain = ops.linear_fwd(x, w, b, F32, ops.EPI_RESIDUAL, residual=res)
    finally:
        lib().vitmi_gemm_set_policy(0)
    t, y, yd, res = t.cpu().double(), y.cpu(), yd.cpu(), res.cpu()
    assert torch.equal(y0.cpu(), plain.cpu())                                   # rate 0 = the plain epilogue
    # dropped samples: the residual, bit for bit
    assert torch.equal(y[~rows], res[~rows]) and torch.equal(yd[~rows], res[~rows])
    # kept samples: residual + scale * t to fp32 rounding (two roundings and a possible fma contraction)
    for name, got, branch in (("path", y, pscale * t), ("dropout+path", yd, pscale * efac * t)):
        want = res.double() + branch
        err = (got.double() - want).abs()[rows]
        bound = (4 * EPS32 * (res.double().abs() + branch.abs()))[rows]
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{name} {dtype} policy {policy} K {K}: worst |err| / bound = {worst:.3f}")
        assert (err <= bound).all(), f"{name}: worst |err| / bound {worst:.3f}"
    assert (y[rows] != res[rows]).any() and (yd != y).any()                     # both masks act


@pytest.mark.parametrize("policy", [1, 2, 3], ids=["tile128", "tile256", "tile256-persistent8"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_epilogue_on_every_gemm_path(dtype, policy):
    check_epilogue(dtype, policy, 256, expect_ws=policy == 3 and dtype == BF)


def test_epilogue_through_the_tail_split_fixup():
    """The residual epilogues split their tail tiles only from 16 K-steps on (csrc/gemm.hip tail_ok):
    at K = 1024 under policy 3 the last 2 of the 18 tiles really go through the fix-up kernel."""
    check_epilogue(BF, 3, 1024, expect_ws=True)


# ------------------------------------------------------------------ droppath_apply
@pytest.mark.parametrize("out_dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_droppath_apply(out_dtype, strided):
    C = 72
    rows, efac = epilogue_masks()
    efac = efac[:, :C]
    src = rnd(M, C + 8, seed=9).to(DEV)
    x = src[:, :C] if strided else src[:, :C].contiguous()
    y = ops.droppath_apply(x, SEED, SITE, P, S, out_dtype).cpu()
    yd = ops.droppath_apply(x, SEED, SITE, P, S, out_dtype, dropout=(DSITE, DP)).cpu()
    xc = x.cpu()
    zeros = torch.zeros(int((~rows).sum()), C, dtype=out_dtype)
    for got in (y, yd):                      # bitwise zeros (no -0.0) on dropped samples
        assert got.dtype == out_dtype and got.shape == (M, C)
        assert torch.equal(got[~rows].view(torch.int16 if out_dtype == BF else torch.int32),
                           zeros.view(torch.int16 if out_dtype == BF else torch.int32))
    want = (xc / (1.0 - P))[rows]
    wantd = (xc.double() * efac / (1.0 - P)).float()[rows]
    if out_dtype == F32:
        assert torch.allclose(y[rows], want, rtol=1e-6, atol=0)
        assert torch.allclose(yd[rows], wantd, rtol=1e-6, atol=0)
    else:                                    # the fp32 product, rounded once to bf16 (rtol 1e-6 before it)
        for got, w_ in ((y[rows], want), (yd[rows], wantd)):
            lo, hi = (w_ * (1 - 1e-6)).to(BF).float(), (w_ * (1 + 1e-6)).to(BF).float()
            g = got.float()
            assert ((g >= torch.minimum(lo, hi)) & (g <= torch.maximum(lo, hi))).all()
    assert (efac[rows] == 0).any() and (yd[rows] == 0).any()


# ------------------------------------------------------------------ the model against the reference
CFG = dict(img_size=32, patch_size=8, embed_dim=128, depth=3, num_heads=2, num_classes=2)
MB, MSEED = 6, 11


@functools.lru_cache(maxsize=None)
def model_case(drop_rate=0.0):
    """Parameters, batch and the CPU reference step of the model case (computed once per drop_rate)."""
    cfg = ViTConfig(**CFG, dtype="fp32", drop_path_rate=0.5, drop_rate=drop_rate)
    params = vit_ref.init_params(cfg, seed=0)
    img, tgt = vit_ref.synthetic_batch(cfg, MB)
    return params, img, tgt, ref.forward_backward(img, tgt, params, cfg, seed=MSEED)


def step(cfg, params, img, tgt, seed=MSEED, train=True):
    model = VisionTransformer(cfg).cuda()
    model.load_param_dict(params)
    model.drop_seed = seed
    model.train(train)
    logits = model(img.cuda())
    cross_entropy(logits, tgt.cuda()).backward()
    return logits.detach().cpu(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


def test_reference_masks_act():
    r = ref.rates(0.5, 3)
    masks = [ref.mask_string(MSEED, ref.PATH_SITE0 + 2 * i + j, MB, r[i]) for i in (1, 2) for j in (0, 1)]
    assert masks == ["011110", "111010", "101000", "011100"]
    params, img, tgt, (l_ref, _, _) = model_case()
    l0, _, _ = vit_ref.forward_backward(img, tgt, params, ViTConfig(**CFG, dtype="fp32"))
    assert (l_ref - l0).abs().max().item() > 1e-3


# bounds: the project's dropout test (tests/test_gpu_model.py test_dropout_training_matches_oracle)
@pytest.mark.parametrize("dtype,drop_rate,ltol,gtol", [("fp32", 0.0, 1e-4, 1e-4), ("bf16", 0.0, 5e-2, 2e-2),
                                                       ("fp32", 0.1, 1e-4, 1e-4)])
def test_model_matches_reference(dtype, drop_rate, ltol, gtol):
    params, img, tgt, (l_ref, _, g_ref) = model_case(drop_rate)
    cfg = ViTConfig(**CFG, dtype=dtype, drop_path_rate=0.5, drop_rate=drop_rate)
    l, g = step(cfg, params, img, tgt)
    errs = sorted(((vit_ref.rel_err(g[k], g_ref[k]), k) for k in g_ref), reverse=True)
    lerr = vit_ref.rel_err(l, l_ref)
    print(f"drop path {dtype} drop_rate {drop_rate}: logits rel {lerr:.3e}, worst grads {errs[:3]}")
    for k in ("blocks.1.attn.proj.bias", "blocks.2.attn.proj.bias", "blocks.0.mlp.fc2.bias", "blocks.1.mlp.fc2.bias",
              "blocks.2.mlp.fc2.bias"):
        print(f"  {k}: rel {vit_ref.rel_err(g[k], g_ref[k]):.3e}")
    assert set(g) == set(g_ref)
    assert lerr <= ltol, f"logits rel {lerr:.3e}"
    assert errs[0][0] <= gtol, f"grad {errs[0][1]} rel {errs[0][0]:.3e}"


# ------------------------------------------------------------------ identity and hygiene
def test_eval_mode_is_the_rate_0_model():
    params, img, tgt, _ = model_case()
    for dtype in ("fp32", "bf16"):
        l0, g0 = step(ViTConfig(**CFG, dtype=dtype), params, img, tgt, train=False)
        l1, g1 = step(ViTConfig(**CFG, dtype=dtype, drop_path_rate=0.5), params, img, tgt, train=False)
        assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0), dtype


def test_rate_0_is_the_model_without_the_field():
    params, img, tgt, _ = model_case()
    for dtype in ("fp32", "bf16"):
        l0, g0 = step(ViTConfig(**CFG, dtype=dtype), params, img, tgt, seed=None)
        l1, g1 = step(ViTConfig(**CFG, dtype=dtype, drop_path_rate=0.0), params, img, tgt, seed=None)
        assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0), dtype


def test_no_rng_draw_when_nothing_drops():
    params, img, tgt, _ = model_case()
    model = VisionTransformer(ViTConfig(**CFG, dtype="bf16")).cuda().train()
    dropping = VisionTransformer(ViTConfig(**CFG, dtype="bf16", drop_path_rate=0.5)).cuda().train()
    model.load_param_dict(params)
    torch.manual_seed(123)          # (after the constructors: their initialisers draw)
    before = torch.get_rng_state()
    model(img.cuda())
    assert torch.equal(before, torch.get_rng_state())
    # and a model that drops paths draws exactly once per forward
    dropping(img.cuda())
    after = torch.get_rng_state()
    torch.set_rng_state(before)
    torch.randint(0, 2 ** 31 - 1, (1,))
    assert torch.equal(after, torch.get_rng_state())


def test_precision_knob_refuses_drop_path():
    params, img, tgt, _ = model_case()
    model = VisionTransformer(ViTConfig(**CFG, dtype="bf16f8", drop_path_rate=0.5)).cuda().train()
    with pytest.raises(ValueError, match="parity / evaluation knob"):
        model(img.cuda())
    model.eval()
    assert model(img.cuda()).shape == (MB, 2)


def test_same_seed_same_step_bitwise():
    params, img, tgt, _ = model_case()
    cfg = ViTConfig(**CFG, dtype="bf16", drop_path_rate=0.5, drop_rate=0.1)
    l0, g0 = step(cfg, params, img, tgt)
    l1, g1 = step(cfg, params, img, tgt)
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    l2, _ = step(cfg, params, img, tgt, seed=MSEED + 1)
    assert not torch.equal(l0, l2)


def test_user_stacked_block_honours_its_own_rate():
    """A Block outside VisionTransformer drops paths from its own ``drop_path`` / ``drop_seed`` (sites
    0x40000000 and 0x40000001): a sample whose two branches are both dropped leaves the block
    unchanged, and passes its output gradient through unchanged."""
    seed, p, Bb, Ss, D = 3, 0.5, 8, 17, 128
    k1, k2 = ref.keep_mask(seed, ref.PATH_SITE0, Bb, p), ref.keep_mask(seed, ref.PATH_SITE0 + 1, Bb, p)
    gone, both = ~k1 & ~k2, k1 & k2
    assert gone.any() and both.any()
    blk = Block(D, 2, dtype="fp32").cuda().train()
    blk.drop_path, blk.drop_seed = p, seed
    x = rnd(Bb, Ss, D, seed=21).to(DEV).requires_grad_()
    dout = rnd(Bb, Ss, D, seed=22).to(DEV)
    out = blk(x)
    out.backward(dout)
    gone_t, both_t = torch.from_numpy(gone).to(DEV), torch.from_numpy(both).to(DEV)
    assert torch.equal(out[gone_t], x[gone_t]) and torch.equal(x.grad[gone_t], dout[gone_t])
    assert not torch.equal(out[both_t], x[both_t])
    blk.eval()
    assert not torch.equal(blk(x)[gone_t], x[gone_t])


# ------------------------------------------------------------------ vitmi.DropPath
def test_droppath_module():
    seed, site, p = 13, 0x40000007, 0.4
    f = ref.sample_factor(seed, site, 6, p)
    assert 0 < int((f == 0).sum()) < 6
    mod = vitmi.DropPath(p).cuda().train()
    mod.drop_seed, mod.site = seed, site
    for shape in ((6, 5, 64), (6, 64)):
        x = rnd(*shape, seed=31).to(DEV).requires_grad_()
        dy = rnd(*shape, seed=32).to(DEV)
        y = mod(x)
        y.backward(dy)
        fb = f.view(6, *([1] * (len(shape) - 1)))
        assert y.shape == x.shape
        assert torch.allclose(y.detach().cpu(), x.detach().cpu() * fb, rtol=1e-6, atol=0)
        assert torch.allclose(x.grad.cpu(), dy.cpu() * fb, rtol=1e-6, atol=0)
        assert torch.equal(y.detach().cpu()[f == 0], torch.zeros_like(y.detach().cpu()[f == 0]))
    mod.eval()
    x = rnd(6, 5, 64, seed=33).to(DEV)
    assert mod(x) is x
    assert vitmi.DropPath(0.0).cuda().train()(x) is x
    with pytest.raises(ValueError):
        vitmi.DropPath(1.0)


# ------------------------------------------------------------------ statistics
def test_kept_share():
    Bs, p, seed = 4096, 0.1, 5
    keep = ref.keep_mask(seed, ref.PATH_SITE0, Bs, p)
    y = ops.droppath_apply(torch.ones(Bs, 4, device=DEV), seed, ref.PATH_SITE0, p, 1, F32).cpu()
    got = (y[:, 0] != 0).numpy()
    assert np.array_equal(got, keep)
    share = got.mean()
    print(f"kept share {share:.4f}")
    assert abs(share - 0.9) < 0.01 and abs(share - 0.9006) < 5e-5
