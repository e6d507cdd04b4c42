"""Patch dropout on the device against the CPU reference tests/ref_patchdrop.py: the subset
selection (exact), the gathered patch embedding against the full one and against torch autograd, the
model's forward and backward, the identity / hygiene properties and one pass at real size."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ref_patchdrop as ref  # noqa: E402
import ref_tokens  # noqa: E402
from oracle import vit_ref  # noqa: E402
from vitmi import ops, optim  # noqa: E402
from vitmi.config import ViTConfig  # noqa: E402
from vitmi.modules import VisionTransformer, cross_entropy  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16


# ------------------------------------------------------------------ selection, exact
# one patch; np below, at and just above a wave; np above the block size; K at both extremes
@pytest.mark.parametrize("B,np_,K,seed", [(6, 16, 8, 11), (5, 9, 6, 7), (3, 196, 147, 5), (3, 576, 144, 5),
                                          (2, 1, 1, 3), (2, 64, 63, 9), (2, 65, 1, 9), (2, 1024, 512, 1)])
def test_selection_is_exact(B, np_, K, seed):
    want = ref.keep_indices(seed, B, np_, K)
    keep, slot = ops.patch_keep(B, np_, K, seed)
    assert keep.dtype == torch.int32 and keep.shape == (B, K) and keep.is_cuda
    assert slot.dtype == torch.int32 and slot.shape == (B, np_)
    assert np.array_equal(keep.cpu().numpy(), want)
    assert np.array_equal(slot.cpu().numpy(), ref.slot_indices(want, np_))     # the inverse map
    keep2, slot2 = ops.patch_keep(B, np_, K, seed)
    assert torch.equal(keep, keep2) and torch.equal(slot, slot2)


# ------------------------------------------------------------------ gathered embed against the full embed
ESEED = 5     # at K = np // 2 some patches are kept by no sample of either case (tests/ref_patchdrop.py)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("near_full", [False, True], ids=["half", "all-but-one"])
@pytest.mark.parametrize("B,C,S,P,D", [(3, 3, 32, 8, 128), (2, 1, 64, 16, 192)])
def test_gathered_embed(dtype, near_full, B, C, S, P, D):
    g = torch.Generator().manual_seed(B * S + D)
    img = torch.rand(B, C, S, S, generator=g)
    w = torch.randn(D, C, P, P, generator=g) * 0.05
    b = torch.randn(D, generator=g) * 0.1
    np_ = (S // P) ** 2
    K = np_ - 1 if near_full else np_ // 2
    cls = torch.randn(D, generator=g) * 0.02
    pos = torch.randn(np_ + 1, D, generator=g) * 0.02
    imgd, wd = img.to(DEV), w.reshape(D, -1).to(DEV).to(dtype)
    bd, clsd, posd = b.to(DEV), cls.to(DEV), pos.to(DEV).reshape(-1)
    keep, slot = ops.patch_keep(B, np_, K, ESEED)
    kn = keep.cpu().numpy().astype(np.int64)
    assert np.array_equal(kn, ref.keep_indices(ESEED, B, np_, K))
    x, patches = ops.patch_embed_keep_fwd(imgd, wd, bd, clsd, posd, P, keep, dtype)
    assert x.shape == (B, K + 1, D) and patches.shape == (B * K, C * P * P)
    # the composed kernel-level entry points: bit-identical
    p2 = ops.patch_im2col_keep(imgd, P, keep, dtype)
    conv = ops.linear_fwd(p2, wd, bd, F32)
    x2 = ops.tokens_assemble_keep(conv, np_, keep, clsd, posd)
    assert torch.equal(patches, p2) and torch.equal(x, x2)
    # the kept rows of the full im2col, bit for bit
    full = ops.patch_im2col(imgd, P, dtype).view(B, np_, -1).cpu()
    assert torch.equal(patches.view(B, K, -1).cpu(), full[torch.arange(B)[:, None], torch.from_numpy(kn)])
    # the gathered conv reference (fp32 conv on the operand-rounded weights and pixels)
    wr = wd.float().cpu().reshape(w.shape)
    ir = img.to(dtype).float()

    def gathered(wl, bl, cl, pl):
        r = F.conv2d(ir, wl, bl, stride=P).flatten(2).transpose(1, 2)
        return ref.gather_tokens(torch.cat([cl.expand(B, 1, D), r], 1) + pl, kn)
    want_x = gathered(wr, b, cls, pos)
    tol = 1e-4 if dtype == F32 else 2e-3
    err = (x.cpu() - want_x).abs().max().item()
    print(f"gathered embed {dtype} K {K}/{np_}: |x - ref| max {err:.3e} (bound {tol * max(1.0, want_x.abs().max().item()):.3e})")
    assert err <= tol * max(1.0, want_x.abs().max().item())
    # backward: composite vs pieces, and vs torch autograd of the gathered reference
    dx = torch.randn(B, K + 1, D, generator=g)
    dxd = dx.to(DEV)

    def zeros():
        return [torch.zeros(D, C * P * P, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV),
                torch.zeros((np_ + 1) * D, device=DEV)]
    grads = zeros()
    ops.patch_embed_keep_bwd(dxd, patches, slot, C, S, P, *grads)
    want = zeros()
    lp = None if dtype == F32 else dtype
    dtok, dtok_lp = ops.tokens_assemble_keep_bwd(dxd, slot, dtype == F32, lp, want[2], want[3])
    gg = dtok_lp if dtok_lp is not None else dtok
    ops.linear_wgrad(gg, patches, want[0])
    ops.bias_grad(gg, want[1])
    for a, e in zip(grads, want):
        assert torch.equal(a, e)
    leaves = [t.clone().requires_grad_(True) for t in (wr, b, cls, pos)]
    gathered(*leaves).backward(dx.to(dtype).float() if dtype != F32 else dx)
    gtol = 1e-4 if dtype == F32 else 2e-2
    for name, got, leaf in zip(("dW", "dbias"), grads, leaves):
        ref_g = leaf.grad.reshape(got.shape)
        rel = ((got.cpu() - ref_g).norm() / ref_g.norm()).item()
        print(f"  {name}: rel {rel:.3e} (bound {gtol:.0e})")
        assert (got.cpu() - ref_g).norm() <= gtol * ref_g.norm()
    # dcls, dpos: sums of the fp32 dx over the samples that kept the patch, judged per element
    # (tests/ref_tokens.py: the bound (B + 1) u sum_b|dx|, and the in-order float32 sum bit for bit)
    zero = torch.zeros(np_ + 1, D)
    per = ref_tokens.pos_bwd(dx.reshape(B, -1), zero, zero[0], B, np_, D, ref.slot_indices(kn, np_))
    for name, got, leaf in (("dcls", grads[2], leaves[2]), ("dpos", grads[3], leaves[3])):
        exact, ref_g, tol_g = per[name]
        got = got.cpu().view(exact.shape)
        ratio = ref_tokens.worst_ratio(got, ref_g, tol_g)
        print(f"  {name}: worst |err|/tol {ratio:.3f}")
        assert ratio <= 1.0, name
        assert torch.equal(got, exact), name
        if dtype == F32:               # autograd's own gradient (for bf16 it sums the rounded dx)
            assert ref_tokens.worst_ratio(leaf.grad.reshape(exact.shape), ref_g, tol_g) <= 1.0, name
    # position rows of patches no sample kept: exactly zero
    unkept = np.where((ref.slot_indices(kn, np_) >= 0).sum(axis=0) == 0)[0]
    assert near_full or len(unkept) > 0
    dpos = grads[3].view(np_ + 1, D).cpu()
    assert not dpos[1 + torch.from_numpy(unkept)].any()
    assert dpos[1 + torch.from_numpy(np.unique(kn))].abs().sum(dim=1).gt(0).all()
    # a rerun is bitwise equal
    x3, patches3 = ops.patch_embed_keep_fwd(imgd, wd, bd, clsd, posd, P, keep, dtype)
    again = zeros()
    ops.patch_embed_keep_bwd(dxd, patches3, slot, C, S, P, *again)
    assert torch.equal(x, x3) and torch.equal(patches, patches3)
    for a, e in zip(grads, again):
        assert torch.equal(a, e)


# ------------------------------------------------------------------ the model against the reference
CFG = dict(img_size=32, patch_size=8, embed_dim=128, depth=3, num_heads=2, num_classes=2)
MB, MSEED = 6, 11
VARIANTS = {
    "plain": dict(patch_drop_rate=0.5),
    "droppath+dropout": dict(patch_drop_rate=0.5, drop_path_rate=0.5, drop_rate=0.1),
    "np9-K6": dict(patch_drop_rate=0.3, img_size=24),
    "embed_norm": dict(patch_drop_rate=0.5, embed_norm=True),
}


@functools.lru_cache(maxsize=None)
def model_case(variant, batch=MB):
    """Parameters, batch and the CPU reference step of a variant (computed once each)."""
    cfg = ViTConfig(**{**CFG, **VARIANTS[variant]}, dtype="fp32")
    params = vit_ref.init_params(cfg, seed=0)
    img, tgt = vit_ref.synthetic_batch(cfg, batch)
    return cfg, params, img, tgt, ref.forward_backward(img, tgt, params, cfg, seed=MSEED)


def build(cfg, params, seed=MSEED, train=True):
    model = VisionTransformer(cfg).cuda()
    model.load_param_dict(params)
    model.drop_seed = seed
    model.train(train)
    return model


def step(cfg, params, img, tgt, seed=MSEED, train=True):
    model = build(cfg, params, seed, train)
    logits = model(img.cuda())
    cross_entropy(logits, tgt.cuda()).backward()
    return logits.detach().cpu(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}


# bounds: tests/test_gpu_droppath.py::test_model_matches_reference
@pytest.mark.parametrize("variant,dtype,ltol,gtol", [
    ("plain", "fp32", 1e-4, 1e-4), ("plain", "bf16", 5e-2, 2e-2), ("droppath+dropout", "fp32", 1e-4, 1e-4),
    ("np9-K6", "fp32", 1e-4, 1e-4), ("embed_norm", "fp32", 1e-4, 1e-4)])
def test_model_matches_reference(variant, dtype, ltol, gtol):
    cfg, params, img, tgt, (l_ref, _, g_ref) = model_case(variant)
    # the mask acts: the reference differs from the same model at rate 0
    l0, _, _ = ref.forward_backward(img, tgt, params, cfg.replace(patch_drop_rate=0.0), seed=MSEED)
    assert (l_ref - l0).abs().max().item() > 1e-3
    l, g = step(cfg.replace(dtype=dtype), params, img, tgt)
    errs = sorted(((vit_ref.rel_err(g[k], g_ref[k]), k) for k in g_ref), reverse=True)
    lerr = vit_ref.rel_err(l, l_ref)
    print(f"patch dropout {variant} {dtype}: logits rel {lerr:.3e}, worst grads {errs[:3]}")
    for k in ("pos_embed", "cls_token", "patch_embed.proj.weight", "patch_embed.proj.bias"):
        print(f"  {k}: rel {vit_ref.rel_err(g[k], g_ref[k]):.3e}")
    assert set(g) == set(g_ref)
    assert lerr <= ltol, f"logits rel {lerr:.3e}"
    assert errs[0][0] <= gtol, f"grad {errs[0][1]} rel {errs[0][0]:.3e}"


# ------------------------------------------------------------------ identity and hygiene
def same(a, b):
    return torch.equal(a[0], b[0]) and set(a[1]) == set(b[1]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_inactive_patch_dropout_is_todays_model(dtype):
    _, params, img, tgt, _ = model_case("plain")
    base = ViTConfig(**CFG, dtype=dtype)
    # rate 0.0 is the config without the field
    assert same(step(base, params, img, tgt, seed=None), step(base.replace(patch_drop_rate=0.0), params, img, tgt, seed=None))
    # eval mode at rate 0.5
    assert same(step(base, params, img, tgt, train=False), step(base.replace(patch_drop_rate=0.5), params, img, tgt, train=False))
    # K = np: one patch, rate 0.001 keeps it (training mode)
    one = ViTConfig(**{**CFG, "img_size": 8}, dtype=dtype)
    assert one.num_patches == 1 and one.replace(patch_drop_rate=0.001).kept_patches == 1
    p1 = vit_ref.init_params(one, seed=0)
    i1, t1 = vit_ref.synthetic_batch(one, MB)
    assert same(step(one, p1, i1, t1), step(one.replace(patch_drop_rate=0.001), p1, i1, t1))


def test_rng_draws():
    _, params, img, _, _ = model_case("plain")
    quiet = VisionTransformer(ViTConfig(**CFG, dtype="bf16", patch_drop_rate=0.0)).cuda().train()
    dropping = VisionTransformer(ViTConfig(**CFG, dtype="bf16", patch_drop_rate=0.5)).cuda().train()
    torch.manual_seed(123)          # (after the constructors: their initialisers draw)
    before = torch.get_rng_state()
    quiet(img.cuda())
    assert torch.equal(before, torch.get_rng_state())               # nothing drops: no draw
    dropping.eval()
    dropping(img.cuda())
    assert torch.equal(before, torch.get_rng_state())               # nor in eval
    dropping.train()
    dropping(img.cuda())                                            # patch dropout alone: exactly one draw
    after = torch.get_rng_state()
    torch.set_rng_state(before)
    torch.randint(0, 2 ** 31 - 1, (1,))
    assert torch.equal(after, torch.get_rng_state())


def test_last_patch_keep():
    cfg, params, img, _, _ = model_case("plain")
    model = build(cfg.replace(dtype="bf16"), params)
    assert model.last_patch_keep is None
    model(img.cuda())
    keep = model.last_patch_keep
    assert keep.shape == (MB, 8) and keep.dtype == torch.int32 and keep.is_cuda
    assert np.array_equal(keep.cpu().numpy(), ref.keep_indices(MSEED, MB, 16, 8))
    with torch.no_grad():           # grad disabled: inactive, like dropout
        assert model(img.cuda()).shape == (MB, 2) and model.last_patch_keep is None
    model(img.cuda())
    model.eval()
    model(img.cuda())
    assert model.last_patch_keep is None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_same_seed_same_step_bitwise(dtype):
    cfg, params, img, tgt, _ = model_case("plain")
    cfg = cfg.replace(dtype=dtype)
    first = step(cfg, params, img, tgt)
    assert same(first, step(cfg, params, img, tgt))
    assert not torch.equal(first[0], step(cfg, params, img, tgt, seed=MSEED + 1)[0])


def test_precision_knob_refuses_patch_dropout():
    cfg, params, img, _, _ = model_case("plain")
    model = build(cfg.replace(dtype="bf16f8"), params)
    with pytest.raises(ValueError, match="parity / evaluation knob"):
        model(img.cuda())
    model.eval()
    assert model(img.cuda()).shape == (MB, 2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_adam_moves_only_the_kept_position_rows(dtype):
    """B = 2, seed 11: patches 0, 2, 5, 6 and 7 are kept by neither sample."""
    cfg, params, img, tgt, _ = model_case("plain", 2)
    kept = np.unique(ref.keep_indices(MSEED, 2, 16, 8))
    assert sorted(set(range(16)) - set(kept.tolist())) == [0, 2, 5, 6, 7]
    model = build(cfg.replace(dtype=dtype), params)
    opt = optim.Adam(model, learning_rate=1e-3)
    before = model.pos_embed.detach().clone()
    cross_entropy(model(img.cuda()), tgt.cuda()).backward()
    grad = model.pos_embed.grad.detach().clone()
    opt.step()
    touched = torch.zeros(17, dtype=torch.bool)
    touched[0] = True
    touched[1 + torch.from_numpy(kept)] = True
    row_grad = grad[0].abs().sum(dim=1).cpu()
    assert not grad[0].cpu()[~touched].any() and row_grad[touched].gt(0).all()
    moved = (model.pos_embed.detach() != before)[0].any(dim=1).cpu()
    assert torch.equal(moved, touched)


# ------------------------------------------------------------------ one real-size pass
def test_vit_b_pass():
    """ViT-B/16 224, depth 2, bs 8, bf16, rate 0.5 (N = 99): forward + backward + Adam."""
    cfg = ViTConfig(depth=2, dtype="bf16", patch_drop_rate=0.5)
    assert cfg.kept_patches == 98
    img, tgt = vit_ref.synthetic_batch(cfg, 8)
    img, tgt = img.cuda(), tgt.cuda()
    runs = []
    for _ in range(2):
        model = VisionTransformer(cfg).cuda().train()
        model.reset_parameters(seed=0)
        model.drop_seed = MSEED
        opt = optim.Adam(model, learning_rate=1e-4)
        logits = model(img)
        cross_entropy(logits, tgt).backward()
        opt.step()
        assert model.last_patch_keep.shape == (8, 98)
        runs.append((logits.detach().cpu(), model.pos_embed.detach().cpu().clone()))
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
