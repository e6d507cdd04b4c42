"""LayerScale on the device against the CPU reference tests/ref_layerscale.py: the fold and backward
kernels and the standalone module's kernels elementwise, then the model (forward and every gradient in
the four compute dtypes, with dropout and drop path on top, eval / no_grad, the identity properties,
frozen parameters, accumulation, determinism, the user-facing modules, Adam's decay set and checkpoints).

Measured on an MI355X (the model case, depth 3, D 128, B 6; bound in brackets):
  fp32    logits rel 4.2e-7 [1e-4], worst gradient rel 1.5e-6 [1e-4] (worst gamma 1.2e-6)
  bf16    logits rel 3.0e-3 [5e-2], worst gradient rel 1.0e-2 [2e-2] (worst gamma 8.3e-3)
  bf16x3  logits max-abs 2.2e-4 [1e-3], worst gradient rel 7.3e-3 [2e-2] (a gamma's)
  bf16f8  logits max-abs 2.5e-4 [1e-3], worst gradient rel 7.7e-3 [2e-2] (worst gamma 6.4e-3)
  fp32 with drop path 0.5 and dropout 0.1: logits rel 2.4e-7, worst gradient rel 8.9e-7 [1e-4 / 1e-4]
  dgamma of vitmi_layerscale_bwd over its worst-case bound: <= 0.065 (at K = 8), <= 0.003 elsewhere;
  vitmi_layerscale_dgamma: 1e-4 of its bound."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_layerscale as ref  # noqa: E402
import vitmi  # noqa: E402
from oracle import vit_ref  # noqa: E402
from vitmi import checkpoint, ops  # noqa: E402
from vitmi.config import ViTConfig  # noqa: E402
from vitmi.modules import Block, LayerScale, VisionTransformer, cross_entropy  # noqa: E402
from vitmi.optim import Adam  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
U = 2.0 ** -23


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def gamma_vec(n, seed):
    """ref.gammas' distribution for one vector of any length (channel 3 exactly 0)."""
    g = torch.Generator().manual_seed(seed)
    t = (0.25 + 1.25 * torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.25, -1.0, 1.0)
    t[ref.ZERO_CHANNEL] = 0.0
    return t.float()


# ------------------------------------------------------------------ the fold and backward kernels
# (128, 128), (128, 512): the model case's; (193, 264): odd row count, K a multiple of 8 but not of 64;
# (5, 3072): block-per-row with a ragged grid of rows; (3072, 8): one unit per row; (768, 3072): ViT-B fc2
SHAPES = [(128, 128), (128, 512), (193, 264), (5, 3072), (3072, 8), (768, 3072)]


@functools.lru_cache(maxsize=None)
def kernel_case(N, K):
    w, b, gam = rnd(N, K, seed=1, scale=0.05), rnd(N, seed=2, scale=0.1), gamma_vec(N, 3)
    dw, db, pre = rnd(N, K, seed=4), rnd(N, seed=5), rnd(N, seed=6)
    want64 = pre.double() + (dw.double() * w.double()).sum(1) + db.double() * b.double()
    mag = pre.abs().double() + (dw.double() * w.double()).abs().sum(1) + (db.double() * b.double()).abs()
    return w, b, gam, dw, db, pre, want64, (K + 4) * U * mag


@pytest.mark.parametrize("N,K", SHAPES)
def test_fold_is_bitwise(N, K):
    w, b, gam = kernel_case(N, K)[:3]
    for out_dtype in (F32, BF):
        w_eff, b_eff = ops.layerscale_fold(w.to(DEV), gam.to(DEV), b.to(DEV), out_dtype)
        assert w_eff.dtype == out_dtype and w_eff.shape == (N, K) and b_eff.dtype == F32
        assert torch.equal(w_eff.cpu(), (gam[:, None] * w).to(out_dtype))
        assert torch.equal(b_eff.cpu(), gam * b)
        w_only, none = ops.layerscale_fold(w.to(DEV), gam.to(DEV), None, out_dtype)
        assert none is None and torch.equal(w_only, w_eff)
    assert (w_eff.cpu()[ref.ZERO_CHANNEL] == 0).all()


def run_bwd(N, K, scale=True, with_dgamma=True):
    w, b, gam, dw, db, pre = kernel_case(N, K)[:6]
    dwd, dbd, dg = dw.to(DEV), db.to(DEV), pre.to(DEV)
    ops.layerscale_bwd(w.to(DEV), b.to(DEV), gam.to(DEV), dwd, dbd, dg if with_dgamma else None, scale)
    return dwd.cpu(), dbd.cpu(), dg.cpu()


@pytest.mark.parametrize("N,K", SHAPES)
def test_bwd(N, K):
    w, b, gam, dw, db, pre, want64, bound = kernel_case(N, K)
    gdw, gdb, gdg = run_bwd(N, K)
    assert torch.equal(gdw, gam[:, None] * dw) and torch.equal(gdb, gam * db)
    err = (gdg.double() - want64).abs()
    print(f"layerscale_bwd ({N}, {K}): worst |err| / bound = {(err / bound).max().item():.4f}")
    assert (err <= bound).all()
    assert gdg[ref.ZERO_CHANNEL] != pre[ref.ZERO_CHANNEL]          # a zero gamma still has a gradient
    # twice: bitwise equal
    rdw, rdb, rdg = run_bwd(N, K)
    assert torch.equal(rdw, gdw) and torch.equal(rdb, gdb) and torch.equal(rdg, gdg)
    # the leave-untouched mode: the same dgamma bound, dw / db as they were
    udw, udb, udg = run_bwd(N, K, scale=False)
    assert torch.equal(udw, dw) and torch.equal(udb, db)
    assert ((udg.double() - want64).abs() <= bound).all()
    # a frozen gamma: the reduction is skipped, the products are the same
    fdw, fdb, fdg = run_bwd(N, K, with_dgamma=False)
    assert torch.equal(fdw, gdw) and torch.equal(fdb, gdb) and torch.equal(fdg, pre)


def test_bwd_without_a_weight_or_a_bias_destination():
    N, K = 128, 512
    w, b, gam, dw, db, pre, want64, bound = kernel_case(N, K)
    dbd = db.to(DEV)
    ops.layerscale_bwd(w.to(DEV), b.to(DEV), gam.to(DEV), None, dbd, None, True)      # only the bias trains
    assert torch.equal(dbd.cpu(), gam * db)
    dwd, dg = dw.to(DEV), pre.to(DEV)
    ops.layerscale_bwd(w.to(DEV), None, gam.to(DEV), dwd, None, dg, True)             # a linear without bias
    assert torch.equal(dwd.cpu(), gam[:, None] * dw)
    assert ((dg.cpu().double() - (want64 - db.double() * b.double())).abs() <= bound).all()


# ------------------------------------------------------------------ the standalone module's kernels
SM, SN = 2167, 320            # the drop-path tests' shape


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
def test_apply_and_dgamma(strided):
    gam = gamma_vec(SN, 7)
    xs, dys = rnd(SM, SN + 8, seed=8), rnd(SM, SN + 8, seed=9)
    xc, dyc = xs[:, :SN].contiguous(), dys[:, :SN].contiguous()
    x = xs.to(DEV)[:, :SN] if strided else xc.to(DEV)
    dy = dys.to(DEV)[:, :SN] if strided else dyc.to(DEV)
    assert x.is_contiguous() != strided
    for out_dtype in (F32, BF):
        y = ops.layerscale_apply(x, gam.to(DEV), out_dtype)
        assert y.dtype == out_dtype and y.shape == (SM, SN) and torch.equal(y.cpu(), (xc * gam).to(out_dtype))
    dg = torch.zeros(SN, device=DEV)
    ops.layerscale_dgamma(dy, x, dg)
    prod = dyc.double() * xc.double()
    err, bound = (dg.cpu().double() - prod.sum(0)).abs(), (SM + 4) * U * prod.abs().sum(0)
    print(f"layerscale_dgamma strided={strided}: worst |err| / bound = {(err / bound).max().item():.4f}")
    assert (err <= bound).all()
    dg2 = torch.zeros(SN, device=DEV)
    ops.layerscale_dgamma(dy, x, dg2)
    assert torch.equal(dg, dg2)
    ops.layerscale_dgamma(dy, x, dg2)                               # += : twice the sum, exactly
    assert torch.equal(dg2, 2 * dg)


# ------------------------------------------------------------------ the model against the reference
CFG = dict(img_size=32, patch_size=8, embed_dim=128, depth=3, num_heads=2, num_classes=2)
MB, MSEED, GSEED = 6, 11, 5


@functools.lru_cache(maxsize=None)
def model_case(drop=False, unit=False):
    """Parameters (gammas included), batch and the CPU reference step, computed once per variant:
    ``drop``: drop path 0.5 and dropout 0.1 at seed MSEED on top; ``unit``: every gamma 1."""
    cfg = ViTConfig(**CFG, dtype="fp32", init_values=1.0, drop_path_rate=0.5 if drop else 0.0,
                    drop_rate=0.1 if drop else 0.0)
    params = dict(vit_ref.init_params(cfg, seed=0))
    params.update(ref.ones(cfg) if unit else ref.gammas(cfg, GSEED))
    img, tgt = vit_ref.synthetic_batch(cfg, MB)
    return params, img, tgt, ref.forward_backward(img, tgt, params, cfg, seed=MSEED if drop else None)


def build(cfg, params):
    model = VisionTransformer(cfg).cuda()
    model.load_param_dict(params)
    return model


def step(cfg, params, img, tgt, seed=None, train=True, frozen=(), backwards=1):
    model = build(cfg, params)
    model.drop_seed = seed
    model.train(train)
    for k, p in model.named_parameters():
        if k.endswith(tuple(frozen)) and frozen:
            p.requires_grad_(False)
    for _ in range(backwards):
        logits = model(img.cuda())
        cross_entropy(logits, tgt.cuda()).backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return logits.detach().cpu(), grads


def ls_cfg(dtype, **kw):
    return ViTConfig(**CFG, dtype=dtype, init_values=1.0, **kw)


def worst_grad(g, g_ref, keys=None):
    return max((vit_ref.rel_err(g[k], g_ref[k]), k) for k in (keys if keys is not None else g_ref))


# bounds: the project's own (tests/test_gpu_droppath.py for fp32 / bf16, tests/test_gpu_model.py
# test_knob_split_qkv_override_small_model for the knobs: logits max-abs 1e-3, gradients 2e-2)
@pytest.mark.parametrize("dtype,ltol,gtol", [("fp32", 1e-4, 1e-4), ("bf16", 5e-2, 2e-2), ("bf16x3", 1e-3, 2e-2),
                                             ("bf16f8", 1e-3, 2e-2)])
def test_model_matches_reference(dtype, ltol, gtol):
    params, img, tgt, (l_ref, _, g_ref) = model_case()
    model = build(ls_cfg(dtype), params)
    if dtype == "bf16f8":
        assert all(blk.split_qkv == "weight" for blk in model.blocks)     # D = 128: the weight-side qkv form
    l, g = step(ls_cfg(dtype), params, img, tgt)
    knob = dtype in ("bf16x3", "bf16f8")
    lerr = (l - l_ref).abs().max().item() if knob else vit_ref.rel_err(l, l_ref)
    errs = sorted(((vit_ref.rel_err(g[k], g_ref[k]), k) for k in g_ref), reverse=True)
    gam = worst_grad(g, g_ref, ref.gamma_names(ls_cfg(dtype)))
    print(f"layer scale {dtype}: logits {'max-abs' if knob else 'rel'} {lerr:.3e}, worst grads {errs[:3]}, "
          f"worst gamma grad {gam}")
    assert set(g) == set(g_ref)
    assert lerr <= ltol, f"logits {lerr:.3e}"
    assert errs[0][0] <= gtol, f"grad {errs[0][1]} rel {errs[0][0]:.3e}"
    assert all(g[k][ref.ZERO_CHANNEL] != 0 for k in ref.gamma_names(ls_cfg(dtype)))


def test_with_dropout_and_drop_path_on_top():
    """Fixes the order dropout -> gamma -> sample factor."""
    params, img, tgt, (l_ref, _, g_ref) = model_case(drop=True)
    l, g = step(ls_cfg("fp32", drop_path_rate=0.5, drop_rate=0.1), params, img, tgt, seed=MSEED)
    lerr, worst = vit_ref.rel_err(l, l_ref), worst_grad(g, g_ref)
    print(f"layer scale fp32 + drop path 0.5 + dropout 0.1: logits rel {lerr:.3e}, worst grad {worst}")
    assert set(g) == set(g_ref) and lerr <= 1e-4 and worst[0] <= 1e-4
    l_plain = model_case()[3][0]
    assert (l_ref - l_plain).abs().max().item() > 1e-3                     # the masks act


def test_eval_and_no_grad_are_the_same_model():
    params, img, tgt, (l_ref, _, _) = model_case()
    for dtype in ("fp32", "bf16"):
        model = build(ls_cfg(dtype), params)
        l_train = model.train()(img.cuda()).detach().cpu()
        l_eval = model.eval()(img.cuda()).detach().cpu()
        with torch.no_grad():
            l_ng = model(img.cuda()).cpu()
            l_ng_train = model.train()(img.cuda()).cpu()
        assert torch.equal(l_train, l_eval) and torch.equal(l_train, l_ng) and torch.equal(l_train, l_ng_train)
        if dtype == "fp32":
            assert vit_ref.rel_err(l_eval, l_ref) <= 1e-4


def test_init_values_none_is_the_model_without_the_field():
    params, img, tgt, _ = model_case()
    plain = {k: v for k, v in params.items() if ".ls" not in k}
    for dtype in ("fp32", "bf16"):
        model = VisionTransformer(ViTConfig(**CFG, dtype=dtype, init_values=None))
        assert not any(".ls" in k or "gamma" in k for k, _ in model.named_parameters())
        l0, g0 = step(ViTConfig(**CFG, dtype=dtype), plain, img, tgt)
        l1, g1 = step(ViTConfig(**CFG, dtype=dtype, init_values=None), plain, img, tgt)
        assert set(g0) == set(g1) == set(plain)
        assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0), dtype


def test_gamma_one_is_the_plain_model():
    params, img, tgt, (_, _, g_ref) = model_case(unit=True)
    plain = {k: v for k, v in params.items() if ".ls" not in k}
    for dtype in ("fp32", "bf16"):
        l0, _ = step(ViTConfig(**CFG, dtype=dtype), plain, img, tgt)
        l1, g1 = step(ls_cfg(dtype), params, img, tgt)
        assert torch.equal(l0, l1), dtype                                   # 1 * W is exact
        if dtype == "fp32":
            worst = worst_grad(g1, g_ref)
            assert set(g1) == set(g_ref) and worst[0] <= 1e-4, worst


def test_frozen_parameters():
    params, img, tgt, (_, _, g_ref) = model_case()
    gam = ref.gamma_names(ls_cfg("fp32"))
    frozen_w = ("attn.proj.weight", "mlp.fc2.weight")
    _, g = step(ls_cfg("fp32"), params, img, tgt, frozen=frozen_w)
    assert set(g) == {k for k in g_ref if not k.endswith(frozen_w)}
    worst = worst_grad(g, g_ref, list(g))
    assert worst[0] <= 1e-4, worst
    assert worst_grad(g, g_ref, gam)[0] <= 1e-4
    # weights and biases of the scaled linears frozen: both of dgamma's terms come from temporaries
    frozen_wb = frozen_w + ("attn.proj.bias", "mlp.fc2.bias")
    _, g = step(ls_cfg("fp32"), params, img, tgt, frozen=frozen_wb)
    assert set(g) == {k for k in g_ref if not k.endswith(frozen_wb)}
    assert worst_grad(g, g_ref, list(g))[0] <= 1e-4
    # the gammas frozen
    _, g = step(ls_cfg("fp32"), params, img, tgt, frozen=("gamma",))
    assert set(g) == set(g_ref) - set(gam)
    assert worst_grad(g, g_ref, list(g))[0] <= 1e-4


def test_two_backwards_accumulate():
    params, img, tgt, _ = model_case()
    _, g1 = step(ls_cfg("fp32"), params, img, tgt)
    _, g2 = step(ls_cfg("fp32"), params, img, tgt, backwards=2)
    worst = max((vit_ref.rel_err(g2[k], 2 * g1[k]), k) for k in g1)
    assert set(g1) == set(g2) and worst[0] <= 1e-6, worst


def test_same_step_twice_is_bitwise():
    params, img, tgt, _ = model_case(drop=True)
    cfg = ls_cfg("bf16", drop_path_rate=0.5, drop_rate=0.1)
    l0, g0 = step(cfg, params, img, tgt, seed=MSEED)
    l1, g1 = step(cfg, params, img, tgt, seed=MSEED)
    assert torch.equal(l0, l1) and set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)


# ------------------------------------------------------------------ the user-facing modules
def test_user_stacked_block_matches_autograd():
    Bb, Ss, D = 6, 17, 128
    blk = Block(D, 2, dtype="fp32", init_values=0.1).cuda()
    names = [k for k, _ in blk.named_parameters()]
    assert names[-2:] == ["ls1.gamma", "ls2.gamma"]
    assert names[:-2] == [k for k, _ in Block(D, 2, dtype="fp32").named_parameters()]     # a prefix
    assert all(torch.equal(p.detach().cpu(), torch.full((D,), 0.1)) for p in (blk.ls1.gamma, blk.ls2.gamma))
    cfg = ViTConfig(img_size=32, patch_size=8, embed_dim=D, depth=1, num_heads=2, dtype="fp32")
    p = {k: v for k, v in vit_ref.init_params(cfg, seed=4).items() if k.startswith("blocks.0.")}
    p.update({"blocks.0.ls1.gamma": gamma_vec(D, 41), "blocks.0.ls2.gamma": gamma_vec(D, 42)})
    with torch.no_grad():
        for k, q in blk.named_parameters():
            q.copy_(p["blocks.0." + k])
    x, dout = rnd(Bb, Ss, D, seed=21), rnd(Bb, Ss, D, seed=22)
    leaves = {k: v.clone().requires_grad_() for k, v in p.items()}
    xr = x.clone().requires_grad_()
    out_ref = ref.block(xr, leaves, 0, cfg)
    out_ref.backward(dout)
    xd = x.to(DEV).requires_grad_()
    out = blk(xd)
    out.backward(dout.to(DEV))
    assert vit_ref.rel_err(out.detach().cpu(), out_ref.detach()) <= 1e-4
    assert vit_ref.rel_err(xd.grad.cpu(), xr.grad) <= 1e-4
    worst = max((vit_ref.rel_err(q.grad.cpu(), leaves["blocks.0." + k].grad), k) for k, q in blk.named_parameters())
    assert worst[0] <= 1e-4, worst


def test_layerscale_module_matches_autograd():
    D = 128
    mod = vitmi.LayerScale(D, 0.5).cuda()
    assert isinstance(mod, LayerScale) and torch.equal(mod.gamma.detach().cpu(), torch.full((D,), 0.5))
    gam = gamma_vec(D, 43)
    with torch.no_grad():
        mod.gamma.copy_(gam)
    x, dy = rnd(6, 17, D, seed=31), rnd(6, 17, D, seed=32)
    xr, gr = x.clone().requires_grad_(), gam.clone().requires_grad_()
    (xr * gr).backward(dy)
    xd = x.to(DEV).requires_grad_()
    y = mod(xd)
    y.backward(dy.to(DEV))
    assert y.shape == x.shape and torch.equal(y.detach().cpu(), x * gam)
    assert torch.equal(xd.grad.cpu(), dy * gam)
    assert vit_ref.rel_err(mod.gamma.grad.cpu(), gr.grad) <= 1e-4
    with pytest.raises(ValueError):
        vitmi.LayerScale(D, float("nan"))


# ------------------------------------------------------------------ optimizer and checkpoints
def test_adam_does_not_decay_gamma():
    params, img, tgt, _ = model_case()
    after = {}
    for wd in (0.1, 0.0):
        model = build(ls_cfg("bf16"), params)
        opt = Adam(model, learning_rate=1e-2, weight_decay=wd)
        cross_entropy(model(img.cuda()), tgt.cuda()).backward()
        opt.step()
        after[wd] = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    for k in ref.gamma_names(ls_cfg("bf16")):
        assert torch.equal(after[0.1][k], after[0.0][k]), k
        assert not torch.equal(after[0.0][k], params[k]), k
    assert not torch.equal(after[0.1]["blocks.1.attn.proj.weight"], after[0.0]["blocks.1.attn.proj.weight"])


def test_checkpoint_round_trip(tmp_path):
    params, img, tgt, _ = model_case()
    model = build(ls_cfg("bf16"), params).eval()
    path = str(tmp_path / "ls.safetensors")
    checkpoint.save_weights(model, path)
    fresh = VisionTransformer(ls_cfg("bf16")).cuda().eval()
    assert all(torch.equal(p.detach().cpu(), torch.ones(128)) for k, p in fresh.named_parameters() if "gamma" in k)
    checkpoint.load_weights(fresh, path)
    assert torch.equal(model(img.cuda()), fresh(img.cuda()))
    plain = {k: v for k, v in params.items() if ".ls" not in k}
    with pytest.raises(KeyError):
        fresh.load_param_dict(plain)
