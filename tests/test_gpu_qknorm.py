"""QK-norm on the device against tests/ref_qknorm.py.

Kernels (vitmi_qknorm_fwd / _bwd through the C ABI, guarded buffers): both dtypes, H in {1, 2, 3, 5, 12,
16, 20, 32} (a row is 24 H 16-byte slots in bf16 and 48 H in fp32, so H = 12 bf16 and every H >= 6 in fp32
spread a row over more than one 256-thread block, and H = 1, 2, 3, 5 pack several rows into one), M in {1,
3, 64, 394} plus, for H = 3 and 12, two rows more than one pass of the capped grid covers (every
grid-stride loop walks), dense and padded row strides, every input family.  A result conforms iff EVERY
element of out, mean, rstd, dq, dk, dgamma_*, dbeta_* and dbias is within its bound.

Model (img 32, patch 8, D 128, depth 3, H 2, batch 6, as tests/test_gpu_layerscale.py): logits and every
gradient against the reference in the four compute dtypes.  fp32 is held to the project's 1e-4 / 1e-4.
The low-precision bounds are not fixed in advance: each is max(the project's bound, 2 x the error of the
reference's own bf16 emulation against the fp32 reference on the same inputs), per quantity, computed
here from the reference alone; the factor 2 covers the kernels' different summation order and rounding
points.  blocks.i.attn.k_norm.bias has an exactly zero gradient (one vector added to every key shifts
each softmax row by a constant), so it is judged absolutely, against the norm of the same block's
k_norm.weight gradient, and left out of the relative ranking.

Measured on an MI355X (bound in brackets; DESIGN.md, "QK-norm", has the table):
  kernels  worst |err| / bound over every H: fp32 out 0.053, dq / dk 0.159, dgamma 0.378, dbeta 0.445, dbias
           0.481; bf16 out / dq / dk 0.995 (half an ulp of the store), dgamma 0.431, dbeta 0.403, dbias 0.990
  fp32     logits rel 4.2e-6 [1e-4], worst gradient 2.5e-6 [1e-4], |d k_norm.bias| / |d k_norm.weight| 9.6e-7
  bf16     logits rel 4.0e-2 [9.5e-2], worst gradient 3.2e-2 [3.8e-2] (blocks.0.attn.k_norm.weight), k_norm.bias 1.9e-2
  bf16x3   logits max-abs 5.2e-4 [5.7e-3], worst gradient 1.9e-2 [2.0e-2], k_norm.bias 1.3e-2
  bf16f8   logits max-abs 5.6e-4 [5.7e-3], worst gradient 2.9e-2 [3.0e-2] (blocks.0.attn.q_norm.bias), k_norm.bias 1.6e-2
  emulated logits rel 4.8e-2 (max-abs 2.9e-3), worst gradients 1.9e-2 (the norm parameters'), the rest near 1e-2"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_qknorm as ref  # noqa: E402
from oracle import vit_ref  # noqa: E402
from vitmi import _lib, checkpoint  # noqa: E402
from vitmi.config import ViTConfig  # noqa: E402
from vitmi.modules import Attention, Block, VisionTransformer, cross_entropy  # noqa: E402
from vitmi.optim import Adam  # noqa: E402

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
DH = ref.DH
HS = (1, 2, 3, 5, 12, 16, 20, 32)
MS = (1, 3, 64, 394)
WALK_HS = (3, 12)            # these also run M = rows of one pass + 2


# ------------------------------------------------------------------ the kernels
def ms_of(H):
    if H not in WALK_HS:
        return MS
    return MS + (max(ref.rows_per_pass(10 ** 6, H, True), ref.rows_per_pass(10 ** 6, H, False)) + 2,)


def dev_vec(t):
    return t.contiguous().to(DEV)


def run_fwd(inp, M, H, bf16, pads):
    dtype = BF if bf16 else F32
    W = 3 * H * DH
    qkv = ref.padded(M, W, W + pads[0], dtype, "nan").set(inp["qkv"]).to(DEV)
    out = ref.padded(M, W, W + pads[1], dtype, "guard").to(DEV)
    mean = ref.padded(M, 2 * H, 2 * H, F32, "guard").to(DEV)
    rstd = ref.padded(M, 2 * H, 2 * H, F32, "guard").to(DEV)
    par = [dev_vec(inp[k]) for k in ("gq", "bq", "gk", "bk")]
    before = qkv.buf.clone()
    rc = _lib.lib().vitmi_qknorm_fwd(int(bf16), M, H, DH, qkv.ptr(), qkv.pitch, *[p.data_ptr() for p in par],
                                     ref.rl.f32_eps(), out.ptr(), out.pitch, mean.ptr(), rstd.ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().vitmi_last_error()
    assert torch.equal(before.view(torch.uint8), qkv.buf.view(torch.uint8)), "the input was written"
    for p in (out, mean, rstd):
        assert ref.guards_intact(p), "guards changed"
    return out.view.cpu(), mean.view.cpu(), rstd.view.cpu()


def run_bwd(inp, r, M, H, bf16, pads, skip=()):
    """{dqkv, dgq, dbq, dgk, dbk, dbias}; a destination named in ``skip`` is passed as NULL and comes back
    as its prev."""
    dtype = BF if bf16 else F32
    W = 3 * H * DH
    qkv = ref.padded(M, W, W + pads[0], dtype, "nan").set(inp["qkv"]).to(DEV)
    dqkv = ref.padded(M, W, W + pads[2], dtype, "guard").set(inp["dqkv"]).to(DEV)
    mean, rstd = dev_vec(r["mean_in"]), dev_vec(r["rstd_in"])
    gq, gk = dev_vec(inp["gq"]), dev_vec(inp["gk"])
    names = ("dgq", "dbq", "dgk", "dbk", "dbias")
    dst = {k: ref.padded(1, inp["prev"][k].numel(), inp["prev"][k].numel() + 4, F32, "guard")
           .set(inp["prev"][k].view(1, -1)).to(DEV) for k in names}
    nws = _lib.lib().vitmi_qknorm_bwd_workspace_size(M, H)
    assert nws == ref.workspace_bytes(M, H)
    ws = ref.padded(1, nws // 4, nws // 4 + 4, F32, "guard").to(DEV)
    before = qkv.buf.clone()
    rc = _lib.lib().vitmi_qknorm_bwd(int(bf16), M, H, DH, qkv.ptr(), qkv.pitch, mean.data_ptr(), rstd.data_ptr(),
                                     gq.data_ptr(), gk.data_ptr(), dqkv.ptr(), dqkv.pitch,
                                     *[None if k in skip else dst[k].ptr() for k in names], ws.ptr(), nws, None)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().vitmi_last_error()
    assert torch.equal(before.view(torch.uint8), qkv.buf.view(torch.uint8)), "the saved input was written"
    for p in (dqkv, ws, *dst.values()):
        assert ref.guards_intact(p), "guards changed"
    res = {k: dst[k].view.cpu().view(-1) for k in names}
    res["dqkv"] = dqkv.view.cpu()
    return res


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", HS)
def test_kernels_conform(H, bf16):
    dtype = BF if bf16 else F32
    D = H * DH
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for mi, M in enumerate(ms_of(H)):
        for fi, fam in enumerate(ref.FAMILIES):
            pads = (0, 0, 0) if (mi + fi) % 2 == 0 else (8, 16, 24)       # dense / ld, ldo, ldd > 3D
            inp, r = ref.reference(fam, M, H, bf16)
            what = (fam, M, pads)
            # forward
            out, mean, rstd = run_fwd(inp, M, H, bf16, pads)
            note("out", ref.worst_ratio(out[:, :2 * D], *r["out"]))
            note("mean", ref.worst_ratio(mean, *r["mean"]))
            note("rstd", ref.worst_ratio(rstd, *r["rstd"]))
            assert torch.equal(bits(out[:, 2 * D:]), bits(inp["qkv"][:, 2 * D:].to(dtype))), (what, "v not bitwise")
            if fam == "const":
                for row in ref.const_heads(M, H):
                    m, h = divmod(row, H)
                    assert torch.equal(out[m, h * DH:(h + 1) * DH], inp["bq"].to(dtype)), (what, row)
                    assert torch.equal(out[m, D + h * DH:D + (h + 1) * DH], inp["bk"].to(dtype)), (what, row)
            # backward, onto the non-zero prev
            b = run_bwd(inp, r, M, H, bf16, pads)
            note("dqk", ref.worst_ratio(b["dqkv"][:, :2 * D], *r["dqk"]))
            for k in ("dgq", "dbq", "dgk", "dbk", "dbias"):
                note(k, ref.worst_ratio(b[k], *r[k]))
            assert torch.equal(bits(b["dqkv"][:, 2 * D:]), bits(inp["dqkv"][:, 2 * D:].to(dtype))), (what, "dv written")
            if fam == "int":
                assert torch.equal(b["dbq"].double(), r["dbq"][0]) and torch.equal(b["dbk"].double(), r["dbk"][0]), what
                assert torch.equal(b["dbias"][2 * D:].double(), r["dbias"][0][2 * D:]), what
            assert max(worst.values()) <= 1.0, (what, worst)
            # NULL destinations: the others and dqkv come out bit for bit the same, the skipped keep prev
            if fam == "rows":
                for skip in (("dbias",), ("dgq", "dbk"), ("dgq", "dbq", "dgk", "dbk", "dbias")):
                    b2 = run_bwd(inp, r, M, H, bf16, pads, skip)
                    for k in b:
                        want = inp["prev"][k] if k in skip else b[k]
                        assert torch.equal(bits(b2[k]), bits(want)), (what, skip, k)
    print(f"qknorm kernels H {H} {'bf16' if bf16 else 'fp32'}: worst |err| / bound "
          f"{({k: round(v, 3) for k, v in worst.items()})}")


# ------------------------------------------------------------------ the model against the reference
CFG = dict(img_size=32, patch_size=8, embed_dim=128, depth=3, num_heads=2, num_classes=2)
MB, MSEED = 6, 11
LS_SEED = 5


def qk_cfg(dtype, **kw):
    return ViTConfig(**CFG, dtype=dtype, qk_norm=True, **kw)


@functools.lru_cache(maxsize=None)
def model_case(drop=False, emulate=False):
    """Parameters (norm parameters included), batch and the CPU reference step, computed once per variant.
    ``drop``: LayerScale, drop path 0.5 and dropout 0.1 at seed MSEED on top; ``emulate``: the bf16
    emulation of the same step."""
    cfg = qk_cfg("fp32", **(dict(init_values=1.0, drop_path_rate=0.5, drop_rate=0.1) if drop else {}))
    params = dict(vit_ref.init_params(cfg, seed=0))
    params.update(ref.model_norm_params(cfg))
    if drop:
        import ref_layerscale
        params.update(ref_layerscale.gammas(cfg, LS_SEED))
    img, tgt = vit_ref.synthetic_batch(cfg, MB)
    return params, img, tgt, ref.forward_backward(img, tgt, params, cfg, seed=MSEED if drop else None,
                                                  emulate=emulate)


def build(cfg, params):
    model = VisionTransformer(cfg).cuda()
    model.load_param_dict(params)
    return model


def step(cfg, params, img, tgt, seed=None, train=True, frozen=(), backwards=1):
    model = build(cfg, params)
    model.drop_seed = seed
    model.train(train)
    for k, p in model.named_parameters():
        if frozen and k.endswith(tuple(frozen)):
            p.requires_grad_(False)
    for _ in range(backwards):
        logits = model(img.cuda())
        cross_entropy(logits, tgt.cuda()).backward()
    grads = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return logits.detach().cpu(), grads


def ranked(keys):
    """The gradients judged relatively: all but k_norm.bias, whose exact value is zero."""
    return [k for k in keys if not k.endswith("k_norm.bias")]


def check_k_norm_bias(g, g_ref, tol_of):
    """|| d k_norm.bias || <= tol x || d k_norm.weight (reference) || of the same block."""
    out = []
    for k in g:
        if k.endswith("k_norm.bias"):
            kw = k[:-len("bias")] + "weight"
            ratio = g[k].double().norm().item() / g_ref[kw].double().norm().item()
            out.append((ratio, k))
            assert ratio <= tol_of(kw), (k, ratio, tol_of(kw))
    return max(out)


def worst_grad(g, g_ref, keys=None):
    return max((vit_ref.rel_err(g[k], g_ref[k]), k) for k in ranked(keys if keys is not None else g_ref))


@pytest.mark.parametrize("dtype,ltol,gtol", [("fp32", 1e-4, 1e-4), ("bf16", 5e-2, 2e-2), ("bf16x3", 1e-3, 2e-2),
                                             ("bf16f8", 1e-3, 2e-2)])
def test_model_matches_reference(dtype, ltol, gtol):
    params, img, tgt, (l_ref, _, g_ref) = model_case()
    knob = dtype in ("bf16x3", "bf16f8")
    lmetric = (lambda a: (a - l_ref).abs().max().item()) if knob else (lambda a: vit_ref.rel_err(a, l_ref))
    gtol_of = lambda k: gtol                                             # noqa: E731
    if dtype != "fp32":
        # the low-precision bound, from the reference alone: max(project's, 2 x the bf16 emulation's error)
        l_emu, _, g_emu = model_case(emulate=True)[3]
        emu = {k: vit_ref.rel_err(g_emu[k], g_ref[k]) for k in ranked(g_ref)}
        print(f"qk-norm emulation: logits {'max-abs' if knob else 'rel'} {lmetric(l_emu):.3e}, worst grads "
              f"{sorted(((v, k) for k, v in emu.items()), reverse=True)[:4]}")
        ltol = max(ltol, 2 * lmetric(l_emu))
        gtol_of = lambda k: max(gtol, 2 * emu[k])                        # noqa: E731
    l, g = step(qk_cfg(dtype), params, img, tgt)
    lerr = lmetric(l)
    errs = sorted(((vit_ref.rel_err(g[k], g_ref[k]) / gtol_of(k), vit_ref.rel_err(g[k], g_ref[k]), k)
                   for k in ranked(g_ref)), reverse=True)
    nrm = sorted(((vit_ref.rel_err(g[k], g_ref[k]), k) for k in ref.norm_names(qk_cfg(dtype)) if k in ranked(g_ref)),
                 reverse=True)
    print(f"qk-norm {dtype}: logits {'max-abs' if knob else 'rel'} {lerr:.3e} [{ltol:.3e}], worst grads (err / bound, "
          f"err, name) {errs[:3]}, worst norm-parameter grads {nrm[:2]}")
    assert set(g) == set(g_ref)
    assert lerr <= ltol, f"logits {lerr:.3e} > {ltol:.3e}"
    assert errs[0][0] <= 1.0, f"grad {errs[0][2]} rel {errs[0][1]:.3e} > {gtol_of(errs[0][2]):.3e}"
    kb = check_k_norm_bias(g, g_ref, gtol_of)
    print(f"qk-norm {dtype}: worst |d k_norm.bias| / |d k_norm.weight| {kb}")
    # a zero weight channel still has a gradient
    assert all(g[k][ref.ZERO_CHANNEL] != 0 for k in ref.norm_names(qk_cfg(dtype)) if k.endswith("q_norm.weight"))


def test_qk_norm_false_is_the_model_without_the_field():
    params, img, tgt, _ = model_case()
    plain = {k: v for k, v in params.items() if "_norm." not in k}
    for dtype in ("fp32", "bf16"):
        model = VisionTransformer(ViTConfig(**CFG, dtype=dtype, qk_norm=False))
        assert not any("q_norm" in k or "k_norm" in k for k in model.state_dict())
        assert list(model.state_dict()) == list(VisionTransformer(ViTConfig(**CFG, dtype=dtype)).state_dict())
        l0, g0 = step(ViTConfig(**CFG, dtype=dtype), plain, img, tgt)
        l1, g1 = step(ViTConfig(**CFG, dtype=dtype, qk_norm=False), plain, img, tgt)
        assert set(g0) == set(g1) == set(plain)
        assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0), dtype
    on = VisionTransformer(qk_cfg("bf16"))
    assert {k for k, _ in on.named_parameters()} == set(params)
    assert all(on.state_dict()[k].shape == (DH,) for k in ref.norm_names(qk_cfg("bf16")))
    assert all(torch.equal(on.state_dict()[k], torch.ones(DH) if k.endswith("weight") else torch.zeros(DH))
               for k in ref.norm_names(qk_cfg("bf16")))


def test_train_eval_and_no_grad_are_the_same_model():
    params, img, tgt, (l_ref, _, _) = model_case()
    for dtype in ("fp32", "bf16"):
        model = build(qk_cfg(dtype), params)
        l_train = model.train()(img.cuda()).detach().cpu()
        l_eval = model.eval()(img.cuda()).detach().cpu()
        with torch.no_grad():
            l_ng = model(img.cuda()).cpu()
            l_ng_train = model.train()(img.cuda()).cpu()
        assert torch.equal(l_train, l_eval) and torch.equal(l_train, l_ng) and torch.equal(l_train, l_ng_train)
        if dtype == "fp32":
            assert vit_ref.rel_err(l_eval, l_ref) <= 1e-4


def test_frozen_parameters():
    params, img, tgt, (_, _, g_ref) = model_case()
    tol = lambda k: 1e-4                                                 # noqa: E731
    # the norm parameters frozen (NULL destinations), one of the four at a time and all
    for frozen in (("q_norm.weight",), ("k_norm.bias", "q_norm.bias"), ("_norm.weight", "_norm.bias")):
        _, g = step(qk_cfg("fp32"), params, img, tgt, frozen=frozen)
        assert set(g) == {k for k in g_ref if not k.endswith(frozen)}
        assert worst_grad(g, g_ref, list(g))[0] <= 1e-4
        if any(k.endswith("k_norm.bias") for k in g):
            check_k_norm_bias(g, g_ref, tol)
    # a frozen qkv bias: no column sums, everything else unchanged
    _, g = step(qk_cfg("fp32"), params, img, tgt, frozen=("attn.qkv.bias",))
    assert set(g) == {k for k in g_ref if not k.endswith("attn.qkv.bias")}
    assert worst_grad(g, g_ref, list(g))[0] <= 1e-4
    # the qkv weight frozen: the norm's backward still runs for the input gradient
    _, g = step(qk_cfg("fp32"), params, img, tgt, frozen=("attn.qkv.weight",))
    assert worst_grad(g, g_ref, list(g))[0] <= 1e-4


def test_two_backwards_accumulate():
    params, img, tgt, _ = model_case()
    _, g1 = step(qk_cfg("fp32"), params, img, tgt)
    _, g2 = step(qk_cfg("fp32"), params, img, tgt, backwards=2)
    worst = max((vit_ref.rel_err(g2[k], 2 * g1[k]), k) for k in ranked(g1))
    assert set(g1) == set(g2) and worst[0] <= 1e-6, worst


def test_same_step_twice_is_bitwise():
    params, img, tgt, _ = model_case(drop=True)
    cfg = qk_cfg("bf16", init_values=1.0, drop_path_rate=0.5, drop_rate=0.1)
    l0, g0 = step(cfg, params, img, tgt, seed=MSEED)
    l1, g1 = step(cfg, params, img, tgt, seed=MSEED)
    assert torch.equal(l0, l1) and set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)


def test_with_layerscale_drop_path_and_dropout():
    params, img, tgt, (l_ref, _, g_ref) = model_case(drop=True)
    cfg = qk_cfg("fp32", init_values=1.0, drop_path_rate=0.5, drop_rate=0.1)
    l, g = step(cfg, params, img, tgt, seed=MSEED)
    lerr, worst = vit_ref.rel_err(l, l_ref), worst_grad(g, g_ref)
    print(f"qk-norm fp32 + LayerScale + drop path 0.5 + dropout 0.1: logits rel {lerr:.3e}, worst grad {worst}")
    assert set(g) == set(g_ref) and lerr <= 1e-4 and worst[0] <= 1e-4
    check_k_norm_bias(g, g_ref, lambda k: 1e-4)


# ------------------------------------------------------------------ the user-facing modules
def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def block_params(D, seed):
    cfg = ViTConfig(img_size=32, patch_size=8, embed_dim=D, depth=1, num_heads=D // DH, dtype="fp32", qk_norm=True)
    p = {k: v for k, v in vit_ref.init_params(cfg, seed=seed).items() if k.startswith("blocks.0.")}
    p.update(ref.model_norm_params(cfg, seed=seed + 20))
    return cfg, p


def compare_module(mod, prefix, run_ref, D):
    cfg, p = block_params(D, 4)
    with torch.no_grad():
        for k, q in mod.named_parameters():
            q.copy_(p[prefix + k])
    x, dout = rnd(6, 17, D, seed=21), rnd(6, 17, D, seed=22)
    leaves = {k: v.clone().requires_grad_() for k, v in p.items()}
    xr = x.clone().requires_grad_()
    out_ref = run_ref(xr, leaves, cfg)
    out_ref.backward(dout)
    xd = x.to(DEV).requires_grad_()
    out = mod(xd)
    out.backward(dout.to(DEV))
    assert vit_ref.rel_err(out.detach().cpu(), out_ref.detach()) <= 1e-4
    assert vit_ref.rel_err(xd.grad.cpu(), xr.grad) <= 1e-4
    named = dict(mod.named_parameters())
    worst = max((vit_ref.rel_err(named[k].grad.cpu(), leaves[prefix + k].grad), k) for k in ranked(named))
    assert worst[0] <= 1e-4, worst
    kb, kw = named["attn.k_norm.bias" if prefix == "blocks.0." else "k_norm.bias"], \
        leaves["blocks.0.attn.k_norm.weight"]
    assert kb.grad.double().norm().item() <= 1e-4 * kw.grad.double().norm().item()


def test_user_stacked_block_matches_autograd():
    D = 128
    blk = Block(D, 2, dtype="fp32", qk_norm=True).cuda()
    names = [k for k, _ in blk.named_parameters()]
    assert [k for k in names if "_norm." in k] == ["attn.q_norm.weight", "attn.q_norm.bias", "attn.k_norm.weight",
                                                    "attn.k_norm.bias"]
    assert [k for k in names if "_norm." not in k] == [k for k, _ in Block(D, 2, dtype="fp32").named_parameters()]
    compare_module(blk, "blocks.0.", lambda x, p, cfg: ref.block(x, p, 0, cfg), D)


def test_user_stacked_attention_matches_autograd():
    D = 192
    attn = Attention(D, 3, dtype="fp32", qk_norm=True).cuda()
    assert [k for k, _ in attn.named_parameters()][-4:] == ["q_norm.weight", "q_norm.bias", "k_norm.weight",
                                                            "k_norm.bias"]
    assert Attention(D, 3, dtype="fp32").q_norm is None
    compare_module(attn, "blocks.0.attn.", lambda x, p, cfg: ref.attention(x, p, "blocks.0.", cfg), D)


# ------------------------------------------------------------------ optimizer, checkpoints, the refusal
def test_adam_does_not_decay_the_norm_parameters():
    params, img, tgt, _ = model_case()
    after = {}
    for wd in (0.1, 0.0):
        model = build(qk_cfg("bf16"), params)
        opt = Adam(model, learning_rate=1e-2, weight_decay=wd)
        cross_entropy(model(img.cuda()), tgt.cuda()).backward()
        opt.step()
        after[wd] = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
    for k in ref.norm_names(qk_cfg("bf16")):
        assert torch.equal(after[0.1][k], after[0.0][k]), k
        if not k.endswith("k_norm.bias"):
            assert not torch.equal(after[0.0][k], params[k]), k
    assert not torch.equal(after[0.1]["blocks.1.attn.qkv.weight"], after[0.0]["blocks.1.attn.qkv.weight"])


def test_checkpoint_round_trip_with_timm_keys(tmp_path):
    from safetensors.torch import load_file
    params, img, tgt, _ = model_case()
    model = build(qk_cfg("bf16"), params).eval()
    path = str(tmp_path / "qk.safetensors")
    checkpoint.save_weights(model, path)
    saved = load_file(path)
    for i in range(CFG["depth"]):
        for n in ("q_norm", "k_norm"):
            assert torch.equal(saved[f"blocks.{i}.attn.{n}.weight"], params[f"blocks.{i}.attn.{n}.weight"])
            assert torch.equal(saved[f"blocks.{i}.attn.{n}.bias"], params[f"blocks.{i}.attn.{n}.bias"])
    fresh = VisionTransformer(qk_cfg("bf16")).cuda().eval()
    checkpoint.load_weights(fresh, path)
    assert torch.equal(model(img.cuda()), fresh(img.cuda()))
    plain = {k: v for k, v in params.items() if "_norm." not in k}
    with pytest.raises(KeyError):
        fresh.load_param_dict(plain)
    with pytest.raises(KeyError):                                          # and a model without the norm refuses the file
        checkpoint.load_weights(VisionTransformer(ViTConfig(**CFG, dtype="bf16")).cuda(), path)


@pytest.mark.parametrize("dtype", ["bf16x3", "bf16f8"])
def test_knob_with_a_long_sequence_raises(dtype):
    cfg = ViTConfig(img_size=136, patch_size=8, embed_dim=128, depth=1, num_heads=2, num_classes=2, dtype=dtype,
                    qk_norm=True)
    assert cfg.seq_len == 290
    model = VisionTransformer(cfg).cuda()
    with pytest.raises(ValueError, match="qk_norm"):
        model(torch.zeros(1, 3, 136, 136, device=DEV))
