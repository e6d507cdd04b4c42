"""Global-norm clipping, decoupled weight decay and non-finite step skipping of the fused Adam
step (vitmi_grad_sumsq, vitmi_clip_finalize, vitmi_adam_step_ctl; vitmi.optim.Adam's
global_clipnorm / weight_decay / skip_nonfinite) against numpy on the CPU.

The fp32 update is compared bit for bit with oracle/optim_ref.adam_step, which is fed a gradient
already multiplied by f32(grad_scale) and then by the coef read back from the device, and
parameters already decayed with the three rounded ops p - (p * wd) * lr."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import optim_ref
from vitmi import _lib, optim

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = int(re.search(r"#define\s+VITMI_GRAD_SUMSQ_CHUNK\s+(\d+)",
                      open(os.path.join(ROOT, "include", "vitmi.h")).read()).group(1))


# ------------------------------------------------------------------ raw entry points
def _stream():
    return torch.cuda.current_stream().cuda_stream


def sumsq(gd: torch.Tensor) -> torch.Tensor:
    lib = _lib.lib()
    n = gd.numel()
    part = torch.full((lib.vitmi_grad_sumsq_partials(n),), -1.0, dtype=torch.float64, device=DEV)
    _lib.check(lib.vitmi_grad_sumsq(n, gd.data_ptr(), part.data_ptr(), _stream()), "grad_sumsq")
    torch.cuda.synchronize()
    return part


def finalize(part: torch.Tensor, ctl: torch.Tensor, scale=1.0, clip=0.0, skip=0):
    """-> (coef, norm, skip, skipped_total) read back from the record"""
    _lib.check(_lib.lib().vitmi_clip_finalize(part.numel(), part.data_ptr(), scale, clip, skip, ctl.data_ptr(),
                                              _stream()), "clip_finalize")
    torch.cuda.synchronize()
    rec = ctl.cpu().numpy()
    u = rec.view(np.uint32)
    return rec[0], rec[1], int(u[2]), int(u[3])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def randn(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ sum of squares
@pytest.mark.parametrize("n", [1, 7, CHUNK - 1, CHUNK, CHUNK + 1, 1_000_003])
def test_sumsq_matches_fp64_and_is_reproducible(n):
    g = randn(n, n)
    gd = g.to(DEV)
    part = sumsq(gd)
    assert part.numel() == -(-n // CHUNK)
    ref = float(np.sum(g.numpy().astype(np.float64) ** 2))
    total = float(np.sum(part.cpu().numpy()))
    rel = abs(total - ref) / ref
    print(f"sumsq n={n}: rel err {rel:.3e}")
    # serial fp64 bound n * 2^-53 = 1.1e-10 at the largest n, times ten
    assert rel <= 1e-9
    again = sumsq(gd)
    assert np.array_equal(bits(part.cpu().numpy()), bits(again.cpu().numpy()))


def test_sumsq_partials_do_not_depend_on_the_length():
    n = 3 * CHUNK + 1003
    gd = randn(n, 11).to(DEV)
    long = sumsq(gd).cpu().numpy()
    short = sumsq(gd[:2 * CHUNK]).cpu().numpy()
    assert short.shape == (2,) and long.shape == (4,)
    assert np.array_equal(bits(short), bits(long[:2]))


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_sumsq_sees_one_nonfinite_element(bad):
    n = CHUNK + 7
    g = randn(n, 12)
    for idx in (0, CHUNK - 1, CHUNK, n - 1):
        x = g.clone()
        x[idx] = bad
        total = float(np.sum(sumsq(x.to(DEV)).cpu().numpy()))
        assert not np.isfinite(total), idx


# ------------------------------------------------------------------ finalize
def test_finalize_record():
    n = CHUNK + 7
    g = randn(n, 13)
    part = sumsq(g.to(DEV))
    ref_norm = float(np.sqrt(np.sum(g.numpy().astype(np.float64) ** 2)))
    ctl = torch.zeros(4, dtype=torch.float32, device=DEV)
    one = bits(np.array([1.0], f32))[0]
    # norm below clip_norm: coef is exactly 1
    coef, norm, skip, tot = finalize(part, ctl, clip=2.0 * ref_norm)
    assert bits(np.array([coef]))[0] == one and (skip, tot) == (0, 0)
    # one fp32 rounding of the fp64 value, plus margin
    assert abs(float(norm) - ref_norm) / ref_norm <= 1e-6
    # norm above it: one fp32 division of f32(clip_norm) by the norm as read back
    clip = 0.5 * ref_norm
    coef, norm, skip, tot = finalize(part, ctl, clip=clip)
    assert bits(np.array([coef]))[0] == bits(np.array([f32(clip) / norm], f32))[0]
    assert coef < 1.0
    # grad_scale scales the norm (and its sign does not matter)
    for scale in (0.25, -0.25):
        coef, norm, _, _ = finalize(part, ctl, scale=scale, clip=clip)
        assert abs(float(norm) - 0.25 * ref_norm) / (0.25 * ref_norm) <= 1e-6
        assert bits(np.array([coef]))[0] == one          # 0.25 |g| < 0.5 |g|
    # clip_norm 0 = off
    coef, norm, skip, tot = finalize(part, ctl, clip=0.0)
    assert bits(np.array([coef]))[0] == one and (skip, tot) == (0, 0)
    # a non-finite total: skipped and counted when asked to, a NaN coef either way
    bad = part.clone()
    bad[0] = float("inf")
    coef, norm, skip, tot = finalize(bad, ctl, clip=clip, skip=1)
    assert (skip, tot) == (1, 1) and np.isnan(coef)
    coef, norm, skip, tot = finalize(bad, ctl, clip=clip, skip=0)
    assert (skip, tot) == (0, 1) and np.isnan(coef)
    coef, norm, skip, tot = finalize(part, ctl, clip=clip, skip=1)
    assert (skip, tot) == (0, 1) and coef < 1.0


# ------------------------------------------------------------------ the step
@pytest.mark.parametrize("n,scale", [(1, 1.0), (7, 1.0), (1_000_003, 1.0), (4099, 0.25)])
def test_adam_step_ctl_clipped_bit_exact(n, scale):
    """per-tensor Adam with clipping certainly active (clip norm 1e-4) over three steps"""
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g)
    ref = (p.numpy().copy(), np.zeros(n, f32), np.zeros(n, f32))
    pd = p.to(DEV).requires_grad_(True)
    opt = optim.Adam([pd], learning_rate=1e-3, grad_scale=scale, global_clipnorm=1e-4)
    for t in range(1, 4):
        gr = torch.randn(n, generator=g) * (10.0 ** (t - 2))
        pd.grad = gr.to(DEV)
        opt.step()
        norm, coef = (x.cpu().numpy() for x in opt.last_clip())
        ref_norm = abs(scale) * float(np.sqrt(np.sum(gr.numpy().astype(np.float64) ** 2)))
        assert abs(float(norm) - ref_norm) <= 1e-6 * ref_norm
        assert coef < 1.0 and coef == f32(1e-4) / norm
        gs = gr.numpy() * f32(scale) * f32(coef)
        ref = optim_ref.adam_step(ref[0], gs, ref[1], ref[2], 1e-3, t)
        torch.cuda.synchronize()
        assert np.array_equal(bits(pd.detach().cpu().numpy()), bits(ref[0])), t
        assert np.array_equal(bits(opt._m[0].cpu().numpy()), bits(ref[1]))
        assert np.array_equal(bits(opt._v[0].cpu().numpy()), bits(ref[2]))
    assert opt.skipped_steps == 0


# under the 8192-block grid cap (2 097 152 threads, two 16-B groups each): a thread's second group is
# partly in range at the first size, and the grid-stride loop takes a second trip at the second
BIG_PARTIAL, BIG_SECOND_TRIP = 8_388_608 + 1031, 16_777_216 + 1203
PAD, SENTINEL = 64, -77.0          # the sentinel is exact in bf16 too


def guarded(n, init=None, dtype=torch.float32):
    """-> (n elements PAD elements into an allocation whose margins hold the sentinel, the allocation)"""
    full = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
    inner = full[PAD:PAD + n]
    inner.copy_(init) if init is not None else inner.zero_()
    return inner, full


def margins_intact(full):
    return bool((full[:PAD] == SENTINEL).all()) and bool((full[-PAD:] == SENTINEL).all())


def int_bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("n", [1, 7, 1_000_003, BIG_PARTIAL, BIG_SECOND_TRIP])
def test_adam_step_ctl_without_record_equals_adam_step(n):
    lib = _lib.lib()
    ptr = lambda t: t.data_ptr() if t is not None else None    # noqa: E731
    for shadow in (True, False):
        g = torch.Generator().manual_seed(n + 1)
        p0 = torch.randn(n, generator=g)
        state = []
        for _ in range(2):
            state.append([guarded(n, p0), guarded(n), guarded(n),
                          guarded(n, dtype=torch.bfloat16) if shadow else (None, None)])
        for t in range(1, 4):
            gd, g_full = guarded(n, torch.randn(n, generator=g) * (10.0 ** (t - 2)))
            g_before = gd.clone()
            alpha = optim.keras_alpha(1e-3, 0.9, 0.999, t)
            (p, m, v, lp), (q, mq, vq, lq) = ([x[0] for x in s] for s in state)
            _lib.check(lib.vitmi_adam_step(n, ptr(p), ptr(gd), ptr(m), ptr(v), ptr(lp), alpha, 0.9, 0.999, 1e-7, 0.5,
                                           _stream()), "adam_step")
            _lib.check(lib.vitmi_adam_step_ctl(n, ptr(q), ptr(gd), ptr(mq), ptr(vq), ptr(lq), alpha, 0.9, 0.999, 1e-7,
                                               0.5, 0.0, 1e-3, None, None, _stream()), "adam_step_ctl")
            torch.cuda.synchronize()
            for (a, a_full), (b, b_full) in zip(*state):
                if a is None:
                    continue
                assert torch.equal(int_bits(a), int_bits(b)), (t, shadow)
                assert margins_intact(a_full) and margins_intact(b_full), (t, shadow)
            assert torch.equal(int_bits(gd), int_bits(g_before)) and margins_intact(g_full)    # only read
            if shadow:
                assert torch.equal(int_bits(lp), int_bits(p.to(torch.bfloat16))), t
        assert not torch.equal(state[0][0][0], p0.to(DEV))             # the steps really moved the parameters


def _decayed(p, wd, lr, sel):
    """the three rounded fp32 ops of the decoupled decay, where sel"""
    return np.where(sel, p - (p * f32(wd)) * f32(lr), p).astype(f32)


def test_weight_decay_mask():
    lib = _lib.lib()
    n, wd, lr = 64 * 5 + 3, 0.05, 1e-3
    mask = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    sel = np.repeat(mask, 64)[:n].astype(bool)
    g = torch.Generator().manual_seed(21)
    p0 = torch.randn(n, generator=g)
    maskd = torch.from_numpy(mask).to(DEV)
    for use_mask in (True, False):                      # NULL mask: every group decays
        s = sel if use_mask else np.ones(n, bool)
        ref = (p0.numpy().copy(), np.zeros(n, f32), np.zeros(n, f32))
        plain = ref
        p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        for t in (1, 2):
            gr = torch.randn(n, generator=g)
            gd = gr.to(DEV)
            alpha = optim.keras_alpha(lr, 0.9, 0.999, t)
            before = ref[0]
            _lib.check(lib.vitmi_adam_step_ctl(n, p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), None,
                                               alpha, 0.9, 0.999, 1e-7, 1.0, wd, lr,
                                               maskd.data_ptr() if use_mask else None, None, _stream()),
                       "adam_step_ctl")
            torch.cuda.synchronize()
            ref = optim_ref.adam_step(_decayed(before, wd, lr, s), gr.numpy(), ref[1], ref[2], lr, t)
            plain = optim_ref.adam_step(before, gr.numpy(), plain[1], plain[2], lr, t)
            got = p.cpu().numpy()
            assert np.array_equal(bits(got), bits(ref[0])), (use_mask, t)
            assert np.array_equal(bits(m.cpu().numpy()), bits(ref[1]))
            assert np.array_equal(bits(v.cpu().numpy()), bits(ref[2]))
            # unmasked groups: the plain step; masked ones really moved
            assert np.array_equal(bits(got[~s]), bits(plain[0][~s]))
            assert not np.array_equal(got[s], plain[0][s])


# ------------------------------------------------------------------ skipping
def _tiny_model(seed, num_classes=3, depth=2):
    from vitmi.config import ViTConfig
    from vitmi.modules import VisionTransformer
    cfg = ViTConfig(img_size=32, patch_size=8, in_chans=3, num_classes=num_classes, embed_dim=128, depth=depth,
                    num_heads=2, dtype="bf16")
    model = VisionTransformer(cfg).to(DEV)
    model.reset_parameters(seed=seed)
    return model


def _batch(seed, num_classes=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(4, 3, 32, 32, generator=g).to(DEV), torch.randint(0, num_classes, (4,), generator=g).to(DEV)


def test_skip_nonfinite_step_leaves_everything_unchanged():
    from vitmi.modules import cross_entropy
    model = _tiny_model(31)
    opt = optim.Adam(model, learning_rate=1e-3, skip_nonfinite=True)
    arena = model.arena()
    img, tgt = _batch(32)
    opt.zero_grad()
    cross_entropy(model(img), tgt).backward()
    arena.grad[arena.numel // 2] = float("nan")
    before = [t.clone() for t in (arena.flat, opt._m, opt._v, arena.flat_lp)]
    assert torch.equal(before[3], before[0].to(torch.bfloat16))
    opt.step()
    torch.cuda.synchronize()
    for a, b in zip(before, (arena.flat, opt._m, opt._v, arena.flat_lp)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                           b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))
    assert opt.skipped_steps == 1 and opt.iterations == 1
    # the next, finite step: the oracle at t = 2 on the untouched state
    opt.zero_grad()
    cross_entropy(model(img), tgt).backward()
    grad = arena.grad.cpu().numpy().copy()
    opt.step()
    torch.cuda.synchronize()
    p, m, v = optim_ref.adam_step(before[0].cpu().numpy(), grad, before[1].cpu().numpy(), before[2].cpu().numpy(),
                                  1e-3, 2)
    assert np.array_equal(bits(arena.flat.cpu().numpy()), bits(p))
    assert np.array_equal(bits(opt._m.cpu().numpy()), bits(m))
    assert np.array_equal(bits(opt._v.cpu().numpy()), bits(v))
    assert torch.equal(arena.flat_lp, arena.flat.to(torch.bfloat16))
    assert opt.skipped_steps == 1


@pytest.mark.parametrize("n", [1, 7, 4099])
def test_skip_nonfinite_per_tensor_and_nan_propagation_without_it(n):
    p0 = randn(n, 41)
    gr = randn(n, 42)
    gr[n - 1] = float("nan")
    # skipped
    pd = p0.to(DEV).requires_grad_(True)
    opt = optim.Adam([pd], skip_nonfinite=True, global_clipnorm=1.0)
    pd.grad = gr.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    assert np.array_equal(bits(pd.detach().cpu().numpy()), bits(p0.numpy()))
    assert not opt._m[0].any() and not opt._v[0].any()
    assert opt.skipped_steps == 1
    # not skipped: nothing is hidden, every parameter becomes NaN as in Keras
    qd = p0.to(DEV).requires_grad_(True)
    opt = optim.Adam([qd], global_clipnorm=1.0)
    qd.grad = gr.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    assert torch.isnan(qd.detach()).all()
    assert opt.skipped_steps == 0


# ------------------------------------------------------------------ the arena model
def _decay_selector(model, arena):
    """elementwise decay set from the names: ndim >= 2 except the class token and the position
    embedding (so no bias and no LayerNorm parameter)"""
    sel = np.zeros(arena.numel, bool)
    for name, p in model.named_parameters():
        if p.ndim >= 2 and name not in ("cls_token", "pos_embed"):
            o = arena.offsets[id(p)]
            sel[o:o + p.numel()] = True
    return sel


def test_arena_model_clip_and_weight_decay_bit_exact():
    from vitmi.modules import cross_entropy
    model = _tiny_model(51)
    wd, lr = 0.05, 1e-3
    opt = optim.Adam(model, learning_rate=lr, weight_decay=wd, global_clipnorm=1.0)
    arena = model.arena()
    sel = _decay_selector(model, arena)
    names = dict(model.named_parameters())
    for k in ("cls_token", "pos_embed", "norm.weight", "norm.bias", "head.bias", "blocks.0.mlp.fc1.bias",
              "blocks.1.norm1.weight"):
        o = arena.offsets[id(names[k])]
        assert not sel[o:o + names[k].numel()].any(), k
    assert sel[arena.offsets[id(names["head.weight"])]] and sel[arena.offsets[id(names["blocks.0.mlp.fc1.weight"])]]
    p0 = arena.flat.cpu().numpy().copy()
    m0, v0 = np.zeros_like(p0), np.zeros_like(p0)
    img, tgt = _batch(52)
    for t in (1, 2):
        opt.zero_grad()
        cross_entropy(model(img), tgt).backward()
        grad = arena.grad.cpu().numpy().copy()
        gnorm = float(np.sqrt(np.sum(grad.astype(np.float64) ** 2)))
        if t == 1:
            opt.global_clipnorm = 0.5 * gnorm            # clipping is certainly active
        opt.step()
        torch.cuda.synchronize()
        norm, coef = (x.cpu().numpy() for x in opt.last_clip())
        assert abs(float(norm) - gnorm) <= 1e-6 * gnorm
        if t == 1:
            assert coef < 1.0
        p0, m0, v0 = optim_ref.adam_step(_decayed(p0, wd, lr, sel), grad * f32(coef), m0, v0, lr, t)
        assert np.array_equal(bits(arena.flat.cpu().numpy()), bits(p0)), t
        assert np.array_equal(bits(opt._m.cpu().numpy()), bits(m0))
        assert np.array_equal(bits(opt._v.cpu().numpy()), bits(v0))
        assert torch.equal(arena.flat_lp, arena.flat.to(torch.bfloat16))
    assert set(opt.state_dict()) == {"iterations", "learning_rate", "m", "v"}


def test_arena_frozen_parameter_is_left_out_of_the_norm():
    from vitmi.modules import cross_entropy
    model = _tiny_model(61)
    opt = optim.Adam(model, learning_rate=1e-3, global_clipnorm=1e-3)
    arena = model.arena()
    img, tgt = _batch(62)
    frozen = model.blocks[0].mlp.fc1.weight
    frozen.requires_grad_(False)
    opt.zero_grad()
    cross_entropy(model(img), tgt).backward()
    # whatever the flat gradient buffer holds there must not count
    arena.view(arena.grad, frozen).fill_(100.0)
    grad = arena.grad.cpu().numpy().astype(np.float64)
    o = arena.offsets[id(frozen)]
    grad[o:o + frozen.numel()] = 0.0
    want = float(np.sqrt(np.sum(grad ** 2)))
    before = frozen.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    norm, coef = (x.cpu().numpy() for x in opt.last_clip())
    assert abs(float(norm) - want) <= 1e-6 * want
    assert coef == f32(1e-3) / norm
    assert torch.equal(frozen.detach(), before)
    assert torch.equal(arena.flat_lp, arena.flat.to(torch.bfloat16))


# ------------------------------------------------------------------ reducer and overlap
def _train(steps, reducer=False, overlap=False, **kw):
    from vitmi import dp
    from vitmi.modules import cross_entropy
    model = _tiny_model(71, depth=3)
    red = dp.attach(model, bucket_mb=0.25) if reducer else None
    opt = optim.Adam(model, learning_rate=1e-3, **kw)
    if overlap:
        opt.overlap_with(red)
    arena = model.arena()
    img, tgt = _batch(72)
    side, coefs = [], []
    for _ in range(steps):
        opt.zero_grad()
        if red is not None:
            red.start()
        cross_entropy(model(img), tgt).backward()
        if red is not None:
            red.finish()
        if overlap:
            side.append(opt._ov["done"])
        opt.step()
        if opt._use_ctl():
            coefs.append(float(opt.last_clip()[1].item()))
    torch.cuda.synchronize()
    return (arena.flat.clone(), opt._m.clone(), opt._v.clone(), arena.flat_lp.clone()), side, coefs, arena


def test_reducer_world_1_equals_no_reducer():
    kw = dict(global_clipnorm=0.05, weight_decay=0.05, skip_nonfinite=True)
    a, _, coefs, _ = _train(2, **kw)
    b, _, coefs_b, _ = _train(2, reducer=True, **kw)
    assert all(c < 1.0 for c in coefs) and coefs == coefs_b
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_overlap_refuses_clipping_and_takes_weight_decay():
    from vitmi import dp
    for kw in (dict(global_clipnorm=1.0), dict(skip_nonfinite=True)):
        model = _tiny_model(73)
        red = dp.attach(model, bucket_mb=0.25)
        opt = optim.Adam(model, **kw)
        with pytest.raises(ValueError):
            opt.overlap_with(red)
    a, _, _, _ = _train(3, reducer=True, weight_decay=0.05)
    b, side, _, arena = _train(3, reducer=True, overlap=True, weight_decay=0.05)
    assert all(d == arena.numel for d in side), side      # the buckets really went on the side stream
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    plain, _, _, _ = _train(3, reducer=True)
    assert not torch.equal(plain[0], a[0])                # and the decay really acted
