"""The weight average of the fused Adam step on the MI355X (vitmi_adam_step_ema, vitmi_ema_apply;
vitmi.optim.Adam's use_ema / ema_momentum / ema_overwrite_frequency, swap_ema, ema_weights,
finalize_variable_values; checkpoints; train.fit) against tests/ref_ema.py.

Every comparison is of bits: the average is three rounded fp32 operations after the step's own, so
there is no tolerance to choose.  Every raw call works on buffers that sit 64 elements into a larger
allocation filled with a sentinel pattern, and the pattern is checked afterwards."""
import functools

import numpy as np
import pytest
import torch

import ref_ema
from kstats import kernel_stats
from vitmi import _lib, checkpoint, optim

pytestmark = pytest.mark.gpu

DEV = "cuda"
f32 = np.float32
BF = torch.bfloat16
LR, WD, PAD = 1e-3, 0.05, 64
SMALL = [1, 3, 4, 5, 63, 64, 65, 1027]
# under the 8192-block grid cap (2 097 152 threads, two 16-B groups each): a thread's second group is
# partly in range at the first size, and the grid-stride loop takes a second trip at the second
BIG_PARTIAL, BIG_SECOND_TRIP = 8_388_608 + 1031, 16_777_216 + 1203
VARIANTS = ("plain", "decay", "coef")
MOMS = (0.0, 0.99)          # what ema_momentum_at gives at steps 1 and 2 for ema_momentum = 0.99


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def bf16_bits(a):
    """bf16(a) (round to nearest even, as the kernels' shadow) as int16, on the CPU"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(BF).view(torch.int16)


class Guarded:
    """n elements of fp32 (or bf16) PAD elements into an allocation whose margins hold a pattern."""

    def __init__(self, n, init=None, dtype=torch.float32, seed=0):
        self.n = n
        it = torch.int32 if dtype == torch.float32 else torch.int16
        raw = torch.zeros(n + 2 * PAD, dtype=it)
        pat = (torch.arange(2 * PAD, dtype=torch.int64) * 2654435761 + 977 * seed + 12345) & 0x7FFF
        raw[:PAD], raw[PAD + n:] = pat[:PAD].to(it), pat[PAD:].to(it)
        raw[PAD:PAD + n] = 0x5A5A if init is None else torch.from_numpy(np.ascontiguousarray(init)).view(it)
        self.raw, self.full = raw, raw.to(DEV)
        self.ptr = self.full.data_ptr() + PAD * self.full.element_size()

    def inner(self):
        """the n elements as an integer tensor on the CPU"""
        return self.full.cpu()[PAD:PAD + self.n]

    def numpy(self):
        return self.inner().numpy().view(f32)

    def margins_intact(self):
        got = self.full.cpu()
        return torch.equal(got[:PAD], self.raw[:PAD]) and torch.equal(got[PAD + self.n:], self.raw[PAD + self.n:])


def record(coef, skip=0):
    """the 16-byte device record (coef, norm, skip, skipped_total)"""
    r = np.zeros(4, np.uint32)
    r[0], r[2] = np.array([coef], f32).view(np.uint32)[0], skip
    return torch.from_numpy(r.view(np.int32)).to(DEV)


def alternating_mask(n):
    return (np.arange((n + 63) // 64) % 2 == 0).astype(np.uint8)


@functools.lru_cache(maxsize=2)
def raw_case(n, variant):
    """inputs (p, g1, g2, m, v, e, decay mask) and the reference's (p, m, v, e) after steps 1 and 2"""
    rng = np.random.default_rng(1000 * VARIANTS.index(variant) + n % 1000)
    p, g1, g2, e = (rng.standard_normal(n, dtype=f32) for _ in range(4))
    m = rng.standard_normal(n, dtype=f32) * f32(0.1)
    v = (rng.standard_normal(n, dtype=f32) * f32(0.1)) ** 2
    mask = alternating_mask(n)
    kw = {}
    if variant == "decay":
        kw = dict(wd=WD, sel=np.repeat(mask, 64)[:n].astype(bool))
    elif variant == "coef":
        kw = dict(coef=0.5)
    s1 = ref_ema.adam_ema_step(p, g1, m, v, e, LR, 1, MOMS[0], **kw)
    s2 = ref_ema.adam_ema_step(s1[0], g2, s1[1], s1[2], s1[3], LR, 2, MOMS[1], **kw)
    return (p, g1, g2, m, v, e, mask), (s1, s2)


def step_ema(n, p, g, m, v, lp, e, t, mom, wd=0.0, mask=None, ctl=None):
    alpha = optim.keras_alpha(LR, 0.9, 0.999, t)
    _lib.check(_lib.lib().vitmi_adam_step_ema(
        n, p.ptr, g.ptr, m.ptr, v.ptr, lp.ptr if lp is not None else None, alpha, 0.9, 0.999, 1e-7, 1.0, wd, LR,
        mask.data_ptr() if mask is not None else None, ctl.data_ptr() if ctl is not None else None, e.ptr, mom,
        _stream()), "adam_step_ema")


def step_ctl(n, p, g, m, v, lp, t, wd=0.0, mask=None, ctl=None):
    alpha = optim.keras_alpha(LR, 0.9, 0.999, t)
    _lib.check(_lib.lib().vitmi_adam_step_ctl(
        n, p.ptr, g.ptr, m.ptr, v.ptr, lp.ptr if lp is not None else None, alpha, 0.9, 0.999, 1e-7, 1.0, wd, LR,
        mask.data_ptr() if mask is not None else None, ctl.data_ptr() if ctl is not None else None, _stream()),
        "adam_step_ctl")


def variant_args(variant, mask):
    if variant == "decay":
        return dict(wd=WD, mask=torch.from_numpy(mask).to(DEV))
    if variant == "coef":
        return dict(ctl=record(0.5))
    return {}


# ------------------------------------------------------------------ 1. the raw step
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", SMALL + [BIG_PARTIAL, BIG_SECOND_TRIP])
def test_raw_step_bit_exact(n, variant):
    (p0, g1, g2, m0, v0, e0, mask), (s1, s2) = raw_case(n, variant)
    kw = variant_args(variant, mask)
    for shadow in (False, True):
        p, m, v, e = (Guarded(n, x, seed=i) for i, x in enumerate((p0, m0, v0, e0)))
        ga, gb = Guarded(n, g1, seed=4), Guarded(n, g2, seed=5)
        lp = Guarded(n, dtype=BF, seed=6) if shadow else None
        # the same inputs through the step without the average
        q, mq, vq = (Guarded(n, x, seed=7 + i) for i, x in enumerate((p0, m0, v0)))
        step_ctl(n, q, ga, mq, vq, None, 1, **kw)
        for t, (g, mom, ref) in enumerate(((ga, MOMS[0], s1), (gb, MOMS[1], s2)), start=1):
            step_ema(n, p, g, m, v, lp, e, t, mom, **kw)
            torch.cuda.synchronize()
            for name, buf, want in zip("pmve", (p, m, v, e), ref):
                assert same_bits(buf.numpy(), want), (name, t, shadow)
            if shadow:
                assert torch.equal(lp.inner(), bf16_bits(ref[0])), (t, shadow)
            if t == 1:
                # p, m, v are the plain step's, and momentum 0 gives the new weights as values
                for a, b in ((p, q), (m, mq), (v, vq)):
                    assert torch.equal(a.inner(), b.inner())
                assert np.array_equal(e.numpy(), p.numpy())
        for buf in (p, m, v, e, ga, gb, q, mq, vq) + ((lp,) if shadow else ()):
            assert buf.margins_intact()
        assert same_bits(ga.numpy(), g1) and same_bits(gb.numpy(), g2)        # the gradients are only read


# ------------------------------------------------------------------ 2. a skipped step
@pytest.mark.parametrize("n", [5, 1027])
def test_skipped_step_leaves_everything(n):
    (p0, g1, _, m0, v0, e0, mask), _ = raw_case(n, "decay")
    p, g, m, v, e = (Guarded(n, x, seed=i) for i, x in enumerate((p0, g1, m0, v0, e0)))
    lp = Guarded(n, dtype=BF, seed=5)
    step_ema(n, p, g, m, v, lp, e, 2, 0.99, wd=WD, mask=torch.from_numpy(mask).to(DEV), ctl=record(0.5, skip=1))
    torch.cuda.synchronize()
    for buf, want in ((p, p0), (g, g1), (m, m0), (v, v0), (e, e0)):
        assert same_bits(buf.numpy(), want) and buf.margins_intact()
    assert torch.equal(lp.inner(), bf16_bits(p0)) and lp.margins_intact()


# ------------------------------------------------------------------ 3. guards
@pytest.mark.parametrize("n", [5, 1027])
def test_step_writes_nothing_outside_its_range(n):
    """decay mask and clip record together; every byte outside [0, n) of all six buffers stays"""
    (p0, g1, _, m0, v0, e0, mask), _ = raw_case(n, "decay")
    sel = np.repeat(mask, 64)[:n].astype(bool)
    want = ref_ema.adam_ema_step(p0, g1, m0, v0, e0, LR, 2, 0.9, coef=0.5, wd=WD, sel=sel)
    p, g, m, v, e = (Guarded(n, x, seed=i) for i, x in enumerate((p0, g1, m0, v0, e0)))
    lp = Guarded(n, dtype=BF, seed=5)
    step_ema(n, p, g, m, v, lp, e, 2, 0.9, wd=WD, mask=torch.from_numpy(mask).to(DEV), ctl=record(0.5))
    torch.cuda.synchronize()
    for buf in (p, g, m, v, e, lp):
        assert buf.margins_intact()
    for buf, w in zip((p, m, v, e), want):
        assert same_bits(buf.numpy(), w)
    assert torch.equal(lp.inner(), bf16_bits(want[0]))


# ------------------------------------------------------------------ 4. swap / copy
def apply(n, p, e, lp, mode):
    _lib.check(_lib.lib().vitmi_ema_apply(n, p.ptr, e.ptr, lp.ptr if lp is not None else None, mode, _stream()),
               "ema_apply")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shadow", [False, True], ids=["fp32", "shadow"])
@pytest.mark.parametrize("n", SMALL + [BIG_PARTIAL])
def test_ema_apply_swap_and_copy(n, shadow):
    (p0, _, _, _, _, e0, _), _ = raw_case(n, "plain")
    p, e = Guarded(n, p0, seed=1), Guarded(n, e0, seed=2)
    lp = Guarded(n, dtype=BF, seed=3) if shadow else None
    bufs = (p, e) + ((lp,) if shadow else ())
    apply(n, p, e, lp, 0)                                   # exchange
    assert same_bits(p.numpy(), e0) and same_bits(e.numpy(), p0)
    assert not shadow or torch.equal(lp.inner(), bf16_bits(e0))
    assert all(b.margins_intact() for b in bufs)
    apply(n, p, e, lp, 0)                                   # and back
    assert same_bits(p.numpy(), p0) and same_bits(e.numpy(), e0)
    assert not shadow or torch.equal(lp.inner(), bf16_bits(p0))
    apply(n, p, e, lp, 1)                                   # p <- ema
    assert same_bits(p.numpy(), e0) and same_bits(e.numpy(), e0)
    assert not shadow or torch.equal(lp.inner(), bf16_bits(e0))
    assert all(b.margins_intact() for b in bufs)


# ------------------------------------------------------------------ 5. launch records
def kname(base, *flags):
    """The kernel's name as recorded: mangled or demangled (tests/test_gpu_launch_stats.py)."""
    return (base + "I" + "".join(f"Lb{int(a)}E" for a in flags) + "E",
            base + "<" + ", ".join("true" if a else "false" for a in flags) + ">")


def assert_recorded(st, forms, work, what):
    got = dict(st.work)
    print(f"{what}: {got}")
    hits = [k for k in got if any(f in k for f in forms)]
    assert len(hits) == 1 and len(got) == 1, (what, forms, got)
    assert got[hits[0]] == work, (what, got, work)


@pytest.mark.parametrize("shadow", [False, True], ids=["fp32", "shadow"])
def test_launch_records(shadow):
    n = 1000
    gen = torch.Generator().manual_seed(1)
    p, g, m, v, e = (torch.randn(n, generator=gen).abs().to(DEV) for _ in range(5))
    lp = torch.empty(n, dtype=BF, device=DEV) if shadow else None
    P = lambda t: t.data_ptr() if t is not None else None    # noqa: E731
    mask, ctl = torch.ones((n + 63) // 64, dtype=torch.uint8, device=DEV), record(1.0)
    per = 38 if shadow else 36
    # p, g, m, v, ema read; p, m, v, ema (+ the bf16 shadow) written; plus the mask bytes and the record
    for wd, mk, ct, extra in ((0.0, None, None, 0), (WD, mask, ctl, (n + 63) // 64 + 16)):
        with kernel_stats() as st:
            _lib.check(_lib.lib().vitmi_adam_step_ema(n, P(p), P(g), P(m), P(v), P(lp), 1e-3, 0.9, 0.999, 1e-7, 1.0, wd,
                                                      LR, P(mk), P(ct), P(e), 0.99, _stream()), "adam_step_ema")
        torch.cuda.synchronize()
        assert_recorded(st, kname("adam_kernel", shadow, True, True), (1, 0.0, float(n * per + extra)),
                        f"adam ema shadow {shadow} extra {extra}")
    # swap: p and ema read and written; copy: ema read, p written
    for mode, by in ((0, 16), (1, 8)):
        with kernel_stats() as st:
            _lib.check(_lib.lib().vitmi_ema_apply(n, P(p), P(e), P(lp), mode, _stream()), "ema_apply")
        torch.cuda.synchronize()
        assert_recorded(st, kname("ema_apply_kernel", shadow, mode == 0),
                        (1, 0.0, float(n * (by + (2 if shadow else 0)))), f"ema apply shadow {shadow} mode {mode}")


# ------------------------------------------------------------------ 6. Adam on a small ViT
def tiny_vit(dtype, seed=11):
    """image 32, patch 16, depth 2, 2 heads; width 128, the narrowest the attention kernels take
    with 2 heads (head_dim is 64)"""
    from vitmi.config import ViTConfig
    from vitmi.modules import VisionTransformer
    cfg = ViTConfig(img_size=32, patch_size=16, in_chans=3, num_classes=3, embed_dim=128, depth=2, num_heads=2,
                    dtype=dtype)
    model = VisionTransformer(cfg).to(DEV)
    model.reset_parameters(seed=seed)
    return model


def batch(seed=12):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(4, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 3, (4,), generator=g).to(DEV)


def backward(model, opt, red=None):
    from vitmi.modules import cross_entropy
    img, tgt = batch()
    opt.zero_grad()
    if red is not None:
        red.start()
    cross_entropy(model(img), tgt).backward()
    if red is not None:
        red.finish()


def train_vit(dtype, steps=3, overlap=False, **kw):
    """-> (flat, m, v, ema, shadow) after `steps` steps, the gradients of each step, model, optimizer"""
    from vitmi import dp
    model = tiny_vit(dtype)
    red = dp.attach(model, bucket_mb=0.25) if overlap else None
    opt = optim.Adam(model, learning_rate=LR, use_ema=True, **kw)
    if overlap:
        opt.overlap_with(red)
    arena, grads, side = model.arena(), [], []
    for _ in range(steps):
        backward(model, opt, red)
        grads.append(arena.grad.cpu().numpy().copy())
        if overlap:
            side.append(opt._ov["done"])
        opt.step()
    torch.cuda.synchronize()
    if overlap:
        assert len(red.bounds) >= 4 and all(d == arena.numel for d in side), side    # really on the side stream
    lp = arena.flat_lp.clone() if arena.flat_lp is not None else None
    return (arena.flat.clone(), opt._m.clone(), opt._v.clone(), opt._ema.clone(), lp), grads, model, opt


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_adam_on_a_small_vit_follows_the_reference(dtype):
    model = tiny_vit(dtype)
    opt = optim.Adam(model, learning_rate=LR, use_ema=True, ema_momentum=0.9)
    arena = model.arena()
    p = arena.flat.cpu().numpy().copy()
    m, v, e = np.zeros_like(p), np.zeros_like(p), p.copy()
    assert same_bits(opt._ema.cpu().numpy(), p)                       # starts as a copy of the parameters
    for t in (1, 2, 3):
        backward(model, opt)
        grad = arena.grad.cpu().numpy().copy()
        opt.step()
        torch.cuda.synchronize()
        p, m, v, e = ref_ema.adam_ema_step(p, grad, m, v, e, LR, t, ref_ema.momentum_at(t, 0.9))
        avg = opt.ema_parameters()
        for name, prm in model.named_parameters():
            o = arena.offsets[id(prm)]
            assert avg[name].shape == prm.shape and avg[name].data_ptr() == opt._ema.data_ptr() + 4 * o   # a view
            assert same_bits(avg[name].cpu().numpy().ravel(), e[o:o + prm.numel()]), (name, t)
            assert same_bits(prm.detach().cpu().numpy().ravel(), p[o:o + prm.numel()]), (name, t)
        assert same_bits(opt._m.cpu().numpy(), m) and same_bits(opt._v.cpu().numpy(), v)
        if arena.flat_lp is not None:
            assert torch.equal(arena.flat_lp, arena.flat.to(BF))
    assert not same_bits(e, p)                                        # the average really lags


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_overlap_gives_the_same_bits(dtype):
    mom = lambda t: min(0.99, t / (t + 2.0))                  # noqa: E731  (read with alpha and lr at the first bucket)
    a, _, _, _ = train_vit(dtype, ema_momentum=mom, weight_decay=WD)
    b, _, _, _ = train_vit(dtype, overlap=True, ema_momentum=mom, weight_decay=WD)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x.view(torch.int16 if x.dtype == BF else torch.int32),
                                                        y.view(torch.int16 if y.dtype == BF else torch.int32))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_frozen_parameter_keeps_its_average(dtype):
    model = tiny_vit(dtype)
    frozen = model.blocks[0].mlp.fc1.weight
    with torch.no_grad():
        frozen.add_(0.5)                                              # parameters and average differ from here
    opt = optim.Adam(model, learning_rate=LR, use_ema=True, ema_momentum=0.5)
    arena = model.arena()
    first = opt._ema.clone()
    with torch.no_grad():
        frozen.sub_(0.25)
    frozen.requires_grad_(False)
    for _ in range(2):
        backward(model, opt)
        opt.step()
    torch.cuda.synchronize()
    o, n = arena.offsets[id(frozen)], frozen.numel()
    assert torch.equal(opt._ema[o:o + n].view(torch.int32), first[o:o + n].view(torch.int32))
    assert not torch.equal(opt._ema[o:o + n], arena.flat[o:o + n])    # not averaged towards the weights either
    moved = model.blocks[1].mlp.fc1.weight
    o2 = arena.offsets[id(moved)]
    assert not torch.equal(opt._ema[o2:o2 + moved.numel()], first[o2:o2 + moved.numel()])
    if arena.flat_lp is not None:
        assert torch.equal(arena.flat_lp, arena.flat.to(BF))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_nonfinite_step_leaves_the_average(dtype):
    model = tiny_vit(dtype)
    opt = optim.Adam(model, learning_rate=LR, use_ema=True, ema_momentum=0.9, skip_nonfinite=True)
    arena = model.arena()
    for _ in range(2):
        backward(model, opt)
        opt.step()
    backward(model, opt)
    arena.grad[arena.numel // 2] = float("nan")
    before = [t.clone() for t in (arena.flat, opt._m, opt._v, opt._ema)]
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps == 1 and opt.iterations == 3
    for a, b in zip(before, (arena.flat, opt._m, opt._v, opt._ema)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(opt._ema, arena.flat)
    # the next, finite step follows the reference at t = 4 from the untouched state
    backward(model, opt)
    grad = arena.grad.cpu().numpy().copy()
    opt.step()
    torch.cuda.synchronize()
    want = ref_ema.adam_ema_step(*(t.cpu().numpy() for t in before[:1]), grad,
                                 *(t.cpu().numpy() for t in before[1:]), LR, 4, ref_ema.momentum_at(4, 0.9))
    for got, w in zip((arena.flat, opt._m, opt._v, opt._ema), want):
        assert same_bits(got.cpu().numpy(), w)


# ------------------------------------------------------------------ 7. ema_weights()
def logits_of(model):
    with torch.no_grad():
        out = model(batch(13)[0]).clone()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_ema_weights_context(dtype):
    model = tiny_vit(dtype)
    opt = optim.Adam(model, learning_rate=1e-2, use_ema=True, ema_momentum=0.5)
    arena = model.arena()
    for _ in range(3):
        backward(model, opt)
        opt.step()
    model.eval()
    other = tiny_vit(dtype, seed=99).eval()
    other.load_param_dict({k: t.clone() for k, t in opt.ema_parameters().items()})
    want_in = logits_of(other)
    p_before, e_before, out_before = arena.flat.clone(), opt._ema.clone(), logits_of(model)
    assert not torch.equal(want_in, out_before)
    with opt.ema_weights() as same:
        assert same is opt
        assert torch.equal(arena.flat.view(torch.int32), e_before.view(torch.int32))
        assert torch.equal(logits_of(model), want_in)                 # the shadow was swapped too
        for call in (opt.step, opt.state_dict, opt.swap_ema, lambda: opt.load_state_dict({})):
            with pytest.raises(RuntimeError):
                call()
        with pytest.raises(RuntimeError):
            with opt.ema_weights():
                pass
        assert torch.equal(arena.flat.view(torch.int32), e_before.view(torch.int32))    # still swapped in
    assert torch.equal(arena.flat.view(torch.int32), p_before.view(torch.int32))
    assert torch.equal(opt._ema.view(torch.int32), e_before.view(torch.int32))
    assert torch.equal(logits_of(model), out_before)
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("inside")
    assert torch.equal(arena.flat.view(torch.int32), p_before.view(torch.int32))
    assert torch.equal(opt._ema.view(torch.int32), e_before.view(torch.int32))
    assert torch.equal(logits_of(model), out_before)
    # swap_ema on its own, twice
    opt.swap_ema()
    assert torch.equal(logits_of(model), want_in)
    opt.swap_ema()
    assert torch.equal(arena.flat.view(torch.int32), p_before.view(torch.int32))
    assert torch.equal(logits_of(model), out_before)
    model.train()
    backward(model, opt)
    opt.step()                                                        # and training goes on


# ------------------------------------------------------------------ 8. overwrite frequency, finalize
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_overwrite_frequency_and_finalize(dtype):
    model = tiny_vit(dtype)
    lr = 1e-2
    opt = optim.Adam(model, learning_rate=lr, use_ema=True, ema_momentum=0.5, ema_overwrite_frequency=2)
    arena = model.arena()

    def check_overwritten():
        torch.cuda.synchronize()
        assert torch.equal(arena.flat.view(torch.int32), opt._ema.view(torch.int32))
        # the next forward computes with them: a model loaded with the same values gives the same logits
        other = tiny_vit(dtype, seed=98).eval()
        other.load_param_dict({k: t.clone() for k, t in opt.ema_parameters().items()})
        model.eval()
        assert torch.equal(logits_of(model), logits_of(other))
        model.train()
        if arena.flat_lp is not None:
            assert torch.equal(arena.flat_lp, arena.flat.to(BF))

    backward(model, opt)
    opt.step()
    backward(model, opt)
    grad = arena.grad.cpu().numpy().copy()
    state = [t.cpu().numpy().copy() for t in (arena.flat, opt._m, opt._v, opt._ema)]
    opt.step()                                                        # t = 2: overwritten
    check_overwritten()
    want = ref_ema.adam_ema_step(state[0], grad, state[1], state[2], state[3], lr, 2, 0.5)
    assert same_bits(opt._ema.cpu().numpy(), want[3]) and not same_bits(want[0], want[3])
    backward(model, opt)
    opt.step()                                                        # t = 3: not overwritten
    torch.cuda.synchronize()
    assert not torch.equal(arena.flat, opt._ema)
    e3 = opt._ema.clone()
    opt.finalize_variable_values()
    check_overwritten()
    assert torch.equal(opt._ema.view(torch.int32), e3.view(torch.int32))          # the average stays


# ------------------------------------------------------------------ 9. checkpoints
class ThreeTensors(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a, self.b, self.c = (torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 64, 1027))


def list_steps(mod, opt, steps, seed=21):
    g = torch.Generator().manual_seed(seed)
    grads = []
    for _ in range(steps):
        gs = [torch.randn(p.numel(), generator=g) for p in opt.params]
        for p, x in zip(opt.params, gs):
            p.grad = x.to(DEV)
        opt.step()
        grads.append([x.numpy() for x in gs])
    torch.cuda.synchronize()
    return grads


def test_checkpoint_restores_the_average_arena(tmp_path):
    (_, _, _, ema, _), _, model, opt = train_vit("bf16", steps=2, ema_momentum=0.9)
    ck = str(tmp_path / "w.safetensors")
    checkpoint.save_weights(model, ck, optimizer=opt)
    m2 = tiny_vit("bf16", seed=97)
    o2 = optim.Adam(m2, use_ema=True)
    checkpoint.load_weights(m2, ck, optimizer=o2)
    assert o2.iterations == 2
    assert torch.equal(o2._ema.view(torch.int32), ema.view(torch.int32))
    assert torch.equal(o2._m, opt._m) and torch.equal(m2.arena().flat, model.arena().flat)
    assert not torch.equal(o2._ema, m2.arena().flat)
    # written without an average, loaded into an optimizer that keeps one: it starts from the loaded weights
    plain = optim.Adam(model)
    ck0 = str(tmp_path / "plain.safetensors")
    checkpoint.save_weights(model, ck0, optimizer=plain)
    m3 = tiny_vit("bf16", seed=96)
    o3 = optim.Adam(m3, use_ema=True)
    assert not torch.equal(o3._ema, model.arena().flat)
    checkpoint.load_weights(m3, ck0, optimizer=o3)
    assert torch.equal(o3._ema.view(torch.int32), model.arena().flat.view(torch.int32))
    # and the other way round: the average in the file is ignored
    o4 = optim.Adam(tiny_vit("bf16", seed=95))
    checkpoint.load_weights(o4._model, ck, optimizer=o4)
    assert o4._ema is None and o4.iterations == 2


def test_checkpoint_restores_the_average_list(tmp_path):
    mod = ThreeTensors(31).to(DEV)
    opt = optim.Adam(list(mod.parameters()), use_ema=True, ema_momentum=0.9)
    list_steps(mod, opt, 2)
    ck = str(tmp_path / "l.safetensors")
    checkpoint.save_weights(mod, ck, optimizer=opt)
    mod2 = ThreeTensors(32).to(DEV)
    o2 = optim.Adam(list(mod2.parameters()), use_ema=True)
    checkpoint.load_weights(mod2, ck, optimizer=o2)
    for a, b, p in zip(o2.ema_parameters(), opt.ema_parameters(), mod2.parameters()):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, p.detach())
    plain = optim.Adam(list(mod.parameters()))
    ck0 = str(tmp_path / "plain.safetensors")
    checkpoint.save_weights(mod, ck0, optimizer=plain)
    mod3 = ThreeTensors(33).to(DEV)
    o3 = optim.Adam(list(mod3.parameters()), use_ema=True)
    checkpoint.load_weights(mod3, ck0, optimizer=o3)
    for e, p in zip(o3.ema_parameters(), mod.parameters()):
        assert torch.equal(e.view(torch.int32), p.detach().view(torch.int32))


# ------------------------------------------------------------------ 10. the list path and fit
def test_list_path_follows_the_reference():
    mod = ThreeTensors(41).to(DEV)
    mom = lambda t: min(0.99, (1 + t) / (10 + t))                     # noqa: E731
    opt = optim.Adam(list(mod.parameters()), learning_rate=LR, use_ema=True, ema_momentum=mom)
    ref = [(p.detach().cpu().numpy().copy(), np.zeros(p.numel(), f32), np.zeros(p.numel(), f32),
            p.detach().cpu().numpy().copy()) for p in opt.params]
    versions = [p._version for p in opt.params]
    for t, gs in enumerate(list_steps(mod, opt, 3), start=1):
        ref = [ref_ema.adam_ema_step(p, g, m, v, e, LR, t, ref_ema.momentum_at(t, mom))
               for (p, m, v, e), g in zip(ref, gs)]
    for prm, m, v, e, (rp, rm, rv, re) in zip(opt.params, opt._m, opt._v, opt.ema_parameters(), ref):
        assert same_bits(prm.detach().cpu().numpy(), rp) and same_bits(e.cpu().numpy(), re)
        assert same_bits(m.cpu().numpy(), rm) and same_bits(v.cpu().numpy(), rv)
    # swap on the list path: exchanged, and the version counters move as in step()
    versions = [p._version for p in opt.params]
    opt.swap_ema()
    torch.cuda.synchronize()
    for prm, e, (rp, _, _, re), ver in zip(opt.params, opt.ema_parameters(), ref, versions):
        assert same_bits(prm.detach().cpu().numpy(), re) and same_bits(e.cpu().numpy(), rp)
        assert prm._version > ver
    opt.swap_ema()
    opt.finalize_variable_values()
    torch.cuda.synchronize()
    for prm, (_, _, _, re) in zip(opt.params, ref):
        assert same_bits(prm.detach().cpu().numpy(), re)


def test_fit_leaves_the_averaged_weights():
    from vitmi import cvt, sls, train
    cfg = cvt.CvTConfig(img_size=64, num_classes=1, proc_dim=5, dtype="fp32",      # tests/test_gpu_sls.py's tiny CvT
                        stages=[cvt.CvTStage(64, 7, 4, 1, qkv_method="dw_bn"),
                                cvt.CvTStage(128, 3, 2, 2, qkv_method="dw_bn", with_cls_token=True)])
    ds = sls.SLSDataset.synthetic(n_pieces=10, image_layers=6, height=64, width=64, device=DEV)
    torch.manual_seed(0)
    model = cvt.CvT(cfg).to(DEV)
    model.reset_parameters(1)
    opt = optim.Adam(list(model.parameters()), learning_rate=1e-3, use_ema=True, ema_momentum=0.9)
    train.fit(model, ds, epochs=2, batch_size=16, optimizer=opt, seed=1, validate=False)
    torch.cuda.synchronize()
    assert opt.iterations == 2 * ((len(ds.train_rows) + 15) // 16) and opt.iterations > 2
    moved = 0
    for p, e, m in zip(opt.params, opt.ema_parameters(), opt._m):
        assert torch.equal(p.detach().view(torch.int32), e.view(torch.int32))
        moved += int(m.abs().sum().item() > 0)
    assert moved > 0
