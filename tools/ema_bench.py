"""Time the weight average of the Adam step at the ViT-B/16 arena size (85.8 M fp32 elements, bf16
shadow), three alternating rounds in one process:
  (a) ``Adam.step()`` without the average followed by ``ema.lerp_(arena.flat, 1 - momentum)``
      (what a user did before ``use_ema``; the reference for time),
  (b) ``Adam.step()`` with ``use_ema``,
  (c) the two kernels alone (vitmi_adam_step_ema; vitmi_ema_apply swap and copy) with the TB/s of
      the bytes they state,
  (d) ``swap_ema()`` against the torch sequence: three copies through a temporary, plus the cast.
Device events around 30 back-to-back calls after 5 warm-up calls, as tools/optim_bench.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-stm_amd"))
import torch  # noqa: E402

from vitmi import ops, optim  # noqa: E402
from vitmi._lib import check, lib  # noqa: E402
from vitmi.config import ViTConfig  # noqa: E402
from vitmi.modules import VisionTransformer  # noqa: E402

MOM = 0.9999


def t(fn, iters=30):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


model = VisionTransformer(ViTConfig()).to("cuda")
arena = model.arena()
n = arena.numel
gen = torch.Generator(device="cuda").manual_seed(0)
arena.bind_grads()
arena.grad.normal_(generator=gen).mul_(1e-3)
m, v, ema = torch.zeros_like(arena.flat), torch.zeros_like(arena.flat), arena.flat.clone()
print(f"arena {n} elements, library {os.environ.get('VITMI_LIB') or 'vitmi/libvitmi.so'}", flush=True)


def step_then_lerp(opt):
    opt.step()
    ema.lerp_(arena.flat, 1.0 - MOM)


def torch_swap():
    tmp = arena.flat.clone()
    arena.flat.copy_(ema)
    ema.copy_(tmp)
    arena.flat_lp.copy_(arena.flat)


rounds = []
for r in range(3):          # alternate the variants: the spread between rounds is the noise
    row = {}
    plain = optim.Adam(model, learning_rate=1e-6)
    row["(a) step + lerp_"] = t(lambda: step_then_lerp(plain))
    del plain
    fused = optim.Adam(model, learning_rate=1e-6, use_ema=True, ema_momentum=MOM)
    row["(b) step use_ema"] = t(fused.step)
    row["(c) ema step kernel"] = t(lambda: check(lib().vitmi_adam_step_ema(
        n, ops._p(arena.flat), ops._p(arena.grad), ops._p(m), ops._p(v), ops._p(arena.flat_lp), 1e-6, 0.9, 0.999,
        1e-7, 1.0, 0.0, 1e-6, None, None, ops._p(ema), MOM, ops._s())))
    row["(c) swap kernel"] = t(lambda: check(lib().vitmi_ema_apply(n, ops._p(arena.flat), ops._p(ema),
                                                                   ops._p(arena.flat_lp), 0, ops._s())))
    row["(c) copy kernel"] = t(lambda: check(lib().vitmi_ema_apply(n, ops._p(arena.flat), ops._p(ema),
                                                                   ops._p(arena.flat_lp), 1, ops._s())))
    row["(d) swap_ema()"] = t(fused.swap_ema)
    row["(d) torch swap"] = t(torch_swap)
    del fused
    rounds.append(row)
    print("  ".join(f"{k} {x:7.1f} us" for k, x in row.items()), flush=True)

best = {k: min(r[k] for r in rounds) for k in rounds[0]}
for k, by in (("(c) ema step kernel", 38), ("(c) swap kernel", 18), ("(c) copy kernel", 10)):
    print(f"{k:20s} {best[k]:7.1f} us ({n * by / best[k] / 1e6:5.2f} TB/s of {by} B per element)")
print(f"step: (a) {best['(a) step + lerp_']:7.1f} us, (b) {best['(b) step use_ema']:7.1f} us; "
      f"(b) faster in {sum(r['(b) step use_ema'] < r['(a) step + lerp_'] for r in rounds)} of {len(rounds)} rounds")
print(f"swap: swap_ema() {best['(d) swap_ema()']:7.1f} us, torch {best['(d) torch swap']:7.1f} us", flush=True)
