"""Time the optimizer step at the ViT-B/16 arena size (85.8 M fp32 elements, bf16 shadow):
the Adam kernel alone, the gradient sum-of-squares kernel alone, the finalize launch, and
``Adam.step()`` plain / with ``global_clipnorm`` / with clipping, weight decay and skipping.
Device events around back-to-back calls after a warm-up, as tools/ln_bench.py times the Adam
kernel; every figure comes from the same process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-stm_amd"))
import torch  # noqa: E402

from vitmi import ops, optim  # noqa: E402
from vitmi._lib import check, lib  # noqa: E402
from vitmi.config import ViTConfig  # noqa: E402
from vitmi.modules import VisionTransformer  # noqa: E402


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
m, v = torch.zeros_like(arena.flat), torch.zeros_like(arena.flat)
part = torch.zeros(lib().vitmi_grad_sumsq_partials(n), dtype=torch.float64, device="cuda")
ctl = torch.zeros(4, device="cuda")
print(f"arena {n} elements, chunks {part.numel()}", flush=True)

rounds = []
for r in range(3):          # alternate the variants: the spread between rounds is the noise
    row = {}
    row["adam kernel"] = t(lambda: check(lib().vitmi_adam_step(
        n, ops._p(arena.flat), ops._p(arena.grad), ops._p(m), ops._p(v), ops._p(arena.flat_lp), 1e-6, 0.9, 0.999,
        1e-7, 1.0, ops._s())))
    row["sumsq kernel"] = t(lambda: check(lib().vitmi_grad_sumsq(n, ops._p(arena.grad), ops._p(part), ops._s())))
    row["finalize"] = t(lambda: check(lib().vitmi_clip_finalize(part.numel(), ops._p(part), 1.0, 1.0, 1, ops._p(ctl),
                                                                ops._s())))
    for name, kw in (("step plain", {}), ("step clip", dict(global_clipnorm=1.0)),
                     ("step clip+decay+skip", dict(global_clipnorm=1.0, weight_decay=0.05, skip_nonfinite=True))):
        opt = optim.Adam(model, learning_rate=1e-6, **kw)
        row[name] = t(opt.step)
        del opt
    rounds.append(row)
    print("  ".join(f"{k} {x:7.1f} us" for k, x in row.items()), flush=True)

best = {k: min(r[k] for r in rounds) for k in rounds[0]}
print(f"adam kernel  {best['adam kernel']:7.1f} us ({n * 30 / best['adam kernel'] / 1e3:6.0f} GB/s)")
print(f"sumsq kernel {best['sumsq kernel']:7.1f} us ({n * 4 / best['sumsq kernel'] / 1e3:6.0f} GB/s)")
print(f"step: plain {best['step plain']:7.1f} us, clip {best['step clip']:7.1f} us, "
      f"clip+decay+skip {best['step clip+decay+skip']:7.1f} us", flush=True)
