"""Time patch dropout at the benchmark's shapes.

(a) A full ViT-B/16 224 bs 256 bf16 forward + backward + Adam step at patch_drop_rate 0 / 0.25 / 0.5 /
    0.75, next to the FLOP ratio flops_per_image_fwd(kept_patches=K) / flops_per_image_fwd().
(b) The embed stage alone at the same rates: forward (im2col, patch GEMM, cls + pos-embed) and
    backward (token split, position / cls sums, weight and bias gradients); at rate 0 the full
    entry points, otherwise the gathered ones with a fixed subset.
(c) vitmi_patch_keep alone at (B, np) = (256, 196) and (64, 576), K = np / 2.

Device events around back-to-back calls after a warm-up; each figure is the median of several such
windows with its min .. max, and the variants alternate within a round so that drift hits them
alike (as tools/droppath_bench.py).  Every figure comes from the same process and the same build.
``--only a`` / ``b`` / ``c`` runs one part."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-stm_amd"))
import torch  # noqa: E402

from vitmi import ops, optim  # noqa: E402
from vitmi.config import config_c3  # noqa: E402
from vitmi.modules import VisionTransformer, cross_entropy  # noqa: E402

RATES = (0.0, 0.25, 0.5, 0.75)
SEED = 7


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def measure(variants, rounds, iters, warmup):
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    return times


def report(title, times, base, extra=None):
    print(title)
    b = statistics.median(times[base])
    for k, v in times.items():
        m = statistics.median(v)
        tail = f"  {extra[k]}" if extra else ""
        print(f"  {k:34s} {m:10.1f} us  ({min(v):.1f} .. {max(v):.1f})  x{m / b:5.3f} of {base}{tail}")


def part_a(rounds, steps):
    B = 256
    models, extra = {}, {}
    full = config_c3().flops_per_image_fwd()
    for rate in RATES:
        name = f"patch_drop_rate {rate}"
        torch.manual_seed(0)
        cfg = config_c3(patch_drop_rate=rate)
        model = VisionTransformer(cfg).to("cuda").train()
        model.reset_parameters(seed=0)
        models[name] = (model, optim.Adam(model, learning_rate=1e-6), list(model.arena().params))
        extra[name] = f"K {cfg.kept_patches:3d}  FLOP ratio {cfg.flops_per_image_fwd(cfg.kept_patches) / full:.3f}"
    gen = torch.Generator(device="cuda").manual_seed(1234)
    img = torch.rand(B, 3, 224, 224, device="cuda", generator=gen)
    tgt = torch.randint(0, 2, (B,), device="cuda", generator=gen)

    def step(name):
        model, opt, params = models[name]

        def run():
            for p in params:
                p.grad = None
            cross_entropy(model(img), tgt).backward()
            opt.step()
        return run

    times = measure({k: step(k) for k in models}, rounds, steps, 3)
    report(f"(a) ViT-B/16 224 bs {B} bf16 fwd + bwd + Adam; {rounds} rounds x {steps} steps, alternating; "
           "median (min .. max)", times, "patch_drop_rate 0.0", extra)
    for k, v in times.items():
        print(f"  {k}: {statistics.median(v) / 1e3:.2f} ms/step, {B / statistics.median(v) * 1e6:.0f} img/s")
    return times


def part_b(rounds, iters):
    B, C, S, P, D = 256, 3, 224, 16, 768
    np_ = (S // P) ** 2
    T = torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(0)
    img = torch.rand(B, C, S, S, device="cuda", generator=gen)
    w = (0.02 * torch.randn(D, C * P * P, device="cuda", generator=gen)).to(T)
    bias = 0.02 * torch.randn(D, device="cuda", generator=gen)
    cls = 0.02 * torch.randn(D, device="cuda", generator=gen)
    pos = 0.02 * torch.randn((np_ + 1) * D, device="cuda", generator=gen)
    grads = [torch.zeros(D, C * P * P, device="cuda"), torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda"),
             torch.zeros((np_ + 1) * D, device="cuda")]
    fwd, bwd = {}, {}
    for rate in RATES:
        K = config_c3(patch_drop_rate=rate).kept_patches
        dx = torch.randn(B, K + 1, D, device="cuda", generator=gen)
        if K == np_:
            _, patches = ops.patch_embed_fwd(img, w, bias, cls, pos, P, T)
            fwd[f"embed fwd rate {rate}"] = lambda: ops.patch_embed_fwd(img, w, bias, cls, pos, P, T)
            bwd[f"embed bwd rate {rate}"] = (lambda dx=dx, patches=patches:
                                             ops.patch_embed_bwd(dx, patches, B, C, S, P, *grads))
        else:
            keep, slot = ops.patch_keep(B, np_, K, SEED)
            _, patches = ops.patch_embed_keep_fwd(img, w, bias, cls, pos, P, keep, T)
            fwd[f"embed fwd rate {rate}"] = lambda keep=keep: ops.patch_embed_keep_fwd(img, w, bias, cls, pos, P, keep, T)
            bwd[f"embed bwd rate {rate}"] = (lambda dx=dx, patches=patches, slot=slot:
                                             ops.patch_embed_keep_bwd(dx, patches, slot, C, S, P, *grads))
    head = f"ViT-B/16 224 bs {B} bf16; {rounds} rounds x {iters} calls, alternating; median (min .. max)"
    report("(b) embed stage forward, " + head, measure(fwd, rounds, iters, 10), "embed fwd rate 0.0")
    report("(b) embed stage backward, " + head, measure(bwd, rounds, iters, 10), "embed bwd rate 0.0")


def part_c(rounds, iters, step_us=None):
    variants = {}
    for B, np_ in ((256, 196), (64, 576)):
        variants[f"patch_keep B {B} np {np_} K {np_ // 2}"] = (lambda B=B, np_=np_:
                                                              ops.patch_keep(B, np_, np_ // 2, SEED))
    times = measure(variants, rounds, iters, 10)
    first = next(iter(times))
    report(f"(c) vitmi_patch_keep (with its two output allocations); {rounds} rounds x {iters} calls, alternating; "
           "median (min .. max)", times, first)
    if step_us is not None:
        print(f"  {first}: {100 * statistics.median(times[first]) / step_us:.3f} % of the rate-0.5 step")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="steps per window of part (a)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patchdrop_bench: needs the GPU (no CPU timing)")
    step_us = None
    if args.only in (None, "a"):
        step_us = statistics.median(part_a(args.rounds, args.steps)["patch_drop_rate 0.5"])
    if args.only in (None, "b"):
        part_b(args.rounds, 50)
    if args.only in (None, "c"):
        part_c(args.rounds, 100, step_us)


if __name__ == "__main__":
    main()
