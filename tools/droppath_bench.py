"""Time stochastic depth (drop path) at the benchmark's shapes.

(a) The ViT-B out-projection residual GEMM (M = 256 * 197, N = K = 768, bf16 operands, fp32 residual
    stream) with the plain RESIDUAL epilogue, with the drop-path epilogue at p = 0.1, with the element
    dropout epilogue at 0.1 and with both, plus the backward's one extra pass per branch
    (vitmi_droppath_apply, fp32 in, bf16 out).
(b) A full ViT-B/16 bs 256 bf16 forward + backward + Adam step at drop_path_rate 0 and 0.1.

Device events around back-to-back calls after a warm-up; each figure is the median of several such
windows with its min .. max, and the variants alternate within a round so that drift hits them
alike (as tools/loss_bench.py).  Every figure comes from the same process and the same build.
``--only a`` / ``--only b`` runs one part."""
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

SITE = 0x40000001


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def report(title, times, base):
    print(title)
    b = statistics.median(times[base])
    for k, v in times.items():
        m = statistics.median(v)
        print(f"  {k:38s} {m:10.1f} us  ({min(v):.1f} .. {max(v):.1f})  {100 * (m / b - 1):+6.2f} % vs {base}")


def part_a(rounds, iters):
    B, S, D = 256, 197, 768
    M = B * S
    gen = torch.Generator(device="cuda").manual_seed(0)
    o = torch.randn(M, D, device="cuda", generator=gen).to(torch.bfloat16)
    w = (0.02 * torch.randn(D, D, device="cuda", generator=gen)).to(torch.bfloat16)
    bias = 0.02 * torch.randn(D, device="cuda", generator=gen)
    res = torch.randn(M, D, device="cuda", generator=gen)
    g = torch.randn(M, D, device="cuda", generator=gen)

    def gemm(**kw):
        return lambda: ops.linear_fwd(o, w, bias, torch.float32, ops.EPI_RESIDUAL, residual=res, **kw)

    variants = {
        "plain RESIDUAL": gemm(),
        "drop path 0.1": gemm(droppath=(7, SITE, 0.1, S)),
        "dropout 0.1": gemm(dropout=(7, 0, 0.1)),
        "dropout 0.1 + drop path 0.1": gemm(dropout=(7, 0, 0.1), droppath=(7, SITE, 0.1, S)),
        "cast_bf16 (the plain backward copy)": lambda: ops.cast_bf16(g),
        "droppath_apply f32 -> bf16": lambda: ops.droppath_apply(g, 7, SITE, 0.1, S, torch.bfloat16),
        "droppath_apply + dropout": lambda: ops.droppath_apply(g, 7, SITE, 0.1, S, torch.bfloat16, dropout=(0, 0.1)),
    }
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    report(f"(a) out-projection residual GEMM M {M} N {D} K {D} bf16; {rounds} rounds x {iters} calls, "
           "alternating; median (min .. max)", times, "plain RESIDUAL")


def part_b(rounds, steps):
    B = 256
    models = {}
    for name, rate in (("drop_path_rate 0", 0.0), ("drop_path_rate 0.1", 0.1)):
        torch.manual_seed(0)
        cfg = config_c3(drop_path_rate=rate)
        model = VisionTransformer(cfg).to("cuda").train()
        model.reset_parameters(seed=0)
        models[name] = (model, optim.Adam(model, learning_rate=1e-6), list(model.arena().params))
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

    variants = {k: step(k) for k in models}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, steps))
    report(f"(b) ViT-B/16 bs {B} bf16 fwd + bwd + Adam; {rounds} rounds x {steps} steps, alternating; "
           "median (min .. max)", times, "drop_path_rate 0")
    for k, v in times.items():
        print(f"  {k}: {B / statistics.median(v) * 1e6:.0f} img/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("droppath_bench: needs the GPU (no CPU timing)")
    if args.only in (None, "a"):
        part_a(args.rounds, 50)
    if args.only in (None, "b"):
        part_b(args.rounds, 5)


if __name__ == "__main__":
    main()
