"""Time LayerScale at the benchmark's shapes.

(a) The fold (vitmi_layerscale_fold, fp32 -> bf16 and fp32 -> fp32) and the in-place backward
    (vitmi_layerscale_bwd: dgamma + scaling, dgamma alone, scaling alone) at the ViT-B out-projection
    (768, 768) and fc2 (768, 3072) weights, as us and bytes/s, beside cast_bf16 of the same element count
    (the streaming rate the same traffic pattern reaches here).  Bytes are the algorithm's, from shapes:
    fold 4 + 2 (bf16) or 4 + 4 per element, backward 4 (dw read) + 4 (w read, with dgamma) + 4 (dw
    write, when scaling).
(b) A full ViT-B/16 bs 256 bf16 forward + backward + Adam step with init_values None and 1e-4.

Device events around back-to-back calls after a warm-up; each figure is the median of several such
windows with its min .. max, and the variants alternate within a round so that drift hits them
alike (as tools/droppath_bench.py).  Every figure comes from the same process and the same build.
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


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def part_a(rounds, iters):
    gen = torch.Generator(device="cuda").manual_seed(0)
    variants, nbytes = {}, {}
    for N, K in ((768, 768), (768, 3072)):
        w = 0.02 * torch.randn(N, K, device="cuda", generator=gen)
        b = 0.02 * torch.randn(N, device="cuda", generator=gen)
        gam = torch.full((N,), 1e-4, device="cuda")
        # the backward scales dw in place: gamma 1 keeps the repeated calls' values where they are
        one = torch.ones(N, device="cuda")
        dw, db, dg = torch.randn(N, K, device="cuda", generator=gen), torch.randn(N, device="cuda"), torch.zeros(
            N, device="cuda")
        e = N * K
        tag = f"({N}, {K})"
        for name, fn, by in (
                ("cast_bf16", lambda w=w: ops.cast_bf16(w), 6 * e),
                ("fold -> bf16", lambda w=w, b=b, gam=gam: ops.layerscale_fold(w, gam, b, torch.bfloat16), 6 * e),
                ("fold -> fp32", lambda w=w, b=b, gam=gam: ops.layerscale_fold(w, gam, b, torch.float32), 8 * e),
                ("bwd dgamma + scale", lambda w=w, b=b, one=one, dw=dw, db=db, dg=dg:
                 ops.layerscale_bwd(w, b, one, dw, db, dg, True), 12 * e),
                ("bwd dgamma only", lambda w=w, b=b, one=one, dw=dw, db=db, dg=dg:
                 ops.layerscale_bwd(w, b, one, dw, db, dg, False), 8 * e),
                ("bwd scale only", lambda w=w, b=b, one=one, dw=dw, db=db:
                 ops.layerscale_bwd(w, b, one, dw, db, None, True), 8 * e)):
            variants[f"{tag} {name}"] = fn
            nbytes[f"{tag} {name}"] = by
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, iters))
    print(f"(a) LayerScale kernels; {rounds} rounds x {iters} back-to-back calls, alternating; median (min .. max); "
          "repeated calls on one buffer: the operands stay in the caches")
    for k, v in times.items():
        m = statistics.median(v)
        print(f"  {k:34s} {m:8.2f} us  ({min(v):.2f} .. {max(v):.2f})  {nbytes[k] / m / 1e6:8.3f} TB/s")


def part_b(rounds, steps):
    B = 256
    models = {}
    for name, iv in (("init_values None", None), ("init_values 1e-4", 1e-4)):
        torch.manual_seed(0)
        cfg = config_c3(init_values=iv)
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
    print(f"(b) ViT-B/16 bs {B} bf16 fwd + bwd + Adam; {rounds} rounds x {steps} steps, alternating; "
          "median (min .. max)")
    base = statistics.median(times["init_values None"])
    for k, v in times.items():
        m = statistics.median(v)
        print(f"  {k:20s} {m:10.1f} us  ({min(v):.1f} .. {max(v):.1f})  {100 * (m / base - 1):+6.2f} %  "
              f"{B / m * 1e6:.0f} img/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layerscale_bench: needs the GPU (no CPU timing)")
    if args.only in (None, "a"):
        part_a(args.rounds, 50)
    if args.only in (None, "b"):
        part_b(args.rounds, 5)


if __name__ == "__main__":
    main()
