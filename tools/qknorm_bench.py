"""Time QK-norm at the benchmark's shapes.

(a) vitmi_qknorm_fwd / _bwd at M = 256 * 197, H = 12, bf16 (the ViT-B qkv buffer, [M, 2304]) and, in the
    same process, vitmi_layernorm_fwd / _bwd at the same M and D = 768 in the forms the block runs them
    (fp32 x -> bf16 y; bf16 dy + fp32 x + fp32 residual gradient -> fp32 dx + its bf16 copy).  Each line
    gives the achieved bytes/s from the bytes the shapes imply (every operand once): the LayerNorm
    kernels' figure is the yardstick for these streaming kernels, not a fixed number.  The backward
    rewrites dqkv in place; with unit gamma and unit-variance rows that map is a projection, so repeated
    calls stay in range.
(b) A full ViT-B/16 bs 256 bf16 forward + backward + Adam step with qk_norm off and on.

Device events around back-to-back calls after a warm-up; each figure is the median of several such
windows with its min .. max, and the variants alternate within a round so that drift hits them alike
(as tools/droppath_bench.py).  Every figure comes from the same process and the same build.
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
    B, S, H, D = 256, 197, 12, 768
    M, W = B * S, 3 * D
    BF, F32 = torch.bfloat16, torch.float32
    gen = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)  # noqa: E731
    qkv, dqkv = rn(M, W).to(BF), rn(M, W).to(BF)
    g64, b64 = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    _, qm, qr = ops.qknorm_fwd(qkv, H, g64, b64, g64, b64, 1e-6)
    dgs = [torch.zeros(64, device="cuda") for _ in range(4)]
    dbias = torch.zeros(W, device="cuda")
    x, dres, dy = rn(M, D), rn(M, D), rn(M, D).to(BF)
    gD, bD = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    _, m1, r1 = ops.layernorm_fwd(x, gD, bD, 1e-6, BF)
    dg, db, dxs = (torch.zeros(D, device="cuda") for _ in range(3))
    dx, dx_lp = torch.empty(M, D, device="cuda"), torch.empty(M, D, device="cuda", dtype=BF)

    # name -> (call, bytes every operand once)
    variants = {
        "qknorm_fwd bf16": (lambda: ops.qknorm_fwd(qkv, H, g64, b64, g64, b64, 1e-6),
                            M * W * 2 * 2 + M * 2 * H * 8),
        "qknorm_bwd bf16 (+ dbias, 4 norm grads)": (lambda: ops.qknorm_bwd(qkv, qm, qr, g64, g64, dqkv, *dgs, dbias),
                                                    M * D * 2 * 7 + M * 2 * H * 8),
        "qknorm_bwd bf16, dbias NULL": (lambda: ops.qknorm_bwd(qkv, qm, qr, g64, g64, dqkv, *dgs, None),
                                        M * D * 2 * 6 + M * 2 * H * 8),
        "layernorm_fwd f32 -> bf16": (lambda: ops.layernorm_fwd(x, gD, bD, 1e-6, BF), M * D * (4 + 2) + M * 8),
        "layernorm_bwd (+ dres, dx_lp, dxsum)": (lambda: ops.layernorm_bwd(dy, x, m1, r1, gD, dg, db, dres=dres, dx=dx,
                                                                           lp_dtype=BF, dxsum=dxs, dx_lp=dx_lp),
                                                 M * D * (2 + 4 + 4 + 4 + 2) + M * 8),
    }
    for fn, _ in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, _) in variants.items():
            times[k].append(window(fn, iters))
    print(f"(a) M {M}, H {H}, D {D}, bf16; {rounds} rounds x {iters} calls, alternating; median (min .. max), "
          "achieved TB/s from shape-derived bytes (the backwards include their fold launch)")
    for k, v in times.items():
        m, nbytes = statistics.median(v), variants[k][1]
        print(f"  {k:42s} {m:9.1f} us  ({min(v):.1f} .. {max(v):.1f})  {nbytes / 1e6:8.1f} MB  {nbytes / m / 1e6:6.2f} TB/s")


def part_b(rounds, steps):
    B = 256
    models = {}
    for name, on in (("qk_norm off", False), ("qk_norm on", True)):
        torch.manual_seed(0)
        model = VisionTransformer(config_c3(qk_norm=on)).to("cuda").train()
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
    base = statistics.median(times["qk_norm off"])
    for k, v in times.items():
        m = statistics.median(v)
        print(f"  {k:14s} {m / 1e3:9.3f} ms  ({min(v) / 1e3:.3f} .. {max(v) / 1e3:.3f})  {100 * (m / base - 1):+6.2f} %  "
              f"{B / m * 1e6:.0f} img/s")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qknorm_bench: needs the GPU (no CPU timing)")
    if args.only in (None, "a"):
        part_a(args.rounds, 50)
    if args.only in (None, "b"):
        part_b(args.rounds, 5)


if __name__ == "__main__":
    main()
