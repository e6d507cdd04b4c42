"""Time the classification recipe's kernels at the benchmark's shapes (B = 256, C = 1000; images
256 x 3 x 224 x 224): the old one-block loss kernel (vitmi_loss_fwd_bwd, CE) against the new launch
pair (vitmi_softmax_xent + its fold) with plain labels, the new entry with the mixed pair, with
smoothing and with metrics, with a dense target, and vitmi_mix_batch with its achieved TB/s.
Device events around back-to-back calls after a warm-up; each figure is the median of several such
windows, and the variants alternate within a round so that drift hits them alike (as
tools/optim_bench.py).  Every figure comes from the same process."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "transformer-stm_amd"))
import torch  # noqa: E402

from vitmi import ops  # noqa: E402
from vitmi._lib import check, lib  # noqa: E402


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def main():
    B, C = 256, 1000
    gen = torch.Generator(device="cuda").manual_seed(0)
    z = 4.0 * torch.randn(B, C, device="cuda", generator=gen)
    la = torch.randint(0, C, (B,), device="cuda", generator=gen)
    lb = torch.randint(0, C, (B,), device="cuda", generator=gen)
    lam = torch.rand(B, device="cuda", generator=gen)
    soft = torch.rand(B, C, device="cuda", generator=gen) / C
    loss, row, dl = torch.empty((), device="cuda"), torch.empty(B, device="cuda"), torch.empty_like(z)
    rec = torch.zeros(4, dtype=torch.float64, device="cuda")
    ws = torch.empty(lib().vitmi_softmax_xent_workspace_size(B), dtype=torch.uint8, device="cuda")
    p, s = ops._p, ops._s

    def new(label_b=None, lam_=None, soft_=None, smoothing=0.0, topk=0, metrics=None):
        return lambda: check(lib().vitmi_softmax_xent(
            B, C, p(z), C, p(la), p(label_b), p(lam_), p(soft_), C, smoothing, topk, p(row), p(loss), p(dl), C,
            p(metrics), p(ws), ws.numel(), s()))

    variants = {
        "old loss_fwd_bwd (CE)": lambda: check(lib().vitmi_loss_fwd_bwd(ops.LOSS_CE, B, C, p(z), p(la), p(loss), p(dl),
                                                                        s())),
        "new plain labels": new(),
        "new mixed pair": new(lb, lam),
        "new pair + smoothing": new(lb, lam, smoothing=0.1),
        "new pair + smoothing + metrics": new(lb, lam, smoothing=0.1, topk=5, metrics=rec),
        "new dense + smoothing": new(soft_=soft, smoothing=0.1),
    }

    img = torch.rand(256, 3, 224, 224, device="cuda", generator=gen)
    out = torch.empty_like(img)
    perm = torch.randperm(256, device="cuda", generator=gen).to(torch.int32)
    lam_img = torch.rand(256, device="cuda", generator=gen)
    box = torch.tensor([[40, 150, 60, 190]] * 256, dtype=torch.int32, device="cuda")
    nobox = torch.zeros(256, 4, dtype=torch.int32, device="cuda")
    ones = torch.ones(256, device="cuda")
    # one 154 MB batch fits the 256 MB Infinity Cache, so back-to-back calls on it are served from
    # there; four batches in rotation (616 MB) are not: that is the figure for a batch fresh from a loader
    imgs = [img] + [torch.rand_like(img) for _ in range(3)]
    turn = [0]

    def rotating():
        turn[0] = (turn[0] + 1) % len(imgs)
        ops.mix_batch(imgs[turn[0]], perm, lam_img, nobox, out)

    mixes = {
        "mix_batch mixup, 4 batches rotating": rotating,
        "mix_batch mixup": lambda: ops.mix_batch(img, perm, lam_img, nobox, out),
        "mix_batch cutmix": lambda: ops.mix_batch(img, perm, ones, box, out),
        "mix_batch copy (lam 1, no box)": lambda: ops.mix_batch(img, perm, ones, nobox, out),
    }

    for fn in list(variants.values()) + list(mixes.values()):      # warm-up: code objects, allocator
        for _ in range(10):
            fn()
    torch.cuda.synchronize()

    rounds = 7
    times = {k: [] for k in list(variants) + list(mixes)}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn, 200))
        for k, fn in mixes.items():
            times[k].append(window(fn, 20))
    print(f"B {B} C {C}; {rounds} rounds, variants alternating; us per call: median (min .. max)")
    for k, v in times.items():
        line = f"{k:34s} {statistics.median(v):9.2f}  ({min(v):.2f} .. {max(v):.2f})"
        if k.startswith("mix_batch"):
            nbytes = img.numel() * (8 if "copy" in k else 12)      # the copy does not read the partner
            line += f"   {nbytes / statistics.median(v) / 1e6:6.2f} TB/s"
        print(line)
    old, plain = statistics.median(times["old loss_fwd_bwd (CE)"]), statistics.median(times["new plain labels"])
    print(f"old / new plain labels: {old / plain:.1f}x")


if __name__ == "__main__":
    main()
