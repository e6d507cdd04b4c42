"""Recipe and data-path conformance on the MI355X: vitmi_softmax_xent (with its finalize launch and metrics
record) and vitmi_mix_batch (csrc/loss.hip), vitmi_sls_preprocess and vitmi_gather_rows (csrc/sls.hip) and
vitmi_patch_keep (csrc/patchdrop.hip) against tests/ref_recipe.py: by the derived PER-ELEMENT bound for the
loss and its gradient, bit for bit everywhere else.

The library is called directly (vitmi._lib.lib()), so every buffer is the test's own guarded allocation:
float inputs between NaN guard rows with NaN behind every pitched row, byte inputs with 0xFF in their gaps,
outputs between fixed-bit guards.  (The integer tables -- labels, perm, box, idx, the resize tables -- are plain
device tensors.)  A HIP error ends the session (check_rc / sync of the attention suite).

Every case asserts
  1. every element within tol (|err| / tol <= 1, the worst ratio is printed), or bitwise equal where the reference
     pins the bits; a NaN reference element is met by a NaN only,
  2. the guards around every buffer bitwise intact and the inputs unchanged,
  3. a second run bitwise equal,
  4. the kernels recorded: for softmax_xent exactly the instance the alignment rule selects (16-byte or scalar,
     dense or not), once, and the finalize launch iff loss or metrics are asked for; for mix_batch the 16-byte or
     the scalar instance, once; nothing for the launches that record nothing.
The matrix is ref_recipe's.  Non-finite rule (include/vitmi.h): a row that holds a NaN logit has a NaN row_loss
and an all-NaN gradient row, the batch loss is NaN, and the other rows keep their bits.

Worst |err| / tol, measured on MI355X (every figure is against the float64 reference):
  softmax_xent, every C at B in {1, 3, 5}, every way and subset: row 0.192 loss 0.114 dlogits 0.662
  softmax_xent, B in {255 .. 2051} at C in {5, 8}:                  row 0.254 loss 0.037 dlogits 0.871
  softmax_xent, the six input families:                              row 0.291 loss 0.202 dlogits 0.657
  softmax_xent, the finite rows of the NaN cases:                    row 0.204            dlogits 0.658
  (the float32 emulation on the CPU, same cases: row 0.254 loss 0.115 dlogits 0.871.)  Everything else is bit for bit."""
import itertools
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_patchdrop  # noqa: E402
import ref_recipe as rr  # noqa: E402
from kstats import kernel_stats  # noqa: E402
from ref_gemm import guards_intact, padded  # noqa: E402
from test_gpu_attn_conformance import check_rc, same_bits, stream, sync  # noqa: E402
from test_gpu_ln_conformance import Snapshot, refused  # noqa: E402
from test_gpu_tokens_conformance import Worst as TokensWorst, din, dout, dvec_out, host, ptr, twice  # noqa: E402
from vitmi import _lib  # noqa: E402

DEV = "cuda"
F32 = torch.float32
f32 = np.float32
GUARD = 0x4B


class Worst(TokensWorst):
    def report(self, what):
        print(f"CONF recipe {what}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in self.items()))
        for k, v in self.items():
            assert v <= 1.0, (what, k, v)


def tens(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dev(a):
    return tens(a).to(DEV)


def npy(p):
    """The window of a float buffer as numpy."""
    return host(p).numpy()


class Guarded:
    """nbytes at ``offset`` bytes past a 16-byte boundary, 256 guard bytes (``fill``) in front and behind."""

    def __init__(self, nbytes, offset=0, init=None, fill=GUARD):
        self.n, self.lo, self.fill = nbytes, 256 + offset, fill
        h = torch.full((self.lo + nbytes + 256,), fill, dtype=torch.uint8)
        if init is not None:
            h[self.lo:self.lo + nbytes] = tens(np.ascontiguousarray(init).view(np.uint8).reshape(-1))
        self.buf = h.to(DEV)
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def bytes(self):
        return self.buf[self.lo:self.lo + self.n].cpu().numpy()

    def guards_ok(self):
        return bool((self.buf[:self.lo] == self.fill).all().item() and (self.buf[self.lo + self.n:] == self.fill).all().item())


def twice_bytes(fn, what, inputs=()):
    """fn() -> {name: Guarded} twice, nothing recorded, guards intact, the second run bitwise the first."""
    with kernel_stats() as st:
        a = fn()
    b = fn()
    sync(what)
    assert not st.k, (what, "a launch that records no statistic recorded one", st.k)
    for k, g in a.items():
        assert g.guards_ok(), (what, f"guards of {k} changed")
        assert torch.equal(g.buf, b[k].buf), (what, k, "second run differs")
    for g in inputs:
        assert g.guards_ok(), (what, "guards of an input changed")
    return a


# ------------------------------------------------------------------------------------------- softmax_xent
class XentProblem:
    """One batch on the device, laid out for one way to the 16-byte or the scalar path."""

    def __init__(self, batch, form, way):
        self.b, self.form, self.way = batch, form, way
        z = batch["z"]
        self.B, self.C = z.shape
        B, C = self.B, self.C
        al = 4 if C % 4 == 0 else 3                       # a pitch that keeps every row base 16-byte aligned
        if way == "base":
            self.z = padded(B, C, C + 4, F32, "nan", offset=1).set(tens(z)).to(DEV)
        else:
            self.z = din(tens(z), 5 if way == "ldl" else al)
        self.dense = form == "dense"
        self.soft = din(tens(batch["soft"]), 5 if way == "lds" else al) if self.dense else None
        self.la = dev(batch["la"])
        self.lb, self.lam = (dev(batch["lb"]), dev(batch["lam"])) if form == "pair" else (None, None)
        self.dl_pad = 5 if way == "lddl" else al
        self.kw = rr.form_args(batch, form)
        self.W = rr.width(C, way)
        self.inputs = [p for p in (self.z, self.soft) if p is not None]
        self.tables = [t for t in (self.la, self.lb, self.lam) if t is not None]
        self.snap = Snapshot(self.inputs)
        self.tsnap = [t.clone() for t in self.tables]

    def width(self, gives_dl):
        """Elements per load of the instance the alignment rule selects: an odd lddl counts only when a gradient
        is written."""
        return rr.width(self.C, "auto") if self.way == "lddl" and not gives_dl else self.W

    def kernel(self, gives_dl):
        return f"softmax_xent_kernelILi{self.width(gives_dl)}ELb{int(self.dense)}E"

    def run(self, outs, eps, topk=1, rec=None, what=""):
        """One call; {name: Padded}.  ``rec``: a record to add to (else a zeroed one per call)."""
        lib = _lib.lib()
        B, C = self.B, self.C
        o = {}
        if "row" in outs:
            o["row"] = dvec_out(B)
        if "loss" in outs:
            o["loss"] = dvec_out(1)
        if "dl" in outs:
            o["dl"] = dout(B, C, self.dl_pad)
        if "metrics" in outs:
            o["metrics"] = rec if rec is not None else dvec_out(8, init=torch.zeros(8))
        nws = lib.vitmi_softmax_xent_workspace_size(B)
        o["ws"] = dvec_out(nws // 4)
        dl = o.get("dl")
        need_la = not self.dense or "metrics" in outs
        rc = lib.vitmi_softmax_xent(B, C, self.z.ptr(), self.z.pitch, self.la.data_ptr() if need_la else None,
                                    self.lb.data_ptr() if self.lb is not None else None,
                                    self.lam.data_ptr() if self.lam is not None else None, ptr(self.soft),
                                    self.soft.pitch if self.soft else 0, eps, topk, ptr(o.get("row")), ptr(o.get("loss")), ptr(dl),
                                    dl.pitch if dl else 0, ptr(o.get("metrics")), o["ws"].ptr(), nws, stream())
        check_rc(rc, what)
        return o

    def twice(self, outs, eps, topk=1, what=""):
        with kernel_stats() as st:
            a = self.run(outs, eps, topk, what=what)
        b = self.run(outs, eps, topk, what=what)
        sync(what)
        want = {self.kernel("dl" in outs): 1}
        if "loss" in outs or "metrics" in outs:
            want["xent_finalize_kernel"] = 1
        assert len(st.k) == len(want) and all(st.calls(k) == 1 for k in want), (what, st.k, want)
        for k, p in a.items():
            assert guards_intact(p), (what, f"guards of {k} changed")
            assert same_bits(p, b[k]), (what, k, "second run differs")
        return a

    def assert_inputs_unchanged(self, what):
        self.snap.assert_unchanged(what)
        for t, before in zip(self.tables, self.tsnap):
            assert torch.equal(t, before), (what, "a table was written to")


def record(p):
    """(loss_sum, rows, top1, topk) of a metrics record."""
    return struct.unpack("<dQQQ", npy(p).tobytes())


def check_xent(got, ref, pr, eps, topk, w, what):
    """The outputs of one call against the reference: row, loss, dl by the bound; loss and loss_sum bitwise the
    fold of the rows the kernel wrote; the hit counts exactly."""
    rows = None
    if "row" in got:
        rows = npy(got["row"])[0]
        w.add("row", rr.ratio(rows, *ref["row"]))
    elif "loss" in got or "metrics" in got:               # the rows were kept in the workspace
        rows = npy(got["ws"])[0][:pr.B]
        w.add("row", rr.ratio(rows, *ref["row"]))
    if "loss" in got:
        loss = npy(got["loss"])[0]
        w.add("loss", rr.ratio(loss, *ref["loss"]))
        assert rr.same_bits_nan(loss, np.array([rr.fold_loss(rows)], f32)), (what, "loss is not the promised fold", loss)
    if "dl" in got:
        w.add("dl", rr.ratio(npy(got["dl"]), *ref["dl"]))
    if "metrics" in got:
        ls, n, h1, hk = record(got["metrics"])
        la = pr.b["la"]
        assert (n, h1, hk) == (pr.B, int(rr.hits(pr.b["z"], la, 1).sum()), int(rr.hits(pr.b["z"], la, topk).sum())), (what, n, h1, hk)
        if rows is not None:
            assert rr.same_bits_nan(np.array([ls]), np.array([rr.fold(rows)])), (what, "loss_sum is not the promised fold")


def run_forms(batch, way, w, subsets_at=rr.XENT_SMOOTHINGS, what=""):
    """Every form and smoothing of one batch on one way: the full output set, then every output subset (at the
    smoothings of ``subsets_at``: both) with the shared values bitwise equal across subsets."""
    B, C = batch["z"].shape
    topk = min(5, C)
    for form in rr.XENT_FORMS:
        if way not in rr.xent_ways(C, form):
            continue
        pr = XentProblem(batch, form, way)
        for eps in rr.XENT_SMOOTHINGS:
            tag = f"{what} B{B} C{C} {way} {form} eps{eps}"
            ref = rr.xent(batch["z"], smoothing=eps, W=pr.W, **pr.kw)
            full = pr.twice(rr.XENT_SUBSETS[-1], eps, topk, tag)
            check_xent(full, ref, pr, eps, topk, w, tag)
            assert not np.isnan(npy(full["dl"])).any() and not np.isnan(npy(full["row"])).any(), tag
            if eps not in subsets_at:
                continue
            for outs in rr.XENT_SUBSETS[:-1]:
                if way == "lddl" and "dl" not in outs:
                    continue                              # without a gradient lddl is not looked at: the "auto" case
                got = pr.twice(outs, eps, topk, f"{tag} {outs}")
                check_xent(got, ref, pr, eps, topk, w, f"{tag} {outs}")
                for k in outs:
                    assert same_bits(got[k], full[k]), (tag, outs, k, "differs from the full call")
                if outs in (("loss",), ("metrics",)):
                    assert np.array_equal(npy(got["ws"])[0][:B].view(np.uint32), npy(full["row"])[0].view(np.uint32)), (tag, "workspace rows")
        pr.assert_inputs_unchanged(f"{what} B{B} C{C} {way} {form}")


@pytest.mark.parametrize("C", rr.XENT_CS)
def test_xent_shapes(C):
    """Every C (both sides of a wave, of the 1024-element register file and of its first step past it, the admitted
    maximum) at B in {1, 3, 5}: three forms, smoothing 0 and 0.1, the 16-byte path and the scalar one reached each
    way alone, every output subset at both smoothings."""
    w = Worst()
    for B, _, way in [c for c in rr.xent_shape_cases() if c[1] == C and c[0] in rr.XENT_BS]:
        run_forms(rr.xent_batch("randn4", B, C), way, w, what="shapes")
    w.report(f"xent C{C}")


@pytest.mark.parametrize("B", rr.XENT_BIG_BS)
def test_xent_large_batches(B):
    """Both sides of the finalize block and of its second and ninth row per thread, and of the switch to four rows
    per block (B >= 2048), at C in {5, 8}."""
    w = Worst()
    for C in rr.XENT_BIG_CS:
        run_forms(rr.xent_batch("randn4", B, C), "auto", w, what="large")
    w.report(f"xent B{B}")


@pytest.mark.parametrize("fam", rr.XENT_FAMILIES)
def test_xent_families(fam):
    w = Worst()
    for C, way, form, eps in itertools.product(rr.XENT_FAMILY_CS, ("auto", "base"), rr.XENT_FORMS, rr.XENT_SMOOTHINGS):
        if way not in rr.xent_ways(C, form) or (fam == "masked" and eps):
            continue
        b = rr.xent_batch(fam, 3, C)
        pr = XentProblem(b, form, way)
        tag = f"family {fam} C{C} {way} {form} eps{eps}"
        got = pr.twice(rr.XENT_SUBSETS[-1], eps, min(5, C), tag)
        ref = rr.xent(b["z"], smoothing=eps, W=pr.W, **pr.kw)
        check_xent(got, ref, pr, eps, min(5, C), w, tag)
        if fam == "masked":
            masked = np.isinf(b["z"])
            assert masked.any() and np.isfinite(npy(got["row"])).all() and (npy(got["dl"])[masked] == 0).all(), tag
        pr.assert_inputs_unchanged(tag)
    w.report(f"xent family {fam}")


@pytest.mark.parametrize("C", (5, 8, 65, 1028))
def test_xent_row_independence(C):
    """Row h alone (B = 1), inside B = 5 and inside B = 2051 (four rows per block) has the same bits: the row loss
    as it is; the gradient, whose last factor is fl(1 / B), as the row's own gradient at B = 1 (where that factor
    is 1) times fl(1 / B), rounded once."""
    big = rr.xent_batch("randn4", 2051, C)
    h = rr.XENT_ROW_H

    def sub(rows):
        return {k: np.ascontiguousarray(v[rows]) for k, v in big.items()}
    for form, eps in itertools.product(rr.XENT_FORMS, rr.XENT_SMOOTHINGS):
        outs = {}
        for name, rows in (("one", slice(h, h + 1)), ("five", slice(0, 5)), ("all", slice(0, 2051))):
            got = XentProblem(sub(rows), form, "auto").twice(("row", "dl"), eps, 1, f"row independence C{C} {form} {name}")
            at = 0 if name == "one" else h
            outs[name] = (npy(got["row"])[0][at].view(np.uint32), npy(got["dl"])[at])
        for name, B in (("five", 5), ("all", 2051)):
            want = (outs["one"][1] * (f32(1) / f32(B))).astype(f32)
            assert outs[name][0] == outs["one"][0] and rr.same_bits_nan(outs[name][1], want), (C, form, eps, name)


def test_xent_record_accumulates_over_three_calls():
    calls = []
    rec = dvec_out(8, init=torch.zeros(8))
    for B, C, form in ((3, 65, "labels"), (5, 68, "dense"), (257, 8, "pair")):
        b = rr.xent_batch("halfint", B, C)
        pr = XentProblem(b, form, "auto")
        topk = min(5, C)
        got = pr.run(("row", "metrics"), 0.1, topk, rec=rec, what="record")
        sync("record")
        rows = npy(got["row"])[0]
        calls.append((rows, rr.hits(b["z"], b["la"], 1), rr.hits(b["z"], b["la"], topk)))
        ls, n, h1, hk = record(rec)
        want = rr.record_after(calls)
        assert rr.same_bits_nan(np.array([ls]), np.array([want[0]])) and (n, h1, hk) == want[1:], (B, C, form, (ls, n, h1, hk), want)
        assert guards_intact(rec)


def hits_of(z, lab, k, way):
    """Per-row (top1, topk) hits of the device, each row scored alone through a zeroed record."""
    out = []
    for i in range(z.shape[0]):
        b = dict(z=z[i:i + 1], la=lab[i:i + 1], lb=lab[i:i + 1], lam=np.ones(1, f32), soft=np.zeros_like(z[i:i + 1]))
        got = XentProblem(b, "labels", way).twice(("metrics",), 0.0, k, f"hits k{k} {way} row {i}")
        _, n, h1, hk = record(got["metrics"])
        assert n == 1
        out.append((h1, hk))
    return out


def test_xent_hits():
    """Exact against the rule at k in {1, 5, C}: ties across a lane boundary and inside one 16-byte group on both
    paths, the all-equal row of 65535 classes with the last label, random rows, and NaN at the label (a miss)."""
    for name, z, lab in rr.tie_cases():
        C = z.shape[1]
        for k, way in itertools.product((1, 5, C), ("auto",) if C % 4 else ("auto", "base")):
            want = [(int(a), int(b)) for a, b in zip(rr.hits(z, lab, 1), rr.hits(z, lab, k))]
            assert hits_of(z, lab, k, way) == want, (name, k, way)
    for C in (5, 68, 4099):
        b = rr.xent_batch("halfint", 37, C)
        b["z"][3, b["la"][3]] = np.nan                    # NaN at the label: a miss, whatever k
        b["la"][5], b["la"][6] = -1, C
        pr = XentProblem(b, "labels", "auto")
        for k in (1, min(5, C), C):
            got = pr.twice(("metrics",), 0.0, k, f"hits C{C} k{k}")
            _, n, h1, hk = record(got["metrics"])
            assert (n, h1, hk) == (37, int(rr.hits(b["z"], b["la"], 1).sum()), int(rr.hits(b["z"], b["la"], k).sum())), (C, k)
        assert not rr.hits(b["z"], b["la"], C)[[3, 5, 6]].any()


@pytest.mark.parametrize("C", rr.XENT_NAN_CS)
def test_xent_nan_rows(C):
    """A NaN logit at column 0, 5, 63, 64, C - 1 and filling one whole aligned group of four, the label elsewhere, on
    the 16-byte and on the scalar path: NaN row_loss, NaN loss (and loss_sum), an all-NaN gradient row; the other
    rows of the batch keep the bits they have without the NaN.

    Before the non-finite rule the kernel dropped a NaN that a lane met before its first finite element: on the
    scalar path at columns 0, 5 and 63 (a finite row_loss and loss, one NaN gradient element), on the 16-byte path
    at the whole group."""
    w = Worst()
    for way in (("auto", "base") if C % 4 == 0 else ("auto",)):
        for (name, cols), form, eps in itertools.product(rr.nan_columns(C), rr.XENT_FORMS, rr.XENT_SMOOTHINGS):
            b = rr.nan_batch(C, cols)
            pr = XentProblem(b, form, way)
            tag = f"nan C{C} {way} {name} {form} eps{eps}"
            got = pr.twice(rr.XENT_SUBSETS[-1], eps, 1, tag)
            row, loss, dl = npy(got["row"])[0], npy(got["loss"])[0], npy(got["dl"])
            print(f"{tag}: row_loss {row} loss {loss} NaN gradients in the row {int(np.isnan(dl[1]).sum())} of {C}")
            assert np.isnan(row[1]) and np.isnan(loss).all() and np.isnan(dl[1]).all(), (tag, row, loss, int(np.isnan(dl[1]).sum()))
            assert np.isnan(record(got["metrics"])[0]), tag
            check_xent(got, rr.xent(b["z"], smoothing=eps, W=pr.W, **pr.kw), pr, eps, 1, w, tag)
            clean = dict(b, z=np.where(np.isnan(b["z"]), f32(0), b["z"]))
            other = XentProblem(clean, form, way).twice(("row", "dl"), eps, 1, f"{tag} clean")
            keep = [0, 2]
            assert np.array_equal(row[keep].view(np.uint32), npy(other["row"])[0][keep].view(np.uint32)), (tag, "another row's loss")
            assert np.array_equal(dl[keep].view(np.uint32), npy(other["dl"])[keep].view(np.uint32)), (tag, "another row's gradient")
            pr.assert_inputs_unchanged(tag)
    w.report(f"xent nan C{C}")


# ------------------------------------------------------------------------------------------- mix_batch
def run_mix(H, W, vec, img_np, perm, lam, box, what, img_off=0, out_off=0, nan_ok=False):
    lib = _lib.lib()
    B, C = img_np.shape[:2]
    img = padded(B * C * H, W, W, F32, "nan", offset=img_off).set(tens(img_np.reshape(B * C * H, W))).to(DEV)
    snap = Snapshot([img])
    pd, ld, bd = dev(perm), dev(lam), dev(box)

    def run():
        o = padded(B * C * H, W, W, F32, "guard", offset=out_off).to(DEV)
        check_rc(lib.vitmi_mix_batch(B, C, H, W, img.ptr(), pd.data_ptr(), ld.data_ptr(), bd.data_ptr(), o.ptr(), stream()), what)
        return {"out": o}
    got = twice(run, what, f"mix_batch_kernelILi{4 if vec else 1}E", [img], nan_ok=nan_ok)
    snap.assert_unchanged(what)
    assert torch.equal(pd.cpu(), tens(perm)) and torch.equal(ld.cpu(), tens(lam)) and torch.equal(bd.cpu(), tens(box)), what
    want = rr.mix(img_np, perm, lam, box)
    assert rr.same_bits_nan(npy(got["out"]).reshape(img_np.shape), want), (what, "not bitwise the reference")


MIX_CASES = [(H, W, True, 0, 0) for H, W in rr.MIX_VEC] + [(H, W, False, 0, 0) for H, W in rr.MIX_SCALAR] + \
            [(H, W, False, io, oo) for H, W in rr.MIX_OFFSET for io, oo in ((1, 0), (0, 1))]


@pytest.mark.parametrize("H,W,vec,img_off,out_off", MIX_CASES, ids=[f"{h}x{w}-{'vec' if v else 'scalar'}-{i}{o}" for h, w, v, i, o in MIX_CASES])
def test_mix_batch(H, W, vec, img_off, out_off):
    """Both sides of one group per thread, of one chunk of 1024 groups, a one-row plane spanning chunks, three
    chunks; the scalar path through W % 4 and through img or out one float off; every box kind (off the 4-alignment,
    wholly in the second chunk, across a chunk boundary), lam in {0, 0.3, 1}, perm identity, roll, out of range;
    B = 3, C = 3, every plane different.  Bit for bit; the copy case does not read its NaN partner."""
    assert (W % 4 == 0 and not img_off and not out_off) == vec
    img = rr.mix_image(rr.MIX_B, rr.MIX_C, H, W)
    for name, perm, lam, box in rr.mix_tables(H, W):
        run_mix(H, W, vec, img, perm, lam, box, f"mix {H}x{W} {name}", img_off, out_off)
    perm, lam, box = rr.mix_copy_table()
    run_mix(H, W, vec, rr.mix_image(rr.MIX_B, rr.MIX_C, H, W, nan_sample=0), perm, lam, box, f"mix {H}x{W} copy", img_off, out_off,
            nan_ok=True)


# ------------------------------------------------------------------------------------------- sls_preprocess
def sls_tables(H, W, Ho, Wo):
    """The device tables from vitmi_sls_resize_table (host), checked against the oracle's."""
    lib = _lib.lib()
    out = []
    for s, d in ((W, Wo), (H, Ho)):
        ofs, wt = np.zeros(d, np.int32), np.zeros(2 * d, np.int16)
        assert lib.vitmi_sls_resize_table(s, d, ofs.ctypes.data, wt.ctypes.data) == 0
        ro, rw = rr.sls_ref.resize_coeffs(s, d)
        assert np.array_equal(ofs, ro) and np.array_equal(wt.reshape(d, 2), rw), (s, d)
        out += [dev(ofs), dev(wt)]
    return out


def run_sls(frames, H, W, Ho, Wo, bgr, pitched, what):
    lib = _lib.lib()
    n = frames.shape[0]
    buf, ib, rb = rr.sls_pack(frames, pitched)
    src = Guarded(buf.size, init=buf, fill=0xFF)
    before = src.buf.clone()
    xo, xw, yo, yw = sls_tables(H, W, Ho, Wo)

    def run():
        o = dout(n, Ho * Wo)
        check_rc(lib.vitmi_sls_preprocess(n, H, W, src.ptr(), ib, rb, bgr, Ho, Wo, xo.data_ptr(), xw.data_ptr(), yo.data_ptr(),
                                          yw.data_ptr(), o.ptr(), stream()), what)
        return {"out": o}
    got = twice(run, what, None)
    assert torch.equal(src.buf, before), (what, "the source was written to")
    want = rr.sls_image(buf, n, H, W, ib, rb, bgr, Ho, Wo)
    assert rr.same_bits_nan(npy(got["out"]).reshape(n, Ho, Wo), want), (what, "not bitwise the reference")


@pytest.mark.parametrize("H,W,Ho,Wo", rr.SLS_SHAPES, ids=[f"{h}x{w}-{a}x{b}" for h, w, a, b in rr.SLS_SHAPES])
def test_sls_preprocess(H, W, Ho, Wo):
    """One-pixel-wide and one-pixel-high sources, shrinking to one pixel, identity, up and down; both channel
    orders; frames of 0, of 255, a 0 / 255 checkerboard and random; dense and pitched (0xFF in the gaps)."""
    for kind, bgr, pitched in itertools.product(rr.SLS_FRAMES, (0, 1), (False, True)):
        run_sls(rr.sls_frames(kind, 2, H, W), H, W, Ho, Wo, bgr, pitched, f"sls {H}x{W}->{Ho}x{Wo} {kind} bgr{bgr} pitched{int(pitched)}")


def test_sls_preprocess_walk():
    """258 frames of 9 x 5 -> 128 x 128: 4,227,072 pixels, one full trip of the 16384-block grid and a partial
    second; every frame differs, so a wrong frame index shows."""
    n, H, W, Ho, Wo = rr.SLS_WALK
    assert rr.SLS_GRID_ITEMS < n * Ho * Wo < 2 * rr.SLS_GRID_ITEMS
    run_sls(rr.sls_walk_frames(n, H, W), H, W, Ho, Wo, 0, False, "sls walk")


# ------------------------------------------------------------------------------------------- gather_rows
def run_gather(n, rb, src_off, dst_off, what, bad=True):
    lib = _lib.lib()
    src_np = rr.gather_src(rr.GATHER_N_SRC, rb)
    idx_np = rr.gather_idx(n, rr.GATHER_N_SRC, bad)
    src = Guarded(src_np.size, src_off, init=src_np, fill=0xFF)
    before = src.buf.clone()
    idx = dev(idx_np)

    def run():
        d = Guarded(n * rb, dst_off)
        check_rc(lib.vitmi_gather_rows(n, rb, src.ptr(), rr.GATHER_N_SRC, idx.data_ptr(), d.ptr(), stream()), what)
        return {"dst": d}
    got = twice_bytes(run, what, [src])
    assert torch.equal(src.buf, before) and torch.equal(idx.cpu(), tens(idx_np)), (what, "an input was written to")
    assert np.array_equal(got["dst"].bytes().reshape(n, rb), rr.gather_rows(src_np, idx_np)), (what, "not bitwise the reference")


@pytest.mark.parametrize("rb", rr.GATHER_ROW_BYTES)
def test_gather_rows(rb):
    """The 16-byte and the byte path, the latter also through src or dst four bytes off at row_bytes % 16 == 0;
    repeated indices, and -1, n_src, INT64_MIN and INT64_MAX giving zero rows; n = 0 writes nothing."""
    for so, do in ((0, 0), (4, 0), (0, 4)):
        run_gather(23, rb, so, do, f"gather rb{rb} src+{so} dst+{do}")
    src, dst = Guarded(rr.GATHER_N_SRC * rb, init=rr.gather_src(rr.GATHER_N_SRC, rb)), Guarded(64)
    refused(_lib.lib().vitmi_gather_rows, (0, rb, src.ptr(), rr.GATHER_N_SRC, dev(np.zeros(1, np.int64)).data_ptr(), dst.ptr(), stream()),
            "", [src, dst], "gather n = 0", rc_want=0)


@pytest.mark.parametrize("n,rb", rr.GATHER_WALKS, ids=[f"{n}x{rb}" for n, rb in rr.GATHER_WALKS])
def test_gather_rows_walk(n, rb):
    """Past one trip of the 16384-block grid on the 16-byte path (1030 rows of 65536 B) and on the byte path (1030
    rows of 4100 B)."""
    assert n * rb // (16 if rb % 16 == 0 else 1) > rr.SLS_GRID_ITEMS
    run_gather(n, rb, 0, 0, f"gather walk {n}x{rb}")


# ------------------------------------------------------------------------------------------- patch_keep
@pytest.mark.parametrize("np_", rr.KEEP_NPS)
def test_patch_keep(np_):
    """np on both sides of a 4-key LDS read, of one 256-patch chunk, of several, up to the whole 4096-key LDS array
    (np % 4 != 0 in a multi-chunk run ranks every patch against the 0xFFFFFFFF padding keys); K in {1, np / 2,
    np - 1, np}; keep and slot exact, slot the inverse of keep."""
    lib = _lib.lib()
    B = rr.KEEP_B
    for K in rr.keep_ks(np_):
        what = f"patch_keep np{np_} K{K}"

        def run():
            o = {"keep": Guarded(B * K * 4), "slot": Guarded(B * np_ * 4)}
            check_rc(lib.vitmi_patch_keep(B, np_, K, rr.KEEP_SEED, ref_patchdrop.PATCH_SITE, o["keep"].ptr(), o["slot"].ptr(), stream()),
                     what)
            return o
        got = twice_bytes(run, what)
        keep = got["keep"].bytes().view(np.int32).reshape(B, K)
        slot = got["slot"].bytes().view(np.int32).reshape(B, np_)
        wk, ws = rr.keep_slot_ref(rr.KEEP_SEED, B, np_, K)
        assert np.array_equal(keep, wk) and np.array_equal(slot, ws), (what, "not the reference's selection")
        for b in range(B):
            assert np.array_equal(slot[b, keep[b]], np.arange(K)) and int((slot[b] >= 0).sum()) == K, (what, b)


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    """The preconditions of the five entry points that tests/test_abi_loss.py and tests/test_abi_patchdrop.py do
    not make: VITMI_ERR_INVALID with a message that names the argument, nothing launched, every buffer unchanged.
    (Sizes too large for a real allocation are refused on the host before a pointer is looked at.)"""
    lib = _lib.lib()
    s = stream()
    # softmax_xent: the workspace's alignment
    B, C = 4, 8
    z, dl, row, loss, rec = din(torch.randn(B, C)), dout(B, C), dvec_out(B), dvec_out(1), dvec_out(8, init=torch.zeros(8))
    ws = dvec_out(64)
    la = dev(np.zeros(B, np.int64))
    bufs = [z, dl, row, loss, rec, ws]
    for off in (1, 2, 3):
        refused(lib.vitmi_softmax_xent, (B, C, z.ptr(), z.pitch, la.data_ptr(), None, None, None, 0, 0.0, 1, None, loss.ptr(), dl.ptr(),
                                         dl.pitch, rec.ptr(), ws.ptr() + off, 200, s), "4-byte aligned", bufs, f"xent workspace + {off}")
    # mix_batch: sizes past the launch's index range
    img, out = din(torch.randn(8, 8)), dout(8, 8)
    t = dev(np.zeros(16, np.int32))
    far = 1 << 60                                         # never dereferenced: refused on the host
    for dims, needle in (((1, 1, 65536, 65536), "too large"), ((65536, 65536, 1, 1), "too large"),
                         ((128, 128, 32768, 32768), "too large for one launch")):
        refused(lib.vitmi_mix_batch, (*dims, img.ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), far, s), needle, [img, out],
                f"mix_batch {dims}")
    # sls_preprocess
    H, W, Ho, Wo, n = 4, 5, 3, 3, 2
    src, o = Guarded(n * H * W * 3, init=np.zeros(n * H * W * 3, np.uint8)), dout(n, Ho * Wo)
    xo, xw, yo, yw = sls_tables(H, W, Ho, Wo)
    tb = [xo.data_ptr(), xw.data_ptr(), yo.data_ptr(), yw.data_ptr()]

    def sls(n_=n, H_=H, W_=W, src_=src.ptr(), ib=H * W * 3, rb=W * 3, Ho_=Ho, Wo_=Wo, tb_=tb, out=o.ptr()):
        return (n_, H_, W_, src_, ib, rb, 0, Ho_, Wo_, *tb_, out, s)
    cases = [("n = -1", sls(n_=-1), "bad sizes"), ("H = 0", sls(H_=0), "bad sizes"), ("W = 0", sls(W_=0), "bad sizes"),
             ("Ho = 0", sls(Ho_=0), "bad sizes"), ("Wo = -2", sls(Wo_=-2), "bad sizes"), ("null src", sls(src_=None), "null"),
             ("null out", sls(out=None), "null"), ("row_bytes < 3 W", sls(rb=3 * W - 1), "source layout"),
             ("img_bytes < row_bytes H", sls(ib=H * W * 3 - 1), "source layout")]
    cases += [(f"null table {i}", sls(tb_=[None if j == i else p for j, p in enumerate(tb)]), "null") for i in range(4)]
    for what, a, needle in cases:
        refused(lib.vitmi_sls_preprocess, a, needle, [src, o], f"sls_preprocess {what}")
    refused(lib.vitmi_sls_preprocess, sls(n_=0), "", [src, o], "sls_preprocess n = 0", rc_want=0)
    # gather_rows
    g_src, g_dst = Guarded(64, init=np.ones(64, np.uint8)), Guarded(64)
    gi = dev(np.zeros(4, np.int64))
    for what, a, needle in [("n = -1", (-1, 16, g_src.ptr(), 4, gi.data_ptr(), g_dst.ptr(), s), "bad sizes"),
                            ("row_bytes = 0", (4, 0, g_src.ptr(), 4, gi.data_ptr(), g_dst.ptr(), s), "bad sizes"),
                            ("null src", (4, 16, None, 4, gi.data_ptr(), g_dst.ptr(), s), "null"),
                            ("null idx", (4, 16, g_src.ptr(), 4, None, g_dst.ptr(), s), "null"),
                            ("null dst", (4, 16, g_src.ptr(), 4, gi.data_ptr(), None, s), "null")]:
        refused(lib.vitmi_gather_rows, a, needle, [g_src, g_dst], f"gather_rows {what}")
    # patch_keep: a refusal leaves keep and slot alone
    keep, slot = Guarded(64), Guarded(64)
    for what, (B_, np_, K_) in (("B = 0", (0, 4, 2)), ("K = 0", (2, 4, 0)), ("K > np", (2, 4, 5)), ("np = 4097", (1, 4097, 2))):
        refused(lib.vitmi_patch_keep, (B_, np_, K_, 1, 2, keep.ptr(), slot.ptr(), s), "1 <= K <= np <= 4096", [keep, slot], f"patch_keep {what}")
