"""tests/ref_recipe.py judged on the CPU (no GPU): the float64 reference agrees with torch's own operators and
autograd; the float32 emulations of the kernels' arithmetic sit inside the derived bounds, or match the bits,
at every case of the GPU matrix (the bounds are not vacuous, nothing is excluded, nothing skipped); and every
mutated emulation is REJECTED, by the bound or by the bit comparison, in every family where it applies.  The
rejections are printed.  The NaN-drop mutant -- the softmax kernel's lane accumulation as it stood before the
non-finite rule of include/vitmi.h -- is rejected by the non-finite cases of the GPU suite."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_patchdrop
import ref_recipe as rr
from oracle import sls_ref

f32, f64 = np.float32, np.float64
CAP = 1.0                        # fixed: an emulation conforms iff every element's |err| / tol <= 1


def judge(emu, ref):
    return {k: rr.ratio(emu[k], *ref[k]) for k in ("row", "loss", "dl")}


def conforms(emu, ref):
    return all(v <= CAP for v in judge(emu, ref).values())


def report(what, rejections, needed=1):
    print(f"MUTANT {what}: rejected by {len(rejections)} case(s): " + "; ".join(str(r) for r in rejections[:6]) +
          (" ..." if len(rejections) > 6 else ""))
    assert len(rejections) >= needed, (what, "not rejected")


# ------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("C", (1, 5, 65, 1000))
@pytest.mark.parametrize("eps", rr.XENT_SMOOTHINGS)
def test_xent_reference_is_torch_cross_entropy(C, eps):
    """Label form: F.cross_entropy(label_smoothing=); pair form: the probability-target form of the same call;
    dense form (sum(t) != 1): -sum q log_softmax(z) with q = (1 - eps) t + eps sum(t) / C; gradients by autograd."""
    B = 5
    b = rr.xent_batch("randn4", B, C)
    z = torch.from_numpy(b["z"]).double().requires_grad_(True)
    for form in rr.XENT_FORMS:
        ref = rr.xent(b["z"], smoothing=eps, **rr.form_args(b, form))
        if form == "labels":
            rows = F.cross_entropy(z, torch.from_numpy(b["la"]), reduction="none", label_smoothing=float(f32(eps)))
        else:
            t = torch.from_numpy(rr.ref_loss.target_dist(B, C, **rr.form_args(b, form))[0])
            if form == "pair":
                rows = F.cross_entropy(z, t, reduction="none", label_smoothing=float(f32(eps)))
            else:
                q = (1 - float(f32(eps))) * t + float(f32(eps)) * t.sum(1, keepdim=True) / C if eps else t
                rows = -(q * F.log_softmax(z, 1)).sum(1)
        (grad,) = torch.autograd.grad(rows.sum() / B, z)
        assert np.allclose(ref["row"][0], rows.detach().numpy(), rtol=1e-12, atol=1e-12), form
        assert np.allclose(ref["loss"][0], (rows.sum() / B).item(), rtol=1e-12, atol=1e-12), form
        assert np.allclose(ref["dl"][0], grad.numpy(), rtol=1e-12, atol=1e-13), form
        for k in ("row", "loss", "dl"):
            assert (ref[k][1] >= 0).all() and np.isfinite(ref[k][1]).all(), (form, k)   # 0: an all-zero target


@pytest.mark.parametrize("C", (5, 65, 1000))
def test_hits_are_torch_topk_without_ties(C):
    b = rr.xent_batch("randn4", 37, C)
    assert all(np.unique(r).size == C for r in b["z"])
    for k in (1, 5, C):
        top = torch.from_numpy(b["z"]).topk(k, 1).indices.numpy()
        want = np.array([b["la"][i] in top[i] for i in range(37)])
        assert np.array_equal(rr.hits(b["z"], b["la"], k), want), k


def test_hits_ties_nan_and_outside():
    z = np.zeros((4, 8), f32)
    z[3, 2] = np.nan
    lab = np.array([0, 7, 8, 2])
    assert rr.hits(z, lab, 1).tolist() == [True, False, False, False]       # the lower index wins the tie
    assert rr.hits(z, lab, 8).tolist() == [True, True, False, False]        # outside and NaN at the label: misses
    assert rr.hits(z, lab, 7).tolist() == [True, False, False, False]


def test_fold_is_the_promised_order():
    """Against a scalar restatement (loops, Python floats), bit for bit; against math.fsum to the fp64 roundings
    of B additions; and a NaN row makes the total NaN."""
    for B in (1, 3, 255, 256, 257, 513, 2051):
        rows = (rr.rng_of("fold", B).standard_normal(B) * 7).astype(f32)
        acc = [0.0] * 256
        for i in range(B):
            acc[i % 256] += float(rows[i])
        for w in range(4):
            x = acc[64 * w:64 * w + 64]
            for o in (32, 16, 8, 4, 2, 1):
                x = [x[i] + x[i ^ o] for i in range(64)]
            acc[64 * w] = x[0]
        want = ((acc[0] + acc[64]) + acc[128]) + acc[192]
        got = rr.fold(rows)
        assert got == want, B
        exact = math.fsum(float(r) for r in rows)
        assert abs(got - exact) <= (B + 10) * 2.0 ** -53 * float(np.abs(rows.astype(f64)).sum())
        assert rr.fold_loss(rows) == f32(want / B)
    rows[5] = np.nan
    assert math.isnan(rr.fold(rows))


# ------------------------------------------------------------------------------------------- xent: emulation
def shape_cases(C):
    return [c for c in rr.xent_shape_cases() if c[1] == C]


@pytest.mark.parametrize("C", sorted({c[1] for c in rr.xent_shape_cases()}))
def test_xent_emulation_conforms_at_every_shape(C):
    """Every (B, C, way) of ref_recipe.xent_shape_cases(), the large batches at C in {5, 8} included, in every form
    and at both smoothings."""
    worst = {"row": 0.0, "loss": 0.0, "dl": 0.0}
    for (B, _, way), form, eps in itertools.product(shape_cases(C), rr.XENT_FORMS, rr.XENT_SMOOTHINGS):
        if way not in rr.xent_ways(C, form):
            continue
        b = rr.xent_batch("randn4", B, C)
        kw = dict(smoothing=eps, W=rr.width(C, way), **rr.form_args(b, form))
        r = judge(rr.emulate_xent(b["z"], **kw), rr.xent(b["z"], **kw))
        for k, v in r.items():
            worst[k] = max(worst[k], v)
            assert v <= CAP, (B, C, way, form, eps, k, v)
    print(f"EMU xent C{C}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("fam", rr.XENT_FAMILIES)
def test_xent_emulation_conforms_in_every_family(fam):
    for C, form, eps, W in itertools.product(rr.XENT_FAMILY_CS, rr.XENT_FORMS, rr.XENT_SMOOTHINGS, (1, 4)):
        if (W == 4 and C % 4) or (fam == "masked" and eps):
            continue
        b = rr.xent_batch(fam, 3, C)
        kw = dict(smoothing=eps, W=W, **rr.form_args(b, form))
        ref = rr.xent(b["z"], **kw)
        emu = rr.emulate_xent(b["z"], **kw)
        r = judge(emu, ref)
        assert all(v <= CAP for v in r.values()), (fam, C, form, eps, W, r)
        if fam == "masked":
            masked = np.isinf(b["z"])
            assert masked.any() and np.isfinite(ref["row"][0]).all() and (emu["dl"][masked] == 0).all()
            assert (ref["dl"][1][masked] == 0).all()              # an exact zero is demanded there


def nan_cases():
    """(C, way, name, cols) of the non-finite cases."""
    return [(C, way, name, cols) for C in rr.XENT_NAN_CS for way in (("auto", "base") if C % 4 == 0 else ("auto",))
            for name, cols in rr.nan_columns(C)]


def test_xent_nan_rows_and_the_nan_drop_mutant():
    """The emulation with the non-finite rule conforms at every NaN case (row, loss and the row's gradient NaN,
    the other rows' bits those of the batch without the NaN).  The NaN-drop mutant is rejected by them: on the
    scalar path wherever the NaN is a lane's first element, on the 16-byte path at the whole group."""
    rejected = []
    for (C, way, name, cols), form, eps in itertools.product(nan_cases(), rr.XENT_FORMS, rr.XENT_SMOOTHINGS):
        b = rr.nan_batch(C, cols)
        W = rr.width(C, way)
        kw = dict(smoothing=eps, W=W, **rr.form_args(b, form))
        ref = rr.xent(b["z"], **kw)
        assert np.isnan(ref["row"][0][1]) and np.isnan(ref["loss"][0]).all() and np.isnan(ref["dl"][0][1]).all()
        assert np.isfinite(ref["row"][0][[0, 2]]).all() and np.isfinite(ref["dl"][0][[0, 2]]).all()
        emu = rr.emulate_xent(b["z"], **kw)
        assert conforms(emu, ref), (C, way, name, form, eps, judge(emu, ref))
        clean = dict(b, z=np.where(np.isnan(b["z"]), f32(0), b["z"]))
        other = rr.emulate_xent(clean["z"], **dict(kw, **rr.form_args(clean, form)))
        for k in ("row", "dl"):
            assert rr.same_bits_nan(emu[k][[0, 2]], other[k][[0, 2]]), (C, way, name, form, k)
        mut = rr.emulate_xent(b["z"], mut="nan_drop", **kw)
        if not conforms(mut, ref):
            rejected.append((C, "W%d" % W, name, form, eps))
    got = {(C, w, name) for C, w, name, _, _ in rejected}
    for C in rr.XENT_NAN_CS:
        for name in ("col0", "col5", "col63"):
            assert (C, "W1", name) in got, (C, name, "the scalar path's dropped NaN was not caught")
        if C % 4 == 0:
            assert (C, "W4", "group") in got, (C, "the 16-byte path's dropped group was not caught")
    report("xent nan_drop", rejected)


def test_xent_mutants_are_rejected():
    B = 5
    for mut in rr.MUTATIONS["xent"]:
        if mut in ("nan_drop", "tie_le"):
            continue                                              # their own tests, above and below
        rejected = []
        for C, form, eps, W in itertools.product((5, 68, 260, 1028, 4099), rr.XENT_FORMS, rr.XENT_SMOOTHINGS, (1, 4)):
            if W == 4 and C % 4:
                continue
            applies = {"no_rescale": C > 64 * W, "sumq_one": form == "dense", "unif_noS": form == "dense" and eps > 0,
                       "wb_lam": form == "pair", "no_invB": True}[mut]
            if not applies:
                continue
            b = rr.xent_batch("randn4", B, C)
            kw = dict(smoothing=eps, W=W, **rr.form_args(b, form))
            if conforms(rr.emulate_xent(b["z"], mut=mut, **kw), rr.xent(b["z"], **kw)):
                assert False, (mut, "conforms where it applies", C, form, eps, W)
            rejected.append((C, form, eps, W))
        report(f"xent {mut}", rejected)


def test_tie_rule_mutant_is_rejected():
    rejected = []
    for name, z, lab in rr.tie_cases():
        C = z.shape[1]
        for k in (1, 5, C):
            want = rr.hits(z, lab, k)
            if name == "equal":
                assert want.tolist() == [k == C]
            else:
                assert want.tolist() == {1: [True, False, True, False], 5: [True] * 4, C: [True] * 4}[k]
            if not np.array_equal(rr.hits(z, lab, k, mut="tie_le"), want):
                rejected.append((name, k))
    assert ("lanes", 1) in rejected and ("equal", 65535) in rejected
    report("xent tie_le", rejected)


# ------------------------------------------------------------------------------------------- mix
def mix_shapes():
    return [(H, W, True) for H, W in rr.MIX_VEC] + [(H, W, False) for H, W in rr.MIX_SCALAR + rr.MIX_OFFSET]


def test_mix_emulation_matches_the_bits_and_mutants_do_not():
    rejected = {m: [] for m in rr.MUTATIONS["mix"]}
    fill = f32(-77.0)
    for H, W, vec in mix_shapes():
        img = rr.mix_image(rr.MIX_B, rr.MIX_C, H, W)
        for name, perm, lam, box in rr.mix_tables(H, W):
            want = rr.mix(img, perm, lam, box)
            assert rr.same_bits_nan(rr.emulate_mix(img, perm, lam, box, vec, fill), want), (H, W, name)
            for m in rejected:
                if not rr.same_bits_nan(rr.emulate_mix(img, perm, lam, box, vec, fill, mut=m), want):
                    rejected[m].append((H, W, name))
        # the copy case: a NaN partner is not read
        perm, lam, box = rr.mix_copy_table()
        nimg = rr.mix_image(rr.MIX_B, rr.MIX_C, H, W, nan_sample=0)
        want = rr.mix(nimg, perm, lam, box)
        assert rr.same_bits_nan(want, nimg) and not np.isnan(want[1]).any()
        assert rr.same_bits_nan(rr.emulate_mix(nimg, perm, lam, box, vec, fill), want), (H, W, "copy")
        if not rr.same_bits_nan(rr.emulate_mix(nimg, perm, lam, box, vec, fill, mut="box_unclamped"), want):
            rejected["box_unclamped"].append((H, W, "copy"))
    for m, r in rejected.items():
        report(f"mix {m}", r)
    # what the matrix adds: groups past the first 256 of a chunk, and chunks past the first
    assert any(H * W // 4 > 256 for H, W in rr.MIX_VEC) and {(H, W) for H, W, _ in rejected["u0_only"]} >= {(257, 4), (33, 128)}
    assert {(H, W) for H, W, _ in rejected["plane_chunk"]} >= {(1025, 4), (1, 4100), (65, 128)}


# ------------------------------------------------------------------------------------------- sls
@pytest.mark.parametrize("H,W,Ho,Wo", rr.SLS_SHAPES)
def test_sls_restatement_is_the_oracle_dense_and_pitched(H, W, Ho, Wo):
    rejected = {m: [] for m in rr.MUTATIONS["sls"] if m != "one_trip"}
    n = 2
    for kind, bgr in itertools.product(rr.SLS_FRAMES, (0, 1)):
        fr = rr.sls_frames(kind, n, H, W)
        want = np.stack([sls_ref.sls_image(f if bgr else f[..., ::-1], Wo, Ho) for f in fr])
        for pitched in (False, True):
            buf, ib, rb = rr.sls_pack(fr, pitched)
            got = rr.sls_image(buf, n, H, W, ib, rb, bgr, Ho, Wo)
            assert rr.same_bits_nan(got, want), (kind, bgr, pitched)
            for m in rejected:
                if not rr.same_bits_nan(rr.sls_image(buf, n, H, W, ib, rb, bgr, Ho, Wo, mut=m), want):
                    rejected[m].append((kind, bgr, pitched))
    for m in rr.EQUIVALENT["sls"]:
        assert not rejected.pop(m), (m, "changes a value after all: move it to MUTATIONS proper")
    print(f"MUTANT sls {H}x{W}->{Ho}x{Wo}: rejecting cases of 16: " + " ".join(f"{m} {len(r)}" for m, r in rejected.items()))


def test_sls_mutants_are_rejected():
    """Every value mutant by the random frames of the full-size case (and whatever else catches it)."""
    H, W, Ho, Wo = rr.SLS_SHAPES[-1]
    fr = rr.sls_frames("random", 1, H, W)
    buf, ib, rb = rr.sls_pack(fr, True)
    want = rr.sls_image(buf, 1, H, W, ib, rb, 0, Ho, Wo)
    for m in rr.MUTATIONS["sls"]:
        if m in rr.EQUIVALENT["sls"] or m == "one_trip":
            continue
        rej = [] if rr.same_bits_nan(rr.sls_image(buf, 1, H, W, ib, rb, 0, Ho, Wo, mut=m), want) else [(H, W, "random")]
        report(f"sls {m}", rej)


def test_sls_walk_frames_differ_and_one_trip_is_rejected():
    n, H, W, Ho, Wo = rr.SLS_WALK
    items = n * Ho * Wo
    assert rr.SLS_GRID_ITEMS < items < 2 * rr.SLS_GRID_ITEMS and items == 4227072
    fr = rr.sls_walk_frames(n, H, W)
    buf, ib, rb = rr.sls_pack(fr, False)
    want = rr.sls_image(buf, n, H, W, ib, rb, 0, Ho, Wo)
    assert len({want[i].tobytes() for i in range(n)}) == n, "two frames of the walk give the same image"
    short = rr.one_trip(want.copy(), f32(-77.0), items, "one_trip")
    report("sls one_trip", [] if rr.same_bits_nan(short, want) else [rr.SLS_WALK])


# ------------------------------------------------------------------------------------------- gather
def test_gather_restatement_and_mutants():
    rej = {m: [] for m in rr.MUTATIONS["gather"]}
    for rb in rr.GATHER_ROW_BYTES:
        src = rr.gather_src(rr.GATHER_N_SRC, rb)
        idx = rr.gather_idx(23, rr.GATHER_N_SRC)
        ok = (idx >= 0) & (idx < rr.GATHER_N_SRC)
        assert (~ok).sum() == 4 and len(set(idx[ok])) < ok.sum()
        want = rr.gather_rows(src, idx)
        t = torch.from_numpy(src)[torch.from_numpy(np.where(ok, idx, 0))].numpy()
        assert np.array_equal(want[ok], t[ok]) and not want[~ok].any() and want[ok].all()
        if not np.array_equal(rr.gather_rows(src, idx, mut="no_zero_row"), want):
            rej["no_zero_row"].append(rb)
    for n, rb in rr.GATHER_WALKS:
        unit = 16 if rb % 16 == 0 else 1
        items = n * rb // unit
        assert rr.SLS_GRID_ITEMS < items < 2 * rr.SLS_GRID_ITEMS
        src = rr.gather_src(rr.GATHER_N_SRC, rb)
        want = rr.gather_rows(src, rr.gather_idx(n, rr.GATHER_N_SRC))
        if not np.array_equal(rr.one_trip(want.copy(), np.uint8(0x4B), items, "one_trip"), want):
            rej["one_trip"].append((n, rb))
    for m, r in rej.items():
        report(f"gather {m}", r)
    assert len(rej["one_trip"]) == 2


# ------------------------------------------------------------------------------------------- patch_keep
def test_keep_restatement_and_mutants():
    rej = {m: [] for m in rr.MUTATIONS["keep"]}
    site = ref_patchdrop.PATCH_SITE
    for np_ in rr.KEEP_NPS:
        for K in rr.keep_ks(np_):
            keep, slot = rr.keep_slot(rr.KEEP_SEED, site, rr.KEEP_B, np_, K)
            k2, s2 = rr.keep_slot_ref(rr.KEEP_SEED, rr.KEEP_B, np_, K)
            assert np.array_equal(keep, k2) and np.array_equal(slot, s2), (np_, K)
            assert (np.diff(keep, axis=1) > 0).all() and keep.min() >= 0 and keep.max() < np_
            for b in range(rr.KEEP_B):
                assert np.array_equal(slot[b, keep[b]], np.arange(K)) and (slot[b] >= 0).sum() == K
            for m in rej:
                km, sm = rr.keep_slot(rr.KEEP_SEED, site, rr.KEEP_B, np_, K, mut=m)
                if not (np.array_equal(km, keep) and np.array_equal(sm, slot)):
                    rej[m].append((np_, K))
    for m, r in rej.items():
        report(f"keep {m}", r)
    # what the matrix adds: padding keys ranked against in a multi-chunk run
    assert {n for n, _ in rej["pad_zero"]} >= {257, 259, 1023, 1025, 4093, 4094, 4095}
    assert {n for n, _ in rej["chunk_base"]} >= {257, 259, 1023, 1025, 4093, 4094, 4095, 4096}
