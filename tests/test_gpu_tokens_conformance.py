"""Token path, head, loss, cast, split, dropout-mask and small-Dense conformance on the MI355X: every kernel
of csrc/elementwise.hip (but the column sums and folds, which tests/test_gpu_ln_conformance.py covers),
csrc/split.hip, csrc/dense.hip and the gathered kernels of csrc/patchdrop.hip against tests/ref_tokens.py:
bit for bit where the arithmetic pins the bits, by the derived PER-ELEMENT bound elsewhere.

The library is called directly (vitmi._lib.lib()), so every buffer is the test's own guarded allocation:
inputs between NaN guard rows (and NaN guard columns, with a pitch that differs per buffer, wherever the
entry point takes a pitch), outputs and accumulators between fixed-bit guards; accumulating outputs start
from a non-zero value.  (The integer lists -- keep, slot, the CE labels -- are plain device tensors: the
guarded buffers hold fp32 and bf16 only.)  A HIP error ends the session (check_rc / sync of the attention suite).

Every case asserts
  1. every element within tol, or bitwise equal where the reference says so (the worst ratio is printed),
  2. the guards around every buffer bitwise intact, no NaN in a valid output (unless the input held one),
  3. a second run bitwise equal,
  4. for the launches that record a statistic (cast_kernel, split3_kernel, split_f8_kernel,
     split_f8_batch_kernel): exactly that kernel, once; for all others: nothing recorded.
The matrix is ref_tokens' (the smallest shapes that reach each arm, and one walk of every grid-stride loop past
the 8192-block cap with an odd last trip).  The refusals use only calls that tests/test_abi_tokens.py shows to
be refused on the host before any launch."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_gemm as rg  # noqa: E402
import ref_tokens as rt  # noqa: E402
from kstats import kernel_stats  # noqa: E402
from oracle import vit_ref  # noqa: E402
from test_gpu_attn_conformance import check_rc, same_bits, stream, sync  # noqa: E402
from test_gpu_ln_conformance import refused  # noqa: E402
from vitmi import _lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
T_F32, T_BF16 = 0, 1
CE, MSE = 0, 1


def up(n, m):
    return rt.cdiv(n, m) * m


# ------------------------------------------------------------------------------------------- buffers
def din(values, pad=0, dtype=F32):
    """A [rows, cols] input of pitch cols + pad between NaN guard rows (and NaN guard columns)."""
    r, c = values.shape
    return rg.padded(r, c, c + pad, dtype, "nan").set(values).to(DEV)


def dvec(v, dtype=F32):
    """A flat input of n elements (16-byte aligned base) between NaN guards."""
    n = v.numel()
    return rg.padded(1, n, up(n, 8) + 8, dtype, "nan").set(v.reshape(1, -1)).to(DEV)


def dout(rows, cols, pad=0, dtype=F32, init=None):
    p = rg.padded(rows, cols, cols + pad, dtype, "guard")
    if init is not None:
        p.set(init.reshape(rows, cols))
    return p.to(DEV)


def dvec_out(n, dtype=F32, init=None):
    p = rg.padded(1, n, up(n, 8) + 8, dtype, "guard")
    if init is not None:
        p.set(init.reshape(1, -1))
    return p.to(DEV)


def ptr(p):
    return None if p is None else p.ptr()


def host(p):
    return p.view.cpu()


def idx(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def assert_stat(st, name, what):
    if name is None:
        assert not st.k, (what, "a launch that records no statistic recorded one", st.k)
        return
    hits = [n for n in st.k if name in n]
    assert len(hits) == 1 and st.k[hits[0]] == 1 and len(st.k) == 1, (what, name, st.k)


def twice(fn, what, stat=None, inputs=(), nan_ok=False, valid=None):
    """fn() twice (the first under kernel_stats); assertions 2 - 4; the first run's outputs {name: Padded}.
    valid: {name: columns that hold numbers} for rows whose tail holds e4m3 bytes."""
    with kernel_stats() as st:
        a = fn()
    b = fn()
    sync(what)
    assert_stat(st, stat, what)
    for k, p in a.items():
        assert rg.guards_intact(p), (what, f"guards of {k} changed")
        vals = host(p)
        if valid and k in valid:
            vals = vals[:, :valid[k]]
        assert nan_ok or not torch.isnan(vals.float()).any(), (what, k, "NaN in a valid output")
        assert same_bits(p, b[k]), (what, k, "second run differs")
    for p in inputs:
        assert rg.guards_intact(p), (what, "guards of an input changed")
    return a


def exact(got, want, what):
    assert rt.same_bits(got, want), (what, "not bitwise the reference",
                                     int((rt.bits_of(got) != rt.bits_of(want)).sum()) if got.shape == want.shape else got.shape)


class Worst(dict):
    def add(self, k, v):
        self[k] = max(self.get(k, 0.0), v)

    def report(self, what):
        print(f"CONF tokens {what}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in self.items()))
        for k, v in self.items():
            assert v <= 1.0, (what, k, v)


# ------------------------------------------------------------------------------------------- im2col
def image(B, C, S, with_special):
    img = rt.family("rows", B * C * S, S, "img")
    if with_special:
        flat = img.view(-1)
        flat[::5] = rt.special(flat[::5].numel())
    return img


@pytest.mark.parametrize("C,S,P", rt.IM2COL_SHAPES, ids=[f"C{c}-S{s}-P{p}" for c, s, p in rt.IM2COL_SHAPES])
def test_im2col(C, S, P):
    """Both forms, both output types, bit for bit; B = 3 carries the special values (a move keeps them; the bf16
    form rounds them to nearest even).  Gathered: K in {1, np / 2, np}, and a keep list with a -1 and an np."""
    lib = _lib.lib()
    np_, Kc = (S // P) ** 2, C * P * P
    for B in rt.IM2COL_BS:
        sp = B == 3
        img4 = image(B, C, S, sp)
        img = din(img4)
        for dtype, T in ((T_F32, F32), (T_BF16, BF)):
            what = f"im2col C{C} S{S} P{P} B{B} {T}"

            def full():
                o = dout(B * np_, Kc, 0, T)
                check_rc(lib.vitmi_patch_im2col(dtype, B, C, S, P, img.ptr(), o.ptr(), stream()), what)
                return {"patches": o}
            got = twice(full, what, None, [img], nan_ok=sp)
            exact(host(got["patches"]), rt.im2col_expected(img4.view(B, C, S, S), P, T == BF), what)
            for K in sorted({1, max(np_ // 2, 1), np_}):
                bad = K > 1 and K == max(np_ // 2, 1)
                keep = rt.keep_lists(B, np_, K, bad=bad)
                kd = idx(keep)

                def gathered():
                    o = dout(B * K, Kc, 0, T)
                    check_rc(lib.vitmi_patch_im2col_keep(dtype, B, C, S, P, K, kd.data_ptr(), img.ptr(), o.ptr(), stream()),
                             what)
                    return {"patches": o}
                gk = twice(gathered, f"{what} keep {K}", None, [img], nan_ok=sp)
                exact(host(gk["patches"]), rt.im2col_expected(img4.view(B, C, S, S), P, T == BF, keep), f"{what} keep {K}")
                assert torch.equal(kd.cpu(), torch.from_numpy(keep))


# ------------------------------------------------------------------------------------------- token assembly
def token_problem(fam, B, np_, D, K):
    pf = "int" if fam == "int" else "randn"
    return dict(tok=rt.family(fam, B * K, D, "tok"), cls=rt.family(pf, 1, D, "cls")[0], pos=rt.family(pf, np_ + 1, D, "pos"),
                dx=rt.family(fam, B, (K + 1) * D, "dx"), ppos=rt.family(pf, np_ + 1, D, "ppos"),
                pcls=rt.family(pf, 1, D, "pcls")[0])


def run_tokens(B, np_, D, fam, keepform, fwd_combos, bwd_combos, w, bad=True):
    lib = _lib.lib()
    K = max(np_ // 2, 1) if keepform else np_
    if keepform == "all":
        K = np_
    pr = token_problem(fam, B, np_, D, K)
    keep = rt.keep_lists(B, np_, K, bad=bad and K > 1) if keepform else None
    slot = rt.slot_lists(rt.keep_lists(B, np_, K), np_, bad=bad and np_ > 1) if keepform else None
    kd, sd = (idx(keep), idx(slot)) if keepform else (None, None)
    tok, cls, pos = din(pr["tok"]), dvec(pr["cls"]), din(pr["pos"])
    dx = din(pr["dx"].view(B * (K + 1), D))
    ins = [tok, cls, pos, dx]
    tag = f"B{B} np{np_} D{D} {fam}" + (f" keep{K}" if keepform else "")
    for use_cls, use_pos in fwd_combos:
        what = f"assemble {tag} cls{int(use_cls)} pos{int(use_pos)}"

        def fwd():
            x = dout(B * (K + 1), D)
            c, p = (cls.ptr() if use_cls else None), (pos.ptr() if use_pos else None)
            if keepform:
                rc = lib.vitmi_tokens_assemble_keep(B, np_, K, D, tok.ptr(), c, p, kd.data_ptr(), x.ptr(), stream())
            else:
                rc = lib.vitmi_tokens_assemble(B, np_, D, tok.ptr(), c, p, x.ptr(), stream())
            check_rc(rc, what)
            return {"x": x}
        got = twice(fwd, what, None, ins)
        want = rt.assemble(pr["tok"], pr["cls"] if use_cls else None, pr["pos"] if use_pos else None, B, np_, D, keep)
        exact(host(got["x"]), want.view(B * (K + 1), D), what)
    for outs in bwd_combos:
        what = f"assemble_bwd {tag} {'+'.join(outs)}"

        def bwd():
            o = {}
            if "dtok" in outs:
                o["dtok"] = dout(B * K, D)
            if "dtok_lp" in outs:
                o["dtok_lp"] = dout(B * K, D, 0, BF)
            if "dcls" in outs:
                o["dcls"] = dvec_out(D, init=pr["pcls"])
            if "dpos" in outs:
                o["dpos"] = dout(np_ + 1, D, 0, F32, pr["ppos"])
            a = [dx.ptr(), ptr(o.get("dtok")), ptr(o.get("dtok_lp")), ptr(o.get("dcls")), ptr(o.get("dpos"))]
            if keepform:
                rc = lib.vitmi_tokens_assemble_keep_bwd(B, np_, K, D, *a, sd.data_ptr(), stream())
            else:
                rc = lib.vitmi_tokens_assemble_bwd(B, np_, D, *a, stream())
            check_rc(rc, what)
            return o
        got = twice(bwd, what, None, ins)
        dtok, dtok_lp = rt.split_bwd(pr["dx"], B, K, D)
        if "dtok" in got:
            exact(host(got["dtok"]), dtok, what)
        if "dtok_lp" in got:
            exact(host(got["dtok_lp"]), dtok_lp, what)
        ref = rt.pos_bwd(pr["dx"], pr["ppos"] if "dpos" in outs else None, pr["pcls"] if "dcls" in outs else None, B, np_, D,
                         slot)
        for k, (ex, r, tol) in ref.items():
            g = host(got[k])
            w.add(k, rt.worst_ratio(g, r, tol))
            exact(g, ex, f"{what} {k}")
            if fam == "int":
                assert torch.equal(g.double(), r), (what, k, "integers: not the exact sum")


FWD_ALL = tuple(itertools.product((True, False), (True, False)))
BWD_ALL = (("dtok",), ("dtok_lp",), ("dcls",), ("dpos",), ("dtok", "dtok_lp", "dcls", "dpos"))


@pytest.mark.parametrize("keepform", (False, True), ids=("full", "keep"))
@pytest.mark.parametrize("D", rt.TOKEN_DS)
def test_tokens(D, keepform):
    """tokens_assemble(_keep) and its backward: cls and pos each present and absent, each backward output alone
    and all together; B on both sides of the unrolled-by-8 batch loop; ``int`` and ``cancel`` through the sums.
    The gathered form carries a -1 and an np in its keep list, a K and a -7 in its slot list."""
    w = Worst()
    for np_, B in itertools.product(rt.TOKEN_NPS, rt.TOKEN_BS):
        run_tokens(B, np_, D, "rows", keepform, FWD_ALL, BWD_ALL, w)
        for fam in ("int", "cancel"):
            run_tokens(B, np_, D, fam, keepform, FWD_ALL[:1], BWD_ALL[-1:], w)
    w.report(f"tokens D{D} {'keep' if keepform else 'full'}")


@pytest.mark.parametrize("keepform", (False, "all"), ids=("full", "keep"))
def test_tokens_walk(keepform):
    """B (np + 1) D / 4 and B np D / 4 past one trip of the capped grid (2^21 items) by an odd amount: the second
    trip of tokens_assemble(_keep)_kernel and tokens_split_bwd_kernel."""
    w = Worst()
    B, np_, D = rt.TOKEN_WALK_FWD
    items = B * (np_ + 1) * D // 4
    assert rt.GRID_ITEMS + 300 < items < rt.GRID_ITEMS + 4096 and (items - rt.GRID_ITEMS) % 256
    run_tokens(B, np_, D, "rows", keepform, FWD_ALL[:1], (), w, bad=False)
    B, np_, D = rt.TOKEN_WALK_BWD
    items = B * np_ * D // 4
    assert rt.GRID_ITEMS + 300 < items < rt.GRID_ITEMS + 4096 and (items - rt.GRID_ITEMS) % 256
    run_tokens(B, np_, D, "rows", keepform, (), BWD_ALL[-1:], w, bad=False)
    w.report(f"tokens walk {'keep' if keepform else 'full'}")


# ------------------------------------------------------------------------------------------- casts
def run_cast(x, what, nan_ok=False):
    lib = _lib.lib()
    n = x.numel()
    src = dvec(x)

    def down():
        o = dvec_out(n, BF)
        check_rc(lib.vitmi_cast_f32_bf16(n, src.ptr(), o.ptr(), stream()), what)
        return {"bf16": o}
    got = twice(down, f"{what} down", "cast_kernel", [src], nan_ok)
    lo = host(got["bf16"])[0]
    exact(lo, rt.cast_down(x), f"{what} down")
    src16 = dvec(lo, BF)

    def upc():
        o = dvec_out(n, F32)
        check_rc(lib.vitmi_cast_bf16_f32(n, src16.ptr(), o.ptr(), stream()), what)
        return {"f32": o}
    got = twice(upc, f"{what} up", None, [src16], nan_ok)
    exact(host(got["f32"])[0], rt.cast_up(lo), f"{what} up")


@pytest.mark.parametrize("n", rt.CAST_NS)
def test_cast(n):
    """Both directions at n below, at and above one 8-element vector, and the walk: n / 8 past 8192 x 256 items by
    300 and a scalar tail of 5."""
    if n > 2 ** 24:
        assert n // 8 > rt.GRID_ITEMS and n % 8
    run_cast(rt.family("rows", 1, n, "cast")[0] * 3, f"cast n{n}")


def test_cast_special():
    run_cast(rt.special(rt.CAST_SPECIAL_N), "cast special", nan_ok=True)


# ------------------------------------------------------------------------------------------- splits
def run_split(x, what, nan_ok=False, patterns_x3=(0, 1), patterns_f8=None, copies=(False, True), pads=(8, 12, 4)):
    lib = _lib.lib()
    rows, K = x.shape
    src = din(x, pads[0])
    if patterns_f8 is None:
        patterns_f8 = rt.f8_patterns(K)
    for kind, pattern, copy in [("x3", p, c) for p in patterns_x3 for c in copies] + \
                               [("f8", p, c) for p in patterns_f8 for c in copies]:
        width = 3 * K if kind == "x3" else rt.f8_width(K, pattern)
        tag = f"{what} {kind} pattern {pattern} copy{int(copy)}"
        fn = lib.vitmi_split_bf16x3 if kind == "x3" else lib.vitmi_split_bf16f8

        def run():
            o = {"dst": dout(rows, width, pads[1], BF)}
            if copy:
                o["hi"] = dout(rows, K, pads[2], BF)
            h = o.get("hi")
            check_rc(fn(rows, K, src.ptr(), src.pitch, o["dst"].ptr(), o["dst"].pitch, pattern, ptr(h), h.pitch if h else 0,
                        stream()), tag)
            return o
        got = twice(run, tag, "split3_kernel" if kind == "x3" else "split_f8_kernel", [src], nan_ok,
                    valid=None if kind == "x3" else {"dst": K})
        want, hi = rt.split_x3(x, pattern) if kind == "x3" else rt.split_f8(x, pattern)
        if kind == "x3":
            exact(host(got["dst"]), want, tag)
        else:
            assert torch.equal(rt.bits_of(host(got["dst"])), rt.bits_of(want)), (tag, "not bitwise the reference")
        if copy:
            exact(host(got["hi"]), hi, f"{tag} hi copy")


@pytest.mark.parametrize("rows,K", rt.SPLIT_SHAPES, ids=[f"{r}x{k}" for r, k in rt.SPLIT_SHAPES])
def test_split(rows, K):
    """split_bf16x3 (both patterns) and split_bf16f8 (the patterns K allows), with and without the hi copy, every
    pitch above the row and different; then the special values (the f8 family without NaN and infinity)."""
    run_split(rt.family("rows", rows, K, "split") * 3, f"split {rows}x{K}")
    run_split(rt.special(rows * K).view(rows, K), f"split {rows}x{K} special", nan_ok=True, patterns_f8=(), copies=(True,))
    if rt.f8_patterns(K):
        run_split(rt.special(rows * K, f8=True).view(rows, K), f"split {rows}x{K} special f8", patterns_x3=(), copies=(True,))


@pytest.mark.parametrize("kind", ("x3", "f8"))
def test_split_walk(kind):
    """rows K / 4 past one trip of the capped grid (2^21 items): the second trip of split3_kernel and
    split_f8_kernel."""
    rows, K = rt.SPLIT_WALK_X3 if kind == "x3" else rt.SPLIT_WALK_F8
    assert rows * K // 4 > rt.GRID_ITEMS and (kind == "f8" or (rows * K // 4 - rt.GRID_ITEMS) % 256)
    x = rt.family("rows", rows, K, "splitwalk") * 3
    if kind == "x3":
        run_split(x, "split walk", patterns_x3=(0,), patterns_f8=(), copies=(True,), pads=(4, 8, 12))
    else:
        run_split(x, "split walk", patterns_x3=(), patterns_f8=(1, 2), copies=(True,), pads=(4, 8, 12))


@pytest.mark.parametrize("which", range(len(rt.BATCH_SETS)), ids=[f"n{len(s)}" for s in rt.BATCH_SETS])
def test_split_weights_batch(which):
    """vitmi_split_bf16f8_weights_mixed: 1, 3 and 8 weights of unequal K with patterns 1 and 3 mixed (the 8-weight
    set is past 2^21 items: the second trip of split_f8_batch_kernel), each bitwise the single-weight split;
    vitmi_split_bf16f8_weights is the same call with pattern 1 throughout."""
    lib = _lib.lib()
    shapes = rt.BATCH_SETS[which]
    n = len(shapes)
    xs = [rt.family("rows", r, K, "batch", j) * 3 for j, (r, K, _) in enumerate(shapes)]
    srcs = [din(x) for x in xs]
    if n == 8:
        assert sum(r * K // 4 for r, K, _ in shapes) > rt.GRID_ITEMS
    for mixed in (True, False):
        pats = [p if mixed else 1 for _, _, p in shapes]
        what = f"split weights n{n} {'mixed' if mixed else 'plain'}"

        def run():
            outs = [dout(r, rt.f8_width(K, p), 0, BF) for (r, K, _), p in zip(shapes, pats)]
            a = ((ctypes.c_void_p * n)(*[s.ptr() for s in srcs]), (ctypes.c_void_p * n)(*[o.ptr() for o in outs]),
                 (ctypes.c_int64 * n)(*[r for r, _, _ in shapes]), (ctypes.c_int64 * n)(*[K for _, K, _ in shapes]))
            if mixed:
                rc = lib.vitmi_split_bf16f8_weights_mixed(n, *a, (ctypes.c_int * n)(*pats), stream())
            else:
                rc = lib.vitmi_split_bf16f8_weights(n, *a, stream())
            check_rc(rc, what)
            return {f"w{j}": o for j, o in enumerate(outs)}
        got = twice(run, what, "split_f8_batch_kernel", srcs, valid={f"w{j}": K for j, (_, K, _) in enumerate(shapes)})
        for j, ((r, K, _), p) in enumerate(zip(shapes, pats)):
            want, _ = rt.split_f8(xs[j], p)
            assert torch.equal(rt.bits_of(host(got[f"w{j}"])), rt.bits_of(want)), (what, j, "not bitwise the reference")


# ------------------------------------------------------------------------------------------- dropout mask
def run_dropout(M, N, what, settings, pads):
    lib = _lib.lib()
    x = rt.family("rows", M, N, "drop") * 3
    for (thresh, scale), T, pad in itertools.product(settings, (F32, BF), pads):
        src = din(x, pad)
        tag = f"{what} thresh {thresh} {T} pad {pad}"
        seed, site = 1234567 + M, 0x10000000 + N

        def run():
            o = dout(M, N, pad and pad + 4, T)
            check_rc(lib.vitmi_dropout_apply(M, N, src.ptr(), src.pitch, o.ptr(), T_F32 if T == F32 else T_BF16, o.pitch, seed,
                                             site, thresh, scale, stream()), tag)
            return {"y": o}
        got = twice(run, tag, None, [src])
        want = rt.dropout_apply(x, seed, site, thresh, scale, T == BF)
        exact(host(got["y"]), want, tag)
        kept = (want != 0).float().mean().item()
        if thresh == 0:
            assert kept == 1.0
        if thresh == 0xFFFFFFFF:
            assert kept <= 1e-3


def drop_settings():
    out = [(0, 1.25), (0xFFFFFFFF, 1.25)]
    for rate in (0.1, 0.5):
        t, s = vit_ref.dropout_params(rate)
        out.append((t, float(np.float32(s))))
    return out


@pytest.mark.parametrize("M,N", rt.DROP_SHAPES, ids=[f"{m}x{n}" for m, n in rt.DROP_SHAPES])
def test_dropout_apply(M, N):
    """y = x * keep * scale, bit for bit (the mask of oracle/vit_ref.py), both output types, dense and pitched,
    thresholds 0 (all kept) and 2^32 - 1 and those of rates 0.1 and 0.5."""
    run_dropout(M, N, f"dropout {M}x{N}", drop_settings(), (0, 8))


def test_dropout_apply_walk():
    M, N = rt.DROP_WALK
    assert M * N // 4 > rt.GRID_ITEMS and (M * N // 4 - rt.GRID_ITEMS) % 256
    run_dropout(M, N, "dropout walk", drop_settings()[2:3], (4,))


# ------------------------------------------------------------------------------------------- head
def head_inputs(fam, B, D, C):
    o = "randn" if fam == "rows" else fam
    p = "int" if fam == "int" else "randn"
    return (rt.family(fam, B, D, "y"), rt.family(o, C, D, "w"), rt.family(o, 1, C, "b")[0], rt.family(fam, B, C, "dl"),
            rt.family(p, C, D, "pw"), rt.family(p, 1, C, "pb")[0])


@pytest.mark.parametrize("D", rt.HEAD_DS)
def test_head(D):
    """head_fwd and head_bwd: D on both sides of a wave and of the 64-column block of the weight gradient, B on
    both sides of its 16 waves, C from 1 to 1000; y dense and pitched (NaN behind each row); bias and db
    present and absent; dw and db accumulate onto a non-zero value."""
    lib = _lib.lib()
    w_ = Worst()
    for C, B, fam in itertools.product(rt.HEAD_CS, rt.HEAD_BS, rt.FAMILIES):
        y, w, b, dl, pw, pb = head_inputs(fam, B, D, C)
        wd, bd, dld = din(w), dvec(b), din(dl)
        for ldy, use_b in itertools.product((D, 3 * D + 5), (True, False)):
            yd = din(y, ldy - D)
            ins = [wd, bd, dld, yd]
            what = f"head D{D} C{C} B{B} {fam} ldy{ldy} bias{int(use_b)}"

            def fwd():
                o = dout(B, C)
                check_rc(lib.vitmi_head_fwd(B, D, C, yd.ptr(), ldy, wd.ptr(), bd.ptr() if use_b else None, o.ptr(), stream()),
                         what)
                return {"logits": o}
            got = twice(fwd, what, None, ins)
            w_.add("logits", rt.worst_ratio(host(got["logits"]), *rt.head_fwd(y, w, b if use_b else None)))

            def bwd():
                o = {"dy": dout(B, D), "dw": dout(C, D, 0, F32, pw)}
                if use_b:
                    o["db"] = dvec_out(C, init=pb)
                check_rc(lib.vitmi_head_bwd(B, D, C, dld.ptr(), yd.ptr(), ldy, wd.ptr(), o["dy"].ptr(), o["dw"].ptr(),
                                            ptr(o.get("db")), stream()), what)
                return o
            got = twice(bwd, f"{what} bwd", None, ins)
            ref = rt.head_bwd(dl, y, w, pw, pb if use_b else None)
            for k, (r, tol) in ref.items():
                g = host(got[k]).view(r.shape)
                w_.add(k, rt.worst_ratio(g, r, tol))
                if fam == "int" and k in ("dw", "db"):
                    assert torch.equal(g.double(), r), (what, k, "integers: not the exact sum")
    w_.report(f"head D{D}")


# ------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("kind", ("ce", "mse"))
def test_loss(kind):
    """loss_fwd_bwd: B on both sides of the block's 256 threads and of two rows per thread, C from 1 to 1000; the
    loss alone, the gradient alone, both (bitwise the same values); the four boundary wrappers bitwise equal to
    the joint call; CE with a label of -1 and a label of C (no class: row loss lse, gradient softmax / B)."""
    lib = _lib.lib()
    code = CE if kind == "ce" else MSE
    w = Worst()
    for B, C, fam in itertools.product(rt.LOSS_BS, rt.LOSS_CS, ("rows", "spike")):
        for outside in ((False, True) if kind == "ce" else (False,)):
            z, t = rt.loss_inputs(kind, fam, B, C)
            if outside:
                t = t.clone()
                t[0], t[-1] = -1, C
            zd = din(z)
            td = t.to(DEV) if kind == "ce" else din(t)
            tp = td.data_ptr() if kind == "ce" else td.ptr()
            what = f"loss {kind} B{B} C{C} {fam}" + (" outside" if outside else "")
            ref = (rt.ce if kind == "ce" else rt.mse)(z, t)
            runs = {}
            for outs in (("loss",), ("dl",), ("loss", "dl")):
                def run():
                    o = {}
                    if "loss" in outs:
                        o["loss"] = dvec_out(1)
                    if "dl" in outs:
                        o["dl"] = dout(B, C)
                    check_rc(lib.vitmi_loss_fwd_bwd(code, B, C, zd.ptr(), tp, ptr(o.get("loss")), ptr(o.get("dl")), stream()),
                             what)
                    return o
                runs[outs] = twice(run, f"{what} {outs}", None, [zd] if kind == "ce" else [zd, td])
            both = runs["loss", "dl"]
            assert same_bits(runs["loss",]["loss"], both["loss"]) and same_bits(runs["dl",]["dl"], both["dl"]), what
            w.add("loss", rt.worst_ratio(host(both["loss"])[0], *ref["loss"]))
            w.add("dl", rt.worst_ratio(host(both["dl"]), *ref["dl"]))
            # the boundary wrappers
            f_fwd, f_bwd = (lib.vitmi_xent_fwd, lib.vitmi_xent_bwd) if kind == "ce" else (lib.vitmi_mse_fwd, lib.vitmi_mse_bwd)
            lo, dl = dvec_out(1), dout(B, C)
            check_rc(f_fwd(B, C, zd.ptr(), tp, lo.ptr(), stream()), f"{what} _fwd")
            check_rc(f_bwd(B, C, zd.ptr(), tp, dl.ptr(), stream()), f"{what} _bwd")
            sync(what)
            assert same_bits(lo, both["loss"]) and same_bits(dl, both["dl"]), (what, "wrapper differs from the joint call")
    w.report(f"loss {kind}")


# ------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize("M,N,K", rt.DENSE_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in rt.DENSE_SHAPES])
def test_dense_f32(M, N, K):
    """dense_f32_fwd / _bwd: linear and ReLU, every operand pitched (NaN behind each row), b, db and dx each
    present and absent, dw and db from a non-zero value.  The backward is handed the device's own y."""
    lib = _lib.lib()
    w_ = Worst()
    for fam, act in itertools.product(rt.FAMILIES, (0, 1)):
        o_ = "randn" if fam == "rows" else fam
        p_ = "int" if fam == "int" else "randn"
        x, w, b = rt.family(fam, M, K, "x"), rt.family(o_, N, K, "w"), rt.family(o_, 1, N, "b")[0]
        dy, pw, pb = rt.family(fam, M, N, "dy"), rt.family(p_, N, K, "pw"), rt.family(p_, 1, N, "pb")[0]
        xd, wd, bd, dyd = din(x, 3), din(w), dvec(b), din(dy, 7)
        for use_b in (True, False):
            what = f"dense {M}x{N}x{K} {fam} act{act} bias{int(use_b)}"

            def fwd():
                o = dout(M, N, 5)
                check_rc(lib.vitmi_dense_f32_fwd(M, N, K, xd.ptr(), xd.pitch, wd.ptr(), bd.ptr() if use_b else None, o.ptr(),
                                                 o.pitch, act, stream()), what)
                return {"y": o}
            got = twice(fwd, what, None, [xd, wd, bd])
            yv = host(got["y"])
            w_.add("y", rt.worst_ratio(yv, *rt.dense_fwd(x, w, b if use_b else None, act)))
            yd = din(yv, 5)
            for use_db, use_dx in itertools.product((True, False), (True, False)):
                tag = f"{what} bwd db{int(use_db)} dx{int(use_dx)}"

                def bwd():
                    o = {"dw": dout(N, K, 0, F32, pw)}
                    if use_db:
                        o["db"] = dvec_out(N, init=pb)
                    if use_dx:
                        o["dx"] = dout(M, K, 2)
                    d = o.get("dx")
                    check_rc(lib.vitmi_dense_f32_bwd(M, N, K, dyd.ptr(), dyd.pitch, yd.ptr(), yd.pitch, xd.ptr(), xd.pitch,
                                                     wd.ptr(), ptr(d), d.pitch if d else 0, o["dw"].ptr(), ptr(o.get("db")),
                                                     act, stream()), tag)
                    return o
                got2 = twice(bwd, tag, None, [xd, wd, dyd, yd])
                ref = rt.dense_bwd(dy, yv, x, w, pw, pb if use_db else None, act)
                for k in got2:
                    r, tol = ref[k]
                    w_.add(k, rt.worst_ratio(host(got2[k]).view(r.shape), r, tol))
    w_.report(f"dense {M}x{N}x{K}")


# ------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing():
    """Calls that the host refuses before any launch (tests/test_abi_tokens.py makes the same ones without a
    device): VITMI_ERR_INVALID, a message that names the argument, nothing recorded, every buffer unchanged."""
    lib = _lib.lib()
    B, C, S, P, D = 2, 3, 32, 8, 128
    np_ = (S // P) ** 2
    img = din(torch.randn(B * C * S, S))
    patches = dout(B * np_, C * P * P)                  # fp32: the widest reading of any dtype code
    wgt, x = din(torch.randn(D, C * P * P)), dout(B * (np_ + 1), D)
    tok, cls, pos = din(torch.randn(B * np_, D)), dvec(torch.randn(D)), din(torch.randn(np_ + 1, D))
    dtok, dtok_lp = dout(B * np_, D), dout(B * np_, D, 0, BF)
    dcls, dpos = dvec_out(D, init=torch.ones(D)), dout(np_ + 1, D, 0, F32, torch.ones(np_ + 1, D))
    ws = dvec_out(lib.vitmi_patch_embed_fwd_workspace_size(T_F32, B, C, S, P, D) // 4 + 64)
    bufs = [img, patches, wgt, x, tok, cls, pos, dtok, dtok_lp, dcls, dpos, ws]
    s = stream()

    def im2col(dtype=T_BF16, B_=B, C_=C, img_=img.ptr(), out=patches.ptr()):
        return (dtype, B_, C_, S, P, img_, out, s)
    for what, a, needle in [("dtype 7", im2col(dtype=7), "dtype"), ("dtype 3", im2col(dtype=3), "dtype"),
                            ("B = -1", im2col(B_=-1), "B >= 0"), ("C = 0", im2col(C_=0), "C > 0"),
                            ("img + 4 bytes", im2col(img_=img.ptr() + 4), "aligned"),
                            ("bf16 patches + 2 bytes", im2col(out=patches.ptr() + 2), "aligned"),
                            ("f32 patches + 8 bytes", im2col(dtype=T_F32, out=patches.ptr() + 8), "aligned")]:
        refused(lib.vitmi_patch_im2col, a, needle, bufs, f"im2col {what}")
    for dtype in (3, 7):
        refused(lib.vitmi_patch_embed_fwd, (dtype, B, C, S, P, D, img.ptr(), wgt.ptr(), None, cls.ptr(), pos.ptr(), patches.ptr(),
                                            x.ptr(), ws.ptr(), ws.cols * 4, s), "dtype", bufs, f"patch_embed_fwd dtype {dtype}")

    def asm(B_=B, tok_=tok.ptr(), x_=x.ptr()):
        return (B_, np_, D, tok_, cls.ptr(), pos.ptr(), x_, s)
    for what, a, needle in [("B = -1", asm(B_=-1), "B >= 0"), ("tok + 4 bytes", asm(tok_=tok.ptr() + 4), "aligned"),
                            ("x + 8 bytes", asm(x_=x.ptr() + 8), "aligned")]:
        refused(lib.vitmi_tokens_assemble, a, needle, bufs, f"tokens_assemble {what}")

    def asb(B_=B, dx_=x.ptr(), dtok_=dtok.ptr(), lp_=dtok_lp.ptr()):
        return (B_, np_, D, dx_, dtok_, lp_, dcls.ptr(), dpos.ptr(), s)
    for what, a, needle in [("B = -1", asb(B_=-1), "B >= 0"), ("dx + 4 bytes", asb(dx_=x.ptr() + 4), "aligned"),
                            ("dtok + 8 bytes", asb(dtok_=dtok.ptr() + 8), "aligned"),
                            ("dtok_lp + 2 bytes", asb(lp_=dtok_lp.ptr() + 2), "aligned")]:
        refused(lib.vitmi_tokens_assemble_bwd, a, needle, bufs, f"tokens_assemble_bwd {what}")
    # head: y = tok [B np, D], w = pos rows, logits / dl in dtok, dy in x, dw in dpos, db in dcls
    HB, HC = 4, 3
    refused(lib.vitmi_head_fwd, (HB, D, HC, tok.ptr(), D - 1, pos.ptr(), cls.ptr(), dtok.ptr(), s), "ldy >= D", bufs,
            "head_fwd ldy < D")
    refused(lib.vitmi_head_bwd, (HB, D, HC, dtok.ptr(), tok.ptr(), D - 1, pos.ptr(), x.ptr(), dpos.ptr(), dcls.ptr(), s),
            "ldy >= D", bufs, "head_bwd ldy < D")
    refused(lib.vitmi_head_bwd, (0, D, HC, dtok.ptr(), tok.ptr(), D, pos.ptr(), x.ptr(), dpos.ptr(), dcls.ptr(), s), "B > 0", bufs,
            "head_bwd B = 0")
    refused(lib.vitmi_cast_f32_bf16, (-8, tok.ptr(), dtok_lp.ptr(), s), "n must be >= 0", bufs, "cast n = -8")
    refused(lib.vitmi_cast_bf16_f32, (-8, dtok_lp.ptr(), dtok.ptr(), s), "n must be >= 0", bufs, "cast_up n = -8")
    for M, N in ((-1, D), (4, -4)):
        refused(lib.vitmi_dropout_apply, (M, N, tok.ptr(), D, dtok.ptr(), T_F32, D, 1, 2, 3, 1.0, s), "negative size", bufs,
                f"dropout_apply M {M} N {N}")
    # zero sizes are served without a launch and without a write
    for fn, a in ((lib.vitmi_patch_im2col, im2col(B_=0)), (lib.vitmi_tokens_assemble, asm(B_=0)),
                  (lib.vitmi_tokens_assemble_bwd, asb(B_=0)), (lib.vitmi_cast_f32_bf16, (0, tok.ptr(), dtok_lp.ptr(), s)),
                  (lib.vitmi_dropout_apply, (0, D, tok.ptr(), D, dtok.ptr(), T_F32, D, 1, 2, 3, 1.0, s))):
        refused(fn, a, "", bufs, "zero size", rc_want=0)
