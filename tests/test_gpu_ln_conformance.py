"""LayerNorm and column-sum conformance on the MI355X: every kernel of csrc/layernorm.hip and the
bias-gradient / fold kernels of csrc/elementwise.hip against the float64 reference and the derived
PER-ELEMENT bound of tests/ref_layernorm.py.

The library is called directly (vitmi._lib.lib()), so every buffer is the test's own guarded allocation:
inputs between NaN guard rows (and NaN guard columns: every pitch is above the logical width and differs
per buffer), outputs between fixed-bit guards.  The backward is fed the reference's mean / rstd rounded
to fp32: it is judged alone.  A HIP error ends the session (check_rc / sync of the attention suite).

Every matrix case asserts
  1. |got - ref| <= tol for EVERY element of y, mean, rstd, dx, dx_lp, dgamma, dbeta, dxsum (the worst
     ratio per output is printed), plus what each family pins exactly (ref_layernorm: ``const``, ``int``),
  2. the guards around every output and the workspace are bitwise intact, no valid output is NaN,
  3. a second run is bitwise equal,
  4. which kernel ran (vitmi_stats_*), and how many fold launches.

Matrix: D at both sides of every 256 boundary (every NV arm) x the M that are no multiple of the small
kernels' 16 / 8 rows per wave; the grid-stride walk of the backward (M past 4 x 512 rows, 8 x, 16 x);
``rows`` everywhere and every family at D = 64, 128, 192, 1028; forward outputs f32, bf16 and every split
form D allows; backward dy {f32, bf16} x dres {none, given} x dx_lp {none, bf16}.  Then every D from 4 to
2048, the bias gradient, the deferred fold queue and the refusals."""
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_gemm as rg  # noqa: E402
import ref_layernorm as rl  # noqa: E402
from kstats import kernel_stats  # noqa: E402
from test_gpu_attn_conformance import check_rc, same_bits, stream, sync  # noqa: E402
from vitmi import _lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
T_F32, T_BF16, T_X3, T_F8, T_F8W = 0, 1, 3, 4, 5          # include/vitmi.h
YNAME = {T_F32: "f32", T_BF16: "bf16", T_X3: "x3", T_F8: "f8", T_F8W: "f8w"}
VITMI_ERR_INVALID = 1
EPS = rl.f32_eps()

DS = (4, 8, 64, 128, 132, 192, 252, 256, 260, 512, 768, 1020, 1024, 1028, 1280, 2044, 2048)
MS = (1, 3, 4, 5, 15, 16, 17, 63, 65)
WALK = ((192, 2053), (768, 2049), (2048, 2051), (128, 4096 + 9), (64, 8192 + 17))
FAMILY_DS = (64, 128, 192, 1028)
OFFSET_DS = (64, 128, 192, 260, 768, 1020, 2048)          # L = 16, 32 and NV = 1, 2, 3, 4, 8
BWD_ALL = tuple((bf, dres, lp) for bf in (False, True) for dres in (False, True) for lp in (False, True))
BWD_WALK = ((False, True, True), (False, False, False), (True, True, False), (True, False, True))
SWEEP_M = 5


def cdiv(a, b):
    return -(-a // b)


def _cases():
    out = []
    for D in DS:
        for M in MS:
            for family in (rl.FAMILIES if D in FAMILY_DS else ("rows",)):
                out.append((D, M, family))
    return out


CASES = _cases()
WALK_CASES = [(D, M, f) for D, M in WALK for f in (("rows", "int") if D in FAMILY_DS else ("rows",))]


# ---------------------------------------------------------------- which kernel, as documented
def y_types(D):
    return [T_F32, T_BF16, T_X3] + ([T_F8] if D % 64 == 0 else []) + ([T_F8W] if D % 128 == 0 else [])


def y_width(D, ydt):
    return {T_F32: D, T_BF16: D, T_X3: 3 * D, T_F8: 2 * D, T_F8W: D + D // 2}[ydt]


def nv_of(D):
    nv = cdiv(D, 256)
    return nv if nv <= 4 else 8


def fwd_kernel(D, ydt):
    """The recorded name (mangled, or demangled) of the forward kernel that serves (D, y type): the small
    kernel at D = 64 / 128 for f32 and bf16, else ln_fwd_kernel<NV, type>."""
    small = D in (64, 128) and ydt in (T_F32, T_BF16)
    base, a = ("ln_fwd_small_kernel", D // 4) if small else ("ln_fwd_kernel", nv_of(D))
    m = {T_F32: "f", T_BF16: "DF16b", T_X3: "NS_7SplitX3E", T_F8: "NS_7SplitF8E", T_F8W: "NS_8SplitF8WE"}[ydt]
    d = {T_F32: "float", T_BF16: "__bf16", T_X3: "vitmi::SplitX3", T_F8: "vitmi::SplitF8", T_F8W: "vitmi::SplitF8W"}[ydt]
    return (f"{base}ILi{a}E{m}EE", f"{base}<{a}, {d}>")


def bwd_kernel(D, bf, lp):
    base, a = ("ln_bwd_small_kernel", D // 4) if D in (64, 128) else ("ln_bwd_kernel", nv_of(D))
    return (f"{base}ILi{a}E{'DF16b' if bf else 'f'}Lb{int(lp)}EE",
            f"{base}<{a}, {'__bf16' if bf else 'float'}, {'true' if lp else 'false'}>")


def colsum_kernel(vec, bf):
    base = "colsum8_kernel" if vec else "colsum_kernel"
    return (f"{base}I{'DF16b' if bf else 'f'}E", f"{base}<{'__bf16' if bf else 'float'}>")


def assert_launches(st, forms, folds, what):
    """Exactly one launch of the kernel named and ``folds`` launches of fold_kernel, nothing else."""
    got = dict(st.k)
    assert got.pop(next((n for n in got if "fold_kernel" in n), None), 0) == folds, (what, "fold launches", st.k)
    if forms is None:
        assert not got, (what, st.k)
        return
    hits = [n for n in got if any(f in n for f in forms)]
    assert len(hits) == 1 and got.pop(hits[0]) == 1 and not got, (what, forms, st.k)


# ---------------------------------------------------------------- device buffers
def up4(n):
    return cdiv(n, 4) * 4


def dev_in(values, pad, dtype=F32, offset=0):
    """A [rows, cols] input of pitch cols + pad whose guard rows and guard columns are NaN."""
    r, c = values.shape
    return rg.padded(r, c, c + pad, dtype, "nan", offset).set(values).to(DEV)


def dev_vec_in(v):
    return rg.padded(1, v.numel(), up4(v.numel()) + 4, F32, "nan").set(v.view(1, -1)).to(DEV)


def dev_out(rows, cols, pad, dtype=F32, offset=0):
    return rg.padded(rows, cols, cols + pad, dtype, "guard", offset).to(DEV)


def dev_vec_out(n, init=None):
    p = rg.padded(1, n, up4(n) + 4, F32, "guard")
    if init is not None:
        p.set(init.view(1, -1))
    return p.to(DEV)


def dev_ws(nbytes):
    n = cdiv(nbytes, 4)
    return rg.padded(1, n, up4(n) + 4, F32, "guard").to(DEV), nbytes


def ptr(p):
    return None if p is None else p.ptr()


def host(p):
    return p.view.cpu()


# ---------------------------------------------------------------- reference (CPU, cached)
@lru_cache(maxsize=4)
def problem(family, M, D):
    inp = rl.inputs(family, M, D)
    return inp, rl.forward(inp["x"], inp["gamma"], inp["beta"], EPS)


@lru_cache(maxsize=8)
def bwd_ref(family, M, D, bf, dres):
    """The backward reference for dy as stored (rounded to bf16 for the bf16 calls)."""
    inp, fwd = problem(family, M, D)
    dy = inp["dy"].to(BF).float() if bf else inp["dy"]
    return rl.backward(inp["x"], fwd["mean_in"], fwd["rstd_in"], inp["gamma"], dy,
                       inp["dres"] if dres else None, inp["prev"])


class Inputs:
    """The device inputs of one (family, M, D): every pitch differs; ``offset`` elements before each base."""

    def __init__(self, family, M, D, offset=0):
        inp, fwd = problem(family, M, D)
        self.family, self.M, self.D, self.offset, self.inp, self.fwd = family, M, D, offset, inp, fwd
        self.x = dev_in(inp["x"], 4, offset=offset)
        self.gamma, self.beta = dev_vec_in(inp["gamma"]), dev_vec_in(inp["beta"])
        self.dy = {False: dev_in(inp["dy"], 12, offset=offset), True: dev_in(inp["dy"], 28, BF, offset=offset)}
        self.dres = dev_in(inp["dres"], 16, offset=offset)
        self.mean, self.rstd = dev_vec_in(fwd["mean_in"]), dev_vec_in(fwd["rstd_in"])

    def all(self):
        return [self.x, self.gamma, self.beta, self.dy[False], self.dy[True], self.dres, self.mean, self.rstd]

    def assert_intact(self, what):
        for p in self.all():
            assert rg.guards_intact(p), (what, "guards of an input changed")


# ---------------------------------------------------------------- calls
def call_fwd(x: Inputs, ydt):
    M, D = x.M, x.D
    y = dev_out(M, y_width(D, ydt), 8, F32 if ydt == T_F32 else BF, x.offset)
    out = {"y": y, "mean": dev_vec_out(M), "rstd": dev_vec_out(M)}
    check_rc(_lib.lib().vitmi_layernorm_fwd(M, D, x.x.ptr(), x.x.pitch, x.gamma.ptr(), x.beta.ptr(), EPS, y.ptr(), ydt,
                                            y.pitch, out["mean"].ptr(), out["rstd"].ptr(), stream()), "layernorm_fwd")
    return out


def call_bwd(x: Inputs, bf, dres, lp, outs=("dgamma", "dbeta", "dxsum")):
    lib = _lib.lib()
    M, D = x.M, x.D
    prev = x.inp["prev"]
    o = {"dx": dev_out(M, D, 20, F32, x.offset)}
    if lp:
        o["dx_lp"] = dev_out(M, D, 24, BF, x.offset)
    for i, k in enumerate(("dgamma", "dbeta", "dxsum")):
        if k in outs:
            o[k] = dev_vec_out(D, prev[i])
    need = lib.vitmi_layernorm_bwd_workspace_size(M, D)
    assert need == 3 * min(max(cdiv(M, 4), 1), 512) * D * 4, need
    o["ws"], nws = dev_ws(need)
    dy, dr, dl = x.dy[bf], x.dres if dres else None, o.get("dx_lp")
    check_rc(lib.vitmi_layernorm_bwd(M, D, dy.ptr(), T_BF16 if bf else T_F32, dy.pitch, x.x.ptr(), x.x.pitch, x.mean.ptr(),
                                     x.rstd.ptr(), x.gamma.ptr(), ptr(dr), dr.pitch if dr else 0, o["dx"].ptr(), o["dx"].pitch,
                                     ptr(dl), dl.pitch if dl else 0, ptr(o.get("dgamma")), ptr(o.get("dbeta")),
                                     ptr(o.get("dxsum")), o["ws"].ptr(), nws, stream()), "layernorm_bwd")
    return o


def twice(fn, forms, folds, what, reps=2, ycols=None):
    """fn() ``reps`` times (the first under kernel_stats); assertions 2-4; returns the first run's buffers.
    ycols: the columns of y that hold bf16 values (the e4m3 bytes behind them are no bf16 numbers)."""
    with kernel_stats() as st:
        a = fn()
    b = fn() if reps > 1 else None
    sync(what)
    assert_launches(st, forms, folds, what)
    for k, p in a.items():
        assert rg.guards_intact(p), (what, f"guards of {k} changed")
        if k != "ws":
            vals = host(p)[:, :ycols] if k == "y" and ycols else host(p)
            assert not torch.isnan(vals.float()).any(), (what, k, "NaN in a valid output")
            assert b is None or same_bits(p, b[k]), (what, k, "second run differs")
    return a


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ---------------------------------------------------------------- judging
def judge_fwd(x: Inputs, outs, what):
    """{output: worst ratio} of the forward outputs {y type: buffers}; the bitwise relations between the
    types and what the ``const`` family pins."""
    D, fwd, w = x.D, x.fwd, {}
    y32 = host(outs[T_F32]["y"])
    same_template = D not in (64, 128)
    for ydt, o in outs.items():
        tag, y = YNAME[ydt], host(o["y"])
        for k in ("mean", "rstd"):
            got = host(o[k])[0]
            w[k] = max(w.get(k, 0.0), rl.worst_ratio(got, *fwd[k]))
            if same_template or ydt in (T_X3, T_F8, T_F8W):      # one template: one mean / rstd
                first = T_F32 if same_template else T_X3
                assert torch.equal(bits(got), bits(host(outs[first][k])[0])), (what, tag, k, "differs between y types")
        hi = y[:, :D]
        if ydt == T_F32:
            w["f32.y"] = rl.worst_ratio(y, *fwd["y"])
        else:
            w[f"{tag}.hi" if ydt != T_BF16 else "bf16.y"] = rl.worst_ratio(hi, *fwd["y_bf16"])
        if ydt == T_X3:
            assert torch.equal(bits(y[:, D:2 * D]), bits(hi)), (what, "x3: the second hi copy differs")
            w["x3.hi+lo"] = rl.worst_ratio(hi.double() + y[:, 2 * D:].double(), *fwd["hi+lo"])
            if same_template:
                assert torch.equal(bits(y), bits(rl.split_x3(y32))), (what, "x3 is not the split of the fp32 y")
        if ydt in (T_F8, T_F8W):
            h, hi8, lo8 = rl.f8_unpack(y, D, wform=ydt == T_F8W)
            assert torch.equal(hi8, rl.split_f8(h.float())[1]), (what, tag, "hi8 is not e4m3(hi)")
            if lo8 is not None:
                w["f8.hi+lo8"] = rl.worst_ratio(h.double() + rl.e4m3_value(lo8) / 512.0, *fwd["hi+lo8"])
            if same_template:
                ch, ch8, cl8 = rl.split_f8(y32)
                assert torch.equal(bits(h), bits(ch)) and torch.equal(hi8, ch8), (what, tag, "not the split of the fp32 y")
                assert lo8 is None or torch.equal(lo8, cl8), (what, tag, "lo8 is not the split of the fp32 y")
        if x.family == "const":
            rows = rl.const_rows(x.M)
            beta = x.inp["beta"] if ydt == T_F32 else x.inp["beta"].to(BF)
            assert torch.equal(bits(hi[rows]), bits(beta.expand(len(rows), D))), (what, tag, "constant row: y != beta")
            assert (host(o["mean"])[0][rows] == rl.CONST_VALUE).all(), (what, tag, "constant row: mean != c")
    return w


def judge_bwd(x: Inputs, o, bf, dres, what, w):
    ref = bwd_ref(x.family, x.M, x.D, bf, dres)
    t = "bf16" if bf else "f32"
    for k in ("dx", "dx_lp", "dgamma", "dbeta", "dxsum"):
        if k not in o:
            continue
        got = host(o[k]) if k in ("dx", "dx_lp") else host(o[k])[0]
        key = f"{t}.{k}"
        w[key] = max(w.get(key, 0.0), rl.worst_ratio(got, *ref[k]))
        if k == "dbeta" and x.family == "int":
            assert torch.equal(got.double(), ref[k][0]), (what, "integer dy: dbeta is not the exact sum")


def run_case(D, M, family, offset=0, reps=2, ytypes=None, combos=BWD_ALL, variants=True):
    """The forward in every y type and the backward in every combination, judged; {output: worst ratio}."""
    what = f"D{D} M{M} {family}" + (f" +{offset}" if offset else "")
    x = Inputs(family, M, D, offset)
    outs = {ydt: twice(lambda ydt=ydt: call_fwd(x, ydt), fwd_kernel(D, ydt), 0, f"{what} fwd {YNAME[ydt]}", reps,
                       ycols=D if ydt in (T_F8, T_F8W) else None)
            for ydt in (ytypes or y_types(D))}
    w = judge_fwd(x, outs, what)
    full = {}
    for bf, dres, lp in combos:
        tag = f"{what} bwd {'bf16' if bf else 'f32'} dres{int(dres)} lp{int(lp)}"
        o = twice(lambda: call_bwd(x, bf, dres, lp), bwd_kernel(D, bf, lp), 3, tag, reps)
        judge_bwd(x, o, bf, dres, tag, w)
        full[bf, dres, lp] = o
    if variants:    # without the three reductions, and with dxsum alone: the same dx, bit for bit
        for bf, dres, lp in combos[:1] + combos[-1:]:
            for outs_, folds in (((), 0), (("dxsum",), 1)):
                tag = f"{what} bwd {'bf16' if bf else 'f32'} dres{int(dres)} lp{int(lp)} outs {outs_}"
                o = twice(lambda: call_bwd(x, bf, dres, lp, outs_), bwd_kernel(D, bf, lp), folds, tag, 1)
                judge_bwd(x, o, bf, dres, tag, w)
                for k in ("dx", "dx_lp")[:1 + lp]:
                    assert same_bits(o[k], full[bf, dres, lp][k]), (tag, k, "differs from the call with the reductions")
    x.assert_intact(what)
    return what, w


def report(what, w):
    print(f"CONF ln {what}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    for name, v in w.items():
        assert v <= 1.0, (what, name, v)


@pytest.mark.parametrize("D,M,family", CASES, ids=[f"D{D}-M{M}-{f}" for D, M, f in CASES])
def test_layernorm_matrix(D, M, family):
    report(*run_case(D, M, family))


@pytest.mark.parametrize("D,M,family", WALK_CASES, ids=[f"D{D}-M{M}-{f}" for D, M, f in WALK_CASES])
def test_layernorm_backward_walk(D, M, family):
    """More rows than one trip of the backward's grid-stride loop covers (512 blocks x 4 waves x 1, 2 or 4
    rows): the second trip, its tail, and the 512 partial rows per reduction that the fold then sums.
    Every TDY x LP instantiation, dres given and not; ``int`` pins every row's count exactly."""
    assert cdiv(M, 4 * (64 // (D // 4) if D in (64, 128) else 1)) > 512
    report(*run_case(D, M, family, combos=BWD_WALK, variants=False))


@pytest.mark.parametrize("D", OFFSET_DS)
def test_layernorm_base_offset(D):
    """x, y, dy, dres, dx and dx_lp start 4 elements into their allocations: 16-byte (bf16: 8-byte) aligned
    and not row aligned, once per kernel template."""
    report(*run_case(D, 5, "rows", offset=4))


def test_case_list_reaches_every_kernel():
    """The tables themselves (no launch): every NV arm and both small kernels, every y type on each, every
    TDY x LP instantiation; rows per wave that do not divide M; a walk case per backward template family."""
    fwd = {fwd_kernel(D, t)[0] for D, _, _ in CASES for t in y_types(D)}
    bwd = {bwd_kernel(D, bf, lp)[0] for D, _, _ in CASES for bf, _, lp in BWD_ALL}
    for a in (1, 2, 3, 4, 8):
        assert {fwd_kernel(a * 256 if a < 8 else 2048, t)[0] for t in YNAME} <= fwd, a
        assert {bwd_kernel(a * 256 if a < 8 else 2048, bf, lp)[0] for bf in (0, 1) for lp in (0, 1)} <= bwd, a
    for D in (64, 128):
        assert {fwd_kernel(D, t)[0] for t in YNAME} <= fwd
        assert {bwd_kernel(D, bf, lp)[0] for bf in (0, 1) for lp in (0, 1)} <= bwd
        assert {bwd_kernel(D, bf, lp)[0] for D_, _ in WALK if D_ == D for bf, _, lp in BWD_WALK} \
            == {bwd_kernel(D, bf, lp)[0] for bf in (0, 1) for lp in (0, 1)}
    assert any(M % 16 for M in MS) and any(M % 8 for M in MS) and {1, 15, 16, 17} <= set(MS)
    assert {D for D, _, f in CASES if f == "const"} == set(FAMILY_DS)
    assert len(fwd) == 5 * 5 + 4 and len(bwd) == 7 * 4


# ---------------------------------------------------------------- every D
def sweep_blocks():
    return [(lo, lo + 252) for lo in range(4, 2049, 256)]


@pytest.mark.parametrize("lo,hi", sweep_blocks(), ids=[f"D{lo}-{hi}" for lo, hi in sweep_blocks()])
def test_layernorm_every_d(lo, hi):
    """Every D of the block at M = 5: the forward (f32) and the backward (f32 dy, dres given) by the bound,
    with the guards and the kernel that ran.  Every failing (D, output) is reported, not the first."""
    failures, block = [], {}
    for D in range(lo, hi + 1, 4):
        try:
            _, w = run_case(D, SWEEP_M, "rows", reps=1, ytypes=(T_F32,), combos=((False, True, False),), variants=False)
        except AssertionError as e:
            failures.append((D, str(e)[:300]))
            continue
        for k, v in w.items():
            block[k] = max(block.get(k, 0.0), v)
            if not v <= 1.0:
                failures.append((D, k, round(v, 3)))
    print(f"CONF ln sweep D{lo}-{hi}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in sorted(block.items())))
    assert not failures, failures


# ---------------------------------------------------------------- bias gradient
BIAS_SHAPES = ((1, 8), (33, 8), (33, 64), (100, 72), (31, 520), (32, 512), (33, 7), (65, 130), (8193, 64), (4100, 7),
               (1000, 2304))


def bias_pitch(N, form):
    """'vec': a pitch above N that keeps the vector kernel; 'odd': one that is no multiple of 8; 'shift': the
    vector pitch behind a base one element into the allocation (not 16-byte aligned)."""
    if form == "odd":
        return N + 3 if (N + 3) % 8 else N + 5
    return cdiv(N, 8) * 8 + 8


def call_bias(dy, prev, M, N, bf):
    lib = _lib.lib()
    need = lib.vitmi_bias_grad_workspace_size(M, N)
    o = {"db": dev_vec_out(N, prev)}
    o["ws"], nws = dev_ws(need)
    check_rc(lib.vitmi_bias_grad(T_BF16 if bf else T_F32, M, N, dy.ptr(), dy.pitch, o["db"].ptr(), o["ws"].ptr(), nws,
                                 stream()), "bias_grad")
    return o


@pytest.mark.parametrize("bf", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("M,N", BIAS_SHAPES, ids=[f"M{M}-N{N}" for M, N in BIAS_SHAPES])
def test_bias_grad(M, N, bf):
    """db += colsum(dy) from a non-zero db: ``int`` equals the exact sum BITWISE, ``randn`` is within the
    bound; guards (the input's guard columns are NaN: a column read past N shows), a bitwise second run,
    and which kernel ran: colsum8_kernel iff N % 8 == 0, the pitch % 8 == 0 and the base is 16-byte aligned."""
    worst = {}
    for family in ("int", "randn"):
        vals, prev = rl.colsum_inputs(family, M, N)
        ref, tol = rl.colsum(vals, prev)
        for form in ("vec", "odd", "shift"):
            what = f"bias M{M} N{N} {'bf16' if bf else 'f32'} {family} {form}"
            dy = rg.padded(M, N, bias_pitch(N, form), BF if bf else F32, "nan", offset=int(form == "shift")).set(vals).to(DEV)
            vec = form == "vec" and N % 8 == 0
            o = twice(lambda: call_bias(dy, prev, M, N, bf), colsum_kernel(vec, bf), 1, what)
            got = host(o["db"])[0]
            assert rg.guards_intact(dy), (what, "guards of the input changed")
            if family == "int":
                assert torch.equal(got.double(), ref), (what, "not the exact sum", (got.double() - ref).abs().max())
            key = f"{'colsum8' if vec else 'colsum'}.{'bf16' if bf else 'f32'}"
            worst[key] = max(worst.get(key, 0.0), rl.worst_ratio(got, ref, tol))
    print(f"CONF bias M{M} N{N}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, (M, N, k, v)


# ---------------------------------------------------------------- the deferred fold queue
def test_fold_queue_matches_immediate_folds():
    """Between vitmi_fold_begin and vitmi_fold_end: six LayerNorm backwards of different D (18 fold jobs) and
    two bias gradients.  The first two backwards share one dgamma, so the second's fold may not ride the
    first's launch (the overlap flush); the 17th job finds the queue full (FOLD_MAX = 16); vitmi_fold_end
    launches the rest: three fold launches.  Every result is bitwise what the same calls give one by one."""
    lib = _lib.lib()
    M = 67
    xs = [Inputs("rows", M, D) for D in (768, 768, 64, 128, 260, 1028)]
    bias = [(100, 72, True), (65, 130, False)]
    bias_in = []
    for m, n, bf in bias:
        vals, prev = rl.colsum_inputs("randn", m, n)
        bias_in.append((rg.padded(m, n, bias_pitch(n, "vec"), BF if bf else F32, "nan").set(vals).to(DEV), prev))

    def run(deferred):
        held = []
        shared = dev_vec_out(768, xs[0].inp["prev"][0])
        if deferred:
            assert lib.vitmi_fold_begin() == 0
        try:
            with kernel_stats() as st:
                for i, x in enumerate(xs):
                    M_, D = x.M, x.D
                    bf, lp = bool(i % 2), i % 3 == 0
                    o = {"dx": dev_out(M_, D, 20), "dbeta": dev_vec_out(D, x.inp["prev"][1]),
                         "dxsum": dev_vec_out(D, x.inp["prev"][2])}
                    o["dgamma"] = shared if i < 2 else dev_vec_out(D, x.inp["prev"][0])
                    if lp:
                        o["dx_lp"] = dev_out(M_, D, 24, BF)
                    o["ws"], nws = dev_ws(lib.vitmi_layernorm_bwd_workspace_size(M_, D))
                    dy, dl = x.dy[bf], o.get("dx_lp")
                    check_rc(lib.vitmi_layernorm_bwd(M_, D, dy.ptr(), T_BF16 if bf else T_F32, dy.pitch, x.x.ptr(), x.x.pitch,
                                                     x.mean.ptr(), x.rstd.ptr(), x.gamma.ptr(), x.dres.ptr(), x.dres.pitch,
                                                     o["dx"].ptr(), o["dx"].pitch, ptr(dl), dl.pitch if dl else 0,
                                                     o["dgamma"].ptr(), o["dbeta"].ptr(), o["dxsum"].ptr(), o["ws"].ptr(), nws,
                                                     stream()), f"fold queue bwd {i}")
                    held.append(o)
                for (m, n, bf), (dy, prev) in zip(bias, bias_in):
                    held.append(call_bias(dy, prev, m, n, bf))
                if deferred:
                    check_rc(lib.vitmi_fold_end(stream()), "fold_end")
        finally:
            if deferred:
                lib.vitmi_fold_end(stream())       # leaves the thread's queue switched off whatever happened
        sync("fold queue")
        return held, st

    one, st1 = run(False)
    two, st2 = run(True)
    assert st1.calls("fold_kernel") == 6 * 3 + 2 and st2.calls("fold_kernel") == 3, (st1.k, st2.k)
    for i, (a, b) in enumerate(zip(one, two)):
        for k in a:
            assert rg.guards_intact(b[k]), (i, k, "guards changed")
            if k != "ws":
                assert same_bits(a[k], b[k]), (i, k, "the queued fold differs from the immediate one")
    # and the shared dgamma holds both backwards' sums (D = 768, the two dy types)
    x = xs[0]
    ref = bwd_ref("rows", M, 768, False, True)["dgamma"]
    ref2 = bwd_ref("rows", M, 768, True, True)["dgamma"]
    prev = x.inp["prev"][0].double()
    got = host(two[0]["dgamma"])[0]
    assert rl.worst_ratio(got, ref[0] + ref2[0] - prev, ref[1] + ref2[1]) <= 1.0


# ---------------------------------------------------------------- refusals
class Snapshot:
    """Device buffers with the bytes they held before a call."""

    def __init__(self, bufs):
        self.bufs = [(p, p.buf.cpu().clone()) for p in bufs]

    def assert_unchanged(self, what):
        for i, (p, before) in enumerate(self.bufs):
            assert torch.equal(p.buf.cpu().view(torch.uint8), before.view(torch.uint8)), (what, i, "written to")


def refused(fn, args, needle, bufs, what, rc_want=VITMI_ERR_INVALID):
    lib = _lib.lib()
    snap = Snapshot(bufs)
    with kernel_stats() as st:
        rc = fn(*args)
    sync(what)
    msg = lib.vitmi_last_error().decode(errors="replace") if rc else ""
    assert rc == rc_want, (what, rc, msg)
    assert needle in msg, (what, msg)
    assert not st.k, (what, "launched", st.k)
    snap.assert_unchanged(what)


def test_layernorm_fwd_refusals():
    """Every precondition of vitmi_layernorm_fwd (include/vitmi.h): VITMI_ERR_INVALID with a message that names
    it, nothing launched, nothing written.  Every buffer is large enough for the call had it been served."""
    lib = _lib.lib()
    M, DA = 5, 2052                                   # allocations wide enough for every D tried
    x = dev_in(torch.randn(M, DA), 12)
    g, b = dev_vec_in(torch.ones(DA)), dev_vec_in(torch.zeros(DA))
    y = dev_out(M, 3 * DA, 16, F32)                   # fp32 units: twice any bf16 row form
    mean, rstd = dev_vec_out(M), dev_vec_out(M)
    bufs = [x, g, b, y, mean, rstd]

    def args(D=192, ydt=T_F32, **o):
        a = dict(M=M, D=D, x=x.ptr(), ldx=x.pitch, g=g.ptr(), b=b.ptr(), eps=EPS, y=y.ptr(), ydt=ydt, ldy=y.pitch,
                 mean=mean.ptr(), rstd=rstd.ptr(), s=stream())
        a.update(o)
        return tuple(a.values())

    cases = [
        ("D % 4", args(D=190), "multiple of 4 in [4, 2048]"),
        ("D = 2052", args(D=2052), "multiple of 4 in [4, 2048]"),
        ("D = 0", args(D=0), "multiple of 4 in [4, 2048]"),
        ("ldx % 4", args(ldx=x.pitch - 2), "strides must be multiples of 4"),
        ("ldy % 4", args(ldy=y.pitch - 2), "strides must be multiples of 4"),
        ("ldx < D", args(ldx=188), "ldx >= D"),
        ("ldy < D", args(ldy=188), "ldy >= D"),
        ("ldy < 3D", args(ydt=T_X3, ldy=3 * 192 - 4), "3D for VITMI_BF16X3"),
        ("ldy < 2D", args(ydt=T_F8, ldy=2 * 192 - 4), "2D for VITMI_BF16F8"),
        ("ldy < 1.5D", args(D=256, ydt=T_F8W, ldy=384 - 4), "1.5D for"),
        ("f8 D = 96", args(D=96, ydt=T_F8), "VITMI_BF16F8 needs D % 64 == 0"),
        ("f8w D = 192", args(D=192, ydt=T_F8W), "VITMI_BF16F8W needs D % 128 == 0"),
        ("y dtype 2", args(ydt=2), "y dtype must be"),
        ("y dtype 7", args(ydt=7), "y dtype must be"),
        ("x + 4 bytes", args(x=x.ptr() + 4), "aligned"),
        ("x + 8 bytes", args(x=x.ptr() + 8), "aligned"),
        ("y f32 + 8 bytes", args(y=y.ptr() + 8), "aligned"),
        ("y bf16 + 4 bytes", args(ydt=T_BF16, y=y.ptr() + 4), "aligned"),
        ("y x3 + 2 bytes", args(ydt=T_X3, y=y.ptr() + 2), "aligned"),
        ("gamma + 4 bytes", args(g=g.ptr() + 4), "aligned"),
    ]
    cases += [(f"null {k}", args(**{k: None}), "null pointer") for k in ("x", "g", "b", "y", "mean", "rstd")]
    for what, a, needle in cases:
        refused(lib.vitmi_layernorm_fwd, a, needle, bufs, f"fwd {what}")
    refused(lib.vitmi_layernorm_fwd, args(M=0), "", bufs, "fwd M = 0", rc_want=0)
    # a bf16 y on an 8-byte boundary that is no 16-byte one is served
    with kernel_stats() as st:
        check_rc(lib.vitmi_layernorm_fwd(*args(ydt=T_BF16, y=y.ptr() + 8)), "fwd bf16 y + 8 bytes")
    sync("fwd bf16 y + 8 bytes")
    assert_launches(st, fwd_kernel(192, T_BF16), 0, "fwd bf16 y + 8 bytes")
    assert all(rg.guards_intact(p) for p in bufs)     # its rows lie inside y's (wider, fp32) window


def test_layernorm_bwd_refusals():
    """Every precondition of vitmi_layernorm_bwd: each stride first no multiple of 4, then below D; the split
    dtypes for dy; a workspace one byte short; every vector base off its alignment."""
    lib = _lib.lib()
    M, D = 5, 192
    f = lambda pad: dev_in(torch.randn(M, D), pad)  # noqa: E731
    dy, x, dres = f(12), f(8), f(16)                   # dy as fp32: the widest reading of any dtype code
    g, mean, rstd = dev_vec_in(torch.ones(D)), dev_vec_in(torch.zeros(M)), dev_vec_in(torch.ones(M))
    dx, dx_lp = dev_out(M, D, 20), dev_out(M, D, 24, BF)
    acc = [dev_vec_out(D, torch.zeros(D)) for _ in range(3)]
    ws, nws = dev_ws(lib.vitmi_layernorm_bwd_workspace_size(M, D))
    bufs = [dy, x, dres, g, mean, rstd, dx, dx_lp, ws] + acc

    def args(**o):
        a = dict(M=M, D=D, dy=dy.ptr(), dt=T_F32, lddy=dy.pitch, x=x.ptr(), ldx=x.pitch, mean=mean.ptr(), rstd=rstd.ptr(),
                 g=g.ptr(), dres=dres.ptr(), ldres=dres.pitch, dx=dx.ptr(), lddx=dx.pitch, dx_lp=dx_lp.ptr(),
                 lddx_lp=dx_lp.pitch, dgamma=acc[0].ptr(), dbeta=acc[1].ptr(), dxsum=acc[2].ptr(), ws=ws.ptr(), nws=nws,
                 s=stream())
        a.update(o)
        return tuple(a.values())

    cases = [("D % 4", args(D=190), "multiple of 4 in [4, 2048]"), ("D = 2052", args(D=2052), "multiple of 4 in [4, 2048]")]
    for k in ("lddy", "ldx", "lddx", "ldres", "lddx_lp"):
        cases.append((f"{k} % 4", args(**{k: D + 6}), "strides must be multiples of 4"))
        cases.append((f"{k} < D", args(**{k: D - 4}), ">= D required"))
    cases += [
        ("dy dtype x3", args(dt=T_X3), "dy dtype must be"),
        ("dy dtype f8", args(dt=T_F8), "dy dtype must be"),
        ("dy dtype 2", args(dt=2), "dy dtype must be"),
        ("workspace one byte short", args(nws=nws - 1), "workspace too small"),
        ("null workspace", args(ws=None), "workspace too small"),
        ("dy f32 + 8 bytes", args(dy=dy.ptr() + 8), "aligned"),
        ("dy bf16 + 4 bytes", args(dt=T_BF16, dy=dy.ptr() + 4), "aligned"),
        ("x + 4 bytes", args(x=x.ptr() + 4), "aligned"),
        ("dres + 8 bytes", args(dres=dres.ptr() + 8), "aligned"),
        ("dx + 4 bytes", args(dx=dx.ptr() + 4), "aligned"),
        ("dx_lp + 4 bytes", args(dx_lp=dx_lp.ptr() + 4), "aligned"),
        ("dx_lp + 2 bytes", args(dx_lp=dx_lp.ptr() + 2), "aligned"),
    ]
    cases += [(f"null {k}", args(**{k: None}), "null pointer") for k in ("dy", "x", "mean", "rstd", "g", "dx")]
    for what, a, needle in cases:
        refused(lib.vitmi_layernorm_bwd, a, needle, bufs, f"bwd {what}")
    refused(lib.vitmi_layernorm_bwd, args(M=0), "", bufs, "bwd M = 0", rc_want=0)
    # strides of outputs that are not asked for are not looked at
    with kernel_stats() as st:
        check_rc(lib.vitmi_layernorm_bwd(*args(dres=None, ldres=0, dx_lp=None, lddx_lp=1)), "bwd without dres, dx_lp")
    sync("bwd without dres, dx_lp")
    assert_launches(st, bwd_kernel(D, False, False), 3, "bwd without dres, dx_lp")
    assert all(rg.guards_intact(p) for p in bufs)


def test_bias_grad_refusals():
    """vitmi_bias_grad: a dtype that is neither fp32 nor bf16, ldy < N, a workspace one byte short, a base
    off its element's alignment; M = 0 leaves db untouched.  (A base that is element aligned and not 16-byte
    aligned is served by the one-column-per-thread kernel: test_bias_grad's 'shift' form.)"""
    lib = _lib.lib()
    M, N = 33, 64
    dy = dev_in(torch.randn(M, N), 8)                  # fp32: the widest reading of any dtype code
    db = dev_vec_out(N, torch.ones(N))
    ws, nws = dev_ws(lib.vitmi_bias_grad_workspace_size(M, N))
    bufs = [dy, db, ws]

    def args(**o):
        a = dict(dt=T_F32, M=M, N=N, dy=dy.ptr(), ldy=dy.pitch, db=db.ptr(), ws=ws.ptr(), nws=nws, s=stream())
        a.update(o)
        return tuple(a.values())

    for what, a, needle in [
        ("dtype x3", args(dt=T_X3), "dtype must be"),
        ("dtype f8w", args(dt=T_F8W), "dtype must be"),
        ("ldy < N", args(ldy=N - 8), "ldy >= N"),
        ("workspace one byte short", args(nws=nws - 1), "workspace too small"),
        ("dy f32 + 2 bytes", args(dy=dy.ptr() + 2), "aligned"),
        ("dy bf16 + 1 byte", args(dt=T_BF16, dy=dy.ptr() + 1), "aligned"),
        ("null dy", args(dy=None), "null pointer"),
        ("null db", args(db=None), "null pointer"),
    ]:
        refused(lib.vitmi_bias_grad, a, needle, bufs, f"bias {what}")
    refused(lib.vitmi_bias_grad, args(M=0), "", bufs, "bias M = 0", rc_want=0)
    assert torch.equal(host(db)[0], torch.ones(N))
