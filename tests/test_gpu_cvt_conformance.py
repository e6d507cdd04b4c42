"""CvT convolution conformance on the MI355X: every kernel of csrc/cvt.hip (im2col / col2im, depthwise 3x3 +
BatchNorm forward and backward, 3x3 average pooling forward and backward) against the float64 reference and
the derived PER-ELEMENT bound of tests/ref_cvt.py.

The library is called directly (vitmi._lib.lib()), so every buffer is the test's own guarded allocation:
inputs between NaN guard rows with NaN guard columns, outputs and the workspace between fixed-bit guards,
every pitch above C and different per buffer.  x, y and dy use different image strides and offsets
(x_off = 1, y_off = 2, dy_off = 0), so the rows an entry point must skip (cls rows, the gaps between images,
the rows after the last image) hold NaN in an input and guard bits in an output.  The backward is fed the
reference's z / mean / rstd rounded to fp32: it is judged alone.  A HIP error ends the session.

Every case asserts
  1. |got - ref| <= tol for EVERY element of every output (the worst ratio per output is printed), plus what
     each family pins exactly (ref_cvt: ``ramp``, ``int``),
  2. every guard and every skipped row bitwise intact, no valid output NaN,
  3. a second run bitwise equal,
  4. inference (training = 0) leaves run_mean / run_var bitwise untouched and returns mean == run_mean bitwise.

Matrix (ref_cvt's lists, the ones tests/test_cvt_ref_cpu.py judges on the CPU): C x (H, W) x B with ``chan``
everywhere and every family at C = 4, 64, 256, 1024; the row walks of the *_rows kernels; the grid caps; every
(H, W) of 1..9 x 1..9; the conv geometries; the refusals."""
import ctypes
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_cvt as rc  # noqa: E402
import ref_gemm as rg  # noqa: E402
from test_gpu_attn_conformance import check_rc, same_bits, stream, sync  # noqa: E402
from vitmi import _lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
T_F32, T_BF16 = 0, 1                                  # include/vitmi.h
VITMI_ERR_INVALID = 1
EPS, MOM = rc.f32(rc.EPS), rc.f32(rc.MOMENTUM)
TAIL = 2                                              # rows after the last image, inside the window


def layout(hw):
    """{buffer: (image stride, offset, pitch - C)}: all different."""
    return {"x": (hw + 3, 1, 4), "y": (hw + 4, 2, 8), "dy": (hw + 1, 0, 12)}


# ---------------------------------------------------------------- device buffers
def image_rows(B, hw, img, off):
    return (torch.arange(B).view(B, 1) * img + off + torch.arange(hw).view(1, -1)).reshape(-1)


class Rows:
    """Token rows [B img + TAIL, C] (pitch C + pad) in a guarded allocation; the images' rows hold ``values``
    (logical [B, H, W, C]) when given, every other row of the window keeps the fill (NaN for an input, the
    guard bits for an output)."""

    def __init__(self, B, hw, C, img, off, pad, dtype, fill, values=None, offset=0):
        self.B, self.hw, self.C, self.img, self.off = B, hw, C, img, off
        p = rg.padded(B * img + TAIL, C, C + pad, dtype, fill, offset)
        self.idx = image_rows(B, hw, img, off)
        if values is not None:
            p.view[self.idx] = values.reshape(B * hw, C).to(dtype)
        self.p = p.to(DEV)
        self.pitch = p.pitch

    def ptr(self):
        return self.p.ptr()

    def logical(self, shape):
        return self.p.view.cpu()[self.idx].reshape(shape)

    def intact(self):
        """The guards of the allocation and the rows of the window outside the images."""
        if not rg.guards_intact(self.p):
            return False
        ints = self.p.view.cpu().contiguous().view(rg._INT[self.p.dtype]).clone()
        ints[self.idx] = self.p._signed()
        return bool((ints == self.p._signed()).all())


def up4(n):
    return rc.cdiv(n, 4) * 4


def vec_in(v):
    return rg.padded(1, v.numel(), up4(v.numel()) + 4, F32, "nan").set(v.reshape(1, -1)).to(DEV)


def vec_out(n, init=None):
    p = rg.padded(1, n, up4(n) + 4, F32, "guard")
    if init is not None:
        p.set(init.reshape(1, -1))
    return p.to(DEV)


def host(p):
    return p.view.cpu()


def ptr(p):
    return None if p is None else p.ptr()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ---------------------------------------------------------------- reference (CPU, cached)
@lru_cache(maxsize=2)
def problem(family, B, H, W, C):
    inp = rc.dw_inputs(family, B, H, W, C)
    fwd = rc.dwconv_bn_forward(inp["x"], inp["w9"], inp["gamma"], inp["beta"], EPS, MOM, inp["run_mean"], inp["run_var"],
                               chain=rc.chain_rows(B, H, W, C))
    return inp, fwd


def bwd_ref(family, B, H, W, C, bf, prev):
    inp, fwd = problem(family, B, H, W, C)
    dy = inp["dy"].to(BF).float() if bf else inp["dy"]
    pv = inp["prev"] if prev else {k: torch.zeros_like(v) for k, v in inp["prev"].items()}
    return rc.dwconv_bn_backward(dy, inp["x"], inp["w9"], inp["gamma"], fwd["z_in"], fwd["mean_in"], fwd["rstd_in"], pv,
                                 rc.chain_pixels(B, H, W, C), rc.chain_rows(B, H, W, C)), pv


class Inputs:
    def __init__(self, family, B, H, W, C):
        inp, fwd = problem(family, B, H, W, C)
        self.case, self.inp, self.fwd = (family, B, H, W, C), inp, fwd
        hw = H * W
        self.L = layout(hw)
        xi, xo, xp = self.L["x"]
        di, do, dp = self.L["dy"]
        self.x = Rows(B, hw, C, xi, xo, xp, F32, "nan", inp["x"])
        self.dy = {False: Rows(B, hw, C, di, do, dp, F32, "nan", inp["dy"]),
                   True: Rows(B, hw, C, di, do, dp + 8, BF, "nan", inp["dy"])}
        self.w9, self.gamma, self.beta = vec_in(inp["w9"]), vec_in(inp["gamma"]), vec_in(inp["beta"])
        self.z = rg.padded(B * hw, C, C, F32, "nan").set(fwd["z_in"].reshape(B * hw, C)).to(DEV)
        self.mean, self.rstd = vec_in(fwd["mean_in"]), vec_in(fwd["rstd_in"])

    def assert_intact(self, what):
        for r in (self.x, self.dy[False], self.dy[True]):
            assert r.intact(), (what, "an input changed")
        for p in (self.w9, self.gamma, self.beta, self.z, self.mean, self.rstd):
            assert rg.guards_intact(p), (what, "guards of an input changed")


def workspace(B, H, W, C):
    need = _lib.lib().vitmi_dwconv_bn_workspace_size(B, H, W, C)
    assert need == rc.dw_workspace_size(B, H, W, C), "dw_blocks differs from tests/ref_cvt.py's formula"
    return vec_out(need // 4), need


# ---------------------------------------------------------------- calls
def call_fwd(x: Inputs, bf, training=True, stats=True):
    _, B, H, W, C = x.case
    yi, yo, yp = x.L["y"]
    o = {"y": Rows(B, H * W, C, yi, yo, yp, BF if bf else F32, "guard"),
         "z": rg.padded(B * H * W, C, C, F32, "guard").to(DEV), "mean": vec_out(C), "rstd": vec_out(C)}
    if stats:
        o["run_mean"], o["run_var"] = vec_out(C, x.inp["run_mean"]), vec_out(C, x.inp["run_var"])
    o["ws"], nws = workspace(B, H, W, C)
    check_rc(_lib.lib().vitmi_dwconv_bn_fwd(B, H, W, C, x.x.ptr(), x.x.pitch, x.x.img, x.x.off, x.w9.ptr(), x.gamma.ptr(),
                                            x.beta.ptr(), EPS, MOM, int(training), ptr(o.get("run_mean")), ptr(o.get("run_var")),
                                            o["z"].ptr(), o["mean"].ptr(), o["rstd"].ptr(), o["y"].ptr(), T_BF16 if bf else T_F32,
                                            o["y"].pitch, yi, yo, o["ws"].ptr(), nws, stream()), "dwconv_bn_fwd")
    return o


def call_bwd(x: Inputs, bf, pv):
    _, B, H, W, C = x.case
    xi, xo, xp = x.L["x"]
    o = {"dx": Rows(B, H * W, C, xi, xo, xp, F32, "guard", pv["dx"]), "dw9": vec_out(9 * C, pv["dw9"]),
         "dgamma": vec_out(C, pv["dgamma"]), "dbeta": vec_out(C, pv["dbeta"])}
    o["ws"], nws = workspace(B, H, W, C)
    dy = x.dy[bf]
    check_rc(_lib.lib().vitmi_dwconv_bn_bwd(B, H, W, C, dy.ptr(), T_BF16 if bf else T_F32, dy.pitch, dy.img, dy.off, x.x.ptr(),
                                            x.x.pitch, xi, xo, x.w9.ptr(), x.gamma.ptr(), x.z.ptr(), x.mean.ptr(), x.rstd.ptr(),
                                            o["dx"].ptr(), o["dw9"].ptr(), o["dgamma"].ptr(), o["dbeta"].ptr(), o["ws"].ptr(),
                                            nws, stream()), "dwconv_bn_bwd")
    return o


def call_pool_fwd(x: Inputs, bf, cp):
    _, B, H, W, C = x.case
    yi, yo, yp = x.L["y"]
    o = {"y": Rows(B, H * W, C, yi, yo, yp, BF if bf else F32, "guard")}
    check_rc(_lib.lib().vitmi_avgpool3_fwd(B, H, W, C, x.x.ptr(), x.x.pitch, x.x.img, x.x.off, o["y"].ptr(),
                                           T_BF16 if bf else T_F32, o["y"].pitch, yi, yo, cp, stream()), "avgpool3_fwd")
    return o


def call_pool_bwd(x: Inputs, bf, cp, prev):
    _, B, H, W, C = x.case
    xi, xo, xp = x.L["x"]
    o = {"dx": Rows(B, H * W, C, xi, xo, xp, F32, "guard", prev)}
    dy = x.dy[bf]
    check_rc(_lib.lib().vitmi_avgpool3_bwd(B, H, W, C, dy.ptr(), T_BF16 if bf else T_F32, dy.pitch, dy.img, dy.off,
                                           o["dx"].ptr(), o["dx"].pitch, xi, xo, cp, stream()), "avgpool3_bwd")
    return o


def intact(p):
    return p.intact() if isinstance(p, Rows) else rg.guards_intact(p)


def twice(fn, what, reps=2):
    """fn() twice; assertions 2 and 3; returns the first run's buffers."""
    a = fn()
    b = fn() if reps > 1 else None
    sync(what)
    for k, p in a.items():
        assert intact(p), (what, f"guards of {k} changed")
        if k != "ws":
            q = p.p if isinstance(p, Rows) else p
            assert b is None or same_bits(q, b[k].p if isinstance(p, Rows) else b[k]), (what, k, "second run differs")
    return a


def ratio(w, key, got, ref, tol, what):
    assert not torch.isnan(got.float()).any(), (what, key, "NaN in a valid output")
    w[key] = max(w.get(key, 0.0), rc.worst_ratio(got, ref, tol))


# ---------------------------------------------------------------- one case
def run_case(family, B, H, W, C, light=False):
    what = f"{family} B{B} H{H} W{W} C{C}"
    x = Inputs(family, B, H, W, C)
    inp, fwd = x.inp, x.fwd
    shape = (B, H, W, C)
    w = {}
    reps = 1 if light else 2
    # forward: fp32 y with the moving statistics, bf16 y without them
    first = None
    for bf, stats in ((False, True),) if light else ((False, True), (True, False)):
        tag = f"{what} fwd {'bf16' if bf else 'f32'}"
        o = twice(lambda: call_fwd(x, bf, True, stats), tag, reps)
        t = "bf16." if bf else ""
        z = host(o["z"]).reshape(shape)
        ratio(w, "z", z, *fwd["z"], tag)
        if family == "ramp":
            assert torch.equal(z.double(), fwd["z"][0]), (tag, "ramp: z is not exact")
            if fwd["chain_exact"]:
                assert torch.equal(host(o["mean"])[0], fwd["mean_exact"]), (tag, "ramp: mean is not the exact mean")
        for k in ("mean", "rstd") + (("run_mean", "run_var") if stats else ()):
            ratio(w, k, host(o[k])[0], *fwd[k], tag)
        ratio(w, t + "y", o["y"].logical(shape), *fwd["y_bf16" if bf else "y"], tag)
        if first is None:
            first = o
        else:
            for k in ("z", "mean", "rstd"):
                assert same_bits(o[k], first[k]), (tag, k, "differs between the y types")
    # inference: the moving statistics normalise and stay as they were
    if not light:
        tag = f"{what} inference"
        inf = rc.dwconv_bn_forward(inp["x"], inp["w9"], inp["gamma"], inp["beta"], EPS, MOM, inp["run_mean"], inp["run_var"],
                                   training=False)
        o = twice(lambda: call_fwd(x, False, False, True), tag)
        assert torch.equal(bits(host(o["run_mean"])[0]), bits(inp["run_mean"])), (tag, "run_mean changed")
        assert torch.equal(bits(host(o["run_var"])[0]), bits(inp["run_var"])), (tag, "run_var changed")
        assert torch.equal(bits(host(o["mean"])[0]), bits(inp["run_mean"])), (tag, "mean != run_mean")
        ratio(w, "inf.rstd", host(o["rstd"])[0], *inf["rstd"], tag)
        ratio(w, "inf.y", o["y"].logical(shape), *inf["y"], tag)
    # backward: fp32 dy onto non-zero accumulators, bf16 dy onto zeros
    for bf, prev in ((False, True),) if light else ((False, True), (True, False)):
        tag = f"{what} bwd {'bf16' if bf else 'f32'}"
        ref, pv = bwd_ref(family, B, H, W, C, bf, prev)
        o = twice(lambda: call_bwd(x, bf, pv), tag, reps)
        t = "bf16." if bf else ""
        ratio(w, t + "dx", o["dx"].logical(shape), *ref["dx"], tag)
        ratio(w, t + "dw9", host(o["dw9"])[0].reshape(9, C), *ref["dw9"], tag)
        for k in ("dgamma", "dbeta"):
            ratio(w, t + k, host(o[k])[0], *ref[k], tag)
        if family == "int":
            assert torch.equal(host(o["dbeta"])[0].double(), ref["dbeta"][0]), (tag, "int: dbeta is not the exact sum")
    # pooling
    for bf, cp in ((False, 0),) if light else ((False, 0), (True, 0), (False, 1), (True, 1)):
        tag = f"{what} pool {'bf16' if bf else 'f32'} count_pad {cp}"
        f = rc.avgpool_fwd(inp["x"], cp)
        o = twice(lambda: call_pool_fwd(x, bf, cp), tag, reps)
        y = o["y"].logical(shape)
        ratio(w, f"pool.{'bf16.' if bf else ''}y", y, *f["y_bf16" if bf else "y"], tag)
        if family == "int" and not bf:
            assert torch.equal(y, rc.avgpool_int_pin(inp["x"], cp)), (tag, "int: y is not fl(S fl(1 / t))")
        prev = torch.zeros(shape) if bf else inp["prev"]["dx"]
        dyv = inp["dy"].to(BF).float() if bf else inp["dy"]
        o = twice(lambda: call_pool_bwd(x, bf, cp, prev), tag + " bwd", reps)
        ratio(w, f"pool.{'bf16.' if bf else ''}dx", o["dx"].logical(shape), *rc.avgpool_bwd(dyv, prev, cp), tag)
    x.assert_intact(what)
    return w


def merge(into, w):
    for k, v in w.items():
        into[k] = max(into.get(k, 0.0), v)


def report(what, w):
    print(f"CONF cvt {what}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
    for name, v in w.items():
        assert v <= 1.0, (what, name, v)


def run_cases(what, cases, light=False):
    total, failures = {}, []
    for case in cases:
        try:
            w = run_case(*case, light=light)
        except AssertionError as e:
            failures.append((case, str(e)[:300]))
            continue
        merge(total, w)
        failures += [(case, k, round(v, 3)) for k, v in w.items() if not v <= 1.0]
    print(f"CONF cvt {what} ({len(cases)} cases): worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in total.items()))
    assert not failures, failures


MATRIX = [(C, f) for C in rc.DW_CHANNELS for f in (rc.FAMILIES if C in rc.FAMILY_CS else ("chan",))]


@pytest.mark.parametrize("C,family", MATRIX, ids=[f"C{C}-{f}" for C, f in MATRIX])
def test_dw_pool_matrix(C, family):
    """Every (H, W) x B of the list at this C and family (36 shapes; ``offset`` at all of them, n <= 240)."""
    cases = [c for c in rc.dw_matrix(C) if c[0] == family]
    assert len(cases) == len(rc.HW) * len(rc.BS)
    run_cases(f"C{C} {family}", cases)


WALK_CASES = [(f, B, H, W, C, least) for B, H, W, C, least in rc.WALKS for f in rc.FAMILIES]


@pytest.mark.parametrize("family,B,H,W,C,least", WALK_CASES, ids=[f"{c[0]}-{'x'.join(map(str, c[1:5]))}" for c in WALK_CASES])
def test_row_walks(family, B, H, W, C, least):
    """W < 8 and more image rows than one trip of the *_rows kernels covers: every thread walks ``least`` rows
    or more (recomputed from the host formulas, which ``workspace`` holds against the library)."""
    G, lanes, per = rc.rows_grid(B, H, W, C)
    assert W < 8 and rc.cdiv(B * H * (C // 4), 256) > rc.dw_blocks(B * H * W, C) and per >= least, (G, lanes, per)
    assert rc.offset_ok(B * H * W)
    report(f"walk {family} {B}x{H}x{W}x{C}", run_case(family, B, H, W, C))


@pytest.mark.parametrize("B,H,W,C", rc.CAPS, ids=["x".join(map(str, c)) for c in rc.CAPS])
def test_grid_caps(B, H, W, C):
    """Past the 4096 x 256 work items of the flat kernels and of dw_bwd_dx_rows_kernel with a remainder (the
    first shape), past dw_blocks' 1024 blocks (the second): ``randn``, fp32, one run and its repeat."""
    cap = rc.CVT_BLOCKS * 256
    assert B * H * W * (C // 4) > cap
    assert B * H * (C // 4) > cap or rc.cdiv(B * H * W, 8 * (256 // (C // 4))) > 1024
    x = run_case("randn", B, H, W, C, light=True)
    report(f"caps {B}x{H}x{W}x{C}", x)


@pytest.mark.parametrize("H", range(1, 10))
def test_every_hw(H):
    """Every W of 1..9 at this H, C = 64, B = 2, ``chan``."""
    run_cases(f"sweep H{H}", [("chan", 2, H, W, 64) for W in range(1, 10)])


# ---------------------------------------------------------------- conv
CONV = rc.conv_cases()
IMG_GAP, ROW_OFF = 2, 1
TRIGGERS = ("plain", "ldx", "base")        # a pitch that is no multiple of 4; a base 4 bytes off a 16-byte boundary


def conv_x(g, inp, trigger="plain"):
    pad = {"plain": 4, "ldx": 3, "base": 4}[trigger]
    return Rows(g.B, g.H * g.W, g.C, g.H * g.W + IMG_GAP, ROW_OFF, pad, F32, "nan", inp["x"], offset=int(trigger == "base"))


def call_im2col(g, Kp, x, bf):
    o = {"p": rg.padded(g.B * g.Ho * g.Wo, Kp, Kp, BF if bf else F32, "guard").to(DEV)}
    check_rc(_lib.lib().vitmi_conv_im2col(T_BF16 if bf else T_F32, g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, g.pt, g.pl, g.Ho, g.Wo,
                                          x.ptr(), x.pitch, x.img, x.off, o["p"].ptr(), Kp, stream()), "conv_im2col")
    return o


def call_col2im(g, Kp, dp, bf, prev):
    hw = g.H * g.W
    o = {"dx": Rows(g.B, hw, g.C, hw + IMG_GAP, ROW_OFF, 8, F32, "guard", prev)}
    check_rc(_lib.lib().vitmi_conv_col2im(T_BF16 if bf else T_F32, g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, g.pt, g.pl, g.Ho, g.Wo,
                                          dp.ptr(), Kp, o["dx"].ptr(), o["dx"].pitch, hw + IMG_GAP, ROW_OFF,
                                          int(prev is not None), stream()), "conv_col2im")
    return o


def run_conv(name, g, Kp, families=("randn", "int"), triggers=("plain",)):
    w = {}
    shape = (g.B, g.H, g.W, g.C)
    for family in families:
        inp = rc.conv_inputs(family, g, Kp)
        ref = rc.im2col(inp["x"], g, Kp)
        for trigger in triggers:
            x = conv_x(g, inp, trigger)
            for bf in (False, True):
                tag = f"{name} {family} im2col {trigger} {'bf16' if bf else 'f32'}"
                got = host(twice(lambda: call_im2col(g, Kp, x, bf), tag)["p"])
                want = ref.float().to(BF) if bf else ref.float()
                assert torch.equal(bits(got), bits(want)), (tag, "not bitwise the (rounded) value, or a padding column not +0")
            assert x.intact(), (name, trigger, "x changed")
        if g.C % 4:
            continue
        for bf in (False, True):
            dpv = inp["dp"].to(BF).float() if bf else inp["dp"]
            dp = rg.padded(g.B * g.Ho * g.Wo, Kp, Kp, BF if bf else F32, "nan").set(inp["dp"]).to(DEV)
            for acc in (False, True):
                tag = f"{name} {family} col2im {'bf16' if bf else 'f32'} accumulate {int(acc)}"
                prev = inp["prev"] if acc else None
                r, tol, t = rc.col2im(dpv, g, prev)
                got = twice(lambda: call_col2im(g, Kp, dp, bf, prev), tag)["dx"].logical(shape)
                ratio(w, f"col2im{'.bf16' if bf else ''}{'.acc' if acc else ''}", got, r, tol, tag)
                unread = (t == 0).view(1, g.H, g.W, 1).expand(shape)
                want = prev if acc else torch.zeros(shape)
                assert torch.equal(bits(got[unread]), bits(want[unread])), (tag, "a pixel no window reads")
                if family == "int":
                    assert torch.equal(got.double(), r), (tag, "int: not the exact sum")
            assert rg.guards_intact(dp), (name, "dpatches changed")
    return w


@pytest.mark.parametrize("name,g,Kp", CONV, ids=[c[0] for c in CONV])
def test_conv_im2col_col2im(name, g, Kp):
    """im2col BITWISE (fp32, and bf16 = round to nearest even; +0 in columns K..Kp-1 and outside the image),
    col2im within its bound (f32 and bf16 dpatches, with and without accumulate, NaN in dpatches' padding
    columns), a pixel no window reads exactly +0 / prev, ``int`` the exact sum."""
    assert rc.geo_ok(g) and Kp >= g.kh * g.kw * g.C
    report(f"conv {name}", run_conv(name, g, Kp))


@pytest.mark.parametrize("name", ("k3s1", "k4s4"))
def test_conv_im2col_scalar_triggers(name):
    """The one-element im2col through a pitch that is no multiple of 4 and through a base 4 bytes off a 16-byte
    boundary (C % 4 and Kp % 4 are cases of the list): the same patches, bit for bit."""
    _, g, Kp = next(c for c in CONV if c[0] == name)
    run_conv(name, g, Kp, families=("randn",), triggers=TRIGGERS)


@pytest.mark.parametrize("name,g,Kp", rc.CONV_CAPS, ids=[c[0] for c in rc.CONV_CAPS])
def test_conv_grid_caps(name, g, Kp):
    assert max(g.B * g.Ho * g.Wo * Kp // 4, g.B * g.H * g.W * g.C // 4) > rc.CVT_BLOCKS * 256
    report(f"conv {name}", run_conv(name, g, Kp, families=("randn",)))


def test_conv_same_geometry_closed_form():
    """vitmi_conv_same_geometry against the closed form over H x k x s = 1..40 x 1..7 x 1..4 (host only), the
    two axes independently."""
    lib = _lib.lib()
    v = [ctypes.c_int(0) for _ in range(4)]
    for H in range(1, 41):
        for k in range(1, 8):
            for s in range(1, 5):
                W, kw = 41 - H, 8 - k
                assert lib.vitmi_conv_same_geometry(H, W, k, kw, s, *[ctypes.addressof(t) for t in v]) == 0
                assert (v[0].value, v[2].value) == rc.same_pad(H, k, s) and (v[1].value, v[3].value) == rc.same_pad(W, kw, s)
    assert lib.vitmi_conv_same_geometry(0, 4, 3, 3, 1, None, None, None, None) == VITMI_ERR_INVALID
    assert lib.vitmi_conv_same_geometry(4, 4, 3, 3, 0, None, None, None, None) == VITMI_ERR_INVALID


# ---------------------------------------------------------------- refusals
class Snapshot:
    def __init__(self, bufs):
        self.bufs = [(p, p.buf.cpu().clone()) for p in bufs]

    def assert_unchanged(self, what):
        for i, (p, before) in enumerate(self.bufs):
            assert torch.equal(p.buf.cpu().view(torch.uint8), before.view(torch.uint8)), (what, i, "written to")


def refused(fn, cases, bufs):
    """Each (what, args, needle): VITMI_ERR_INVALID with a message that names the precondition, nothing written."""
    lib = _lib.lib()
    snap = Snapshot(bufs)
    for what, args, needle in cases:
        rc_ = fn(*args)
        msg = lib.vitmi_last_error().decode(errors="replace") if rc_ else ""
        assert rc_ == VITMI_ERR_INVALID, (what, rc_, msg)
        assert needle in msg, (what, msg)
    sync("refusals")
    snap.assert_unchanged("refusals")


B0, H0, W0, C0 = 2, 3, 5, 64
HW0 = H0 * W0


def dw_buffers():
    x = Rows(B0, HW0, C0, HW0 + 3, 1, 4, F32, "nan", torch.randn(B0, H0, W0, C0))
    dy = Rows(B0, HW0, C0, HW0 + 1, 0, 12, F32, "nan", torch.randn(B0, H0, W0, C0))
    y = Rows(B0, HW0, C0, HW0 + 4, 2, 8, F32, "guard")
    dx = Rows(B0, HW0, C0, HW0 + 3, 1, 4, F32, "guard", torch.zeros(B0, H0, W0, C0))
    return x, dy, y, dx


def test_dwconv_bn_fwd_refusals():
    lib = _lib.lib()
    x, _, y, _ = dw_buffers()
    w9, g, b = vec_in(torch.randn(9 * C0)), vec_in(torch.ones(C0)), vec_in(torch.zeros(C0))
    z = rg.padded(B0 * HW0, C0, C0, F32, "guard").to(DEV)
    mean, rstd, rm, rv = vec_out(C0), vec_out(C0), vec_out(C0, torch.zeros(C0)), vec_out(C0, torch.ones(C0))
    ws, nws = workspace(B0, H0, W0, C0)

    def args(**o):
        a = dict(B=B0, H=H0, W=W0, C=C0, x=x.ptr(), ldx=x.pitch, x_img=x.img, x_off=x.off, w=w9.ptr(), g=g.ptr(), b=b.ptr(),
                 eps=EPS, mom=MOM, training=1, rm=rm.ptr(), rv=rv.ptr(), z=z.ptr(), mean=mean.ptr(), rstd=rstd.ptr(), y=y.ptr(),
                 ydt=T_F32, ldy=y.pitch, y_img=y.img, y_off=y.off, ws=ws.ptr(), nws=nws, s=stream())
        a.update(o)
        return tuple(a.values())

    cases = [(f"C = {C}", args(C=C), "C must be a multiple of 4 dividing 1024") for C in (0, 2, 12, 48, 96, 2048)]
    cases += [
        ("B = 0", args(B=0), "bad sizes"), ("W = 0", args(W=0), "bad sizes"),
        ("ldx % 4", args(ldx=C0 + 6), "bad row layout"), ("ldx < C", args(ldx=C0 - 4), "bad row layout"),
        ("x_img short", args(x_img=HW0), "bad row layout"), ("x_off < 0", args(x_off=-1), "bad row layout"),
        ("ldy % 4", args(ldy=C0 + 6), "bad output layout"), ("ldy < C", args(ldy=C0 - 4), "bad output layout"),
        ("y_img short", args(y_img=HW0 + 1), "bad output layout"), ("y_off < 0", args(y_off=-1), "bad output layout"),
        ("y dtype 2", args(ydt=2), "bad dtype"), ("y dtype -1", args(ydt=-1), "bad dtype"),
        ("workspace one byte short", args(nws=nws - 1), "workspace"), ("null workspace", args(ws=None), "workspace"),
        ("inference without run_mean", args(training=0, rm=None), "inference needs"),
        ("inference without run_var", args(training=0, rv=None), "inference needs"),
    ]
    cases += [(f"null {k}", args(**{k: None}), "null pointer") for k in ("x", "w", "g", "b", "z", "mean", "rstd", "y")]
    cases += [(f"{k} + 4 bytes", args(**{k: p.ptr() + 4}), "16-byte aligned")
              for k, p in (("x", x), ("w", w9), ("g", g), ("b", b), ("z", z), ("mean", mean), ("rstd", rstd), ("ws", ws))]
    refused(lib.vitmi_dwconv_bn_fwd, cases, [x.p, y.p, w9, g, b, z, mean, rstd, rm, rv, ws])


def test_dwconv_bn_bwd_refusals():
    lib = _lib.lib()
    x, dy, _, dx = dw_buffers()
    w9, g = vec_in(torch.randn(9 * C0)), vec_in(torch.ones(C0))
    z = rg.padded(B0 * HW0, C0, C0, F32, "nan").set(torch.randn(B0 * HW0, C0)).to(DEV)
    mean, rstd = vec_in(torch.zeros(C0)), vec_in(torch.ones(C0))
    dw9, dg, db = vec_out(9 * C0, torch.zeros(9 * C0)), vec_out(C0, torch.zeros(C0)), vec_out(C0, torch.zeros(C0))
    ws, nws = workspace(B0, H0, W0, C0)

    def args(**o):
        a = dict(B=B0, H=H0, W=W0, C=C0, dy=dy.ptr(), dt=T_F32, lddy=dy.pitch, dy_img=dy.img, dy_off=dy.off, x=x.ptr(),
                 ldx=x.pitch, x_img=x.img, x_off=x.off, w=w9.ptr(), g=g.ptr(), z=z.ptr(), mean=mean.ptr(), rstd=rstd.ptr(),
                 dx=dx.ptr(), dw=dw9.ptr(), dg=dg.ptr(), db=db.ptr(), ws=ws.ptr(), nws=nws, s=stream())
        a.update(o)
        return tuple(a.values())

    cases = [(f"C = {C}", args(C=C), "C must be a multiple of 4 dividing 1024") for C in (0, 2, 12, 48, 96, 2048)]
    cases += [
        ("ldx % 4", args(ldx=C0 + 6), "bad row layout"), ("ldx < C", args(ldx=C0 - 4), "bad row layout"),
        ("x_img short", args(x_img=HW0), "bad row layout"), ("x_off < 0", args(x_off=-1), "bad row layout"),
        ("lddy % 4", args(lddy=C0 + 6), "bad dy layout"), ("lddy < C", args(lddy=C0 - 4), "bad dy layout"),
        ("dy_img short", args(dy_img=HW0 - 1), "bad dy layout"), ("dy_off < 0", args(dy_off=-1), "bad dy layout"),
        ("dy dtype 3", args(dt=3), "bad dtype"), ("dy dtype -1", args(dt=-1), "bad dtype"),
        ("workspace one byte short", args(nws=nws - 1), "workspace"), ("null workspace", args(ws=None), "workspace"),
    ]
    cases += [(f"null {k}", args(**{k: None}), "null pointer") for k in ("dy", "x", "w", "g", "z", "mean", "rstd", "dx", "dw")]
    cases += [(f"{k} + 4 bytes", args(**{k: p.ptr() + 4}), "16-byte aligned")
              for k, p in (("x", x), ("w", w9), ("g", g), ("z", z), ("mean", mean), ("rstd", rstd), ("dx", dx), ("ws", ws))]
    refused(lib.vitmi_dwconv_bn_bwd, cases, [x.p, dy.p, dx.p, w9, g, z, mean, rstd, dw9, dg, db, ws])


def test_avgpool3_refusals():
    lib = _lib.lib()
    x, dy, y, dx = dw_buffers()

    def fargs(**o):
        a = dict(B=B0, H=H0, W=W0, C=C0, x=x.ptr(), ldx=x.pitch, x_img=x.img, x_off=x.off, y=y.ptr(), ydt=T_F32, ldy=y.pitch,
                 y_img=y.img, y_off=y.off, cp=0, s=stream())
        a.update(o)
        return tuple(a.values())

    def bargs(**o):
        a = dict(B=B0, H=H0, W=W0, C=C0, dy=dy.ptr(), dt=T_F32, lddy=dy.pitch, dy_img=dy.img, dy_off=dy.off, dx=dx.ptr(),
                 ldx=dx.pitch, x_img=dx.img, x_off=dx.off, cp=0, s=stream())
        a.update(o)
        return tuple(a.values())

    fc = [(f"C = {C}", fargs(C=C), "C must be a multiple of 4 dividing 1024") for C in (0, 2, 12, 48, 96, 2048)]
    fc += [("ldx % 4", fargs(ldx=C0 + 6), "bad row layout"), ("ldx < C", fargs(ldx=C0 - 4), "bad row layout"),
           ("x_img short", fargs(x_img=HW0), "bad row layout"), ("x_off < 0", fargs(x_off=-1), "bad row layout"),
           ("ldy % 4", fargs(ldy=C0 + 6), "bad output layout"), ("ldy < C", fargs(ldy=C0 - 4), "bad output layout"),
           ("y_img short", fargs(y_img=HW0 + 1), "bad output layout"), ("y_off < 0", fargs(y_off=-1), "bad output layout"),
           ("y dtype 2", fargs(ydt=2), "bad dtype"), ("null x", fargs(x=None), "null pointer"),
           ("null y", fargs(y=None), "null pointer"), ("x + 4 bytes", fargs(x=x.ptr() + 4), "16-byte aligned")]
    refused(lib.vitmi_avgpool3_fwd, fc, [x.p, y.p])
    bc = [(f"C = {C}", bargs(C=C), "C must be a multiple of 4 dividing 1024") for C in (0, 2, 12, 48, 96, 2048)]
    bc += [("ldx % 4", bargs(ldx=C0 + 6), "bad row layout"), ("ldx < C", bargs(ldx=C0 - 4), "bad row layout"),
           ("x_img short", bargs(x_img=HW0), "bad row layout"), ("x_off < 0", bargs(x_off=-1), "bad row layout"),
           ("lddy % 4", bargs(lddy=C0 + 6), "bad dy layout"), ("lddy < C", bargs(lddy=C0 - 4), "bad dy layout"),
           ("dy_img short", bargs(dy_img=HW0 - 1), "bad dy layout"), ("dy_off < 0", bargs(dy_off=-1), "bad dy layout"),
           ("dy dtype 2", bargs(dt=2), "bad dtype"), ("null dy", bargs(dy=None), "null pointer"),
           ("null dx", bargs(dx=None), "null pointer"), ("dx + 4 bytes", bargs(dx=dx.ptr() + 4), "16-byte aligned")]
    refused(lib.vitmi_avgpool3_bwd, bc, [dy.p, dx.p])


def test_conv_refusals():
    lib = _lib.lib()
    g = rc.same_geo(2, 5, 7, 4, 3, 3, 2)
    K = 9 * 4
    inp = rc.conv_inputs("randn", g, 64)
    x = conv_x(g, inp)
    pat = rg.padded(g.B * g.Ho * g.Wo, 64, 64, F32, "guard").to(DEV)
    dp = rg.padded(g.B * g.Ho * g.Wo, 64, 64, F32, "nan").set(inp["dp"]).to(DEV)
    dx = Rows(g.B, g.H * g.W, g.C, g.H * g.W + IMG_GAP, ROW_OFF, 8, F32, "guard", inp["prev"])

    def geo(**o):
        a = dict(B=g.B, H=g.H, W=g.W, C=g.C, kh=g.kh, kw=g.kw, s=g.s, pt=g.pt, pl=g.pl, Ho=g.Ho, Wo=g.Wo)
        a.update(o)
        return list(a.values())

    def iargs(dt=T_F32, xp=x.ptr(), ldx=x.pitch, img=x.img, off=x.off, p=pat.ptr(), Kp=64, **o):
        return tuple([dt] + geo(**o) + [xp, ldx, img, off, p, Kp, stream()])

    def cargs(dt=T_F32, d=dp.ptr(), Kp=64, dxp=dx.ptr(), ldx=dx.pitch, img=dx.img, off=dx.off, acc=0, **o):
        return tuple([dt] + geo(**o) + [d, Kp, dxp, ldx, img, off, acc, stream()])

    common = lambda f, kp: [  # noqa: E731
        ("pt >= kh", f(pt=3), "bad padding"), ("pl >= kw", f(pl=3), "bad padding"), ("pt < 0", f(pt=-1), "bad padding"),
        ("Ho = 0", f(Ho=0), "bad padding"), ("window below the input", f(Ho=g.Ho + 2), "outside the input"),
        ("window right of the input", f(Wo=g.Wo + 2), "outside the input"), ("s = 0", f(s=0), "bad sizes"),
        ("C = 0", f(C=0), "bad sizes"), ("Kp < K", f(Kp=K - 4), kp), ("ldx < C", f(ldx=2), "bad row layout"),
        ("img_stride short", f(img=g.H * g.W), "bad row layout"), ("row_off < 0", f(off=-1), "bad row layout")]
    ic = common(iargs, "Kp < kh*kw*C") + [("dtype 2", iargs(dt=2), "bad dtype"), ("null x", iargs(xp=None), "null pointer"),
                          ("null patches", iargs(p=None), "null pointer")]
    refused(lib.vitmi_conv_im2col, ic, [x.p, pat])
    cc = common(cargs, "required") + [("C % 4", cargs(C=3, Kp=64), "C % 4 == 0 required"),
                                      ("ldx % 4", cargs(ldx=dx.pitch + 2), "required"),
                          ("null dpatches", cargs(d=None), "null pointer"), ("null dx", cargs(dxp=None), "null pointer"),
                          ("dx + 4 bytes", cargs(dxp=dx.ptr() + 4), "16-byte aligned")]
    refused(lib.vitmi_conv_col2im, cc, [dp, dx.p])
