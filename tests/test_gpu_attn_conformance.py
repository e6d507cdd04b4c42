"""Attention conformance on the MI355X: every kernel of csrc/attention.hip that an entry point can
reach, against the float64 reference and the derived PER-ELEMENT bound of tests/ref_attention.py.

The library is called directly (vitmi._lib.lib()), so every buffer is the test's own guarded
allocation.  The backward is fed the reference's o (rounded to the storage type) and lse (fp32): it
is judged alone, and one reference per (family, type, B, N, H, scale) serves every kernel policy.

Every matrix case asserts
  1. |got - ref| <= tol for EVERY element of o, lse, dq, dk, dv (the worst ratio per output is printed),
  2. the guard rows before and after o, lse, dqkv, the workspace and dbias are bitwise intact, the
     inputs (qkv, o, dO, lse) sit in allocations whose guard rows are NaN, and no valid output is NaN,
  3. a second run is bitwise equal,
  4. with the bias gradient: the column-sum bound of ref_attention, and dqkv bitwise equal to the call
     without it,
  5. which kernels ran (vitmi_stats_*).

Matrix: policies 0-3 x bf16 and policies 0, 1 x fp32; (B, H) = (2, 3) and (1, 1); the N at the edges of
every host-side decision and of the 32 / 64 / 128-row tiles (385: four 128-row blocks of the streamed
kernels); scale 0.125 and 0.3 (and 0.125 / sqrt 2 once); all four input families at N = 33, 197, 225,
257, ``rows`` elsewhere.  Then the x3 / f8 forwards, every N from 1 to 260, and the persistent walk
of the backward kernels with more (batch, head) pairs than compute units."""
from dataclasses import dataclass
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_attention as ra  # noqa: E402
import ref_gemm as rg  # noqa: E402
from kstats import kernel_stats  # noqa: E402
from test_gpu_attn_dispatch import expected as dispatch_expected, kname  # noqa: E402
from vitmi import _lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
CODE = {F32: 0, BF: 1}
TN = {BF: "bf16", F32: "f32"}
DH = 64
SEQ_MAX = 256
VITMI_ERR_INVALID, VITMI_ERR_HIP = 1, 2
RUNS = ((0, BF), (1, BF), (2, BF), (3, BF), (0, F32), (1, F32))      # (policy, operand type)
SHAPES = ((2, 3), (1, 1))
NS = (1, 31, 32, 33, 64, 65, 192, 193, 197, 224, 225, 256, 257, 300, 385)
SCALES = (0.125, 0.3)
FAMILY_NS = (33, 197, 225, 257)
SWEEP = dict(B=2, H=2, family="rows", scale=0.3, lo=1, hi=260)
OUTPUTS = ("o", "lse", "dq", "dk", "dv")


def cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Case:
    pol: int
    T: torch.dtype
    B: int
    H: int
    N: int
    family: str
    scale: float

    @property
    def id(self):
        return f"p{self.pol}-{TN[self.T]}-B{self.B}H{self.H}-N{self.N}-{self.family}-s{self.scale:.4g}"


def _cases():
    keys = []
    for B, H in SHAPES:
        for N in NS:
            for scale in SCALES:
                for family in (ra.FAMILIES if N in FAMILY_NS else ("rows",)):
                    keys.append((B, H, N, family, scale))
    keys.append((2, 3, 197, "rows", 0.125 / 2 ** 0.5))
    # the runs of one reference next to each other: the reference cache stays small
    return [Case(pol, T, *k) for k in keys for pol, T in RUNS]


CASES = _cases()


# ---------------------------------------------------------------- which kernels, as documented
def expected_kernels(pol, T, N):
    """The name forms (test_gpu_attn_dispatch.kname) of the kernels one forward + one backward record,
    in launch order, from the dispatch test's statement of csrc/attention.hip attn_plan; the last
    form, base<a, b> or the plain name, serves as the label."""
    return list(dispatch_expected(pol, T, N))


def assert_kernels(st, exp, what):
    got = {n: c for n, c in st.k.items() if "attn_" in n}
    for forms in exp:
        hits = [n for n in got if any(f in n for f in forms)]
        assert len(hits) == 1 and got.pop(hits[0]) == 1, (what, forms, st.k)
    assert not got, (what, "not expected", got)


# ---------------------------------------------------------------- reference (CPU, cached)
@lru_cache(maxsize=12)
def problem(family, T, B, N, H, scale):
    qkv, do = ra.inputs(family, B, N, H, T, seed=7)
    return qkv, do, ra.reference(qkv, do, B, N, H, scale, T)


# ---------------------------------------------------------------- device buffers and calls
def stream():
    return torch.cuda.current_stream().cuda_stream


def check_rc(rc, what):
    if rc == VITMI_ERR_HIP:      # a faulted device: nothing more is launched on it
        pytest.exit(f"{what}: HIP error {_lib.lib().vitmi_last_error().decode(errors='replace')}", returncode=3)
    assert rc == 0, (what, rc, _lib.lib().vitmi_last_error().decode(errors="replace"))


def sync(what=""):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:    # as above
        pytest.exit(f"{what}: {e}", returncode=3)


def dev_in(x):
    """An input in an allocation whose guard rows are NaN."""
    return ra.aligned(x.shape[0], x.shape[1], x.dtype, "nan").set(x).to(DEV)


def dev_out(rows, cols, dtype):
    return ra.aligned(rows, cols, dtype, "guard").to(DEV)


def dev_ws(nbytes):
    """A workspace of nbytes (a multiple of 4) on a 256-byte boundary, guard floats around it."""
    n = cdiv(nbytes, 4)
    return rg.padded(1, n, cdiv(n, 64) * 64, F32, "guard").to(DEV), n * 4


def same_bits(a: rg.Padded, b: rg.Padded):
    return torch.equal(a.buf.view(torch.uint8), b.buf.view(torch.uint8))


class Inputs:
    def __init__(self, qkv, do, ref):
        self.qkv, self.do = dev_in(qkv), dev_in(do)
        self.o, self.lse = dev_in(ref["o_in"]), dev_in(ref["lse_in"])

    def assert_intact(self, what):
        for k in ("qkv", "do", "o", "lse"):
            assert rg.guards_intact(getattr(self, k)), (what, f"guard rows of the input {k} changed")


def run_fwd(T, B, N, H, scale, x: Inputs):
    D = H * DH
    o, lse = dev_out(B * N, D, T), dev_out(B * H, N, F32)
    check_rc(_lib.lib().vitmi_attention_fwd(CODE[T], B, N, H, DH, scale, x.qkv.ptr(), o.ptr(), lse.ptr(), stream()), "fwd")
    return {"o": o, "lse": lse}


def run_bwd(T, B, N, H, scale, x: Inputs, bias=False):
    lib = _lib.lib()
    D = H * DH
    dqkv = dev_out(B * N, 3 * D, T)
    if bias:
        ws, nws = dev_ws(lib.vitmi_attention_bwd_bias_workspace_size(B, N, H))
        db = ra.aligned(1, 3 * D, F32, "guard").set(torch.zeros(1, 3 * D)).to(DEV)
        check_rc(lib.vitmi_attention_bwd_bias(CODE[T], B, N, H, DH, scale, x.qkv.ptr(), x.o.ptr(), x.do.ptr(), x.lse.ptr(),
                                              dqkv.ptr(), db.ptr(), ws.ptr(), nws, stream()), "bwd_bias")
        return {"dqkv": dqkv, "ws": ws, "dbias": db}
    ws, nws = dev_ws(lib.vitmi_attention_bwd_workspace_size(B, N, H))
    assert nws == B * H * N * 4
    check_rc(lib.vitmi_attention_bwd(CODE[T], B, N, H, DH, scale, x.qkv.ptr(), x.o.ptr(), x.do.ptr(), x.lse.ptr(),
                                     dqkv.ptr(), ws.ptr(), nws, stream()), "bwd")
    return {"dqkv": dqkv, "ws": ws}


def judge(bufs, ref, H, what):
    """{output: worst |err| / tol}; asserts the guards and that no valid output is NaN."""
    D = H * DH
    got = {"o": bufs["o"].view.cpu(), "lse": bufs["lse"].view.cpu()}
    g = bufs["dqkv"].view.cpu()
    got.update(dq=g[:, :D], dk=g[:, D:2 * D], dv=g[:, 2 * D:])
    worst = {}
    for name in OUTPUTS:
        assert not torch.isnan(got[name]).any(), (what, name, "NaN in a valid output")
        worst[name] = ra.worst_ratio(got[name], *ref[name])
    for k, b in bufs.items():
        assert rg.guards_intact(b), (what, f"guard rows of {k} changed")
    return worst


def run_case(pol, T, B, H, N, family, scale, reps=2, bias=True):
    """One forward + backward under a policy, judged; returns ({output: worst ratio}, kernels)."""
    lib = _lib.lib()
    what = Case(pol, T, B, H, N, family, scale).id
    qkv, do, ref = problem(family, T, B, N, H, scale)
    exp = expected_kernels(pol, T, N)
    x = Inputs(qkv, do, ref)
    lib.vitmi_attention_set_policy(pol)
    try:
        outs = []
        for rep in range(reps):
            if rep == 0:
                with kernel_stats() as st:
                    bufs = {**run_fwd(T, B, N, H, scale, x), **run_bwd(T, B, N, H, scale, x)}
            else:
                bufs = {**run_fwd(T, B, N, H, scale, x), **run_bwd(T, B, N, H, scale, x)}
            sync(what)
            outs.append(bufs)
        wb = run_bwd(T, B, N, H, scale, x, bias=True) if bias else None
        sync(what)
    finally:
        lib.vitmi_attention_set_policy(0)
    worst = judge(outs[0], ref, H, what)                                        # 1, 2
    if reps > 1:
        for k in ("o", "lse", "dqkv"):                                          # 3
            assert same_bits(outs[0][k], outs[1][k]), (what, k, "second run differs")
    if bias:                                                                    # 4
        assert same_bits(outs[0]["dqkv"], wb["dqkv"]), (what, "dqkv differs with the bias gradient")
        for k, b in wb.items():
            assert rg.guards_intact(b), (what, f"guard rows of {k} (bias call) changed")
        db = wb["dbias"].view.cpu()[0]
        assert not torch.isnan(db).any(), (what, "NaN in dbias")
        worst["dbias"] = ra.worst_ratio(db, *ra.bias_bound(wb["dqkv"].view.cpu(), B * N, T == BF))
    x.assert_intact(what)
    assert_kernels(st, exp, what)                                               # 5
    return worst, exp


def kernel_of(exp, name):
    """The label of the kernel that wrote an output."""
    if name in ("o", "lse"):
        return exp[0][-1]
    if len(exp) == 1:            # the streamed fp32 backward records nothing
        return "attn_bwd_dq_f32" if name == "dq" else "attn_bwd_dkv_f32"
    return (exp[1] if name == "dq" or len(exp) == 2 else exp[2])[-1]


def report(what, worst, exp):
    print(f"CONF {what}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + "; kernels " + " ".join(k[-1].replace(" ", "") for k in exp))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_attention_matrix(c):
    worst, exp = run_case(c.pol, c.T, c.B, c.H, c.N, c.family, c.scale)
    report(c.id, worst, exp)
    for name, w in worst.items():
        assert w <= 1.0, (c.id, name, w)


def sweep_blocks():
    return [(lo, min(lo + 31, SWEEP["hi"])) for lo in range(SWEEP["lo"], SWEEP["hi"] + 1, 32)]


def test_case_list_reaches_every_kernel_family():
    """The tables themselves (no launch): the matrix reaches every kernel family of csrc/attention.hip,
    the single-pass backward at NKB 1, 2, 3, 6, 7; with the every-N sweep all of NKB 1..7."""
    reached = {k for c in CASES for k in expected_kernels(c.pol, c.T, c.N)}
    swept = {k for lo, hi in sweep_blocks() for N in range(lo, hi + 1) for pol, T in RUNS for k in expected_kernels(pol, T, N)}
    S = SEQ_MAX
    want = [kname("attn_fwd_bf16"), kname("attn_bwd_dq_bf16"), kname("attn_bwd_dkv_bf16"),
            kname("attn_fwd_seq_bf16", S, 0), kname("attn_fwd_seq64_bf16", S, 0),
            kname("attn_bwd_dq_seq_bf16", S, 0), kname("attn_bwd_dq_seq_bf16", S, 7), kname("attn_bwd_dq_seq64_bf16", S, 7),
            kname("attn_bwd_dkv_seq_bf16", S, 0), kname("attn_bwd_dkv_seq_bf16", S, 7),
            kname("attn_fwd_seq_f32", S), kname("attn_bwd_dq_seq_f32", S), kname("attn_bwd_dkv_seq_f32", S),
            kname("attn_fwd_f32")]
    for k in want + [kname("attn_bwd_fused_seq_bf16", n) for n in (1, 2, 3, 6, 7)]:
        assert k in reached, k
    for n in range(1, 8):
        assert kname("attn_bwd_fused_seq_bf16", n) in swept, n
    assert swept >= set(want)
    assert {(c.B, c.H) for c in CASES} == set(SHAPES) and {c.N for c in CASES} == set(NS)
    assert all({c.scale for c in CASES if (c.B, c.H, c.N) == (B, H, N)} >= set(SCALES) for B, H in SHAPES for N in NS)
    assert all({c.family for c in CASES if c.N == N} == set(ra.FAMILIES) for N in FAMILY_NS)


# ---------------------------------------------------------------- vitmi_attention_fwd_x3 / _f8
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("pol", (0, 1, 2, 3))
def test_attention_fwd_knobs(pol, N, scale):
    """o and lse of both entry points: within the reference bound and bitwise vitmi_attention_fwd's
    (under the same policy; policy 1 does not apply to them, so there under policy 0); o3 =
    [hi | hi | lo]: both hi copies bitwise o, hi + lo within the x3 bound; o8 = [hi | e4m3 block]: hi
    bitwise o (the e4m3 payload is tests/test_gpu_f8.py's); every guard intact.  N > 256 is refused
    with VITMI_ERR_INVALID and nothing is launched or written."""
    lib = _lib.lib()
    B, H = SHAPES[0]
    D = H * DH
    what = f"knobs p{pol} N{N} s{scale}"
    qkv, do, ref = problem("rows", BF, B, N, H, scale)
    x = Inputs(qkv, do, ref)
    base = "attn_fwd_seq_bf16" if pol == 2 else "attn_fwd_seq64_bf16"
    lib.vitmi_attention_set_policy(pol)
    try:
        o3, o8 = dev_out(B * N, 3 * D, BF), dev_out(B * N, 2 * D, BF)
        a = {"o": dev_out(B * N, D, BF), "lse": dev_out(B * H, N, F32)}
        b = {"o": dev_out(B * N, D, BF), "lse": dev_out(B * H, N, F32)}
        with kernel_stats() as st:
            rc3 = lib.vitmi_attention_fwd_x3(B, N, H, DH, scale, x.qkv.ptr(), a["o"].ptr(), o3.ptr(), a["lse"].ptr(), stream())
            rc8 = lib.vitmi_attention_fwd_f8(B, N, H, DH, scale, x.qkv.ptr(), b["o"].ptr(), o8.ptr(), b["lse"].ptr(), stream())
        sync(what)
        if N > SEQ_MAX:
            assert rc3 == VITMI_ERR_INVALID and rc8 == VITMI_ERR_INVALID, (what, rc3, rc8)
            assert not st.k, (what, st.k)
            for p in (o3, o8, *a.values(), *b.values()):
                fresh = rg.Padded(p.rows, p.cols, p.pitch, p.dtype, p.bits, p.offset)
                assert torch.equal(p.buf.cpu().view(torch.uint8), fresh.buf.view(torch.uint8)), (what, "written to")
            return
        check_rc(rc3, what)
        check_rc(rc8, what)
        lib.vitmi_attention_set_policy(0 if pol == 1 else pol)
        plain = run_fwd(BF, B, N, H, scale, x)
        sync(what)
    finally:
        lib.vitmi_attention_set_policy(0)
    assert_kernels(st, [kname(base, SEQ_MAX, 1), kname(base, SEQ_MAX, 2)], what)
    worst = {}
    for tag, r in (("x3", a), ("f8", b)):
        for k in ("o", "lse"):
            got = r[k].view.cpu()
            assert not torch.isnan(got).any(), (what, tag, k)
            worst[f"{tag}.{k}"] = ra.worst_ratio(got, *ref[k])
            assert same_bits(r[k], plain[k]), (what, tag, k, "differs from vitmi_attention_fwd")
    o = plain["o"].view.cpu()
    y3, y8 = o3.view.cpu(), o8.view.cpu()
    assert torch.equal(y3[:, :D].view(torch.int16), o.view(torch.int16)), (what, "o3 hi != o")
    assert torch.equal(y3[:, D:2 * D].view(torch.int16), o.view(torch.int16)), (what, "o3 second hi != o")
    assert torch.equal(y8[:, :D].view(torch.int16), o.view(torch.int16)), (what, "o8 hi != o")
    assert not torch.isnan(y3).any()
    worst["hi+lo"] = ra.worst_ratio(y3[:, :D].double() + y3[:, 2 * D:].double(), *ref["hi+lo"])
    for p in (o3, o8, *a.values(), *b.values(), *plain.values()):
        assert rg.guards_intact(p), (what, "guard rows changed")
    x.assert_intact(what)
    print(f"CONF {what}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; kernels {base}")
    for name, w in worst.items():
        assert w <= 1.0, (what, name, w)


# ---------------------------------------------------------------- every N
@pytest.mark.parametrize("lo,hi", sweep_blocks(), ids=[f"N{lo}-{hi}" for lo, hi in sweep_blocks()])
def test_attention_every_n(lo, hi):
    """Every N of the block under every (policy, type): assertions 1, 2 and 5.  One float64 reference
    per N serves the six runs; every failing (N, run, output) is reported, not the first."""
    failures, block = [], {}
    for N in range(lo, hi + 1):
        for pol, T in RUNS:
            tag = f"N{N} p{pol} {TN[T]}"
            try:
                worst, exp = run_case(pol, T, SWEEP["B"], SWEEP["H"], N, SWEEP["family"], SWEEP["scale"], reps=1, bias=False)
            except AssertionError as e:
                failures.append((tag, str(e)[:300]))
                continue
            for k, w in worst.items():
                key = (kernel_of(exp, k).replace(" ", ""), k)
                block[key] = max(block.get(key, 0.0), w)
                if not w <= 1.0:
                    failures.append((tag, k, round(w, 3)))
    print(f"CONF sweep N{lo}-{hi}: worst |err|/tol " + " ".join(f"{a}.{b} {w:.3f}" for (a, b), w in sorted(block.items())))
    assert not failures, failures


# ---------------------------------------------------------------- more pairs than compute units
def pairs_shape(which):
    """(B, H) with B H = CUs - 1, CUs or CUs + 3: H = 3 where 3 divides the count, else the next small
    divisor (256 CUs: 255 = 85 x 3, 256 = 64 x 4, 259 = 37 x 7)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bh = cus + {"cus-1": -1, "cus": 0, "cus+3": 3}[which]
    H = next(h for h in (3, 4, 5, 7, 2, 1) if bh % h == 0)
    return bh // H, H


@pytest.mark.parametrize("N", (33, 197))
@pytest.mark.parametrize("pol", (0, 3))
@pytest.mark.parametrize("which", ("cus-1", "cus", "cus+3"))
def test_attention_persistent_walk(which, pol, N):
    """The persistent backward kernels (one workgroup per compute unit walking the pairs through both
    LDS buffers): one pair per workgroup, and two pairs in some workgroups and one in the others.
    Assertions 1-3 and 5."""
    B, H = pairs_shape(which)
    worst, exp = run_case(pol, BF, B, H, N, "rows", 0.3, reps=2, bias=False)
    report(f"walk {which} B{B}H{H} p{pol} N{N}", worst, exp)
    for name, w in worst.items():
        assert w <= 1.0, (which, pol, N, name, w)
