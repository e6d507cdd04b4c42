"""GEMM conformance matrix on the MI355X: every row of csrc/gemm.hip's dispatch table x the layouts
it is instantiated for x operand type x kernel path, against the float64 reference and the derived
per-element bound of tests/ref_gemm.py.

Every case asserts
  1. |got - ref| <= tol for EVERY element of every output (the worst ratio is printed),
  2. the guard rows / pitch columns / leading elements around every buffer are bitwise intact and no
     valid output is NaN (operand padding is NaN: a read past the range check poisons an output),
  3. a second run is bitwise equal,
  4. which kernels ran (vitmi_stats_*): gemm_kernel / gemm256_kernel / gemm_tail_fixup_kernel /
     splitk_reduce*, against a host-side model of the launch plan,
  5. the workspace query is > 0 exactly when that plan splits.

Shapes are the smallest that reach the code: *edges* 261 x 264 (2x2 tiles of 256, 3x3 of 128, 5 ragged
rows, 8 ragged columns) over two K-steps; *tail* 515 x 520 x 1024, 9 tiles on policy 3's 8 blocks
(ntail 1, S 4, 16 K-steps: every tail-splitting epilogue goes through gemm_tail_fixup_kernel),
645 x 648 (the same plan with a 133 x 136 tail tile) and 515 x 776 (12 tiles: ntail 4, S 2); *small* M = 1, N = 1, N % 8 != 0 and the one-K-step fallback;
*split-K* a 136 x 136 output over a 4000-long reduction."""
from dataclasses import dataclass
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import ref_gemm as rg  # noqa: E402
from kstats import kernel_stats  # noqa: E402
from vitmi import _lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF, "f32": F32}
CODE = {F32: 0, BF: 1}
EPI = {"store": 0, "gelu": 1, "residual": 2, "dgelu": 3, "accum": 4}
AUX_TILED, SPLIT_X3, SPLIT_F8 = 0x100, 0x200, 0x400
VITMI_BF16F8, VITMI_BF16F8W = 4, 5
PATH_SITE, DROP_SITE, RATE_DROP, RATE_PATH = 0x40000003, 4, 0.25, 0.5
TAIL_SMAX, TAIL_MINK = 4, 16     # csrc/gemm.hip TAIL_SMAX / TAIL_MINK

L_FWD = ("KK",)
L_3 = ("KK", "KN", "NN")
L_ALL = ("KK", "KN", "NN", "NK")

# ---------------------------------------------------------------- the table
# dispatch<T> row -> (base epilogue, C types, layouts, entry point, operand types)
#   C type "op": the operand type (BIAS_GELU on bf16 operands writes bf16, on fp32 operands fp32)
ROWS = {
    "store":              ("store",    ("bf16", "f32"), L_3,   "gemm",     ("bf16", "f32")),
    "gelu":               ("gelu",     ("op",),         L_3,   "gemm",     ("bf16", "f32")),
    "residual":           ("residual", ("f32",),        L_3,   "gemm",     ("bf16", "f32")),
    "dgelu":              ("dgelu",    ("bf16", "f32"), L_3,   "gemm",     ("bf16", "f32")),
    "accum":              ("accum",    ("f32",),        L_ALL, "gemm",     ("bf16", "f32")),
    "gelu+drop":          ("gelu",     ("op",),         L_FWD, "dropout",  ("bf16", "f32")),
    "residual+drop":      ("residual", ("f32",),        L_FWD, "dropout",  ("bf16", "f32")),
    "residual+path":      ("residual", ("f32",),        L_FWD, "droppath", ("bf16", "f32")),
    "residual+drop+path": ("residual", ("f32",),        L_FWD, "droppath", ("bf16", "f32")),
    "gelu|x3":            ("gelu",     ("bf16",),       L_FWD, "fwd",      ("bf16",)),
}
# rows whose Epi::tail_split holds (every one but ACCUM; SPLIT_F8 is in the f8 table below)
TAIL_SPLITS = {r for r in ROWS if r != "accum"}


@dataclass(frozen=True)
class Case:
    row: str
    lay: str
    T: str          # operand type
    C: str          # output type
    M: int
    N: int
    K: int
    pol: int
    var: str = ""   # "" | "ldc+1" | "offset1" | "vst-tail" | "dense" | "ws-null" | "ws-short"

    @property
    def id(self):
        v = f"-{self.var}" if self.var else ""
        return f"{self.row}-{self.lay}-{self.T}>{self.C}-{self.M}x{self.N}x{self.K}-p{self.pol}{v}"


def kmajor_reduction(lay):
    return lay != "NN"            # a k-major operand needs K % BK == 0


def _cases():
    out = []

    def add(row, M, N, kk, kn, pols_bf16, var="", lays=None, types=None, ctypes_=None):
        base, cts, rlays, _, ops_t = ROWS[row]
        for T in (types or ops_t):
            for lay in (lays or rlays):
                K = kk[T] if kmajor_reduction(lay) else kn
                for C in (ctypes_ or cts):
                    C = T if C == "op" else C
                    for pol in (pols_bf16 if T == "bf16" else (1,)):
                        out.append(Case(row, lay, T, C, M, N, K, pol, var))

    for row in ROWS:
        # edges: two K-steps (bf16 K = 128, fp32 K = 96), ragged K = 100 where both operands are m-major
        add(row, 261, 264, {"bf16": 128, "f32": 96}, 100, (1, 2, 3))
        # tail: 16 K-steps (bf16 only: the fp32 operands have no gemm256 path)
        add(row, 515, 520, {"bf16": 1024}, 1000, (1, 2, 3), types=("bf16",))
    for row in sorted(TAIL_SPLITS):
        add(row, 515, 776, {"bf16": 1024}, 1000, (3,), lays=("KK",), types=("bf16",))
        # the tail tile of 515 x 520 is the 3 x 8 corner: 645 x 648 (9 tiles again) leaves the fix-up
        # kernel a 133 x 136 corner, enough elements for a rounding error to show
        add(row, 645, 648, {"bf16": 1024}, 1000, (3,), types=("bf16",))
    # ACCUM at the tail shape plans 4 K-slabs: onto the pitched C above it runs unsplit (the reduce
    # kernels need ldc == N); onto a dense C it splits
    add("accum", 515, 520, {"bf16": 1024}, 1000, (1, 2, 3), var="dense", types=("bf16",))
    # small: M = 1, N = 1, N % 8 != 0, and one K-step (policy 2 must fall back to the 128 kernel)
    for (M, N, K) in ((5, 8, 128), (1, 13, 64), (1, 1, 64), (130, 136, 64)):
        for row in ("store", "gelu", "residual", "dgelu", "accum"):
            add(row, M, N, {"bf16": K, "f32": K}, K, (1, 2), lays=("KK", "KN"))
    # the 128x128 kernel's scalar store branch: ldc % 4 != 0, and a C that is not 8-byte aligned
    for row in ("store", "gelu", "dgelu"):
        for var in ("ldc+1", "offset1"):
            add(row, 261, 264, {"bf16": 128}, 100, (1,), var=var, types=("bf16",), ctypes_=("bf16",))
        # ... and the vector branch's `col0 + 4 > N` tail: ldc % 4 == 0 with N % 4 != 0
        for (M, N) in ((1, 13), (131, 133)):
            add(row, M, N, {"bf16": 64}, 64, (1,), var="vst-tail", lays=("KK", "NN"), types=("bf16",), ctypes_=("bf16",))
    # split-K: 136 x 136 over a 4000-long ragged reduction onto a nonzero C.  A k-major bf16 operand
    # needs K % 64 == 0, so there the nearest served length is 4032 (the refusal of 4000 is tested
    # below); fp32 operands take 4000 = 125 x 32 in every layout
    add("accum", 136, 136, {"bf16": 4032, "f32": 4000}, 4000, (1, 2, 3))
    add("accum", 1, 136, {"bf16": 4032, "f32": 4000}, 4000, (1, 2), lays=("KK", "KN"))
    # a NULL workspace, and one a byte short of the tail plan: the unsplit launch, same bound
    for var in ("ws-null", "ws-short"):
        for row in ("store", "gelu", "residual", "dgelu"):
            add(row, 515, 520, {"bf16": 1024}, 1000, (3,), var=var, lays=("KK",), types=("bf16",), ctypes_=None)
    add("accum", 136, 136, {"bf16": 4032, "f32": 4000}, 4000, (1, 2), var="ws-null", lays=("NN", "NK"))
    return out


CASES = _cases()


# ---------------------------------------------------------------- host-side model of the launch plan
def cdiv(a, b):
    return -(-a // b)


def cus():
    return _lib.lib().vitmi_device_cus()


def tail_plan(nwg, gx, nk):
    """csrc/gemm.hip tail_plan: (S, ntail) or None."""
    ntail = nwg % gx
    if nwg < gx or ntail == 0 or 2 * ntail > gx or nk < 4:
        return None
    S = min(gx // ntail, TAIL_SMAX)
    if S < 2:
        return None
    ks = max(cdiv(nk, S), 2)
    S = cdiv(nk, ks)
    while S > 1 and nk - (S - 1) * ks < 2:
        ks += 1
        S = cdiv(nk, ks)
    return (S, ntail) if S > 1 else None


def grid256(nwg, pol):
    gx = cus()
    if gx < 8 or pol == 3:
        gx = 8
    return min(gx, nwg)


def choose_splits(bf16, M, N, K, pol):
    big = bf16 and N % 8 == 0 and pol >= 2
    t = 256 if big else 128
    tiles = cdiv(M, t) * cdiv(N, t)
    ktiles = cdiv(K, 64 if bf16 else 32)
    avail = max(cus(), 8)
    cap, slab = 64, M * N * 4
    if slab > 0 and (32 << 20) // slab > cap:
        cap = min((32 << 20) // slab, 512)
    return max(min((avail if big else 2 * avail) // tiles, ktiles // 4, cap), 1)


def plan(base, bf16, M, N, Kred, pol, tail_split, f8=False, ws="query", dense_c=True):
    """What the launch is expected to be: {"big", "fixup", "reduce", "ws"}; Kred in operand units
    as the kernel walks them (2K / 1.5K bf16 units for the VITMI_BF16F8 forms).  A split-K ACCUM
    needs its workspace and a dense C (the reduce kernels add onto ldc == N); otherwise the same
    sum runs unsplit."""
    use256 = f8 or (bf16 and N % 8 == 0 and pol >= 2)
    nk = cdiv(Kred, 64 if bf16 else 32)
    p = {"big": use256 and nk >= 2, "fixup": False, "reduce": False, "ws": False}
    if base == "accum":
        s = choose_splits(bf16, M, N, Kred, pol)
        p["ws"] = s > 1
        p["reduce"] = s > 1 and ws == "query" and dense_c
        return p
    if use256:
        nwg = cdiv(M, 256) * cdiv(N, 256)
        tp = tail_plan(nwg, grid256(nwg, pol), nk)
        p["ws"] = tp is not None
        p["fixup"] = (tp is not None and p["big"] and tail_split and ws == "query"
                      and nk >= (0 if base == "dgelu" else TAIL_MINK))
    return p


def assert_kernels(st, p, what):
    assert st.calls("gemm256_kernel") == (1 if p["big"] else 0), (what, st.k)
    assert st.calls("gemm_kernel") == (0 if p["big"] else 1), (what, st.k)
    assert st.calls("gemm_tail_fixup_kernel") == (1 if p["fixup"] else 0), (what, st.k)
    assert st.calls("splitk_reduce") == (1 if p["reduce"] else 0), (what, st.k)


# ---------------------------------------------------------------- inputs (CPU, built once)
def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def pitch_of(cols, dtype, dense):
    q = 8 if dtype == BF else 4          # 16-byte multiples
    return cols if dense else cdiv(max(cols, 1), q) * q + q


@lru_cache(maxsize=None)
def operands(T, lay, M, N, K, dense):
    """(A, B) as stored, NaN in the pitch columns and in the guard rows (for an m-major operand those
    are the rows before 0 and past K of a larger allocation)."""
    ak, bk = rg.LAYOUTS[lay]
    dt = DT[T]
    ar, ac = (M, K) if ak else (K, M)
    br, bc = (N, K) if bk else (K, N)
    a = rg.padded(ar, ac, pitch_of(ac, dt, dense), dt, "nan").set(rnd(ar, ac, seed=1))
    b = rg.padded(br, bc, pitch_of(bc, dt, dense), dt, "nan").set(rnd(br, bc, seed=2, scale=0.05))
    return a, b


@lru_cache(maxsize=None)
def side(M, N, T):
    return dict(bias=rnd(N, seed=3), aux=rg.gelu_grad(rnd(M, N, seed=4)).to(DT[T]), residual=rnd(M, N, seed=5),
                prev=rnd(M, N, seed=6))


@lru_cache(maxsize=None)
def rows_per_sample(M):
    """A sequence length that divides M into 3..16 samples (261 = 9 x 29, 515 = 5 x 103)."""
    return M // max(d for d in range(3, 17) if M % d == 0)


@lru_cache(maxsize=None)
def drop_seed(M):
    """A seed whose drop-path mask keeps some samples of M and drops others."""
    rps = rows_per_sample(M)
    for s in range(1, 64):
        f = rg.path_factor(s, PATH_SITE, RATE_PATH, M, rps)
        if 0 < int((f == 0).sum()) < M:
            return s
    raise AssertionError("no mixed drop-path mask")


def drop_args(row, M):
    if "+" not in row:
        return None, None
    seed = drop_seed(M)
    drop =(seed, DROP_SITE, RATE_DROP) if "drop" in row.split("+")[1:] else None
    path = (seed, PATH_SITE, RATE_PATH, rows_per_sample(M)) if "path" in row.split("+")[1:] else None
    return drop, path


@lru_cache(maxsize=None)
def reference(row, lay, T, C, M, N, K):
    """The float64 reference and bound of a (row, layout, types, shape): once, shared by every path."""
    base = ROWS[row][0]
    a, b = operands(T, lay, M, N, K, ROWS[row][3] != "gemm")
    s = side(M, N, T)
    drop, path = drop_args(row, M)
    return rg.reference(a.view, b.view, lay, base, bias=None if base in ("dgelu", "accum") else s["bias"],
                        aux=s["aux"], residual=s["residual"], prev=s["prev"], out_bf16=C == "bf16",
                        drop=drop, path=path, split_x3=row == "gelu|x3")


# ---------------------------------------------------------------- running a case
def stream():
    return torch.cuda.current_stream().cuda_stream


def check_rc(rc, what):
    assert rc == 0, (what, rc, _lib.lib().vitmi_last_error().decode(errors="replace"))


def workspace(nbytes, var):
    """(tensor or None, pointer, size) for the case's workspace variant."""
    if var == "ws-null" or nbytes == 0:
        return None, None, 0
    if var == "ws-short":
        nbytes -= 1
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return ws, ws.data_ptr(), nbytes


def launch(c: Case, bufs, ws_ptr, ws_n):
    lib = _lib.lib()
    base, _, _, entry, _ = ROWS[c.row]
    ak, bk = rg.LAYOUTS[c.lay]
    a, b, C = bufs["a"], bufs["b"], bufs["C"]
    p = lambda k: bufs[k].ptr() if bufs.get(k) is not None else None          # noqa: E731
    ld = lambda k: bufs[k].pitch if bufs.get(k) is not None else 0            # noqa: E731
    bias = bufs["bias"].data_ptr() if bufs.get("bias") is not None else None
    t, ct = CODE[DT[c.T]], CODE[DT[c.C]]
    if entry == "gemm":
        return lib.vitmi_gemm(t, int(ak), int(bk), c.M, c.N, c.K, a.ptr(), a.pitch, b.ptr(), b.pitch, C.ptr(),
                              C.pitch, ct, EPI[base], bias, p("aux"), ld("aux"), p("residual"), ld("residual"),
                              ws_ptr, ws_n, stream())
    drop, path = drop_args(c.row, c.M)
    if entry == "fwd":
        return lib.vitmi_linear_fwd(t, c.M, c.N, c.K, a.ptr(), b.ptr(), bias, C.ptr(), ct, EPI[base] | SPLIT_X3,
                                    p("aux"), p("residual"), ws_ptr, ws_n, stream())
    if entry == "dropout":
        thresh, scale = rg.vit_ref.dropout_params(drop[2])
        return lib.vitmi_linear_fwd_dropout(t, c.M, c.N, c.K, a.ptr(), b.ptr(), bias, C.ptr(), ct, EPI[base], p("aux"),
                                            p("residual"), ws_ptr, ws_n, drop[0], drop[1], thresh, scale, stream())
    dthresh, dscale = rg.vit_ref.dropout_params(drop[2]) if drop else (0, 1.0)
    pthresh, pscale = rg.vit_ref.dropout_params(path[2])
    return lib.vitmi_linear_fwd_droppath(t, c.M, c.N, c.K, a.ptr(), b.ptr(), bias, C.ptr(), ct, EPI[base], p("residual"),
                                         ws_ptr, ws_n, path[0], drop[1] if drop else 0, dthresh, dscale, path[3],
                                         path[1], pthresh, pscale, stream())


def c_pitch(c: Case):
    """ldc of a case: N + 8 through vitmi_gemm (N + 1: the scalar-store variant), dense for the
    split-K shapes and the "dense" variant, and for the linear_* entry points."""
    if ROWS[c.row][3] != "gemm":
        return 3 * c.N if c.row == "gelu|x3" else c.N
    if c.var == "dense" or (ROWS[c.row][0] == "accum" and c.K >= 4000):
        return c.N
    if c.var == "vst-tail":
        return cdiv(c.N, 4) * 4 + 4
    return c.N + 1 if c.var == "ldc+1" else c.N + 8


def make_bufs(c: Case):
    """Device buffers of a case: operands (shared CPU images), side inputs with NaN padding, outputs
    with guard fill.  Pitches: ldc = N + 8, ldaux = N + 16, ldr = N + 4 through vitmi_gemm (dense for
    split-K, whose C must be dense, and for the linear_* entry points, which take no pitch)."""
    base, _, _, entry, _ = ROWS[c.row]
    dense = entry != "gemm"
    a, b = operands(c.T, c.lay, c.M, c.N, c.K, dense)
    s = side(c.M, c.N, c.T)
    M, N = c.M, c.N
    cdt = F32 if base in ("residual", "accum") else DT[c.C]
    wide = 3 * N if c.row == "gelu|x3" else N
    ldc = c_pitch(c)
    off = 0
    if c.var == "offset1":
        off = 1 if (rg.GUARD_ROWS * ldc) % 2 == 0 else 2
    bufs = {"a": a.to(DEV), "b": b.to(DEV)}
    Cb = rg.padded(M, wide, ldc, cdt, "guard", offset=off)
    if base == "accum":
        Cb.set(s["prev"])
    bufs["C"] = Cb.to(DEV)
    if c.var == "offset1":
        assert bufs["C"].ptr() % 4 == 2
    if c.var == "vst-tail":      # the vector store branch, whose last group is the scalar `col0 + 4 > N` tail
        assert bufs["C"].ptr() % 8 == 0 and ldc % 4 == 0 and N % 4 != 0
    if base not in ("dgelu", "accum"):
        bufs["bias"] = s["bias"].to(DEV)
    if base == "gelu":
        bufs["aux"] = rg.padded(M, N, N if dense else N + 16, DT[c.T], "guard").to(DEV)
    if base == "dgelu":
        bufs["aux"] = rg.padded(M, N, N if dense else N + 16, DT[c.T], "nan").set(s["aux"]).to(DEV)
    if base == "residual":
        bufs["residual"] = rg.padded(M, N, N if dense else N + 4, F32, "nan").set(s["residual"]).to(DEV)
    return bufs


def ws_query(c: Case):
    lib = _lib.lib()
    base, _, _, entry, _ = ROWS[c.row]
    ak, bk = rg.LAYOUTS[c.lay]
    if entry == "gemm":
        return lib.vitmi_gemm_workspace_size(CODE[DT[c.T]], int(ak), int(bk), c.M, c.N, c.K, EPI[base])
    return lib.vitmi_linear_fwd_workspace_size(CODE[DT[c.T]], c.M, c.N, c.K)


def compare(c: Case, bufs, ref):
    """{output: worst ratio}; asserts bound, NaN-freedom and guards."""
    worst = {}
    N = c.N
    got = {"C": bufs["C"].view.cpu()}
    if "aux" in ref:
        got["aux"] = bufs["aux"].view.cpu()
    if c.row == "gelu|x3":
        y = got["C"]
        assert torch.equal(y[:, :N], y[:, N:2 * N]), "SPLIT_X3: the two hi copies differ"
        got["C"], got["hi+lo"] = y[:, :N], y[:, :N].double() + y[:, 2 * N:].double()
    for name, (r, tol) in ref.items():
        assert not torch.isnan(got[name]).any(), (c.id, name, "NaN in a valid output")
        worst[name] = rg.worst_ratio(got[name], r, tol)
    for k, bbuf in bufs.items():
        if isinstance(bbuf, rg.Padded):
            assert rg.guards_intact(bbuf), (c.id, f"guard bytes of {k} changed")
    return worst


def run_case(c: Case):
    lib = _lib.lib()
    base = ROWS[c.row][0]
    ref = reference(c.row, c.lay, c.T, c.C, c.M, c.N, c.K)
    p = plan(base, c.T == "bf16", c.M, c.N, c.K, c.pol, c.row in TAIL_SPLITS,
             ws="query" if not c.var.startswith("ws-") else c.var, dense_c=c_pitch(c) == c.N)
    lib.vitmi_gemm_set_policy(c.pol)
    try:
        nws = ws_query(c)
        assert (nws > 0) == p["ws"], (c.id, "workspace query", nws, p)
        outs = []
        for rep in range(2):
            bufs = make_bufs(c)
            ws, ws_ptr, ws_n = workspace(nws, c.var)
            if rep == 0:
                with kernel_stats() as st:
                    rc = launch(c, bufs, ws_ptr, ws_n)
            else:
                rc = launch(c, bufs, ws_ptr, ws_n)
            check_rc(rc, c.id)
            torch.cuda.synchronize()
            outs.append(bufs)
        worst = compare(c, outs[0], ref)
        print(f"{c.id}: worst |err|/tol " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; kernels {st.summary()}")
        for name, w in worst.items():
            assert w <= 1.0, (c.id, name, w)
        for k in ("C", "aux"):
            if k in outs[0]:
                assert torch.equal(outs[0][k].buf.view(torch.uint8), outs[1][k].buf.view(torch.uint8)), (c.id, k, "second run differs")
        assert_kernels(st, p, c.id)
        return outs[0]
    finally:
        lib.vitmi_gemm_set_policy(0)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_gemm_matrix(c):
    run_case(c)


def test_table_reaches_what_it_claims():
    """The table itself (no launch): under policy 3 the tail shapes plan a fix-up for every row whose
    Epi::tail_split holds and none for ACCUM; the one-K-step shape falls back; split-K plans a reduce."""
    tails = [c for c in CASES if c.M == 515 and c.pol == 3 and not c.var]
    assert {c.row for c in tails} == set(ROWS)
    for c in tails:
        p = plan(ROWS[c.row][0], True, c.M, c.N, c.K, 3, c.row in TAIL_SPLITS)
        assert p["fixup"] == (c.row != "accum") and p["big"], c.id
    assert tail_plan(9, 8, 16) == (4, 1) and tail_plan(12, 8, 16) == (2, 4)
    assert tail_plan(9, 8, 12) is not None         # K = 768 plans, but only DGELU splits there
    one = [c for c in CASES if (c.M, c.N, c.K) == (130, 136, 64) and c.pol == 2 and c.T == "bf16"]
    assert one and all(not plan(ROWS[c.row][0], True, c.M, c.N, c.K, 2, True)["big"] for c in one)
    sk = [c for c in CASES if c.K >= 4000 and not c.var]
    assert {c.lay for c in sk if c.M == 136} == set(L_ALL) and {c.lay for c in sk if c.M == 1} == {"KK", "KN"}
    assert all(plan("accum", c.T == "bf16", c.M, c.N, c.K, c.pol, False)["reduce"] for c in sk)


# ---------------------------------------------------------------- VITMI_BF16F8 operands (gemm256 only)
# row -> (base, C type, epilogue flag, N at the edges shape, N at the tail shape); dtype 4, and one
# VITMI_BF16F8W (dtype 5) case
F8_ROWS = {
    "f8 store>bf16": ("store", "bf16", 0, 272, 528),
    "f8 store>f32":  ("store", "f32", 0, 272, 528),
    "f8 residual":   ("residual", "f32", 0, 272, 528),
    "f8 gelu|f8":    ("gelu", "bf16", SPLIT_F8, 320, 576),
}
F8_CASES = [(row, "edges", pol, False) for row in F8_ROWS for pol in (2, 3)] + \
           [(row, shape, 3, False) for row in F8_ROWS for shape in ("tail", "tail2")] + \
           [("f8 store>f32", "edges", 2, True)]


@lru_cache(maxsize=None)
def f8_inputs(M, N, K, wform):
    xs, xd = rg.f8_rows(rnd(M, K, seed=1), weight=False, wform=wform)
    ws_, wd = rg.f8_rows(rnd(N, K, seed=2, scale=0.05), weight=True, wform=wform)
    return xs, xd, ws_, wd


@pytest.mark.parametrize("row,shape,pol,wform", F8_CASES,
                         ids=[f"{r}-{s}-p{p}{'-f8w' if w else ''}" for r, s, p, w in F8_CASES])
def test_gemm_matrix_f8(row, shape, pol, wform):
    """The four VITMI_BF16F8 rows (and one VITMI_BF16F8W case) against float64 products of the
    decoded [hi | e4m3] rows, t_acc over K' = 2K (1.5K).  SPLIT_F8 output rows [hi | hi8 | lo8]:
    hi within the GELU bound, hi8 = e4m3(hi) exactly, hi + lo8 / 2^9 within the GELU bound with the
    e4m3 half-ulp 2^-4 ubf |ref| (+ 2^-19, half the least e4m3 subnormal / 2^9) for the bf16 term."""
    lib = _lib.lib()
    base, C, flag, n_edge, n_tail = F8_ROWS[row]
    # (tail2: a 133-row corner tile 144 / 192 columns wide for the fix-up kernel, as in the bf16 table)
    M, N, K = {"edges": (261, n_edge, 128), "tail": (515, n_tail, 512), "tail2": (645, n_tail + 128, 512)}[shape]
    kred = K + K // 2 if wform else 2 * K
    xs, xd, ws_, wd = f8_inputs(M, N, K, wform)
    s = side(M, N, "bf16")
    ref = rg.reference(xd, wd, "KK", base, bias=s["bias"], residual=s["residual"], out_bf16=C == "bf16",
                       aux_bf16=True, k_acc=kred)
    p = plan(base, True, M, N, kred, pol, flag != SPLIT_F8, f8=True)
    dtype = VITMI_BF16F8W if wform else VITMI_BF16F8
    wide = 2 * N if flag else N
    lib.vitmi_gemm_set_policy(pol)
    try:
        nws = lib.vitmi_linear_fwd_workspace_size(dtype, M, N, K)
        assert (nws > 0) == p["ws"], (nws, p)
        outs = []
        for rep in range(2):
            x = rg.padded(M, kred, kred, BF, "nan").to(DEV)
            w = rg.padded(N, kred, kred, BF, "nan").to(DEV)
            # (the e4m3 bytes travel as bf16 bit patterns: copy them bitwise)
            x.view.view(torch.int16).copy_(xs.view(torch.int16))
            w.view.view(torch.int16).copy_(ws_.view(torch.int16))
            Cb = rg.padded(M, wide, wide, DT[C], "guard").to(DEV)
            bufs = {"x": x, "w": w, "C": Cb, "bias": s["bias"].to(DEV)}
            if base == "gelu":
                bufs["aux"] = rg.padded(M, N, N, BF, "guard").to(DEV)
            if base == "residual":
                bufs["residual"] = rg.padded(M, N, N, F32, "nan").set(s["residual"]).to(DEV)
            ws, ws_ptr, ws_n = workspace(nws, "")
            ptr = lambda k: bufs[k].ptr() if k in bufs else None       # noqa: E731
            call = lambda: lib.vitmi_linear_fwd(dtype, M, N, K, x.ptr(), w.ptr(), bufs["bias"].data_ptr(), Cb.ptr(),  # noqa: E731
                                                CODE[DT[C]], EPI[base] | flag, ptr("aux"), ptr("residual"), ws_ptr,
                                                ws_n, stream())
            if rep == 0:
                with kernel_stats() as st:
                    rc = call()
            else:
                rc = call()
            check_rc(rc, row)
            torch.cuda.synchronize()
            outs.append(bufs)
        bufs = outs[0]
        y = bufs["C"].view.cpu()
        got = {"C": y[:, :N]}
        if "aux" in ref:
            got["aux"] = bufs["aux"].view.cpu()
        if flag:
            e = y.contiguous().view(torch.uint8)[:, 2 * N:].reshape(M, N // 64, 2, 64)
            hi8, lo8 = e[:, :, 0].reshape(M, N).view(rg.E4), e[:, :, 1].reshape(M, N).view(rg.E4)
            assert torch.equal(hi8.view(torch.uint8), rg._e4m3(got["C"].float()).view(torch.uint8)), "hi8 != e4m3(hi)"
            r, tol = ref["C"]
            got["hi+lo8"] = got["C"].double() + lo8.double() / 512.0
            ref = dict(ref)
            ref["hi+lo8"] = (r, tol - rg.UBF * r.abs() + 2.0 ** -4 * rg.UBF * r.abs() + 2.0 ** -19)
        worst = {}
        for name, (r, tol) in ref.items():
            assert not torch.isnan(got[name].double()).any(), (row, name)
            worst[name] = rg.worst_ratio(got[name], r, tol)
        print(f"{row}-{shape}-p{pol}{'-f8w' if wform else ''}: worst |err|/tol "
              + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; kernels {st.summary()}")
        for name, wv in worst.items():
            assert wv <= 1.0, (row, name, wv)
        for k, b in bufs.items():
            if isinstance(b, rg.Padded):
                assert rg.guards_intact(b), (row, k)
        for k in ("C", "aux"):
            if k in bufs:
                assert torch.equal(bufs[k].buf.view(torch.uint8), outs[1][k].buf.view(torch.uint8)), (row, k)
        assert_kernels(st, p, row)
    finally:
        lib.vitmi_gemm_set_policy(0)


# ---------------------------------------------------------------- AUX_TILED on the GELU -> DGELU pair
@pytest.mark.parametrize("M,N,K,fpol,bpol", [(261, 264, 128, 1, 1), (261, 264, 128, 2, 2), (261, 264, 128, 1, 2),
                                             (261, 264, 128, 2, 1), (515, 520, 1024, 3, 3), (645, 648, 1024, 3, 3)])
def test_gemm_matrix_aux_tiled(M, N, K, fpol, bpol):
    """gelu' kept in the opaque tile-native buffer: the DGELU result through it elementwise (the
    bound of DGELU plus |acc2| x the GELU bound of the gelu' it read), the GELU activation itself, and
    the bytes past vitmi_aux_tiled_bytes untouched."""
    lib = _lib.lib()
    a, b = operands("bf16", "KK", M, N, K, True)
    dy, w2 = operands("bf16", "KN", M, N, 256, True)      # C2[M, N] = dy[M, 256] W2[256, N] * gelu'
    s = side(M, N, "bf16")
    fwd = rg.reference(a.view, b.view, "KK", "gelu", bias=s["bias"], out_bf16=True)
    gp, gp_tol = fwd["aux"]
    bwd = rg.reference(dy.view, w2.view, "KN", "dgelu", aux=gp, out_bf16=True)
    A2, B2 = rg.logical(dy.view, w2.view, "KN")
    r2, t2 = bwd["C"]
    t2 = t2 + (A2 @ B2).abs() * gp_tol
    nb = lib.vitmi_aux_tiled_bytes(M, N)
    assert nb == cdiv(M, 256) * cdiv(N, 256) * 131072
    try:
        outs = []
        for rep in range(2):
            ad, bd, dyd, w2d = a.to(DEV), b.to(DEV), dy.to(DEV), w2.to(DEV)
            aux = rg.padded(1, nb // 2, nb // 2, BF, "guard").to(DEV)
            Cf = rg.padded(M, N, N + 8, BF, "guard").to(DEV)
            Cb = rg.padded(M, N, N + 8, BF, "guard").to(DEV)
            bias = s["bias"].to(DEV)
            lib.vitmi_gemm_set_policy(fpol)
            nws = lib.vitmi_gemm_workspace_size(1, 1, 1, M, N, K, EPI["gelu"])
            ws, wp, wn = workspace(nws, "")
            with kernel_stats() as sf:
                check_rc(lib.vitmi_gemm(1, 1, 1, M, N, K, ad.ptr(), ad.pitch, bd.ptr(), bd.pitch, Cf.ptr(), Cf.pitch, 1,
                                        EPI["gelu"] | AUX_TILED, bias.data_ptr(), aux.ptr(), N, None, 0, wp, wn,
                                        stream()), "gelu|tiled")
            lib.vitmi_gemm_set_policy(bpol)
            nws2 = lib.vitmi_gemm_workspace_size(1, 1, 0, M, N, 256, EPI["dgelu"])
            ws2, wp2, wn2 = workspace(nws2, "")
            with kernel_stats() as sb:
                check_rc(lib.vitmi_gemm(1, 1, 0, M, N, 256, dyd.ptr(), dyd.pitch, w2d.ptr(), w2d.pitch, Cb.ptr(),
                                        Cb.pitch, 1, EPI["dgelu"] | AUX_TILED, None, aux.ptr(), N, None, 0, wp2, wn2,
                                        stream()), "dgelu|tiled")
            torch.cuda.synchronize()
            outs.append((Cf, Cb, aux, ad, bd, dyd, w2d))
        Cf, Cb, aux = outs[0][:3]
        wf = rg.worst_ratio(Cf.view.cpu(), *fwd["C"])
        wb = rg.worst_ratio(Cb.view.cpu(), r2, t2)
        print(f"aux-tiled {M}x{N}x{K} p{fpol}/p{bpol}: worst |err|/tol gelu {wf:.3f} dgelu {wb:.3f}; "
              f"kernels {sf.summary()} / {sb.summary()}")
        assert wf <= 1.0 and wb <= 1.0
        assert not torch.isnan(Cb.view).any() and not torch.isnan(Cf.view).any()
        for t in outs[0]:
            assert rg.guards_intact(t)       # aux: the rows before and after its nb bytes
        for x, y in zip(outs[0][:3], outs[1][:3]):
            assert torch.equal(x.buf.view(torch.uint8), y.buf.view(torch.uint8))
        assert_kernels(sf, plan("gelu", True, M, N, K, fpol, True), "gelu|tiled")
        assert_kernels(sb, plan("dgelu", True, M, N, 256, bpol, True), "dgelu|tiled")
    finally:
        lib.vitmi_gemm_set_policy(0)


# ---------------------------------------------------------------- DGELU with the fused bias gradient
@pytest.mark.parametrize("pol", [1, 2, 3])
@pytest.mark.parametrize("C", ["bf16", "f32"])
def test_gemm_matrix_dgrad_bias(pol, C):
    """vitmi_linear_dgrad_bias at the tail shape: dx elementwise, and db += the column sums of dx
    against the float64 column sums.  Bound of db[k]: the sum over the rows of dx's own bound (the
    sums take dx before or after its rounding, depending on the path) + (M + 1) u32 sum |dx| for the
    fp32 additions in any order + u32 |db before|."""
    lib = _lib.lib()
    M, N, K = 515, 520, 1024                       # dx [M, N] = dy [M, K] W [K, N]
    dy, w = operands("bf16", "KN", M, N, K, True)
    s = side(M, N, "bf16")
    r, tol = rg.reference(dy.view, w.view, "KN", "dgelu", aux=s["aux"], out_bf16=C == "bf16")["C"]
    db0 = rnd(N, seed=9)
    rdb = db0.double() + r.sum(0)
    tdb = tol.sum(0) + (M + 1) * rg.U32 * r.abs().sum(0) + rg.U32 * (db0.double().abs() + rdb.abs())
    lib.vitmi_gemm_set_policy(pol)
    try:
        nws = lib.vitmi_linear_dgrad_bias_workspace_size(1, M, K, N)
        assert nws > 0
        outs = []
        for rep in range(2):
            dyd, wd = dy.to(DEV), w.to(DEV)
            aux = rg.padded(M, N, N, BF, "nan").set(s["aux"]).to(DEV)
            dx = rg.padded(M, N, N, DT[C], "guard").to(DEV)
            db = rg.padded(1, N, N, F32, "guard").set(db0.view(1, N)).to(DEV)
            ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
            with kernel_stats() as st:
                check_rc(lib.vitmi_linear_dgrad_bias(1, M, K, N, dyd.ptr(), wd.ptr(), dx.ptr(), CODE[DT[C]], EPI["dgelu"],
                                                     aux.ptr(), db.ptr(), ws.data_ptr(), nws, stream()), "dgrad_bias")
            torch.cuda.synchronize()
            outs.append((dx, db, aux, dyd, wd))
        dx, db = outs[0][:2]
        wx = rg.worst_ratio(dx.view.cpu(), r, tol)
        wdb = rg.worst_ratio(db.view.cpu()[0], rdb, tdb)
        print(f"dgrad+bias {M}x{N}x{K} >{C} p{pol}: worst |err|/tol dx {wx:.3f} db {wdb:.3f}; kernels {st.summary()}")
        assert wx <= 1.0 and wdb <= 1.0
        assert not torch.isnan(dx.view).any() and not torch.isnan(db.view).any()
        for t in outs[0]:
            assert rg.guards_intact(t)
        for x, y in zip(outs[0][:2], outs[1][:2]):
            assert torch.equal(x.buf.view(torch.uint8), y.buf.view(torch.uint8))
        # (this entry point runs its GEMM without a workspace: never a tail split)
        assert_kernels(st, plan("dgelu", True, M, N, K, pol, True, ws="ws-null"), "dgrad_bias")
    finally:
        lib.vitmi_gemm_set_policy(0)


# ---------------------------------------------------------------- degenerate sizes and refusals
@pytest.mark.parametrize("T,pol", [("bf16", 1), ("bf16", 2), ("f32", 1)])
def test_gemm_degenerate_sizes(T, pol):
    """M = 0 returns OK and writes nothing; K = 0 STORE gives C = bias; K = 0 ACCUM leaves C as it
    was."""
    lib = _lib.lib()
    dt = DT[T]
    N = 264
    lib.vitmi_gemm_set_policy(pol)
    try:
        a, b = operands(T, "KK", 261, N, 128 if T == "bf16" else 96, False)
        ad, bd = a.to(DEV), b.to(DEV)
        bias = rnd(N, seed=3).to(DEV)
        # M = 0
        C = rg.padded(0, N, N + 8, dt, "guard").to(DEV)
        with kernel_stats() as st:
            check_rc(lib.vitmi_gemm(CODE[dt], 1, 1, 0, N, a.cols, ad.ptr(), ad.pitch, bd.ptr(), bd.pitch, C.ptr(), C.pitch,
                                    CODE[dt], 0, bias.data_ptr(), None, 0, None, 0, None, 0, stream()), "M = 0")
        torch.cuda.synchronize()
        assert rg.guards_intact(C) and not st.k
        # K = 0: STORE writes the bias, ACCUM adds nothing
        M = 37
        C = rg.padded(M, N, N + 8, dt, "guard").to(DEV)
        check_rc(lib.vitmi_gemm(CODE[dt], 1, 1, M, N, 0, ad.ptr(), ad.pitch, bd.ptr(), bd.pitch, C.ptr(), C.pitch,
                                CODE[dt], 0, bias.data_ptr(), None, 0, None, 0, None, 0, stream()), "K = 0 store")
        prev = rnd(M, N, seed=6)
        Ca = rg.padded(M, N, N + 8, F32, "guard").set(prev).to(DEV)
        check_rc(lib.vitmi_gemm(CODE[dt], 1, 1, M, N, 0, ad.ptr(), ad.pitch, bd.ptr(), bd.pitch, Ca.ptr(), Ca.pitch,
                                0, EPI["accum"], None, None, 0, None, 0, None, 0, stream()), "K = 0 accum")
        torch.cuda.synchronize()
        assert torch.equal(C.view.cpu(), bias.cpu().to(dt).expand(M, N)) and rg.guards_intact(C)
        assert torch.equal(Ca.view.cpu(), prev) and rg.guards_intact(Ca)
    finally:
        lib.vitmi_gemm_set_policy(0)


def test_gemm_workspace_short_is_the_unsplit_result():
    """A workspace one byte short of the tail plan: bitwise the NULL-workspace result (no split)."""
    for row in ("store", "dgelu"):
        short = run_case(Case(row, "KK", "bf16", "bf16", 515, 520, 1024, 3, "ws-short"))
        null = run_case(Case(row, "KK", "bf16", "bf16", 515, 520, 1024, 3, "ws-null"))
        assert torch.equal(short["C"].buf.view(torch.uint8), null["C"].buf.view(torch.uint8))


def test_gemm_refusals():
    """Documented preconditions that are refused, not served (VITMI_ERR_INVALID + a message, nothing
    launched, C untouched): a k-major bf16 operand over a reduction that is no multiple of 64 (so the
    4000-long split-K reduction exists for bf16 in the NN layout only); under gemm256 a C pitch that
    is no multiple of 8 or a C that is not 16-byte aligned; an ldc below N."""
    lib = _lib.lib()
    a, b = operands("bf16", "KK", 136, 136, 4032, False)
    ad, bd = a.to(DEV), b.to(DEV)

    def refused(pol, M, N, K, ak, bk, ldc, off, epi, cdt, what):
        lib.vitmi_gemm_set_policy(pol)
        try:
            C = rg.padded(M, N, max(ldc, N), cdt, "guard", offset=off).to(DEV)
            with kernel_stats() as st:
                rc = lib.vitmi_gemm(1, ak, bk, M, N, K, ad.ptr(), ad.pitch, bd.ptr(), bd.pitch, C.ptr(), ldc, CODE[cdt],
                                    epi, None, None, 0, None, 0, None, 0, stream())
            torch.cuda.synchronize()
            assert rc == 1 and lib.vitmi_last_error(), (what, rc)
            assert not st.k and rg.guards_intact(C), what
            assert what in lib.vitmi_last_error().decode(), (what, lib.vitmi_last_error())
        finally:
            lib.vitmi_gemm_set_policy(0)

    for ak, bk in ((1, 1), (1, 0), (0, 1)):
        refused(1, 136, 136, 4000, ak, bk, 136, 0, EPI["accum"], F32, "K % 64 == 0")
    refused(2, 136, 136, 128, 1, 1, 136 + 4, 0, EPI["store"], BF, "16-byte aligned C/aux/residual rows")
    refused(2, 136, 136, 128, 1, 1, 136 + 8, 1, EPI["store"], BF, "16-byte aligned C/aux/residual rows")
    refused(1, 136, 136, 128, 1, 1, 128, 0, EPI["store"], BF, "ldc too small")
