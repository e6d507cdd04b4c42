"""Which attention kernel runs, on the MI355X: every kernel policy x operand type x the sequence
lengths at the edges of every host-side decision of csrc/attention.hip (the 32-row wave count, the
NWC = 7 specialisations for N in (192, 224], the single-pass backward's limit 224, SEQ_MAX = 256).

Every case asserts
  (a) the set of attention kernels recorded (vitmi_stats_*) by one forward and one backward with bias
      gradient, and their call counts,
  (b) the flops and bytes recorded for each, against the formulas written out below,
  (c) the outputs against the fp32 reference of test_gpu_ops.test_attention_fwd_bwd at that test's
      tolerances, and every column c of the bias gradient against the column sums of the returned
      g = dqkv: |dbias_c - sum_r g[r,c]| <= (2^-8 + n 2^-24) sum_r |g[r,c]|, n = B N.  For bf16 the
      2^-8 is twice the half-ulp with which each summand was rounded to bf16 (the kernels may sum the
      fp32 values before that rounding); n 2^-24 bounds the fp32 summation.  fp32 drops the 2^-8.  A
      wrong count of partial rows misses or adds whole rows: orders above this bound."""
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

from kstats import kernel_stats  # noqa: E402
from vitmi import ops  # noqa: E402
from vitmi._lib import lib  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
B, H, DH = 2, 2, 64
D = H * DH
SCALE = 64 ** -0.5
SEQ_MAX, FUSED_NMAX = 256, 224
POLICIES = (0, 1, 2, 3)
NS = (1, 32, 33, 192, 193, 224, 225, 256, 257)
VITMI_ERR_INVALID = 1


def cdiv(a, b):
    return (a + b - 1) // b


def kname(base, *targs):
    """The kernel's name as recorded: mangled (base + I Li<a>E... E) or demangled (base<a, b>)."""
    if not targs:
        return (base,)
    return (base + "I" + "".join(f"Li{a}E" for a in targs) + "E", base + "<" + ", ".join(map(str, targs)) + ">")


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1.0)).item()


# ---------------------------------------------------------------- the dispatch, as documented
def work(T, N):
    """(forward, one kernel of the two-kernel backward, single-pass backward) -> (calls, flops, bytes)."""
    es, bh = (2 if T == BF else 4), B * H
    t = bh * N * DH
    fwd = (1, 4.0 * bh * N * N * DH, t * 4 * es + bh * N * 4)     # QK^T, PV; q/k/v read, o + lse written
    two = (1, 4.0 * bh * N * N * DH, t * 6 * es + bh * N * 8)     # each of dQ and dK/dV
    one = (1, 8.0 * bh * N * N * DH, t * 8 * 2 + bh * N * 8)      # dP, dQ, dV, dK in one pass
    return fwd, two, one


def expected(pol, T, N):
    """{kernel name forms: (calls, flops, bytes)} of one forward + one backward."""
    fwd, two, one = work(T, N)
    nkb = cdiv(N, 32)
    seq = N <= SEQ_MAX and pol != 1
    if T == F32:
        if seq:
            return {kname("attn_fwd_seq_f32", SEQ_MAX): fwd, kname("attn_bwd_dq_seq_f32", SEQ_MAX): two,
                    kname("attn_bwd_dkv_seq_f32", SEQ_MAX): two}
        return {kname("attn_fwd_f32"): fwd}                     # the streamed fp32 backward records nothing
    if not seq:
        return {kname("attn_fwd_bf16"): fwd, kname("attn_bwd_dq_bf16"): two, kname("attn_bwd_dkv_bf16"): two}
    q64 = pol != 2
    e = {kname("attn_fwd_seq64_bf16" if q64 else "attn_fwd_seq_bf16", SEQ_MAX, 0): fwd}
    if pol == 0 and N <= FUSED_NMAX:
        e[kname("attn_bwd_fused_seq_bf16", nkb)] = one
        return e
    nwc = 7 if nkb == 7 else 0                                  # N in (192, 224]
    if q64 and nwc:
        e[kname("attn_bwd_dq_seq64_bf16", SEQ_MAX, 7)] = two
    else:
        e[kname("attn_bwd_dq_seq_bf16", SEQ_MAX, nwc)] = two
    e[kname("attn_bwd_dkv_seq_bf16", SEQ_MAX, nwc)] = two
    return e


def assert_recorded(st, exp, what):
    got = {n: w for n, w in st.work.items() if "attn_" in n}
    print(f"{what}: {got}")
    for forms, w in exp.items():
        hits = [n for n in got if any(f in n for f in forms)]
        assert len(hits) == 1, (what, forms, got)
        assert got.pop(hits[0]) == w, (what, forms, w)
    assert not got, (what, "not expected", got)


# ---------------------------------------------------------------- inputs and the fp32 reference, built once
def rnd(*shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def attn_ref(qkv, N):
    q, k, v = qkv.float().view(B, N, 3, H, DH).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * SCALE
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * N, D)
    return o, torch.logsumexp(s, -1).reshape(B * H, N)


@lru_cache(maxsize=None)
def problem(T, N):
    qkv, do = rnd(B * N, 3 * D, dtype=T, seed=22), rnd(B * N, D, dtype=T, seed=23)
    o_ref, lse_ref = attn_ref(qkv, N)
    qq = qkv.float().clone().requires_grad_()
    attn_ref(qq, N)[0].backward(do.float())
    return qkv.to(DEV), do.to(DEV), o_ref, lse_ref, qq.grad.view(B * N, 3, D)


# ---------------------------------------------------------------- the tests
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("T", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("pol", POLICIES)
def test_attention_dispatch(pol, T, N):
    qkv, do, o_ref, lse_ref, g_ref = problem(T, N)
    db = torch.zeros(3 * D, device=DEV)
    try:
        ops.attention_set_policy(pol)
        with kernel_stats() as st:
            o, lse = ops.attention_fwd(qkv, B, N, H, SCALE)
            dqkv = ops.attention_bwd(qkv, o, do, lse, B, N, H, SCALE, bias_grad=db)
        torch.cuda.synchronize()
    finally:
        ops.attention_set_policy(0)
    what = f"policy {pol} {'bf16' if T == BF else 'f32'} N {N}"
    assert_recorded(st, expected(pol, T, N), what)                      # (a), (b)
    assert rel(o.float(), o_ref) < (1e-2 if T == BF else 1e-5)          # (c)
    assert rel(lse, lse_ref) < 1e-5
    d = dqkv.float().cpu().view(B * N, 3, D)
    for i, name in enumerate("qkv"):
        assert rel(d[:, i], g_ref[:, i]) < (2e-2 if T == BF else 1e-5), name
    g = dqkv.double().cpu()
    err = (db.double().cpu() - g.sum(0)).abs()
    bound = ((2.0 ** -8 if T == BF else 0.0) + B * N * 2.0 ** -24) * g.abs().sum(0)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: bias gradient worst |err|/bound {worst:.3g}")
    assert (err <= bound).all(), (what, worst)


@pytest.mark.parametrize("N", [n for n in NS if n <= SEQ_MAX])
@pytest.mark.parametrize("pol", POLICIES)
def test_attention_fwd_knob_dispatch(pol, N):
    """vitmi_attention_fwd_x3 (XM = 1) and _f8 (XM = 2) exist only as whole-sequence kernels: the
    64-query form unless the policy is 2 (policy 1 does not apply), with the split output's bytes."""
    qkv, _, o_ref, lse_ref, _ = problem(BF, N)
    bh = B * H
    fl = 4.0 * bh * N * N * DH
    try:
        ops.attention_set_policy(pol)
        with kernel_stats() as st:
            o, o3, lse = ops.attention_fwd_x3(qkv, B, N, H, SCALE)
            o_8, o8, lse_8 = ops.attention_fwd_f8(qkv, B, N, H, SCALE)
        torch.cuda.synchronize()
    finally:
        ops.attention_set_policy(0)
    base = "attn_fwd_seq_bf16" if pol == 2 else "attn_fwd_seq64_bf16"
    assert_recorded(st, {kname(base, SEQ_MAX, 1): (1, fl, bh * N * DH * 2 * (3 + 1 + 3) + bh * N * 4),
                         kname(base, SEQ_MAX, 2): (1, fl, bh * N * DH * 2 * (3 + 1 + 2) + bh * N * 4)},
                    f"x3/f8 policy {pol} N {N}")
    for oo, ll in ((o, lse), (o_8, lse_8)):
        assert rel(oo.float(), o_ref) < 1e-2
        assert rel(ll, lse_ref) < 1e-5


@pytest.mark.parametrize("pol", POLICIES)
def test_attention_fwd_knob_refuses_long_sequence(pol):
    N = SEQ_MAX + 1
    qkv = problem(BF, N)[0]
    o = torch.empty(B * N, D, dtype=BF, device=DEV)
    ox = torch.empty(B * N, 3 * D, dtype=BF, device=DEV)
    lse = torch.empty(B * H, N, device=DEV)
    p, s = ops._p, ops._s()
    try:
        ops.attention_set_policy(pol)
        with kernel_stats() as st:
            assert lib().vitmi_attention_fwd_x3(B, N, H, DH, SCALE, p(qkv), p(o), p(ox), p(lse), s) == VITMI_ERR_INVALID
            assert lib().vitmi_attention_fwd_f8(B, N, H, DH, SCALE, p(qkv), p(o), p(ox), p(lse), s) == VITMI_ERR_INVALID
    finally:
        ops.attention_set_policy(0)
    assert not st.work, st.work
