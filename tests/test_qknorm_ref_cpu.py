"""tests/ref_qknorm.py checked on the CPU: the float64 reference against F.layer_norm + autograd, the model
reference against oracle/vit_ref.py when QK-norm is off, the fp32 emulation of the kernels' arithmetic
inside the per-element bound for every family and shape of the GPU suite, and mutants that each leave it
(so the suite can fail)."""
import pytest
import torch
import torch.nn.functional as F

import ref_qknorm as ref
from oracle import vit_ref
from vitmi.config import ViTConfig

HS = (1, 2, 3, 5, 12, 16, 20, 32)
MS = (1, 3, 64, 394)
DH = ref.DH


def test_reference_is_layer_norm_and_autograd_in_float64():
    M, H = 7, 3
    D = H * DH
    inp, r = ref.reference("rows", M, H, False)
    qkv = inp["qkv"].double().requires_grad_()
    par = {k: inp[k].double().requires_grad_() for k in ("gq", "bq", "gk", "bk")}
    q = F.layer_norm(qkv[:, :D].reshape(M, H, DH), (DH,), par["gq"], par["bq"], ref.rl.f32_eps())
    k = F.layer_norm(qkv[:, D:2 * D].reshape(M, H, DH), (DH,), par["gk"], par["bk"], ref.rl.f32_eps())
    out = torch.cat([q.reshape(M, D), k.reshape(M, D), qkv[:, 2 * D:]], 1)
    out.backward(inp["dqkv"].double())
    assert (r["out"][0] - out[:, :2 * D].detach()).abs().max() < 1e-12
    # the backward is a function of the statistics rounded to fp32: equal to autograd up to that rounding
    prev = inp["prev"]
    for got, want in ((r["dqk"][0], qkv.grad[:, :2 * D]), (r["dgq"][0] - prev["dgq"], par["gq"].grad),
                      (r["dbq"][0] - prev["dbq"], par["bq"].grad), (r["dgk"][0] - prev["dgk"], par["gk"].grad),
                      (r["dbk"][0] - prev["dbk"], par["bk"].grad), (r["dbias"][0] - prev["dbias"], qkv.grad.sum(0))):
        assert vit_ref.rel_err(got, want) < 1e-6
    assert torch.equal(qkv.grad[:, 2 * D:], inp["dqkv"][:, 2 * D:].double())
    assert (r["out"][1] > 0).all() and (r["dqk"][1] > 0).all()


def test_bf16_bounds_carry_the_store_term():
    _, r32 = ref.reference("randn", 5, 2, False)
    _, r16 = ref.reference("randn", 5, 2, True)
    assert (r16["out"][1] >= ref.UBF * r16["out"][0].abs()).all()
    assert (r16["dqk"][1] >= ref.UBF * r16["dqk"][0].abs()).all()
    assert r32["out"][1].max() < 1e-4                      # the fp32 bound has no such term


def test_model_reference_without_qk_norm_is_vit_ref_bitwise():
    cfg = ViTConfig(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2, num_classes=2, dtype="fp32")
    params = vit_ref.init_params(cfg, seed=0)
    img, tgt = vit_ref.synthetic_batch(cfg, 3)
    l0, loss0, g0 = vit_ref.forward_backward(img, tgt, params, cfg)
    l1, loss1, g1 = ref.forward_backward(img, tgt, params, cfg)
    assert torch.equal(l0, l1) and torch.equal(loss0, loss1)
    assert set(g0) == set(g1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    # and with it on, the norm acts and its parameters have gradients (k_norm.bias: zero up to rounding)
    on = cfg.replace(qk_norm=True)
    p = dict(params)
    p.update(ref.model_norm_params(on))
    l2, _, g2 = ref.forward_backward(img, tgt, p, on)
    assert (l2 - l0).abs().max() > 1e-4
    assert set(g2) == set(p)
    for i in range(cfg.depth):
        kw, kb = g2[f"blocks.{i}.attn.k_norm.weight"], g2[f"blocks.{i}.attn.k_norm.bias"]
        assert kb.norm() < 1e-4 * kw.norm()


def test_bf16_emulation_is_near_the_reference():
    cfg = ViTConfig(img_size=32, patch_size=8, embed_dim=128, depth=2, num_heads=2, num_classes=2, dtype="fp32",
                    qk_norm=True)
    p = dict(vit_ref.init_params(cfg, seed=0))
    p.update(ref.model_norm_params(cfg))
    img, tgt = vit_ref.synthetic_batch(cfg, 3)
    l0, _, g0 = ref.forward_backward(img, tgt, p, cfg)
    l1, _, g1 = ref.forward_backward(img, tgt, p, cfg, emulate=True)
    lerr = vit_ref.rel_err(l1, l0)
    assert 1e-4 < lerr < 0.2, lerr                        # it rounds, and it is the same model
    assert all(vit_ref.rel_err(g1[k], g0[k]) < 0.2 for k in g0 if not k.endswith("k_norm.bias"))


def ratios(inp, r, H, bf16, mut_f=None, mut_b=None):
    """worst |got - ref| / tol of the emulated forward and backward, per output."""
    D = H * DH
    f = ref.emulate_fwd(inp, H, bf16, mut=mut_f)
    b = ref.emulate_bwd(inp, r["mean_in"], r["rstd_in"], H, bf16, mut=mut_b)
    out = {"out": ref.worst_ratio(f["out"][:, :2 * D], *r["out"]), "mean": ref.worst_ratio(f["mean"], *r["mean"]),
           "rstd": ref.worst_ratio(f["rstd"], *r["rstd"]), "dqk": ref.worst_ratio(b["dqkv"][:, :2 * D], *r["dqk"])}
    for k in ("dgq", "dbq", "dgk", "dbk", "dbias"):
        out[k] = ref.worst_ratio(b[k], *r[k])
    out["v"] = 0.0 if torch.equal(f["out"][:, 2 * D:], inp["qkv"][:, 2 * D:]) else float("inf")
    out["dv"] = 0.0 if torch.equal(b["dqkv"][:, 2 * D:], inp["dqkv"][:, 2 * D:]) else float("inf")
    return out, f, b


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H", HS)
def test_emulation_within_the_bound(H, bf16):
    worst = {}
    for M in MS:
        for fam in ref.FAMILIES:
            inp, r = ref.reference(fam, M, H, bf16)
            got, f, b = ratios(inp, r, H, bf16)
            for k, v in got.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(got.values()) <= 1.0, (fam, M, got)
            D = H * DH
            if fam == "const":
                for row in ref.const_heads(M, H):
                    m, h = divmod(row, H)
                    assert torch.equal(f["out"][m, h * DH:(h + 1) * DH], ref._store(inp["bq"], bf16))
                    assert torch.equal(f["out"][m, D + h * DH:D + (h + 1) * DH], ref._store(inp["bk"], bf16))
            if fam == "int":
                assert torch.equal(b["dbq"].double(), r["dbq"][0]) and torch.equal(b["dbk"].double(), r["dbk"][0])
                assert torch.equal(b["dbias"][2 * D:].double(), r["dbias"][0][2 * D:])
    print(f"H {H} {'bf16' if bf16 else 'fp32'}: worst ratios {({k: round(v, 3) for k, v in worst.items()})}")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_mutants_leave_the_bound(bf16):
    M, H = 64, 3
    D = H * DH
    inp, r = ref.reference("rows", M, H, bf16)
    base, _, _ = ratios(inp, r, H, bf16)
    assert max(base.values()) <= 1.0
    # the neighbouring head's statistics
    got, _, _ = ratios(inp, r, H, bf16, mut_f="nbrstats", mut_b="nbrstats")
    assert got["out"] > 1.0 and got["dqk"] > 1.0 and got["dgq"] > 1.0
    # k normalised with q's gamma: q stays right
    got, f, b = ratios(inp, r, H, bf16, mut_f="kgammaq", mut_b="kgammaq")
    assert got["out"] > 1.0 and got["dqk"] > 1.0
    assert ref.worst_ratio(f["out"][:, :D], r["out"][0][:, :D], r["out"][1][:, :D]) <= 1.0
    # the last row skipped: every sum shows it, the int family bitwise
    got, _, _ = ratios(inp, r, H, bf16, mut_b="droplast")
    assert got["dqk"] > 1.0 and got["dbias"] > 1.0 and got["dgq"] > 1.0 and got["dbq"] > 1.0
    inp_i, r_i = ref.reference("int", M, H, bf16)
    _, _, b = ratios(inp_i, r_i, H, bf16, mut_b="droplast")
    assert not torch.equal(b["dbk"].double(), r_i["dbk"][0])
    assert not torch.equal(b["dbias"][2 * D:].double(), r_i["dbias"][0][2 * D:])
    # v not copied
    got, _, _ = ratios(inp, r, H, bf16, mut_f="vnocopy")
    assert got["v"] == float("inf")
    # a truncating bf16 store
    if bf16:
        got, _, _ = ratios(inp, r, H, bf16, mut_f="trunc", mut_b="trunc")
        assert got["out"] > 1.0 and got["dqk"] > 1.0


def test_geometry_mirror():
    # a pass covers whole rows, at most the grid cap of 256-thread blocks unless one unit is larger
    for bf16 in (False, True):
        for H in range(1, 33):
            S = 3 * H * (8 if bf16 else 16)
            R = ref.rows_per_pass(10 ** 6, H, bf16)
            assert R * S % 256 == 0 and R * S // 256 <= max(ref.GRID_CAP, S)
            assert ref.rows_per_pass(1, H, bf16) * S % 256 == 0
