"""The BatchNorm-input-free backward of conv3 + bn3 (csrc/pfr_bnfree.hip) on the CPU: the algebra of the file's header against fp64 autograd,
and an fp32 torch emulation of pfr_bn3_bwd_coef / pfr_bn3_bwd_weights against the a-priori error bounds that tests/test_bnfree_gpu.py
holds the kernels to.  The references, the bounds, the input makers and the checks live here; the GPU file imports them, so the kernels
and the emulation face the same inputs and the same assertions.

Error criterion.  A fp32 sum of n terms, in any order, with or without fma, is off by at most (n + 2) u Σ|term| to first order, u = 2⁻²⁴.
The references compute each value and the sum of the absolute values of the same terms in fp64; the per-element tolerance is
bnfree_bounds(n, abs_sum) = 2 (n + 2) u abs_sum — the factor 2 covers the second-order terms and the rounded sub-expressions zsum / M and
dβ z̄ — with n the longest chain: nparts for dβ, K + nparts for dγ, K + 3 for dW, C for S, C + K for bias.  Derived, not measured: it
follows the conditioning of every element (about 1e-5 relative for a post-ReLU Z); a wrong term misses it by orders of magnitude.
dW, dγ, dβ also meet the project's relative-L2 bound for fp32-accumulated parameter gradients, TOL_G = 1e-4 (tests/test_dwconvk_gpu.py)."""
import functools

import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24
TOL_G = 1e-4
EPS = 1e-5
F64 = torch.float64

COEF_CASES = [(8, 64, 1), (6, 40, 63), (256, 64, 64), (512, 128, 65), (1024, 256, 196)]      # (C, K, nparts)
WEIGHT_CASES = [(8, 64), (256, 64), (512, 128), (1024, 256), (6, 128)]                       # (C, K)
CHAIN_CASES = [(2, 56, 256, 64), (3, 28, 512, 128), (1, 9, 256, 64), (2, 57, 256, 64)]       # (N, H, C, K)
WDTYPES = [torch.bfloat16, torch.float32]
WIDS = ["bf16", "f32"]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def bnfree_bounds(n, abs_sum):
    """the a-priori bound of a fp32 sum of n terms whose absolute values add up to abs_sum"""
    return 2.0 * (n + 2) * U * abs_sum


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_problem(M, C, K, seed, zdtype=None, wdtype=None, gdtype=None):
    """fp64 Z = relu(randn·A + 0.5) [M][K], W [C][K], γ of both signs, β, and G = mask ∘ (randn + 0.5 x̂ + 0.3) [M][C]: the correlation with
    x̂ and the offset make dγ and dβ of order M, so every term of the formulas matters.  Z, W, G are rounded to their storage dtypes (Z and
    W before x̂ is formed from them)."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(K, K, generator=g, dtype=F64) / K ** 0.5
    Z = torch.relu(torch.randn(M, K, generator=g, dtype=F64) @ A + 0.5)
    W = torch.randn(C, K, generator=g, dtype=F64) / K ** 0.5
    if zdtype is not None:
        Z = Z.to(zdtype).double()
    if wdtype is not None:
        W = W.to(wdtype).double()
    sign = torch.randint(0, 2, (C,), generator=g).double() * 2 - 1
    gamma = ((0.5 + torch.rand(C, generator=g, dtype=F64)) * sign).float().double()
    beta = (0.1 * torch.randn(C, generator=g, dtype=F64)).float().double()
    x = Z @ W.t()
    xhat = (x - x.mean(0)) * (x.var(0, unbiased=False) + EPS).rsqrt()
    mask = (torch.rand(M, C, generator=g) > 0.5).double()
    G = mask * (torch.randn(M, C, generator=g, dtype=F64) + 0.5 * xhat + 0.3)
    if gdtype is not None:
        G = G.to(gdtype).double()
    return dict(Z=Z, W=W, gamma=gamma, beta=beta, G=G, M=M, C=C, K=K)


def autograd_reference(p):
    """fp64 autograd of (G * batch_norm(Z Wᵀ, γ, β, eps = 1e-5)).sum()"""
    Z, W, gm, bt = (p[k].clone().requires_grad_() for k in ("Z", "W", "gamma", "beta"))
    y = F.batch_norm(Z @ W.t(), None, None, gm, bt, training=True, eps=EPS)
    dZ, dW, dg, db = torch.autograd.grad((p["G"] * y).sum(), (Z, W, gm, bt))
    return dict(dZ=dZ, dW=dW, dgamma=dg, dbeta=db)


def bnfree_reference(p):
    """the formulas of the header of csrc/pfr_bnfree.hip, evaluated in fp64 from G1 = GᵀZ, G2 = ZᵀZ and the column sums of Z"""
    Z, W, G, gm, M = p["Z"], p["W"], p["G"], p["gamma"], p["M"]
    G1, G2, zsum = G.t() @ Z, Z.t() @ Z, Z.sum(0)
    zb = zsum / M
    x = Z @ W.t()
    r = (x.var(0, unbiased=False) + EPS).rsqrt()
    db = G.sum(0)
    dg = r * (W * (G1 - db[:, None] * zb[None, :])).sum(1)
    A, B, C0 = gm * r, -gm * r * r * dg / M, -gm * r * db / M
    S = W.t() @ (B[:, None] * W)
    bias = C0 @ W - zb @ S
    dW = A[:, None] * G1 + B[:, None] * (W @ (G2 - M * zb[:, None] * zb[None, :])) + C0[:, None] * (M * zb)[None, :]
    main = G @ (A[:, None] * W)
    rest = Z @ S + bias
    return dict(dbeta=db, dgamma=dg, A=A, B=B, C0=C0, S=S, bias=bias, dW=dW, dZ=main + rest, dZ_rest=rest, invstd=r)


def _case_seed(*a):
    s = 17
    for v in a:
        s = s * 1009 + int(v)
    return s % (2 ** 31)


@functools.lru_cache(maxsize=None)
def coef_inputs(C, K, nparts, wdtype):
    """the fp32 inputs of pfr_bn3_bwd_coef: part [nparts][2][C] = per-row-group sums of G in row 0 and NaN in row 1 (it must not be read: the
    flag-2 producer leaves it meaningless), zsum and G1 of a real post-ReLU Z and G (the G1 − dβ z̄ cancellation is real), invstd in
    [0.5, 3], γ of both signs"""
    M = max(81, 8 * nparts + 3)
    p = make_problem(M, C, K, _case_seed(C, K, nparts), zdtype=torch.bfloat16, wdtype=wdtype, gdtype=torch.bfloat16)
    g = torch.Generator().manual_seed(_case_seed(C, K, nparts, 1))
    part = torch.full((nparts, 2, C), float("nan"))
    for t, rows in enumerate(torch.tensor_split(torch.arange(M), nparts)):
        part[t, 0] = p["G"][rows].sum(0).float()
    invstd = 0.5 + 2.5 * torch.rand(C, generator=g)
    return dict(part=part, G1=(p["G"].t() @ p["Z"]).float(), zsum=p["Z"].sum(0).float(), W=p["W"].to(wdtype), gamma=p["gamma"].float(),
                invstd=invstd, M=M, C=C, K=K, nparts=nparts)


@functools.lru_cache(maxsize=None)
def weights_inputs(C, K, wdtype):
    """the fp32 inputs of pfr_bn3_bwd_weights: G1, G2, zsum of a real Z and G, and SYNTHETIC coefficient rows (B and C0 of both signs), so
    that the errors of the first stage do not compound"""
    M = 777
    p = make_problem(M, C, K, _case_seed(C, K), zdtype=torch.bfloat16, wdtype=wdtype, gdtype=torch.bfloat16)
    g = torch.Generator().manual_seed(_case_seed(C, K, 2))
    coef = torch.randn(3, C, generator=g) * torch.tensor([1.0, 0.3, 0.2])[:, None]
    assert (coef[1] > 0).any() and (coef[1] < 0).any() and (coef[2] > 0).any() and (coef[2] < 0).any()
    return dict(coef=coef, G1=(p["G"].t() @ p["Z"]).float(), G2=(p["Z"].t() @ p["Z"]).float(), zsum=p["Z"].sum(0).float(),
                W=p["W"].to(wdtype), M=M, C=C, K=K)


@functools.lru_cache(maxsize=None)
def chain_inputs(N, H, C, K):
    """bf16 Z, W, G of one conv3 + bn3, fp64 autograd on those rounded values, and the error of the MATERIALISED form (fp64 arithmetic with
    bf16 rounding of x = Z Wᵀ, of dx and of dZ = dx W) against it"""
    M = N * H * H
    p = make_problem(M, C, K, _case_seed(N, H, C, K), zdtype=torch.bfloat16, wdtype=torch.bfloat16, gdtype=torch.bfloat16)
    ref = autograd_reference(p)
    bf = lambda t: t.bfloat16().double()
    x = bf(p["Z"] @ p["W"].t())
    mu, r = x.mean(0), (x.var(0, unbiased=False) + EPS).rsqrt()
    xh = (x - mu) * r
    db, dg = p["G"].sum(0), (p["G"] * xh).sum(0)
    dx = bf(p["gamma"] * r * (p["G"] - db / M - xh * dg / M))
    dZ_mat = bf(dx @ p["W"])
    return dict(p=p, ref=ref, err_mat=rel(dZ_mat, ref["dZ"]), gabs=p["G"].abs().sum(0))


# ---------------------------------------------------------------------------------------------------------------- fp64 references of the two kernels
def coef_reference(inp):
    """fp64 values of pfr_bn3_bwd_coef on its (fp32 / bf16) inputs, and the a-priori tolerance of each"""
    C, K, M, nparts = inp["C"], inp["K"], inp["M"], inp["nparts"]
    p0 = inp["part"][:, 0].double()
    G1, zb, W, gm, r = inp["G1"].double(), inp["zsum"].double() / M, inp["W"].double(), inp["gamma"].double(), inp["invstd"].double()
    db, db_abs = p0.sum(0), p0.abs().sum(0)
    dg = r * (W * (G1 - db[:, None] * zb[None, :])).sum(1)
    dg_abs = r.abs() * (W.abs() * (G1.abs() + db_abs[:, None] * zb.abs()[None, :])).sum(1)
    tol_db, tol_dg = bnfree_bounds(nparts, db_abs), bnfree_bounds(K + nparts, dg_abs)
    c0, c1, c2 = gm * r, -gm * r * r * dg / M, -gm * r * db / M
    val = dict(dbeta=db, dgamma=dg, coef0=c0, coef1=c1, coef2=c2)
    tol = dict(dbeta=tol_db, dgamma=tol_dg, coef0=4 * U * c0.abs(), coef1=tol_dg * (gm * r * r / M).abs() + 4 * U * c1.abs(),
               coef2=tol_db * (gm * r / M).abs() + 4 * U * c2.abs())
    return val, tol


def weights_reference(inp, S_stored):
    """fp64 values of pfr_bn3_bwd_weights on its inputs, and the a-priori tolerance of each.  bias is the documented contract: built from
    the S the kernel STORED (rounded to bf16), so that its two terms cancel as (Z − z̄) S does.  S_stored [K][K] as read back."""
    C, K, M = inp["C"], inp["K"], inp["M"]
    A, B, C0 = inp["coef"].double()
    G1, G2, zs, W = inp["G1"].double(), inp["G2"].double(), inp["zsum"].double(), inp["W"].double()
    zb = zs / M
    cov, cov_abs = G2 - zs[:, None] * zb[None, :], G2.abs() + (zs[:, None] * zb[None, :]).abs()
    dW = A[:, None] * G1 + B[:, None] * (W @ cov) + C0[:, None] * zs[None, :]
    dW_abs = (A[:, None] * G1).abs() + B.abs()[:, None] * (W.abs() @ cov_abs) + (C0[:, None] * zs[None, :]).abs()
    S = W.t() @ (B[:, None] * W)
    S_abs = W.abs().t() @ (B.abs()[:, None] * W.abs())
    Ss = S_stored.double()
    bias = C0 @ W - zb @ Ss
    bias_abs = C0.abs() @ W.abs() + zb.abs() @ Ss.abs()
    wa_t = (inp["coef"][0].float()[:, None] * inp["W"].float()).bfloat16().t().contiguous()     # bf16(fp32(A_c W[c][k])), [K][C]
    val = dict(dW=dW, S=S, bias=bias, wa_t=wa_t)
    tol = dict(dW=bnfree_bounds(K + 3, dW_abs), S=2.0 ** -8 * S.abs() + bnfree_bounds(C, S_abs), bias=bnfree_bounds(C + K, bias_abs))
    return val, tol


def _worst(got, val, tol):
    """max over the elements of |got − val| / tol (≤ 1 passes); NaN / inf in `got` fail"""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), "non-finite output"
    return ((got - val).abs() / tol.clamp_min(1e-300)).max().item()


def check_coef(got, inp, label=""):
    """got: dbeta, dgamma [C], coef [3][C] of ONE non-accumulating call"""
    val, tol = coef_reference(inp)
    out = dict(dbeta=got["dbeta"], dgamma=got["dgamma"], coef0=got["coef"][0], coef1=got["coef"][1], coef2=got["coef"][2])
    w = {k: _worst(out[k], val[k], tol[k]) for k in val}
    l2 = {k: rel(out[k], val[k]) for k in ("dgamma", "dbeta")}
    print(label, "err/bound", {k: f"{v:.3f}" for k, v in w.items()}, "relL2", {k: f"{v:.1e}" for k, v in l2.items()})
    assert all(v <= 1.0 for v in w.values()), w
    assert all(v <= TOL_G for v in l2.values()), l2


def bf16_ulps(a, b):
    """|a − b| in units of the last place of bf16, elementwise (same-sign neighbours)"""
    return (a.cpu().contiguous().view(torch.int16).int() - b.cpu().contiguous().view(torch.int16).int()).abs()


def check_weights(got, inp, label=""):
    """got: dW [C][K] fp32, wa_t [K][C] bf16, S [K][K] bf16, bias [K] fp32 of ONE non-accumulating call -> elements of wa_t that are not
    bit-equal to bf16(fp32(A_c W[c][k]))"""
    val, tol = weights_reference(inp, got["S"].cpu())
    w = {k: _worst(got[k], val[k], tol[k]) for k in ("dW", "S", "bias")}
    l2 = rel(got["dW"], val["dW"])
    ulps = bf16_ulps(got["wa_t"], val["wa_t"])
    off = int((ulps != 0).sum())
    print(label, "err/bound", {k: f"{v:.3f}" for k, v in w.items()}, f"dW relL2 {l2:.1e}  wa_t: {off} of {ulps.numel()} not bit-equal")
    assert all(v <= 1.0 for v in w.values()), w
    assert l2 <= TOL_G, l2
    assert int(ulps.max()) <= 1
    return off


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation of the kernels
def emulate_coef(inp):
    """bn3_coef_kernel in fp32 torch, the expression order of the .hip file (torch's own summation order inside the sums)"""
    W, G1, zsum, gm, r = inp["W"].float(), inp["G1"], inp["zsum"], inp["gamma"], inp["invstd"]
    inv_m = torch.tensor(1.0) / torch.tensor(float(inp["M"]))
    db = inp["part"][:, 0].sum(0)
    t1 = (W * (G1 - db[:, None] * (zsum * inv_m)[None, :])).sum(1)
    dg = r * t1
    coef = torch.stack([gm * r, -gm * r * r * dg * inv_m, -gm * r * db * inv_m])
    assert all(t.dtype == torch.float32 for t in (db, dg, coef))
    return dict(dbeta=db, dgamma=dg, coef=coef)


def emulate_weights(inp):
    """bn3_weights_kernel in fp32 torch: bf16 rounding of wa_t and S, bias from the ROUNDED S"""
    W, G1, G2, zsum = inp["W"].float(), inp["G1"], inp["G2"], inp["zsum"]
    A, B, C0 = inp["coef"]
    inv_m = torch.tensor(1.0) / torch.tensor(float(inp["M"]))
    zk = zsum * inv_m
    t = W @ (G2 - zsum[:, None] * zk[None, :])
    dW = A[:, None] * G1 + (B[:, None] * t + C0[:, None] * zsum[None, :])
    wa_t = (A[:, None] * W).bfloat16().t().contiguous()
    S = ((W * B[:, None]).t() @ W).bfloat16()
    bias = C0 @ W - zk @ S.float()
    assert dW.dtype == torch.float32 and bias.dtype == torch.float32
    return dict(dW=dW, wa_t=wa_t, S=S, bias=bias)


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("mck", [(81, 8, 64), (2352, 512, 128)], ids=lambda s: "x".join(map(str, s)))
def test_header_formulas_equal_fp64_autograd(mck):
    """dβ, dγ, A, B, C0, S, bias, dW and dZ = G (A∘W) + Z S + bias from G1, G2 and the column sums alone equal fp64 autograd to 1e-9, and the
    Z S + bias part is a third of dZ or more: a wrong S or bias could not hide behind the G (A∘W) term"""
    p = make_problem(*mck, seed=_case_seed(*mck))
    ref, f = autograd_reference(p), bnfree_reference(p)
    e = {k: rel(f[k], ref[k]) for k in ("dZ", "dW", "dgamma", "dbeta")}
    share = (f["dZ_rest"].norm() / ref["dZ"].norm()).item()
    print(mck, {k: f"{v:.1e}" for k, v in e.items()}, f"|Z S + bias| / |dZ| = {share:.2f}", "mean |dgamma|, |dbeta| / M",
          (ref["dgamma"].abs().mean() / p["M"]).item(), (ref["dbeta"].abs().mean() / p["M"]).item())
    assert all(v <= 1e-9 for v in e.values()), e
    assert share >= 0.3, share


@pytest.mark.parametrize("wdtype", WDTYPES, ids=WIDS)
@pytest.mark.parametrize("ckn", COEF_CASES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_emulation_of_the_coefficient_kernel_meets_the_bounds(ckn, wdtype):
    inp = coef_inputs(*ckn, wdtype)
    assert torch.isnan(inp["part"][:, 1]).all() and (inp["gamma"] > 0).any() and (inp["gamma"] < 0).any()
    assert inp["invstd"].min() >= 0.5 and inp["invstd"].max() <= 3.0
    check_coef(emulate_coef(inp), inp, f"{ckn} {wdtype}")


@pytest.mark.parametrize("wdtype", WDTYPES, ids=WIDS)
@pytest.mark.parametrize("ck", WEIGHT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_emulation_of_the_weights_kernel_meets_the_bounds(ck, wdtype):
    inp = weights_inputs(*ck, wdtype)
    assert check_weights(emulate_weights(inp), inp, f"{ck} {wdtype}") == 0


def emulate_chain_dz(p):
    """the BatchNorm-input-free data gradient in fp64 arithmetic with the roundings of the HIP chain: bf16 wcat = [(A∘W)ᵀ | S], bias from the
    rounded S, bf16 output"""
    f = bnfree_reference(p)
    bf = lambda t: t.bfloat16().double()
    S = bf(f["S"])
    bias = f["C0"] @ p["W"] - (p["Z"].sum(0) / p["M"]) @ S
    return bf(p["G"] @ bf(f["A"][:, None] * p["W"]) + p["Z"] @ S + bias)


@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_roundings_of_the_chain_cost_no_more_than_the_materialised_form(case):
    """dZ of the BN-input-free form with its bf16 roundings (weights and output) against the materialised form with its own (x, dx and
    output), both in fp64 arithmetic, both against fp64 autograd: the criterion tests/test_bnfree_gpu.py puts to the kernels, ≤ 1.25×"""
    c = chain_inputs(*case)
    e = rel(emulate_chain_dz(c["p"]), c["ref"]["dZ"])
    print(case, f"input-free {e:.3e}  materialised {c['err_mat']:.3e}  ratio {e / c['err_mat']:.3f}")
    assert e <= 1.25 * c["err_mat"]
