"""csrc/pfr_bnfree.hip on the device, through the C-ABI: pfr_bn3_bwd_coef and pfr_bn3_bwd_weights against fp64 on the same fp32 / bf16
inputs with the a-priori bounds of tests/test_bnfree_host.py (references, bounds, inputs and checks are imported from there: the fp32
emulation on the CPU passes the very same assertions), and the chain as the engine issues it — Gram matrix, statistics, G1, coefficient
rows, weights, two-source data gradient — in bf16 against fp64 autograd of (G * batch_norm(Z Wᵀ)).sum() on the bf16-rounded operands.

Every output buffer starts as NaN with 64 sentinel elements behind it that must survive; every call sequence runs twice and must give the
same bits (fixed summation orders, no atomics)."""
import math

import pytest
import torch

from test_bnfree_host import (CHAIN_CASES, COEF_CASES, TOL_G, U, WDTYPES, WEIGHT_CASES, WIDS, chain_inputs, check_coef, check_weights,
                              coef_inputs, rel, weights_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 777.0
ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
P = lambda t: 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """an output buffer: NaN where the kernel writes, 64 sentinel elements behind it"""

    def __init__(self, *shape, dtype=torch.float32):
        self.n = math.prod(shape)
        self.buf = torch.empty(self.n + 64, dtype=dtype, device=DEV)
        self.t = self.buf[:self.n].view(shape)
        self.buf[self.n:] = SENTINEL
        self.refill()

    def refill(self):
        self.t.fill_(float("nan"))

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def _same_bits(a, b):
    """torch.equal that takes NaN for what it is: a bit pattern"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- A
def _coef_call(lib, d, inp, wid, o, accumulate, nparts=None, wdtype=None):
    lib.pfr_bn3_bwd_coef(P(d["part"]), inp["nparts"] if nparts is None else nparts, P(d["G1"]), P(d["zsum"]), P(d["W"]),
                         wid if wdtype is None else wdtype, P(d["gamma"]), P(d["invstd"]), inp["C"], inp["K"], float(inp["M"]),
                         o["dgamma"].ptr(), o["dbeta"].ptr(), o["coef"].ptr(), accumulate, _stream())


@pytest.mark.parametrize("wdtype", WDTYPES, ids=WIDS)
@pytest.mark.parametrize("ckn", COEF_CASES, **ids)
def test_bn3_bwd_coef_against_fp64(ckn, wdtype):
    """dβ, dγ and the coefficient rows A = γr, B = −γr²dγ/M, C0 = −γr dβ/M, (C, K, nparts) with C no multiple of the 4 waves of a block, K
    below one wave and nparts on either side of the 64-lane stride; bf16 and fp32 weights; row 1 of the partials is NaN and must not be
    read.  accumulate = 0 into NaN gives finite values, accumulate = 1 afterwards twice those; coef is overwritten in both modes."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    C, K, nparts = ckn
    inp = coef_inputs(C, K, nparts, wdtype)
    d = {k: inp[k].to(DEV).contiguous() for k in ("part", "G1", "zsum", "W", "gamma", "invstd")}
    runs = []
    for _ in range(2):
        o = dict(dgamma=Out(C), dbeta=Out(C), coef=Out(3, C))
        _coef_call(lib, d, inp, dtype_id(wdtype), o, 0)
        torch.cuda.synchronize()
        once = {k: v.buf.clone() for k, v in o.items()}
        o["coef"].refill()
        _coef_call(lib, d, inp, dtype_id(wdtype), o, 1)
        torch.cuda.synchronize()
        assert all(v.intact() for v in o.values())
        runs.append((once, {k: v.buf.clone() for k, v in o.items()}))
    for a, b in zip(runs[0], runs[1]):
        assert all(_same_bits(a[k], b[k]) for k in a)
    once, twice = ({k: v[:-64].cpu() for k, v in r.items()} for r in runs[0])
    check_coef(dict(dbeta=once["dbeta"], dgamma=once["dgamma"], coef=once["coef"].view(3, C)), inp, f"{ckn} {wdtype}")
    for k in ("dgamma", "dbeta"):
        assert bool(((twice[k].double() - 2 * once[k].double()).abs() <= 2 * U * (2 * once[k].double()).abs()).all()), k
    assert torch.equal(twice["coef"], once["coef"])


def test_bn3_bwd_coef_refuses_bad_arguments():
    """nparts = 0 and a weight dtype that is neither bf16 nor fp32 raise, and nothing is launched: the buffers keep their fill"""
    from pets_face_recognition_amd._hip import lib, PfrError
    C, K, nparts = COEF_CASES[0]
    inp = coef_inputs(C, K, nparts, torch.float32)
    d = {k: inp[k].to(DEV).contiguous() for k in ("part", "G1", "zsum", "W", "gamma", "invstd")}
    o = dict(dgamma=Out(C), dbeta=Out(C), coef=Out(3, C))
    with pytest.raises(PfrError):
        _coef_call(lib, d, inp, 0, o, 0, nparts=0)
    with pytest.raises(PfrError):
        _coef_call(lib, d, inp, 0, o, 0, wdtype=2)
    torch.cuda.synchronize()
    assert all(v.untouched() for v in o.values())


# ---------------------------------------------------------------------------------------------------------------- B
def _weights_call(lib, d, inp, wid, dW, wa_t, S, bias, accumulate, K=None):
    lib.pfr_bn3_bwd_weights(P(d["coef"]), P(d["G1"]), P(d["G2"]), P(d["zsum"]), P(d["W"]), wid, inp["C"], inp["K"] if K is None else K,
                            float(inp["M"]), dW.ptr(), wa_t.ptr(), 0 if S is None else S.ptr(), bias.ptr(), accumulate, _stream())


@pytest.mark.parametrize("wdtype", WDTYPES, ids=WIDS)
@pytest.mark.parametrize("ck", WEIGHT_CASES, **ids)
def test_bn3_bwd_weights_against_fp64(ck, wdtype):
    """dW (a-priori bound and 1e-4 in L2), the data-gradient weights wa_t[k][c] = bf16(fp32(A_c W[c][k])), S = Wᵀ diag(B) W in bf16, and
    bias_k = Σ_c C0_c W[c][k] − Σ_j z̄_j S[j][k] from the S the kernel stored, with synthetic coefficient rows (B, C0 of both signs), in
    both output layouts — separate wa_t [K][C] + S [K][K], and S = NULL: wcat [K][C + K], row k = [A∘W column k | S row k] — which must
    hold the same bits; accumulate = 1 doubles dW and overwrites the rest.
    wa_t observed on the MI355X: bit-equal to the fp32 product rounded once (0 elements differ in every case, both weight dtypes); one
    bf16 unit in the last place is what the test allows."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    C, K = ck
    inp = weights_inputs(C, K, wdtype)
    d = {k: inp[k].to(DEV).contiguous() for k in ("coef", "G1", "G2", "zsum", "W")}
    wid, bf = dtype_id(wdtype), torch.bfloat16
    runs = []
    for _ in range(2):
        sep = dict(dW=Out(C, K), wa_t=Out(K, C, dtype=bf), S=Out(K, K, dtype=bf), bias=Out(K))
        cat = dict(dW=Out(C, K), wcat=Out(K, C + K, dtype=bf), bias=Out(K))
        _weights_call(lib, d, inp, wid, sep["dW"], sep["wa_t"], sep["S"], sep["bias"], 0)
        _weights_call(lib, d, inp, wid, cat["dW"], cat["wcat"], None, cat["bias"], 0)
        torch.cuda.synchronize()
        once = {k: v.buf.clone() for k, v in sep.items()}
        for k in ("wa_t", "S", "bias"):
            sep[k].refill()
        _weights_call(lib, d, inp, wid, sep["dW"], sep["wa_t"], sep["S"], sep["bias"], 1)
        torch.cuda.synchronize()
        assert all(v.intact() for v in sep.values()) and all(v.intact() for v in cat.values())
        runs.append((once, {k: v.buf.clone() for k, v in sep.items()}, {k: v.buf.clone() for k, v in cat.items()}))
    for a, b in zip(runs[0], runs[1]):
        assert all(_same_bits(a[k], b[k]) for k in a)
    once, twice, cat = ({k: v[:-64].cpu() for k, v in r.items()} for r in runs[0])
    got = dict(dW=once["dW"].view(C, K), wa_t=once["wa_t"].view(K, C), S=once["S"].view(K, K), bias=once["bias"])
    off = check_weights(got, inp, f"{ck} {wdtype}")
    print(f"wa_t elements not bit-equal to bf16(fp32(A W)): {off}")
    wcat = cat["wcat"].view(K, C + K)
    assert _same_bits(wcat[:, :C], got["wa_t"]) and _same_bits(wcat[:, C:], got["S"])
    assert _same_bits(cat["dW"], once["dW"]) and _same_bits(cat["bias"], once["bias"])
    assert bool(((twice["dW"].double() - 2 * once["dW"].double()).abs() <= 2 * U * (2 * once["dW"].double()).abs()).all())
    assert all(_same_bits(twice[k], once[k]) for k in ("wa_t", "S", "bias"))


def test_bn3_bwd_weights_refuses_k_96():
    """K must be 64, 128 or 256 (the S blocks index with K − 1 as a mask): K = 96 raises and launches nothing"""
    from pets_face_recognition_amd._hip import lib, PfrError
    C, K = 8, 128
    inp = weights_inputs(C, K, torch.float32)
    d = {k: inp[k].to(DEV).contiguous() for k in ("coef", "G1", "G2", "zsum", "W")}
    bf = torch.bfloat16
    o = dict(dW=Out(C, K), wa_t=Out(K, C + K, dtype=bf), S=Out(K, K, dtype=bf), bias=Out(K))
    with pytest.raises(PfrError):
        _weights_call(lib, d, inp, 0, o["dW"], o["wa_t"], o["S"], o["bias"], 0, K=96)
    with pytest.raises(PfrError):
        _weights_call(lib, d, inp, 0, o["dW"], o["wa_t"], None, o["bias"], 0, K=96)
    torch.cuda.synchronize()
    assert all(v.untouched() for v in o.values())


# ---------------------------------------------------------------------------------------------------------------- C
def test_chain_cases_take_both_gram_branches():
    from pets_face_recognition_amd._hip import lib
    assert {lib.pfr_gram_ws_floats(N * H * H, K) > 0 for N, H, _, K in CHAIN_CASES} == {True, False}


def _run_chain(lib, N, H, C, K, Z, W, G, gamma, beta, part, bnx, bncoef):
    """one pass of the backward of conv3 + bn3 as FEEngine issues it -> the output buffers"""
    M, st, bf = N * H * H, _stream(), torch.bfloat16
    # 1. G2 = ZᵀZ and the column sums of Z: one streaming pass where the geometry has one, else weight-gradient GEMM + column sums
    gram = Out(K * K + K)
    nws = lib.pfr_gram_ws_floats(M, K)
    if nws > 0:
        ws = torch.empty(nws, dtype=torch.float32, device=DEV)
        lib.pfr_gram_colsum(P(Z), 1, M, K, gram.ptr(), P(ws), st)
    else:
        ws = torch.empty(max(1, lib.pfr_conv2d_wgrad_splits(M, K, K) * K * K), dtype=torch.float32, device=DEV)
        lib.pfr_conv2d_wgrad(P(Z), P(Z), gram.ptr(), P(ws), 1, N, H, H, K, K, 1, 1, 1, 0, H, H, K, 0, 0, 0, 1.0, 0, st)
        cws = torch.empty(max(1, lib.pfr_colsum_ws_floats(M, K)), dtype=torch.float32, device=DEV)
        lib.pfr_colsum(P(Z), 1, M, K, gram.t[K * K:].data_ptr(), 0, P(cws), st)
    zsum_ptr = gram.t[K * K:].data_ptr()
    # 2. invstd (and the rest of the forward coefficients) from the Gram matrix
    fin = Out(4, C)
    lib.pfr_bn_finalize_from_gram(gram.ptr(), P(W), 1, C, K, float(M), P(gamma), P(beta), 1e-5, 0.1, 0, 0, fin.t[0].data_ptr(),
                                  fin.t[1].data_ptr(), fin.t[2].data_ptr(), fin.t[3].data_ptr(), 0, st)
    # 3. G1 = GᵀZ
    G1 = Out(C, K)
    ws1 = torch.empty(max(1, lib.pfr_conv2d_wgrad_splits(M, C, K) * C * K), dtype=torch.float32, device=DEV)
    lib.pfr_conv2d_wgrad(P(Z), P(G), G1.ptr(), P(ws1), 1, N, H, H, K, C, 1, 1, 1, 0, H, H, C, 0, 0, 0, 1.0, 0, st)
    # 5. dβ, dγ, coefficient rows   6. dW, wcat = [(A∘W)ᵀ | S], bias   7. dZ = [G | Z] wcatᵀ + bias
    dgamma, dbeta, coef = Out(C), Out(C), Out(3, C)
    lib.pfr_bn3_bwd_coef(P(part), part.shape[0], G1.ptr(), zsum_ptr, P(W), 1, P(gamma), fin.t[1].data_ptr(), C, K, float(M), dgamma.ptr(),
                         dbeta.ptr(), coef.ptr(), 0, st)
    dW, wcat, bias = Out(C, K), Out(K, C + K, dtype=bf), Out(K)
    lib.pfr_bn3_bwd_weights(coef.ptr(), G1.ptr(), gram.ptr(), zsum_ptr, P(W), 1, C, K, float(M), dW.ptr(), wcat.ptr(), 0, bias.ptr(), 0, st)
    npart = lib.pfr_conv1x1_dgrad2_bn_parts(1, N, H, H, C, K, K)
    assert npart > 0
    dZ, part2 = Out(M, K, dtype=bf), Out(npart, 2, K)
    lib.pfr_conv1x1_dgrad2_bn(P(G), P(Z), wcat.ptr(), bias.ptr(), dZ.ptr(), 1, N, H, H, C, K, K, P(bnx), P(bncoef), part2.ptr(), st)
    torch.cuda.synchronize()
    return dict(gram=gram, fin=fin, G1=G1, dgamma=dgamma, dbeta=dbeta, coef=coef, dW=dW, wcat=wcat, bias=bias, dZ=dZ, part2=part2)


@pytest.mark.parametrize("case", CHAIN_CASES, **ids)
def test_bn_input_free_chain_against_fp64_autograd(case):
    """pfr_gram_colsum (or its fallback pfr_conv2d_wgrad(Z, Z) + pfr_colsum) → pfr_bn_finalize_from_gram → G1 = pfr_conv2d_wgrad(Z, G) →
    pfr_bn3_bwd_coef (7 partial rows of Σ G with a ragged last group, NaN in row 1) → pfr_bn3_bwd_weights (concatenated) →
    pfr_conv1x1_dgrad2_bn, bf16, under pfr_set_tuning("sconv", 2) / ("bnb", 2).  dβ to 1e-5 Σ|G| per channel, dγ and dW to 1e-4 in L2.
    dZ: its relative L2 error against fp64 autograd may be at most 1.25× that of the MATERIALISED form emulated on the CPU (fp64
    arithmetic, bf16 rounding of x, dx and dZ = dx W) — the two forms round at different points, hence the margin — and
    max |ΔdZ| ≤ 1e-2 max |dZ|.
    Relative L2 error of dZ, (this chain on the MI355X, materialised form): (2,56,256,64) (2.51e-03, 2.47e-03); (3,28,512,128) (2.48e-03,
    2.47e-03); (1,9,256,64) (2.58e-03, 2.56e-03); (2,57,256,64) (2.52e-03, 2.47e-03)."""
    from pets_face_recognition_amd._hip import lib
    N, H, C, K = case
    M = N * H * H
    c = chain_inputs(*case)
    p, ref = c["p"], c["ref"]
    bf = torch.bfloat16
    Z, W, G = (p[k].to(bf).to(DEV).contiguous() for k in ("Z", "W", "G"))
    assert torch.equal(Z.double().cpu(), p["Z"]) and torch.equal(G.double().cpu(), p["G"])      # the reference saw the same values
    gamma, beta = p["gamma"].float().to(DEV), p["beta"].float().to(DEV)
    rows = M // 7 + 1
    assert 0 < M - 6 * rows < rows
    part = torch.full((7, 2, C), float("nan"), device=DEV)
    for t in range(7):
        part[t, 0] = G[t * rows:(t + 1) * rows].float().sum(0)
    g = torch.Generator().manual_seed(M + K)
    # the BN that dZ feeds (bn2): input away from its ReLU threshold; its sums are checked by test_two_source_data_gradient_with_bn_sums
    bnx = ((0.5 + torch.rand(M, K, generator=g)) * (torch.randint(0, 2, (M, K), generator=g) * 2 - 1)).to(bf).to(DEV)
    bncoef = torch.stack([0.1 * torch.randn(K, generator=g), 1 + 0.1 * torch.rand(K, generator=g), 1 + 0.1 * torch.rand(K, generator=g),
                          0.2 * (torch.rand(K, generator=g) - 0.5)]).to(DEV)
    try:
        lib.pfr_set_tuning(b"sconv", 2)
        lib.pfr_set_tuning(b"bnb", 2)
        runs = [_run_chain(lib, N, H, C, K, Z, W, G, gamma, beta, part, bnx, bncoef) for _ in range(2)]
    finally:
        lib.pfr_set_tuning(b"sconv", 1)
        lib.pfr_set_tuning(b"bnb", 0)
    o = runs[0]
    for k, v in o.items():
        assert v.intact() and runs[1][k].intact(), k
        assert _same_bits(v.buf, runs[1][k].buf), k
        assert bool(torch.isfinite(v.t.float()).all()), k
    db, dg, dW, dZ = (o[k].t.double().cpu() for k in ("dbeta", "dgamma", "dW", "dZ"))
    e_db = ((db - ref["dbeta"]).abs() / c["gabs"]).max().item()
    e_dg, e_dW, e_dZ = rel(dg, ref["dgamma"]), rel(dW, ref["dW"]), rel(dZ, ref["dZ"])
    e_max = ((dZ - ref["dZ"]).abs().max() / ref["dZ"].abs().max()).item()
    print(case, f"gram pass {lib.pfr_gram_ws_floats(M, K) > 0}  dbeta {e_db:.2e}  dgamma {e_dg:.2e}  dW {e_dW:.2e}  "
          f"dZ {e_dZ:.3e} (materialised {c['err_mat']:.3e}, ratio {e_dZ / c['err_mat']:.3f})  max {e_max:.2e}")
    assert e_db <= 1e-5
    assert e_dg <= TOL_G and e_dW <= TOL_G
    assert e_dZ <= 1.25 * c["err_mat"]
    assert e_max <= 1e-2
