"""CPU checks of tests/token_oracle.py: (1) its float64 references equal torch float64 autograd; (2) its bounds are neither wrong nor
vacuous — a numpy fp32 restatement of each kernel's arithmetic (same passes, same polynomial) stays under them on every input set the GPU
file uses, and every planted defect exceeds them on at least one of those sets; (3) the input sets leave nothing out of the comparison.
This is the evidence that tests/test_token_kernels_gpu.py would fail on a subtly wrong kernel."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_oracle as O

F64, BF, F32 = torch.float64, torch.bfloat16, torch.float32
f32 = np.float32
RATIOS = {}


def note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["%-28s %.4f" % (k, v) for k, v in sorted(RATIOS.items())]
    print("\nfp32 restatement, worst err / bound:\n" + "\n".join(lines))
    out = os.environ.get("PFR_TOKEN_BOUNDS_OUT")
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------ fp32 restatements
def npf(t):
    return t.numpy().astype(f32)


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def stored(a, dtype):
    """fp32 array -> rounded to the output dtype -> float64 tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(dtype).to(F64)


def row_sum(a):
    """sum over axis 1 the way the kernels do: channel c on lane c % 64, serial over the lane's channels, then a 6-level fold"""
    R, C = a.shape
    per = (C + 63) // 64
    p = np.zeros((R, per * 64), f32)
    p[:, :C] = a
    s = np.cumsum(p.reshape(R, per, 64), axis=1, dtype=f32)[:, -1, :]
    w = 64
    while w > 1:
        w //= 2
        s = s[:, :w] + s[:, w:2 * w]
    return s[:, 0]


def col_sum(a):
    return np.cumsum(a, axis=0, dtype=f32)[-1]


def ln_fwd_f32(c, dtype, defect=None):
    x, gam, bet = npf(c["x"]), npf(c["gamma"]), npf(c["beta"])
    R, C = x.shape
    xs = x
    if defect == "drop_chunk":
        xs = x.copy()
        xs[:, C - O.kpack(dtype):] = 0
    invC = f32(1) / f32(C)
    mu = row_sum(xs) * invC
    with np.errstate(all="ignore"):
        if defect == "one_pass":
            var = row_sum(xs * xs) * invC - mu * mu
        else:
            d = xs - mu[:, None]
            if defect == "drop_chunk":
                d[:, C - O.kpack(dtype):] = 0
            var = row_sum(d * d) * (f32(1) / f32(max(C - 1, 1)) if defect == "c_minus_1" else invC)
        if defect == "eps_outside":
            rs = (f32(1) / np.sqrt(var)).astype(f32) + f32(O.EPS)
        else:
            rs = (f32(1) / np.sqrt(var + f32(O.EPS))).astype(f32)
        mu_y = np.roll(mu, -1) if defect == "next_row_mean" else mu
        y = fma((x - mu_y[:, None]) * rs[:, None], gam, bet)
    return mu, rs, y


def ln_bwd_f32(c, mu, rs, dtype, defect=None):
    x, gam, dy = npf(c["x"]), npf(c["gamma"]), npf(c["dy"])
    dres = npf(c["dres"]) if c["dres"] is not None else None
    C = x.shape[1]
    invC = f32(1) / f32(C)
    xh = (x - mu[:, None]) * rs[:, None]
    g = dy * gam
    a = (row_sum(g) * invC)[:, None]
    b = (row_sum(g * xh) * invC)[:, None]
    if defect == "dres_before_scale" and dres is not None:
        dx = rs[:, None] * (g - a - xh * b + dres)
    else:
        v = rs[:, None] * (g - a - xh * b)
        dx = v + dres if dres is not None else v
    dxs = stored(dx, dtype)
    dgam = col_sum(dy * (x if defect == "dgamma_with_x" else xh))
    return dxs, dgam, col_sum(dy), col_sum(npf(dxs))


def cdf_pdf_f32(z, defect=None):
    a = list(O.AS_A)
    if defect == "coefficient":
        a[4] = 1.061415429             # a5 = 1.061405429 altered in its sixth digit
    with np.errstate(all="ignore"):
        ax = np.abs(z) * f32(O.SQRT1_2)
        ex = np.exp(-(ax * ax)).astype(f32)
        t = (f32(1) / fma(f32(O.AS_P), ax, f32(1))).astype(f32)
        p = fma(f32(a[4]), t, f32(a[3]))
        for k in (2, 1, 0):
            p = fma(p, t, f32(a[k]))
        half = f32(0.5) * p * t * ex
        cdf = np.where(z >= 0, f32(1) - half, half).astype(f32)
        pdf = (f32(1.0 if defect == "pdf_factor" else O.INV_SQRT_2PI) * ex).astype(f32)
    return cdf, pdf


def gelu_fwd_f32(z, defect=None):
    with np.errstate(all="ignore"):
        if defect == "tanh":
            return (f32(0.5) * z * (f32(1) + np.tanh(f32(math.sqrt(2 / math.pi)) * (z + f32(0.044715) * z * z * z)))).astype(f32)
        return (z * cdf_pdf_f32(z, defect)[0]).astype(f32)


def gelu_bwd_f32(z, dy, defect=None):
    cdf, pdf = cdf_pdf_f32(z, defect)
    with np.errstate(all="ignore"):
        return (dy * (cdf + z * pdf)).astype(f32)


def gemm_act_f32(c, dtype, defect=None):
    """-> stored y2 (act 2) / the given one (act 3), stored y, the fp32 activation before its rounding"""
    if "acc32" in c:
        acc = c["acc32"]                                  # real-valued set: the fp32 accumulator
    else:
        acc = npf(c["lin"])                               # exact: every order gives it
    if c["act"] == 2:
        pre = (npf(stored(acc, dtype)) + npf(c["bias"])).astype(f32)
        y2 = stored(pre, dtype)
        y = gelu_fwd_f32(pre if defect == "unrounded_y2" else npf(y2))
    else:
        y2 = c["y2"]
        z = npf(y2)
        if defect == "neighbour_row":
            z = np.roll(z, -1, axis=0)
        y = gelu_bwd_f32(z, npf(stored(acc, dtype)))
    return y2, stored(y, dtype), y


def tile_stats_f32(vals, mt, defect=None):
    """vals: fp32 [M][N] the values the statistics see -> mean [T][N], M2 [T][N]"""
    M = vals.shape[0]
    mean, m2 = [], []
    for t0 in range(0, M, mt):
        blk = vals[t0:t0 + mt]
        n = f32(blk.shape[0])
        k = blk[0]
        d = blk - k
        s1, s2 = col_sum(d), col_sum(d * d)
        mean.append(k + s1 / n)
        m2.append(col_sum(blk * blk) if defect == "m2_about_zero" else s2 - s1 * s1 / n)
    return np.stack(mean), np.stack(m2)


# ------------------------------------------------------------------------------------------------ the GPU file's input sets
def ln_sets():
    for dtype in (F32, BF):
        for C in O.ln_widths(dtype):
            g = O.ln_geom(C, dtype)
            rbs = (4, 6, 8) if g is not None and g[1] == 1 else (4,)
            for rows in sorted({r for rb in rbs for r in O.ln_row_counts(C, dtype, rb)}):
                for use_res in (0, 1):
                    yield rows, C, dtype, use_res
        yield O.LN_MANY_ROWS, O.kpack(dtype), dtype, 1


def ln_ratios(c, dtype, fwd_defect=None, bwd_defect=None):
    """worst err / bound of the restatement over y, mean, rstd, dx, dgamma, dbeta, dxsum"""
    mu, rs, y = ln_fwd_f32(c, dtype, fwd_defect)
    m_ref, _, r_ref, y_ref = O.ln_fwd_ref(c["x"], c["gamma"], c["beta"], O.EPS)
    b_m, b_r, b_y = O.ln_fwd_bounds(c["x"], c["gamma"], c["beta"], O.EPS, dtype)
    out = {"y": O.worst_ratio(stored(y, dtype), y_ref, b_y), "mean": O.worst_ratio(stored(mu, F32), m_ref, b_m),
           "rstd": O.worst_ratio(stored(rs, F32), r_ref, b_r)}
    if fwd_defect is None:
        mu64, rs64 = stored(mu, F32), stored(rs, F32)
        dxs, dg, db, dxsum = ln_bwd_f32(c, mu, rs, dtype, bwd_defect)
        ref = O.ln_bwd_ref(c["dy"], c["x"], mu64, rs64, c["gamma"], c["dres"])
        b_dx, b_dg, b_db = O.ln_bwd_bounds(c["dy"], c["x"], mu64, rs64, c["gamma"], c["dres"], dtype)
        out.update(dx=O.worst_ratio(dxs, ref["dx"], b_dx), dgamma=O.worst_ratio(stored(dg, F32), ref["dgamma"], b_dg),
                   dbeta=O.worst_ratio(stored(db, F32), ref["dbeta"], b_db),
                   dxsum=O.worst_ratio(stored(dxsum, F32), dxs.sum(0), O.colsum_bound(dxs)))
    return out


# ------------------------------------------------------------------------------------------------ (1) the oracle is the definition
def test_oracle_equals_torch_float64_autograd():
    g = O.rng("autograd")
    x = torch.randn(37, 52, generator=g, dtype=F64, requires_grad=True)
    gam = torch.randn(52, generator=g, dtype=F64, requires_grad=True)
    bet = torch.randn(52, generator=g, dtype=F64, requires_grad=True)
    dy, dres = torch.randn(37, 52, generator=g, dtype=F64), torch.randn(37, 52, generator=g, dtype=F64)
    y = F.layer_norm(x, (52,), gam, bet, O.EPS)
    y.backward(dy)
    mean, var, rstd, y_ref = O.ln_fwd_ref(x.detach(), gam.detach(), bet.detach(), O.EPS)
    assert (y_ref - y.detach()).abs().max() < 1e-12
    assert (var - x.detach().var(1, unbiased=False)).abs().max() < 1e-12
    r = O.ln_bwd_ref(dy, x.detach(), mean, rstd, gam.detach(), dres)
    assert (r["dx"] - (x.grad + dres)).abs().max() < 1e-12
    assert (r["dgamma"] - gam.grad).abs().max() < 1e-12 and (r["dbeta"] - bet.grad).abs().max() < 1e-12
    z = (torch.randn(4096, generator=g, dtype=F64) * 3).requires_grad_(True)
    out = F.gelu(z, approximate="none")
    out.backward(torch.ones_like(out))
    assert (O.gelu_ref(z.detach()) - out.detach()).abs().max() < 1e-12
    assert (O.gelu_grad_ref(z.detach()) - z.grad).abs().max() < 1e-12
    m = torch.randn(70, 9, generator=g, dtype=F64)
    mean_t, m2_t, rows = O.tile_stats_ref(m, 32)
    assert rows.tolist() == [32, 32, 6]
    assert ((rows[:, None] * mean_t).sum(0) - m.sum(0)).abs().max() < 1e-12
    assert (m2_t[2] - m[64:].var(0, unbiased=False) * 6).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------ (2) bounds: not wrong, not vacuous
FWD_DEFECTS = ["eps_outside", "c_minus_1", "one_pass", "drop_chunk", "next_row_mean"]
BWD_DEFECTS = ["dres_before_scale", "dgamma_with_x"]


def test_layernorm_bounds_hold_for_the_restatement_and_catch_the_planted_defects():
    caught = {d: 0.0 for d in FWD_DEFECTS + BWD_DEFECTS}
    for rows, C, dtype, use_res in ln_sets():
        c = O.ln_case(rows, C, dtype, use_res)
        for b in O.ln_fwd_bounds(c["x"], c["gamma"], c["beta"], O.EPS, dtype):
            assert bool(torch.isfinite(b).all()), ("a vacuous bound", rows, C, dtype)
        for k, r in ln_ratios(c, dtype).items():
            note("layernorm %s %s" % (k, "bf16" if dtype == BF else "fp32"), r)
            assert r < 1, (k, r, rows, C, dtype, use_res)
        if rows > 40 or use_res == 0:
            continue             # (the defects are planted on the small sets with a residual gradient)
        for d in FWD_DEFECTS:
            if d == "drop_chunk" and C <= O.kpack(dtype):
                continue
            caught[d] = max(caught[d], max(ln_ratios(c, dtype, fwd_defect=d).values()))
        for d in BWD_DEFECTS:
            caught[d] = max(caught[d], max(ln_ratios(c, dtype, bwd_defect=d).values()))
    for d, r in caught.items():
        assert r > 1, ("planted defect not caught", d, r)


def test_one_pass_variance_is_caught_on_the_large_mean_row():
    c = O.ln_case(8, 96, F32, 1)
    assert abs(float(c["x"][-2].mean()) - 1000) < 1 and float(c["x"][-2].std()) < 0.05
    _, _, y = ln_fwd_f32(c, F32, "one_pass")
    _, _, _, y_ref = O.ln_fwd_ref(c["x"], c["gamma"], c["beta"], O.EPS)
    _, _, b_y = O.ln_fwd_bounds(c["x"], c["gamma"], c["beta"], O.EPS, F32)
    assert O.worst_ratio(stored(y, F32)[-2], y_ref[-2], b_y[-2]) > 1
    _, _, y = ln_fwd_f32(c, F32)
    assert O.worst_ratio(stored(y, F32)[-2], y_ref[-2], b_y[-2]) < 1


def gelu_sets():
    zb = O.bf16_all_finite()
    yield "bf16", BF, zb, O.gelu_dy(zb.numel(), BF)
    zf = O.gelu_f32_inputs()
    yield "fp32", F32, zf, O.gelu_dy(zf.numel(), F32)


def test_gelu_bounds_hold_for_the_restatement_and_catch_the_planted_defects():
    caught = {"tanh": 0.0, "coefficient": 0.0, "pdf_factor": 0.0}
    for name, dtype, z, dy in gelu_sets():
        zf, dyf = npf(z), npf(dy)
        b_f, b_b = O.gelu_fwd_bound(z, dtype), O.gelu_bwd_bound(z, dy, dtype)
        assert bool(torch.isfinite(b_f[z.abs() < 1e30]).all()) and bool(torch.isfinite(b_b[z.abs() < 1e30]).all())
        rf = O.worst_ratio(stored(gelu_fwd_f32(zf), dtype), O.gelu_ref(z), b_f)
        rb = O.worst_ratio(stored(gelu_bwd_f32(zf, dyf), dtype), dy * O.gelu_grad_ref(z), b_b)
        note("gelu fwd " + name, rf)
        note("gelu bwd " + name, rb)
        assert rf < 1 and rb < 1, (name, rf, rb)
        for d in ("tanh", "coefficient"):
            caught[d] = max(caught[d], O.worst_ratio(stored(gelu_fwd_f32(zf, d), dtype), O.gelu_ref(z), b_f))
        caught["pdf_factor"] = max(caught["pdf_factor"],
                                   O.worst_ratio(stored(gelu_bwd_f32(zf, dyf, "pdf_factor"), dtype), dy * O.gelu_grad_ref(z), b_b))
    for d, r in caught.items():
        assert r > 1, ("planted defect not caught", d, r)


def gemm_sets():
    for dtype in (F32, BF):
        for mt in (64, 128):
            for M in O.gemm_ms(mt):
                for N in O.GEMM_NS(dtype):
                    for K in O.GEMM_KS(dtype):
                        if mt == 128 and (N, K) != (72, 96):
                            continue          # (the 128-row tiles' row counts at one (N, K): the arithmetic does not depend on the tile)
                        for act in (2, 3):
                            yield dtype, M, K, N, act, mt
    yield BF, O.SLIN_SHAPE[0], O.SLIN_SHAPE[1], O.SLIN_SHAPE[2], 3, 64


def test_gemm_act_and_statistics_bounds_hold_and_catch_the_planted_defects():
    caught = {"neighbour_row": 0.0, "m2_about_zero": 0.0, "stats_of_unrounded": 0.0, "unrounded_y2": 0.0}
    for dtype, M, K, N, act, mt in gemm_sets():
        c = O.gemm_case(M, K, N, act)
        name = "bf16" if dtype == BF else "fp32"
        y2, ys, y32 = gemm_act_f32(c, dtype)
        if act == 2:
            assert torch.equal(y2, c["y2"]), "the exact operands are not exact"
        ref, bound = O.gemm_act_ref(c, y2), O.gemm_act_bound(c, y2, dtype)
        r = O.worst_ratio(ys, ref, bound)
        note("gemm_act act %d %s" % (act, name), r)
        assert r < 1, (dtype, M, K, N, act, r)
        # statistics of the stored activation
        mean_ref, m2_ref, _ = O.tile_stats_ref(ys, mt)
        bm, b2 = O.tile_stats_bounds(ys, mt)
        mean, m2 = tile_stats_f32(npf(ys), mt)
        rm, r2 = O.worst_ratio(stored(mean, F32), mean_ref, bm), O.worst_ratio(stored(m2, F32), m2_ref, b2)
        note("colstats mean " + name, rm)
        note("colstats M2 " + name, r2)
        assert rm < 1 and r2 < 1, (dtype, M, K, N, act, rm, r2)
        if M > 300:
            continue
        if act == 3 and M > 1:
            caught["neighbour_row"] = max(caught["neighbour_row"], O.worst_ratio(gemm_act_f32(c, dtype, "neighbour_row")[1], ref, bound))
        if M > 1:
            caught["m2_about_zero"] = max(caught["m2_about_zero"],
                                          O.worst_ratio(stored(tile_stats_f32(npf(ys), mt, "m2_about_zero")[1], F32), m2_ref, b2))
        caught["stats_of_unrounded"] = max(caught["stats_of_unrounded"], O.worst_ratio(stored(tile_stats_f32(y32, mt)[0], F32), mean_ref, bm))
    # GELU of the unrounded accumulator: invisible with exact operands (rounding changes nothing), so the GPU file also runs one real-valued set
    for dtype in (F32, BF):
        c = O.gemm_real_case(dtype)
        y2, ys, _ = gemm_act_f32(c, dtype)
        r = O.worst_ratio(ys, O.gemm_act_ref(c, y2), O.gemm_act_bound(c, y2, dtype))
        note("gemm_act act 2 real %s" % ("bf16" if dtype == BF else "fp32"), r)
        assert r < 1
        assert O.worst_ratio(y2, c["y2_ref"], O.gemm_real_y2_bound(c, dtype)) < 1
        _, yd, _ = gemm_act_f32(c, dtype, "unrounded_y2")
        caught["unrounded_y2"] = max(caught["unrounded_y2"], O.worst_ratio(yd, O.gemm_act_ref(c, y2), O.gemm_act_bound(c, y2, dtype)))
    for d, r in caught.items():
        assert r > 1, ("planted defect not caught", d, r)


# ------------------------------------------------------------------------------------------------ (3) nothing is left out
def test_input_sets_and_comparison_leave_no_element_out():
    zb = O.bf16_all_finite()
    assert zb.numel() == 65280 and torch.unique(zb.to(F32).view(torch.int32)).numel() == 65280 and bool(torch.isfinite(zb).all())
    assert torch.equal(O.rounded(zb, BF), zb)
    zf = O.gelu_f32_inputs()
    assert zf.numel() % 4 == 0 and torch.equal(O.rounded(zf, F32), zf)
    have = set(zf.to(F32).view(torch.int32).tolist())
    for p in O.GELU_F32_POINTS:
        for s in (1.0, -1.0):
            assert int(torch.tensor(s * p, dtype=F32).view(torch.int32)) in have, (s, p)
    assert float(zf.min()) <= -12 and float(zf.max()) >= 12
    # the comparison: a NaN, an infinity and a plain miss are all outside; an exact hit is inside a zero-free bound
    ref, bound = torch.zeros(4, dtype=F64), torch.full((4,), 1e-3, dtype=F64)
    for bad in (float("nan"), float("inf"), 2e-3):
        got = torch.zeros(4, dtype=F64)
        got[2] = bad
        assert O.worst_ratio(got, ref, bound) > 1
        with pytest.raises(AssertionError):
            O.assert_within(got, ref, bound)
    assert O.assert_within(ref.clone(), ref, bound) == 0.0
    # LayerNorm widths: every instance boundary of the dispatch and the generic kernels, in both dtypes
    for dtype in (F32, BF):
        geoms = {O.ln_geom(C, dtype) for C in O.ln_widths(dtype)}
        assert {(16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4), None} <= geoms
    assert O.ln_geom(O.LN_BF16_GENERIC_MAX, BF) is None and O.ln_geom(2048, BF) == (64, 4)
