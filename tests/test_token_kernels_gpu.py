"""Per-element float64 and exact tests of the token kernel family against tests/token_oracle.py: pfr_layernorm_fwd / _bwd / _bwd_dxsum,
pfr_gelu_fwd / _bwd, pfr_gemm_act / _colstats / _colsums on every kernel route (asserted by launch id), pfr_colsum_final_batch with
mt > 0, and the four ViT token kernels.  tests/test_token_oracle_host.py shows on the CPU that the bounds used here hold for a correct fp32
kernel and are exceeded by subtly wrong ones.

Conventions: outputs are pre-filled with NaN and live inside a larger buffer whose margins hold a sentinel that must survive; every
device tensor stays named until after the synchronise; nothing is skipped — a forced route that does not take its launch fails."""
import contextlib
import ctypes
import functools
import os
import struct

import pytest
import torch

import token_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -1024.0
MARGIN = 64          # elements on each side (a multiple of the 16-byte chunk in both dtypes)
NAN = float("nan")
RATIOS = {}


def L():
    from pets_face_recognition_amd._hip import lib
    return lib


def err_type():
    from pets_face_recognition_amd._hip.lib import PfrError
    return PfrError


def did(dt):
    return 1 if dt == BF else 0


def nm(dt):
    return "bf16" if dt == BF else "fp32"


def stream():
    return torch.cuda.current_stream().cuda_stream


def note(key, r):
    RATIOS[key] = max(RATIOS.get(key, 0.0), r)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = ["%-28s %.4f" % (k, v) for k, v in sorted(RATIOS.items())]
    print("\ndevice, worst err / bound:\n" + "\n".join(lines))
    out = os.environ.get("PFR_TOKEN_BOUNDS_OUT")
    if out:
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


@contextlib.contextmanager
def knobs(**kw):
    """set tuning knobs, restore what they held before in `finally`"""
    lib, old = L(), {}
    try:
        for k, v in kw.items():
            cur = ctypes.c_int(0)
            lib.pfr_get_tuning(k.encode(), ctypes.addressof(cur))
            old[k] = cur.value
            lib.pfr_set_tuning(k.encode(), v)
        yield
    finally:
        for k, v in old.items():
            lib.pfr_set_tuning(k.encode(), v)


class Guarded:
    """an output of `shape` inside a larger buffer: NaN inside, the sentinel in both margins"""

    def __init__(self, shape, dtype, fill=NAN):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + 2 * MARGIN,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[MARGIN:MARGIN + n].view(*shape)
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        assert bool((self.buf[:MARGIN] == SENT).all()) and bool((self.buf[MARGIN + self.n:] == SENT).all()), "margin overwritten: " + what
        return self.t


def dev(t, dt):
    return t.to(dt).to(DEV).contiguous()


def cpu64(t):
    return t.detach().cpu().to(F64)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_run(c, dtype, rows, C, want_null_stats=False):
    """forward, backward through both entry points, every output guarded.  -> dict of guarded outputs (checked) as CPU tensors"""
    lib, st, d = L(), stream(), did(dtype)
    x, dy = dev(c["x"], dtype), dev(c["dy"], dtype)
    gam, bet = dev(c["gamma"], F32), dev(c["beta"], F32)
    dres = dev(c["dres"], dtype) if c["dres"] is not None else None
    y, mu, rs = Guarded((rows, C), dtype), Guarded((rows,), F32), Guarded((rows,), F32)
    lib.pfr_layernorm_fwd(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), y.ptr(), mu.ptr(), rs.ptr(), d, rows, C, O.EPS, st)
    y_again = Guarded((rows, C), dtype)
    if want_null_stats:
        lib.pfr_layernorm_fwd(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), y_again.ptr(), 0, 0, d, rows, C, O.EPS, st)
    else:
        mu2, rs2 = Guarded((rows,), F32), Guarded((rows,), F32)
        lib.pfr_layernorm_fwd(x.data_ptr(), gam.data_ptr(), bet.data_ptr(), y_again.ptr(), mu2.ptr(), rs2.ptr(), d, rows, C, O.EPS, st)
    nb = lib.pfr_layernorm_bwd_blocks(rows)
    ok = lib.pfr_layernorm_bwd_dxsum_ok(d, C)
    assert ok == (1 if O.ln_geom(C, dtype) is not None else 0), "pfr_layernorm_bwd_dxsum_ok disagrees with the dispatch"
    outs = []
    for k in range(3):       # 0: _bwd_dxsum (with the column sums where the kernel has them), 1: the same again, 2: _bwd
        dx, part = Guarded((rows, C), dtype), Guarded((2, nb, C), F32)
        dsum = Guarded((nb, C), F32) if ok else None
        rp = dres.data_ptr() if dres is not None else 0
        if k < 2:
            lib.pfr_layernorm_bwd_dxsum(dy.data_ptr(), x.data_ptr(), mu.ptr(), rs.ptr(), gam.data_ptr(), rp, dx.ptr(), part.ptr(),
                                        dsum.ptr() if ok else 0, d, rows, C, st)
        else:
            lib.pfr_layernorm_bwd(dy.data_ptr(), x.data_ptr(), mu.ptr(), rs.ptr(), gam.data_ptr(), rp, dx.ptr(), part.ptr(), d, rows, C, st)
        outs.append((dx, part, dsum))
    torch.cuda.synchronize()
    what = "layernorm %s rows %d C %d" % (nm(dtype), rows, C)
    r = {"y": y.check(what), "mean": mu.check(what), "rstd": rs.check(what), "ok": ok}
    assert torch.equal(y_again.check(what), r["y"]), what + ": a second forward call (or one without mean / rstd) gives other bits"
    if not want_null_stats:
        assert torch.equal(mu2.check(what), r["mean"]) and torch.equal(rs2.check(what), r["rstd"])
    dx0, part0, dsum0 = (g.check(what) if g is not None else None for g in outs[0])
    for dx, part, dsum in outs[1:]:
        assert torch.equal(dx.check(what), dx0) and torch.equal(part.check(what), part0), what + ": backward calls differ in bits"
    if ok:
        assert torch.equal(outs[1][2].check(what), dsum0)
    r.update(dx=dx0, part=part0, dsum=dsum0)
    return r


def ln_check(c, dtype, rows, C, r):
    what = "layernorm %s rows %d C %d" % (nm(dtype), rows, C)
    m_ref, _, r_ref, y_ref = O.ln_fwd_ref(c["x"], c["gamma"], c["beta"], O.EPS)
    b_m, b_r, b_y = O.ln_fwd_bounds(c["x"], c["gamma"], c["beta"], O.EPS, dtype)
    note("layernorm y " + nm(dtype), O.assert_within(r["y"], y_ref, b_y, what + " y"))
    note("layernorm mean " + nm(dtype), O.assert_within(r["mean"], m_ref, b_m, what + " mean"))
    note("layernorm rstd " + nm(dtype), O.assert_within(r["rstd"], r_ref, b_r, what + " rstd"))
    mu64, rs64 = cpu64(r["mean"]), cpu64(r["rstd"])
    ref = O.ln_bwd_ref(c["dy"], c["x"], mu64, rs64, c["gamma"], c["dres"])
    b_dx, b_dg, b_db = O.ln_bwd_bounds(c["dy"], c["x"], mu64, rs64, c["gamma"], c["dres"], dtype)
    note("layernorm dx " + nm(dtype), O.assert_within(r["dx"], ref["dx"], b_dx, what + " dx"))
    part = cpu64(r["part"])
    note("layernorm dgamma " + nm(dtype), O.assert_within(part[0].sum(0), ref["dgamma"], b_dg, what + " dgamma"))
    note("layernorm dbeta " + nm(dtype), O.assert_within(part[1].sum(0), ref["dbeta"], b_db, what + " dbeta"))
    if r["ok"]:
        dxs = cpu64(r["dx"])
        note("layernorm dxsum " + nm(dtype), O.assert_within(cpu64(r["dsum"]).sum(0), dxs.sum(0), O.colsum_bound(dxs), what + " dxsum"))


LN_PARAMS = [(dt, C) for dt in (F32, BF) for C in O.ln_widths(dt)]


@pytest.mark.parametrize("use_res", [0, 1])
@pytest.mark.parametrize("dtype,C", LN_PARAMS, ids=["%s-%d" % (nm(dt), C) for dt, C in LN_PARAMS])
def test_layernorm_per_element(dtype, C, use_res):
    """every width of the dispatch (instance boundaries, the generic kernels, the widest rows) at the row counts around one forward
    workgroup batch, under each rows-in-flight knob the width reacts to"""
    g = O.ln_geom(C, dtype)
    rbs = (4, 6, 8) if g is not None and g[1] == 1 else (4,)
    first = True
    for rb in rbs:
        with knobs(ln_rb=rb):
            for rows in O.ln_row_counts(C, dtype, rb):
                c = O.ln_case(rows, C, dtype, use_res)
                r = ln_run(c, dtype, rows, C, want_null_stats=first)
                first = False
                ln_check(c, dtype, rows, C, r)
    if g is None:     # the generic backward has no column sums: asking for them is an argument error, nothing is launched
        lib, rows = L(), 3
        c = O.ln_case(rows, C, dtype, use_res)
        x, dy, gam = dev(c["x"], dtype), dev(c["dy"], dtype), dev(c["gamma"], F32)
        mu, rs = torch.zeros(rows, device=DEV), torch.ones(rows, device=DEV)
        nb = lib.pfr_layernorm_bwd_blocks(rows)
        dx, part, dsum = Guarded((rows, C), dtype), Guarded((2, nb, C), F32), Guarded((nb, C), F32)
        with pytest.raises(err_type(), match=r"rc=-1"):
            lib.pfr_layernorm_bwd_dxsum(dy.data_ptr(), x.data_ptr(), mu.data_ptr(), rs.data_ptr(), gam.data_ptr(), 0, dx.ptr(), part.ptr(),
                                        dsum.ptr(), did(dtype), rows, C, stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(dx.check("generic dxsum").float()).all()) and bool(torch.isnan(dsum.check("generic dxsum")).all())


@pytest.mark.parametrize("dtype", [F32, BF], ids=nm)
def test_layernorm_many_rows_reach_the_backward_grid_cap(dtype):
    lib = L()
    rows, C = O.LN_MANY_ROWS, O.kpack(dtype)
    assert lib.pfr_layernorm_bwd_blocks(rows) == 1024 and lib.pfr_layernorm_bwd_blocks(16384) == 1024 and lib.pfr_layernorm_bwd_blocks(16368) == 1023
    c = O.ln_case(rows, C, dtype, 1)
    ln_check(c, dtype, rows, C, ln_run(c, dtype, rows, C))


# ------------------------------------------------------------------------------------------------ GELU
def gelu_run(z, dy, dtype):
    """-> forward, backward (out of place), backward in place (dx aliasing dy), as CPU tensors"""
    lib, st, d, n = L(), stream(), did(dtype), z.numel()
    zd, dyd = dev(z, dtype), dev(dy, dtype)
    y, dx = Guarded((n,), dtype), Guarded((n,), dtype)
    inpl = Guarded((n,), dtype)
    inpl.t.copy_(dyd)
    lib.pfr_gelu_fwd(zd.data_ptr(), y.ptr(), d, n, st)
    lib.pfr_gelu_bwd(zd.data_ptr(), dyd.data_ptr(), dx.ptr(), d, n, st)
    lib.pfr_gelu_bwd(zd.data_ptr(), inpl.ptr(), inpl.ptr(), d, n, st)
    torch.cuda.synchronize()
    yy, dd = y.check("gelu fwd"), dx.check("gelu bwd")
    a, b = inpl.check("gelu bwd in place"), dd
    assert torch.equal(a.view(torch.int16 if dtype == BF else torch.int32), b.view(torch.int16 if dtype == BF else torch.int32)), "in place differs"
    return yy.cpu(), dd.cpu()


@pytest.mark.parametrize("dtype", [BF, F32], ids=nm)
def test_gelu_per_element(dtype):
    """bf16: every finite bit pattern; fp32: a dense grid over [-12, 12] and the edge points.  No element is excluded."""
    z = O.bf16_all_finite() if dtype == BF else O.gelu_f32_inputs()
    dy = O.gelu_dy(z.numel(), dtype)
    y, dx = gelu_run(z, dy, dtype)
    ref_y, ref_dx = O.gelu_ref(z), dy * O.gelu_grad_ref(z)
    # (the largest finite values times a gradient of 1000 overflow the format: those elements are judged by their class, +-inf)
    assert torch.equal(O.finite_class(y), O.finite_class(O.rounded(ref_y, dtype)))
    assert torch.equal(O.finite_class(dx), O.finite_class(O.rounded(ref_dx, dtype)))
    keep = torch.isfinite(O.rounded(ref_dx, dtype))
    note("gelu fwd " + nm(dtype), O.assert_within(y, ref_y, O.gelu_fwd_bound(z, dtype), "gelu fwd " + nm(dtype)))
    note("gelu bwd " + nm(dtype), O.assert_within(dx[keep], ref_dx[keep], O.gelu_bwd_bound(z, dy, dtype)[keep], "gelu bwd " + nm(dtype)))


@pytest.mark.parametrize("dtype", [BF, F32], ids=nm)
def test_gelu_non_finite_inputs(dtype):
    kp = O.kpack(dtype)
    z = torch.zeros(2 * kp, dtype=F64)
    z[0], z[1], z[2] = float("nan"), float("inf"), float("-inf")
    dy = torch.ones(2 * kp, dtype=F64)
    y, dx = gelu_run(z, dy, dtype)
    assert bool(torch.isnan(y[0])) and float(y[1]) == float("inf")
    assert torch.equal(O.finite_class(y), O.finite_class(O.gelu_ref(z)))
    assert torch.equal(O.finite_class(dx), O.finite_class(dy * O.gelu_grad_ref(z)))


@pytest.mark.parametrize("dtype", [BF, F32], ids=nm)
def test_gelu_past_the_grid_cap_and_ragged_length(dtype):
    """(8192 * 256 + 3) chunks: the grid-stride loop runs; the values repeat a short pattern, so the result must repeat its bits"""
    lib, st, d, kp = L(), stream(), did(dtype), O.kpack(dtype)
    base = (O.bf16_all_finite() if dtype == BF else O.gelu_f32_inputs())[:4096 * kp]
    n = (8192 * 256 + 3) * kp
    rep = n // base.numel() + 1
    small = dev(base, dtype)
    z = small.repeat(rep)[:n].contiguous()
    dy = dev(O.gelu_dy(base.numel(), dtype), dtype)
    dyb = dy.repeat(rep)[:n].contiguous()
    y, dx = Guarded((n,), dtype), Guarded((n,), dtype)
    ys, dxs = Guarded((base.numel(),), dtype), Guarded((base.numel(),), dtype)
    lib.pfr_gelu_fwd(z.data_ptr(), y.ptr(), d, n, st)
    lib.pfr_gelu_bwd(z.data_ptr(), dyb.data_ptr(), dx.ptr(), d, n, st)
    lib.pfr_gelu_fwd(small.data_ptr(), ys.ptr(), d, base.numel(), st)
    lib.pfr_gelu_bwd(small.data_ptr(), dy.data_ptr(), dxs.ptr(), d, base.numel(), st)
    torch.cuda.synchronize()
    it = torch.int16 if dtype == BF else torch.int32
    assert torch.equal(y.check("gelu big").view(it), ys.check("gelu small").repeat(rep)[:n].view(it))
    assert torch.equal(dx.check("gelu big").view(it), dxs.check("gelu small").repeat(rep)[:n].view(it))
    # a length that is no multiple of the chunk: an argument error, nothing launched, the pre-fill untouched
    out = Guarded((4 * kp,), dtype)
    for call in (lambda: lib.pfr_gelu_fwd(small.data_ptr(), out.ptr(), d, kp + 1, st),
                 lambda: lib.pfr_gelu_bwd(small.data_ptr(), dy.data_ptr(), out.ptr(), d, 2 * kp - 1, st)):
        with pytest.raises(err_type(), match=r"rc=-1"):
            call()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.check("gelu ragged").float()).all())


# ------------------------------------------------------------------------------------------------ gemm_act
TILE, PERSIST, SLIN = 1, 2, 6
OFF = dict(sconv=0, sconv3=0, sstem=0)
Y_SEEN = {}          # (dtype, M, K, N, act) -> (route, y bits on the CPU): every route must give the first one's bits


@functools.lru_cache(maxsize=None)
def gcase(M, K, N, act):
    return O.gemm_case(M, K, N, act)


def last_id():
    v = L().pfr_debug_last_conv_kernel()
    return v >> 24, v & 0xFFFFFF


def gemm_launch(c, dtype, with_stats, mt=0):
    """one pfr_gemm_act (or _colstats) launch -> y2 (act 2: the guarded output; act 3: the input), y, stats or None, launch id"""
    lib, st, d = L(), stream(), did(dtype)
    M, K, N, act = c["M"], c["K"], c["N"], c["act"]
    x, w = dev(c["x"], dtype), dev(c["w"], dtype)
    bias = dev(c["bias"], F32) if act == 2 else None
    y = Guarded((M, N), dtype)
    y2 = Guarded((M, N), dtype)
    if act == 3:
        y2.t.copy_(dev(c["y2"], dtype))
    T = (M + mt - 1) // mt if with_stats else 0
    stats = Guarded((T, 2, N), F32) if with_stats else None
    if with_stats:
        lib.pfr_gemm_act_colstats(x.data_ptr(), w.data_ptr(), y.ptr(), d, M, K, N, bias.data_ptr() if bias is not None else 0, act, y2.ptr(),
                                  stats.ptr(), st)
    else:
        lib.pfr_gemm_act(x.data_ptr(), w.data_ptr(), y.ptr(), d, M, K, N, bias.data_ptr() if bias is not None else 0, act, y2.ptr(), st)
    kid = last_id()
    torch.cuda.synchronize()
    what = "gemm_act %s M %d K %d N %d act %d" % (nm(dtype), M, K, N, act)
    return y2.check(what).cpu(), y.check(what).cpu(), (stats.check(what).cpu() if with_stats else None), kid


def gemm_check(c, dtype, y2, y, route):
    what = "gemm_act %s M %d K %d N %d act %d route %s" % (nm(dtype), c["M"], c["K"], c["N"], c["act"], route)
    assert torch.equal(y2, c["y2"].to(dtype)), what + ": y2 is not the exact pre-activation"
    y2_64 = cpu64(y2)
    note("gemm_act act %d %s" % (c["act"], nm(dtype)), O.assert_within(y, O.gemm_act_ref(c, y2_64), O.gemm_act_bound(c, y2_64, dtype), what))
    key = (dtype, c["M"], c["K"], c["N"], c["act"])
    if key in Y_SEEN:
        assert torch.equal(Y_SEEN[key][1], y), what + ": y differs in bits from route " + Y_SEEN[key][0]
    else:
        Y_SEEN[key] = (route, y)


def stats_check(c, dtype, y, stats, mt):
    """each tile's (mean, M2) against the float64 statistics of the STORED y; the merge of pfr_colsum_final_batch with mt > 0"""
    lib, M, N = L(), c["M"], c["N"]
    what = "colstats %s M %d K %d N %d act %d mt %d" % (nm(dtype), M, c["K"], N, c["act"], mt)
    ys = cpu64(y)
    mean_ref, m2_ref, rows = O.tile_stats_ref(ys, mt)
    assert int(rows[-1]) == M - (rows.numel() - 1) * mt
    shift = c["lin"][::mt].abs()          # the kernel's shift: the first row's accumulator of each tile
    bm, b2 = O.tile_stats_bounds(ys, mt, shift)
    note("colstats mean " + nm(dtype), O.assert_within(stats[:, 0], mean_ref, bm, what + " mean"))
    note("colstats M2 " + nm(dtype), O.assert_within(stats[:, 1], m2_ref, b2, what + " M2"))
    part = stats.to(DEV).contiguous()
    out = Guarded((N,), F32)
    raw = struct.pack("<QQiiiiii", part.data_ptr(), out.ptr(), stats.shape[0], N, 0, mt, M, 0)
    tab = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    lib.pfr_colsum_final_batch(tab.data_ptr(), 1, N, stream())
    torch.cuda.synchronize()
    note("colstats merge " + nm(dtype), O.assert_within(out.check(what).cpu(), ys.sum(0), O.tile_merge_bound(ys, mt, shift), what + " merged column sum"))


def tile_detail(tile, K, dtype):
    """pfr_igemm.hip launch_tile: 64-byte k-steps below K = 512; FAST when K is a multiple of the k-step; pfr_gemm_act has no residual or
    accumulate target, so the operand-row form (bit 6, EPRE) is never its launch — for act 3 the launcher excludes it outright"""
    return tile | (16 if K % (4 * O.kpack(dtype)) == 0 else 0)


@pytest.mark.parametrize("tile", [-1, 0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [F32, BF], ids=nm)
def test_gemm_act_tile_kernel_routes(dtype, tile):
    """the tile kernel at the heuristic's choice and at every forced 4-wave tile (the 256-row tiles need K % 64 == 0: none of these K), with
    and without the statistics epilogue"""
    lib = L()
    with knobs(igemm_p=0, slin=0, igemm_tile=tile, **OFF):
        for N in O.GEMM_NS(dtype):
            for K in O.GEMM_KS(dtype):
                mt = lib.pfr_gemm_act_mtile(5, K, N, did(dtype))
                want_tile = tile if tile >= 0 else (1 if N > 64 else 3)
                assert mt == (128 if want_tile in (0, 2) else 64)
                for M in O.gemm_ms(mt):
                    assert lib.pfr_gemm_act_mtile(M, K, N, did(dtype)) == mt
                    for act in (2, 3):
                        c = gcase(M, K, N, act)
                        y2, y, _, kid = gemm_launch(c, dtype, False)
                        assert kid == (TILE, tile_detail(want_tile, K, dtype)), (kid, M, K, N, act)
                        gemm_check(c, dtype, y2, y, "tile %d" % tile)
                        y2s, ysb, stats, kid = gemm_launch(c, dtype, True, mt)
                        assert kid == (TILE, tile_detail(want_tile, K, dtype)), (kid, M, K, N, act)
                        assert torch.equal(y2s, y2) and torch.equal(ysb, y), "the statistics launch stores other bits"
                        stats_check(c, dtype, y, stats, mt)


@pytest.mark.parametrize("dtype", [F32, BF], ids=nm)
def test_gemm_act_persistent_kernel_route(dtype):
    """igemm_p = 2: the persistent kernel takes every launch whose K is a multiple of its k-step (four chunks): K = 96 of the set"""
    lib, K = L(), 96
    with knobs(igemm_p=2, igemm_ptile=-1, slin=0, igemm_tile=-1, **OFF):
        for N in O.GEMM_NS(dtype):
            for M in O.gemm_ms(lib.pfr_gemm_act_mtile(5, K, N, did(dtype))):
                for act in (2, 3):
                    c = gcase(M, K, N, act)
                    y2, y, _, kid = gemm_launch(c, dtype, False)
                    assert kid == (PERSIST, 1 if N > 64 else 3), (kid, M, K, N, act)
                    gemm_check(c, dtype, y2, y, "persistent")


def test_gemm_act_streaming_linear_route_and_column_sums():
    """slin = 2, bf16, K = 96: epilogues 3 (GELU) and 4 (GELU backward) of the streaming Linear against the tile kernel's bits and the
    oracle; pfr_gemm_act_colsums: the partial rows add up to the float64 column sum of the stored output"""
    lib, st = L(), stream()
    M, K, N = O.SLIN_SHAPE
    for act in (2, 3):
        c = gcase(M, K, N, act)
        with knobs(igemm_p=0, slin=0, igemm_tile=-1, **OFF):
            assert lib.pfr_gemm_act_colsum_parts(M, K, N, 1) == 0
            y2, y, _, kid = gemm_launch(c, BF, False)
            assert kid[0] == TILE
            gemm_check(c, BF, y2, y, "tile")
        with knobs(igemm_p=0, slin=2, igemm_tile=-1, **OFF):
            y2, y, _, kid = gemm_launch(c, BF, False)
            assert kid == (SLIN, (3 if act == 2 else 4) | (64 << 4)), kid
            gemm_check(c, BF, y2, y, "streaming")
            if act == 3:
                parts = lib.pfr_gemm_act_colsum_parts(M, K, N, 1)
                assert parts > 0
                x, w, z = dev(c["x"], BF), dev(c["w"], BF), dev(c["y2"], BF)
                out, sums = Guarded((M, N), BF), Guarded((parts, N), F32)
                lib.pfr_gemm_act_colsums(x.data_ptr(), w.data_ptr(), out.ptr(), 1, M, K, N, z.data_ptr(), sums.ptr(), st)
                kid = last_id()
                torch.cuda.synchronize()
                assert kid == (SLIN, 4 | (64 << 4)), kid
                assert torch.equal(out.check("colsums y").cpu(), y)
                ys = cpu64(y)
                note("colsums bf16", O.assert_within(cpu64(sums.check("colsums")).sum(0), ys.sum(0), O.colsum_bound(ys), "colsums"))


@pytest.mark.parametrize("dtype", [F32, BF], ids=nm)
def test_gemm_act_real_valued_operands(dtype):
    """one set whose pre-activation is NOT exact: y2 inside the accumulation bound, y per element against GELU of the stored y2"""
    lib, st, d = L(), stream(), did(dtype)
    c = O.gemm_real_case(dtype)
    M, K, N = O.GEMM_REAL_SHAPE
    x, w, bias = dev(c["x"], dtype), dev(c["w"], dtype), dev(c["bias"], F32)
    y, y2 = Guarded((M, N), dtype), Guarded((M, N), dtype)
    lib.pfr_gemm_act(x.data_ptr(), w.data_ptr(), y.ptr(), d, M, K, N, bias.data_ptr(), 2, y2.ptr(), st)
    torch.cuda.synchronize()
    y2c = cpu64(y2.check("real y2"))
    note("gemm_act y2 real " + nm(dtype), O.assert_within(y2c, c["y2_ref"], O.gemm_real_y2_bound(c, dtype), "real-valued y2"))
    note("gemm_act act 2 real " + nm(dtype),
         O.assert_within(y.check("real y").cpu(), O.gemm_act_ref(c, y2c), O.gemm_act_bound(c, y2c, dtype), "real-valued y"))


# ------------------------------------------------------------------------------------------------ ViT tokens
@pytest.mark.parametrize("dtype", [F32, BF], ids=nm)
def test_vit_token_kernels_exact(dtype):
    lib, st, d = L(), stream(), did(dtype)
    for B in O.VIT_B:
        for S in O.VIT_S:
            for D in O.VIT_D(dtype):
                what = "vit %s B %d S %d D %d" % (nm(dtype), B, S, D)
                g = O.rng("vit", B, S, D, str(dtype))
                patches = torch.randn(B, max(S - 1, 1), D, generator=g).to(dtype)
                cls, pos = torch.randn(D, generator=g), torch.randn(S, D, generator=g)
                dtok = torch.randn(B, S, D, generator=g).to(dtype)
                pd, cd, posd, dtd = patches.to(DEV), cls.to(DEV), pos.to(DEV), dtok.to(DEV)
                tok = Guarded((B, S, D), dtype)
                lib.pfr_vit_tokens_fwd(pd.data_ptr() if S > 1 else 0, cd.data_ptr(), posd.data_ptr(), tok.ptr(), d, B, S, D, st)
                dpat, dpos, dcls = Guarded((B, max(S - 1, 1), D), dtype), Guarded((S, D), F32), Guarded((D,), F32)
                lib.pfr_vit_tokens_bwd(dtd.data_ptr(), dpat.ptr() if S > 1 else 0, dpos.ptr(), dcls.ptr(), d, B, S, D, st)
                ctok, dz = Guarded((B, D), dtype), Guarded((B, S, D), dtype)
                lib.pfr_vit_cls_fwd(dtd.data_ptr(), ctok.ptr(), d, B, S, D, st)
                lib.pfr_vit_cls_bwd(pd.data_ptr(), dz.ptr(), d, B, S, D, st)      # (dy = the first B x D block of `patches`)
                torch.cuda.synchronize()
                want = torch.empty(B, S, D)
                want[:, 0] = cls + pos[0]
                if S > 1:
                    want[:, 1:] = patches.float() + pos[1:]
                assert torch.equal(tok.check(what).cpu(), want.to(dtype)), what + " tokens_fwd"
                acc = torch.zeros(S, D)
                for b in range(B):           # ascending b, fp32
                    acc = acc + dtok[b].float()
                assert torch.equal(dpos.check(what).cpu(), acc), what + " dpos"
                assert torch.equal(dcls.check(what).cpu(), acc[0]), what + " dclass_token"
                got = dpat.check(what).cpu()
                if S > 1:
                    assert torch.equal(got, dtok[:, 1:]), what + " dpatches"
                else:
                    assert bool(torch.isnan(got.float()).all())
                assert torch.equal(ctok.check(what).cpu(), dtok[:, 0]), what + " cls_fwd"
                dyv = patches.reshape(-1)[:B * D].view(B, D)
                wz = torch.zeros(B, S, D, dtype=dtype)
                wz[:, 0] = dyv
                gz = dz.check(what).cpu()
                it = torch.int16 if dtype == BF else torch.int32
                assert torch.equal(gz.view(it), wz.view(it)), what + " cls_bwd"
