"""Exact-integer and per-element float64 tests of the implicit-GEMM convolution family (pfr_igemm.hip, pfr_igemm_p.hip, pfr_sconv.hip,
pfr_sconv3.hip, pfr_sstem.hip, pfr_slin.hip, pfr_wgrad.hip, pfr_wgrad9.hip) against tests/conv_oracle.py.

Exact tests: with the oracle's integer data every product and partial sum is exact in fp32 and every expected value is exact in bf16,
whatever the k order, split count or tile, so EVERY kernel variant must give torch.equal to the float64 reference cast to the output
dtype.  Outputs are pre-filled with NaN (or the accumulate target), padding columns of a padded pitch and the tail of the weight-gradient
workspace with a sentinel that must survive.  Every case asserts pfr_debug_last_conv_kernel after its launch: a case whose forced kernel
did not take the launch FAILS.  The expected ids restate the launchers' eligibility rules (include/pfr_hip.h documents the encoding).

Rounding test: real-valued data, element by element within the derived bound of conv_oracle.rounding_bound (nothing fitted to a run)."""
import contextlib
import ctypes
import functools

import pytest
import torch

import conv_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SENT = -1024.0          # exact in bf16 and fp32
TILE, PERSIST, SCONV, SCONV3, SSTEM, SLIN, WG_TILE, WG_BIG, SWGRAD, WGRAD9 = range(1, 11)
TILE_BQBP = {0: (128, 128), 1: (64, 128), 2: (128, 64), 3: (64, 64), 4: (256, 256), 5: (256, 128)}
STREAM_OFF = dict(sconv=0, sconv3=0, sstem=0, slin=0)


def L():
    from pets_face_recognition_amd._hip import lib
    return lib


def ops():
    from pets_face_recognition_amd._hip import ops as o
    return o


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


def last_id(what):
    v = L().pfr_debug_last_conv_kernel()
    print("conv-id 0x%07x family %d detail 0x%x  %s" % (v, v >> 24, v & 0xFFFFFF, what))
    return v >> 24, v & 0xFFFFFF


def kp_of(dt):
    return 8 if dt == BF else 4


def dev(t, dt):
    return None if t is None else t.to(dt).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ expected ids (the launchers' rules)
def tile_detail(tile, kch_knob, C, K, dt, odt, pro=False, post_rows=False, Cout=0, ldy=0, pclass=False):
    """pfr_igemm.hip launch_tile / launch_tile_k: the 256-row tiles always run 128-byte k-steps; the others the forced k-step when C
    allows it (kch_knob 0: 128-byte steps for K >= 512); FAST = C a multiple of the k-step; EPRE = bf16 -> bf16, FAST, a masked
    residual or an accumulate target to read back, 16-byte output rows"""
    kp = kp_of(dt)
    if tile >= 4:
        kch = 8
    elif kch_knob == 4:
        kch = 4
    else:
        kch = 8 if C % (8 * kp) == 0 and (kch_knob == 8 or K >= 512) else 4
    fast = C % (kch * kp) == 0
    epre = (not pro) and dt == BF and odt == BF and fast and post_rows and Cout % 8 == 0 and ldy % 8 == 0
    return tile | (8 if kch == 8 else 0) | (16 if fast else 0) | (32 if pro else 0) | (64 if epre else 0) | (256 if pclass and fast else 0)


def persist_detail(ptile, pkch, C, Cout, rows, dt, odt, post, ldy, pclass=False):
    """pfr_igemm_p.hip launch_p: the lean epilogue (and with it the 128-byte k-steps) needs bf16 output, whole tiles, no post-ops"""
    bq, bp = TILE_BQBP[ptile]
    lean = odt == BF and not post and rows % bq == 0 and Cout % bp == 0 and (ldy * 2) % 16 == 0
    k8 = lean and pkch == 8 and C % (8 * kp_of(dt)) == 0
    return ptile | (8 if k8 else 0) | (16 if lean else 0) | (256 if pclass else 0)


# ------------------------------------------------------------------------------------------------ runners
def run_fwd(c, dt, odt, ldy=None, what=""):
    """one forward launch of an oracle case; asserts the exact result and the surviving padding; -> (family, detail)"""
    o, lib = ops(), L()
    N, H, W, C, Cout, R, stride, pad = c["geom"]
    OH, OW = c["ohw"]
    M, ld = N * OH * OW, ldy or Cout
    flags = c["flags"]
    x, w = dev(c["x"], dt), dev(c["w"], dt)
    out = torch.full((M, ld), SENT, dtype=F64)
    out[:, :Cout] = c["acc"].reshape(M, Cout) if c["acc"] is not None else float("nan")
    out = dev(out, odt).reshape(N, OH, OW, ld)
    res = None
    if c["res"] is not None:
        res = torch.zeros(M, ld, dtype=F64)
        res[:, :Cout] = c["res"].reshape(M, Cout)
        res = dev(res, odt)
    kpo = kp_of(odt)
    if "join" in flags:
        assert stride == 1 and ld == Cout and dt == odt
        mask = c["mask%d" % kpo].to(DEV)
        lib.pfr_conv2d_dgrad_join(x.data_ptr(), w.data_ptr(), out.data_ptr(), 1 if dt == BF else 0, N, H, W, C, Cout, R, R, pad, 0, OH, OW,
                                  res.data_ptr(), mask.data_ptr(), torch.cuda.current_stream().cuda_stream)
    else:
        pro = None if c["pro"] is None else (dev(c["pro"][0], F32), dev(c["pro"][1], F32), c["pro"][2])
        o.conv2d_fwd(x, w, stride=stride, pad=pad, out_hw=(OH, OW), out=out, bias=dev(c["bias"], F32), accumulate=c["acc"] is not None,
                     out_relu=c["relu"], pro=pro, residual=res)
    torch.cuda.synchronize()
    fam = last_id("%s %s %s->%s ldy %d" % (what, c["geom"], dt, odt, ld))
    got = out.reshape(M, ld).cpu()
    O.assert_exact(got[:, :Cout], O.fwd_ref(c, kpo).reshape(M, Cout), "%s %s %s %s->%s" % (what, c["geom"], sorted(flags), dt, odt))
    assert bool((got[:, Cout:] == SENT).all()), "padding columns overwritten"
    return fam


def run_dgrad(c, dt, what=""):
    o = ops()
    N, H, W, C, Cout, R, stride, pad = c["geom"]
    wt = o.weight_dgrad_layout(dev(c["w"], dt))
    out = dev(c["acc"], dt) if c["acc"] is not None else torch.full((N, H, W, C), float("nan"), device=DEV, dtype=dt)
    o.conv2d_dgrad(dev(c["dy"], dt), wt, (H, W), stride, pad, R, R, out=out, accumulate=c["acc"] is not None)
    torch.cuda.synchronize()
    fam = last_id("%s dgrad %s %s acc %s" % (what, c["geom"], dt, c["acc"] is not None))
    O.assert_exact(out, c["ref"], "%s dgrad %s %s acc %s" % (what, c["geom"], dt, c["acc"] is not None))
    return fam


@functools.lru_cache(maxsize=None)
def wgrad_ref(geom, pro, scale, accumulate):
    c = O.wgrad_case(geom, pro, accumulate)
    N, H, W, C, Cout, R, stride, pad = geom
    return O.conv_wgrad_ref(c["x"], c["dy"], R, R, stride, pad, c["pro"], scale, c["acc"])


def run_wgrad(geom, dt, pro="", scale=1.0, accumulate=False, what=""):
    """one pfr_conv2d_wgrad launch: the workspace is sized from pfr_conv2d_wgrad_splits under the CURRENT knobs and padded with a
    sentinel tail that must be untouched"""
    lib = L()
    c = O.wgrad_case(geom, pro, accumulate)
    N, H, W, C, Cout, R, stride, pad = geom
    OH, OW = c["dy"].shape[1:3]
    M, KK = N * OH * OW, R * R * C
    need = lib.pfr_conv2d_wgrad_splits(M, Cout, KK) * Cout * KK
    ws = torch.full((need + 1024,), SENT, device=DEV, dtype=F32)
    dw = dev(c["acc"], F32) if accumulate else torch.full((Cout, R, R, C), float("nan"), device=DEV, dtype=F32)
    x, dy = dev(c["x"], dt), dev(c["dy"], dt)
    ps = psh = None
    prelu = 0
    if c["pro"] is not None:
        ps, psh, prelu = dev(c["pro"][0], F32), dev(c["pro"][1], F32), c["pro"][2]
    lib.pfr_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), 1 if dt == BF else 0, N, H, W, C, Cout, R, R, stride, pad,
                         OH, OW, Cout, 0 if ps is None else ps.data_ptr(), 0 if psh is None else psh.data_ptr(), prelu, float(scale),
                         int(accumulate), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    desc = "%s wgrad %s %s pro '%s' scale %s acc %s" % (what, geom, dt, pro, scale, accumulate)
    fam = last_id(desc)
    O.assert_exact(dw, wgrad_ref(geom, pro, scale, accumulate), desc)
    assert bool((ws[need:] == SENT).all()), "workspace tail overwritten: " + desc
    return fam


# ------------------------------------------------------------------------------------------------ forward, tile kernel
@pytest.mark.parametrize("kch", [4, 8])
@pytest.mark.parametrize("tile", range(6))
def test_forward_tile_kernel_exact(tile, kch):
    """every forced tile x k-step of the one-tile-per-workgroup kernel on the eight edge geometries, fp32, bf16 and bf16 -> fp32.  The
    256-row tiles exist for bf16 -> bf16 with K % 64 == 0 only (pick_tile falls back to the heuristic otherwise: those are not run)."""
    with knobs(igemm_p=0, igemm_tile=tile, igemm_kch=kch, **STREAM_OFF):
        for geom in O.FWD_GEOMS:
            N, H, W, C, Cout, R, stride, pad = geom
            K = R * R * C
            for dt, odt in ((F32, F32), (BF, BF), (BF, F32)):
                if tile >= 4 and ((dt, odt) != (BF, BF) or K % 64):
                    continue
                ld = O.LDY.get(geom)
                fam = run_fwd(O.fwd_case(geom), dt, odt, ld, "tile %d kch %d" % (tile, kch))
                assert fam == (TILE, tile_detail(tile, kch, C, K, dt, odt)), (geom, dt, odt, fam)


# ------------------------------------------------------------------------------------------------ forward, persistent kernel
@pytest.mark.parametrize("pkch", [4, 8])
@pytest.mark.parametrize("ptile", range(4))
def test_forward_persistent_kernel_exact(ptile, pkch):
    """igemm_p = 2 on every geometry whose C is a multiple of the persistent kernel's k-step (4 chunks)"""
    with knobs(igemm_p=2, igemm_ptile=ptile, igemm_pkch=pkch, igemm_ppf=0, **STREAM_OFF):
        ran = 0
        for geom in O.FWD_GEOMS:
            N, H, W, C, Cout, R, stride, pad = geom
            for dt, odt in ((F32, F32), (BF, BF), (BF, F32)):
                if C % (4 * kp_of(dt)):
                    continue
                c = O.fwd_case(geom)
                ld = O.LDY.get(geom) or Cout
                fam = run_fwd(c, dt, odt, ld, "persistent %d pkch %d" % (ptile, pkch))
                M = N * c["ohw"][0] * c["ohw"][1]
                assert fam == (PERSIST, persist_detail(ptile, pkch, C, Cout, M, dt, odt, False, ld)), (geom, dt, odt, fam)
                ran += 1
        assert ran >= 15


# ------------------------------------------------------------------------------------------------ epilogues
@pytest.mark.parametrize("kernel", ["tile0", "tile3", "persistent"])
def test_forward_epilogues_exact(kernel):
    """bias, residual, accumulate, out-ReLU, bias + residual + ReLU, the operand prologue with and without ReLU, and the masked residual
    join of pfr_conv2d_dgrad_join.  The persistent kernel has no operand prologue (igemm_p_launch declines it): the prologue cases run
    on the tile kernels only, where the id must say PRO.  EPRE is taken exactly when bf16 -> bf16 rows are read back (join, accumulate)
    with Cout % 8 == 0 and ldy % 8 == 0; one accumulate case with ldy = 76 must take the plain flavour."""
    tile = {"tile0": 0, "tile3": 3}.get(kernel)
    kn = dict(igemm_p=0, igemm_tile=tile, igemm_kch=4) if tile is not None else dict(igemm_p=2, igemm_ptile=1, igemm_pkch=8, igemm_ppf=0)
    with knobs(**kn, **STREAM_OFF):
        for geom in O.EPI_GEOMS:
            N, H, W, C, Cout, R, stride, pad = geom
            K = R * R * C
            for epi in O.EPIS:
                c = O.fwd_case(geom, epi)
                has_pro = c["pro"] is not None
                if has_pro and tile is None:
                    continue
                for dt, odt in ((BF, BF), (F32, F32)) + (((BF, F32),) if has_pro else ()):
                    fam = run_fwd(c, dt, odt, None, "%s %s" % (kernel, epi))
                    rows_back = "join" in c["flags"] or "acc" in c["flags"]
                    if tile is not None:
                        want = (TILE, tile_detail(tile, 4, C, K, dt, odt, has_pro, rows_back, Cout, Cout))
                    else:
                        M = N * c["ohw"][0] * c["ohw"][1]
                        want = (PERSIST, persist_detail(1, 8, C, Cout, M, dt, odt, True, Cout))
                    assert fam == want, (geom, epi, dt, odt, fam, want)
                    if tile is not None and (dt, odt) == (BF, BF):
                        assert bool(fam[1] & 64) == rows_back and bool(fam[1] & 32) == has_pro
        if tile is not None:     # rows read back, but a pitch that is no multiple of 8: the plain flavour, padding columns intact
            geom = O.EPI_GEOMS[0]
            fam = run_fwd(O.fwd_case(geom, "acc"), BF, BF, 76, "%s acc ldy 76" % kernel)
            assert fam == (TILE, tile_detail(tile, 4, 64, 576, BF, BF, False, True, 72, 76)) and not fam[1] & 64


# ------------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("mode", [0, 2])
def test_data_gradient_exact(mode):
    """ops.conv2d_dgrad over pfr_weight_dgrad_layout weights, with and without accumulate: stride 1; stride 2 on odd extents (the plain
    dilated path); stride 2 on even extents (the parity-class path: with igemm_p = 2 the id must say persistent + pclass, with igemm_p = 0
    the tile kernel's pclass, which exists for R > 1 only); the stride-2 1x1, where only class (0, 0) has taps — the other classes must
    hold exact zeros without accumulate and the old values with it (the reference has exactly that); 7x7 stride 2 pad 3 at C = 8."""
    kn = dict(igemm_p=0, igemm_tile=3, igemm_kch=4) if mode == 0 else dict(igemm_p=2, igemm_ptile=3, igemm_pkch=8, igemm_ppf=0)
    with knobs(**kn, **STREAM_OFF):
        for geom in O.DGRAD_GEOMS:
            N, H, W, C, Cout, R, stride, pad = geom      # the launch reduces over Cout (its "C") and produces C channels (its "Cout")
            even = stride == 2 and H % 2 == 0 and W % 2 == 0
            for accumulate in (False, True):
                for dt in (BF, F32):
                    fam = run_dgrad(O.dgrad_case(geom, accumulate), dt, "igemm_p %d" % mode)
                    if mode == 0:
                        want = (TILE, tile_detail(3, 4, Cout, R * R * Cout, dt, dt, False, accumulate, C, C, even and R > 1))
                    else:
                        rows = N * (H // 2) * (W // 2) if even else N * H * W
                        want = (PERSIST, persist_detail(3, 8, Cout, C, rows, dt, dt, accumulate, C, even))
                    assert fam == want, (geom, accumulate, dt, fam, want)
                    if even and (mode == 2 or R > 1):
                        assert fam[1] & 256, "parity-class path not taken"


# ------------------------------------------------------------------------------------------------ streaming and halo kernels
def test_streaming_1x1_kernel_exact():
    """sconv = 2 (whenever eligible), checked against the integer reference directly; also the residual-join form"""
    with knobs(sconv=2):
        for geom in O.SCONV_GEOMS:
            fam = run_fwd(O.fwd_case(geom), BF, BF, None, "sconv")
            assert fam[0] == SCONV and fam[1] & 31 == 0, (geom, fam)
        for geom in O.SCONV_JOIN_GEOMS:
            fam = run_fwd(O.fwd_case(geom, "join"), BF, BF, None, "sconv join")
            assert fam[0] == SCONV and fam[1] & 31 == 1, (geom, fam)


def test_halo_staged_3x3_kernel_exact():
    with knobs(sconv=2, sconv3=1):
        for geom in O.SCONV3_GEOMS:
            fam = run_fwd(O.fwd_case(geom), BF, BF, None, "sconv3")
            assert fam == (SCONV3, 0), (geom, fam)
            fam = run_dgrad(O.dgrad_case(geom, False), BF, "sconv3")
            assert fam == (SCONV3, 0), (geom, fam)


def test_halo_staged_stem_kernel_exact():
    """(64, 32, 32): the smallest case of test_halo_staged_stem_kernel_bit_identical that pfr_sstem.hip takes — sstem_geom needs
    N * (H / 4) * (W / 8) >= 2048 4x8-pixel patches (one per wave of 512 workgroups), and 64 * 8 * 4 is exactly 2048; (300, 8, 8),
    (5, 112, 112) and (7, 60, 88) have fewer and fall to the tile kernel.  Channels 12..15 are zero (the space-to-depth padding).  Plain
    store, and the bias + ReLU inference epilogue (conv rounded to bf16, bias added in fp32, rounded: exact on integers)."""
    N, H, W = O.STEM_GEOM[:3]
    with knobs(sstem=1, sconv=1):
        fam = run_fwd(O.fwd_case(O.STEM_GEOM, "", (H, W), 12), BF, BF, None, "sstem")
        assert fam == (SSTEM, 0), fam
        fam = run_fwd(O.fwd_case(O.STEM_GEOM, "bias+relu", (H, W), 12), BF, BF, None, "sstem inference")
        assert fam == (SSTEM, 2), fam


def test_streaming_linear_kernel_exact():
    """slin = 2: plain, bias, bias + residual (the kernel's forms: a residual without a bias is not one of them and is not run)"""
    with knobs(slin=2):
        for geom in O.SLIN_GEOMS:
            for ep, epi in enumerate(("", "bias", "bias+res")):
                fam = run_fwd(O.fwd_case(geom, epi), BF, BF, None, "slin " + epi)
                assert fam[0] == SLIN and fam[1] & 7 == ep, (geom, epi, fam)


# ------------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("splits", [1, 3, 1000])
@pytest.mark.parametrize("tile", range(4))
def test_weight_gradient_tile_kernel_exact(tile, splits):
    """every forced tile x split count (1000 must clamp to ceil(M / 256): at least 256 reduction rows per split) on the forward table
    (Cout raised to the 16-byte chunk), stride 2 on odd and even extents, 7x7 at C = 8, M = 162, M = 588 and M = 1; scale 0.5 / 4
    with accumulate into an integer-valued dw on two of them"""
    with knobs(wgrad_tile=tile, wgrad_splits=splits, wgrad_big=0, swgrad=0, wgrad9=0):
        for gi, geom in enumerate(O.WGRAD_GEOMS):
            N, H, W, C, Cout, R, stride, pad = geom
            OH, OW = O.out_hw(H, W, R, R, stride, pad)
            M = N * OH * OW
            want = (WG_TILE, tile | (min(splits, (M + 255) // 256) << 8))
            for dt in (BF, F32):
                forms = [(1.0, False)] + ([(0.5, True), (4.0, True)] if gi in (0, 9) else [])
                for scale, acc in forms:
                    fam = run_wgrad(geom, dt, "", scale, acc, "wgrad tile %d splits %d" % (tile, splits))
                    assert fam == want, (geom, dt, fam, want)


def test_weight_gradient_other_kernels_exact():
    """wgrad_big = 2 at Cout = 256, KK = 576; swgrad = 2 on a 1x1 / stride-1 bf16 launch; wgrad9 in {0, 2} on 3x3 (W = 7, 9, 16: the 8-,
    16- and 32-pixel row slots); the fused-prologue form (its own kernel: id bit 2)"""
    with knobs(wgrad_big=2, swgrad=0, wgrad9=0, wgrad_tile=-1, wgrad_splits=0):
        for scale, acc in ((1.0, False), (0.5, True)):
            fam = run_wgrad(O.WGRAD_BIG_GEOM, BF, "", scale, acc, "wgrad_big")
            assert fam[0] == WG_BIG, fam
    with knobs(swgrad=2, wgrad_big=0, wgrad9=0, wgrad_tile=-1, wgrad_splits=0):
        for scale, acc in ((1.0, False), (4.0, True)):
            fam = run_wgrad(O.SWGRAD_GEOM, BF, "", scale, acc, "swgrad")
            assert fam[0] == SWGRAD and fam[1] >> 8 >= 8, fam
    for mode in (0, 2):
        with knobs(wgrad9=mode, swgrad=0, wgrad_big=0, wgrad_tile=-1, wgrad_splits=0):
            for geom in O.WGRAD9_GEOMS:
                for scale, acc in ((1.0, False), (0.5, True)):
                    fam = run_wgrad(geom, BF, "", scale, acc, "wgrad9 %d" % mode)
                    assert fam[0] == (WGRAD9 if mode else WG_TILE), (geom, mode, fam)
    with knobs(wgrad9=0, swgrad=0, wgrad_big=0, wgrad_tile=-1, wgrad_splits=0):
        for geom in O.WGRAD_PRO_GEOMS:
            for pro in ("pro", "prorelu"):
                for dt in (BF, F32):
                    fam = run_wgrad(geom, dt, pro, 1.0, False, "wgrad prologue")
                    assert fam[0] == WG_TILE and fam[1] & 4, (geom, pro, dt, fam)


# ------------------------------------------------------------------------------------------------ BatchNorm partials: the one exact consequence
@pytest.mark.parametrize("family", ["tile", "persistent", "sconv", "sconv3", "sstem"])
def test_statistics_launch_gives_the_exact_column_mean(family):
    """stats = True with integer data: every tile's column sum is an integer a kernel holds exactly, so the finalised mean can differ
    from the exact column mean only by the fp32 roundings of mean_t and of pfr_bn_finalize's merge sum_t rows_t * mean_t / M.  The
    issue's "1e-6 relative" has no scale for a column whose mean is near zero (the integer data are nearly zero-mean), so the bound
    asserted is the one those roundings give, per channel, with u = 2^-24:
        |mean - exact| <= u * ((P / 16 + 20) * S / M + max|y|),     S = sum_t |sum_t|   (P parts of mt rows)
    — merge_parts adds P / 16 products per lane, then 16 lanes, then divides (P / 16 + 17 roundings of partial sums bounded by S), a
    part's mean_t = shift + sum / rows carries two more (2 u |mean_t| + u |shift|, |shift| <= max|y| being a value of the column), one
    spare.  For the kernels whose parts are not consecutive rows (sconv's interleaved ranges, the halo kernels' patches) S is replaced by
    its upper bound sum |y|.  This is 3e-7 .. 4e-5 absolute here; a dropped or doubled row moves a mean by |y| / M >= 1.5e-5 * |y|.
    The stored output must still be exact.  One geometry per kernel family."""
    o = ops()
    cfg = {"tile": (dict(igemm_p=0, igemm_tile=3, igemm_kch=4, **STREAM_OFF), O.FWD_GEOMS[0], TILE),
           "persistent": (dict(igemm_p=2, igemm_ptile=3, igemm_pkch=8, igemm_ppf=0, **STREAM_OFF), O.FWD_GEOMS[0], PERSIST),
           "sconv": (dict(sconv=2), O.SCONV_GEOMS[2], SCONV), "sconv3": (dict(sconv=2, sconv3=1), O.SCONV3_GEOMS[1], SCONV3),
           "sstem": (dict(sstem=1, sconv=1), O.STEM_GEOM, SSTEM)}[family]
    kn, geom, want = cfg
    N, H, W, C, Cout, R, stride, pad = geom
    stem = family == "sstem"
    c = O.fwd_case(geom, "", (H, W) if stem else None, 12 if stem else None)
    ref = O.fwd_ref(c)
    with knobs(**kn):
        y, part = o.conv2d_fwd(dev(c["x"], BF), dev(c["w"], BF), stride=stride, pad=pad, out_hw=c["ohw"], stats=True)
        mt = o.conv2d_fwd.last_mt
        fam = last_id("stats " + family)
        coef = o.bn_finalize(part, mt, ref.numel() // Cout, None, None, 1e-5, 0.1, None, None)
        torch.cuda.synchronize()
    assert fam[0] == want and (want in (TILE, PERSIST) or fam[1] & (16 if want == SCONV else 1)), fam
    O.assert_exact(y, ref, "stats " + family)
    cols = ref.reshape(-1, Cout)
    M = cols.shape[0]
    P = (M + mt - 1) // mt
    if want in (TILE, PERSIST):
        S = sum(cols[t * mt:(t + 1) * mt].sum(0).abs() for t in range(P))
    else:
        S = cols.abs().sum(0)
    bound = 2.0 ** -24 * ((P / 16 + 20) * S / M + cols.abs().max(0).values)
    err = (coef[0].cpu().to(F64) - cols.mean(0)).abs()
    print("stats %s: P %d, worst |mean err| %.3e, bound there %.3e, worst err / bound %.3f" %
          (family, P, err.max().item(), bound[err.argmax()].item(), (err / bound).max().item()))
    assert bool((err <= bound).all())


# ------------------------------------------------------------------------------------------------ per-element rounding bound
def _real_case(geom, seed, dt, epi=False, ohw=None, zero_from=None):
    N, H, W, C, Cout, R, stride, pad = geom
    g = O.rng(seed)
    OH, OW = ohw or O.out_hw(H, W, R, R, stride, pad)
    rt = lambda t: t.to(dt).to(F64)                          # inputs pre-rounded to the compute dtype
    c = {"x": rt(torch.randn(N, H, W, C, generator=g)), "w": rt(torch.randn(Cout, R, R, C, generator=g) / (R * R * C) ** 0.5)}
    if zero_from is not None:
        c["x"][..., zero_from:] = 0
    c["bias"] = torch.randn(Cout, generator=g).float().to(F64) if epi else None
    c["res"] = rt(torch.randn(N, OH, OW, Cout, generator=g)) if epi == "bias+res" else None
    c["dy"] = rt(torch.randn(N, OH, OW, Cout, generator=g))
    return c


def _check_fwd_rounding(geom, dt, epi, want_family, what, ohw=None, zero_from=None):
    """epi: False (plain store), "bias+res" or "bias+relu".  K = R * S * C, A = conv(|x|, |w|).
    bf16 output: the epilogues round the accumulator to bf16 once (plain store: n_r = 1, |v| = |conv|) and, with post-ops, add bias and
    residual to that in fp32 and round again (n_r = 2, |v| = |conv| and |conv + bias + residual|, the value before the ReLU:
    pfr_igemm.hip epilogue "statistics see the value as stored", pfr_slin.hip "round to bf16, then add in fp32, round again",
    pfr_sstem.hip "added to the bf16-rounded result in the read-back pass").
    fp32 output: a plain store counts as one rounding of |y|; with post-ops the two fp32 additions round |conv + residual| and
    |conv + residual + bias| (n_r = 2).  The fp32 path's MFMA is the full-precision v_mfma_f32_32x32x2_f32 (products rounded once to
    fp32: inside the 2^-23 = 2 * 2^-24 per term of the accumulation bound)."""
    o = ops()
    N, H, W, C, Cout, R, stride, pad = geom
    c = _real_case(geom, 11 + C + Cout, dt, epi, ohw, zero_from)
    relu = epi == "bias+relu"
    conv = O.conv_fwd_ref(c["x"], c["w"], stride, pad, ohw)
    pre = O.conv_fwd_ref(c["x"], c["w"], stride, pad, ohw, c["bias"], c["res"])
    ref = pre.clamp_min(0) if relu else pre
    A = O.conv_fwd_ref(c["x"].abs(), c["w"].abs(), stride, pad, ohw)
    out = torch.full(ref.shape, float("nan"), device=DEV, dtype=dt)
    o.conv2d_fwd(dev(c["x"], dt), dev(c["w"], dt), stride=stride, pad=pad, out_hw=ref.shape[1:3], out=out, bias=dev(c["bias"], F32),
                 residual=dev(c["res"], dt), out_relu=relu)
    torch.cuda.synchronize()
    fam = last_id(what)
    assert fam[0] == want_family, (what, fam)
    if dt == BF:
        values = [conv, pre] if epi else [conv]
    else:
        values = ([conv + c["res"], pre] if c["res"] is not None else [pre]) if epi else [ref]
    O.assert_within(out, ref, O.rounding_bound(values, R * R * C, A, dt == BF), what)
    return fam


ROUND_GEOMS = [O.FWD_GEOMS[0], O.FWD_GEOMS[2], O.FWD_GEOMS[4]]


def _check_wgrad_rounding(geom, dt, want_family, what):
    """fp32 output.  K = M: the slabs of a split launch and their sum are one summation order of the same M products, which the
    accumulation bound M * 2^-23 * A (A = sum |dy| |x|, scaled) covers for any order; the reduce pass's multiplication by `scale`
    is the one rounding of the output value (n_r = 1, |v| = |dw|)."""
    o = ops()
    N, H, W, C, Cout, R, stride, pad = geom
    c = _real_case(geom, 31 + C, dt)
    M = c["dy"].numel() // Cout
    ref = O.conv_wgrad_ref(c["x"], c["dy"], R, R, stride, pad, None, 0.5)
    A = O.conv_wgrad_ref(c["x"].abs(), c["dy"].abs(), R, R, stride, pad, None, 0.5)
    dw = o.conv2d_wgrad(dev(c["x"], dt), dev(c["dy"], dt), R, R, stride, pad, scale=0.5)
    torch.cuda.synchronize()
    assert last_id(what)[0] == want_family, what
    O.assert_within(dw, ref, O.rounding_bound([ref], M, A, False), what)


@pytest.mark.parametrize("family", ["tile", "persistent", "sconv", "sconv3", "sstem", "slin", "dgrad", "wgrad", "wgrad_big", "swgrad", "wgrad9"])
def test_real_valued_results_within_the_derived_rounding_bound(family):
    """randn data pre-rounded to the compute dtype, one knob set per kernel family of the exact tests, three geometries each (the stem,
    wgrad-big and swgrad have one eligible geometry in this file: theirs); every element within
    sum over the n_r roundings of u_out * |v| + K * 2^-23 * A (conv_oracle.rounding_bound; n_r, |v|, K and A per case in the helpers'
    docstrings).  Stem (K = 256): plain store n_r = 1, bias + ReLU inference epilogue n_r = 2.
    Data gradient (tile kernel, plain store): n_r = 1, K = R * S * Cout."""
    o = ops()
    if family == "tile":
        with knobs(igemm_p=0, igemm_tile=0, igemm_kch=4, **STREAM_OFF):
            for geom in ROUND_GEOMS:
                for dt in (BF, F32):
                    for epi in (False, "bias+res"):
                        _check_fwd_rounding(geom, dt, epi, TILE, "round tile %s %s epi %s" % (geom, dt, epi))
    elif family == "persistent":
        with knobs(igemm_p=2, igemm_ptile=1, igemm_pkch=8, igemm_ppf=0, **STREAM_OFF):
            for geom in ROUND_GEOMS[:2] + [O.FWD_GEOMS[3]]:
                for dt in (BF, F32):
                    for epi in (False, "bias+res"):
                        _check_fwd_rounding(geom, dt, epi, PERSIST, "round persistent %s %s epi %s" % (geom, dt, epi))
    elif family == "sconv":
        with knobs(sconv=2):
            for geom in O.SCONV_GEOMS[:3]:
                _check_fwd_rounding(geom, BF, False, SCONV, "round sconv %s" % (geom,))
    elif family == "sconv3":
        with knobs(sconv=2, sconv3=1):
            for geom in O.SCONV3_GEOMS:
                _check_fwd_rounding(geom, BF, False, SCONV3, "round sconv3 %s" % (geom,))
    elif family == "sstem":
        hw = O.STEM_GEOM[1:3]
        with knobs(sstem=1, sconv=1):
            fam = _check_fwd_rounding(O.STEM_GEOM, BF, False, SSTEM, "round sstem plain", hw, 12)
            assert fam == (SSTEM, 0), fam
            fam = _check_fwd_rounding(O.STEM_GEOM, BF, "bias+relu", SSTEM, "round sstem bias + ReLU", hw, 12)
            assert fam == (SSTEM, 2), fam
    elif family == "slin":
        with knobs(slin=2):
            for geom in O.SLIN_GEOMS:
                _check_fwd_rounding(geom, BF, "bias+res", SLIN, "round slin %s" % (geom,))
    elif family == "dgrad":
        with knobs(igemm_p=0, igemm_tile=3, igemm_kch=4, **STREAM_OFF):
            for geom in O.DGRAD_GEOMS[:3]:
                N, H, W, C, Cout, R, stride, pad = geom
                for dt in (BF, F32):
                    c = _real_case(geom, 23 + C, dt)
                    ref = O.conv_dgrad_ref(c["dy"], c["w"], (H, W), stride, pad)
                    A = O.conv_dgrad_ref(c["dy"].abs(), c["w"].abs(), (H, W), stride, pad)
                    out = torch.full(ref.shape, float("nan"), device=DEV, dtype=dt)
                    o.conv2d_dgrad(dev(c["dy"], dt), o.weight_dgrad_layout(dev(c["w"], dt)), (H, W), stride, pad, R, R, out=out)
                    torch.cuda.synchronize()
                    assert last_id("round dgrad %s %s" % (geom, dt))[0] == TILE
                    O.assert_within(out, ref, O.rounding_bound([ref], R * R * Cout, A, dt == BF), "dgrad %s %s" % (geom, dt))
    elif family == "wgrad":
        with knobs(wgrad9=0, swgrad=0, wgrad_big=0):
            for geom in (O.WGRAD_GEOMS[0], O.WGRAD_GEOMS[2], O.WGRAD_GEOMS[9]):
                for dt in (BF, F32):
                    _check_wgrad_rounding(geom, dt, WG_TILE, "round wgrad %s %s" % (geom, dt))
    elif family == "wgrad_big":
        with knobs(wgrad_big=2, wgrad9=0, swgrad=0):
            _check_wgrad_rounding(O.WGRAD_BIG_GEOM, BF, WG_BIG, "round wgrad_big")
    elif family == "swgrad":
        with knobs(swgrad=2, wgrad9=0, wgrad_big=0):
            _check_wgrad_rounding(O.SWGRAD_GEOM, BF, SWGRAD, "round swgrad")
    else:
        with knobs(wgrad9=2, swgrad=0, wgrad_big=0):
            for geom in O.WGRAD9_GEOMS:
                _check_wgrad_rounding(geom, BF, WGRAD9, "round wgrad9 %s" % (geom,))
