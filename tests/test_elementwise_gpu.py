"""csrc/pfr_elementwise.hip and the normalisation kernels of csrc/pfr_head.hip on the device, through the C-ABI, each against an fp64 CPU
reference written out here from torch expressions and computed from inputs already rounded to the compute dtype.  Every engine and the
optimiser call these kernels on every step; the whole-model tests reach them only behind tolerances that cannot see a dropped tail
element or a wrong last channel.

Conventions (those of tests/test_se_gpu.py): output buffers are pre-filled with NaN, so an element the kernel does not write fails the
comparison; buffers with guard elements are NaN outside the view the kernel gets (sources: 5.0, so that an over-read cannot put a NaN
where a guard is expected); one print per case shows the measured errors.

Bounds (relative error in the L2 norm), those of tests/test_dwconv3_gpu.py and tests/test_se_gpu.py: tensors stored in the compute dtype
fp32 1e-5, bf16 4e-3 (one output rounding, 2⁻⁸); quantities accumulated in fp32 (column sums, parameter gradients) 1e-4; statistics as in
tests/test_dwconvk_gpu.py, |Δmean| <= 1e-4·std and variance 1e-4 relative against fp64 statistics of the stored input; pure data movement
and casts bit-exact.  Where a test needs another bound its docstring derives it."""
import functools
import re
import struct

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]
TOL_Y = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
TOL_G = 1e-4
NAN = float("nan")
ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
P = lambda t: 0 if t is None else t.data_ptr()
f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))      # a Python scalar as the C-ABI's `float` parameter receives it
EPS = f32(1e-5)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _kp(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def _err_arg():
    """what include/pfr_hip.h defines as the return value of a failed argument check"""
    from pets_face_recognition_amd._hip.lib import HEADER_PATH
    return int(re.search(r"#define\s+PFR_ERR_ARG\s+\((-?\d+)\)", open(HEADER_PATH).read()).group(1))


def _view(vals, off, fill=NAN):
    """vals (CPU) copied `off` elements behind a 16-byte boundary of a larger device allocation filled with `fill`: off = 0 is a
    16-byte-aligned view, off = 1 one that only the scalar paths take.  -> (whole allocation, view, index of the view's first element)"""
    lo = 16 // vals.element_size() + off
    base = torch.full((lo + vals.numel() + 1,), fill, dtype=vals.dtype, device=DEV)
    assert base.data_ptr() % 16 == 0
    base[lo:lo + vals.numel()] = vals.to(DEV)
    return base, base[lo:lo + vals.numel()], lo


def _guards(base, lo, n, fill=NAN):
    """the elements before and behind the view still hold the fill value"""
    g = torch.cat([base[:lo], base[lo + n:]]).float().cpu()
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def _same_bits(got, ref):
    """bit-identical, except that a NaN only has to be a NaN"""
    got, ref = got.cpu().contiguous(), ref.cpu().contiguous()
    if got.dtype != ref.dtype or got.shape != ref.shape:
        return False
    ng, nr = torch.isnan(got), torch.isnan(ref)
    it = torch.int16 if got.element_size() == 2 else torch.int32
    return bool(torch.equal(ng, nr) and torch.equal(got[~ng].view(it), ref[~nr].view(it)))


# ================================================================================================ 1. data movement
# fp32 bit patterns: exact round-to-nearest-even ties (down to even, up to even), values that round up into the next binade, the largest
# finite bf16, the tie and FLT_MAX that overflow to inf, subnormals (smallest, a bf16-representable one, ties), ±0, ±inf, NaN
_SPECIAL_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F7FFFFF, 0x3FFF8000, 0xBFFFC000, 0x7F7F0000,
                 0xFF7F0000, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0x7F7F7FFF, 0x00000001, 0x00400000, 0x00008000, 0x00018000, 0x80008001,
                 0x007FFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345]
CAST_PAIRS = [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.float32, torch.float32)]
CAST_BIG_N = 8 * 256 * 4096 + 8 * 256 + 5


def _cast_values(n, src):
    sp = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in _SPECIAL_BITS], dtype=torch.int32).view(torch.float32)
    k = sp.numel()
    if n < 2 * k:      # short vectors: a window of the list that moves with n
        x = sp[(torch.arange(n) + n) % k].clone()
    else:              # the list at both ends: the head runs on the vector path of an aligned call, the tail on the scalar path
        x = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
        x[:k] = sp
        x[n - k:] = sp.flip(0)
    return x.to(src)


def _cast_case(n, src, dst, offs):
    from pets_face_recognition_amd._hip import lib, dtype_id
    x = _cast_values(n, src)
    ref = x.to(dst)
    sb, sv, _ = _view(x, offs[0], fill=5.0)
    db, dv, lo = _view(torch.full((n,), NAN, dtype=dst), offs[1])
    lib.pfr_cast(P(sv), dtype_id(src), P(dv), dtype_id(dst), n, _stream())
    torch.cuda.synchronize()
    return _same_bits(dv, ref), _guards(db, lo, n)


@pytest.mark.parametrize("pair", CAST_PAIRS, ids=["f32-bf16", "bf16-f32", "f32-f32"])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2055])
def test_cast_bit_exact(n, pair):
    """pfr_cast against torch.Tensor.to, bit for bit (a NaN has to stay a NaN).  n: 1 (a single thread), 7 / 8 / 9 (below, at and above
    the 8 values a thread of the fp32 -> bf16 vector path takes), 2055 = 8 * 256 + 7 (more than one workgroup and a 7-element scalar
    tail).  Each n on 16-byte-aligned pointers and on views one element further on the source, the destination or both (the scalar
    path); the elements around every destination keep their NaN."""
    for offs in ((0, 0), (1, 0), (0, 1), (1, 1)):
        same, guards = _cast_case(n, pair[0], pair[1], offs)
        print(n, pair, offs, "bits equal", same, "guards intact", guards)
        assert same and guards, (n, pair, offs)


def test_cast_second_grid_stride_sweep():
    """n = 8*256*4096 + 8*256 + 5: the grid is capped at 4096 workgroups of 256 threads with 8 values each, so 2048 values go to a
    second sweep of the vector loop and 5 to the scalar tail (fp32 -> bf16, aligned); once more on offset views, where the scalar loop
    makes nine sweeps."""
    for offs in ((0, 0), (1, 1)):
        same, guards = _cast_case(CAST_BIG_N, torch.float32, torch.bfloat16, offs)
        print(CAST_BIG_N, offs, "bits equal", same, "guards intact", guards)
        assert same and guards, offs


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rc", [(1, 1), (1, 130), (63, 65), (64, 64), (65, 63), (129, 200), (512, 33)], **ids)
def test_transpose2d_bit_exact(rc, dtype):
    """pfr_transpose2d (64 x 64 tiles through LDS): one element; one row over three tiles; one below / at / one above the tile edge in
    either direction; several tiles both ways with ragged edges; a tall matrix of eight row tiles"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, cols = rc
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 1000 + cols)).to(dtype)
    xb, xv, _ = _view(x.reshape(-1), 0, fill=5.0)
    yb, yv, lo = _view(torch.full((rows * cols,), NAN, dtype=dtype), 0)
    lib.pfr_transpose2d(P(xv), P(yv), dtype_id(dtype), rows, cols, _stream())
    torch.cuda.synchronize()
    same, guards = _same_bits(yv.reshape(cols, rows), x.t().contiguous()), _guards(yb, lo, rows * cols)
    print(rc, dtype, "bits equal", same, "guards intact", guards)
    assert same and guards


def _copy2d_case(rows, cols, scale, acc, seed):
    from pets_face_recognition_amd._hip import lib
    lds, ldd = cols + 5, cols + 3
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(rows + 1, lds, generator=g)[:rows]          # (one row more: a device pointer also where rows = 0)
    prior = torch.randn(rows, ldd, generator=g)
    dst = _nan((rows + 1, ldd))          # (one row more: the element behind the last row's padding is a guard as well)
    if acc:
        dst[:rows, :cols] = prior[:, :cols].to(DEV)
    srcd = torch.cat([src, torch.full((1, lds), 5.0)]).to(DEV)
    lib.pfr_copy2d_f32(P(srcd), lds, P(dst), ldd, rows, cols, scale, acc, _stream())
    torch.cuda.synchronize()
    ref = src[:, :cols].double() * scale + (prior[:, :cols].double() if acc else 0.0)
    got = dst.cpu()
    return torch.equal(got[:rows, :cols], ref.float()) and bool(torch.isnan(got[:rows, cols:]).all()) and bool(torch.isnan(got[rows]).all())


def test_copy2d_f32_strided_exact():
    """pfr_copy2d_f32 with ld_src = cols + 5 and ld_dst = cols + 3 (different, both larger than cols), rows in {0, 1, 147}, cols in
    {0, 3, 64}, scale in {1, 0.125}, overwrite and accumulate; and 8200 x 64 = 524 800 elements, more than the 2048 x 256 threads of the
    capped grid (a second sweep).  Exact: a power-of-two scale is exact and the accumulating form is one correctly rounded fp32 addition
    (as a fused multiply-add it rounds the same exact sum).  The padding columns of dst keep their NaN."""
    for rows in (0, 1, 147):
        for cols in (0, 3, 64):
            for scale in (1.0, 0.125):
                for acc in (0, 1):
                    ok = _copy2d_case(rows, cols, scale, acc, rows * 100 + cols)
                    assert ok, (rows, cols, scale, acc)
    assert 8200 * 64 > 2048 * 256
    for acc in (0, 1):
        ok = _copy2d_case(8200, 64, 0.125, acc, 7)
        print("copy2d 8200x64 accumulate", acc, "exact", ok)
        assert ok


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 9, 8), (5, 3, 49, 4), (1, 32, 16, 32), (3, 1, 1, 4)], **ids)
def test_nhwc_to_nchw_f32(shape, accumulate):
    """pfr_nhwc_to_nchw_f32, (N, C, HW, Cp): RGB in 8-channel pixels; 735 outputs (three workgroups, the last ragged) from 4-channel
    pixels; no padding at all (Cp = C); a single channel and pixel.  Overwrite: bit-exact.  Accumulate: the sum with the prior contents
    within one fp32 ulp of the exact sum, asserted as |got - exact| <= 2^-24 |exact| (what a correctly rounded addition gives: half an
    ulp, and ulp(s) > 2^-24 |s|)."""
    from pets_face_recognition_amd._hip import lib
    N, C, HW, Cp = shape
    g = torch.Generator().manual_seed(N + C + HW + Cp)
    x = torch.randn(N, HW, Cp, generator=g)
    prior = torch.randn(N, C, HW, generator=g)
    yb, yv, lo = _view(prior.reshape(-1) if accumulate else torch.full((N * C * HW,), NAN), 0)
    xd = x.to(DEV)
    lib.pfr_nhwc_to_nchw_f32(P(xd), P(yv), N, C, HW, Cp, accumulate, _stream())
    torch.cuda.synchronize()
    got = yv.cpu().reshape(N, C, HW)
    moved = x[:, :, :C].permute(0, 2, 1).contiguous()
    assert _guards(yb, lo, N * C * HW)
    if not accumulate:
        assert torch.equal(got, moved)
    else:
        exact = moved.double() + prior.double()
        excess = ((got.double() - exact).abs() - 2.0 ** -24 * exact.abs()).max().item()
        print(shape, "accumulate: max excess over half an ulp", f"{excess:.2e}")
        assert excess <= 0


ADD_GRID_CAP = 8192      # pfr_add: `if (blocks > 8192) blocks = 8192`, 256 threads, one 16-byte chunk per thread and sweep


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_add(dtype):
    """pfr_add against the fp64 sum rounded once: n = kp (one chunk), 3 kp, 257 kp (a second workgroup with one live thread) and
    (256 * 8192 + 257) kp, above the 256 x 8192 chunks of the capped grid (a second sweep).  n % kp != 0 is refused with the header's
    PFR_ERR_ARG and the output keeps its NaN."""
    from pets_face_recognition_amd._hip import lib, dtype_id, PfrError
    kp, did, st = _kp(dtype), dtype_id(dtype), _stream()
    for nch in (1, 3, 257, 256 * ADD_GRID_CAP + 257):
        n = nch * kp
        g = torch.Generator().manual_seed(nch)
        a, b = torch.randn(n, generator=g).to(dtype), (torch.randn(n, generator=g) * 3).to(dtype)
        yb, yv, lo = _view(torch.full((n,), NAN, dtype=dtype), 0)
        ad, bd = a.to(DEV), b.to(DEV)
        lib.pfr_add(P(ad), P(bd), P(yv), did, n, st)
        torch.cuda.synchronize()
        e = rel(yv, a.double() + b.double())
        print("add", dtype, n, f"{e:.2e}")
        assert e <= TOL_Y[dtype] and _guards(yb, lo, n), (n, e)
    n = 3 * kp + 1
    a, y = torch.ones(n + kp, dtype=dtype, device=DEV), _nan((n + kp,), dtype)
    with pytest.raises(PfrError, match=rf"rc={_err_arg()}\)"):
        lib.pfr_add(P(a), P(a), P(y), did, n, st)
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


# ================================================================================================ 2. column sums
def _colsum_path(dtype, rows, C):
    """which of pfr_colsum's kernels a call with a workspace takes, from pfr_colsum_parts"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    parts = lib.pfr_colsum_parts(dtype_id(dtype), rows, C)
    if parts == 0:
        return "single", 0
    if C % _kp(dtype) == 0:
        assert parts == lib.pfr_colreduce_blocks(C, dtype_id(dtype), rows)       # the chunked kernel's row blocks
        return "chunked", parts
    assert parts == min(max(2048 // ((C + 63) // 64), 8), (rows + 255) // 256)     # one partial row per 256-row block, capped
    return "scalar", parts


def _colsum_input(rows, C, dtype):
    g = torch.Generator().manual_seed(rows * 1000 + C)
    return (torch.randn(rows, C, generator=g) + 3.0).to(dtype)       # offset 3 in every column: the sums do not cancel


def _colsum_run(x, dtype, accumulate, with_ws=True):
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = x.shape
    prior = torch.randn(C, generator=torch.Generator().manual_seed(C))
    ob, out, lo = _view(prior if accumulate else torch.full((C,), NAN), 0)
    nws = lib.pfr_colsum_ws_floats(rows, C) if with_ws else 0
    ws = _nan((nws,)) if nws else None
    xd = x.to(DEV)
    lib.pfr_colsum(P(xd), dtype_id(dtype), rows, C, P(out), accumulate, P(ws), _stream())
    torch.cuda.synchronize()
    ref = x.double().sum(0) + (prior.double() if accumulate else 0.0)
    return rel(out, ref), _guards(ob, lo, C), out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [8, 24, 96, 1000, 3, 6, 169])
def test_colsum_three_paths(C, dtype):
    """pfr_colsum, overwrite and accumulate, bound 1e-4 (fp32 accumulation).  C in {8, 24, 96, 1000} (multiples of the chunk width in
    both dtypes; 1000 = 15 full 64-column blocks and a ragged one): rows in {1, 3, 17, 256} take the single kernel (fewer rows than its
    four row lanes; 17 = one unrolled batch of 16 and a remainder; 256 the last single-kernel size), rows in {257, 4099} the chunked
    partials.  C in {3, 6, 169} (the Swin position-table head counts, no multiple of 4) at 4099 rows take the scalar partials.  The path
    of every case is asserted from pfr_colsum_parts.  Without a workspace 257 and 2048 rows take the single kernel."""
    scalar = C % 4 != 0
    for rows in ((4099,) if scalar else (1, 3, 17, 256, 257, 4099)):
        path, parts = _colsum_path(dtype, rows, C)
        assert path == ("scalar" if scalar else "single" if rows <= 256 else "chunked"), (rows, C, path)
        x = _colsum_input(rows, C, dtype)
        for acc in (0, 1):
            e, guards, _ = _colsum_run(x, dtype, acc)
            print("colsum", dtype, (rows, C), path, parts, "accumulate", acc, f"{e:.2e}")
            assert e <= TOL_G and guards, (rows, C, acc, e)
    if not scalar:
        for rows in (257, 2048):
            e, guards, _ = _colsum_run(_colsum_input(rows, C, dtype), dtype, 0, with_ws=False)
            print("colsum without workspace", dtype, (rows, C), f"{e:.2e}")
            assert e <= TOL_G and guards, (rows, C, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_colsum_deferred_batch_bit_identical(dtype):
    """pfr_colsum_partial + one pfr_colsum_final_batch over three tensors of different width, (4099, 96) chunked, (4099, 169) scalar,
    (300, 24) chunked with few parts, overwrite and accumulate mixed: bit-identical to pfr_colsum with a workspace on the same tensors.
    colsum_final_batch_kernel follows colsum_final_kernel's order of additions for that (four accumulators over rows r, r+16, r+32, r+48
    while a whole group of four is left, the last rows into the first); with its earlier eight pairwise-added accumulators the fp32
    (4099, 96) tensor, 129 partial rows, differed from pfr_colsum by up to 1.6e-7 relative (up to 64 partial rows the orders coincide)."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    did, st = dtype_id(dtype), _stream()
    shapes, accs = [(4099, 96), (4099, 169), (300, 24)], [0, 1, 0]
    xs = [_colsum_input(r, C, dtype) for r, C in shapes]
    want = [_colsum_run(x, dtype, a)[2] for x, a in zip(xs, accs)]
    outs, keep, raw = [], [], b""
    for x, a, (rows, C) in zip(xs, accs, shapes):
        parts = lib.pfr_colsum_parts(did, rows, C)
        assert parts > 0
        ws, xd = _nan((lib.pfr_colsum_ws_floats(rows, C),)), x.to(DEV)
        out = torch.randn(C, generator=torch.Generator().manual_seed(C)).to(DEV) if a else _nan((C,))
        lib.pfr_colsum_partial(P(xd), did, rows, C, P(ws), st)
        raw += struct.pack("<QQiiiiii", P(ws), P(out), parts, C, a, 0, 0, 0)
        outs.append(out)
        keep += [ws, xd]
    tab = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    lib.pfr_colsum_final_batch(P(tab), len(shapes), max(C for _, C in shapes), st)
    torch.cuda.synchronize()
    diff = [((o.double() - w.double()).abs() / w.double().abs()).max().item() for o, w in zip(outs, want)]
    print("colsum deferred batch against pfr_colsum", dtype, "largest relative difference per tensor", [f"{d:.2e}" for d in diff])
    for o, w, sh in zip(outs, want, shapes):
        assert torch.equal(o, w) and not torch.isnan(o).any(), sh


# ================================================================================================ 3. BatchNorm statistics
def _stats_excess(out, x, eps=EPS):
    """(mean excess, variance excess) over the bounds, <= 0 passes.  Mean: |Δmean| - 1e-4 std.  Variance, recovered from the fp32 invstd
    as 1 / invstd² - eps: |Δvar| - (1e-4 var + 1e-6 (var + eps)); the second term is what the fp32 invstd itself resolves of var + eps
    (rsqrt to 2 ulp, squared: 4 * 2 * 2^-24 < 1e-6) and is all that is left where the variance is 0."""
    x64 = x.double()
    mean_ref, var_ref = x64.mean(0), x64.var(0, unbiased=False)
    mean, invstd = out[0].double().cpu(), out[1].double().cpu()
    assert torch.isfinite(mean).all() and torch.isfinite(invstd).all()
    var = 1.0 / invstd.square() - eps
    dm = ((mean - mean_ref).abs() - 1e-4 * var_ref.sqrt()).max().item()
    dv = ((var - var_ref).abs() - (1e-4 * var_ref + 1e-6 * (var_ref + eps))).max().item()
    return dm, dv


def _stats_run(x, with_ws=True, gamma=None, beta=None, rm=None, rv=None, momentum=0.1):
    """pfr_bn_stats -> pfr_bn_finalize through ops.bn_stats / ops.bn_finalize (with_ws = False: the finalize without its grouping
    workspace, called directly).  -> ([4, C] mean / invstd / scale / shift, nparts, rows per part)"""
    from pets_face_recognition_amd._hip import lib, ops
    rows, C = x.shape
    xd = x.to(DEV)
    part, rpp = ops.bn_stats(xd)
    out = _nan((4, C))
    if with_ws:
        ops.bn_finalize(part, rpp, rows, gamma, beta, EPS, momentum, rm, rv, out=out)
    else:
        lib.pfr_bn_finalize(P(part), part.shape[0], rpp, C, float(rows), P(gamma), P(beta), EPS, momentum, P(rm), P(rv), P(out[0]), P(out[1]),
                            P(out[2]), P(out[3]), 0, _stream())
    torch.cuda.synchronize()
    return out, part.shape[0], rpp


def _stats_input(rows, C, dtype, far_mean=True):
    g = torch.Generator().manual_seed(rows * 10000 + C)
    x = torch.randn(rows, C, generator=g) * (0.5 + torch.rand(C, generator=g) * 2) + torch.randn(C, generator=g) * 2
    x[:, 1] = 2.5                           # a constant column: variance 0, and a mean that the merge reproduces exactly
    if far_mean and dtype == torch.float32:
        x[:, 2] = 1000.0 + torch.randn(rows, generator=g)      # mean 1000, std 1: what the shifted sums are for
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C", [8, 24, 88, 1408])
def test_bn_statistics_small_row_counts(C, dtype):
    """pfr_bn_stats -> pfr_bn_finalize at rows in {1, 2, 5, 257} (one row: variance 0 and invstd = 1 / sqrt(eps), finite; two; fewer
    rows than row lanes; one more than 256) and C in {8, 24, 88, 1408} (one bf16 chunk; no power of two; 88 and 1408 the EfficientNet
    widths, 1408 = more chunk columns than one workgroup's 256 in fp32).  Column 1 is constant (variance 0), column 2 has mean 1000 and
    standard deviation 1 in fp32."""
    for rows in (1, 2, 5, 257):
        x = _stats_input(rows, C, dtype)
        out, nparts, rpp = _stats_run(x)
        dm, dv = _stats_excess(out, x)
        print("bn stats", dtype, (rows, C), "parts", nparts, "x", rpp, f"mean excess {dm:.2e} var excess {dv:.2e}")
        assert dm <= 0 and dv <= 0, (rows, C, dm, dv)
        if rows == 1:
            assert torch.equal(out[0].cpu(), x[0].float())
            assert ((out[1].double().cpu() * EPS ** 0.5 - 1).abs() <= 1e-6).all()
        assert rel(out[2], out[1]) <= 1e-6 and rel(out[3], -out[0].double() * out[1].double()) <= 1e-6      # gamma = 1, beta = 0


@pytest.mark.parametrize("with_ws", [True, False], ids=["grouped", "direct"])
@pytest.mark.parametrize("rc", [(34496, 64), (2049, 1024)], **ids)
def test_bn_statistics_with_empty_trailing_partials(rc, with_ws):
    """fp32 [34496, 64] (batch 11 at 56 x 56: 512 parts of 68 rows, parts 508..511 start behind the last row) and [2049, 1024] (512 parts
    of 5 rows, parts 410..511 empty): pfr_bn_stats rounds rows / parts up, so (nparts - 1) * rpp >= rows, which is asserted from the
    library's own queries.  The finalize has to count 0 rows for the empty parts; with total - i * rpp, which is negative there, the
    merged row count of the first geometry is 33896 instead of 34496; measured before the counts were clamped at 0: |Δmean| up to 0.073 std
    (grouped) / 0.117 std (direct) and the variance up to 0.13 / 0.47 (absolute) beyond its bound there, |Δmean| up to 9.5 std at [2049, 1024]; with the clamp
    |Δmean| <= 1e-6 std.  Both merges: grouped (512 parts > 256: with the
    workspace) and direct (no workspace: the strided loop)."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = rc
    nparts, rpp = lib.pfr_colreduce_blocks(C, dtype_id(torch.float32), rows), lib.pfr_bn_stats_rows_per_part(C, dtype_id(torch.float32), rows)
    assert (nparts - 1) * rpp >= rows, (nparts, rpp)
    x = _stats_input(rows, C, torch.float32, far_mean=False)
    out, np_, rpp_ = _stats_run(x, with_ws=with_ws)
    assert (np_, rpp_) == (nparts, rpp)
    dm, dv = _stats_excess(out, x)
    m_err = ((out[0].double().cpu() - x.double().mean(0)).abs() / x.double().std(0, unbiased=False))[2:].max().item()
    print("bn stats", rc, "parts", nparts, "x", rpp, "empty", nparts - (rows + rpp - 1) // rpp, f"mean excess {dm:.2e} var excess {dv:.2e}",
          f"max |Δmean| / std {m_err:.2e}")
    assert dm <= 0 and dv <= 0, (dm, dv)


def test_bn_running_statistics_two_rows():
    """the running-statistics update at rows = 2 (unbiased factor 2 / 1, the largest there is) against F.batch_norm's in fp64, 1e-4"""
    C = 24
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, C, generator=g) * 2 + 1
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    out, _, _ = _stats_run(x, rm=rm, rv=rv, momentum=f32(0.1))
    rm64, rv64 = rm0.double(), rv0.double()
    F.batch_norm(x.double(), rm64, rv64, None, None, training=True, momentum=f32(0.1), eps=EPS)
    e = dict(rm=rel(rm, rm64), rv=rel(rv, rv64))
    print("bn running stats", {k: f"{v:.2e}" for k, v in e.items()})
    assert all(v <= TOL_G for v in e.values()), e


# ================================================================================================ 4. BatchNorm apply / backward
BAND = 2.0 ** -8       # one bf16 ulp at 1, the scale of the pre-activations (gamma about 1, x̂ of unit variance)


@functools.lru_cache(maxsize=None)
def _bn_case(rc, dtype):
    """fp64 autograd of A: relu(bn(x)), B: relu(bn(x) + res), C: bn(x) + res and forward of D: relu(bn(x) + a2 res + b2).  Where the
    pre-activation of A / B lies within BAND of 0 the ReLU mask of a correct kernel may differ from the reference's; those elements are
    taken out of the comparison by giving them dout = 0 (the only way to take them out of the dgamma / dbeta sums as well).  `share` is
    their fraction."""
    rows, C = rc
    g = torch.Generator().manual_seed(rows * 1000 + C + 1)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).to(dtype)
    res = torch.randn(rows, C, generator=g).to(dtype)
    dout = torch.randn(rows, C, generator=g).to(dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    a2, b2 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    x64, r64, g64, b64 = (t.double().requires_grad_() for t in (x, res, gamma, beta))
    u = F.batch_norm(x64, None, None, g64, b64, training=True, eps=EPS)
    z = u + r64
    out = dict(x=x, res=res, gamma=gamma, beta=beta, a2=a2, b2=b2, u=u.detach(), z=z.detach(), yA=F.relu(u).detach(), yB=F.relu(z).detach(),
               yC=z.detach(), yD=F.relu(u + a2.double() * r64 + b2.double()).detach())
    share = 0.0
    for k, pre, y in (("A", u, F.relu(u)), ("B", z, F.relu(z)), ("C", z, z)):
        band = pre.detach().abs() <= BAND if k != "C" else torch.zeros_like(pre, dtype=torch.bool)
        d = torch.where(band, torch.zeros_like(dout), dout)
        share = max(share, band.double().mean().item())
        gr = torch.autograd.grad(y, (x64, r64, g64, b64), d.double(), retain_graph=True, allow_unused=True)
        out.update({"dout" + k: d, "band" + k: band, "dx" + k: gr[0], "gres" + k: gr[1], "dg" + k: gr[2], "db" + k: gr[3]})
    out["share"] = share
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("rc", [(5, 8), (70, 24), (257, 88), (33, 1408)], **ids)
def test_bn_act_and_backward_all_mask_modes(rc, dtype):
    """pfr_bn_act (one operand; with the residual; with a scaled second operand), pfr_bn_act_mask (the bit mask) and pfr_bn_bwd_reduce /
    finalize / apply in mask modes 0 (none: bn(x) + res), 1 (stored output > 0), 2 (recomputed scale x + shift > 0: relu(bn(x))) and 3 (the
    bit mask), against fp64 autograd.  (rows, C): (5, 8) fewer rows than row lanes, one bf16 chunk; (70, 24) and (257, 88) widths that are
    no power of two, 257 = one more than the 256 rows of the first unrolled sweep; (33, 1408) more fp32 chunk columns than one workgroup
    holds.  Elements whose reference pre-activation lies within one bf16 ulp (2^-8) of 0 are excluded (dout = 0 there); their share has to
    stay below 1 %, which the seeds satisfy in the fp64 reference alone: 0 of 40, 0.36 %, 0.29 %, 0.32 % with fp32 inputs and 0, 0.30 %, 0.28 %, 0.32 % with bf16 inputs."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = rc
    c = _bn_case(rc, dtype)
    assert c["share"] < 0.01, c["share"]
    did, st, kp = dtype_id(dtype), _stream(), _kp(dtype)
    x, res, gamma, beta, a2, b2 = (c[k].to(DEV) for k in ("x", "res", "gamma", "beta", "a2", "b2"))
    nb = lib.pfr_colreduce_blocks(C, did, rows)
    sp, f = _nan((nb, 2, C)), _nan((4, C))       # f: mean, invstd, scale, shift
    lib.pfr_bn_stats(P(x), did, rows, C, P(sp), st)
    lib.pfr_bn_finalize(P(sp), nb, lib.pfr_bn_stats_rows_per_part(C, did, rows), C, float(rows), P(gamma), P(beta), EPS, 0.1, 0, 0, P(f[0]),
                        P(f[1]), P(f[2]), P(f[3]), 0, st)
    yA, yB, yBm, yC, yD = (_nan((rows, C), dtype) for _ in range(5))
    mask = torch.full((rows, C // kp), 0xAA, dtype=torch.uint8, device=DEV)
    lib.pfr_bn_act(P(x), P(f[2]), P(f[3]), 0, 0, 0, P(yA), did, rows, C, 1, st)
    lib.pfr_bn_act(P(x), P(f[2]), P(f[3]), P(res), 0, 0, P(yB), did, rows, C, 1, st)
    lib.pfr_bn_act_mask(P(x), P(f[2]), P(f[3]), P(res), 0, 0, P(yBm), P(mask), did, rows, C, 1, st)
    lib.pfr_bn_act(P(x), P(f[2]), P(f[3]), P(res), 0, 0, P(yC), did, rows, C, 0, st)
    lib.pfr_bn_act(P(x), P(f[2]), P(f[3]), P(res), P(a2), P(b2), P(yD), did, rows, C, 1, st)
    torch.cuda.synchronize()
    e = dict(yA=rel(yA, c["yA"]), yB=rel(yB, c["yB"]), yC=rel(yC, c["yC"]), yD=rel(yD, c["yD"]))
    assert torch.equal(yBm, yB)
    bits = ((mask.cpu().int()[:, :, None] >> torch.arange(kp, dtype=torch.int32)) & 1).reshape(rows, C).bool()
    assert torch.equal(bits[~c["bandB"]], (c["z"] > 0)[~c["bandB"]])
    eg = {}
    for mode, k, outp in ((0, "C", 0), (1, "B", P(yB)), (2, "A", 0), (3, "B", P(mask))):
        dout = c["dout" + k].to(DEV)
        part, coef, dg, db = _nan((nb, 2, C)), _nan((3, C)), _nan((C,)), _nan((C,))
        dx, gres = _nan((rows, C), dtype), (_nan((rows, C), dtype) if k != "A" else None)
        lib.pfr_bn_bwd_reduce(P(dout), outp, P(x), P(f[0]), P(f[1]), P(f[2]), P(f[3]), mode, did, rows, C, P(part), st)
        lib.pfr_bn_bwd_finalize(P(part), nb, C, float(rows), P(gamma), P(f[0]), P(f[1]), P(dg), P(db), P(coef), 0, st)
        lib.pfr_bn_bwd_apply(P(dout), outp, P(x), P(coef), P(f[2]), P(f[3]), mode, P(dx), P(gres), did, rows, C, st)
        torch.cuda.synchronize()
        e[f"dx{mode}"] = rel(dx, c["dx" + k])
        if gres is not None:
            e[f"gres{mode}"] = rel(gres, c["gres" + k])
        eg[f"dg{mode}"], eg[f"db{mode}"] = rel(dg, c["dg" + k]), rel(db, c["db" + k])
    print(rc, dtype, f"excluded {c['share']:.4f}", {k: f"{v:.2e}" for k, v in {**e, **eg}.items()})
    assert all(v <= TOL_Y[dtype] for v in e.values()), e
    assert all(v <= TOL_G for v in eg.values()), eg


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_bn_eval_coeff_and_fold_bn(dtype):
    """pfr_bn_eval_coeff and pfr_fold_bn, three descriptors in one launch, (Cout, K) = (8, 27) gamma null, fp32 source; (24, 1) beta null,
    source in the compute dtype, K = 1 (every element writes a bias); (130, 577) both given, fp32 source, 75 010 elements = five sweeps of
    the 64 x 256 threads per descriptor.  running_var holds 1e-12 in every fifth channel next to eps = 1e-5.  Reference, the kernel's header
    comment in fp64: w' = w γ / sqrt(rv + eps), b' = β - rm γ / sqrt(rv + eps).  Folded weights 1e-5 / 4e-3, bias, scale and shift 1e-5."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    did, st = dtype_id(dtype), _stream()
    g = torch.Generator().manual_seed(17)
    raw, cases = b"", []
    for (co, k), has_g, has_b, src_f32 in (((8, 27), False, True, 1), ((24, 1), True, False, 0), ((130, 577), True, True, 1)):
        w = torch.randn(co, k, generator=g)
        w = w if src_f32 else w.to(dtype)
        gamma, beta = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
        rm, rv = torch.randn(co, generator=g), torch.rand(co, generator=g) + 0.1
        rv[::5] = 1e-12
        sc = (gamma.double() if has_g else 1.0) / (rv.double() + EPS).sqrt()
        ref_w, ref_b = w.double() * sc[:, None], (beta.double() if has_b else 0.0) - rm.double() * sc
        d = dict(w=w.to(DEV), gamma=gamma.to(DEV) if has_g else None, beta=beta.to(DEV) if has_b else None, rm=rm.to(DEV), rv=rv.to(DEV),
                 wout=_nan((co, k), dtype), bout=_nan((co,)), coef=_nan((2, co)), ref_w=ref_w, ref_b=ref_b, ref_s=sc, shape=(co, k))
        raw += struct.pack("<QQQQQQQqqfi", P(d["w"]), P(d["gamma"]), P(d["beta"]), P(d["rm"]), P(d["rv"]), P(d["wout"]), P(d["bout"]), co, k, EPS,
                           src_f32)
        lib.pfr_bn_eval_coeff(co, P(d["gamma"]), P(d["beta"]), P(d["rm"]), P(d["rv"]), EPS, P(d["coef"][0]), P(d["coef"][1]), st)
        cases.append(d)
    assert len(raw) == 3 * 80
    tab = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    lib.pfr_fold_bn(P(tab), 3, did, st)
    torch.cuda.synchronize()
    for d in cases:
        e = dict(w=rel(d["wout"], d["ref_w"]), b=rel(d["bout"], d["ref_b"]), scale=rel(d["coef"][0], d["ref_s"]), shift=rel(d["coef"][1], d["ref_b"]))
        print("fold", dtype, d["shape"], {k: f"{v:.2e}" for k, v in e.items()})
        assert e["w"] <= TOL_Y[dtype] and max(e["b"], e["scale"], e["shift"]) <= 1e-5, e


# ================================================================================================ 5. pools
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", [(1, 1, 8), (3, 49, 24), (2, 35, 1408), (65, 4, 16)], **ids)
def test_avgpool_forward_backward(shape, dtype):
    """pfr_avgpool_fwd / pfr_avgpool_bwd, (N, HW, C): one pixel of one bf16 chunk; a 7 x 7 map; the EfficientNet-B2 head width at an odd
    pixel count; 65 images x 2..4 chunks = more (n, chunk) pairs than one 64-thread workgroup of the forward kernel"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, HW, C = shape
    g = torch.Generator().manual_seed(N * 100 + HW + C)
    x, dy = (torch.randn(N, HW, C, generator=g) + 0.5).to(dtype), torch.randn(N, C, generator=g).to(dtype)
    yb, y, ylo = _view(torch.full((N * C,), NAN, dtype=dtype), 0)
    db, dx, dlo = _view(torch.full((N * HW * C,), NAN, dtype=dtype), 0)
    xd, dyd = x.to(DEV), dy.to(DEV)
    lib.pfr_avgpool_fwd(P(xd), P(y), dtype_id(dtype), N, HW, C, _stream())
    lib.pfr_avgpool_bwd(P(dyd), P(dx), dtype_id(dtype), N, HW, C, _stream())
    torch.cuda.synchronize()
    e = dict(y=rel(y.reshape(N, C), x.double().mean(1)), dx=rel(dx.reshape(N, HW, C), (dy.double() / HW)[:, None, :].expand(N, HW, C)))
    print("avgpool", shape, dtype, {k: f"{v:.2e}" for k, v in e.items()})
    assert all(v <= TOL_Y[dtype] for v in e.values()), e
    assert _guards(yb, ylo, N * C) and _guards(db, dlo, N * HW * C)


def test_avgpool_rejects_a_ragged_width():
    """C = 12 in bf16 is no multiple of the 8-channel chunk: both entry points refuse it with PFR_ERR_ARG and leave the output untouched
    (they used to pool channels 0..7 and skip 8..11 silently); an empty batch is a no-op"""
    from pets_face_recognition_amd._hip import lib, dtype_id, PfrError
    did, st = dtype_id(torch.bfloat16), _stream()
    x, y, dx = torch.ones(2, 5, 12, dtype=torch.bfloat16, device=DEV), _nan((2, 12), torch.bfloat16), _nan((2, 5, 12), torch.bfloat16)
    with pytest.raises(PfrError, match=rf"rc={_err_arg()}\)"):
        lib.pfr_avgpool_fwd(P(x), P(y), did, 2, 5, 12, st)
    with pytest.raises(PfrError, match=rf"rc={_err_arg()}\)"):
        lib.pfr_avgpool_bwd(P(x), P(dx), did, 2, 5, 12, st)
    lib.pfr_avgpool_fwd(P(x), P(y), did, 0, 5, 16, st)
    lib.pfr_avgpool_bwd(P(x), P(dx), did, 0, 5, 16, st)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(dx).all()


# ================================================================================================ 6. L2 normalisation
L2_EPS = f32(1e-12)
L2_REG_D = [4, 252, 512, 516, 2048]      # register path (fp32 in, no transposed copy): one float4; the last lane ragged below 512 = 2 x 64 float4;
#                                          exactly the two-chunk kernel's capacity; the first size of the eight-chunk kernel; its capacity
L2_WAVE_D = [1, 3, 510, 2052]            # wave kernel: one element; fewer than a float4; no multiple of 4; above the register path's limit
L2_ROWS = [1, 4, 5, 33]                  # one wave; one full workgroup of four; a second with one live wave; nine workgroups


def _l2_input(rows, D, dtype, zero_row=True):
    x = torch.randn(rows, D, generator=torch.Generator().manual_seed(rows * 10000 + D)).to(dtype)
    if zero_row and rows >= 4:
        x[2] = 0
    return x


def _l2_fwd_case(rows, D, in_dt, out_dt, ldt=0):
    from pets_face_recognition_amd._hip import lib, dtype_id
    x = _l2_input(rows, D, in_dt)
    xn, inv = _nan((rows, D), out_dt), _nan((rows,))
    xnT = _nan((D, ldt), out_dt) if ldt else None
    xd = x.to(DEV)
    lib.pfr_l2norm_fwd(P(xd), dtype_id(in_dt), P(xn), P(xnT), dtype_id(out_dt), P(inv), rows, D, ldt, L2_EPS, _stream())
    torch.cuda.synchronize()
    x64 = x.double()
    live = x64.norm(dim=1) > 0
    e = dict(xn=rel(xn, F.normalize(x64, eps=L2_EPS)), inv=rel(inv[live.to(DEV)], 1.0 / x64.norm(dim=1)[live]))
    assert not torch.isnan(xn).any()
    if (~live).any():       # an all-zero row: output 0 and inv_norm = 1 / eps
        assert (xn.cpu()[~live] == 0).all() and ((inv.double().cpu()[~live] * L2_EPS - 1).abs() <= 1e-6).all()
    if ldt:
        assert torch.equal(xnT[:, :rows], xn.t()) and torch.isnan(xnT[:, rows:]).all()
    return e


@pytest.mark.parametrize("D", L2_REG_D + L2_WAVE_D)
def test_l2norm_forward_dispatch(D):
    """pfr_l2norm_fwd against fp64 F.normalize over its dispatch, rows in {1, 4, 5, 33}: fp32 -> fp32 and fp32 -> bf16 (the register path for
    D % 4 == 0, D <= 2048, else the wave kernel) and bf16 -> bf16 (always the wave kernel).  xn: 1e-5 / 4e-3 by the output dtype; inv_norm
    1e-5.  Row 2 is all zero where there are four rows or more."""
    for rows in L2_ROWS:
        for in_dt, out_dt in ((torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16)):
            e = _l2_fwd_case(rows, D, in_dt, out_dt)
            print("l2norm", (rows, D), in_dt, out_dt, {k: f"{v:.2e}" for k, v in e.items()})
            assert e["xn"] <= TOL_Y[out_dt] and e["inv"] <= 1e-5, (rows, D, e)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_l2norm_forward_transposed_copy(dtype):
    """D = 512 with the transposed output at ldt = rows + 7 > rows: the wave kernel although the register path could take the size; xnT
    holds the same bits as xn, its padding columns keep their NaN"""
    for rows in L2_ROWS:
        e = _l2_fwd_case(rows, 512, dtype, dtype, ldt=rows + 7)
        print("l2norm + transposed", (rows, 512), dtype, {k: f"{v:.2e}" for k, v in e.items()})
        assert e["xn"] <= TOL_Y[dtype] and e["inv"] <= 1e-5, (rows, e)


@pytest.mark.parametrize("D", L2_REG_D)
def test_l2norm_dual_outputs_agree(D):
    """pfr_l2norm_dual writing both outputs: the bf16 row is the fp32 row cast with round-to-nearest-even, bit for bit, and inv_norm is
    bit-identical to the one pfr_l2norm_fwd returns on the same rows"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    for rows in L2_ROWS:
        x = _l2_input(rows, D, torch.float32).to(DEV)
        xb, xf, inv = _nan((rows, D), torch.bfloat16), _nan((rows, D)), _nan((rows,))
        xn2, inv2 = _nan((rows, D)), _nan((rows,))
        lib.pfr_l2norm_dual(P(x), P(xb), P(xf), P(inv), rows, D, L2_EPS, _stream())
        lib.pfr_l2norm_fwd(P(x), dtype_id(torch.float32), P(xn2), 0, dtype_id(torch.float32), P(inv2), rows, D, 0, L2_EPS, _stream())
        torch.cuda.synchronize()
        e = rel(xf, F.normalize(x.double().cpu(), eps=L2_EPS))
        print("l2norm dual", (rows, D), f"{e:.2e}")
        assert e <= 1e-5 and not torch.isnan(xf).any()
        assert _same_bits(xb, xf.cpu().to(torch.bfloat16)) and torch.equal(inv, inv2) and torch.equal(xf, xn2)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("D", L2_REG_D + L2_WAVE_D)
def test_l2norm_backward(D, accumulate):
    """pfr_l2norm_bwd against fp64 autograd of F.normalize, fp32 -> fp32 and bf16 -> bf16, rows in {1, 4, 5, 33}, overwrite and accumulate
    onto prior contents; inv_norm is the reference's, rounded to fp32.  Bound 1e-5 / 4e-3 relative to the reference gradient.  D = 1: the
    gradient is the difference of two equal terms, exactly 0 in the reference, so the error is taken relative to those terms,
    |inv_norm dxn|, with the same bound."""
    from pets_face_recognition_amd._hip import lib, dtype_id
    for rows in L2_ROWS:
        for dtype in DTYPES:
            x = _l2_input(rows, D, dtype, zero_row=False)
            g = torch.Generator().manual_seed(rows + D)
            dxn, prior = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g).to(dtype)
            x64 = x.double().requires_grad_()
            ref, = torch.autograd.grad(F.normalize(x64, eps=L2_EPS), x64, dxn.double())
            inv = (1.0 / x.double().norm(dim=1)).float()
            dx = prior.to(DEV) if accumulate else _nan((rows, D), dtype)
            xd, invd, dxnd = x.to(DEV), inv.to(DEV), dxn.to(DEV)
            lib.pfr_l2norm_bwd(P(xd), dtype_id(dtype), P(invd), P(dxnd), P(dx), dtype_id(dtype), rows, D, accumulate, _stream())
            torch.cuda.synchronize()
            want = ref + (prior.double() if accumulate else 0.0)
            den = want.norm() if D > 1 or accumulate else (inv.double()[:, None] * dxn.double()).norm()
            e = ((dx.double().cpu() - want).norm() / den).item()
            print("l2norm bwd", (rows, D), dtype, "accumulate", accumulate, f"{e:.2e}")
            assert e <= TOL_Y[dtype], (rows, D, dtype, e)


# ================================================================================================ 7. optimiser steps
OPT_BIG_N = 4 * 256 * 4096 + 4 * 256 + 3
LR_SGD, LR_ADAM, WD, MOM, GSCALE = f32(0.01), f32(1e-3), f32(1e-2), f32(0.9), f32(0.5)
B1, B2, ADAM_EPS, COEF, CLIPV = f32(0.9), f32(0.999), f32(1e-8), f32(0.6), f32(0.75)
AVG_W = [f32(0.75), f32(0.5), f32(0.2)]          # both branches of the two-branch lerp
OPT_KINDS = {
    # fn, momentum, first step flag on step 0, initial momentum buffer given, clip, avg
    "sgd_first": ("sgd", MOM, 1, False, False, False),
    "sgd_continue": ("sgd", MOM, 0, True, False, False),
    "sgd_no_momentum_first": ("sgd", 0.0, 1, False, False, False),
    "sgd_no_momentum": ("sgd", 0.0, 0, False, False, False),
    "sgd_clip": ("sgd", MOM, 1, False, True, False),
    "sgd_avg": ("sgd", MOM, 1, False, True, True),
    "sgd_avg_no_clip": ("sgd", MOM, 0, True, False, True),
    "adamw": ("adamw", 0.0, 0, False, False, False),
    "adamw_clip": ("adamw", 0.0, 0, False, True, False),
    "adamw_avg": ("adamw", 0.0, 0, False, True, True),
}


@functools.lru_cache(maxsize=None)
def _opt_case(kind, n):
    """inputs and the fp64 recurrence over three steps, from fp32-rounded inputs and scalars"""
    fn, momentum, first, has_mom0, clip, avg = OPT_KINDS[kind]
    g = torch.Generator().manual_seed(n % 100003 + len(kind))
    p0, grads = torch.randn(n, generator=g), [torch.randn(n, generator=g) * 2 for _ in range(3)]
    s0 = [torch.randn(n, generator=g) for _ in range(3)]           # initial momentum / exp_avg, exp_avg_sq (squared below), average
    c = dict(p0=p0, g=grads, mom0=s0[0] if has_mom0 else None, m0=s0[0] * 0.1, v0=s0[1].square() * 0.1, avg0=s0[2])
    p, a = p0.double(), s0[2].double()
    mom, m, v = s0[0].double(), c["m0"].double(), c["v0"].double()
    for i, gr in enumerate(grads):
        gg = gr.double() * GSCALE
        if clip:
            gg = (gg * COEF).clamp(-CLIPV, CLIPV)
        if fn == "sgd":
            d = WD * p + gg
            b = d if (momentum == 0.0 or (first and i == 0)) else momentum * mom + d
            mom = b
            p = p - LR_SGD * b
        else:
            p = p * (1.0 - LR_ADAM * WD)
            m = B1 * m + (1.0 - B1) * gg
            v = B2 * v + (1.0 - B2) * gg * gg
            p = p - (LR_ADAM / (1.0 - B1 ** (i + 1))) * m / (v.sqrt() / (1.0 - B2 ** (i + 1)) ** 0.5 + ADAM_EPS)
        a = a + AVG_W[i] * (p - a)
    c["ref"] = dict(p=p, mom=mom if (fn == "sgd" and momentum != 0.0) else None, m=m if fn == "adamw" else None, v=v if fn == "adamw" else None,
                    avg=a if avg else None)
    return c


def _opt_run(kind, sdt, n, off):
    """three steps on views `off` elements behind a 16-byte boundary -> ({name: result}, guards intact)"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    fn, momentum, first, has_mom0, clip, avg = OPT_KINDS[kind]
    c, st = _opt_case(kind, n), _stream()
    nanv = torch.full((n,), NAN)
    bufs = dict(p=_view(c["p0"], off), shadow=_view(nanv.to(sdt), off))
    if fn == "sgd" and momentum != 0.0:
        bufs["mom"] = _view(c["mom0"] if has_mom0 else nanv, off)       # first step: written, never read
    if fn == "adamw":
        bufs["m"], bufs["v"] = _view(c["m0"], off), _view(c["v0"], off)
    if avg:
        bufs["avg"] = _view(c["avg0"], off)
    gb = [_view(gr, off, fill=5.0) for gr in c["g"]]
    coef = torch.tensor([COEF], device=DEV) if clip else None
    clipv = CLIPV if clip else 0.0
    v = {k: b[1] for k, b in bufs.items()}
    for i in range(3):
        gr, fs = gb[i][1], int(bool(first) and i == 0)
        if fn == "sgd":
            head = (P(v["p"]), P(gr), P(v.get("mom")), P(v["shadow"]), dtype_id(sdt), n, LR_SGD, momentum, WD, GSCALE, fs)
            if avg:
                lib.pfr_sgd_step_avg(*head, P(coef), clipv, P(v["avg"]), AVG_W[i], st)
            elif clip:
                lib.pfr_sgd_step_clip(*head, P(coef), clipv, st)
            else:
                lib.pfr_sgd_step(*head, st)
        else:
            head = (P(v["p"]), P(gr), P(v["m"]), P(v["v"]), P(v["shadow"]), dtype_id(sdt), n, LR_ADAM, B1, B2, ADAM_EPS, WD, i + 1, GSCALE)
            if avg:
                lib.pfr_adamw_step_avg(*head, P(coef), clipv, P(v["avg"]), AVG_W[i], st)
            elif clip:
                lib.pfr_adamw_step_clip(*head, P(coef), clipv, st)
            else:
                lib.pfr_adamw_step(*head, st)
    torch.cuda.synchronize()
    guards = all(_guards(b, lo, n) for b, _, lo in bufs.values()) and all(_guards(b, lo, n, fill=5.0) for b, _, lo in gb)
    return {k: t.cpu() for k, t in v.items()}, guards


def _opt_check(kind, sdt, n):
    c = _opt_case(kind, n)
    a, ga = _opt_run(kind, sdt, n, 0)
    b, gb = _opt_run(kind, sdt, n, 1)
    e = {k: rel(a[k], r) for k, r in c["ref"].items() if r is not None}
    print("optimiser", kind, sdt, n, {k: f"{v:.2e}" for k, v in e.items()})
    assert ga and gb, "a guard element next to a view was overwritten"
    assert all(v <= 1e-6 for v in e.values()), e
    assert _same_bits(a["shadow"], a["p"].to(sdt)), "shadow is not the rounded-to-nearest-even copy of p"
    for k in a:      # 16-byte-aligned buffers (vector path) and views one element in (scalar path): the same bits
        assert _same_bits(a[k], b[k]), (k, "aligned and offset runs differ")


@pytest.mark.parametrize("sdt", DTYPES, ids=["shadow-fp32", "shadow-bf16"])
@pytest.mark.parametrize("kind", list(OPT_KINDS))
def test_optimizer_steps_over_sub_buffers(kind, sdt):
    """pfr_sgd_step (first_step 1 / 0, momentum 0.9 / 0), pfr_sgd_step_clip, pfr_sgd_step_avg (with and without clipping),
    pfr_adamw_step, pfr_adamw_step_clip, pfr_adamw_step_avg: three steps at n in {1, 3, 4, 5, 1023} (below, at and above the four values
    a thread of the SGD vector loop takes; 1023 = 255 vectors and a 3-element tail over four workgroups), against the same recurrence in
    fp64 from fp32-rounded inputs: 1e-6 on p, momentum, exp_avg, exp_avg_sq and the average.  The shadow is bit-equal to p (fp32) or to
    p rounded to nearest even (bf16).  Every run twice, in 16-byte-aligned views and in views one element further into their allocations
    (shadow and average too): all outputs bit-identical, and the elements before and behind every view untouched.  A momentum buffer
    that the first step only writes starts as NaN."""
    for n in (1, 3, 4, 5, 1023):
        _opt_check(kind, sdt, n)


@pytest.mark.parametrize("kind", ["sgd_avg", "adamw"])
def test_optimizer_second_grid_stride_sweep(kind):
    """n = 4*256*4096 + 4*256 + 3: the grids are capped at 4096 workgroups of 256 threads, so the SGD vector loop (four values a thread)
    makes a second sweep over 256 vectors and leaves a 3-element tail; the scalar loops (AdamW, and SGD on the offset views) make five.
    bf16 shadow; the checks of test_optimizer_steps_over_sub_buffers."""
    _opt_check(kind, torch.bfloat16, OPT_BIG_N)
