"""csrc/pfr_dwconv3.hip and the ReLU6 forms of the BatchNorm kernels on the device: depthwise 3x3 convolution, stride 1 and 2 (forward
with the BatchNorm + ReLU6 prologue and the statistics epilogue, data gradient, weight gradient with its accumulate flag) against
F.conv2d(groups=C, padding=1, stride=s) and autograd in fp64 on the CPU, computed from inputs already rounded to the compute dtype;
pfr_bn_act_clamp / pfr_bn_bwd_*_clamp against the autograd of F.hardtanh(F.batch_norm(x, training=True), 0, 6) in fp64.

Bounds (relative error in the L2 norm), those of tests/test_dwconv_gpu.py for the same reasons: forward and data gradient fp32 1e-5
(9 fp32 FMAs), bf16 4e-3 (one output rounding, 2⁻⁸); weight gradient, dgamma and dbeta 1e-4 in both dtypes (fp32 accumulation).
Statistics: |Δmean| <= 1e-4·std and variance 1e-4 relative against fp64 statistics of the STORED y."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 1, 16),
          (2, 2, 3, 24),
          (3, 7, 7, 960),     # MobileNetV2's last stage, odd N
          (2, 5, 9, 96),      # odd in both directions: at stride 2 the last column feeds no output through tap 2
          (1, 14, 14, 144),   # C no multiple of 32
          (2, 16, 16, 32),
          (1, 28, 30, 200)]
STRIDES = [1, 2]
DTYPES = [torch.float32, torch.bfloat16]
TOL_Y = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
TOL_G = 1e-4
ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _case(shape, stride, dtype):
    """inputs (rounded to dtype, NHWC) and the fp64 CPU references (plain and with the prologue), computed once per case"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape) * 7 + stride + (100 if dtype == torch.bfloat16 else 0))
    x0 = torch.randn(N, H, W, C, generator=g)
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).to(dtype)
    scale = torch.rand(C, generator=g) * 2 + 1          # [1, 3]
    shift = torch.rand(C, generator=g) * 2 + 0.5        # [0.5, 2.5]: clamp(shift) != 0, so padding before activating is wrong
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(N, OH, OW, C, generator=g).to(dtype)
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    for k in (2, 3, 4, 6, 10):     # x rescaled until the activated operand saturates at both ends (the small cases are few draws)
        x = (x0 * k).to(dtype)
        z = nchw(x) * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
        if (z >= 6).double().mean() >= 0.05 and (z <= 0).double().mean() >= 0.05:
            break
    x64, w64 = nchw(x).requires_grad_(), w.double().requires_grad_()
    y = F.conv2d(x64, w64, padding=1, stride=stride, groups=C)
    assert tuple(y.shape) == (N, C, OH, OW)
    dx, dw = torch.autograd.grad(y, (x64, w64), nchw(dy))
    a = z.clamp(0, 6)
    assert (z >= 6).double().mean() >= 0.05 and (z <= 0).double().mean() >= 0.05      # the upper clamp and the lower one are visible
    w64p = w.double().requires_grad_()
    yp = F.conv2d(a, w64p, padding=1, stride=stride, groups=C)
    dwp, = torch.autograd.grad(yp, w64p, nchw(dy))
    return dict(x=x, w=w, dy=dy, scale=scale, shift=shift, y=nhwc(y), dx=nhwc(dx), dw=dw, yp=nhwc(yp), dwp=dwp, OH=OH, OW=OW)


def _taps(w):
    return w.view(w.shape[0], 9).t().contiguous().to(DEV)


def _fwd(c, shape, stride, dtype, pro, stats=False):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    did = dtype_id(dtype)
    x, wt = c["x"].to(DEV), _taps(c["w"])
    sc, sh = c["scale"].to(DEV), c["shift"].to(DEV)
    y = _nan((N, c["OH"], c["OW"], C), dtype)
    part, rpp = None, 0
    if stats:
        rpp = lib.pfr_dwconv3_rows_per_part(did, N, H, W, C, stride)
        assert rpp >= 1
        part = _nan(((N * c["OH"] * c["OW"] + rpp - 1) // rpp, 2, C), torch.float32)
    lib.pfr_dwconv3_fwd(x.data_ptr(), wt.data_ptr(), y.data_ptr(), did, N, H, W, C, stride, sc.data_ptr() if pro else 0,
                        sh.data_ptr() if pro else 0, 6.0, part.data_ptr() if stats else 0, _stream())
    torch.cuda.synchronize()
    return y, part, rpp


def _wgrad(c, shape, stride, dtype, pro, dw, accumulate):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    did = dtype_id(dtype)
    parts = lib.pfr_dwconv3_wgrad_parts(did, N, H, W, C, stride)
    assert parts >= 1
    ws = _nan((parts, 9, C), torch.float32)
    x, dy, sc, sh = c["x"].to(DEV), c["dy"].to(DEV), c["scale"].to(DEV), c["shift"].to(DEV)
    lib.pfr_dwconv3_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), did, N, H, W, C, stride, sc.data_ptr() if pro else 0,
                          sh.data_ptr() if pro else 0, 6.0, accumulate, _stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("stride", STRIDES, ids=["s1", "s2"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_dwconv3_plain_forward_dgrad_wgrad(shape, stride, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    c = _case(shape, stride, dtype)
    y, _, _ = _fwd(c, shape, stride, dtype, pro=False)
    dx = _nan((N, H, W, C), dtype)
    dy = c["dy"].to(DEV)
    lib.pfr_dwconv3_dgrad(dy.data_ptr(), _taps(c["w"]).data_ptr(), dx.data_ptr(), dtype_id(dtype), N, H, W, C, stride, _stream())
    dw = _nan((C, 1, 3, 3), torch.float32)
    _wgrad(c, shape, stride, dtype, False, dw, 0)
    e = dict(y=rel(y, c["y"]), dx=rel(dx, c["dx"]), dw=rel(dw, c["dw"]))
    print(shape, stride, dtype, {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] <= TOL_Y[dtype] and e["dx"] <= TOL_Y[dtype], e
    assert e["dw"] <= TOL_G, e


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("stride", STRIDES, ids=["s1", "s2"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_dwconv3_prologue_forward_wgrad_and_border(shape, stride, dtype):
    """operand = relu6(scale*x + shift), padding of the ACTIVATED tensor: the border output pixels alone meet the forward bound"""
    N, H, W, C = shape
    c = _case(shape, stride, dtype)
    y, _, _ = _fwd(c, shape, stride, dtype, pro=True)
    dw = _nan((C, 1, 3, 3), torch.float32)
    _wgrad(c, shape, stride, dtype, True, dw, 0)
    border = torch.zeros(c["OH"], c["OW"], dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    e = dict(y=rel(y, c["yp"]), border=rel(y.cpu()[:, border], c["yp"][:, border]), dw=rel(dw, c["dwp"]))
    print(shape, stride, dtype, {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] <= TOL_Y[dtype] and e["border"] <= TOL_Y[dtype], e
    assert e["dw"] <= TOL_G, e


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("stride", STRIDES, ids=["s1", "s2"])
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_dwconv3_statistics_epilogue(shape, stride, dtype):
    """stats_part merged by pfr_bn_finalize (gamma = 1, beta = 0, eps = 0: invstd² = 1 / var) against fp64 statistics of the stored y;
    two runs are bit-identical (no atomics)"""
    from pets_face_recognition_amd._hip import lib
    N, H, W, C = shape
    c = _case(shape, stride, dtype)
    y, part, rpp = _fwd(c, shape, stride, dtype, pro=True, stats=True)
    y2, part2, _ = _fwd(c, shape, stride, dtype, pro=True, stats=True)
    assert torch.equal(y, y2) and torch.equal(part, part2) and torch.isfinite(part).all()
    assert rel(y, c["yp"]) <= TOL_Y[dtype]
    rows = N * c["OH"] * c["OW"]
    out = _nan((4, C), torch.float32)
    lib.pfr_bn_finalize(part.data_ptr(), part.shape[0], rpp, C, float(rows), 0, 0, 0.0, 0.1, 0, 0, out[0].data_ptr(), out[1].data_ptr(),
                        out[2].data_ptr(), out[3].data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    y64 = y.double().cpu().view(rows, C)
    mean_ref, var_ref = y64.mean(0), y64.var(0, unbiased=False)
    mean, var = out[0].double().cpu(), 1.0 / out[1].double().cpu().square()
    dm = ((mean - mean_ref).abs() - 1e-4 * var_ref.sqrt()).max().item()
    dv = ((var - var_ref).abs() - 1e-4 * var_ref).max().item()
    print(shape, stride, dtype, f"mean excess {dm:.2e} var excess {dv:.2e}")
    assert dm <= 0 and dv <= 0


def test_dwconv3_wgrad_accumulate_flag():
    shape, stride, dtype = (2, 5, 9, 96), 2, torch.float32
    c = _case(shape, stride, dtype)
    dw = _nan((96, 1, 3, 3), torch.float32)
    _wgrad(c, shape, stride, dtype, True, dw, 0)          # overwrite: NaN in the buffer does not survive
    assert torch.isfinite(dw).all() and rel(dw, c["dwp"]) <= TOL_G
    _wgrad(c, shape, stride, dtype, True, dw, 1)          # accumulate: the sum of both calls
    assert rel(dw, 2 * c["dwp"]) <= TOL_G


@functools.lru_cache(maxsize=None)
def _bn_case(rows, C, dtype):
    g = torch.Generator().manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).to(dtype)
    dout = torch.randn(rows, C, generator=g).to(dtype)
    gamma = torch.rand(C, generator=g) + 2.0            # z = gamma*xhat + beta with beta near 3: ~11 % beyond either bound
    beta = torch.rand(C, generator=g) + 2.5
    x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    z = F.batch_norm(x64, None, None, g64, b64, training=True, eps=1e-5)
    assert (z >= 6).double().mean() >= 0.05 and (z <= 0).double().mean() >= 0.05
    y = F.hardtanh(z, 0.0, 6.0)
    dx, dg, db = torch.autograd.grad(y, (x64, g64, b64), dout.double())
    return dict(x=x, dout=dout, gamma=gamma, beta=beta, y=y.detach(), dx=dx, dg=dg, db=db)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rc", [(37, 16), (196, 144), (98, 960)], **ids)
def test_bn_relu6_forward_backward(rc, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = rc
    c = _bn_case(rows, C, dtype)
    did, st = dtype_id(dtype), _stream()
    x, dout, gamma, beta = (c[k].to(DEV) for k in ("x", "dout", "gamma", "beta"))
    P = lambda t: t.data_ptr()
    sp = _nan((lib.pfr_colreduce_blocks(C, did, rows), 2, C), torch.float32)
    lib.pfr_bn_stats(P(x), did, rows, C, P(sp), st)
    f = _nan((4, C), torch.float32)      # mean, invstd, scale, shift
    lib.pfr_bn_finalize(P(sp), sp.shape[0], lib.pfr_bn_stats_rows_per_part(C, did, rows), C, float(rows), P(gamma), P(beta), 1e-5, 0.1, 0, 0,
                        P(f[0]), P(f[1]), P(f[2]), P(f[3]), 0, st)

    def run(hi, clamp):
        y, dx = _nan((rows, C), dtype), _nan((rows, C), dtype)
        part = _nan((lib.pfr_colreduce_blocks(C, did, rows), 2, C), torch.float32)
        coef, dg, db = _nan((3, C), torch.float32), _nan((C,), torch.float32), _nan((C,), torch.float32)
        if clamp:
            lib.pfr_bn_act_clamp(P(x), P(f[2]), P(f[3]), P(y), hi, did, rows, C, st)
            lib.pfr_bn_bwd_reduce_clamp(P(dout), P(x), P(f[0]), P(f[1]), P(f[2]), P(f[3]), hi, 2, did, rows, C, P(part), st)
        else:
            lib.pfr_bn_act(P(x), P(f[2]), P(f[3]), 0, 0, 0, P(y), did, rows, C, 1, st)
            lib.pfr_bn_bwd_reduce(P(dout), 0, P(x), P(f[0]), P(f[1]), P(f[2]), P(f[3]), 2, did, rows, C, P(part), st)
        lib.pfr_bn_bwd_finalize(P(part), part.shape[0], C, float(rows), P(gamma), P(f[0]), P(f[1]), P(dg), P(db), P(coef), 0, st)
        if clamp:
            lib.pfr_bn_bwd_apply_clamp(P(dout), P(x), P(coef), P(f[2]), P(f[3]), hi, 2, P(dx), did, rows, C, st)
        else:
            lib.pfr_bn_bwd_apply(P(dout), 0, P(x), P(coef), P(f[2]), P(f[3]), 2, P(dx), 0, did, rows, C, st)
        torch.cuda.synchronize()
        return y, part, dg, db, dx

    y, _, dg, db, dx = run(6.0, True)
    e = dict(y=rel(y, c["y"]), dx=rel(dx, c["dx"]), dg=rel(dg, c["dg"]), db=rel(db, c["db"]))
    print(rc, dtype, {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] <= TOL_Y[dtype] and e["dx"] <= TOL_Y[dtype], e
    assert e["dg"] <= TOL_G and e["db"] <= TOL_G, e
    # hi = 0: no upper bound — pfr_bn_act(relu = 1) and mask_mode 2 of pfr_bn_bwd_reduce / pfr_bn_bwd_apply, bit for bit
    for a, b in zip(run(0.0, True), run(0.0, False)):
        assert torch.equal(a, b)
    assert not torch.equal(y, run(0.0, True)[0])
    # mask_mode 0 (a BatchNorm without activation): every gradient passes
    part0, part1 = _nan((lib.pfr_colreduce_blocks(C, did, rows), 2, C), torch.float32), None
    lib.pfr_bn_bwd_reduce_clamp(P(dout), P(x), P(f[0]), P(f[1]), 0, 0, 0.0, 0, did, rows, C, P(part0), st)
    part1 = torch.empty_like(part0)
    lib.pfr_bn_bwd_reduce(P(dout), 0, P(x), P(f[0]), P(f[1]), 0, 0, 0, did, rows, C, P(part1), st)
    torch.cuda.synchronize()
    assert torch.equal(part0, part1)


def test_host_pointer_in_any_position_is_an_error_code():
    """every non-NULL pointer is checked before a launch: a host pointer next to real device pointers returns an error, no fault"""
    from pets_face_recognition_amd._hip import lib, PfrError
    N, H, W, C = 1, 4, 4, 8
    host = (ctypes.c_float * 8192)()
    hp = ctypes.addressof(host)
    d = lambda *s: torch.zeros(*s, device=DEV)
    x, y, w, a, b = d(N, H, W, C), d(N, H, W, C), d(9, C), d(C), d(C)
    dw, coef = d(C, 9), d(3, C)
    part = d(N * H * W, 2, C)
    ws = d(lib.pfr_dwconv3_wgrad_parts(0, N, H, W, C, 1), 9, C)
    st = _stream()
    P = lambda t: t.data_ptr()
    # (function, arguments with the pointer positions first marked by their index)
    calls = [
        (lib.pfr_dwconv3_fwd, [P(x), P(w), P(y), 0, N, H, W, C, 1, P(a), P(b), 6.0, P(part), st], [0, 1, 2, 9, 10, 12]),
        (lib.pfr_dwconv3_dgrad, [P(y), P(w), P(x), 0, N, H, W, C, 1, st], [0, 1, 2]),
        (lib.pfr_dwconv3_wgrad, [P(x), P(y), P(ws), P(dw), 0, N, H, W, C, 1, P(a), P(b), 6.0, 0, st], [0, 1, 2, 3, 10, 11]),
        (lib.pfr_bn_act_clamp, [P(x), P(a), P(b), P(y), 6.0, 0, N * H * W, C, st], [0, 1, 2, 3]),
        (lib.pfr_bn_bwd_reduce_clamp, [P(y), P(x), P(a), P(b), P(a), P(b), 6.0, 2, 0, N * H * W, C, P(part), st], [0, 1, 2, 3, 4, 5, 11]),
        (lib.pfr_bn_bwd_apply_clamp, [P(y), P(x), P(coef), P(a), P(b), 6.0, 2, P(y), 0, N * H * W, C, st], [0, 1, 2, 3, 4, 7]),
    ]
    for fn, args, ptrs in calls:
        fn(*args)                                   # all device pointers: accepted
        for i in ptrs:
            bad = list(args)
            bad[i] = hp
            with pytest.raises(PfrError, match="not a device pointer"):
                fn(*bad)
    torch.cuda.synchronize()
