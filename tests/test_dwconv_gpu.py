"""csrc/pfr_dwconv.hip on the device: depthwise 7x7 convolution (forward, mirrored-tap data gradient, weight / bias gradient with
its accumulate flag) and layer scale with per-sample stochastic depth, against F.conv2d(groups=C) / plain tensor arithmetic and
their autograd in fp64 on the CPU, computed from inputs already rounded to the compute dtype.

Bounds (relative error in the L2 norm): forward and data gradient fp32 1e-5 (49 fp32 FMAs: 49·2⁻²⁴ ≈ 3e-6), bf16 4e-3 (one output
rounding, 2⁻⁸); weight, bias and layer-scale gradients 1e-4 in both dtypes (fp32 accumulation: the column-sum tests' bound)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 2, 2, 96),      # plane smaller than the halo (last stage at a 64-pixel input)
          (3, 7, 7, 768),     # ConvNeXt-T's last stage, odd N
          (2, 14, 14, 384),
          (2, 5, 9, 96),      # non-square, no tile multiple
          (1, 56, 56, 96),    # 64 + 32 channels
          (2, 8, 8, 32),
          (1, 16, 16, 200)]   # C no multiple of 64 (nor of the 32-channel chunk)
DTYPES = [torch.float32, torch.bfloat16]
TOL_Y = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
TOL_G = 1e-4


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """inputs (rounded to dtype, NHWC) and the fp64 CPU reference, computed once per (shape, dtype)"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(hash(shape) % 1000 + (1 if dtype == torch.bfloat16 else 0))
    x = torch.randn(N, H, W, C, generator=g).to(dtype)
    dy = torch.randn(N, H, W, C, generator=g).to(dtype)
    w = (torch.randn(C, 1, 7, 7, generator=g) / 7).to(dtype)
    b = torch.randn(C, generator=g) * 0.5
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_()
    w64 = w.double().requires_grad_()
    b64 = b.double().requires_grad_()
    y = F.conv2d(x64, w64, b64, padding=3, groups=C)
    dx, dw, db = torch.autograd.grad(y, (x64, w64, b64), dy.double().permute(0, 3, 1, 2))
    return dict(x=x, dy=dy, w=w, b=b, y=y.detach().permute(0, 2, 3, 1), dx=dx.permute(0, 2, 3, 1), dw=dw, db=db)


def _taps(w):
    C = w.shape[0]
    return w.view(C, 49).t().contiguous().to(DEV)


def _wgrad(x, dy, dtype, shape, dw, db, accumulate):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    parts = lib.pfr_dwconv2d_wgrad_parts(dtype_id(dtype), N, H, W, C, 7)
    assert parts >= 1
    ws = torch.empty(parts, 50, C, dtype=torch.float32, device=DEV)
    lib.pfr_dwconv2d_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), 0 if db is None else db.data_ptr(), dtype_id(dtype),
                           N, H, W, C, 7, accumulate, _stream())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dwconv_forward_dgrad_wgrad(shape, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    c = _case(shape, dtype)
    did = dtype_id(dtype)
    x, dy, wt, b = c["x"].to(DEV), c["dy"].to(DEV), _taps(c["w"]), c["b"].to(DEV)
    y = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=DEV)
    lib.pfr_dwconv2d_fwd(x.data_ptr(), wt.data_ptr(), b.data_ptr(), y.data_ptr(), did, N, H, W, C, 7, 0, _stream())
    dx = torch.full((N, H, W, C), float("nan"), dtype=dtype, device=DEV)
    lib.pfr_dwconv2d_fwd(dy.data_ptr(), wt.data_ptr(), 0, dx.data_ptr(), did, N, H, W, C, 7, 1, _stream())
    dw = torch.full((C, 1, 7, 7), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
    _wgrad(x, dy, dtype, shape, dw, db, 0)
    torch.cuda.synchronize()
    e = dict(y=rel(y, c["y"]), dx=rel(dx, c["dx"]), dw=rel(dw, c["dw"]), db=rel(db, c["db"]))
    print(shape, dtype, {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] <= TOL_Y[dtype] and e["dx"] <= TOL_Y[dtype], e
    assert e["dw"] <= TOL_G and e["db"] <= TOL_G, e


def test_dwconv_wgrad_accumulate_flag():
    shape, dtype = (2, 5, 9, 96), torch.float32
    c = _case(shape, dtype)
    C = shape[3]
    x, dy = c["x"].to(DEV), c["dy"].to(DEV)
    dw = torch.full((C, 1, 7, 7), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
    _wgrad(x, dy, dtype, shape, dw, db, 0)          # overwrite: NaN in the buffer does not survive
    torch.cuda.synchronize()
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert rel(dw, c["dw"]) <= TOL_G and rel(db, c["db"]) <= TOL_G
    _wgrad(x, dy, dtype, shape, dw, db, 1)          # accumulate: the sum of both calls
    torch.cuda.synchronize()
    assert rel(dw, 2 * c["dw"]) <= TOL_G and rel(db, 2 * c["db"]) <= TOL_G
    dw2 = torch.zeros_like(dw)
    _wgrad(x, dy, dtype, shape, dw2, None, 0)       # no bias gradient wanted
    torch.cuda.synchronize()
    assert rel(dw2, c["dw"]) <= TOL_G


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("with_rs", [False, True], ids=["plain", "rowscale"])
@pytest.mark.parametrize("shape", [(3, 4, 96), (2, 49, 768)], ids=lambda s: "x".join(map(str, s)))
def test_layer_scale_forward_backward(shape, with_rs, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, HW, C = shape
    did = dtype_id(dtype)
    g = torch.Generator().manual_seed(11 + N)
    u = torch.randn(N, HW, C, generator=g).to(dtype)
    res = torch.randn(N, HW, C, generator=g).to(dtype)
    dz = torch.randn(N, HW, C, generator=g).to(dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    rs = torch.tensor([0.0, 1.25, 1.25][:N]) if with_rs else None        # sample 0 dropped
    u64 = u.double().requires_grad_()
    g64 = gamma.double().requires_grad_()
    s64 = rs.double().view(N, 1, 1) if with_rs else 1.0
    y_ref = res.double() + s64 * g64 * u64
    du_ref, dg_ref = torch.autograd.grad(y_ref, (u64, g64), dz.double())

    ud, resd, dzd, gd = u.to(DEV), res.to(DEV), dz.to(DEV), gamma.to(DEV)
    rsd = rs.to(DEV) if with_rs else None
    rsp = rsd.data_ptr() if with_rs else 0
    y = torch.full((N, HW, C), float("nan"), dtype=dtype, device=DEV)
    lib.pfr_layer_scale_fwd(ud.data_ptr(), gd.data_ptr(), rsp, resd.data_ptr(), y.data_ptr(), did, N, HW, C, _stream())
    parts = lib.pfr_layer_scale_bwd_parts(N, HW, C)
    part = torch.full((parts, C), float("nan"), dtype=torch.float32, device=DEV)
    du = torch.full((N, HW, C), float("nan"), dtype=dtype, device=DEV)
    dg = torch.full((C,), float("nan"), dtype=torch.float32, device=DEV)
    lib.pfr_layer_scale_bwd(dzd.data_ptr(), ud.data_ptr(), gd.data_ptr(), rsp, du.data_ptr(), part.data_ptr(), dg.data_ptr(), did, N, HW, C,
                            0, _stream())
    torch.cuda.synchronize()
    e = dict(y=rel(y, y_ref.detach()), du=rel(du, du_ref), dg=rel(dg, dg_ref))
    print(shape, with_rs, dtype, {k: f"{v:.2e}" for k, v in e.items()})
    assert e["y"] <= TOL_Y[dtype] and e["du"] <= TOL_Y[dtype] and e["dg"] <= TOL_G, e
    if with_rs:
        assert torch.equal(y[0], resd[0]) and torch.all(du[0] == 0)      # a dropped sample: identity forward, no gradient
    lib.pfr_layer_scale_bwd(dzd.data_ptr(), ud.data_ptr(), gd.data_ptr(), rsp, du.data_ptr(), part.data_ptr(), dg.data_ptr(), did, N, HW, C,
                            1, _stream())
    torch.cuda.synchronize()
    assert rel(dg, 2 * dg_ref) <= TOL_G
    # merge left to the caller (the engine's deferred column-sum batch): the partial rows sum to the gradient
    lib.pfr_layer_scale_bwd(dzd.data_ptr(), ud.data_ptr(), gd.data_ptr(), rsp, du.data_ptr(), part.data_ptr(), 0, did, N, HW, C, 0, _stream())
    torch.cuda.synchronize()
    assert rel(part.sum(0), dg_ref) <= TOL_G


def test_host_pointer_in_any_position_is_an_error_code():
    """every non-NULL pointer is checked before a launch: a host pointer next to real device pointers returns an error, no fault"""
    import ctypes
    from pets_face_recognition_amd._hip import lib, PfrError
    N, H, W, C = 1, 4, 4, 8
    host = (ctypes.c_float * 8192)()
    hp = ctypes.addressof(host)
    d = lambda *s: torch.zeros(*s, device=DEV)
    x, y, w, b = d(N, H, W, C), d(N, H, W, C), d(49, C), d(C)
    dw, db = d(C, 49), d(C)
    ws = d(lib.pfr_dwconv2d_wgrad_parts(0, N, H, W, C, 7), 50, C)
    rs, part = d(N), d(lib.pfr_layer_scale_bwd_parts(N, H * W, C), C)
    st = _stream()
    P = lambda t: t.data_ptr()
    calls = {
        lib.pfr_dwconv2d_fwd: ([P(x), P(w), P(b), P(y)], (0, N, H, W, C, 7, 0, st)),
        lib.pfr_dwconv2d_wgrad: ([P(x), P(y), P(ws), P(dw), P(db)], (0, N, H, W, C, 7, 0, st)),
        lib.pfr_layer_scale_fwd: ([P(x), P(b), P(rs), P(y), P(y)], (0, N, H * W, C, st)),
        lib.pfr_layer_scale_bwd: ([P(x), P(y), P(b), P(rs), P(dw), P(part), P(db)], (0, N, H * W, C, 0, st)),
    }
    for fn, (ptrs, rest) in calls.items():
        fn(*ptrs, *rest)                                   # all device pointers: accepted
        for i in range(len(ptrs)):
            bad = list(ptrs)
            bad[i] = hp
            with pytest.raises(PfrError, match="not a device pointer"):
                fn(*bad, *rest)
    torch.cuda.synchronize()
