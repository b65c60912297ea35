"""csrc/pfr_dwconvk.hip on the device: depthwise K x K convolution, K = 3 | 5, stride 1 | 2, padding K/2 (forward with the BatchNorm +
activation prologue and the statistics epilogue, data gradient, weight gradient with its accumulate flag) against
F.conv2d(groups=C, padding=K//2, stride=s) and autograd in fp64 on the CPU, on the activated operand computed from the stored, rounded x.

Criteria, those of tests/test_dwconv3_gpu.py: relative error in the L2 norm of forward and data gradient fp32 1e-5, bf16 4e-3 (one
output rounding, 2⁻⁸); weight gradient 1e-4 in both dtypes (fp32 accumulation).  Statistics: |Δmean| <= 1e-4·std and variance 1e-4
relative against fp64 statistics of the STORED y.  pro_act 1 at K = 3 equals pfr_dwconv3_fwd bit for bit.

Shapes [N,H,W,C]: [2,2,3,8] a plane smaller than the 5x5 window (every tap clamped); [2,9,7,8] an odd plane, one bf16 chunk;
[3,12,10,24] odd batch; [1,5,5,1040] fp32 / [1,5,5,2112] bf16 more than 256 chunk columns (the second workgroup column; 2112 is B2's
widest); [2,16,16,96] several row parts (the partial merge)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(2, 2, 3, 8), (2, 9, 7, 8), (3, 12, 10, 24), "wide", (2, 16, 16, 96)]
WIDE = {torch.float32: (1, 5, 5, 1040), torch.bfloat16: (1, 5, 5, 2112)}
DTYPES = [torch.float32, torch.bfloat16]
TOL_Y = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
TOL_G = 1e-4
ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
# (K, pro_act): act 0 and 2 at both K, act 1 at K = 3 only
KA = [(3, 0), (3, 2), (5, 0), (5, 2), (3, 1)]


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _activate(z, act):
    if act == 1:
        return z.clamp(0, 6)
    if act == 2:
        return z * torch.sigmoid(z)
    return z


@functools.lru_cache(maxsize=None)
def _case(shape, K, stride, dtype, act):
    """inputs (rounded to dtype, NHWC) and the fp64 CPU reference on the activated operand, computed once per case"""
    N, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape) * 7 + stride + 10 * K + (100 if dtype == torch.bfloat16 else 0))
    x = (torch.randn(N, H, W, C, generator=g) * 3).to(dtype)
    w = (torch.randn(C, 1, K, K, generator=g) / K).to(dtype)
    scale = torch.rand(C, generator=g) * 2 + 1          # [1, 3]
    shift = torch.rand(C, generator=g) * 2 + 0.5        # act(shift) != 0, so padding before activating is wrong
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    dy = torch.randn(N, OH, OW, C, generator=g).to(dtype)
    nchw = lambda t: t.double().permute(0, 3, 1, 2)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    z = nchw(x)
    if act:
        z = z * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    a = _activate(z, act).requires_grad_()
    w64 = w.double().requires_grad_()
    y = F.conv2d(a, w64, padding=K // 2, stride=stride, groups=C)
    assert tuple(y.shape) == (N, C, OH, OW)
    da, dw = torch.autograd.grad(y, (a, w64), nchw(dy))
    return dict(x=x, w=w, dy=dy, scale=scale, shift=shift, y=nhwc(y), da=nhwc(da), dw=dw, OH=OH, OW=OW)


def _taps(w):
    return w.view(w.shape[0], -1).t().contiguous().to(DEV)


def _fwd(c, shape, K, stride, dtype, act, stats=False):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    did = dtype_id(dtype)
    x, wt = c["x"].to(DEV), _taps(c["w"])
    sc, sh = c["scale"].to(DEV), c["shift"].to(DEV)
    y = _nan((N, c["OH"], c["OW"], C), dtype)
    part, rpp = None, 0
    if stats:
        rpp = lib.pfr_dwconvk_rows_per_part(did, N, H, W, C, K, stride)
        assert rpp >= 1
        part = _nan(((N * c["OH"] * c["OW"] + rpp - 1) // rpp, 2, C), torch.float32)
    lib.pfr_dwconvk_fwd(x.data_ptr(), wt.data_ptr(), y.data_ptr(), did, N, H, W, C, K, stride, act, sc.data_ptr() if act else 0,
                        sh.data_ptr() if act else 0, 6.0, part.data_ptr() if stats else 0, _stream())
    torch.cuda.synchronize()
    return y, part, rpp


def _wgrad(c, shape, K, stride, dtype, act, dw, accumulate):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, H, W, C = shape
    did = dtype_id(dtype)
    parts = lib.pfr_dwconvk_wgrad_parts(did, N, H, W, C, K, stride)
    assert parts >= 1
    ws = _nan((parts, K * K, C), torch.float32)
    x, dy, sc, sh = c["x"].to(DEV), c["dy"].to(DEV), c["scale"].to(DEV), c["shift"].to(DEV)
    lib.pfr_dwconvk_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), did, N, H, W, C, K, stride, act,
                          sc.data_ptr() if act else 0, sh.data_ptr() if act else 0, 6.0, accumulate, _stream())
    torch.cuda.synchronize()
    return parts


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2], ids=["s1", "s2"])
@pytest.mark.parametrize("ka", KA, ids=lambda ka: f"k{ka[0]}a{ka[1]}")
@pytest.mark.parametrize("shape", SHAPES, **ids)
def test_dwconvk_forward_dgrad_wgrad_statistics(shape, ka, stride, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    K, act = ka
    shape = WIDE[dtype] if shape == "wide" else shape
    N, H, W, C = shape
    c = _case(shape, K, stride, dtype, act)
    did = dtype_id(dtype)
    y, part, rpp = _fwd(c, shape, K, stride, dtype, act, stats=True)
    y2, part2, _ = _fwd(c, shape, K, stride, dtype, act, stats=True)
    y3, _, _ = _fwd(c, shape, K, stride, dtype, act, stats=False)
    assert torch.equal(y, y2) and torch.equal(part, part2) and torch.equal(y, y3) and torch.isfinite(part).all()   # no atomics
    # data gradient (of the operand the kernel convolves: the activated tensor)
    dx = _nan((N, H, W, C), dtype)
    dy = c["dy"].to(DEV)
    lib.pfr_dwconvk_dgrad(dy.data_ptr(), _taps(c["w"]).data_ptr(), dx.data_ptr(), did, N, H, W, C, K, stride, _stream())
    # weight gradient: overwrite (NaN in the buffer does not survive), then accumulate (the sum of both calls)
    dw = _nan((C, 1, K, K), torch.float32)
    parts = _wgrad(c, shape, K, stride, dtype, act, dw, 0)
    dw1 = dw.clone()
    _wgrad(c, shape, K, stride, dtype, act, dw, 1)
    e = dict(y=rel(y, c["y"]), dx=rel(dx, c["da"]), dw=rel(dw1, c["dw"]), dw2=rel(dw, 2 * c["dw"]))
    # statistics partials merged by pfr_bn_finalize (gamma = 1, beta = 0, eps = 0: invstd² = 1 / var) against the stored y in fp64
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
    print(shape, ka, stride, dtype, {k: f"{v:.2e}" for k, v in e.items()}, f"mean excess {dm:.2e} var excess {dv:.2e}",
          f"stat parts {part.shape[0]} wgrad parts {parts}")
    assert e["y"] <= TOL_Y[dtype] and e["dx"] <= TOL_Y[dtype], e
    assert e["dw"] <= TOL_G and e["dw2"] <= TOL_G, e
    assert dm <= 0 and dv <= 0
    if shape == (2, 16, 16, 96):
        assert part.shape[0] > 1 and parts > 1     # the partial merges are exercised
    if act == 1:     # K = 3: pfr_dwconv3_fwd bit for bit
        x, wt, sc, sh = c["x"].to(DEV), _taps(c["w"]), c["scale"].to(DEV), c["shift"].to(DEV)
        y0 = _nan(tuple(y.shape), dtype)
        lib.pfr_dwconv3_fwd(x.data_ptr(), wt.data_ptr(), y0.data_ptr(), did, N, H, W, C, stride, sc.data_ptr(), sh.data_ptr(), 6.0, 0,
                            _stream())
        torch.cuda.synchronize()
        assert torch.equal(y, y0)


def test_dwconvk_border_pixels_see_padding_of_the_activated_tensor():
    """silu(shift) != 0: padding x before the prologue would be wrong exactly at the border output pixels"""
    shape, K, stride, dtype = (2, 9, 7, 8), 5, 1, torch.float32
    c = _case(shape, K, stride, dtype, 2)
    y, _, _ = _fwd(c, shape, K, stride, dtype, 2)
    border = torch.ones(c["OH"], c["OW"], dtype=torch.bool)
    border[2:-2, 2:-2] = False
    assert rel(y.cpu()[:, border], c["y"][:, border]) <= TOL_Y[dtype]
