"""csrc/pfr_prelu.hip on the device, through the C-ABI, against fp64 torch on the CPU: pfr_bn_act_prelu, pfr_bn_bwd_reduce_prelu +
pfr_bn_bwd_finalize + pfr_prelu_slope_finalize, pfr_bn_bwd_apply_prelu.

Shapes (rows, C): (1, 8) a single row, (37, 8) a ragged last row block, (64*3 + 5, 64) more than one row block, (1029, 512) the widest
layer; fp32 adds C = 4 (its 16-byte chunk).  Inputs are rounded to the compute dtype first and every side starts from those values.
Slopes include 0, 1, a negative value and 0.25.

Forward: against F.prelu of the fp32 u = scale*x + shift in fp64, rounded to fp32: within 2 ulp in fp32 (u is one fused multiply-add,
the slope product one more rounding), within one bf16 rounding of it in bf16.  Channel 0 has shift 0 and x = 0 in every third row:
u == 0 exactly, y == 0.

Backward: the BatchNorm is batch_norm(x, training=True); mean, invstd, scale = γ·invstd and shift = β − mean·scale are taken in fp64
from the rounded x and handed to the kernels in fp32.  The reference is fp64 autograd of prelu(batch_norm(x)).  x is drawn so that no
u lies in (0, 1e-3) of zero: the sign of such a u is decided by the rounding of the coefficients, and one flipped mask bit is an O(1)
difference at that element on either side of the comparison.

The bound is measured, not fixed: the same sums (the same fp32 coefficients, u, g and products, elementwise in fp32, then
torch.sum over the rows in fp32) are done by torch on the CPU, their error against fp64 is taken, and the kernel is allowed 4 x that
(a different summation order of the same fp32 terms) plus 2^-24, half an ulp of the fp32 result itself (a single-term sum is exact on
the CPU).  bf16 dx is stored rounded: one bf16 rounding, 2^-8 (8 significant bits), is added for it.  Errors of sums are condition-aware as in
tests/test_mobilenet_gpu.py: ‖a − b‖ over the norm of what is summed, ‖Σ_rows |term|‖, so a sum that cancels is not compared with
its own rounding noise; the coefficient rows inherit the scale of the sums they are made from, and dx = coef0*g + coef1*x + coef2 is
itself a sum of three terms that cancel (entirely so for a single row).

Measured CPU-fp32 errors on these inputs (worst over the shapes, this metric): dgamma 3.3e-08, dbeta 3.0e-08, dslope 5.9e-06,
coef 6.2e-08, dx 5.7e-08 (fp32 inputs); 2.3e-08, 1.1e-08, 4.1e-05, 6.7e-08, 5.7e-08 (bf16-rounded inputs).  The dslope figures are
the single-row case: its variance is 0, invstd = eps^-1/2 = 316, and u = β is recovered from scale*x + shift with both near 316·x;
every other shape is below 5e-08.  Factor 4."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 8), (37, 8), (64 * 3 + 5, 64), (1029, 512)]
CASES = [(s, torch.float32) for s in SHAPES + [(37, 4)]] + [(s, torch.bfloat16) for s in SHAPES]
IDS = [f"{r}x{c}-{'fp32' if d == torch.float32 else 'bf16'}" for (r, c), d in CASES]
EPS = 1e-5
FACTOR = 4.0
P = lambda t: t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _slopes(C, g):
    s = torch.rand(C, generator=g) * 0.7 - 0.2
    s[:4] = torch.tensor([0.0, 1.0, -0.3, 0.25])
    return s


@functools.lru_cache(maxsize=None)
def _fwd_case(shape, dtype):
    rows, C = shape
    g = torch.Generator().manual_seed(rows * 131 + C)
    x = torch.randn(rows, C, generator=g).to(dtype)
    scale = torch.rand(C, generator=g) + 0.5
    shift = torch.randn(C, generator=g)
    shift[0] = 0.0
    x[::3, 0] = 0.0
    slope = _slopes(C, g)
    u = torch.addcmul(shift.double(), x.double(), scale.double()).float()          # the fp32 u: one rounding (fused multiply-add)
    y = F.prelu(u.double(), slope.double())
    return dict(x=x, scale=scale, shift=shift, slope=slope, y=y)


@functools.lru_cache(maxsize=None)
def _bwd_case(shape, dtype):
    rows, C = shape
    g = torch.Generator().manual_seed(rows * 977 + C)
    x = torch.randn(rows, C, generator=g).to(dtype)
    dout = torch.randn(rows, C, generator=g).to(dtype)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    slope = _slopes(C, g)

    def stats(x):
        x64 = x.double()
        mean, var = x64.mean(0), x64.var(0, unbiased=False)
        invstd = (var + EPS).rsqrt()
        return mean, invstd, (x64 - mean) * invstd * gamma.double() + beta.double()

    for _ in range(20):      # no u within (0, 1e-3) of zero (module docstring)
        mean, invstd, u = stats(x)
        near = u.abs() < 1e-3
        if not near.any():
            break
        x = torch.where(near, (x.float() + torch.where(u >= 0, 0.25, -0.25)).to(dtype), x)
    assert not near.any()
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    f = torch.stack([mean, invstd, scale, shift]).float()
    # ---- fp64 autograd of prelu(batch_norm(x))
    x64, g64, b64, s64 = (t.double().requires_grad_() for t in (x, gamma, beta, slope))
    # (batch_norm written out: F.batch_norm refuses a single row in training mode)
    y = F.prelu((x64 - x64.mean(0)) * (x64.var(0, unbiased=False) + EPS).rsqrt() * g64 + b64, s64)
    y.backward(dout.double())
    xhat = (x.double() - mean) * invstd
    gm = dout.double() * torch.where(u > 0, torch.ones_like(u), slope.double().expand_as(u))

    def coef_of(dgamma, dbeta, mean, invstd, gam):
        cg = gam * invstd
        cx = -gam * invstd * invstd * dgamma / rows
        return torch.stack([cg, cx, -gam * invstd * dbeta / rows - cx * mean])

    ref = dict(dgamma=g64.grad, dbeta=b64.grad, dslope=s64.grad, dx=x64.grad, coef=coef_of(g64.grad, b64.grad, mean, invstd, gamma.double()))
    # ---- what each sum is summed from (the condition of the sum), and the scale the coefficient rows inherit from them
    cond = dict(dgamma=(gm * xhat).abs().sum(0), dbeta=gm.abs().sum(0), dslope=(dout.double() * u.clamp(max=0)).abs().sum(0))
    cg = (gamma.double() * invstd).abs()
    c1 = cg * invstd * cond["dgamma"] / rows
    cond["coef"] = torch.stack([cg, c1, cg * cond["dbeta"] / rows + c1 * mean.abs()])
    rc = ref["coef"]
    cond["dx"] = (rc[0] * gm).abs() + (rc[1] * x.double()).abs() + rc[2].abs()      # dx = coef0*g + coef1*x + coef2: three terms that cancel
    # ---- the same sums by torch in fp32 on the CPU, from the fp32 coefficients the kernels get
    x32, d32, s32 = x.float(), dout.float(), slope
    u32 = x32 * f[2] + f[3]
    g32 = d32 * torch.where(u32 > 0, torch.ones_like(u32), s32.expand_as(u32))
    cpu = dict(dbeta=g32.sum(0), dgamma=(g32 * ((x32 - f[0]) * f[1])).sum(0), dslope=(d32 * u32.clamp(max=0)).sum(0))
    cpu["coef"] = coef_of(cpu["dgamma"], cpu["dbeta"], f[0], f[1], gamma)
    cpu["dx"] = cpu["coef"][0] * g32 + cpu["coef"][1] * x32 + cpu["coef"][2]
    case = dict(x=x, dout=dout, gamma=gamma, slope=slope, f=f, ref=ref, cond=cond)
    case["cpu_err"] = {k: _err(cpu[k], case, k) for k in ref}
    return case


def _err(v, case, k):
    d = (v.double().cpu() - case["ref"][k]).norm()
    return (d / ((case["cond"][k] if k in case["cond"] else case["ref"][k]).norm() + 1e-300)).item()


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_bn_act_prelu_forward(shape, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = shape
    c = _fwd_case(shape, dtype)
    x, scale, shift, slope = (c[k].to(DEV) for k in ("x", "scale", "shift", "slope"))
    y = _nan((rows, C), dtype)
    lib.pfr_bn_act_prelu(P(x), P(scale), P(shift), P(slope), P(y), dtype_id(dtype), rows, C, _stream())
    torch.cuda.synchronize()
    y, want = y.cpu(), c["y"]
    assert torch.isfinite(y).all()
    assert (y[::3, 0] == 0).all()                                  # u == 0 exactly: 0 for every slope
    w32 = want.float()
    if dtype == torch.float32:
        ulp = torch.maximum((torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).abs(), torch.tensor(2.0 ** -149)).double()
        worst = ((y.double() - w32.double()).abs() / ulp).max().item()
        print(f"{shape} fp32: worst forward error {worst:.2f} ulp")
        assert worst <= 2.0
    else:
        # one bf16 rounding of the fp32 value: half a bf16 ulp of it (8 significant bits: at most 2^-8 relative), plus the fp32 value's own 2 ulp
        bound = want.abs() * (2.0 ** -8 + 2.0 ** -22) + 2.0 ** -133
        excess = ((y.double() - want).abs() - bound).max().item()
        print(f"{shape} bf16: forward error over one bf16 rounding {excess:.2e}")
        assert excess <= 0


def _run_reduce(case, shape, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = shape
    did, st = dtype_id(dtype), _stream()
    x, dout, slope, f = (case[k].to(DEV) for k in ("x", "dout", "slope", "f"))
    nb = lib.pfr_colreduce_blocks(C, did, rows)
    part = _nan((3 * nb * C,))
    lib.pfr_bn_bwd_reduce_prelu(P(dout), P(x), P(f[0]), P(f[1]), P(f[2]), P(f[3]), P(slope), did, rows, C, P(part), st)
    return part, nb, (x, dout, slope, f)


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_bn_prelu_backward(shape, dtype):
    """reduce + finalize (dgamma, dbeta, dslope, coef) and apply (dx) against fp64 autograd, bounds from the CPU-fp32 sums"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    rows, C = shape
    case = _bwd_case(shape, dtype)
    did, st = dtype_id(dtype), _stream()
    part, nb, (x, dout, slope, f) = _run_reduce(case, shape, dtype)
    gamma = case["gamma"].to(DEV)
    dg, db, ds, coef, dx = _nan((C,)), _nan((C,)), _nan((C,)), _nan((3, C)), _nan((rows, C), dtype)
    lib.pfr_bn_bwd_finalize(P(part), nb, C, float(rows), P(gamma), P(f[0]), P(f[1]), P(dg), P(db), P(coef), 0, st)
    lib.pfr_prelu_slope_finalize(P(part), nb, C, P(ds), 0, st)
    lib.pfr_bn_bwd_apply_prelu(P(dout), P(x), P(coef), P(f[2]), P(f[3]), P(slope), P(dx), did, rows, C, st)
    torch.cuda.synchronize()
    got = dict(dgamma=dg, dbeta=db, dslope=ds, coef=coef, dx=dx)
    errs = {k: _err(v, case, k) for k, v in got.items()}
    bounds = {k: FACTOR * case["cpu_err"][k] + 2.0 ** -24 for k in got}
    if dtype == torch.bfloat16:
        bounds["dx"] += 2.0 ** -8
    print(shape, dtype, "kernel", {k: f"{v:.2e}" for k, v in errs.items()}, "CPU fp32", {k: f"{v:.2e}" for k, v in case["cpu_err"].items()})
    for k in got:
        assert torch.isfinite(got[k].float()).all(), k
        assert errs[k] <= bounds[k], (k, errs[k], case["cpu_err"][k])
    # accumulate adds to what dslope holds
    once = ds.clone()
    lib.pfr_prelu_slope_finalize(P(part), nb, C, P(ds), 1, st)
    torch.cuda.synchronize()
    assert torch.equal(ds, once + once)


@pytest.mark.parametrize("shape,dtype", [CASES[3], CASES[7], CASES[8]], ids=[IDS[3], IDS[7], IDS[8]])
def test_bn_prelu_reduce_is_deterministic(shape, dtype):
    case = _bwd_case(shape, dtype)
    a, _, keep_a = _run_reduce(case, shape, dtype)
    b, _, keep_b = _run_reduce(case, shape, dtype)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_bn_prelu_reduce_at_u_zero():
    """u == 0 exactly (scale 1, shift 0, x = 0): the element adds dout*slope to Σg (torch's prelu_backward takes the slope side at 0) and
    nothing to the slope gradient; all terms are small integers, so the sums are exact"""
    from pets_face_recognition_amd._hip import lib
    rows, C = 37, 8
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-2, 3, (rows, C), generator=g).float()
    dout = torch.randint(-3, 4, (rows, C), generator=g).float()
    slope = torch.tensor([0.0, 1.0, -2.0, 0.25, 0.5, 2.0, -1.0, 4.0])
    assert (x == 0).any()
    x64 = x.double().requires_grad_()
    s64 = slope.double().requires_grad_()
    F.prelu(x64, s64).backward(dout.double())
    f = torch.stack([torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)]).to(DEV)
    nb = lib.pfr_colreduce_blocks(C, 0, rows)
    part = _nan((3 * nb * C,))
    xd, dd, sd = x.to(DEV), dout.to(DEV), slope.to(DEV)
    lib.pfr_bn_bwd_reduce_prelu(P(dd), P(xd), P(f[0]), P(f[1]), P(f[2]), P(f[3]), P(sd), 0, rows, C, P(part), _stream())
    torch.cuda.synchronize()
    bn = part[:2 * nb * C].view(nb, 2, C).sum(0).double().cpu()
    sl = part[2 * nb * C:].view(nb, C).sum(0).double().cpu()
    assert torch.equal(bn[0], x64.grad.sum(0)) and torch.equal(bn[1], (x64.grad * x.double()).sum(0))
    assert torch.equal(sl, s64.grad)
