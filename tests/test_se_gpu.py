"""csrc/pfr_se.hip and the SiLU forms of the BatchNorm kernels on the device, through the C-ABI, against fp64 autograd of the torch
expression on the CPU, computed from inputs already rounded to the compute dtype.

Squeeze-and-excitation, (N, HW, C, S) in {(3,1,16,4), (2,35,96,6), (4,256,144,6), (2,4,2112,88)}: pfr_avgpool_fwd → pfr_se_gate_fwd →
pfr_se_scale_fwd, and backward pfr_se_scale_bwd_reduce → pfr_se_gate_bwd (with and without accumulate) → pfr_se_bwd_apply.
pfr_bn_act_silu / pfr_bn_bwd_*_silu and pfr_bn_residual_rows / pfr_row_scale on [70,24] and [3*35,96] rows with u = γ x̂ + β spanning
[-8, 8]: both SiLU tails and the minimum near u = -1.28.

Bounds (relative error in the L2 norm), those of tests/test_dwconv3_gpu.py: tensors stored in the compute dtype fp32 1e-5, bf16 4e-3
(one output rounding, 2⁻⁸; in bf16 the pooled operand of the gate is itself rounded to bf16, so the fp32 gate and what follows from it
carry that 2⁻⁸ too); parameter gradients and column sums, accumulated in fp32, 1e-4 in fp32 and, where they inherit the rounded pooled
operand, 4e-3 in bf16."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
TOL_Y = {torch.float32: 1e-5, torch.bfloat16: 4e-3}
TOL_G = {torch.float32: 1e-4, torch.bfloat16: 4e-3}
ids = dict(ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s))
P = lambda t: t.data_ptr()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def _se_case(nhcs, dtype):
    N, HW, C, S = nhcs
    g = torch.Generator().manual_seed(N * 1000 + HW + C + S)
    a = (torch.randn(N, HW, C, generator=g) + 0.5).to(dtype)
    dy = torch.randn(N, HW, C, generator=g).to(dtype)
    w1 = torch.randn(S, C, generator=g) / C ** 0.5 * 2
    b1 = torch.randn(S, generator=g)
    w2 = torch.randn(C, S, generator=g) / S ** 0.5 * 2
    b2 = torch.empty(C).uniform_(-2, 2, generator=g)
    a64 = a.double().requires_grad_()
    p = [t.double().requires_grad_() for t in (w1, b1, w2, b2)]
    pooled = a64.mean(1)
    pre = pooled @ p[0].t() + p[1]
    gate = torch.sigmoid(F.silu(pre) @ p[2].t() + p[3])
    y = a64 * gate[:, None, :]
    grads = torch.autograd.grad(y, [a64] + p, dy.double())
    return dict(a=a, dy=dy, w1=w1, b1=b1, w2=w2, b2=b2, pre=pre.detach(), gate=gate.detach(), y=y.detach(), da=grads[0], dw1=grads[1],
                db1=grads[2], dw2=grads[3], db2=grads[4])


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("nhcs", [(3, 1, 16, 4), (2, 35, 96, 6), (4, 256, 144, 6), (2, 4, 2112, 88)], **ids)
def test_se_forward_backward(nhcs, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    N, HW, C, S = nhcs
    c = _se_case(nhcs, dtype)
    did, st = dtype_id(dtype), _stream()
    a, dy, w1, b1, w2, b2 = (c[k].to(DEV) for k in ("a", "dy", "w1", "b1", "w2", "b2"))
    pooled, pre, gate, y = _nan((N, C), dtype), _nan((N, S)), _nan((N, C)), _nan((N, HW, C), dtype)
    lib.pfr_avgpool_fwd(P(a), P(pooled), did, N, HW, C, st)
    lib.pfr_se_gate_fwd(P(pooled), P(w1), P(b1), P(w2), P(b2), P(pre), P(gate), did, N, C, S, st)
    lib.pfr_se_scale_fwd(P(a), P(gate), P(y), did, N, HW, C, st)
    dgate, dpooled, ws, da = _nan((N, C)), _nan((N, C)), _nan((N, S)), _nan((N, HW, C), dtype)
    dw1, db1, dw2, db2 = _nan((S, C)), _nan((S,)), _nan((C, S)), _nan((C,))
    lib.pfr_se_scale_bwd_reduce(P(dy), P(a), P(dgate), did, N, HW, C, st)
    args = (P(dgate), P(pooled), P(pre), P(gate), P(w1), P(w2), P(ws), P(dpooled), P(dw1), P(db1), P(dw2), P(db2), did, N, C, S)
    lib.pfr_se_gate_bwd(*args, 0, st)          # overwrite: NaN in the buffers does not survive
    lib.pfr_se_bwd_apply(P(dy), P(gate), P(dpooled), P(da), did, N, HW, C, st)
    torch.cuda.synchronize()
    once = [t.clone() for t in (dw1, db1, dw2, db2)]
    lib.pfr_se_gate_bwd(*args, 1, st)          # accumulate: the sum of both calls
    torch.cuda.synchronize()
    e = dict(pre=rel(pre, c["pre"]), gate=rel(gate, c["gate"]), y=rel(y, c["y"]), da=rel(da, c["da"]),
             dgate=rel(dgate, (c["dy"].double() * c["a"].double()).sum(1)))
    eg = {k: rel(t, c[k]) for k, t in zip(("dw1", "db1", "dw2", "db2"), once)}
    eg2 = {k: rel(t, 2 * c[k]) for k, t in zip(("dw1", "db1", "dw2", "db2"), (dw1, db1, dw2, db2))}
    print(nhcs, dtype, {k: f"{v:.2e}" for k, v in {**e, **eg}.items()})
    assert all(v <= TOL_Y[dtype] for v in e.values()), e
    assert all(v <= TOL_G[dtype] for v in eg.values()), eg
    assert all(v <= TOL_G[dtype] for v in eg2.values()), eg2


@functools.lru_cache(maxsize=None)
def _bn_case(rc, dtype):
    """rows = N * HW samples-major; u = γ x̂ + β spans [-8, 8]: γ = 4 with x̂ to ±2 and more, β = 0 → |u| up to 8 and beyond"""
    (N, HW), C = rc
    rows = N * HW
    g = torch.Generator().manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).to(dtype)
    dout = torch.randn(rows, C, generator=g).to(dtype)
    res = torch.randn(rows, C, generator=g).to(dtype)
    gamma = torch.full((C,), 4.0) + torch.rand(C, generator=g) * 0.2
    beta = torch.rand(C, generator=g) * 0.4 - 0.2
    rs = torch.tensor([0.0, 2.0, 1.25, 0.0, 2.0][:N] + [2.0] * max(0, N - 5))
    x64, g64, b64 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    u = F.batch_norm(x64, None, None, g64, b64, training=True, eps=1e-5)
    assert u.min() < -8 and u.max() > 8 and ((u > -1.4) & (u < -1.1)).any()
    y = F.silu(u)
    dx, dg, db = torch.autograd.grad(y, (x64, g64, b64), dout.double(), retain_graph=True)
    # row-mode stochastic depth on the LINEAR BatchNorm: y = res + rs[n] * u
    yr = res.double() + rs.double().repeat_interleave(HW)[:, None] * u
    dxr, dgr, dbr = torch.autograd.grad(yr, (x64, g64, b64), dout.double())
    return dict(x=x, dout=dout, res=res, gamma=gamma, beta=beta, rs=rs, y=y.detach(), dx=dx, dg=dg, db=db, yr=yr.detach(), dxr=dxr,
                dgr=dgr, dbr=dbr)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rc", [((70, 1), 24), ((3, 35), 96)], ids=["70x24", "3*35x96"])
def test_bn_silu_and_row_scale_residual(rc, dtype):
    from pets_face_recognition_amd._hip import lib, dtype_id
    (N, HW), C = rc
    rows = N * HW
    c = _bn_case(rc, dtype)
    did, st = dtype_id(dtype), _stream()
    x, dout, res, gamma, beta, rs = (c[k].to(DEV) for k in ("x", "dout", "res", "gamma", "beta", "rs"))
    nb = lib.pfr_colreduce_blocks(C, did, rows)
    sp = _nan((nb, 2, C))
    lib.pfr_bn_stats(P(x), did, rows, C, P(sp), st)
    f = _nan((4, C))      # mean, invstd, scale, shift
    lib.pfr_bn_finalize(P(sp), sp.shape[0], lib.pfr_bn_stats_rows_per_part(C, did, rows), C, float(rows), P(gamma), P(beta), 1e-5, 0.1, 0, 0,
                        P(f[0]), P(f[1]), P(f[2]), P(f[3]), 0, st)
    # ---- BatchNorm + SiLU
    y, dx = _nan((rows, C), dtype), _nan((rows, C), dtype)
    part, coef, dg, db = _nan((nb, 2, C)), _nan((3, C)), _nan((C,)), _nan((C,))
    lib.pfr_bn_act_silu(P(x), P(f[2]), P(f[3]), P(y), did, rows, C, st)
    lib.pfr_bn_bwd_reduce_silu(P(dout), P(x), P(f[0]), P(f[1]), P(f[2]), P(f[3]), did, rows, C, P(part), st)
    lib.pfr_bn_bwd_finalize(P(part), nb, C, float(rows), P(gamma), P(f[0]), P(f[1]), P(dg), P(db), P(coef), 0, st)
    lib.pfr_bn_bwd_apply_silu(P(dout), P(x), P(coef), P(f[2]), P(f[3]), P(dx), did, rows, C, st)
    # ---- y = res + rs[n] (a x + b); backward: pfr_row_scale, then the linear BatchNorm step
    yr, dbr_in, dxr = _nan((rows, C), dtype), _nan((rows, C), dtype), _nan((rows, C), dtype)
    part2, coef2, dg2, db2 = _nan((nb, 2, C)), _nan((3, C)), _nan((C,)), _nan((C,))
    lib.pfr_bn_residual_rows(P(x), P(f[2]), P(f[3]), P(res), P(rs), P(yr), did, N, HW, C, st)
    lib.pfr_row_scale(P(dout), P(rs), P(dbr_in), did, N, HW, C, st)
    lib.pfr_bn_bwd_reduce_clamp(P(dbr_in), P(x), P(f[0]), P(f[1]), 0, 0, 0.0, 0, did, rows, C, P(part2), st)
    lib.pfr_bn_bwd_finalize(P(part2), nb, C, float(rows), P(gamma), P(f[0]), P(f[1]), P(dg2), P(db2), P(coef2), 0, st)
    lib.pfr_bn_bwd_apply_clamp(P(dbr_in), P(x), P(coef2), 0, 0, 0.0, 0, P(dxr), did, rows, C, st)
    torch.cuda.synchronize()
    e = dict(y=rel(y, c["y"]), dx=rel(dx, c["dx"]), yr=rel(yr, c["yr"]), dxr=rel(dxr, c["dxr"]))
    eg = dict(dg=rel(dg, c["dg"]), db=rel(db, c["db"]), dgr=rel(dg2, c["dgr"]), dbr=rel(db2, c["dbr"]))
    print(rc, dtype, {k: f"{v:.2e}" for k, v in {**e, **eg}.items()})
    assert all(v <= TOL_Y[dtype] for v in e.values()), e
    assert eg["dg"] <= 1e-4 and eg["db"] <= 1e-4, eg          # fp32 sums of inputs that are exact in either dtype
    assert eg["dgr"] <= TOL_G[dtype] and eg["dbr"] <= TOL_G[dtype], eg     # bf16: row_scale * dout is stored rounded
