"""csrc/pfr_mha.hip through the C-ABI against fp64 torch on the CPU: pfr_mha_fwd / pfr_mha_bwd in fp32 and bf16 at the real ViT
sequence lengths and the edges of the 64-query / 32-key blocking, a query row with scaled scores near ±120, the two padding rules
(NaN neighbour in the batch), stray stores, run-to-run bit identity and the refused shapes.

The reference is fed the inputs AS ROUNDED to the kernel's dtype, so what is measured is the kernel's own error.  Bounds: those of
tests/test_swin_gpu.py::test_window_attention_kernel (relative L2: 2e-5 fp32, 2e-2 bf16).  Measured on an MI355X: fp32 out 4e-7 .. 6e-7,
dqkv 4e-7 .. 7e-7; bf16 out 1.8e-3 .. 1.9e-3, dqkv 2.5e-3 .. 2.7e-3 at every S including 257, so the bf16 bound needs no widening."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 64
SCALE = 1.0 / math.sqrt(HD)
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2}
CASES = [(2, 3, 197), (2, 2, 65), (3, 2, 64), (2, 2, 50), (1, 2, 257), (2, 1, 1)]   # (B, heads, S)
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
SENT = 4096


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _rel_part(a, b, whole):
    """relative error of one of dq / dk / dv; where the exact part is identically zero (S = 1: one key, dS = 0, so dq = dk = 0) the
    error is taken against the norm of the whole gradient instead of 0/0"""
    b = b.double().cpu()
    return rel(a, b) if b.norm() > 0 else (a.double().cpu().norm() / whole.double().norm()).item()


def _inputs(B, heads, S, dtype, seed=0, big_row=None):
    """qkv [B,S,3C] with q, k ~ N(0, 2): the scaled scores q·k/8 have a standard deviation of about 2 (neither uniform nor one-hot);
    v, dout ~ N(0, 1); all rounded to `dtype`.  big_row = (b, s, factor) multiplies one query row."""
    g = torch.Generator().manual_seed(1000 * S + 10 * heads + B + seed)
    C = heads * HD
    qkv = torch.randn(B, S, 3 * C, generator=g)
    qkv[..., :2 * C] *= math.sqrt(2.0)
    if big_row is not None:
        b, s, f = big_row
        qkv[b, s, :C] *= f
    dout = torch.randn(B, S, C, generator=g)
    return qkv.to(dtype).float(), dout.to(dtype).float()


def _reference(qkv, dout, heads):
    """fp64: out, lse [B,heads,S], dqkv"""
    B, S, C3 = qkv.shape
    C = C3 // 3
    x = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(B, S, heads, HD).permute(0, 2, 1, 3) for t in x.split(C, dim=-1))
    s = q @ k.transpose(-1, -2) * SCALE
    out = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, S, C)
    out.backward(dout.double())
    return out.detach(), torch.logsumexp(s.detach(), dim=-1), x.grad


@functools.lru_cache(maxsize=None)
def _case(B, heads, S, dtype):
    qkv, dout = _inputs(B, heads, S, dtype)
    return (qkv, dout) + _reference(qkv, dout, heads)


def _run(qkv, dout, heads, dtype, out_for_bwd=None):
    """the kernels on the device; `out` and `dqkv` carry SENT sentinel elements behind their last row, checked here on every call"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    B, S, C3 = qkv.shape
    C = C3 // 3
    st = torch.cuda.current_stream().cuda_stream
    did = dtype_id(dtype)
    qd = qkv.to(DEV, dtype).contiguous()
    dd = dout.to(DEV, dtype).contiguous()
    ob = torch.full((B * S * C + SENT,), -7.0, dtype=dtype, device=DEV)
    gb = torch.full((B * S * C3 + SENT,), -7.0, dtype=dtype, device=DEV)
    lse = torch.full((B * heads * S + SENT,), -7.0, dtype=torch.float32, device=DEV)
    lib.pfr_mha_fwd(qd.data_ptr(), ob.data_ptr(), lse.data_ptr(), did, B, S, heads, HD, SCALE, st)
    lib.pfr_mha_bwd(qd.data_ptr(), ob.data_ptr(), dd.data_ptr(), lse.data_ptr(), gb.data_ptr(), did, B, S, heads, HD, SCALE, st)
    torch.cuda.synchronize()
    for t, n in ((ob, B * S * C), (gb, B * S * C3), (lse, B * heads * S)):
        assert torch.all(t[n:] == -7.0), "store behind the last row"
    return ob[:B * S * C].view(B, S, C).clone(), lse[:B * heads * S].view(B, heads, S).clone(), gb[:B * S * C3].view(B, S, C3).clone()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,heads,S", CASES)
def test_mha_fwd_bwd_vs_fp64(B, heads, S, dtype):
    qkv, dout, out_ref, lse_ref, dqkv_ref = _case(B, heads, S, dtype)
    out, lse, dqkv = _run(qkv, dout, heads, dtype)
    C = heads * HD
    e_o, e_l, e_g = rel(out, out_ref), rel(lse, lse_ref), rel(dqkv, dqkv_ref)
    e_q, e_k, e_v = (_rel_part(dqkv[..., i * C:(i + 1) * C], dqkv_ref[..., i * C:(i + 1) * C], dqkv_ref) for i in range(3))
    print(f"S={S} {dtype}: out {e_o:.3e} lse {e_l:.3e} dqkv {e_g:.3e} (dq {e_q:.3e} dk {e_k:.3e} dv {e_v:.3e})")
    t = TOL[dtype]
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all()
    assert e_o < t and e_l < t and e_g < t and e_q < t and e_k < t and e_v < t


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mha_stability_large_scores(dtype):
    """one query row times 60: its scaled scores have a standard deviation of ~120; same bounds"""
    B, heads, S = 1, 2, 197
    qkv, dout = _inputs(B, heads, S, dtype, seed=3, big_row=(0, 77, 60.0))
    C = heads * HD
    s = (qkv[0, 77, :HD].double() @ qkv[0, :, C:C + HD].double().t()) * SCALE
    assert s.abs().max() > 100                                   # the row really is extreme
    out_ref, lse_ref, dqkv_ref = _reference(qkv, dout, heads)
    out, lse, dqkv = _run(qkv, dout, heads, dtype)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    e = (rel(out, out_ref), rel(lse, lse_ref), rel(dqkv, dqkv_ref), rel(out[0, 77], out_ref[0, 77]))
    print(f"{dtype}: out {e[0]:.3e} lse {e[1]:.3e} dqkv {e[2]:.3e} out[big row] {e[3]:.3e}")
    assert max(e) < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mha_padding_rows_are_zero_filled_not_the_neighbour(dtype):
    """B = 2, S = 65: batch element 1 all NaN.  Element 0's results are finite and bit-identical to a B = 1 run: the padding K / V / Q /
    dout rows of its tiles come from zero-fill, not from the rows that follow in memory."""
    heads, S = 2, 65
    qkv1, dout1 = _inputs(1, heads, S, dtype, seed=5)
    qkv2 = torch.cat([qkv1, torch.full_like(qkv1, float("nan"))])
    dout2 = torch.cat([dout1, torch.full_like(dout1, float("nan"))])
    o1, l1, g1 = _run(qkv1, dout1, heads, dtype)
    o2, l2, g2 = _run(qkv2, dout2, heads, dtype)
    for a in (o2[0], l2[0], g2[0]):
        assert torch.isfinite(a.float()).all()
    assert torch.equal(o2[0], o1[0]) and torch.equal(l2[0], l1[0]) and torch.equal(g2[0], g1[0])
    assert torch.isnan(o2[1].float()).all()                      # (and the NaN element is computed, not skipped)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mha_no_stray_stores_and_bit_reproducible(dtype):
    """4096 sentinel elements behind `out`, `lse` and `dqkv` stay untouched (_run checks them); two runs are bit-identical"""
    B, heads, S = 2, 3, 197
    qkv, dout = _case(B, heads, S, dtype)[:2]
    a = _run(qkv, dout, heads, dtype)
    b = _run(qkv, dout, heads, dtype)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_mha_inference_without_lse_and_refused_shapes():
    from pets_face_recognition_amd._hip import lib, dtype_id, PfrError
    st = torch.cuda.current_stream().cuda_stream
    for dtype in DTYPES:
        did = dtype_id(dtype)
        assert lib.pfr_mha_supported(did, 257, 12, 64) == 1
        assert lib.pfr_mha_supported(did, 258, 12, 64) == 0
        assert lib.pfr_mha_supported(did, 197, 16, 80) == 0
        B, heads, S = 2, 2, 50
        qkv, dout, out_ref = _case(B, heads, S, dtype)[:3]
        qd = qkv.to(DEV, dtype)
        out = torch.full((B, S, heads * HD), -7.0, dtype=dtype, device=DEV)
        lib.pfr_mha_fwd(qd.data_ptr(), out.data_ptr(), 0, did, B, S, heads, HD, SCALE, st)       # lse = NULL: inference
        torch.cuda.synchronize()
        assert rel(out, out_ref) < TOL[dtype]
        # a refused shape is an error and launches nothing: `out` keeps its fill
        out.fill_(-7.0)
        big = torch.zeros(1, 258, 3 * HD, dtype=dtype, device=DEV)
        with pytest.raises(PfrError, match="unsupported shape"):
            lib.pfr_mha_fwd(big.data_ptr(), out.data_ptr(), 0, did, 1, 258, 1, HD, SCALE, st)
        with pytest.raises(PfrError, match="unsupported shape"):
            lib.pfr_mha_fwd(qd.data_ptr(), out.data_ptr(), 0, did, B, S, heads, 80, SCALE, st)
        with pytest.raises(PfrError, match="unsupported shape"):
            lib.pfr_mha_bwd(qd.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), did, 1, 258, 1, HD, SCALE, st)
        torch.cuda.synchronize()
        assert torch.all(out == -7.0)
