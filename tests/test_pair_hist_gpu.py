"""All-pairs verification on the device: pfr_pair_hist (the match GEMM with a genuine / impostor histogram epilogue) and match.pair_histogram
against host restatements of the contract in include/pfr_hip.h.

The contract restated here:  score s of (a row i, b row j) = the fp32 accumulator (f32, bf16) or ((float) acc * s_a[i]) * s_b[j] (int8);
x = (s - lo) * inv_w as two fp32 operations;  bin = clamp(floor(x), 0, bins - 1), a NaN score -> slot `bins`;  kind = classes equal;
hist[kind][bin] += 1;  symmetric mode counts every pair i < j once;  the call adds to the table.

int8 scores and integer-valued bf16 / f32 data are exact in any summation order, so those tables must be EQUAL.  Random unit rows are
compared through a sandwich of suffix counts whose slack is derived from the number formats (test_unit_rows_sandwich)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


def _lo_invw(bins, lo, hi):
    lo32, hi32 = torch.tensor(lo, dtype=F32), torch.tensor(hi, dtype=F32)
    return float(lo32), float(torch.tensor(float(bins), dtype=F32) / (hi32 - lo32))


def _host_table(s, ca, cb, sym, lo, inv_w, bins):
    """the bin rule on an fp32 score matrix s [Na, Nb] (host) -> int64 [2, bins + 1]"""
    assert s.dtype == F32
    x = (s - torch.tensor(lo, dtype=F32)) * torch.tensor(inv_w, dtype=F32)
    slot = torch.floor(x).clamp(0, bins - 1)
    slot = torch.where(torch.isnan(s), torch.full_like(slot, float(bins)), slot).long()
    slot = slot + (ca.long()[:, None] == cb.long()[None, :]).long() * (bins + 1)
    if sym:
        i, j = torch.arange(s.shape[0])[:, None], torch.arange(s.shape[1])[None, :]
        slot = slot[i < j]
    return torch.bincount(slot.reshape(-1), minlength=2 * (bins + 1)).view(2, bins + 1)


def _launch(a, sa, ca, b, sb, cb, dtype, lo, inv_w, bins, hist=None, Na=None, Nb=None):
    from pets_face_recognition_amd._hip import lib, dtype_id
    if hist is None:
        hist = torch.zeros((2, bins + 1), dtype=torch.int64, device=DEV)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    Na = a.shape[0] if Na is None else Na
    Nb = (0 if b is None else b.shape[0]) if Nb is None else Nb
    rc = lib.pfr_pair_hist(ptr(a), ptr(sa), ptr(ca), Na, ptr(b), ptr(sb), ptr(cb), Nb, dtype_id(dtype),
                           a.shape[1], lo, inv_w, bins, hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return hist


def _classes(n, layout, g):
    if layout == "random7":
        return torch.randint(0, 7, (n,), generator=g, dtype=torch.int32)
    if layout == "equal":
        return torch.full((n,), 5, dtype=torch.int32)
    return torch.arange(n, dtype=torch.int32) * 3 - 11          # all distinct


# ---- 1. int8: bit-exact against the definition
@pytest.mark.parametrize("Na,Nb", [(2, None), (63, None), (64, None), (65, None), (129, None), (300, None), (70, 130), (1, 300)])
def test_int8_equals_the_definition(Na, Nb):
    from pets_face_recognition_amd.match import quantize_rows
    g = torch.Generator().manual_seed(100 + Na)
    sym = Nb is None
    for D in (64, 200, 512):
        xa = torch.randn(Na, D, generator=g)
        qa, sa = quantize_rows(xa.to(DEV))
        if sym:
            qb, sb = qa, sa
        else:
            qb, sb = quantize_rows(torch.randn(Nb, D, generator=g).to(DEV))
        acc = (qa.cpu().double() @ qb.cpu().double().t()).to(torch.int64)       # exact: integers below 2^53 in any order
        assert acc.abs().max() < 2 ** 24
        s = (acc.float() * sa.cpu()[:, None]) * sb.cpu()[None, :]
        for layout in ("random7", "equal", "distinct"):
            ca = _classes(Na, layout, g)
            cb = ca if sym else _classes(Nb, layout, g)
            for bins in (2, 64, 8192):
                lo, inv_w = _lo_invw(bins, -1.0, 1.0)
                want = _host_table(s, ca, cb, sym, lo, inv_w, bins)
                got = _launch(qa, sa, ca.to(DEV), None if sym else qb, None if sym else sb, None if sym else cb.to(DEV), torch.int8,
                              lo, inv_w, bins)
                assert torch.equal(got.cpu(), want), (Na, Nb, D, layout, bins)
                assert int(want.sum()) == (Na * (Na - 1) // 2 if sym else Na * Nb)


# ---- 2. bf16 / f32: exact on integer data
def _int_rows(n, D, seed):
    return torch.randint(-2, 3, (n, D), generator=torch.Generator().manual_seed(seed)).float()


def _int_case(N, D, dtype, rng=None):
    from pets_face_recognition_amd.match import pair_histogram
    x = _int_rows(N, D, 7 * N + D)
    cls = torch.randint(0, 9, (N,), generator=torch.Generator().manual_seed(N))
    bins = min(8 * D, 8192)
    rng = (-4.0 * D, 4.0 * D) if rng is None else rng
    hist, lo, inv_w = pair_histogram(x.to(DEV), cls.to(DEV), bins=bins, range=rng, compute_dtype=dtype, normalize=False)
    s = (x.double() @ x.double().t()).float()                  # integers below 2^24: exact in fp32 and in any summation order
    want = _host_table(s, cls, cls, True, lo, inv_w, bins)
    return hist.cpu(), want


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [64, 512])
def test_integer_data_is_exact(dtype, D):
    for N in (127, 128, 129, 257, 385):
        got, want = _int_case(N, D, dtype)
        assert torch.equal(got, want), (N, D, dtype)
        assert int(got.sum()) == N * (N - 1) // 2 and int(got[:, -1].sum()) == 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_out_of_range_scores_saturate(dtype):
    got, want = _int_case(257, 512, dtype, rng=(-8.0, 8.0))
    assert torch.equal(got, want)
    bins = want.shape[1] - 1
    assert int(want[:, 0].sum() + want[:, bins - 1].sum()) > int(want.sum()) // 2      # most scores sit in the end bins


# ---- 3. random unit rows: sandwich against float64
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unit_rows_sandwich(dtype):
    """C(b) = pairs of one kind with bin >= b.  A device score differs from the float64 score by at most E, so it lands at most
    m = ceil(E / w) bins away (w = 2 / bins):  C_ref(b + m) <= C_gpu(b) <= C_ref(b - m).
    E is derived: f32 E = (D + 8) 2^-23 (m = 1); bf16 E = 2^-8 + E_f32 (two 2^-9 relative operand roundings with sum |a_i b_i| <= 1; m = 9)."""
    from pets_face_recognition_amd.match import pair_histogram
    N, D, bins = 300, 512, 4096
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, D, generator=g)
    cls = torch.randint(0, 30, (N,), generator=g)
    hist, lo, inv_w = pair_histogram(x.to(DEV), cls.to(DEV), bins=bins, compute_dtype=dtype)
    hist = hist.cpu()
    same = cls[:, None] == cls[None, :]
    upper = torch.arange(N)[:, None] < torch.arange(N)[None, :]
    assert int(hist.sum()) == N * (N - 1) // 2
    assert int(hist[1].sum()) == int((same & upper).sum())
    assert int(hist[:, bins].sum()) == 0
    xn = x.double() / x.double().norm(dim=1, keepdim=True)
    s = xn @ xn.t()
    ref_bin = torch.floor((s - lo) * inv_w).clamp(0, bins - 1).long()
    E = (D + 8) * 2.0 ** -23 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    m = math.ceil(E / (2.0 / bins))
    assert m == (9 if dtype == torch.bfloat16 else 1)
    for kind in (0, 1):
        sel = upper & (same if kind else ~same)
        ref = torch.bincount(ref_bin[sel], minlength=bins)
        c_ref = torch.cat([ref.flip(0).cumsum(0).flip(0), torch.zeros(1, dtype=torch.long)])      # index 0 .. bins
        c_gpu = torch.cat([hist[kind, :bins].flip(0).cumsum(0).flip(0), torch.zeros(1, dtype=torch.long)])
        b = torch.arange(bins + 1)
        lower = c_ref[(b + m).clamp(max=bins)]
        upper_c = c_ref[(b - m).clamp(min=0)]
        assert bool((lower <= c_gpu).all()) and bool((c_gpu <= upper_c).all()), (dtype, kind)


# ---- 4. counter width
def test_one_bin_beyond_32_bits():
    """93 000 identical rows, all classes distinct: the single impostor bin must hold 93 000 * 92 999 / 2 = 4 324 453 500 > 2^32 (the
    smallest N that crosses 2^32 is 92 683); every other slot stays 0.  Also the worst case of same-address atomics."""
    from pets_face_recognition_amd.match import quantize_rows
    N, bins = 93000, 4096
    row = torch.randn(1, 128, generator=torch.Generator().manual_seed(9))
    q8, sc = quantize_rows(row.to(DEV).expand(N, 128).contiguous())
    cls = torch.arange(N, dtype=torch.int32, device=DEV)
    lo, inv_w = _lo_invw(bins, -1.0, 1.0)
    hist = _launch(q8, sc, cls, None, None, None, torch.int8, lo, inv_w, bins).cpu()
    acc = (q8[:1].cpu().double() @ q8[:1].cpu().double().t()).to(torch.int64)
    s = (acc.float() * sc[:1].cpu()[:, None]) * sc[:1].cpu()[None, :]
    b = int(torch.floor((s - torch.tensor(lo, dtype=F32)) * torch.tensor(inv_w, dtype=F32)).clamp(0, bins - 1))
    want = torch.zeros((2, bins + 1), dtype=torch.int64)
    want[0, b] = N * (N - 1) // 2
    assert N * (N - 1) // 2 == 4324453500 > 2 ** 32
    assert torch.equal(hist, want), (int(hist.sum()), int(hist[0, b]))


# ---- 5. accumulation and empties
def test_accumulates_and_ignores_empty_sets():
    bins = 64
    lo, inv_w = _lo_invw(bins, -64.0, 64.0)
    xa, xb = _int_rows(70, 64, 1).to(DEV), _int_rows(130, 64, 2).to(DEV)
    g = torch.Generator().manual_seed(3)
    ca, cb = _classes(70, "random7", g).to(DEV), _classes(130, "random7", g).to(DEV)
    t1 = _launch(xa, None, ca, None, None, None, F32, lo, inv_w, bins)
    t2 = _launch(xa, None, ca, xb, None, cb, F32, lo, inv_w, bins)
    both = _launch(xa, None, ca, None, None, None, F32, lo, inv_w, bins)
    both = _launch(xa, None, ca, xb, None, cb, F32, lo, inv_w, bins, hist=both)
    assert torch.equal(both, t1 + t2) and int(t1.sum()) == 70 * 69 // 2 and int(t2.sum()) == 70 * 130
    # symmetric Na == 1, Na == 0 and an empty second set: return 0, add nothing
    z = torch.zeros((2, bins + 1), dtype=torch.int64, device=DEV)
    # (row counts are passed explicitly: an empty tensor's pointer is NULL, and a NULL b means symmetric mode)
    _launch(xa, None, ca, None, None, None, F32, lo, inv_w, bins, hist=z, Na=1)
    _launch(xa, None, ca, None, None, None, F32, lo, inv_w, bins, hist=z, Na=0)
    _launch(xa, None, ca, xb, None, cb, F32, lo, inv_w, bins, hist=z, Nb=0)
    _launch(xa, None, ca, xb, None, cb, F32, lo, inv_w, bins, hist=z, Na=0)
    assert int(z.abs().sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nan_row_lands_in_the_nan_slot_only(dtype):
    from pets_face_recognition_amd.match import pair_histogram
    N, D, bins = 130, 64, 64
    x = _int_rows(N, D, 4)
    x[77, 5] = float("nan")
    cls = torch.randint(0, 7, (N,), generator=torch.Generator().manual_seed(6))
    hist, lo, inv_w = pair_histogram(x.to(DEV), cls.to(DEV), bins=bins, range=(-64.0, 64.0), compute_dtype=dtype, normalize=False)
    s = (x.double() @ x.double().t()).float()
    want = _host_table(s, cls, cls, True, lo, inv_w, bins)
    assert int(want[:, bins].sum()) == N - 1
    assert torch.equal(hist.cpu(), want)


# ---- 6. match.pair_histogram: device against CPU
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_device_path_equals_cpu_path(dtype):
    from pets_face_recognition_amd.match import pair_histogram
    D, bins = 64, 512
    xa, xb = _int_rows(257, D, 11), _int_rows(129, D, 12)
    g = torch.Generator().manual_seed(13)
    ca, cb = torch.randint(0, 9, (257,), generator=g), torch.randint(0, 9, (129,), generator=g)
    kw = dict(bins=bins, range=(-4.0 * D, 4.0 * D), compute_dtype=dtype, normalize=False)
    for args_cpu in ((xa, ca), (xa, ca, xb, cb)):
        h_cpu, lo_c, w_c = pair_histogram(*args_cpu, **kw)
        h_dev, lo_d, w_d = pair_histogram(*[t.to(DEV) for t in args_cpu], **kw)
        assert (lo_c, w_c) == (lo_d, w_d)
        assert h_dev.dtype == torch.int64 and h_dev.shape == (2, bins + 1)
        assert torch.equal(h_dev.cpu(), h_cpu)
