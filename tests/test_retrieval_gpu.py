"""Exact retrieval ranks on the device: pfr_rank_count (the match GEMM with a rank-counting epilogue), pfr_pair_scores_gather (the
thresholds it is fed) and match.positive_ranks / retrieval_metrics against the brute-force oracle of tests/retrieval_oracle.py.

The contract restated here (include/pfr_hip.h): score s(i, j) = the fp32 accumulator (f32, bf16) or ((float) acc * s_a[i]) * s_b[j] (int8);
item (s, id) precedes threshold (t, tid) iff s > t || (s == t && id < tid);  cnt[i][k] += the number of b rows j with b_id[j] != excl[i]
that precede threshold k of row i;  the call adds.

int8 scores and integer-valued bf16 / f32 rows are exact in any summation order, so counts and ranks must be EQUAL to the oracle's.  On
random unit rows the device order is checked through its own consistency (a total order gives a permutation of 0 .. N - 2) and through a
sandwich whose slack is the format error derived in tests/test_pair_hist_gpu.py."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retrieval_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _gather(a, sa, b, sb, col, dtype):
    """pfr_pair_scores_gather over the whole list width -> fp32 [Na, ld] (NaN where nothing was written)"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    col = col.to(device=DEV, dtype=I32).contiguous()
    out = torch.full(col.shape, float("nan"), dtype=torch.float32, device=DEV)
    lib.pfr_pair_scores_gather(_ptr(a), _ptr(sa), a.shape[0], _ptr(b), _ptr(sb), 0 if b is None else b.shape[0], dtype_id(dtype), a.shape[1],
                               col.data_ptr(), col.shape[1], out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return out


def _count(a, sa, b, sb, ids, excl, thr, tid, tcnt, dtype, cnt=None):
    """pfr_rank_count over lists of any width, sliced into launches of at most pfr_rank_count_max_thr() thresholds -> int32 [Na, ld]"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    cap = lib.pfr_rank_count_max_thr()
    assert cap >= 16
    Na, ld = thr.shape
    thr, tid, tcnt = thr.to(DEV).float(), tid.to(device=DEV, dtype=I32), tcnt.to(device=DEV, dtype=torch.int64)
    ids = ids.to(device=DEV, dtype=I32).contiguous()
    excl = None if excl is None else excl.to(device=DEV, dtype=I32).contiguous()
    if cnt is None:
        cnt = torch.zeros((Na, ld), dtype=I32, device=DEV)
    for k0 in range(0, ld, cap):
        w = min(cap, ld - k0)
        tv, ti, part = thr[:, k0:k0 + w].contiguous(), tid[:, k0:k0 + w].contiguous(), cnt[:, k0:k0 + w].contiguous()
        tc = (tcnt - k0).clamp(0, w).to(I32).contiguous()
        lib.pfr_rank_count(_ptr(a), _ptr(sa), Na, _ptr(b), _ptr(sb), ids.data_ptr(), 0 if b is None else b.shape[0], dtype_id(dtype),
                           a.shape[1], _ptr(excl), tv.data_ptr(), ti.data_ptr(), tc.data_ptr(), w, part.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
        cnt[:, k0:k0 + w] = part
    return cnt


# ---- 1. int8: counts equal the definition, thresholds from the gather
@pytest.mark.parametrize("Na,Nb", [(2, None), (63, None), (64, None), (65, None), (129, None), (300, None), (70, 130), (1, 300)])
def test_int8_counts_equal_the_definition(Na, Nb):
    from pets_face_recognition_amd.match import quantize_rows
    g = torch.Generator().manual_seed(100 + Na)
    sym = Nb is None
    nb = Na if sym else Nb
    for D in (64, 200, 512):
        qa, sa = quantize_rows(torch.randn(Na, D, generator=g).to(DEV))
        qb, sb = (None, None) if sym else quantize_rows(torch.randn(Nb, D, generator=g).to(DEV))
        qbh, sbh = (qa, sa) if sym else (qb, sb)
        acc = (qa.cpu().double() @ qbh.cpu().double().t()).to(torch.int64)       # exact: integers below 2^53 in any order
        assert acc.abs().max() < 2 ** 24
        s = (acc.float() * sa.cpu()[:, None]) * sbh.cpu()[None, :]
        ids = torch.arange(nb)
        excl = torch.arange(Na) if sym else None
        for layout in ("random7", "equal", "distinct"):
            ca = O.class_layout(layout, Na, seed=Na)
            cb = ca if sym else O.class_layout(layout, Nb, seed=Nb)
            col, npos = O.padded(O.positive_lists(ca, cb, sym))
            if col.shape[1] == 0:
                continue                                                        # no positives at all: nothing to launch
            thr = _gather(qa, sa, qb, sb, col, torch.int8).cpu()
            ok = col >= 0
            want_thr = torch.gather(s, 1, col.clamp_min(0))
            assert torch.equal(thr[ok], want_thr[ok]) and bool(torch.isnan(thr[~ok]).all()), (Na, Nb, D, layout)
            got = _count(qa, sa, qb, sb, ids, excl, thr, col, npos, torch.int8).cpu().long()
            want = O.counts_from_scores(s, ids, want_thr, col, npos, excl)
            assert torch.equal(got, want), (Na, Nb, D, layout)
            if layout == "equal":
                # every item is a positive: each row's counts are a permutation of 0 .. n - 1
                assert torch.equal(got.sort(dim=1).values, torch.arange(col.shape[1]).expand(Na, -1))


# ---- 2. bf16 / f32: ranks equal the oracle on (tie-heavy) integer rows
def _int_rows(n, D, seed):
    return torch.randint(-2, 3, (n, D), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("D", [64, 512])
def test_integer_rows_rank_exactly(dtype, D):
    from pets_face_recognition_amd.match import positive_ranks
    for N in (127, 128, 129, 257, 385):
        x = _int_rows(N, D, 7 * N + D)
        cls = torch.randint(0, 9, (N,), generator=torch.Generator().manual_seed(N))
        ranks, npos = positive_ranks(x.to(DEV), cls.to(DEV), compute_dtype=dtype, normalize=False)
        s = (x.double() @ x.double().t()).float()                  # integers below 2^24: exact in fp32 and in any summation order
        assert O.as_lists(ranks, npos) == O.ranks_from_scores(s, cls, cls, True), (N, D, dtype)


# ---- 3. the gather and the count agree bit for bit
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gather_agrees_with_count_bit_for_bit(dtype):
    """Thresholds for ALL the other columns of every row, taken from the gather.  With distinct ids the order is total, so if
    a threshold is the very number the count launch computes for that pair, the N - 1 counts of a row are a permutation of
    0 .. N - 2: a threshold off by one ulp either counts itself or collides with a neighbour."""
    from pets_face_recognition_amd.match import _hist_operand
    N, D = 130, 512
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(9))
    a, _ = _hist_operand(x.to(DEV), dtype, True)
    col = torch.stack([torch.cat([torch.arange(i), torch.arange(i + 1, N)]) for i in range(N)])
    thr = _gather(a, None, None, None, col, dtype)
    assert not bool(torch.isnan(thr).any())
    cnt = _count(a, None, None, None, torch.arange(N), torch.arange(N), thr, col, torch.full((N,), N - 1), dtype)
    assert torch.equal(cnt.cpu().long().sort(dim=1).values, torch.arange(N - 1).expand(N, -1))
    # and the numbers are scores: within the format error of the float64 products
    xn = (x.double() / x.double().norm(dim=1, keepdim=True))
    E = (D + 8) * 2.0 ** -23 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    assert float((thr.cpu().double() - torch.gather(xn @ xn.t(), 1, col)).abs().max()) <= E


# ---- 4. random unit rows: sandwich against float64
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_unit_rows_sandwich(dtype):
    """A device score differs from the float64 score s64 by at most E (tests/test_pair_hist_gpu.py: f32 E = (D + 8) 2^-23, bf16
    E = 2^-8 + that).  An item that precedes positive p on the device has s64_j >= s64_p - 2E, and every item with s64_j > s64_p + 2E
    precedes it, so   1 + #{j : s64_j > s64_p + 2E}  <=  r  <=  1 + #{j : s64_j >= s64_p - 2E}   (the query and p itself excluded)."""
    from pets_face_recognition_amd.match import _hist_operand, positive_ranks
    N, D = 300, 512
    g = torch.Generator().manual_seed(5)
    cls = torch.arange(N) % 30
    x = torch.randn(30, D, generator=g)[cls] * 0.7 + torch.randn(N, D, generator=g)
    E = (D + 8) * 2.0 ** -23 + (2.0 ** -8 if dtype == torch.bfloat16 else 0.0)
    xn = x.double() / x.double().norm(dim=1, keepdim=True)
    s64 = xn @ xn.t()
    col, npos = O.padded(O.positive_lists(cls, cls, True))
    assert col.shape == (N, 9) and bool((npos == 9).all())
    a, _ = _hist_operand(x.to(DEV), dtype, True)
    thr = _gather(a, None, None, None, col, dtype)
    r = 1 + _count(a, None, None, None, torch.arange(N), torch.arange(N), thr, col, npos, dtype).cpu().long()
    sp = torch.gather(s64, 1, col)                                                  # [N, 9]
    other = torch.ones(N, N, dtype=torch.bool)
    other[torch.arange(N), torch.arange(N)] = False
    for k in range(col.shape[1]):
        oth = other.clone()
        oth[torch.arange(N), col[:, k]] = False
        lo = 1 + ((s64 > (sp[:, k] + 2 * E)[:, None]) & oth).sum(dim=1)
        hi = 1 + ((s64 >= (sp[:, k] - 2 * E)[:, None]) & oth).sum(dim=1)
        print(f"{dtype} k={k}: max slack hi - lo = {int((hi - lo).max())}, violations {int(((r[:, k] < lo) | (r[:, k] > hi)).sum())}")
        assert bool((lo <= r[:, k]).all()) and bool((r[:, k] <= hi).all()), (dtype, k)
    ranks, np_dev = positive_ranks(x.to(DEV), cls.to(DEV), compute_dtype=dtype)
    assert torch.equal(np_dev.cpu().long(), torch.bincount(cls)[cls] - 1)
    assert torch.equal(ranks.cpu().long(), r.sort(dim=1).values)


# ---- 5. the call adds
def test_the_call_adds_and_column_chunks_accumulate():
    N, D, dtype = 200, 64, torch.bfloat16
    x = _int_rows(N, D, 3).to(DEV).to(dtype).contiguous()
    cls = O.class_layout("random7", N, seed=1)
    col, npos = O.padded(O.positive_lists(cls, cls, True))
    thr = _gather(x, None, None, None, col, dtype)
    ids, excl = torch.arange(N), torch.arange(N)
    one = _count(x, None, None, None, ids, excl, thr, col, npos, dtype)
    s = (x.cpu().double() @ x.cpu().double().t()).float()
    assert torch.equal(one.cpu().long(), O.counts_from_scores(s, ids, thr.cpu(), col, npos, excl))
    two = _count(x, None, None, None, ids, excl, thr, col, npos, dtype, cnt=one.clone())
    assert torch.equal(two, 2 * one)
    h = 72                                                                           # (no multiple of the tile)
    parts = _count(x, None, x[:h].contiguous(), None, ids[:h], excl, thr, col, npos, dtype)
    parts = _count(x, None, x[h:].contiguous(), None, ids[h:], excl, thr, col, npos, dtype, cnt=parts)
    assert torch.equal(parts, one)


# ---- 6. argument errors launch nothing
def test_argument_errors_leave_the_table_untouched():
    from pets_face_recognition_amd._hip import lib, PfrError
    from pets_face_recognition_amd.match import quantize_rows
    N, D = 40, 128
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(2)).to(DEV)
    q8, sc = quantize_rows(x)
    cap = lib.pfr_rank_count_max_thr()
    ld = cap + 1
    ids = torch.arange(N, dtype=I32, device=DEV)
    thr = torch.zeros((N, ld), dtype=torch.float32, device=DEV)
    tid = torch.zeros((N, ld), dtype=I32, device=DEV)
    tc = torch.ones(N, dtype=I32, device=DEV)
    cnt = torch.full((N, ld), 7, dtype=I32, device=DEV)

    def call(a, sa, dtype, D_, thr_ptr, ld_):
        return lib.pfr_rank_count(a.data_ptr(), _ptr(sa), N, 0, 0, ids.data_ptr(), 0, dtype, D_, ids.data_ptr(), thr_ptr, tid.data_ptr(),
                                  tc.data_ptr(), ld_, cnt.data_ptr(), st)
    for args in ((x, None, 0, D, thr.data_ptr(), ld),          # ld above the cap
                 (x, None, 0, D, 0, cap),                      # null thr_val
                 (q8, None, 2, D, thr.data_ptr(), cap),        # int8 without scales
                 (x, None, 0, D + 1, thr.data_ptr(), cap)):    # D no multiple of the k-step
        with pytest.raises(PfrError) as e:
            call(*args)
        assert "rc=-1" in str(e.value)
    with pytest.raises(PfrError) as e:
        lib.pfr_pair_scores_gather(q8.data_ptr(), 0, N, 0, 0, 0, 2, D, tid.data_ptr(), cap, thr.data_ptr(), st)
    assert "rc=-1" in str(e.value)
    torch.cuda.synchronize()
    assert bool((cnt == 7).all()) and bool((thr == 0).all())
    # empty operands add nothing and are no error
    assert lib.pfr_rank_count(x.data_ptr(), 0, 0, 0, 0, ids.data_ptr(), 0, 0, D, 0, thr.data_ptr(), tid.data_ptr(), tc.data_ptr(), cap,
                              cnt.data_ptr(), st) == 0
    assert call(q8, sc, 2, D, thr.data_ptr(), cap) == 0          # (the same call with its scales is fine)


# ---- 7. the wrapper on the device equals its CPU path
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_retrieval_metrics_equal_the_cpu_path(dtype):
    from pets_face_recognition_amd.match import retrieval_metrics
    x, cls = _int_rows(257, 64, 21), torch.randint(0, 40, (257,), generator=torch.Generator().manual_seed(4))
    O.assert_metrics_equal(retrieval_metrics(x.to(DEV), cls.to(DEV), ks=(1, 5, 10), compute_dtype=dtype, normalize=False),
                           retrieval_metrics(x, cls, ks=(1, 5, 10), normalize=False))
    q, cq = _int_rows(70, 64, 22), torch.randint(0, 40, (70,), generator=torch.Generator().manual_seed(5))
    O.assert_metrics_equal(retrieval_metrics(q.to(DEV), cq.to(DEV), x.to(DEV), cls.to(DEV), compute_dtype=dtype, normalize=False),
                           retrieval_metrics(q, cq, x, cls, normalize=False))
    none = retrieval_metrics(x.to(DEV), torch.arange(257).to(DEV), compute_dtype=dtype, normalize=False)
    assert none["queries"] == 0 and none["mAP"] != none["mAP"]
