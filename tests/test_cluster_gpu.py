"""Threshold clustering on the device: pfr_pairs_above (the match GEMM with a compacting-append and a union-find epilogue), pfr_cc_union,
pfr_cc_flatten and match.pairs_above / match.cluster.

The expected edge set comes from pfr_pair_scores_gather over ALL the columns of every row: an existing entry point, tested on its own
(tests/test_retrieval_gpu.py), that runs the same tile code.  The comparison is therefore on the kernel's own score bits and is EXACT for
every dtype: no tolerance anywhere in this file.  Expected labels are the oracle union-find (tests/cluster_oracle.py) over that set."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32
INF = float("inf")
PFR_ERR_ARG = -1
SHAPES = [(2, None), (63, None), (64, None), (65, None), (127, None), (128, None), (129, None), (300, None), (70, 130), (1, 300)]
DTYPES = [torch.float32, torch.bfloat16, torch.int8]
DIMS = (64, 200, 512)                       # (200 is zero padded to the 128-byte k-step by the operand preparation)
CANARY = -7


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _case(Na, Nb, D, dtype):
    """random unit rows -> the prepared operands and the gathered scores of every pair, computed once per case and shared:
    (a, sa, b, sb, S fp32 [Na, nb] on the host, valid bool [Na, nb]: the pairs the entry point visits)"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    from pets_face_recognition_amd.match import _hist_operand
    g = torch.Generator().manual_seed(1000 * Na + 7 * (Nb or 0) + D)
    sym = Nb is None
    nb = Na if sym else Nb
    a, sa = _hist_operand(torch.randn(Na, D, generator=g).to(DEV), dtype, True)
    b, sb = (None, None) if sym else _hist_operand(torch.randn(Nb, D, generator=g).to(DEV), dtype, True)
    col = torch.arange(nb, dtype=I32, device=DEV).expand(Na, nb).contiguous()
    out = torch.full((Na, nb), float("nan"), dtype=torch.float32, device=DEV)
    lib.pfr_pair_scores_gather(_ptr(a), _ptr(sa), Na, _ptr(b), _ptr(sb), 0 if sym else Nb, dtype_id(dtype), a.shape[1], col.data_ptr(), nb,
                               out.data_ptr(), _stream())
    S = out.cpu()
    assert not bool(torch.isnan(S).any())
    valid = torch.ones(Na, nb, dtype=torch.bool).triu(1) if sym else torch.ones(Na, nb, dtype=torch.bool)
    return a, sa, b, sb, S, valid


def _above(a, sa, b, sb, dtype, thr, cap=None, a_off=0, b_off=0, room=64, count=None, parent=None, status=None, edges=True, raw=False):
    """one pfr_pairs_above call -> (rc, edge_i, edge_j, edge_s, count) with `room` canary elements behind cap"""
    from pets_face_recognition_amd._hip.lib import lib as L
    from pets_face_recognition_amd._hip import dtype_id
    L._load()
    ei = ej = es = None
    if edges:
        ei = torch.full((cap + room,), CANARY, dtype=I32, device=DEV)
        ej = torch.full((cap + room,), CANARY, dtype=I32, device=DEV)
        es = torch.full((cap + room,), float(CANARY), dtype=torch.float32, device=DEV)
        if count is None:
            count = torch.zeros(1, dtype=torch.int64, device=DEV)
    rc = L._dll.pfr_pairs_above(_ptr(a), _ptr(sa), a.shape[0], a_off, _ptr(b), _ptr(sb), 0 if b is None else b.shape[0], b_off,
                                dtype if raw else dtype_id(dtype), a.shape[1], thr, _ptr(ei), _ptr(ej), _ptr(es), cap or 0, _ptr(count),
                                _ptr(parent), 0 if parent is None else parent.numel(), _ptr(status), _stream())
    torch.cuda.synchronize()
    return rc, ei, ej, es, count


def _expected(S, valid, thr):
    """-> (i, j, score bits) int64 tensors sorted by (i, j)"""
    ok = valid & (S >= thr)
    i, j = ok.nonzero(as_tuple=True)                 # (row-major: sorted by (i, j))
    return i, j, S[i, j].view(I32).long()


def _sorted_edges(ei, ej, es, n, nb, a_off=0, b_off=0):
    i, j, s = ei[:n].cpu().long() - a_off, ej[:n].cpu().long() - b_off, es[:n].cpu().view(I32).long()
    order = torch.argsort(i * nb + j)
    return i[order], j[order], s[order]


def _thresholds(S, valid):
    v = S[valid].sort().values
    exact = float(v[(2 * v.numel()) // 3])             # one gathered score exactly: equality qualifies
    return [float(v[v.numel() // 2]), float(v[min(v.numel() - 1, (99 * v.numel()) // 100)]), exact]


# ---- 1. the edge set equals the gathered one, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Na,Nb", SHAPES)
def test_edges_equal_the_gathered_set(Na, Nb, dtype):
    sym = Nb is None
    nb = Na if sym else Nb
    a_off, b_off = 1000, (1000 if sym else 5000)
    for D in DIMS:
        a, sa, b, sb, S, valid = _case(Na, Nb, D, dtype)
        for k, thr in enumerate(_thresholds(S, valid)):
            wi, wj, ws = _expected(S, valid, thr)
            assert wi.numel() >= 1                                      # (every threshold is a gathered score: it qualifies itself)
            rc, ei, ej, es, count = _above(a, sa, b, sb, dtype, thr, cap=wi.numel(), a_off=a_off, b_off=b_off)
            assert rc == 0 and int(count) == wi.numel(), (Na, Nb, D, dtype, k)
            gi, gj, gs = _sorted_edges(ei, ej, es, wi.numel(), nb, a_off, b_off)
            assert torch.equal(gi, wi) and torch.equal(gj, wj) and torch.equal(gs, ws), (Na, Nb, D, dtype, k)
            if sym:
                assert bool((gi < gj).all())                            # no diagonal, no j <= i
            assert bool((ei[wi.numel():] == CANARY).all()) and bool((ej[wi.numel():] == CANARY).all())
            assert bool((es[wi.numel():] == float(CANARY)).all())


def test_wrapper_sorts_and_relaunches_once(monkeypatch):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import PfrError
    g = torch.Generator().manual_seed(5)
    x = torch.randn(300, 64, generator=g)
    xd = x.to(DEV)
    ci, cj, cs = match.pairs_above(xd, 0.1)
    assert ci.dtype == torch.int64 and cs.dtype == torch.float32 and ci.is_cuda
    key = ci * 300 + cj
    assert bool((key[1:] > key[:-1]).all()) and bool((ci < cj).all())   # sorted by (i, j), each pair once
    n = ci.numel()
    assert n > 8
    # a default capacity below the count: exactly one more launch, with the exact count, and the same result
    calls = []
    real = match.lib.pfr_pairs_above
    monkeypatch.setattr(match, "PAIRS_ABOVE_DEFAULT_CAP", 8)
    monkeypatch.setattr(match.lib, "pfr_pairs_above", lambda *args: (calls.append(args[14]), real(*args))[1])
    ri, rj, rs = match.pairs_above(xd, 0.1)
    assert calls == [8, n] and torch.equal(ri, ci) and torch.equal(rj, cj) and torch.equal(rs.view(I32), cs.view(I32))
    del calls[:]
    with pytest.raises(PfrError, match=str(n)):
        match.pairs_above(xd, 0.1, max_pairs=n - 1)
    assert len(calls) == 1                                              # max_pairs: an error instead of the second launch
    assert match.pairs_above(xd, 0.1, max_pairs=n)[0].numel() == n
    # two-set mode and the device / host paths agree on well separated scores
    # (fp32 unit rows of D = 64: either path is within (D + 8) 2^-23 < 1e-5 of the float64 score, test_pair_hist_gpu.py)
    qi, qj, qs = match.pairs_above(xd[:70], 0.1, emb_b=xd[70:200])
    xn = torch.nn.functional.normalize(x.double(), dim=1)
    s64 = xn[:70] @ xn[70:200].t()
    got = torch.zeros(70, 130, dtype=torch.bool)
    got[qi.cpu(), qj.cpu()] = True
    assert bool(got[s64 > 0.1 + 1e-5].all()) and not bool(got[s64 < 0.1 - 1e-5].any()) and int(got.sum()) == qi.numel()
    assert float((qs.cpu().double() - s64[qi.cpu(), qj.cpu()]).abs().max()) < 1e-5


# ---- 2. capacity
@pytest.mark.parametrize("dtype", [torch.float32, torch.int8])
def test_capacity_and_count(dtype):
    a, sa, b, sb, S, valid = _case(300, None, 64, dtype)
    thr = _thresholds(S, valid)[1]
    wi, wj, ws = _expected(S, valid, thr)
    n = wi.numel()
    assert n > 100
    want = set(zip(wi.tolist(), wj.tolist(), ws.tolist()))
    for cap in (0, n - 1, n):
        rc, ei, ej, es, count = _above(a, sa, b, sb, dtype, thr, cap=cap)
        assert rc == 0 and int(count) == n, cap                         # the count is exact whatever was written
        got = list(zip(ei[:cap].tolist(), ej[:cap].tolist(), es[:cap].view(I32).tolist()))
        assert len(set(got)) == cap and set(got) <= want, cap           # what is written is cap DISTINCT members of the set
        assert bool((ei[cap:] == CANARY).all()) and bool((ej[cap:] == CANARY).all()) and bool((es[cap:] == float(CANARY)).all()), cap
        rc, _, _, _, count = _above(a, sa, b, sb, dtype, thr, cap=cap, count=count)
        assert rc == 0 and int(count) == 2 * n                          # a second call ADDS
    # edge_s is optional
    from pets_face_recognition_amd._hip import lib, dtype_id
    ei = torch.full((n,), CANARY, dtype=I32, device=DEV)
    ej = torch.full((n,), CANARY, dtype=I32, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    lib.pfr_pairs_above(_ptr(a), _ptr(sa), 300, 0, 0, 0, 0, 0, dtype_id(dtype), a.shape[1], thr, ei.data_ptr(), ej.data_ptr(), 0, n,
                        count.data_ptr(), 0, 0, 0, _stream())
    assert int(count) == n and set(zip(ei.tolist(), ej.tolist())) == {(i, j) for i, j, _ in want}


# ---- 3. special scores
def test_nan_rows_and_infinite_thresholds():
    from pets_face_recognition_amd.match import _hist_operand
    N = 130
    x = torch.randn(N, 64, generator=torch.Generator().manual_seed(6))
    x[5] = float("nan")
    x[129] = float("nan")
    for dtype in (torch.float32, torch.bfloat16):
        a, _ = _hist_operand(x.to(DEV), dtype, False)
        clean = (N - 2) * (N - 3) // 2
        rc, ei, ej, es, count = _above(a, None, None, None, dtype, -INF, cap=clean)
        assert rc == 0 and int(count) == clean                           # every non-NaN pair, and only those
        nodes = set(ei[:clean].tolist()) | set(ej[:clean].tolist())
        assert nodes == set(range(N)) - {5, 129} and not bool(torch.isnan(es[:clean]).any())
        rc, ei, ej, es, count = _above(a, None, None, None, dtype, INF, cap=4)
        assert rc == 0 and int(count) == 0 and bool((ei == CANARY).all())
        rc, ei, ej, es, count = _above(a, None, None, None, dtype, float("nan"), cap=4)
        assert rc == 0 and int(count) == 0
        # the union epilogue follows the same rule: the NaN rows stay alone, everything else is one component
        parent = torch.arange(N, dtype=I32, device=DEV)
        status = torch.zeros(1, dtype=I32, device=DEV)
        rc, *_ = _above(a, None, None, None, dtype, -INF, parent=parent, status=status, edges=False)
        assert rc == 0 and int(status) == 0
        lab = _flatten(parent)
        assert lab[5] == 5 and lab[129] == 129 and set(lab.tolist()) == {0, 5, 129}


# ---- 4. labels
def _flatten(parent, in_place=False):
    from pets_face_recognition_amd._hip import lib
    labels = parent if in_place else torch.full_like(parent, CANARY)
    lib.pfr_cc_flatten(parent.data_ptr(), parent.numel(), labels.data_ptr(), _stream())
    torch.cuda.synchronize()
    return labels.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Na", [n for n, nb in SHAPES if nb is None])
def test_cluster_equals_the_oracle(Na, dtype):
    from pets_face_recognition_amd import match
    for D in DIMS:
        a, sa, _, _, S, valid = _case(Na, None, D, dtype)
        x = torch.randn(Na, D, generator=torch.Generator().manual_seed(1000 * Na + D))     # the rows _case prepared
        for k, thr in enumerate(_thresholds(S, valid)):
            wi, wj, _ = _expected(S, valid, thr)
            want = O.components(Na, zip(wi.tolist(), wj.tolist()))
            labels = match.cluster(x.to(DEV), thr, compute_dtype=dtype)                      # (raises when status is set)
            assert labels.dtype == torch.int64 and labels.tolist() == want, (Na, D, dtype, k)
            # the raw entry point on the prepared operand, with both outputs at once
            parent = torch.arange(Na, dtype=I32, device=DEV)
            status = torch.zeros(1, dtype=I32, device=DEV)
            rc, ei, ej, es, count = _above(a, sa, None, None, dtype, thr, cap=wi.numel(), parent=parent, status=status)
            assert rc == 0 and int(count) == wi.numel() and int(status) == 0
            assert bool((parent.cpu() <= torch.arange(Na)).all()) and bool((parent >= 0).all())
            assert _flatten(parent).tolist() == want, (Na, D, dtype, k)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_workgroup_contention(dtype):
    """8 classes interleaved as i % 8: every component spans every row tile, so every workgroup hooks into the same 8 trees"""
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd.match import _hist_operand
    N = 1024
    cls = torch.arange(N) % 8
    x = torch.zeros(N, 64)
    x[torch.arange(N), cls] = 8.0                                      # same class: 64, different class: 0 — exact in every dtype
    labels = match.cluster(x.to(DEV), 32.0, compute_dtype=dtype, normalize=False)
    assert torch.equal(labels.cpu(), cls)
    a, _ = _hist_operand(x.to(DEV), dtype, False)
    parent = torch.arange(N, dtype=I32, device=DEV)
    status = torch.zeros(1, dtype=I32, device=DEV)
    rc, ei, ej, es, count = _above(a, None, None, None, dtype, 32.0, cap=8 * 128 * 127 // 2, parent=parent, status=status)
    assert rc == 0 and int(status) == 0 and int(count) == 8 * 128 * 127 // 2
    assert bool((parent.cpu() <= torch.arange(N)).all()) and torch.equal(_flatten(parent).long(), cls)
    assert bool((es[:int(count)] == 64.0).all()) and bool((ei[:int(count)] % 8 == ej[:int(count)] % 8).all())


def test_one_clique_and_chunked_launches():
    from pets_face_recognition_amd import match
    row = torch.randn(1, 64, generator=torch.Generator().manual_seed(8))
    labels = match.cluster(row.expand(300, 64).contiguous().to(DEV), 0.5)
    assert labels.tolist() == [0] * 300
    for dtype in DTYPES:
        _, _, _, _, S, valid = _case(300, None, 200, dtype)
        x = torch.randn(300, 200, generator=torch.Generator().manual_seed(1000 * 300 + 200)).to(DEV)
        for thr in _thresholds(S, valid):
            one = match.cluster(x, thr, compute_dtype=dtype)
            assert torch.equal(match.cluster(x, thr, compute_dtype=dtype, chunk=128), one)
            assert torch.equal(match.cluster(x, thr, compute_dtype=dtype, chunk=300), one)
            assert 1 <= len(set(one.tolist())) <= 300


# ---- 5. pfr_cc_union + pfr_cc_flatten on hand-built graphs
def _union(parent, edges, status):
    from pets_face_recognition_amd._hip import lib
    e = torch.tensor(edges, dtype=I32, device=DEV).reshape(-1, 2)
    ei, ej = e[:, 0].contiguous(), e[:, 1].contiguous()
    lib.pfr_cc_union(parent.data_ptr(), parent.numel(), ei.data_ptr(), ej.data_ptr(), e.shape[0], status.data_ptr(), _stream())
    torch.cuda.synchronize()


def _check_forest(parent, edges, status):
    N = parent.numel()
    assert int(status) == 0
    p = parent.cpu()
    assert bool((p <= torch.arange(N)).all()) and bool((p >= 0).all())            # parent[x] <= x afterwards
    ok = [(u, v) for u, v in edges if 0 <= u < N and 0 <= v < N]
    want = O.components(N, ok)
    assert _flatten(parent).tolist() == want                                       # labels are the component minimum
    return want


def test_union_and_flatten_on_hand_built_graphs():
    N = 4096
    g = torch.Generator().manual_seed(9)
    fresh = lambda: (torch.arange(N, dtype=I32, device=DEV), torch.zeros(1, dtype=I32, device=DEV))
    # a path: shuffled, half of the edges reversed, every edge twice
    path = [(i, i + 1) for i in range(N - 1)]
    perm = torch.randperm(2 * (N - 1), generator=g).tolist()
    edges = [(path[k % (N - 1)] if k % 2 else path[k % (N - 1)][::-1]) for k in perm]
    parent, status = fresh()
    _union(parent, edges, status)
    assert _check_forest(parent, edges, status) == [0] * N
    # a star around the LAST node: every hook moves the centre's root
    edges = [(N - 1, i) for i in range(N - 1)]
    parent, status = fresh()
    _union(parent, edges, status)
    assert _check_forest(parent, edges, status) == [0] * N
    # a binary tree
    edges = [(i, (i - 1) // 2) for i in range(1, N)]
    parent, status = fresh()
    _union(parent, edges, status)
    assert _check_forest(parent, edges, status) == [0] * N
    # two components (even and odd nodes), joined by one late edge in a second call
    edges = [(i, i + 2) for i in range(N - 2)]
    parent, status = fresh()
    _union(parent, edges, status)
    assert _check_forest(parent, edges, status) == [i % 2 for i in range(N)]
    _union(parent, [(N - 1, N - 2)], status)
    assert _check_forest(parent, edges + [(N - 1, N - 2)], status) == [0] * N
    # self-loops, -1 padding and ids outside the range are ignored
    edges = [(5, 5), (-1, 3), (3, -1), (-1, -1), (7, N), (N + 5, 2), (1, 2), (2000, 9)]
    parent, status = fresh()
    _union(parent, edges, status)
    want = _check_forest(parent, edges, status)
    assert want[2] == 1 and want[2000] == 9 and sum(1 for x in range(N) if want[x] != x) == 2
    # flatten in place: labels may alias parent
    parent, status = fresh()
    _union(parent, path, status)
    assert _flatten(parent, in_place=True).tolist() == [0] * N and parent.tolist() == [0] * N


# ---- 6. argument errors: PFR_ERR_ARG and nothing written
def test_argument_errors_write_nothing():
    from pets_face_recognition_amd._hip.lib import lib as L
    a, sa, _, _, S, valid = _case(65, None, 64, torch.int8)
    af, _, bf, _, _, _ = _case(70, 130, 64, torch.float32)
    L._load()
    ei = torch.full((64,), CANARY, dtype=I32, device=DEV)
    ej = torch.full((64,), CANARY, dtype=I32, device=DEV)
    es = torch.full((64,), float(CANARY), dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    parent = torch.arange(130, dtype=I32, device=DEV)
    status = torch.zeros(1, dtype=I32, device=DEV)
    host = torch.zeros(64, dtype=I32)
    big = 2 ** 31 - 1

    def call(a=af, sa=None, Na=70, a_off=0, b=bf, sb=None, Nb=130, b_off=0, dtype=0, D=64, ei=ei, ej=ej, es=es, cap=32, count=count,
             parent=parent, n_nodes=130, status=status):
        return L._dll.pfr_pairs_above(_ptr(a), _ptr(sa), Na, a_off, _ptr(b), _ptr(sb), Nb, b_off, dtype, D, -INF, _ptr(ei), _ptr(ej),
                                      _ptr(es), cap, _ptr(count), _ptr(parent), n_nodes, _ptr(status), _stream())
    cases = [dict(ei=None, ej=None, es=None, count=None, parent=None, status=None),        # neither output
             dict(a=None), dict(ej=None), dict(count=None), dict(status=None),            # null among the required
             dict(a=host), dict(ei=host), dict(count=host), dict(parent=host), dict(status=host), dict(b=host),      # host pointers
             dict(dtype=3), dict(dtype=-1), dict(D=48), dict(D=0), dict(dtype=1, D=32), dict(dtype=2, D=64),          # dtype / D
             dict(a=a, b=None, Na=65, dtype=2, D=a.shape[1]), dict(a=a, sa=sa, b=a, Nb=65, Na=65, dtype=2, D=a.shape[1]),   # int8, no scales
             dict(cap=-1), dict(a_off=-1), dict(b_off=-1), dict(Na=-1), dict(Nb=-1), dict(n_nodes=-1),
             dict(a_off=big - 69), dict(b_off=big - 129), dict(b=None, a_off=big - 69)]
    for kw in cases:
        assert call(**kw) == PFR_ERR_ARG, kw
    from pets_face_recognition_amd._hip import lib
    for bad in (lambda: lib.pfr_cc_union(parent.data_ptr(), 130, host.data_ptr(), ei.data_ptr(), 8, status.data_ptr(), _stream()),
                lambda: lib.pfr_cc_union(0, 130, ei.data_ptr(), ej.data_ptr(), 8, status.data_ptr(), _stream()),
                lambda: lib.pfr_cc_union(parent.data_ptr(), 130, ei.data_ptr(), ej.data_ptr(), 8, 0, _stream()),
                lambda: lib.pfr_cc_flatten(parent.data_ptr(), 130, host.data_ptr(), _stream()),
                lambda: lib.pfr_cc_flatten(0, 130, ei.data_ptr(), _stream())):
        with pytest.raises(Exception, match="rc=-1"):
            bad()
    torch.cuda.synchronize()
    assert bool((ei == CANARY).all()) and bool((ej == CANARY).all()) and bool((es == float(CANARY)).all())
    assert int(count) == 0 and int(status) == 0 and torch.equal(parent.cpu(), torch.arange(130, dtype=I32)) and not bool(host.any())
    # the offsets at the very edge of int32 are still fine, and the empty shapes return 0 without looking at anything
    assert call(a_off=big - 70, b_off=big - 130, cap=0, parent=None, status=None) == 0
    assert call(Na=0, a=None) == 0 and call(Nb=0, b=host) == 0 and call(b=None, Na=1) == 0
    torch.cuda.synchronize()
    assert int(count) == 70 * 130 and bool((ei == CANARY).all())


# ---- 7. end to end
@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_reports_the_same_values_on_the_device(method):
    from test_cluster_host import _controller, _cluster_keys, separated_set
    emb, classes = separated_set()
    # (numeric thresholds far from every score of the set; 'opt' is a score of the set itself — the weakest sampled genuine pair — where
    #  the last bit of either path's normalisation decides, and is covered on the host)
    thrs = [0.9, 0.75]
    extra = {"cluster": dict(thresholds=thrs)}
    c_cpu, batches, _, _ = _controller(extra, emb, classes)
    m_cpu = getattr(c_cpu, method)([batches])["Val"]
    c_dev, batches, _, _ = _controller(extra, emb, classes)
    dev_batches = [{k: v.to(DEV) for k, v in b.items()} for b in batches]
    m_dev = getattr(c_dev, method)([dev_batches])["Val"]
    keys = _cluster_keys(thrs)
    assert list(m_dev.keys())[-len(keys):] == keys
    for k in keys:
        assert m_dev[k] == m_cpu[k], k
    assert m_dev["Cluster F thr=0.9"] == 1.0 and m_dev["Clusters thr=0.9"] == 20
