"""DBSCAN clustering on the device: pfr_neighbor_count, pfr_dbscan_link, pfr_dbscan_labels and match.neighbor_counts / match.dbscan.

As in tests/test_cluster_gpu.py the expected adjacency comes from pfr_pair_scores_gather over ALL the columns of every row (the same tile
code, tested on its own), so every comparison is on the kernels' own score bits and is EXACT for every dtype: no tolerance anywhere in
this file.  Expected degrees, core sets and labels are the plain-Python oracle (tests/dbscan_oracle.py) over those scores.  The prepared
operands and gathered scores are the cached cases of test_cluster_gpu.py (computed once per session, shared, never modified)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_oracle as DO
from test_cluster_gpu import _case, _ptr, _stream, DTYPES, DIMS, DEV, I32, INF, PFR_ERR_ARG

pytestmark = pytest.mark.gpu
SIZES = [2, 63, 64, 65, 127, 128, 129, 300]
MIN_SAMPLES = (1, 2, 3, 5, 8)
CANARY = -7
ROOM = 16
I64 = torch.int64


def _thresholds(S, valid):
    """the 0.90 / 0.97 / 0.99 quantiles of the gathered scores and one more gathered score: every threshold is a score, equality qualifies"""
    v = S[valid].sort().values
    return [float(v[int(q * (v.numel() - 1))]) for q in (0.90, 0.97, 0.99)] + [float(v[(2 * v.numel()) // 3])]


def _adjacency(S, thr):
    ok = (S >= thr) & torch.ones_like(S, dtype=torch.bool).triu(1)
    return (ok | ok.t()).tolist()


def _rows(N, D):
    """the rows test_cluster_gpu._case(N, None, D, ·) prepared"""
    return torch.randn(N, D, generator=torch.Generator().manual_seed(1000 * N + D))


def _raw(a, sa, dtype, thr, mn, blocks=None, deg=None, link=True, off=0, n_nodes=None):
    """the three entry points on a prepared operand, outputs with ROOM canary elements behind them.  blocks: the row ranges of a blocked
    run (a symmetric launch per block, a two-set launch per pair of blocks).  -> (rcs, deg, parent, best, labels, status)"""
    from pets_face_recognition_amd._hip.lib import lib as L
    from pets_face_recognition_amd._hip import dtype_id
    L._load()
    N = a.shape[0]
    n_nodes = off + N if n_nodes is None else n_nodes
    T = dtype if isinstance(dtype, int) else dtype_id(dtype)
    if deg is None:
        deg = torch.full((n_nodes + ROOM,), CANARY, dtype=I32, device=DEV)
        deg[:n_nodes] = 0
    parent = torch.full((n_nodes + ROOM,), CANARY, dtype=I32, device=DEV)
    parent[:n_nodes] = torch.arange(n_nodes, dtype=I32)
    best = torch.full((n_nodes + ROOM,), CANARY, dtype=I64, device=DEV)
    best[:n_nodes] = 0
    labels = torch.full((n_nodes + ROOM,), CANARY, dtype=I32, device=DEV)
    status = torch.zeros(1, dtype=I32, device=DEV)
    blocks = blocks or [(0, N)]
    launches = []
    for k, (r0, r1) in enumerate(blocks):
        launches.append((r0, r1, None, None))
        launches += [(r0, r1, c0, c1) for c0, c1 in blocks[k + 1:]]
    sp = lambda r: 0 if sa is None else sa[r:].data_ptr()
    rcs = []
    for fn in ("count", "link") if link else ("count",):
        for r0, r1, c0, c1 in launches:
            head = (a[r0:].data_ptr(), sp(r0), r1 - r0, off + r0) + ((0, 0, 0, 0) if c0 is None else (a[c0:].data_ptr(), sp(c0), c1 - c0, off + c0))
            if fn == "count":
                rcs.append(L._dll.pfr_neighbor_count(*head, T, a.shape[1], thr, deg.data_ptr(), n_nodes, _stream()))
            else:
                rcs.append(L._dll.pfr_dbscan_link(*head, T, a.shape[1], thr, deg.data_ptr(), mn, parent.data_ptr(), best.data_ptr(), n_nodes,
                                                  status.data_ptr(), _stream()))
    if link:
        rcs.append(L._dll.pfr_dbscan_labels(parent.data_ptr(), deg.data_ptr(), best.data_ptr(), mn, n_nodes, labels.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return rcs, deg, parent, best, labels, status


def _canaries_intact(n, *tensors):
    return all(bool((t[n:] == CANARY).all()) for t in tensors)


# ---- 1. counts, core set and labels equal the oracle
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", SIZES)
def test_counts_core_set_and_labels_equal_the_oracle(N, dtype):
    from pets_face_recognition_amd import match
    for D in DIMS:
        a, sa, _, _, S, valid = _case(N, None, D, dtype)
        x = _rows(N, D).to(DEV)
        every_kind = False
        for k, thr in enumerate(_thresholds(S, valid)):
            adj = _adjacency(S, thr)
            cnt = match.neighbor_counts(x, thr, compute_dtype=dtype)
            assert cnt.dtype == I64 and cnt.is_cuda and cnt.tolist() == [sum(r) for r in adj], (N, D, dtype, k)
            for ms in MIN_SAMPLES:
                deg, core, want = DO.dbscan(S, thr, ms, adj=adj)
                labels, cmask = match.dbscan(x, thr, min_samples=ms, compute_dtype=dtype, return_core=True)      # (raises when status is set)
                assert labels.dtype == I64 and cmask.dtype == torch.bool
                assert cmask.tolist() == core and labels.tolist() == want, (N, D, dtype, k, ms)
                nc, nb, nn, ncl = DO.kinds(core, want)
                every_kind |= nc >= 1 and nb >= 1 and nn >= 1 and ncl >= 2
        # a grid that never sees a border or a noise point would hide failures
        assert every_kind or N < 63, (N, D, dtype)


# ---- 2. the raw entry points
@pytest.mark.parametrize("dtype", DTYPES)
def test_raw_entry_points_canaries_accumulation_and_offsets(dtype):
    for N, D, ms in ((129, 200, 3), (300, 64, 5)):
        a, sa, _, _, S, valid = _case(N, None, D, dtype)
        thr = _thresholds(S, valid)[1]
        deg_w, core_w, want = DO.dbscan(S, thr, ms, adj=_adjacency(S, thr))
        rcs, deg, parent, best, labels, status = _raw(a, sa, dtype, thr, ms - 1)
        assert set(rcs) == {0} and int(status) == 0
        assert deg[:N].tolist() == deg_w and labels[:N].tolist() == want, (N, D, dtype)
        assert _canaries_intact(N, deg, parent, best, labels)
        assert bool((parent[:N].cpu() <= torch.arange(N)).all()) and bool((parent[:N] >= 0).all())
        # only border nodes carry a key, and it decodes to a qualifying core neighbour
        key = best[:N].cpu()
        for x in range(N):
            has = int(key[x]) != 0
            assert has == ((not core_w[x]) and want[x] >= 0), x
            if has:
                c = 0xFFFFFFFF - (int(key[x]) & 0xFFFFFFFF)
                assert core_w[c] and S[min(x, c), max(x, c)] >= thr
        # deg ACCUMULATES: a second count launch on the same array doubles it (and writes nothing else)
        rcs2, deg2, *_ = _raw(a, sa, dtype, thr, ms - 1, deg=deg.clone(), link=False)
        assert set(rcs2) == {0} and deg2[:N].tolist() == [2 * d for d in deg_w] and _canaries_intact(N, deg2)
        # a blocked run with node offsets — two and three blocks, cut off the tile grid — reproduces the one-launch result
        for blocks in ([(0, 70), (70, N)], [(0, 1), (1, 128), (128, N)]):
            rcs3, deg3, parent3, best3, labels3, status3 = _raw(a, sa, dtype, thr, ms - 1, blocks=blocks)
            assert set(rcs3) == {0} and int(status3) == 0
            assert torch.equal(deg3, deg) and torch.equal(labels3, labels) and torch.equal(best3, best), (N, D, dtype, blocks)
        # a node set larger than the rows (ids off .. off + N): the nodes outside are noise, untouched by the launches
        off = 37
        rcs4, deg4, parent4, best4, labels4, status4 = _raw(a, sa, dtype, thr, ms - 1, off=off, n_nodes=off + N + 5)
        assert set(rcs4) == {0} and int(status4) == 0 and deg4[off:off + N].tolist() == deg_w
        assert labels4[off:off + N].tolist() == [l + off if l >= 0 else -1 for l in want]
        outside = list(range(off)) + list(range(off + N, off + N + 5))
        assert bool((deg4[outside] == 0).all()) and labels4[outside].tolist() == ([-1] * len(outside) if ms > 1 else outside)
        assert _canaries_intact(off + N + 5, deg4, parent4, best4, labels4)


def test_chunked_launches_and_repeated_calls_give_identical_labels():
    from pets_face_recognition_amd import match
    N, D = 300, 200
    x = _rows(N, D).to(DEV)
    for dtype in DTYPES:
        _, _, _, _, S, valid = _case(N, None, D, dtype)
        for thr in _thresholds(S, valid)[1:3]:
            cnt = match.neighbor_counts(x, thr, compute_dtype=dtype)
            assert torch.equal(match.neighbor_counts(x, thr, compute_dtype=dtype, chunk=128), cnt)
            assert torch.equal(match.neighbor_counts(x, thr, compute_dtype=dtype, chunk=N), cnt)
            for ms in (3, 5):
                one, core = match.dbscan(x, thr, min_samples=ms, compute_dtype=dtype, return_core=True)
                for chunk in (128, N):
                    l2, c2 = match.dbscan(x, thr, min_samples=ms, compute_dtype=dtype, chunk=chunk, return_core=True)
                    assert torch.equal(l2, one) and torch.equal(c2, core), (dtype, thr, ms, chunk)
                assert torch.equal(match.dbscan(x, thr, min_samples=ms, compute_dtype=dtype), one)          # two calls: the same labels
            # min_samples=1: every node is core, the result is match.cluster's
            assert torch.equal(match.dbscan(x, thr, min_samples=1, compute_dtype=dtype), match.cluster(x, thr, compute_dtype=dtype))


# ---- 3. border ties on exact scores
@pytest.mark.parametrize("dtype", DTYPES)
def test_border_ties_on_exact_scores(dtype):
    from pets_face_recognition_amd import match
    from test_dbscan_host import exact_tie_rows
    x, want = exact_tie_rows()
    for chunk in (None, 4):
        labels, core = match.dbscan(x.to(DEV), 8.0, min_samples=4, compute_dtype=dtype, normalize=False, chunk=chunk, return_core=True)
        assert labels.tolist() == want["labels"] and core.tolist() == want["core"], (dtype, chunk)
    assert match.neighbor_counts(x.to(DEV), 8.0, compute_dtype=dtype, normalize=False).tolist() == [3, 4, 4, 4, 4, 4, 4, 3, 2, 2, 2]
    # the set in another order: still the oracle's labels (the smallest core index, the smallest tied neighbour)
    perm = torch.tensor([10, 4, 9, 0, 5, 8, 1, 6, 2, 7, 3])
    S = x[perm] @ x[perm].t()                                    # exact integers: the score of every dtype up to the common int8 scale
    assert match.dbscan(x[perm].to(DEV), 8.0, min_samples=4, compute_dtype=dtype, normalize=False).tolist() == DO.dbscan(S, 8.0, 4)[2]


def test_signed_zero_scores_tie():
    """A -0.0 score needs a negative factor behind a zero accumulator (the accumulators start at +0 and (+0) + (-0) = +0), so the pair of
    zeros is built on the raw int8 entry points: node 1 is stored NEGATED with the scale -1 — the same real row, every score unchanged,
    but its zero dot products come out as -0.0.  Cliques {0, 1, 2, 3} and {4, 5, 6, 7} (16 or 17 within, -15 or -16 across); node 8 scores
    -0.0 with node 1, +0.0 with node 5 and -1 with the other cores.  Threshold 0.0, 3 neighbours: node 8 is a border node whose two
    candidates tie once -0.0 is canonicalised, so the smaller index (node 1, cluster 0) wins; compared as raw bit patterns +0.0 would win
    and node 8 would land in cluster 4."""
    from pets_face_recognition_amd._hip import lib
    q = torch.zeros(9, 128, dtype=torch.int8)
    q[0:4, 0], q[4:8, 0] = 4, -4
    q[0:8, 1] = 1
    q[1, 1] = q[5, 1] = 0
    q[8, 1] = -1
    sc = torch.ones(9)
    q[1], sc[1] = -q[1], -1.0
    q, sc = q.to(DEV), sc.to(DEV)
    col = torch.arange(9, dtype=I32, device=DEV).expand(9, 9).contiguous()
    out = torch.full((9, 9), float("nan"), device=DEV)
    lib.pfr_pair_scores_gather(q.data_ptr(), sc.data_ptr(), 9, 0, 0, 0, 2, 128, col.data_ptr(), 9, out.data_ptr(), _stream())
    S = out.cpu()
    assert S[1, 8] == 0 and bool(torch.signbit(S[1, 8])) and S[5, 8] == 0 and not bool(torch.signbit(S[5, 8]))      # the premise
    assert S[0, 1] == 16 and S[1, 2] == 16 and S[0, 2] == 17 and S[1, 4] == -16 and S[0, 8] == -1
    deg_w, core_w, want = DO.dbscan(S, 0.0, 4)
    assert core_w == [True] * 8 + [False] and want == [0] * 4 + [4] * 4 + [0]
    rcs, deg, parent, best, labels, status = _raw(q, sc, 2, 0.0, 3)
    assert set(rcs) == {0} and int(status) == 0
    assert deg[:9].tolist() == deg_w == [3, 4, 3, 3, 3, 4, 3, 3, 2] and labels[:9].tolist() == want
    assert int(best[8]) & (2 ** 64 - 1) == (0x80000000 << 32) | (0xFFFFFFFF - 1)          # ord(+0.0), node 1
    assert _canaries_intact(9, deg, parent, best, labels)


# ---- 4. contention
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cross_workgroup_contention(dtype):
    """8 classes of 128 interleaved as i % 8 (every class spans every row tile: every workgroup adds to the same degrees and hooks into
    the same 8 trees), plus one extra row per class that qualifies against exactly ONE node of it — node c, through a private axis.
    Degrees: 127 inside a class, 128 for the nodes 0 .. 7 (their extra), 1 for the extras.
      min_samples=128: every class member is core, the classes are the clusters, the extras are border nodes.
      min_samples=129: only the nodes 0 .. 7 are core (the extra is their 128th neighbour); their 127 class mates and the extra are
                       border nodes of theirs — the same labels from a different core set.  (Everything is noise one step later.)
      min_samples=130: nobody is core: everything is noise."""
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd.match import _hist_operand
    N = 1024
    cls = torch.arange(N) % 8
    x = torch.zeros(N + 8, 64)
    x[torch.arange(N), cls] = 8.0                                # same class: 64, different class: 0 — exact in every dtype
    x[torch.arange(8), 8 + torch.arange(8)] = 8.0                # node c's private axis ...
    x[N + torch.arange(8), 8 + torch.arange(8)] = 8.0            # ... and the extra row that shares it (64 with node c, 0 with the rest)
    want = torch.cat([cls, torch.arange(8)])
    degs = torch.cat([torch.full((N,), 127), torch.ones(8, dtype=I64)])
    degs[:8] = 128
    xd = x.to(DEV)
    assert torch.equal(match.neighbor_counts(xd, 32.0, compute_dtype=dtype, normalize=False).cpu(), degs)
    for ms, core in ((128, degs >= 127), (129, degs >= 128)):
        labels, cmask = match.dbscan(xd, 32.0, min_samples=ms, compute_dtype=dtype, normalize=False, return_core=True)
        assert torch.equal(labels.cpu(), want) and torch.equal(cmask.cpu(), core), ms
    labels, cmask = match.dbscan(xd, 32.0, min_samples=130, compute_dtype=dtype, normalize=False, return_core=True)
    assert bool((labels == -1).all()) and not bool(cmask.any())
    # the raw entry points: the status word stays clear and the forest keeps parent[x] <= x
    a, _ = _hist_operand(xd, dtype, False)
    rcs, deg, parent, best, labels, status = _raw(a, None, dtype, 32.0, 127)
    assert set(rcs) == {0} and int(status) == 0 and torch.equal(deg[:N + 8].cpu().long(), degs)
    assert bool((parent[:N + 8].cpu() <= torch.arange(N + 8)).all()) and torch.equal(labels[:N + 8].cpu().long(), want)
    assert _canaries_intact(N + 8, deg, parent, best, labels)


# ---- 5. special values
def test_nan_rows_and_special_thresholds():
    from pets_face_recognition_amd import match
    N = 130
    x = torch.randn(N, 64, generator=torch.Generator().manual_seed(6))
    x[5] = float("nan")
    x[129] = float("nan")
    xd = x.to(DEV)
    clean = torch.tensor([i not in (5, 129) for i in range(N)])
    for dtype in (torch.float32, torch.bfloat16):
        # thr = -inf: every non-NaN pair qualifies, a NaN score never does
        cnt = match.neighbor_counts(xd, -INF, compute_dtype=dtype, normalize=False).cpu()
        assert torch.equal(cnt, torch.where(clean, N - 3, 0))
        labels, core = match.dbscan(xd, -INF, min_samples=2, compute_dtype=dtype, normalize=False, return_core=True)
        assert torch.equal(labels.cpu(), torch.where(clean, 0, -1)) and torch.equal(core.cpu(), clean)       # NaN rows are noise ...
        labels = match.dbscan(xd, -INF, min_samples=1, compute_dtype=dtype, normalize=False).cpu()
        assert torch.equal(labels, torch.where(clean, 0, torch.arange(N)))                                   # ... or singleton clusters
        for thr in (INF, float("nan")):                                                                       # nothing qualifies
            assert not bool(match.neighbor_counts(xd, thr, compute_dtype=dtype, normalize=False).any())
            assert bool((match.dbscan(xd, thr, min_samples=2, compute_dtype=dtype, normalize=False) == -1).all())
            assert torch.equal(match.dbscan(xd, thr, min_samples=1, compute_dtype=dtype, normalize=False).cpu(), torch.arange(N))
    # the wrapper's own edge cases on the device
    from pets_face_recognition_amd._hip import PfrError
    assert match.dbscan(xd[:1], 0.5).tolist() == [-1] and match.dbscan(xd[:1], 0.5, min_samples=1).tolist() == [0]
    assert match.dbscan(xd[:0], 0.5).numel() == 0 and match.neighbor_counts(xd[:1], 0.5).tolist() == [0]
    with pytest.raises(PfrError):
        match.dbscan(xd, 0.5, min_samples=0)


# ---- 6. argument errors: PFR_ERR_ARG and nothing written
def test_argument_errors_write_nothing():
    from pets_face_recognition_amd._hip.lib import lib as L
    a8, sa8, _, _, _, _ = _case(65, None, 64, torch.int8)
    af, _, bf, _, _, _ = _case(70, 130, 64, torch.float32)
    L._load()
    n = 200
    deg = torch.full((n,), 3, dtype=I32, device=DEV)
    parent = torch.arange(n, dtype=I32, device=DEV)
    best = torch.zeros(n, dtype=I64, device=DEV)
    labels = torch.full((n,), CANARY, dtype=I32, device=DEV)
    status = torch.zeros(1, dtype=I32, device=DEV)
    host = torch.zeros(256, dtype=I32)
    big = 2 ** 31 - 1

    def count(a=af, sa=None, Na=70, a_off=0, b=bf, sb=None, Nb=130, b_off=70, dtype=0, D=64, deg=deg, n_nodes=n, **_):
        return L._dll.pfr_neighbor_count(_ptr(a), _ptr(sa), Na, a_off, _ptr(b), _ptr(sb), Nb, b_off, dtype, D, -INF, _ptr(deg), n_nodes, _stream())

    def link(a=af, sa=None, Na=70, a_off=0, b=bf, sb=None, Nb=130, b_off=70, dtype=0, D=64, deg=deg, n_nodes=n, mn=0, parent=parent,
             best=best, status=status):
        return L._dll.pfr_dbscan_link(_ptr(a), _ptr(sa), Na, a_off, _ptr(b), _ptr(sb), Nb, b_off, dtype, D, -INF, _ptr(deg), mn, _ptr(parent),
                                      _ptr(best), n_nodes, _ptr(status), _stream())
    both = [dict(a=None), dict(deg=None), dict(a=host), dict(b=host), dict(deg=host),                                # null / host pointers
            dict(dtype=3), dict(dtype=-1), dict(D=48), dict(D=0), dict(dtype=1, D=32), dict(dtype=2, D=64),            # dtype / D
            dict(a=a8, b=None, Na=65, dtype=2, D=a8.shape[1]), dict(a=a8, sa=sa8, b=a8, Nb=65, Na=65, dtype=2, D=a8.shape[1]),   # int8, no scales
            dict(Na=-1), dict(Nb=-1), dict(n_nodes=-1), dict(a_off=-1), dict(b_off=-1),                                # negative sizes
            dict(n_nodes=199), dict(b_off=71), dict(a_off=131), dict(b=None, a_off=131), dict(n_nodes=69, b=None),     # off + rows > n_nodes
            dict(a_off=big - 69, n_nodes=big), dict(b_off=big - 129, n_nodes=big)]
    for kw in both:
        assert count(**kw) == PFR_ERR_ARG, kw
        assert link(**kw) == PFR_ERR_ARG, kw
    for kw in (dict(mn=-1), dict(parent=None), dict(best=None), dict(status=None), dict(parent=host), dict(best=host), dict(status=host)):
        assert link(**kw) == PFR_ERR_ARG, kw

    def lab(parent=parent, deg=deg, best=best, mn=0, n_nodes=n, labels=labels):
        return L._dll.pfr_dbscan_labels(_ptr(parent), _ptr(deg), _ptr(best), mn, n_nodes, _ptr(labels), _stream())
    for kw in (dict(parent=None), dict(deg=None), dict(best=None), dict(labels=None), dict(parent=host), dict(deg=host), dict(best=host),
               dict(labels=host), dict(mn=-1), dict(n_nodes=-1)):
        assert lab(**kw) == PFR_ERR_ARG, kw
    torch.cuda.synchronize()
    assert bool((deg == 3).all()) and torch.equal(parent.cpu(), torch.arange(n, dtype=I32)) and not bool(best.any())
    assert bool((labels == CANARY).all()) and int(status) == 0 and not bool(host.any())
    # the empty shapes return 0 without looking at anything
    for fn in (count, link):
        assert fn(Na=0, a=None, a_off=0) == 0 and fn(Nb=0, b=host, b_off=0) == 0 and fn(b=None, Na=1) == 0
    assert lab(n_nodes=0, parent=None, labels=None) == 0
    torch.cuda.synchronize()
    assert bool((deg == 3).all()) and bool((labels == CANARY).all())
    # and the exact fit is accepted: a_off + Na == b_off, b_off + Nb == n_nodes
    assert count() == 0 and link(mn=10 ** 6) == 0 and lab(mn=10 ** 6) == 0
    torch.cuda.synchronize()
    assert bool((deg >= 3).all()) and int(deg.sum()) == 3 * n + 2 * 70 * 130 and bool((labels == -1).all()) and int(status) == 0


# ---- 7. end to end
@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_reports_the_same_values_on_the_device(method):
    from test_cluster_host import _controller, separated_set
    from test_dbscan_host import dbscan_keys
    emb, classes = separated_set()
    # (numeric thresholds far from every score of the set, as in test_cluster_gpu.py)
    thrs = [0.9, 0.75]
    extra = {"dbscan": dict(thresholds=thrs, min_samples=3)}
    c_cpu, batches, _, _ = _controller(extra, emb, classes)
    m_cpu = getattr(c_cpu, method)([batches])["Val"]
    c_dev, batches, _, _ = _controller(extra, emb, classes)
    dev_batches = [{k: v.to(DEV) for k, v in b.items()} for b in batches]
    m_dev = getattr(c_dev, method)([dev_batches])["Val"]
    keys = dbscan_keys(thrs)
    assert list(m_dev.keys())[-len(keys):] == keys
    for k in keys:
        assert m_dev[k] == m_cpu[k], k
    assert m_dev["DBSCAN F thr=0.9"] == 1.0 and m_dev["DBSCAN clusters thr=0.9"] == 20 and m_dev["DBSCAN noise thr=0.9"] == 0
