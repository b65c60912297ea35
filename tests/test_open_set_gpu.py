"""Open-set identification on the device: pfr_class_extremes, pfr_extremes_decode and match.class_extremes / open_set_metrics.

As in tests/test_cluster_gpu.py and tests/test_dbscan_gpu.py the expected values are computed over the scores pfr_pair_scores_gather
returns for ALL the columns of every row (the same tile code, tested on its own), so every comparison is on the kernels' own score bits
and is EXACT for every dtype: no tolerance anywhere in this file.  Expected keys are the oracle (tests/open_set_oracle.py) over those
scores.  The prepared operands and gathered scores are the cached cases of test_cluster_gpu.py (computed once, shared, never modified);
shapes that file does not have are cached here and RELEASED when this module is done, so that no device memory of these tests stays
allocated under the tests that run after them."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import open_set_oracle as OO
from test_cluster_gpu import _case as _shared_case, _ptr, _stream, DTYPES, DIMS, SHAPES, DEV, I32, PFR_ERR_ARG

pytestmark = pytest.mark.gpu
SIZES = [2, 63, 64, 65, 127, 128, 129, 300]
SMALLEST_D = {torch.float32: 32, torch.bfloat16: 64, torch.int8: 128}
CANARY = -7
ROOM = 16
I64 = torch.int64
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _own_case(Na, Nb, D, dtype):
    return _shared_case.__wrapped__(Na, Nb, D, dtype)


def _case(Na, Nb, D, dtype):
    """test_cluster_gpu's cached case where it has the shape, this module's own (released at the end) otherwise"""
    return (_shared_case if (Na, Nb) in SHAPES and D in DIMS else _own_case)(Na, Nb, D, dtype)


@pytest.fixture(scope="module", autouse=True)
def _release_own_cases():
    yield
    _own_case.cache_clear()


def _dll():
    from pets_face_recognition_amd._hip.lib import lib as L
    L._load()
    return L._dll


def _tid(dtype):
    from pets_face_recognition_amd._hip import dtype_id
    return dtype if isinstance(dtype, int) else dtype_id(dtype)


def _new_keys(n_nodes, kinds=3):
    keys = [torch.full((n_nodes + ROOM,), CANARY, dtype=I64, device=DEV) for _ in range(kinds)]
    for k in keys:
        k[:n_nodes] = 0
    return keys


def _raw(a, sa, dtype, cls, blocks=None, off=0, n_nodes=None, worst=True, keys=None):
    """pfr_class_extremes on ONE node set, outputs with ROOM canary elements behind them.  blocks: the row ranges of a blocked run (a
    symmetric launch per block, a two-set both_sides=1 launch per pair of blocks).  -> (rcs, [best_pos, best_neg, worst_pos])"""
    N = a.shape[0]
    n_nodes = off + N if n_nodes is None else n_nodes
    keys = _new_keys(n_nodes) if keys is None else keys
    c = cls.to(device=DEV, dtype=I32).contiguous()
    blocks = blocks or [(0, N)]
    sp = lambda r: 0 if sa is None else sa[r:].data_ptr()
    rcs = []
    for k, (r0, r1) in enumerate(blocks):
        for c0, c1 in [(None, None)] + blocks[k + 1:]:
            head = (a[r0:].data_ptr(), sp(r0), r1 - r0, off + r0) + ((0, 0, 0, 0) if c0 is None else (a[c0:].data_ptr(), sp(c0), c1 - c0, off + c0))
            rcs.append(_dll().pfr_class_extremes(*head, _tid(dtype), a.shape[1], c[r0:].data_ptr(), 0 if c0 is None else c[c0:].data_ptr(), 1,
                                                 keys[0].data_ptr(), keys[1].data_ptr(), keys[2].data_ptr() if worst else 0, n_nodes, _stream()))
    torch.cuda.synchronize()
    return rcs, keys


def _decode(keys, n):
    """pfr_extremes_decode of the three key arrays -> six host lists of n, canaries checked"""
    out = []
    for kind, k in ((0, keys[0]), (0, keys[1]), (1, keys[2])):
        score = torch.full((n + ROOM,), float(CANARY), dtype=torch.float32, device=DEV)
        index = torch.full((n + ROOM,), CANARY, dtype=I32, device=DEV)
        assert _dll().pfr_extremes_decode(k.data_ptr(), n, kind, score.data_ptr(), index.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert bool((score[n:] == CANARY).all()) and bool((index[n:] == CANARY).all())
        out += [score[:n].tolist(), index[:n].tolist()]
    return tuple(out)


def _intact(n, keys):
    return all(bool((k[n:] == CANARY).all()) for k in keys)


def _unsigned(keys, n):
    return [OO.as_unsigned(k[:n].cpu()) for k in keys]


def _gather(a, sa, dtype, b=None, sb=None):
    """every score of the prepared operands (NaN allowed, unlike _case)"""
    from pets_face_recognition_amd._hip import lib
    Na, nb = a.shape[0], (a if b is None else b).shape[0]
    col = torch.arange(nb, dtype=I32, device=DEV).expand(Na, nb).contiguous()
    out = torch.zeros((Na, nb), dtype=torch.float32, device=DEV)
    lib.pfr_pair_scores_gather(_ptr(a), _ptr(sa), Na, _ptr(b), _ptr(sb), 0 if b is None else nb, _tid(dtype), a.shape[1], col.data_ptr(), nb,
                               out.data_ptr(), _stream())
    return out.cpu()


# ---- 1. keys, decoded scores and indices equal the oracle
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", SIZES)
def test_keys_and_decoded_values_equal_the_oracle(N, dtype):
    for D in (SMALLEST_D[dtype], 200):
        a, sa, _, _, S, _ = _case(N, None, D, dtype)
        for name, cls in OO.class_patterns(N, N + D).items():
            want = OO.extremes(S, cls.tolist())
            rcs, keys = _raw(a, sa, dtype, cls)
            assert set(rcs) == {0} and _intact(N, keys), (N, D, dtype, name)
            assert _unsigned(keys, N) == want, (N, D, dtype, name)
            assert _decode(keys, N) == OO.decoded(want), (N, D, dtype, name)


def test_across_a_super_tile_edge():
    N, D = 2049, 64
    a, sa, _, _, S, _ = _case(N, None, D, torch.bfloat16)
    cls = OO.class_patterns(N, 9)["negative"]
    rcs, keys = _raw(a, sa, torch.bfloat16, cls)
    assert set(rcs) == {0} and _intact(N, keys)
    want = OO.extremes_torch(S, cls)
    for got, w in zip(keys, want):
        assert torch.equal(got[:N].cpu(), w)
    assert int((want[0] != 0).sum()) > N // 2 and int((want[0] == 0).sum()) > N // 8 and bool((want[1] != 0).all())      # every kind of row


# ---- 2. ties, NaN, signed zeros
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_duplicated_rows_and_a_nan_row(dtype):
    from pets_face_recognition_amd.match import _hist_operand
    from test_open_set_host import int_rows
    N = 130
    x = int_rows(N, 64, 5, nan_row=70)
    a, sa = _hist_operand(x.to(DEV), dtype, False)
    S = _gather(a, sa, dtype)
    assert S[0, 3] == S[0, N - 1] and bool(torch.isnan(S[70, 80])) and bool(torch.isnan(S[5, 70]))     # the premises
    for name, cls in OO.class_patterns(N, 3).items():
        want = OO.extremes(S, cls.tolist())
        rcs, keys = _raw(a, sa, dtype, cls)
        assert set(rcs) == {0} and _intact(N, keys) and _unsigned(keys, N) == want, name
        d = _decode(keys, N)
        assert d == OO.decoded(want)
        assert d[1][70] == -1 and d[3][70] == -1 and d[5][70] == -1 and 70 not in d[1] and 70 not in d[3]       # the NaN row: nothing, nobody's partner
    # one class: rows 0, 3 and N - 1 are the same row, so everybody scores the same against them — the smallest index is kept
    _, keys = _raw(a, sa, dtype, torch.zeros(N, dtype=I64))
    d = _decode(keys, N)
    assert all(p != N - 1 and (p != 3 or x_ == 0) for x_, p in enumerate(d[1]) if p >= 0)


def test_signed_zero_scores_tie():
    """int8 rows of zeros: the accumulator is 0 and the score is (0 * sa) * sb — node 0 carries the scale -1, so its scores are -0.0, node 1
    the scale +1, +0.0.  The other nodes sit on axes of their own: every score of the set is a zero.  With -0.0 canonicalised all of them
    tie and the smallest index wins — node 0 for everybody else; compared as raw bit patterns +0.0 (node 1) would beat -0.0 (node 0)."""
    n = 9
    q = torch.zeros(n, 128, dtype=torch.int8)
    for k in range(2, n):
        q[k, k] = 4
    sc = torch.ones(n)
    sc[0] = -1.0
    q, sc = q.to(DEV), sc.to(DEV)
    S = _gather(q, sc, 2)
    assert bool((S.triu(1) == 0).all()) and bool(torch.signbit(S[0, 5])) and not bool(torch.signbit(S[1, 5]))          # the premise
    for cls in (torch.arange(n), torch.zeros(n, dtype=I64)):
        want = OO.extremes(S, cls.tolist())
        rcs, keys = _raw(q, sc, 2, cls)
        assert set(rcs) == {0} and _intact(n, keys) and _unsigned(keys, n) == want
        d = _decode(keys, n)
        best = d[3] if int(cls[1]) == 1 else d[1]
        assert best == [1] + [0] * (n - 1)
        k = keys[1] if int(cls[1]) == 1 else keys[0]
        assert (int(k[5]) & (2 ** 64 - 1)) == (0x80000000 << 32) | 0xFFFFFFFF                                    # ord(+0.0), node 0


# ---- 3. blocks, the one-sided form, worst_pos = NULL, determinism
@pytest.mark.parametrize("dtype", DTYPES)
def test_blocked_run_equals_one_launch(dtype):
    N, D = 300, 200
    a, sa, _, _, S, _ = _case(N, None, D, dtype)
    for name in ("threes", "negative"):
        cls = OO.class_patterns(N, 21)[name]
        _, one = _raw(a, sa, dtype, cls)
        rcs, blk = _raw(a, sa, dtype, cls, blocks=[(0, 100), (100, 228), (228, 300)])
        assert set(rcs) == {0} and len(rcs) == 6 and all(torch.equal(x, y) for x, y in zip(one, blk)), (dtype, name)
        # a node set larger than the rows: ids off .. off + N, nothing outside is touched
        off = 37
        rcs, big = _raw(a, sa, dtype, cls, off=off, n_nodes=off + N + 5)
        assert set(rcs) == {0} and _intact(off + N + 5, big)
        for k, w in zip(big, OO.extremes(S, cls.tolist(), a_off=off, n_nodes=off + N + 5)):
            assert OO.as_unsigned(k[:off + N + 5].cpu()) == w
        # worst_pos = NULL leaves the other two unchanged; two runs give equal bits
        _, two = _raw(a, sa, dtype, cls, worst=False)
        assert torch.equal(two[0], one[0]) and torch.equal(two[1], one[1]) and not bool(two[2][:N].any()) and _intact(N, two)
        _, again = _raw(a, sa, dtype, cls)
        assert all(torch.equal(x, y) for x, y in zip(one, again))
        # keys accumulate: a second run over the finished keys changes nothing
        _, acc = _raw(a, sa, dtype, cls, keys=[k.clone() for k in one])
        assert all(torch.equal(x, y) for x, y in zip(one, acc))


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_sided_two_set_form(dtype):
    Na, Nb, D = 130, 200, 64
    a, sa, b, sb, S, _ = _case(Na, Nb, D, dtype)
    a_off, b_off, n_nodes = 11, 5000, 11 + Na + 9
    ca, cb = OO.class_patterns(Na, 1)["negative"], OO.class_patterns(Nb, 2)["threes"]
    ca_d, cb_d = ca.to(device=DEV, dtype=I32), cb.to(device=DEV, dtype=I32)
    keys = _new_keys(n_nodes)
    rc = _dll().pfr_class_extremes(a.data_ptr(), _ptr(sa), Na, a_off, b.data_ptr(), _ptr(sb), Nb, b_off, _tid(dtype), a.shape[1], ca_d.data_ptr(),
                                   cb_d.data_ptr(), 0, keys[0].data_ptr(), keys[1].data_ptr(), keys[2].data_ptr(), n_nodes, _stream())
    torch.cuda.synchronize()
    want = OO.extremes(S, ca.tolist(), cb.tolist(), a_off=a_off, b_off=b_off, n_nodes=n_nodes)
    assert rc == 0 and _intact(n_nodes, keys) and _unsigned(keys, n_nodes) == want
    for k in keys:                                              # nothing outside [a_off, a_off + Na)
        assert not bool(k[:a_off].any()) and not bool(k[a_off + Na:n_nodes].any())
    d = _decode(keys, n_nodes)
    assert d == OO.decoded(want) and min(p for p in d[3][a_off:a_off + Na]) >= b_off


# ---- 4. argument errors and empty shapes: nothing written
def test_argument_errors_write_nothing():
    a8, sa8, _, _, _, _ = _case(65, None, 64, torch.int8)
    af, _, bf, _, _, _ = _case(70, 130, 64, torch.float32)
    n = 200
    keys = [torch.full((n,), 3, dtype=I64, device=DEV) for _ in range(3)]
    cls = torch.zeros(n, dtype=I32, device=DEV)
    score = torch.full((n,), float(CANARY), device=DEV)
    index = torch.full((n,), CANARY, dtype=I32, device=DEV)
    host = torch.zeros(256, dtype=I64)
    big = 2 ** 31 - 1

    def ext(a=af, sa=None, Na=70, a_off=0, b=bf, sb=None, Nb=130, b_off=70, dtype=0, D=64, ca=cls, cb=cls, both=1, pos=keys[0], neg=keys[1],
            worst=keys[2], n_nodes=n):
        return _dll().pfr_class_extremes(_ptr(a), _ptr(sa), Na, a_off, _ptr(b), _ptr(sb), Nb, b_off, dtype, D, _ptr(ca), _ptr(cb), both, _ptr(pos),
                                         _ptr(neg), _ptr(worst), n_nodes, _stream())
    bad = [dict(a=None), dict(pos=None), dict(neg=None), dict(ca=None), dict(cb=None), dict(cb=None, both=0),                  # null pointers
           dict(a=host), dict(b=host), dict(ca=host), dict(cb=host), dict(pos=host), dict(neg=host), dict(worst=host),         # host pointers
           dict(dtype=3), dict(dtype=-1), dict(D=48), dict(D=0), dict(dtype=1, D=32), dict(dtype=2, D=64),                     # dtype / D
           dict(a=a8, b=None, Na=65, dtype=2, D=a8.shape[1]), dict(a=a8, sa=sa8, b=a8, Nb=65, Na=65, dtype=2, D=a8.shape[1]),   # int8, no scales
           dict(Na=-1), dict(Nb=-1), dict(n_nodes=-1), dict(a_off=-1), dict(b_off=-1),                                         # negative sizes
           dict(n_nodes=199), dict(b_off=71), dict(a_off=131), dict(b=None, a_off=131), dict(n_nodes=69, b=None),              # off + rows > n_nodes
           dict(n_nodes=69, both=0), dict(a_off=big - 69, n_nodes=big), dict(b_off=big - 129, n_nodes=big), dict(b_off=big - 128, both=0)]
    for kw in bad:
        assert ext(**kw) == PFR_ERR_ARG, kw

    def dec(k=keys[0], n_=n, kind=0, s=score, i=index):
        return _dll().pfr_extremes_decode(_ptr(k), n_, kind, _ptr(s), _ptr(i), _stream())
    for kw in (dict(k=None), dict(s=None), dict(i=None), dict(k=host), dict(s=host), dict(i=host), dict(n_=-1), dict(kind=2), dict(kind=-1)):
        assert dec(**kw) == PFR_ERR_ARG, kw
    # the empty shapes return 0 without looking at anything
    assert ext(Na=0, a=None, a_off=0) == 0 and ext(Nb=0, b=host, b_off=0) == 0 and ext(b=None, Na=1) == 0 and dec(n_=0, k=None, s=None, i=None) == 0
    torch.cuda.synchronize()
    assert all(bool((k == 3).all()) for k in keys) and bool((score == CANARY).all()) and bool((index == CANARY).all()) and not bool(host.any())
    # the exact fit is accepted, and the one-sided form takes a b_off + Nb beyond n_nodes
    assert ext() == 0 and ext(both=0, b_off=10 ** 6, n_nodes=70) == 0 and dec() == 0 and dec(kind=1, k=keys[2]) == 0
    torch.cuda.synchronize()
    # (one class: every pair is a mate pair — best_pos and worst_pos of all 200 nodes moved away from the 3 they held, best_neg did not; the
    #  keys are unsigned, so the int64 view of a real key may be negative)
    assert bool((keys[0] != 3).all()) and bool((keys[2] != 3).all()) and bool((keys[1] == 3).all()) and bool((index >= 0).all())


# ---- 5. the Python surface
@pytest.mark.parametrize("dtype", DTYPES)
def test_match_class_extremes_equals_its_cpu_path(dtype):
    from pets_face_recognition_amd import match
    g = torch.Generator().manual_seed(4)
    # entries in {-4, 0, 4}, no zero row: exact in fp32 and bf16; in int8 every row has the scale 4 / 127, so equal dots are equal scores
    # and the order of the scores is the order of the dots — the indices are compared for every dtype, the scores where they are exact
    x = 4.0 * torch.randint(-1, 2, (300, 64), generator=g).float()
    y = 4.0 * torch.randint(-1, 2, (130, 64), generator=g).float()
    x[:, 0] = 4.0
    y[:, 0] = 4.0
    x[7], x[200] = x[0], x[0]
    exact = dtype != torch.int8
    for name in ("threes", "negative", "one"):
        cx, cy = OO.class_patterns(300, 5)[name], OO.class_patterns(130, 6)[name]
        for kw in (dict(), dict(emb_b=y, classes_b=cy)):
            cpu = match.class_extremes(x, cx, normalize=False, **kw)
            kd = {k: (v.to(DEV) if k == "emb_b" else v) for k, v in kw.items()}
            for chunk in (None, 128):
                dev = match.class_extremes(x.to(DEV), cx, compute_dtype=dtype, normalize=False, chunk=chunk, **kd)
                for k in (1, 3, 5):
                    assert dev[k].dtype == I64 and dev[k].is_cuda and torch.equal(dev[k].cpu(), cpu[k]), (dtype, name, chunk, k)
                for k in (0, 2, 4):
                    assert dev[k].dtype == torch.float32 and (not exact or torch.equal(dev[k].cpu(), cpu[k])), (dtype, name, chunk, k)
            lean = match.class_extremes(x.to(DEV), cx, compute_dtype=dtype, normalize=False, weakest=False, **kd)
            assert lean.weak_score is None and lean.weak_index is None and torch.equal(lean.pos_index.cpu(), cpu.pos_index)
    # the wrapper's own edge cases on the device
    one = match.class_extremes(x[:1].to(DEV), torch.zeros(1, dtype=I64))
    assert one.pos_index.tolist() == [-1] and one.neg_score.tolist() == [-INF] and one.weak_score.tolist() == [INF]
    assert match.class_extremes(x[:0].to(DEV), torch.zeros(0, dtype=I64)).pos_index.numel() == 0


def _oracle_stats(emb, classes):
    """OpenSetStats over the oracle's extremes of the kernel's own fp32 scores of the normalised rows"""
    from pets_face_recognition_amd.match import _hist_operand
    from pets_face_recognition_amd.engine.metrics import OpenSetStats
    a, sa = _hist_operand(emb.to(DEV), torch.float32, True)
    d = OO.decoded(OO.extremes(_gather(a, sa, torch.float32), classes.tolist()))
    return OpenSetStats(torch.tensor(d[0]), torch.tensor(d[1]), torch.tensor(d[2]), torch.tensor(d[3]))


def test_open_set_metrics_on_the_device():
    from pets_face_recognition_amd import match
    g = torch.Generator().manual_seed(8)
    classes = torch.arange(150) // 3
    emb = torch.randn(50, 64, generator=g)[classes] + 1.6 * torch.randn(150, 64, generator=g)        # loose classes: hits and misses
    classes[::10] = -1
    st = _oracle_stats(emb, classes)
    fpir = (0.1, 0.01, 0.0, 1.0)
    m = match.open_set_metrics(emb.to(DEV), classes, fpir=fpir)
    assert m == st.metrics(fpir) and 0.0 < m["rank1"] < 1.0 and m["DIR@FPIR=0.01"] <= m["DIR@FPIR=0.1"] <= m["DIR@FPIR=1.0"] == m["rank1"]


@pytest.mark.parametrize("method", ["_evaluate", "test_epoch_end"])
def test_controller_reports_the_oracle_values_on_the_device(method):
    from test_cluster_host import _controller, separated_set
    from test_open_set_host import open_set_keys
    emb, classes = separated_set()
    classes = classes.clone()
    classes[0] = 5                                              # one wrong label
    fpirs = [0.1, 0.01]
    c, batches, _, _ = _controller({"open_set": dict(fpir=fpirs)}, emb, classes)
    dev_batches = [{k: v.to(DEV) for k, v in b.items()} for b in batches]
    m = getattr(c, method)([dev_batches])["Val"]
    keys = open_set_keys(fpirs)
    assert list(m.keys())[-len(keys):] == keys
    st = _oracle_stats(emb, classes)
    assert m["OpenSet rank1"] == st.rank1() and m["OpenSet suspects"] >= 1
    for f in fpirs:
        assert m[f"OpenSet DIR@FPIR={f}"] == st.dir_at_fpir(f) and m[f"OpenSet TH@FPIR={f}"] == (st.threshold_at_fpir(f) + 1.0) / 2.0
