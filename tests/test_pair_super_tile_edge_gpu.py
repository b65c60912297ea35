"""The pair entry points across a super-tile edge (pfr_pair_hist, pfr_pairs_above, pfr_neighbor_count / pfr_dbscan_link symmetric,
pfr_rank_count on two sets): N = 2049 is 17 tiles per side, so the queue (csrc/pfr_tilewalk.h) holds three super-tiles of the upper
triangle — (0, 0), (0, 1) and (1, 1) — and the ragged one-row tile row / column 16.  Two k-steps per row (D = 64 fp32, 128 bf16), so the
prefetch branch of the tile product runs.  The expected values come from pfr_pair_scores_gather on the same operands, bit for bit.
Row 2048 is a copy of row 5 and row 2047 a copy of row 130: their pairs (5, 2048) in tile (0, 16) and (130, 2047) in tile (1, 15)
score 1 and qualify at every threshold, so a tile decoded to the wrong (tm, tn) changes every answer."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_oracle as O
import dbscan_oracle as DO
import test_cluster_gpu as C
import test_dbscan_gpu as DB
import test_pair_hist_gpu as PH

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32
N = 2049
CASES = [(torch.float32, 64), (torch.bfloat16, 128)]


@functools.lru_cache(maxsize=None)
def _case(dtype, D):
    """-> (a, S fp32 [N, N] on the host: the gathered score of every pair, valid: the pairs i < j, thr)"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    from pets_face_recognition_amd.match import _hist_operand
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(2049 + D))
    x[2048] = x[5]
    x[2047] = x[130]
    a, sa = _hist_operand(x.to(DEV), dtype, True)
    assert sa is None
    col = torch.arange(N, dtype=I32, device=DEV).expand(N, N).contiguous()
    out = torch.full((N, N), float("nan"), dtype=torch.float32, device=DEV)
    lib.pfr_pair_scores_gather(a.data_ptr(), 0, N, 0, 0, 0, dtype_id(dtype), a.shape[1], col.data_ptr(), N, out.data_ptr(), C._stream())
    S = out.cpu()
    assert not bool(torch.isnan(S).any())
    valid = torch.ones(N, N, dtype=torch.bool).triu(1)
    v = S[valid].sort().values
    thr = float(v[int(0.9995 * (v.numel() - 1))])            # a gathered score: equality qualifies; about 1 000 pairs
    # the premises: the planted pairs qualify, and so do pairs of the last column's other tiles and of every super-tile
    ok = valid & (S >= thr)
    assert bool(ok[5, 2048]) and bool(ok[130, 2047])
    for r0, r1, c0, c1 in ((0, 128, 0, 128), (0, 128, 1920, 2048), (1920, 2048, 1920, 2048), (0, 2048, 2048, 2049)):
        assert int(ok[r0:r1, c0:c1].sum()) >= 1, (r0, c0)          # tiles (0, 0), (0, 15), (15, 15) and the column of tile column 16
    return a, S, valid, thr


@pytest.mark.parametrize("dtype,D", CASES)
def test_pair_hist(dtype, D):
    a, S, _, _ = _case(dtype, D)
    cls = torch.randint(0, 9, (N,), generator=torch.Generator().manual_seed(3), dtype=I32)
    cls[2048] = cls[5]                                                         # the planted pair of tile (0, 16) is genuine
    bins = 512
    lo, inv_w = PH._lo_invw(bins, -1.0, 1.0)
    want = PH._host_table(S, cls, cls, True, lo, inv_w, bins)
    got = PH._launch(a, None, cls.to(DEV), None, None, None, dtype, lo, inv_w, bins)
    assert torch.equal(got.cpu(), want)
    assert int(want.sum()) == N * (N - 1) // 2 and int(want[1].sum()) > N


@pytest.mark.parametrize("dtype,D", CASES)
def test_pairs_above_edges_and_union(dtype, D):
    a, S, valid, thr = _case(dtype, D)
    wi, wj, ws = C._expected(S, valid, thr)
    parent = torch.arange(N, dtype=I32, device=DEV)
    status = torch.zeros(1, dtype=I32, device=DEV)
    rc, ei, ej, es, count = C._above(a, None, None, None, dtype, thr, cap=wi.numel(), parent=parent, status=status)
    assert rc == 0 and int(count) == wi.numel() and int(status) == 0
    gi, gj, gs = C._sorted_edges(ei, ej, es, wi.numel(), N)
    assert torch.equal(gi, wi) and torch.equal(gj, wj) and torch.equal(gs, ws)
    assert bool((ei[wi.numel():] == C.CANARY).all()) and bool((ej[wi.numel():] == C.CANARY).all())
    want = O.components(N, zip(wi.tolist(), wj.tolist()))
    assert want[2048] == want[5] and want[2047] == want[130]
    assert C._flatten(parent).tolist() == want
    # the union alone (no edge list)
    parent = torch.arange(N, dtype=I32, device=DEV)
    rc, *_ = C._above(a, None, None, None, dtype, thr, parent=parent, status=status, edges=False)
    assert rc == 0 and int(status) == 0 and C._flatten(parent).tolist() == want


@pytest.mark.parametrize("dtype,D", CASES)
@pytest.mark.parametrize("Na,Nb", [(130, 2049), (2049, 130), (2049, 2049)])
def test_rank_count(Na, Nb, dtype, D):
    """the rectangular walk: 2 x 17 and 17 x 2 tiles, two super-tiles each, and 17 x 17 (four super-tiles; tile (16, 16) holds the one
    valid element (2048, 2048), the last threshold of the last row).  Every row has five thresholds — the scores of its columns 0,
    127, 128, Nb - 1 (the ragged last tile column) and one that moves with the row — and a count runs over ALL columns, so every tile
    of the rectangle feeds every row's counts; the last row (2048 of the tall case) sits alone in tile row 16."""
    import retrieval_oracle as RO
    import test_retrieval_gpu as R
    from pets_face_recognition_amd.match import _hist_operand
    g = torch.Generator().manual_seed(Na + D)
    a, _ = _hist_operand(torch.randn(Na, D, generator=g).to(DEV), dtype, True)
    b, _ = _hist_operand(torch.randn(Nb, D, generator=g).to(DEV), dtype, True)
    S = R._gather(a, None, b, None, torch.arange(Nb).expand(Na, Nb), dtype).cpu()
    assert not bool(torch.isnan(S).any())
    rows = torch.arange(Na)
    col = torch.stack([torch.zeros(Na, dtype=torch.int64), torch.full((Na,), 127), torch.full((Na,), 128), torch.full((Na,), Nb - 1),
                       (rows * 7 + 3) % Nb], dim=1)
    npos = torch.full((Na,), col.shape[1])
    thr = R._gather(a, None, b, None, col, dtype).cpu()
    assert torch.equal(thr, torch.gather(S, 1, col))                           # the thresholds are the gathered scores, bit for bit
    ids = torch.arange(Nb)
    got = R._count(a, None, b, None, ids, None, thr, col, npos, dtype).cpu().long()
    want = RO.counts_from_scores(S, ids, thr, col, npos, None)
    assert torch.equal(got, want)
    assert int(want.max()) > Nb // 2 and int(want.min()) < Nb // 8             # thresholds at both ends of the rows' orders


@pytest.mark.parametrize("dtype,D", CASES)
def test_neighbor_count_and_dbscan_link(dtype, D):
    a, S, valid, thr = _case(dtype, D)
    ok = valid & (S >= thr)
    adj_t = ok | ok.t()
    ms = 3
    deg_w, core_w, labels_w = DO.dbscan(S, thr, ms, adj=adj_t.tolist())
    assert deg_w == adj_t.sum(1).tolist()
    nc, nb, nn, ncl = DO.kinds(core_w, labels_w)
    assert nc >= 1 and nb >= 1 and nn >= 1 and ncl >= 2                       # every kind of node
    rcs, deg, parent, best, labels, status = DB._raw(a, None, dtype, thr, ms - 1)
    assert set(rcs) == {0} and int(status) == 0 and DB._canaries_intact(N, deg, parent, best, labels)
    assert deg[:N].tolist() == deg_w
    assert labels[:N].tolist() == labels_w


@pytest.mark.parametrize("dtype,D", CASES)
def test_card_max_scores_with_17_gallery_tiles(dtype, D):
    """16 gallery cards of 100 photos take a tile each (two do not fit 128 rows) and a card of 29 opens the 17th: 2 x 17 tiles, the
    gallery side crosses the super-tile edge and ends in a part-filled tile.  The last gallery card holds a copy of a photo of query
    card 0 and gallery card 15 one of query card 2: their maxima, in tiles (0, 16) and (1, 15), are 1 up to rounding, far above any
    other score of these rows."""
    import test_card_max_gpu as CM
    from pets_face_recognition_amd.match import card_tiles
    qc, gc = [3, 100, 30], [100] * 16 + [29]
    qseg, gseg = CM._offsets(qc), CM._offsets(gc)
    assert card_tiles(qseg).shape[0] == 2 and card_tiles(gseg).shape[0] == 17
    q, g = CM._unit_rows(int(qseg[-1]), D, 1, dtype), CM._unit_rows(int(gseg[-1]), D, 2, dtype)
    g[int(gseg[16]) + 28] = q[1]                                              # query card 0, gallery card 16
    g[int(gseg[15]) + 50] = q[int(qseg[2]) + 7]                               # query card 2, gallery card 15
    want = CM._oracle(q, qseg, g, gseg)
    assert float(want[0, 16]) > 0.99 and float(want[2, 15]) > 0.99 and float(want[0, :16].max()) < 0.9
    got = CM._kernel(q, qseg, g, gseg).cpu()[:, :len(gc)].double()
    assert not bool(torch.isinf(got).any())
    err = float((got - want).abs().max())
    print(f"17 gallery tiles D={D} {dtype}: max |kernel - fp64 oracle| = {err:.3e}")
    assert err < CM.TOL, (D, dtype, err)
