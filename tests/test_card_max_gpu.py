"""Max-strategy card matching on the device: pfr_card_max_scores (photo GEMM with a segmented-max epilogue) and pfr_card_max_rescore against
an fp64 oracle on the SAME rows the kernel reads (fp32 unit rows, or their bf16 rounding), at the smallest shapes where the kernel can go
wrong; card_match(strategy='max') against the oracle ranking; calc_scores(strategy='max') against the rows the reference's own functions
wrote into tests/golden/max_strategy.npz (tools/make_max_strategy_golden.py)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda"
TOL = 2e-6
NINF = -float("inf")


def _offsets(counts):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(counts, dtype=torch.long).cumsum(0)])


def _unit_rows(P, D, seed, dtype):
    """unit rows normalised in fp64, rounded to fp32 and then to `dtype`: exactly what the kernel is given"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, D, generator=g, dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).float().to(dtype)


def _oracle(q, qseg, g, gseg):
    """fp64 max dot per card pair of the rows as given, -inf where a card has no photos"""
    Q, G = qseg.numel() - 1, gseg.numel() - 1
    out = torch.full((Q, G), NINF, dtype=torch.float64)
    if q.shape[0] == 0 or g.shape[0] == 0:
        return out
    s = q.double() @ g.double().t()
    qcard = torch.repeat_interleave(torch.arange(Q), qseg[1:] - qseg[:-1])
    gcard = torch.repeat_interleave(torch.arange(G), gseg[1:] - gseg[:-1])
    cols = torch.full((s.shape[0], G), NINF, dtype=torch.float64).scatter_reduce_(1, gcard[None, :].expand(s.shape[0], -1), s, "amax")
    return out.scatter_reduce_(0, qcard[:, None].expand(-1, G), cols, "amax")


def _kernel(q, qseg, g, gseg, col0=0, n=None, out=None):
    """one pfr_card_max_scores launch on rows as given (fp32 or bf16, D a multiple of the k-step)"""
    from pets_face_recognition_amd._hip import lib, dtype_id
    from pets_face_recognition_amd.match import card_tiles
    Q, G = qseg.numel() - 1, gseg.numel() - 1
    n = G - col0 if n is None else n
    if out is None:
        out = torch.full((Q, (n + 3) // 4 * 4), 7.0, dtype=torch.float32, device=DEV)
    qt, gt = card_tiles(qseg), card_tiles(gseg)
    keep = [q.to(DEV).contiguous(), g.to(DEV).contiguous(), qseg.to(DEV), gseg.to(DEV), qt.to(DEV), gt.to(DEV)]
    lib.pfr_card_max_scores(keep[0].data_ptr(), keep[2].data_ptr(), keep[4].data_ptr(), qt.shape[0], q.shape[0], Q, keep[1].data_ptr(),
                            keep[3].data_ptr(), keep[5].data_ptr(), gt.shape[0], g.shape[0], dtype_id(q.dtype), q.shape[1], col0, n,
                            out.data_ptr(), out.shape[1], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out


def _rescore_all(q, qseg, g, gseg):
    """pfr_card_max_rescore on every pair (candidate lists of at most 512 gallery cards)"""
    from pets_face_recognition_amd._hip import lib
    Q, G = qseg.numel() - 1, gseg.numel() - 1
    qd, gd, qs, gs = q.to(DEV).contiguous(), g.to(DEV).contiguous(), qseg.to(DEV), gseg.to(DEV)
    outs = []
    for c0 in range(0, G, 512):
        kc = min(512, G - c0)
        cand = torch.arange(c0, c0 + kc, dtype=torch.int32, device=DEV).repeat(Q, 1).contiguous()
        o = torch.empty((Q, kc), dtype=torch.float32, device=DEV)
        lib.pfr_card_max_rescore(qd.data_ptr(), qs.data_ptr(), Q, gd.data_ptr(), gs.data_ptr(), G, q.shape[1], cand.data_ptr(), kc, o.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        outs.append(o)
    torch.cuda.synchronize()
    return torch.cat(outs, 1).cpu()


_RS = np.random.RandomState(7)
LAYOUTS = {                                                       # (photos per query card, photos per gallery card)
    "one_query_card": ([3], _RS.randint(1, 6, 40).tolist()),
    "one_tile_each": ([2, 3, 1, 4], [1, 5, 2, 2, 3, 1]),
    "tiles_3x3_ragged": (_RS.randint(1, 6, 100).tolist(), _RS.randint(1, 6, 110).tolist()),     # ~300 x ~330 rows, part-filled last tiles
    "100_plus_29": ([100, 29], [29, 100, 1]),
    "empties_everywhere": ([0, 0, 3, 4, 0], [2, 0, 0, 0, 5, 0, 126, 0, 0, 1, 0]),
    "empty_after_full_tile": ([128, 0, 1], [0, 128, 0, 0, 2]),
    "only_empties_query": ([0, 0, 0], [2, 3]),
    "only_empties_gallery": ([2, 3], [0, 0, 0, 0]),
    "128_beside_singles": ([1, 1, 128, 1, 1], [1] * 130),
    "ragged_0_to_39": (np.random.RandomState(3).randint(0, 40, 200)[:60].tolist(), np.random.RandomState(3).randint(0, 40, 200).tolist()),
    "lone_128": ([128], [128]),
    "lone_empty": ([0], [0]),
}


def _check_case(layout, D, dtype):
    qc, gc = LAYOUTS[layout]
    qseg, gseg = _offsets(qc), _offsets(gc)
    q, g = _unit_rows(int(qseg[-1]), D, 1, dtype), _unit_rows(int(gseg[-1]), D, 2, dtype)
    want = _oracle(q, qseg, g, gseg)
    got = _kernel(q, qseg, g, gseg).cpu()[:, :len(gc)].double()
    empty = torch.isinf(want)
    assert torch.equal(torch.isinf(got) & (got < 0), empty), layout      # -inf in whole rows / columns of the empty cards, nowhere else
    assert bool((empty == ((qseg[1:] == qseg[:-1])[:, None] | (gseg[1:] == gseg[:-1])[None, :])).all())
    if (~empty).any():
        err = float((got - want)[~empty].abs().max())
        print(f"{layout} D={D} {dtype}: max |kernel - fp64 oracle| = {err:.3e}")
        assert err < TOL, (layout, D, dtype, err)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("D,dtype", [(32, torch.float32), (64, torch.bfloat16)])
def test_kernel_vs_fp64_oracle_minimum_ksteps(layout, D, dtype):
    _check_case(layout, D, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", ["tiles_3x3_ragged", "128_beside_singles"])
def test_kernel_vs_fp64_oracle_d512(layout, dtype):
    _check_case(layout, 512, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wrapper_pads_d48(dtype):
    """match.card_max_scores normalises on the device and pads D = 48 to the k-step (32 fp32 / 64 bf16 columns).
    fp32: against the fp64 oracle on fp64-normalised rows.
    bf16: the oracle is evaluated in fp64 on the bf16 rows the wrapper itself prepares (its `_CardSide(...).op`, read back), so the same
    2e-6 tests the kernel and the padding and not the rounding; that those rows ARE the unit rows rounded to bf16 (relative error <= 2^-8 per
    element: the fp32 normalisation and one bf16 rounding) with ZERO pad columns is asserted separately."""
    from pets_face_recognition_amd import match
    qc, gc = LAYOUTS["tiles_3x3_ragged"]
    qseg, gseg = _offsets(qc), _offsets(gc)
    g = torch.Generator().manual_seed(5)
    q, gg = 3.0 * torch.randn(int(qseg[-1]), 48, generator=g), 0.2 * torch.randn(int(gseg[-1]), 48, generator=g)
    unit = lambda x: x.double() / x.double().norm(dim=1, keepdim=True)
    got = match.card_max_scores(q.to(DEV), qseg, gg.to(DEV), gseg, compute_dtype=dtype).cpu().double()
    if dtype == torch.float32:
        want = _oracle(unit(q), qseg, unit(gg), gseg)
    else:
        rows = []
        for x, seg in ((q, qseg), (gg, gseg)):
            op = match._CardSide(x.to(DEV), seg, dtype, DEV, False, "test").op.cpu()
            assert op.dtype == torch.bfloat16 and op.shape == (x.shape[0], 64) and bool((op[:, 48:] == 0).all())
            assert bool(((op[:, :48].double() - unit(x)).abs() <= 2.0 ** -8 * unit(x).abs() + 1e-30).all())
            rows.append(op)
        want = _oracle(rows[0], qseg, rows[1], gseg)
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"D=48 {dtype}: {err:.3e}")
    assert err < TOL


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_all_cosines_negative_stay_negative(dtype):
    """queries around +c, gallery around -c: every cosine is negative.  A padding row that got through (a zero or duplicated row) or a
    zero-initialised table would put a 0 or a larger value into a maximum; the last tiles are part-filled on both axes"""
    D = 64
    qc, gc = np.random.RandomState(13).randint(1, 5, 60).tolist(), [1] * 140 + [3, 2]
    qseg, gseg = _offsets(qc), _offsets(gc)
    g = torch.Generator().manual_seed(11)
    c = torch.randn(D, generator=g, dtype=torch.float64)
    mk = lambda P, sign: sign * c + 0.3 * torch.randn(P, D, generator=g, dtype=torch.float64)
    unit = lambda x: (x / x.norm(dim=1, keepdim=True)).float().to(dtype)
    q, gg = unit(mk(int(qseg[-1]), 1.0)), unit(mk(int(gseg[-1]), -1.0))
    assert int(qseg[-1]) % 128 and int(gseg[-1]) % 128
    want = _oracle(q, qseg, gg, gseg)
    assert float(want.max()) < -0.1
    got = _kernel(q, qseg, gg, gseg).cpu()[:, :len(gc)].double()
    assert float(got.max()) < -0.1 and float((got - want).abs().max()) < TOL


def test_window_leaves_the_rest_untouched():
    qc, gc = LAYOUTS["tiles_3x3_ragged"]
    qseg, gseg = _offsets(qc), _offsets(gc)
    q, g = _unit_rows(int(qseg[-1]), 32, 1, torch.float32), _unit_rows(int(gseg[-1]), 32, 2, torch.float32)
    full = _kernel(q, qseg, g, gseg).cpu()[:, :len(gc)]
    for col0, n, ld in ((37, 41, 52), (1, 1, 4), (len(gc) - 3, 3, 8)):
        out = torch.full((len(qc), ld), 7.0, dtype=torch.float32, device=DEV)
        got = _kernel(q, qseg, g, gseg, col0=col0, n=n, out=out).cpu()
        assert torch.equal(got[:, :n], full[:, col0:col0 + n]), (col0, n)
        assert bool((got[:, n:] == 7.0).all()), (col0, n)
    # the chunked caller passes only the tiles of its window: same result
    from pets_face_recognition_amd import match
    qs = match._CardSide(q.to(DEV), qseg, torch.float32, DEV, False, "test")
    gs = match._CardSide(g.to(DEV), gseg, torch.float32, DEV, False, "test")
    t0, t1 = gs.tile_range(60, 30)
    assert 0 < t0 < t1 <= gs.tiles_h.shape[0] and t1 - t0 < gs.tiles_h.shape[0]
    out = torch.full((len(qc), 32), 7.0, dtype=torch.float32, device=DEV)
    match._card_max_chunk(qs, gs, torch.float32, 60, 30, out, 32)
    ref = match.card_max_scores(q.to(DEV), qseg, g.to(DEV), gseg)[:, 60:90]
    assert torch.equal(out[:, :30], ref) and bool((out[:, 30:] == 7.0).all())


def test_deterministic_and_equal_to_the_rescore_kernel():
    """two calls give the same bits; in fp32 the segmented max of the tile kernel and pfr_card_max_rescore on every pair give the same bits
    (both accumulate each dot product in the same k order); D = 40 for the re-scoring alone exercises its zero-filled last k-group"""
    for layout, D in (("tiles_3x3_ragged", 64), ("128_beside_singles", 32), ("empties_everywhere", 32)):
        qc, gc = LAYOUTS[layout]
        qseg, gseg = _offsets(qc), _offsets(gc)
        q, g = _unit_rows(int(qseg[-1]), D, 3, torch.float32), _unit_rows(int(gseg[-1]), D, 4, torch.float32)
        a = _kernel(q, qseg, g, gseg).cpu()[:, :len(gc)]
        b = _kernel(q, qseg, g, gseg).cpu()[:, :len(gc)]
        assert torch.equal(a, b)
        assert torch.equal(a, _rescore_all(q, qseg, g, gseg)), layout
    qc, gc = LAYOUTS["one_tile_each"]
    qseg, gseg = _offsets(qc), _offsets(gc)
    q, g = _unit_rows(int(qseg[-1]), 40, 3, torch.float32), _unit_rows(int(gseg[-1]), 40, 4, torch.float32)
    pad = lambda x: torch.nn.functional.pad(x, (0, 24))
    assert torch.equal(_rescore_all(q, qseg, g, gseg), _kernel(pad(q), qseg, pad(g), gseg).cpu()[:, :len(gc)])
    # padding entries and cards outside the gallery are -inf
    from pets_face_recognition_amd._hip import lib
    cand = torch.tensor([[0, -1, len(gc), 1]] * len(qc), dtype=torch.int32, device=DEV)
    o = torch.zeros((len(qc), 4), dtype=torch.float32, device=DEV)
    lib.pfr_card_max_rescore(q.to(DEV).data_ptr(), qseg.to(DEV).data_ptr(), len(qc), g.to(DEV).data_ptr(), gseg.to(DEV).data_ptr(), len(gc), 40,
                             cand.data_ptr(), 4, o.data_ptr(), torch.cuda.current_stream().cuda_stream)
    o = o.cpu()
    assert bool(torch.isinf(o[:, 1:3]).all()) and bool(torch.isfinite(o[:, [0, 3]]).all())


def _check_order(idx, sc, ref, tol=TOL):
    """near-tie rule of tests/test_match_gpu.py::_check_calc_scores for one modality: reference order = score descending, ties to the lower
    index; two cards may be swapped only when their reference scores are closer than the tolerance; every query is checked"""
    for qi in range(ref.shape[0]):
        r = ref[qi]
        want = sorted([j for j in range(len(r)) if np.isfinite(r[j])], key=lambda j: (-r[j], j))[:idx.shape[1]]
        n = len(want)
        got = idx[qi, :n].tolist()
        assert (idx[qi, n:] == -1).all() and np.isinf(sc[qi, n:]).all()
        assert n == idx.shape[1] or sorted(got) == sorted(want)
        for p, (a, b) in enumerate(zip(got, want)):
            assert abs(sc[qi, p] - r[a]) < tol, (qi, p, sc[qi, p], r[a])
            if a != b:
                assert abs(r[a] - r[b]) < tol, (qi, p, a, b)


def test_card_match_max_vs_oracle_ranking():
    """17 x 230 cards as in test_card_match_mean_strategy_vs_reference_formula; fp32 and bf16 (selected on bf16 scores, returned scores
    re-scored in fp32: they meet the fp32 tolerance, which bf16-input scores would miss by three orders of magnitude)"""
    from pets_face_recognition_amd.match import card_match
    g = torch.Generator().manual_seed(8)
    D, nq, ng = 512, 17, 230
    qn = torch.randint(1, 5, (nq,), generator=g); gn = torch.randint(1, 6, (ng,), generator=g)
    qseg, gseg = _offsets(qn.tolist()), _offsets(gn.tolist())
    centers = torch.randn(40, D, generator=g)
    gcls = torch.randint(0, 40, (ng,), generator=g); qcls = torch.randint(0, 40, (nq,), generator=g)
    gemb = torch.cat([centers[gcls[i]] + 1.5 * torch.randn(int(gn[i]), D, generator=g) for i in range(ng)])
    qemb = torch.cat([centers[qcls[i]] + 1.5 * torch.randn(int(qn[i]), D, generator=g) for i in range(nq)])
    unit = lambda x: x.double() / x.double().norm(dim=1, keepdim=True)
    ref = ((_oracle(unit(qemb), qseg, unit(gemb), gseg) + 1) / 2).clamp_min(0).numpy()
    res = {}
    for dt in (torch.float32, torch.bfloat16):
        for k, chunk in ((100, 131072), (10, 64)):              # one gallery chunk / several
            sc, idx = card_match(qemb.to(DEV), qseg, gemb.to(DEV), gseg, k=k, compute_dtype=dt, strategy="max", chunk=chunk)
            torch.cuda.synchronize()
            assert sc.shape == idx.shape == (nq, k)
            _check_order(idx.cpu().numpy(), sc.cpu().numpy(), ref)
            res[dt, k] = (sc.cpu(), idx.cpu())
    # The bf16 returned scores ARE the fp32 ones, bit for bit: the re-scoring reads the fp32 path's own operand rows and accumulates in
    # the fp32 tile kernel's k order.  k = 100: kc = 250 covers all 230 cards, so the whole lists are equal; k = 10 (kc = 38 of 230, a
    # selection that is not certified): exact wherever the two lists name the same card.
    assert torch.equal(res[torch.float32, 100][0], res[torch.bfloat16, 100][0])
    assert torch.equal(res[torch.float32, 100][1], res[torch.bfloat16, 100][1])
    (s32, i32), (sbf, ibf) = res[torch.float32, 10], res[torch.bfloat16, 10]
    same = i32 == ibf
    assert float(same.float().mean()) > 0.9 and torch.equal(s32[same], sbf[same])


def _check_calc_scores(res_idx, res_sc, cnt, top1, m3, m10, rows):
    """tests/test_match_gpu.py::_check_calc_scores, restated"""
    have = {r[0]: r for r in rows}
    for qi in range(res_idx.shape[0]):
        if qi not in have:
            assert cnt[qi] == 0 and (res_idx[qi] == -1).all()
            continue
        _, t1, rm3, rm10, ans = have[qi]
        n = len(ans)
        assert cnt[qi] == n and (res_idx[qi, n:] == -1).all()
        assert abs(top1[qi] - t1) < TOL and abs(m3[qi] - rm3) < TOL and abs(m10[qi] - rm10) < TOL
        got = res_idx[qi, :n].tolist()
        assert sorted(got) == sorted(ans) or n == 100
        sc = res_sc[qi, :n]
        for p, (a, b) in enumerate(zip(got, ans)):
            if a != b:
                assert b in got and abs(sc[p] - sc[got.index(b)]) < TOL, (qi, p, a, b)


def _max_rows_restatement(q, g, k=100, thresholds=(0.9069641, 0.985643)):
    """generate_tsv.py:91-125 with the max strategy, on ragged arrays (as oracle.match_ref.calc_scores_reference states the mean form)"""
    import torch.nn.functional as F
    qh, qhs, qb, qbs, qt = q
    gh, ghs, gb, gbs, gt = g

    def sim(a, b):                                   # (cos + 1) / 2 of every photo pair of the two modalities, [Pq, Pg]
        a, b = torch.from_numpy(a), torch.from_numpy(b)
        return (F.cosine_similarity(a[:, None, :], b[None, :, :], dim=2) + 1) / 2
    sh, sb = sim(qh, gh), sim(qb, gb)
    rows = []
    for i in range(len(qt)):
        cand = []
        for j in range(len(gt)):
            if int(gt[j]) != int(qt[i]):
                continue
            bh, bb = sh[qhs[i]:qhs[i + 1], ghs[j]:ghs[j + 1]], sb[qbs[i]:qbs[i + 1], gbs[j]:gbs[j + 1]]
            s0 = bh.max().item() if bh.numel() else 0
            s1 = bb.max().item() if bb.numel() else 0
            if s0 + s1 == 0:
                continue
            cand.append((j, s1 if qhs[i + 1] == qhs[i] or (s0 == 0 and s1 > thresholds[int(qt[i]) - 1]) else s0))
        cand.sort(key=lambda x: x[1], reverse=True)
        if cand:
            sc = [c[1] for c in cand]
            rows.append((i, sc[0], float(np.mean(sc[:3])), float(np.mean(sc[:10])), [c[0] for c in cand[:k]]))
    return rows


def test_calc_scores_max_equals_reference_rows():
    from pathlib import Path
    from pets_face_recognition_amd.match import calc_scores, calc_scores_db, create_table
    from oracle.match_ref import calc_scores_case
    z = np.load(os.path.join(GOLD, "max_strategy.npz"))
    q = [z[f"q_{n}"] for n in ("head", "head_seg", "body", "body_seg", "type")]
    g = [z[f"g_{n}"] for n in ("head", "head_seg", "body", "body_seg", "type")]
    dev = lambda t: [torch.from_numpy(t[0]).to(DEV), t[1], torch.from_numpy(t[2]).to(DEV), t[3], t[4]]
    rows = [(int(qi), t1, a, b, ans[ans >= 0].tolist())
            for qi, t1, a, b, ans in zip(z["rows_query"], z["top1"], z["mean3"], z["mean10"], z["answer"])]
    for chunk in (32768, 64):
        r = calc_scores(*dev(q), *dev(g), k=100, chunk=chunk, strategy="max")
        _check_calc_scores(r["idx"].cpu().numpy(), r["scores"].cpu().numpy(), r["count"].cpu().numpy(), r["top1"].cpu().numpy(),
                           r["mean3"].cpu().numpy(), r["mean10"].cpu().numpy(), rows)

    def db(prefix, t):
        h, hs, b, bs, ty = t
        return {Path(f"/cards/{prefix}{c:04d}"): {"head_vectors": [torch.from_numpy(v) for v in h[hs[c]:hs[c + 1]]],
                                                  "body_vectors": [torch.from_numpy(v) for v in b[bs[c]:bs[c + 1]]],
                                                  "type": int(ty[c])} for c in range(len(ty))}
    out = calc_scores_db(db("q", q), db("g", g), device=DEV, strategy="max")
    assert [o[0] for o in out] == [f"q{int(i):04d}" for i in z["rows_query"]]
    for o, t1, ans in zip(out, z["top1"], z["answer"]):
        assert abs(o[1] - t1) < TOL
        names = o[4].split(",")
        assert len(names) == int((ans >= 0).sum()) and names[0] == f"g{int(ans[0]):04d}"
    df = create_table({Path("/cards"): (db("q", q), db("g", g))}, device=DEV, strategy="max")
    assert df["query"].tolist() == [o[0] for o in out] and df["answer"].iloc[0] == out[0][4]
    # the max rows are not the mean rows: the strategy argument reaches the kernel
    mean = calc_scores(*dev(q), *dev(g), k=100)
    assert float((mean["top1"].cpu() - r["top1"].cpu()).abs().max()) > 1e-3

    # a second ragged case (other seed, D = 64, several gallery chunks) against the restatement above
    qq, gg = calc_scores_case(seed=5, Q=16, G=700, D=64, n_id=90)
    rows = _max_rows_restatement(qq, gg)
    r = calc_scores(*dev(list(qq)), *dev(list(gg)), k=100, chunk=256, strategy="max")
    _check_calc_scores(r["idx"].cpu().numpy(), r["scores"].cpu().numpy(), r["count"].cpu().numpy(), r["top1"].cpu().numpy(),
                       r["mean3"].cpu().numpy(), r["mean10"].cpu().numpy(), rows)
