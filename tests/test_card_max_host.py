"""Host side of the max-strategy card matching (no GPU): pfr_card_tiles against a Python restatement of its packing rule, the CPU paths of
match.card_max_scores / card_match(strategy='max') against a literal double loop of the reference's formula and against the pair scores the
reference's own max_strategy_cal_scores wrote into tests/golden/max_strategy.npz, the refusals and the untouched 'mean' default."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TOL = 2e-6          # the absolute tolerance of tests/test_match_gpu.py::_check_calc_scores


def _tiles_py(seg, cap=128):
    """the packing rule of pfr_card_tiles: whole cards in order, a non-empty card that does not fit opens a tile, empty cards go with the
    next non-empty card, trailing ones with the last tile"""
    n, tiles, first, end, rows = len(seg) - 1, [], 0, 0, 0
    for c in range(n):
        k = seg[c + 1] - seg[c]
        if k and rows + k > cap:
            tiles.append([first, end - first, seg[first], rows])
            first, rows = end, 0
        if k:
            rows, end = rows + k, c + 1
    return tiles + [[first, n - first, seg[first], rows]] if n else []


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64).tolist()


TILE_CASES = {
    "single_photo": [1] * 300,
    "exactly_128": [128],
    "128_between_singles": [1, 1, 128, 1, 1],
    "100_plus_29": [100, 29],
    "empty_first": [0, 0, 3, 4],
    "empty_last": [3, 4, 0, 0],
    "empty_consecutive": [2, 0, 0, 0, 5, 0, 126, 0, 0, 1],
    "empty_after_full_tile": [128, 0, 1],
    "only_empties": [0, 0, 0, 0],
    "one_card": [5],
    "one_empty_card": [0],
    "ragged": [int(v) for v in np.random.RandomState(3).randint(0, 40, 200)],
}


@pytest.mark.parametrize("name", sorted(TILE_CASES))
def test_card_tiles_equals_restatement_and_invariants(name):
    from pets_face_recognition_amd.match import card_tiles
    from pets_face_recognition_amd._hip import lib
    counts = TILE_CASES[name]
    seg = _offsets(counts)
    got = card_tiles(seg).tolist()
    assert got == _tiles_py(seg), name
    # the two-pass form of the C call: a size query writes nothing and returns the count
    s = torch.tensor(seg)
    assert lib.pfr_card_tiles(s.data_ptr(), len(counts), 0, 0) == len(got)
    # invariants: every card in exactly one tile, <= 128 rows per tile, contiguous rows
    card, row = 0, seg[0]
    for c0, nc, r0, nr in got:
        assert c0 == card and nc >= 1 and r0 == row and 0 <= nr <= 128
        assert nr == seg[c0 + nc] - seg[c0]
        card, row = c0 + nc, r0 + nr
    assert card == len(counts) and row == seg[-1]
    # empty cards never close a tile: a tile starts with its empties and, unless it is the last, ends with a non-empty card
    for c0, nc, r0, nr in got[:-1]:
        assert counts[c0 + nc - 1] > 0


def test_card_tiles_refusals():
    from pets_face_recognition_amd.match import card_tiles
    from pets_face_recognition_amd._hip import lib, PfrError
    with pytest.raises(PfrError, match="card 1 has 129 photos"):
        card_tiles(_offsets([3, 129]))
    s = torch.tensor(_offsets([3, 129]))
    assert lib.pfr_card_tiles(s.data_ptr(), 2, 0, 0) == -3          # PFR_ERR_UNSUPPORTED
    s = torch.tensor([0, 5, 3, 9])
    assert lib.pfr_card_tiles(s.data_ptr(), 3, 0, 0) == -1          # PFR_ERR_ARG: decreasing offsets
    with pytest.raises(PfrError, match="decrease"):
        card_tiles([0, 5, 3, 9])
    # a fill with too little room is an argument error
    s = torch.tensor(_offsets([100, 100, 100]))
    buf = torch.zeros((1, 4), dtype=torch.int32)
    assert lib.pfr_card_tiles(s.data_ptr(), 3, buf.data_ptr(), 1) == -1
    assert lib.pfr_card_tiles(s.data_ptr(), 0, 0, 0) == 0


# ---- CPU paths ---------------------------------------------------------------------------------------------------------------------
def _double_loop(qe, qseg, ge, gseg, dtype=torch.float32):
    """max over the photo pairs of (F.cosine_similarity + 1) / 2, card pair by card pair; NaN where a card has no photos"""
    qe, ge = qe.to(dtype), ge.to(dtype)
    out = torch.full((len(qseg) - 1, len(gseg) - 1), float("nan"), dtype=dtype)
    for i in range(len(qseg) - 1):
        a = qe[qseg[i]:qseg[i + 1]]
        for j in range(len(gseg) - 1):
            b = ge[gseg[j]:gseg[j + 1]]
            if len(a) and len(b):
                out[i, j] = ((F.cosine_similarity(a.repeat_interleave(len(b), 0), b.repeat(len(a), 1)) + 1) / 2).max()
    return out


_CACHE = {}


def _golden():
    """(npz, head inputs as tensors, fp32 double loop, fp64 double loop) — computed once for the module"""
    if not _CACHE:
        z = np.load(os.path.join(GOLD, "max_strategy.npz"))
        qe, ge = torch.from_numpy(z["q_head"]), torch.from_numpy(z["g_head"])
        qseg, gseg = z["q_head_seg"].tolist(), z["g_head_seg"].tolist()
        _CACHE["v"] = (z, qe, qseg, ge, gseg, _double_loop(qe, qseg, ge, gseg), _double_loop(qe, qseg, ge, gseg, torch.float64))
    return _CACHE["v"]


def test_reference_yardstick_is_within_half_the_tolerance_of_fp64():
    """the tolerance is about the path under test, not about the fp32 yardstick: the fp32 double loop and the reference's own recorded
    scores are within TOL / 2 of an fp64 evaluation"""
    z, _, _, _, _, ref32, ref64 = _golden()
    has = ~torch.isnan(ref64)
    assert bool((torch.isnan(ref32) == torch.isnan(ref64)).all()) and int(has.sum()) > 3000
    assert float((ref32.double() - ref64)[has].abs().max()) < TOL / 2
    gold = torch.from_numpy(z["pair_scores"])
    assert bool((torch.isnan(gold) == torch.isnan(ref64)).all())
    assert float((gold - ref64)[has].abs().max()) < TOL / 2


def test_cpu_card_max_scores_equals_double_loop_and_golden():
    from pets_face_recognition_amd.match import card_max_scores
    z, qe, qseg, ge, gseg, ref32, _ = _golden()
    dots = card_max_scores(qe, qseg, ge, gseg)
    assert dots.shape == ref32.shape and dots.dtype == torch.float32
    has = ~torch.isnan(ref32)
    assert bool((torch.isinf(dots) & (dots < 0) == ~has).all())          # -inf exactly where a card has no photos
    got = (dots + 1) / 2
    assert float((got - ref32)[has].abs().max()) < TOL
    assert float((got.double() - torch.from_numpy(z["pair_scores"]))[has].abs().max()) < TOL


def _check_order(idx, sc, ref):
    """near-tie rule of tests/test_match_gpu.py::_check_calc_scores: the returned order equals the reference order (score descending, ties to
    the lower index) except that two cards may be swapped when their reference scores are closer than TOL; every query is checked"""
    for qi in range(ref.shape[0]):
        r = ref[qi]
        cands = [j for j in range(len(r)) if not np.isnan(r[j])]
        want = sorted(cands, key=lambda j: (-r[j], j))[:idx.shape[1]]
        n = len(want)
        got = idx[qi, :n].tolist()
        assert (idx[qi, n:] == -1).all() and np.isinf(sc[qi, n:]).all()
        assert n == idx.shape[1] or sorted(got) == sorted(want)
        for p, (a, b) in enumerate(zip(got, want)):
            assert abs(sc[qi, p] - r[a]) < TOL, (qi, p)
            if a != b:
                assert abs(r[a] - r[b]) < TOL, (qi, p, a, b)


@pytest.mark.parametrize("k", [10, 100])
def test_cpu_card_match_max_order_and_scores(k):
    from pets_face_recognition_amd.match import card_match
    z, qe, qseg, ge, gseg, ref32, _ = _golden()
    sc, idx = card_match(qe, qseg, ge, gseg, k=k, strategy="max")
    assert sc.shape == idx.shape == (ref32.shape[0], k) and idx.dtype == torch.int32
    _check_order(idx.numpy(), sc.numpy(), ref32.numpy())
    _check_order(idx.numpy(), sc.numpy(), z["pair_scores"])          # the scores the reference's own max_strategy_cal_scores recorded


def test_cpu_card_match_max_pads_to_k():
    """k above the number of gallery cards: [Q, k] with −inf / −1 past the candidates, as the device path returns"""
    from pets_face_recognition_amd.match import card_match
    g = torch.Generator().manual_seed(2)
    qe, ge = torch.randn(5, 8, generator=g), torch.randn(6, 8, generator=g)
    sc, idx = card_match(qe, [0, 2, 2, 5], ge, [0, 1, 1, 4, 6], k=7, strategy="max")
    assert sc.shape == idx.shape == (3, 7) and idx.dtype == torch.int32
    assert sorted(idx[0, :3].tolist()) == [0, 2, 3] and (idx[0, 3:] == -1).all() and torch.isinf(sc[0, 3:]).all()
    assert (idx[1] == -1).all() and torch.isinf(sc[1]).all() and torch.isfinite(sc[0, :3]).all()


def test_cpu_chunked_path_agrees_across_chunk_sizes():
    """(the fp32 matmul of another block shape may round differently: same −inf pattern, values within the tolerance)"""
    from pets_face_recognition_amd import match
    _, qe, qseg, ge, gseg, _, _ = _golden()
    qs, gs = torch.tensor(qseg), torch.tensor(gseg)
    a = match._card_max_scores_torch(qe, qs, ge, gs, chunk=2048)
    b = match._card_max_scores_torch(qe, qs, ge, gs, chunk=7)
    fin = torch.isfinite(a)
    assert torch.equal(fin, torch.isfinite(b)) and torch.equal(a[~fin], b[~fin]) and float((a - b)[fin].abs().max()) < TOL


def test_refusals_and_defaults():
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import PfrError
    g = torch.Generator().manual_seed(1)
    qe, ge = torch.randn(9, 16, generator=g), torch.randn(140, 16, generator=g)
    qseg, gseg = [0, 2, 5, 9], [0, 3, 3, 8, 11]
    for fn, args in ((match.card_match, (qe, qseg, ge, gseg)), (match.calc_scores_db, ({}, {})), (match.create_table, ({},)),
                     (match.calc_scores, (qe, qseg, qe, qseg, [1, 1, 1], ge, gseg, ge, gseg, [1, 1, 1, 1]))):
        with pytest.raises(PfrError, match="unknown strategy"):
            fn(*args, strategy="median")
    with pytest.raises(PfrError, match="card 1 has 129 photos"):
        match.card_max_scores(qe, qseg, ge, [0, 3, 132, 140])
    with pytest.raises(PfrError, match="card 1 has 129 photos"):
        match.card_match(qe, qseg, ge, [0, 3, 132, 140], k=2, strategy="max")
    # 'mean' is the default and is untouched: the same bits with and without the argument
    a = match.card_match(qe, qseg, ge, gseg, k=3)
    b = match.card_match(qe, qseg, ge, gseg, k=3, strategy="mean")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_c_abi_declares_the_three_symbols():
    from pets_face_recognition_amd._hip.lib import parse_header
    protos = parse_header()
    assert protos["pfr_card_tiles"][0] is ctypes.c_long and protos["pfr_card_tiles"][2] == ["seg", "ncards", "tiles", "cap"]
    assert protos["pfr_card_max_scores"][2][-1] == "stream" and protos["pfr_card_max_rescore"][2][-1] == "stream"
