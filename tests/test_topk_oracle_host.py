"""CPU tests of tests/topk_oracle.py: the key is strictly monotone and invertible to the bit, the exact best-K equals a stable descending
argsort under heavy ties, chunk by chunk equals the whole row, filter + merge equals the best-K, the state layout round-trips, and the
real-valued re-scoring case pins the order (its gaps are far outside the rounding bound)."""
import numpy as np
import pytest
import torch

import topk_oracle as O


def _sorted_sample():
    f = np.float32
    tiny, den = np.finfo(f).tiny, f(2.0 ** -149)
    big = np.finfo(f).max
    pos = [f(0.0), den, f(2 * den), np.nextafter(tiny, f(0)), tiny, np.nextafter(tiny, f(1)), f(1e-20), np.nextafter(f(1), f(0)), f(1.0),
           np.nextafter(f(1), f(2)), f(3.5), np.nextafter(big, f(0)), big, f(np.inf)]
    neg = [-x for x in reversed(pos)]      # -inf ... -0.0
    return np.array(neg + pos, dtype=f)


def test_fkey_is_strictly_monotone_over_the_float_line():
    x = _sorted_sample()
    assert np.signbit(x[13]) and x[13] == 0 and not np.signbit(x[14]) and x[14] == 0     # -0.0 directly below +0.0
    assert np.all(np.diff(x.astype(np.float64)) >= 0)
    k = O.fkey(x)
    assert k.dtype == np.uint32
    assert np.all(k[1:] > k[:-1]), "keys must increase strictly along the sorted sample (-0.0 < +0.0 included)"
    assert k[0] > 0, "key 0 is reserved: it means 'list not full' in thrk and marks an empty slot"
    # adjacent floats map to adjacent keys on both sides of zero
    for a in (np.float32(1.0), np.float32(-1.0), np.float32(2.0 ** -149), np.float32(-2.0 ** -149)):
        b = np.nextafter(a, np.float32(np.inf))
        ka, kb = (int(v) for v in O.fkey(np.array([a, b])))
        assert kb - ka == 1


def test_fkey_inverse_is_bit_identical():
    rs = np.random.RandomState(1)
    bits = np.concatenate([rs.randint(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32), _sorted_sample().view(np.uint32)])
    x = bits.view(np.float32)
    back = O.fkey_inv(O.fkey(x))
    assert np.array_equal(back.view(np.uint32), bits)
    k = rs.randint(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(O.fkey(O.fkey_inv(k)), k)


def test_pack_orders_by_key_then_lower_index():
    key = np.array([5, 5, 7, 5], np.uint32)
    idx = np.array([9, 2, 4000000000, 0], np.int64)
    e = O.pack(key, idx)
    k2, i2 = O.unpack(e)
    assert np.array_equal(k2, key) and np.array_equal(i2, idx)
    assert [int(i) for i in O.unpack(np.sort(e)[::-1])[1]] == [4000000000, 0, 2, 9]


def _tie_scores(rs, rows, n, values=7):
    return rs.randint(-values // 2, values // 2 + 1, (rows, n)).astype(np.float32) * 0.5


@pytest.mark.parametrize("K", [1, 10, 257])
def test_topk_exact_equals_stable_descending_argsort(K):
    rs = np.random.RandomState(K)
    s = _tie_scores(rs, 5, 3000)
    s[0, :] = 0.25                        # one value only
    s[1, ::3] = -0.0                      # -0.0 ranks below +0.0: argsort sees them equal, so keep this row out of the index check
    ent, thr = O.topk_exact(s, 1000003, K)
    order = torch.argsort(torch.tensor(s), dim=1, descending=True, stable=True)[:, :K].numpy()
    for r in range(5):
        key, idx = O.unpack(ent[r])
        assert np.array_equal(O.fkey_inv(key), np.take(s[r], order[r]))
        if r != 1:
            assert np.array_equal(idx, order[r] + 1000003)
        assert thr[r] == O.fkey(np.take(s[r], order[r]))[-1]
    few, thr = O.topk_exact(s[:, :K - 1], 0, K) if K > 1 else (None, None)
    if few is not None:
        assert all(len(e) == K - 1 for e in few) and not thr.any(), "thrk is 0 while fewer than K entries exist"


def test_topk_exact_skips_self_index():
    s = np.array([[3.0, 9.0, 1.0, 9.0]], np.float32)
    ent, thr = O.topk_exact(s, 10, 2, self_idx=[11])
    assert [int(i) for i in O.unpack(ent[0])[1]] == [13, 10] and thr[0] == O.fkey(np.float32(3.0))
    ent, _ = O.topk_exact(s, 10, 2, self_idx=[-1])
    assert [int(i) for i in O.unpack(ent[0])[1]] == [11, 13]


@pytest.mark.parametrize("cuts", [(5, 3005), (1, 2, 3, 1540, 3076), (2999,), (1536, 3073)])
def test_topk_exact_chunk_by_chunk_equals_whole_row(cuts):
    rs = np.random.RandomState(len(cuts))
    n, K = 4099, 100
    s = _tie_scores(rs, 4, n, values=41)
    self_idx = np.array([-1, 0, n - 1, 1537])
    whole, thr_w = O.topk_exact(s, 0, K, self_idx=self_idx)
    seed, thr = None, None
    edges = [0, *cuts, n]
    for a, b in zip(edges[:-1], edges[1:]):
        seed, thr = O.topk_exact(s[:, a:b], a, K, self_idx=self_idx, seed=seed)
    for r in range(4):
        assert np.array_equal(seed[r], whole[r])
    assert np.array_equal(thr, thr_w)


def test_filter_set_then_merge_equals_topk_exact():
    rs = np.random.RandomState(3)
    K, n0, n1 = 20, 300, 700
    s = _tie_scores(rs, 6, n0 + n1, values=61)
    seed, thr = O.topk_exact(s[:, :n0], 0, K)
    cand = O.filter_set(s[:, n0:], thr, n0, exclude_self=False)
    want, thr_w = O.topk_exact(s, 0, K)
    for r in range(6):
        key, _ = O.unpack(cand[r])
        assert np.all(key > thr[r]) and len(np.unique(cand[r])) == len(cand[r])
        assert len(cand[r]) == int((O.fkey(s[r, n0:]) > thr[r]).sum())
        got, t = O.best_entries([seed[r], cand[r]], K)
        assert np.array_equal(got, want[r]) and t == thr_w[r]
    # exclude_self drops exactly the diagonal entry
    a = O.filter_set(s[:, n0:], np.zeros(6, np.uint32), 2, exclude_self=False)
    b = O.filter_set(s[:, n0:], np.zeros(6, np.uint32), 2, exclude_self=True)
    for r in range(6):
        gone = set(a[r].tolist()) - set(b[r].tolist())
        assert (len(gone) == 1 and int(O.unpack(np.array(list(gone), np.uint64))[1][0]) == r) if r >= 2 else not gone


def test_state_layout_round_trip_and_size_check():
    rows, K = 7, 100
    total = rows * K * 8 + rows * 4 + 64 + rows * 8
    L = O.StateLayout(rows, K, total)
    rs = np.random.RandomState(4)
    cur = rs.randint(0, 2 ** 62, (rows, K)).astype(np.uint64)
    st = L.read(L.write(cur=cur, cur_n=np.arange(rows), flags=3, thrk=np.arange(rows) + 5, ccnt=np.arange(rows) * 2))
    assert np.array_equal(st["cur"], cur) and st["flags"] == 3 and not st["flag_pad"].any()
    assert st["cur_n"].tolist() == list(range(rows)) and st["thrk"].tolist() == [r + 5 for r in range(rows)]
    assert st["ccnt"].tolist() == [2 * r for r in range(rows)]
    with pytest.raises(AssertionError, match="layout changed"):
        O.StateLayout(rows, K, total + 4)


def test_rescore_exact_certificate_by_hand():
    q = np.array([[1, 2, 0, 0]], np.float32)
    g = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 1, 0, 0], [0, 0, 1, 0]], np.float32)   # dots 1, 2, 3, 0
    cand = np.array([[3, -1, 1, 0]])
    cs = np.array([[0.5, 99.0, 2.25, 1.0]], np.float32)
    sc, ix, cert, _ = O.rescore_exact(q, g, None, cand, cs, 2)
    assert sc.tolist() == [[2.0, 1.0]] and ix.tolist() == [[1, 0]]
    assert cert.tolist() == [[0.5, 0.0]]          # max(|0 - .5|, |2 - 2.25|, |1 - 1|); 1.0 - 1.0
    sc, ix, cert, _ = O.rescore_exact(q, g, np.array([1, 1, 1, 1.0]), np.array([[3, 1, 0, -1]]), cs, 2)
    assert np.isposinf(cert[0, 1])                # last candidate missing
    sc, ix, cert, _ = O.rescore_exact(q, g, None, np.array([[-1, -1, -1, 2]]), cs, 2)
    assert sc[0, 0] == 3.0 and np.isneginf(sc[0, 1]) and ix.tolist() == [[2, -1]] and np.isposinf(cert[0, 1])   # fewer than K valid


@pytest.mark.parametrize("with_scale", [False, True])
def test_real_valued_rescore_case_pins_the_order(with_scale):
    """The GPU test accepts a swap only inside the rounding bound.  That must not make it vacuous: on the fixed seed every rank boundary
    has the pair next to it far outside the bound (so the order across every boundary is decided), and the check itself rejects a swap of
    two such neighbours and a skipped entry."""
    q, g, scale, cand = O.rescore_real_case(with_scale)
    _, ix, _, dots = O.rescore_exact(q, g, scale, cand, None, cand.shape[1])
    for r in range(q.shape[0]):
        b = O.rescore_bound(q[r], g[cand[r]], None if scale is None else scale[cand[r]])
        assert b.max() < 2e-6, "the bound is a small multiple of 2^-24 * sum |x y| (sum |x y| <= 1 for unit rows)"
        order = np.argsort(-dots[r], kind="stable")
        d, bb = dots[r][order], b[order]
        far1 = (d[:-1] - d[1:]) > 8 * (bb[:-1] + bb[1:])          # ranks i, i + 1
        far2 = (d[:-2] - d[2:]) > 8 * (bb[:-2] + bb[2:])          # ranks i, i + 2
        # boundary i | i + 1 is straddled by the pairs (i, i + 1), (i - 1, i + 1) and (i, i + 2)
        n = len(d)
        for i in range(n - 1):
            assert far1[i] or (i >= 1 and far2[i - 1]) or (i + 2 < n and far2[i]), f"rank boundary {i}: every pair next to it is within reach of rounding"
        assert far1.mean() > 0.97, "almost every neighbouring pair must be decided"
        ranked = cand[r][order]
        O.check_order_within_bound(ranked, cand[r], dots[r], b)
        O.check_order_within_bound(ranked[:10], cand[r], dots[r], b)
        swapped = ranked.copy()
        at = 40 + int(np.argmax(far1[40:]))
        swapped[[at, at + 1]] = swapped[[at + 1, at]]
        with pytest.raises(AssertionError, match="outside the rounding bound"):
            O.check_order_within_bound(swapped, cand[r], dots[r], b)
        with pytest.raises(AssertionError, match="skipped"):
            O.check_order_within_bound(np.delete(ranked, 3)[:10], cand[r], dots[r], b)
