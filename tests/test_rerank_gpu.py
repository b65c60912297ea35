"""k-reciprocal re-ranking on the device: pfr_rerank_expand / _average / _score through the C-ABI and through match.rerank, against the dense
fp64 restatement of the contract in tests/rerank_oracle.py, which consumes the same fp32 rows and the same nbr / cand lists.

The bound (u = 2^-24, the unit roundoff of fp32; every row is a unit vector, every V <= 1, every row of V and V' sums to 1):
  dot product of D terms, any summation order:          |err| <= D u Σ|a_i b_i| <= D u
  argument of exp, -(2 - 2 dot):                         |err| <= 2 D u + 2 u;  w = exp(.) has relative error <= 2 D u + 4 u (expf: 1 ulp = 2 u)
  Σ w over n <= E terms: relative <= that + E u;  V = w / Σ w: relative <= 4 D u + E u + 10 u  <= (4 D + 2 E + 16) u, absolute too (V <= 1)
  hence a V row sums to 1 within the rounding of its OWN sum and divisions: <= E u (n - 1 <= E - 2 additions, one division each)
  V' = (1 / k2') Σ of k2' rows: relative error of every term as above, plus (k2' + 1) u for the sum and the division
  m = Σ_j min(V'[i][j], V'[c][j]): |min(a', b') - min(a, b)| <= max(|a' - a|, |b' - b|), the sum of <= E2 terms adds E2 u relative, m <= 1:
      |m_dev - m| <= (4 D + 2 E + 16 + k2 + 1 + E2) u <= tol_m = (4 D + 2 E + 2 E2 + 16) u
  dJ = 1 - m / (2 - m) has slope 2 / (2 - m)^2 <= 2 on [0, 1];  2 - 2 cos is exact up to one rounding, the blend a few u more:
      |dist_dev - final| <= 2 (1 - lambda) tol_m + 2 lambda D u
The bound is derived, not measured: a device value outside it is a bug in the kernels."""
import ctypes

import numpy as np
import pytest
import torch

from rerank_oracle import U, capacity, dist_bound, lists_from_rows, make_set, oracle, tol_m

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cabi(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam):
    """the three entry points on device copies of the inputs -> dict of CPU tensors"""
    from pets_face_recognition_amd._hip import lib
    from pets_face_recognition_amd.match import rerank_row_capacity
    N, D = emb32.shape
    R, kc = cand.shape
    E, E2 = rerank_row_capacity(k1, k2)
    assert (E, E2) == capacity(k1, k2)
    d = lambda t, dt: t.to(device=DEV, dtype=dt).contiguous()
    e, nb, rw, cd, cc = d(emb32, torch.float32), d(nbr, torch.int32), d(rows, torch.int32), d(cand, torch.int32), d(cand_cos, torch.float32)
    new = lambda shape, dt, fill: torch.full(shape, fill, dtype=dt, device=DEV)        # (filled: an unwritten slot shows)
    v_idx, v_val, v_cnt = new((N, E), torch.int32, -7), new((N, E), torch.float32, 9.0), new((N,), torch.int32, -7)
    q_idx, q_val, q_cnt = new((N, E2), torch.int32, -7), new((N, E2), torch.float32, 9.0), new((N,), torch.int32, -7)
    dist, idx = new((R, k), torch.float32, 9.0), new((R, k), torch.int32, -7)
    s = torch.cuda.current_stream().cuda_stream
    lib.pfr_rerank_expand(e.data_ptr(), N, D, nb.data_ptr(), k1, v_idx.data_ptr(), v_val.data_ptr(), v_cnt.data_ptr(), E, s)
    lib.pfr_rerank_average(nb.data_ptr(), N, k1, k2, v_idx.data_ptr(), v_val.data_ptr(), v_cnt.data_ptr(), E, q_idx.data_ptr(), q_val.data_ptr(),
                           q_cnt.data_ptr(), E2, s)
    lib.pfr_rerank_score(q_idx.data_ptr(), q_val.data_ptr(), q_cnt.data_ptr(), N, E2, rw.data_ptr(), R, cd.data_ptr(), cc.data_ptr(), kc,
                         float(lam), k, dist.data_ptr(), idx.data_ptr(), s)
    torch.cuda.synchronize()
    out = dict(v_idx=v_idx, v_val=v_val, v_cnt=v_cnt, q_idx=q_idx, q_val=q_val, q_cnt=q_cnt, dist=dist, idx=idx)
    return {k_: v.cpu() for k_, v in out.items()}


def check_rows(idx, val, cnt, want_sets, want_dense, tol, cap):
    """sparse rows (ascending, padded, counted) against the oracle's sets (EXACT) and dense values (within tol)"""
    idx, val, cnt = idx.numpy(), val.double().numpy(), cnt.numpy()
    for i in range(len(cnt)):
        n = int(cnt[i])
        assert 0 <= n <= cap
        ids = idx[i, :n]
        assert (np.diff(ids) > 0).all(), (i, ids)                       # ascending, duplicate free
        if want_sets is not None:
            assert set(ids.tolist()) == want_sets[i], (i, sorted(ids.tolist()), sorted(want_sets[i]))
        else:
            assert set(ids.tolist()) == set(np.nonzero(want_dense[i])[0].tolist()), i
        assert (idx[i, n:] == -1).all() and (val[i, n:] == 0).all()
        if n:
            assert np.abs(val[i, :n] - want_dense[i, ids]).max() <= tol, (i, np.abs(val[i, :n] - want_dense[i, ids]).max(), tol)


def check_case(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam):
    """C-ABI and match.rerank_lists on the same lists: sets exact, weights / scores within the derived bound, order, padding, determinism"""
    from pets_face_recognition_amd.match import rerank_lists
    N, D = emb32.shape
    R, kc = cand.shape
    E, E2 = capacity(k1, k2)
    O = oracle(emb32, nbr, rows, cand, cand_cos, k1, k2, lam)
    got = cabi(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam)
    tv = (4 * D + 2 * E + 16) * U
    check_rows(got["v_idx"], got["v_val"], got["v_cnt"], O["sets"], O["V"], tv, E)
    for i in range(N):                                                   # every V row sums to 1 within E u
        assert abs(got["v_val"][i].double().sum().item() - 1.0) <= E * U, (i, got["v_val"][i].double().sum().item() - 1.0)
    check_rows(got["q_idx"], got["q_val"], got["q_cnt"], None, O["Vq"], tv + (k2 + 1) * U, E2)
    bound = dist_bound(D, k1, k2, lam)
    fin, cn, rw = O["final"], cand.numpy(), rows.numpy()
    dist, idx = got["dist"].double().numpy(), got["idx"].numpy()
    worst = 0.0
    for r in range(R):
        nv = int(np.isfinite(fin[r]).sum())
        kk = min(k, nv)
        assert (idx[r, kk:] == -1).all() and np.isposinf(dist[r, kk:]).all(), r
        assert len(set(idx[r, :kk].tolist())) == kk and rw[r] not in idx[r, :kk] and (idx[r, :kk] >= 0).all(), r
        assert (np.diff(dist[r, :kk]) >= 0).all(), r
        if kk:
            pos = [cn[r].tolist().index(j) for j in idx[r, :kk]]
            e1 = np.abs(dist[r, :kk] - fin[r, pos]).max()
            e2 = np.abs(dist[r, :kk] - np.sort(fin[r])[:kk]).max()     # the t-th device distance against the oracle's t-th smallest, every t
            worst = max(worst, e1, e2)
            assert e1 <= bound and e2 <= bound, (r, e1, e2, bound)
            assert dist[r, kk - 1] <= np.sort(fin[r])[kk - 1] + bound
    print(f"N={N} D={D} k1={k1} k2={k2} lambda={lam} kc={kc} k={k}: worst |dist - oracle| = {worst:.3e}, bound {bound:.3e}")
    # determinism, and the Python path on the same lists: the same bits
    again = cabi(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam)
    for name in got:
        assert torch.equal(got[name], again[name]), name
    d2, i2 = rerank_lists(emb32.to(DEV), nbr.to(DEV), rows.to(DEV), cand.to(DEV), cand_cos.to(DEV), k, k1, k2, lam)
    assert torch.equal(d2.cpu(), got["dist"]) and torch.equal(i2.cpu(), got["idx"])
    return O, got


def std_lists(emb32, k1, kc, rows=None):
    nbr, rows, cand, cand_cos = lists_from_rows(emb32, k1, max(kc, 1), rows)
    return nbr, rows, cand, cand_cos


# ---- 1. sets are exact (and everything else holds) over the sizes and k1 that change the path
@pytest.mark.parametrize("k1", [1, 5, 8, 10])            # E = 4, 24, 54, 77 (crosses the 64-lane boundary)
def test_sizes_and_layouts(k1):
    k2, lam, D = 3, 0.3, 64
    for N in sorted({1, 2, k1, k1 + 1, 65, 300}):
        emb32 = make_set("random", N, D, seed=10 * k1 + N)
        kc = max(1, min(20, N - 1))
        check_case(emb32, *std_lists(emb32, k1, kc), k=min(10, kc), k1=k1, k2=k2, lam=lam)
    # one tight cluster of k1 + 1 items: every expansion is accepted, everything is a duplicate
    emb32 = make_set("tight", k1 + 1, D, seed=k1)
    O, got = check_case(emb32, *std_lists(emb32, k1, k1), k=k1, k1=k1, k2=k2, lam=lam)
    assert all(s == set(range(k1 + 1)) for s in O["sets"]) and (got["v_cnt"] == k1 + 1).all()
    # classes of unequal size
    emb32 = make_set("clustered", 300, D, seed=k1 + 1, k1=k1)
    O, got = check_case(emb32, *std_lists(emb32, k1, 40), k=10, k1=k1, k2=k2, lam=lam)
    assert len({len(s) for s in O["sets"]}) > 1


@pytest.mark.parametrize("k1", [5, 10])
def test_padding_inside_the_neighbour_table(k1):
    """N - 1 < k1 pads the rows; entries outside [0, N) — -1, N, a huge value, INT_MIN — in the MIDDLE of a row are skipped, never dereferenced"""
    D, N = 64, k1 - 1
    emb32 = make_set("random", N, D, seed=3)
    nbr, rows, cand, cand_cos = std_lists(emb32, k1, N - 1)
    assert (nbr[:, N:] == -1).all()
    check_case(emb32, nbr, rows, cand, cand_cos, k=N - 1, k1=k1, k2=2, lam=0.3)
    emb32 = make_set("clustered", 65, D, seed=4, k1=k1)
    nbr, rows, cand, cand_cos = std_lists(emb32, k1, 30)
    nbr = nbr.clone()
    for i, bad in zip(range(0, 65, 3), [-1, 65, 2 ** 30, -2 ** 31, 1 << 20] * 5):
        nbr[i, 1 + i % k1] = bad
        nbr[(i + 1) % 65, 2] = bad
    cand = cand.clone(); cand_cos = cand_cos.clone()
    cand[5, 3], cand[6, 0], cand[7, 29] = 65, -5, 2 ** 30              # padding inside a candidate list is skipped as well
    check_case(emb32, nbr, rows, cand, cand_cos, k=30, k1=k1, k2=3, lam=0.3)


# ---- 2. the bound over D, at the default (k1, k2) too
@pytest.mark.parametrize("D", [64, 200, 512])
@pytest.mark.parametrize("k1,k2", [(8, 3), (20, 6)])
def test_bound_over_embedding_widths(D, k1, k2):
    emb32 = make_set("clustered", 300, D, seed=D + k1, k1=k1)
    check_case(emb32, *std_lists(emb32, k1, 100), k=10, k1=k1, k2=k2, lam=0.3)


# ---- 3. corners
@pytest.fixture(scope="module")
def clustered300():
    emb32 = make_set("clustered", 300, 64, seed=77, k1=8)
    return emb32, std_lists(emb32, 8, 100)


def test_lambda_one_reproduces_the_input_order_bit_for_bit(clustered300):
    emb32, (nbr, rows, cand, cand_cos) = clustered300
    k = 25
    _, got = check_case(emb32, nbr, rows, cand, cand_cos, k=k, k1=8, k2=3, lam=1.0)
    assert torch.equal(got["idx"], cand[:, :k])
    assert torch.equal(got["dist"], 2 - 2 * cand_cos[:, :k])


def test_lambda_zero(clustered300):
    emb32, (nbr, rows, cand, cand_cos) = clustered300
    check_case(emb32, nbr, rows, cand, cand_cos, k=10, k1=8, k2=3, lam=0.0)


def test_k2_one_is_the_identity(clustered300):
    emb32, (nbr, rows, cand, cand_cos) = clustered300
    _, got = check_case(emb32, nbr, rows, cand, cand_cos, k=10, k1=8, k2=1, lam=0.3)
    assert torch.equal(got["q_idx"], got["v_idx"]) and torch.equal(got["q_val"], got["v_val"]) and torch.equal(got["q_cnt"], got["v_cnt"])
    _, got3 = check_case(emb32, nbr, rows, cand, cand_cos, k=10, k1=8, k2=3, lam=0.3)
    assert not torch.equal(got3["q_cnt"], got["q_cnt"])


@pytest.mark.parametrize("case", ["kc=1", "kc=N-1", "kc>valid", "k=kc", "rows"])
def test_candidate_list_corners(case):
    N, D, k1 = 65, 64, 8
    emb32 = make_set("clustered", N, D, seed=9, k1=k1)
    if case == "kc=1":
        check_case(emb32, *std_lists(emb32, k1, 1), k=1, k1=k1, k2=3, lam=0.3)
    elif case == "kc=N-1":          # every other item is a candidate: the unrestricted re-ranking
        check_case(emb32, *std_lists(emb32, k1, N - 1), k=10, k1=k1, k2=3, lam=0.3)
    elif case == "kc>valid":        # -1 / -inf padded lists, +inf / -1 padded outputs
        nbr, rows, cand, cand_cos = std_lists(emb32, k1, N - 1)
        pad = 6
        cand = torch.cat([cand, torch.full((N, pad), -1, dtype=torch.int32)], 1)
        cand_cos = torch.cat([cand_cos, torch.full((N, pad), -float("inf"))], 1)
        _, got = check_case(emb32, nbr, rows, cand, cand_cos, k=N - 1 + pad, k1=k1, k2=3, lam=0.3)
        assert (got["idx"][:, N - 1:] == -1).all() and (got["idx"][:, :N - 1] >= 0).all()
    elif case == "k=kc":
        check_case(emb32, *std_lists(emb32, k1, 33), k=33, k1=k1, k2=3, lam=0.3)
    else:                           # R < N output rows in shuffled order
        rows = torch.randperm(N, generator=torch.Generator().manual_seed(1))[:23].int()
        O, got = check_case(emb32, *std_lists(emb32, k1, 20, rows), k=10, k1=k1, k2=3, lam=0.3)
        full = cabi(emb32, *std_lists(emb32, k1, 20), 10, k1, 3, 0.3)
        assert torch.equal(got["idx"], full["idx"][rows.long()]) and torch.equal(got["dist"], full["dist"][rows.long()])


# ---- 4. match.rerank: the lists of cosine_topk on the device, one set and query / gallery
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_match_rerank_one_set(dtype):
    from pets_face_recognition_amd.match import rerank, rerank_inputs, cosine_topk
    N, D, k, k1, k2, lam, kc = 300, 64, 10, 8, 3, 0.3, 50
    x = (make_set("clustered", N, D, seed=21, k1=k1) * 2.5).to(DEV)
    emb32, nbr, rows, cand, cand_cos, off = rerank_inputs(x, k, k1=k1, candidates=kc, compute_dtype=dtype)
    assert off == 0 and cand.shape == (N, kc) and nbr.shape == (N, k1 + 1)
    O, got = check_case(emb32.cpu(), nbr.cpu(), rows.cpu(), cand.cpu(), cand_cos.cpu(), k, k1, k2, lam)
    dist, idx = rerank(x, k, k1=k1, k2=k2, lambda_value=lam, candidates=kc, compute_dtype=dtype)
    assert torch.equal(dist.cpu(), got["dist"]) and torch.equal(idx.cpu(), got["idx"])
    # lists computed by the caller
    sc, ix = cosine_topk(emb32, emb32, kc, compute_dtype=dtype, exclude_self=True, normalize=False)
    d2, i2 = rerank(x, k, k1=k1, k2=k2, lambda_value=lam, candidates=kc, neighbors=(sc, ix))
    assert torch.equal(d2, dist) and torch.equal(i2, idx)
    # it does something: some row's top 10 differs from the cosine top 10
    assert int((idx != cand[:, :k]).any(dim=1).sum()) >= 1
    # k beyond the candidates: padded
    d3, i3 = rerank(x[:7], 10, k1=k1, k2=k2, lambda_value=lam)
    assert d3.shape == (7, 10) and bool((i3[:, 6:] == -1).all()) and bool(torch.isinf(d3[:, 6:]).all()) and bool((i3[:, :6] >= 0).all())
    d4, i4 = rerank(x[:1], 3, k1=k1)
    assert bool((i4 == -1).all()) and bool(torch.isinf(d4).all())


def test_match_rerank_query_gallery():
    from pets_face_recognition_amd.match import rerank, rerank_inputs
    Nq, G, D, k, k1, k2, lam, kc = 40, 200, 64, 10, 8, 3, 0.3, 30
    x = make_set("clustered", Nq + G, D, seed=31, k1=k1)
    perm = torch.randperm(Nq + G, generator=torch.Generator().manual_seed(2))
    q, g = x[perm[:Nq]].to(DEV), x[perm[Nq:]].to(DEV)
    emb32, nbr, rows, cand, cand_cos, off = rerank_inputs(q, k, k1=k1, candidates=kc, emb_b=g, compute_dtype=torch.float32)
    assert off == Nq and emb32.shape[0] == Nq + G and rows.tolist() == list(range(Nq)) and int(cand.min()) >= Nq and cand.shape == (Nq, kc)
    O, got = check_case(emb32.cpu(), nbr.cpu(), rows.cpu(), cand.cpu(), cand_cos.cpu(), k, k1, k2, lam)     # the oracle runs on the union
    dist, idx = rerank(q, k, k1=k1, k2=k2, lambda_value=lam, candidates=kc, emb_b=g, compute_dtype=torch.float32)
    assert torch.equal(dist.cpu(), got["dist"]) and torch.equal(idx.cpu() + Nq, got["idx"])                     # gallery numbering


def test_recall_at_k_with_rerank_follows_the_oracle():
    """The counts must EQUAL those of the oracle's order.  The set (noisy classes of 4; chosen on the oracle alone) has no near-tie on a K boundary: the smallest
    gap between the K-th and the (K + 1)-th oracle distance is several times the derived bound, which the test asserts, so no allowance is needed; its re-ranked
    counts differ from the cosine-order counts and from 100 % at both K."""
    from pets_face_recognition_amd.match import recall_at_k, rerank_inputs
    N, D, k1, k2, lam, ks = 120, 64, 8, 3, 0.3, (1, 10)
    g = torch.Generator().manual_seed(37)
    cls = torch.arange(N) // 4
    x = (torch.randn(N // 4, D, generator=g)[cls] + 2.0 * torch.randn(N, D, generator=g)).to(DEV)
    base = recall_at_k(x, cls.to(DEV), ks, compute_dtype=torch.float32)
    assert recall_at_k(x, cls.to(DEV), ks, compute_dtype=torch.float32, rerank=None) == base
    got = recall_at_k(x, cls.to(DEV), ks, compute_dtype=torch.float32, rerank=dict(k1=k1, k2=k2, lambda_value=lam))
    emb32, nbr, rows, cand, cand_cos, _ = rerank_inputs(x, max(ks), k1=k1, compute_dtype=torch.float32)
    fin = oracle(emb32, nbr, rows, cand, cand_cos, k1, k2, lam)["final"]
    srt = np.sort(fin, axis=1)
    assert min((srt[:, K] - srt[:, K - 1]).min() for K in ks) > 2 * dist_bound(D, k1, k2, lam)      # no row can fall either way
    ranked = np.take_along_axis(cand.cpu().numpy(), np.argsort(fin, axis=1, kind="stable"), 1)
    same = cls.numpy()[ranked] == cls.numpy()[:, None]
    want = {K: [int(same[:, :K].any(1).sum()), N] for K in ks}
    print("cosine order", base, "re-ranked", got, "oracle", want)
    assert got == want
    assert all(want[K][0] != base[K][0] and want[K][0] < N for K in ks)


def test_workspace_budget_is_enforced(monkeypatch):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import PfrError
    x = make_set("random", 50, 64, seed=1).to(DEV)
    E, E2 = capacity(20, 6)
    monkeypatch.setattr(match, "RERANK_WORKSPACE_BUDGET", 50 * (E + E2) * 8 - 1)
    with pytest.raises(PfrError, match=rf"N \* \(E \+ E2\) \* 8 = 50 \* \({E} \+ {E2}\) \* 8 = {50 * (E + E2) * 8} bytes exceeds the budget"):
        match.rerank(x, 5, compute_dtype=torch.float32)
    monkeypatch.setattr(match, "RERANK_WORKSPACE_BUDGET", 50 * (E + E2) * 8)
    dist, idx = match.rerank(x, 5, compute_dtype=torch.float32)
    assert dist.shape == (50, 5) and bool((idx >= 0).all())
