"""Brute-force restatement of the retrieval-rank contract (include/pfr_hip.h, pfr_rank_count; match.positive_ranks / retrieval_metrics)
for the tests: a dense score matrix, per query a STABLE descending argsort over the original indices with the query removed, the ranks of
its positives read off that order, and AP / INP / CMC straight from their definitions in float64.  Python loops throughout."""
import math

import numpy as np
import torch


def class_layout(name, n, seed=0):
    """the class layouts of the tests: 'random7' (7 classes at random), 'equal' (one class), 'distinct' (no query has a positive)"""
    if name == "random7":
        return torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(seed))
    if name == "equal":
        return torch.full((n,), 3, dtype=torch.long)
    if name == "distinct":
        return torch.arange(n) * 2 + 1
    raise ValueError(name)


def positive_lists(ca, cb, sym):
    """-> list over the queries of the ascending gallery indices of the same class (the query itself left out when `sym`)"""
    ca, cb = [int(c) for c in ca], [int(c) for c in cb]
    return [[j for j in range(len(cb)) if cb[j] == ca[i] and not (sym and j == i)] for i in range(len(ca))]


def padded(lists, fill=-1):
    """list of lists -> (int64 [N, Pmax] padded with `fill`, int64 [N] lengths)"""
    pmax = max([len(l) for l in lists], default=0)
    out = torch.full((len(lists), pmax), fill, dtype=torch.int64)
    for i, l in enumerate(lists):
        out[i, :len(l)] = torch.tensor(l, dtype=torch.int64)
    return out, torch.tensor([len(l) for l in lists], dtype=torch.int64)


def ranks_from_scores(S, ca, cb, sym):
    """S [Nq, Nb] (any float tensor without NaN) -> list over the queries of the ascending 1-based ranks of the query's positives in the
    stable descending order of its row (ties: the lower index first), the query's own column removed when `sym`"""
    S = np.asarray(S.detach().cpu().double())
    pos = positive_lists(ca, cb, sym)
    out = []
    for i in range(S.shape[0]):
        ids = np.array([j for j in range(S.shape[1]) if not (sym and j == i)], dtype=np.int64)
        order = ids[np.argsort(-S[i, ids], kind="stable")] if len(ids) else ids
        place = {int(j): r + 1 for r, j in enumerate(order)}
        out.append(sorted(place[j] for j in pos[i]))
    return out


def counts_from_scores(S, ids, thr, tid, tcnt, excl=None):
    """the count of pfr_rank_count by brute force: S [Na, Nb] fp32 scores, ids [Nb], thresholds thr / tid [Na, ld] with tcnt [Na], excl [Na]
    or None -> int64 [Na, ld] (0 past tcnt).  Comparisons in the scores' own fp32."""
    S, thr = np.asarray(S.detach().cpu().float()), np.asarray(thr.detach().cpu().float())
    ids, tid, tcnt = (np.asarray(t.detach().cpu()).astype(np.int64) for t in (ids, tid, tcnt))
    ex = None if excl is None else np.asarray(excl.detach().cpu()).astype(np.int64)
    out = np.zeros(thr.shape, dtype=np.int64)
    for i in range(S.shape[0]):
        n = int(tcnt[i])
        keep = np.ones(S.shape[1], dtype=bool) if ex is None else ids != ex[i]
        t, ti = thr[i, :n, None], tid[i, :n, None]
        pre = (S[i][None, :] > t) | ((S[i][None, :] == t) & (ids[None, :] < ti))
        out[i, :n] = (pre & keep[None, :]).sum(axis=1)
    return torch.from_numpy(out)


def metrics(ranks, ks=(1, 5, 10)):
    """list of rank lists -> the metric dict of match.retrieval_metrics, float64, from the definitions"""
    valid = [r for r in ranks if len(r)]
    out = {}
    if not valid:
        out = {"mAP": math.nan, "mINP": math.nan}
        out.update((f"CMC@K={k}", math.nan) for k in ks)
        out.update(mean_first_rank=math.nan, queries=0)
        return out
    ap = [sum((k + 1) / r for k, r in enumerate(sorted(rs))) / len(rs) for rs in valid]
    inp = [len(rs) / max(rs) for rs in valid]
    first = [min(rs) for rs in valid]
    q = len(valid)
    out = {"mAP": math.fsum(ap) / q, "mINP": math.fsum(inp) / q}
    out.update((f"CMC@K={k}", sum(1 for f in first if f <= k) / q) for k in ks)
    out.update(mean_first_rank=math.fsum(first) / q, queries=q)
    return out


def as_lists(ranks, npos):
    """the (ranks, npos) tensors of match.positive_ranks -> list of lists; checks the padding on the way"""
    ranks, npos = ranks.detach().cpu().long(), npos.detach().cpu().long()
    out = []
    for i in range(ranks.shape[0]):
        n = int(npos[i])
        assert bool((ranks[i, n:] == 0).all()), f"row {i}: padding is not 0"
        out.append([int(v) for v in ranks[i, :n]])
    return out


def assert_metrics_equal(got, want, tol=1e-12):
    assert list(got.keys()) == list(want.keys()), (list(got.keys()), list(want.keys()))
    for k in want:
        if k == "queries":
            assert got[k] == want[k], (k, got[k], want[k])
        elif math.isnan(want[k]):
            assert math.isnan(got[k]), (k, got[k])
        else:
            assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])
