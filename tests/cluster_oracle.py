"""Independent restatement of the threshold clustering for the tests: a host union-find over an edge list, and the clustering metrics from
a DENSE contingency matrix in Python integers / float64 (the package computes them from torch.unique counts and builds nothing dense)."""
import math
from fractions import Fraction

import torch


def components(n, edges):
    """edges: iterable of (u, v) -> list of n labels, each the smallest node id of the component (union by index, full compression)"""
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root
    for u, v in edges:
        ru, rv = find(int(u)), find(int(v))
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return [find(x) for x in range(n)]


def edges_from_scores(s, thr, sym):
    """dense scores [Na, Nb] -> sorted list of (i, j) with s >= thr (IEEE: NaN never), i < j only when sym"""
    ok = s >= thr
    if sym:
        ok = ok & torch.ones_like(ok).triu(1)
    return sorted(map(tuple, ok.nonzero().tolist()))


def metrics(labels, classes):
    """the contract's numbers from the dense contingency table"""
    labels, classes = [int(x) for x in labels], [int(x) for x in classes]
    N = len(labels)
    ks, cs = sorted(set(labels)), sorted(set(classes))
    table = [[0] * len(cs) for _ in ks]
    for k, c in zip(labels, classes):
        table[ks.index(k)][cs.index(c)] += 1
    a = [sum(row) for row in table]
    b = [sum(table[k][c] for k in range(len(ks))) for c in range(len(cs))]
    c2 = lambda x: x * (x - 1) // 2
    tp = sum(c2(n) for row in table for n in row)
    ratio = lambda x, y: float(Fraction(x, y)) if y else float("nan")
    f = lambda p, r: 2 * p * r / (p + r) if p + r > 0 else float("nan")
    p, r = ratio(tp, sum(map(c2, a))), ratio(tp, sum(map(c2, b)))
    bp = float(sum(Fraction(table[k][c] ** 2, a[k]) for k in range(len(ks)) for c in range(len(cs))) / N) if N else float("nan")
    br = float(sum(Fraction(table[k][c] ** 2, b[c]) for k in range(len(ks)) for c in range(len(cs)) if b[c]) / N) if N else float("nan")
    return {"pairwise_precision": p, "pairwise_recall": r, "pairwise_f": f(p, r), "bcubed_precision": bp, "bcubed_recall": br,
            "bcubed_f": f(bp, br), "clusters": len(ks), "singletons": sum(1 for x in a if x == 1)}


def assert_metrics_equal(got, want, tol=1e-12):
    assert list(got.keys()) == list(want.keys())
    for k, w in want.items():
        g = got[k]
        if isinstance(w, int):
            assert g == w, (k, g, w)
        elif math.isnan(w):
            assert math.isnan(g), (k, g, w)
        else:
            assert abs(g - w) <= tol, (k, g, w)
