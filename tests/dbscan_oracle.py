"""Independent restatement of the DBSCAN contract of include/pfr_hip.h for the tests, in plain Python over a DENSE score matrix: boolean
adjacency, degrees and the core set, the components of the core nodes (cluster_oracle.components) relabelled to the smallest core index,
the best core neighbour of every other node by (score, -index) with -0.0 canonicalised, and noise."""
import cluster_oracle as O


def adjacency(S, thr):
    """dense scores [N][N] (torch tensor or nested lists) -> N x N list of bools: s >= thr (IEEE: NaN never), no diagonal, symmetric.
    Only the upper triangle i < j of S is read: the pairs the entry points visit."""
    rows = S.tolist() if hasattr(S, "tolist") else S
    n = len(rows)
    adj = [[False] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            if rows[i][j] >= thr:
                adj[i][j] = adj[j][i] = True
    return adj


def dbscan(S, thr, min_samples, adj=None):
    """-> (deg, core, labels): lists of N ints / bools / ints (label -1 = noise).  adj: the adjacency of (S, thr) when the caller has it
    already (a grid of min_samples over one threshold)."""
    rows = S.tolist() if hasattr(S, "tolist") else S
    n = len(rows)
    adj = adjacency(rows, thr) if adj is None else adj
    deg = [sum(r) for r in adj]
    core = [d >= min_samples - 1 for d in deg]
    comp = O.components(n, [(i, j) for i in range(n) for j in range(i + 1, n) if adj[i][j] and core[i] and core[j]])
    # components() labels by the smallest node id; only core nodes were united, so a core node's label is the smallest CORE index
    labels = [-1] * n
    for x in range(n):
        if core[x]:
            labels[x] = comp[x]
            continue
        best = None
        for c in range(n):
            if adj[x][c] and core[c]:
                s = rows[min(x, c)][max(x, c)] + 0.0          # -0.0 -> +0.0 (Python compares them equal anyway; said for the record)
                if best is None or (s, -c) > best:
                    best = (s, -c)
        if best is not None:
            labels[x] = comp[-best[1]]
    return deg, core, labels


def kinds(core, labels):
    """-> (number of core nodes, of border nodes, of noise nodes, of clusters)"""
    n_core = sum(core)
    n_noise = sum(1 for l in labels if l < 0)
    return n_core, len(labels) - n_core - n_noise, n_noise, len({l for l in labels if l >= 0})
