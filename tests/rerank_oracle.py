"""Dense fp64 restatement of the k-reciprocal re-ranking contract (include/pfr_hip.h, pfr_rerank_*), written from the published algorithm
(Zhong et al., CVPR 2017) for the tests: Python sets for the integer part, N x N float64 matrices for the rest.  It consumes the SAME fp32
inputs as the code under test — unit rows, nbr, rows, cand, cand_cos — so ties at the list boundaries cannot make the two disagree."""
import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32


def capacity(k1, k2):
    kh = round(k1 / 2)
    E = (k1 + 1) + (k1 + 1) * (kh + 1)
    return E, k2 * E


def tol_m(D, k1, k2):
    """bound on |m_dev - m| (see tests/test_rerank_gpu.py for the derivation)"""
    E, E2 = capacity(k1, k2)
    return (4 * D + 2 * E + 2 * E2 + 16) * U


def dist_bound(D, k1, k2, lam):
    return 2 * (1 - lam) * tol_m(D, k1, k2) + 2 * lam * D * U


def oracle(emb32, nbr, rows, cand, cand_cos, k1, k2, lam):
    """-> dict(sets: list of N Python sets R*(i), V, Vq: float64 [N, N], final: float64 [R, kc] (+inf where the candidate is padding))"""
    emb = emb32.detach().cpu().double().numpy()
    nbr, rows, cand = (np.asarray(t.detach().cpu()) for t in (nbr, rows, cand))
    cos = cand_cos.detach().cpu().double().numpy()
    lam = float(np.float32(lam))
    N = emb.shape[0]
    kh = round(k1 / 2)
    L = [[int(e) for e in row if 0 <= e < N] for row in nbr]

    def recip(i, k):
        return {j for j in L[i][:k + 1] if i in L[j][:k + 1]}

    S = emb @ emb.T
    V = np.zeros((N, N))
    sets = []
    for i in range(N):
        r0 = recip(i, k1)
        rs = set(r0)
        for j in r0:
            rj = recip(j, kh)
            if 3 * len(rj & r0) > 2 * len(rj):
                rs |= rj
        sets.append(rs)
        js = sorted(rs)
        if js:
            w = np.exp(-(2.0 - 2.0 * S[i, js]))
            V[i, js] = w / w.sum()
    Vq = np.zeros((N, N))
    for i in range(N):
        ns = L[i][:k2]
        if ns:
            Vq[i] = V[ns].sum(0) / len(ns)
    final = np.full(cand.shape, np.inf)
    for r, i in enumerate(rows):
        if not 0 <= i < N:
            continue
        for t, c in enumerate(cand[r]):
            if 0 <= c < N:
                m = np.minimum(Vq[i], Vq[c]).sum()
                final[r, t] = (1.0 - lam) * (1.0 - m / (2.0 - m)) + lam * (2.0 - 2.0 * cos[r, t])
    return {"sets": sets, "V": V, "Vq": Vq, "final": final}


def unit_rows(x):
    x = x.float()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def lists_from_rows(emb32, k1, kc, rows=None):
    """nbr / cand lists from the fp32 dot products of unit rows (CPU torch, self excluded, -1 / -inf padded)"""
    N = emb32.shape[0]
    S = emb32 @ emb32.t()
    S.fill_diagonal_(-float("inf"))
    order = torch.argsort(S, dim=1, descending=True, stable=True)[:, :max(N - 1, 0)]
    sc = torch.gather(S, 1, order)

    def pad(s, i, w):
        s, i = s[:, :w], i[:, :w].int()
        p = w - s.shape[1]
        if p > 0:
            s = torch.cat([s, torch.full((N, p), -float("inf"))], 1)
            i = torch.cat([i, torch.full((N, p), -1, dtype=torch.int32)], 1)
        return s.contiguous(), i.contiguous()

    nbr = torch.cat([torch.arange(N, dtype=torch.int32)[:, None], pad(sc, order, k1)[1]], 1).contiguous()
    cand_cos, cand = pad(sc, order, kc)
    if rows is None:
        rows = torch.arange(N, dtype=torch.int32)
    rows = rows.int()
    return nbr, rows, cand[rows.long()].contiguous(), cand_cos[rows.long()].contiguous()


def make_set(layout, N, D, seed, k1=5):
    g = torch.Generator().manual_seed(seed)
    if layout == "random":
        x = torch.randn(N, D, generator=g)
    elif layout == "tight":          # one tight cluster: every expansion is accepted and everything is a duplicate
        x = torch.randn(1, D, generator=g) + 0.01 * torch.randn(N, D, generator=g)
    else:                            # classes of unequal size 1, 2, 3, ... items
        sizes, c = [], 1
        while sum(sizes) < N:
            sizes.append(min(c, N - sum(sizes)))
            c = c % (k1 + 3) + 1
        cls = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
        x = torch.randn(len(sizes), D, generator=g)[cls] + 0.25 * torch.randn(N, D, generator=g)
    return unit_rows(x)
