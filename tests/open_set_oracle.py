"""Independent restatement of the pfr_class_extremes / pfr_extremes_decode contract of include/pfr_hip.h for the tests, over a DENSE score
matrix and class vectors: the mate rule (equal classes, not negative), distractors, the NaN gate, the -0.0 canonicalisation, the tie rule
(highest — for the weakest mate lowest — score, then the smallest partner index), the 64-bit key encoding and its decoding.  `extremes` is
plain Python, pair by pair, in the order a reader would write it; `extremes_torch` is the same contract with torch ops for sets too large
for a Python loop (the two are compared in tests/test_open_set_host.py)."""
import functools
import math
import struct

import torch

MASK32 = 0xFFFFFFFF
INF = float("inf")


@functools.lru_cache(maxsize=None)
def ord32(s):
    """order-preserving uint32 of a float32 value, -0.0 canonicalised to +0.0"""
    u = struct.unpack("<I", struct.pack("<f", s + 0.0))[0]
    return (~u & MASK32) if u & 0x80000000 else (u ^ 0x80000000)


def unord32(k):
    u = (k ^ 0x80000000) if k & 0x80000000 else (~k & MASK32)
    return struct.unpack("<f", struct.pack("<I", u))[0]


def key(s, partner, lowest=False):
    o = ord32(s)
    return (((~o & MASK32) if lowest else o) << 32) | (MASK32 - partner)


def decode(k, kind):
    """-> (score, index) of pfr_extremes_decode"""
    partner = MASK32 - (k & MASK32)
    if k == 0 or partner >= 2 ** 31:
        return (INF if kind else -INF), -1
    o = k >> 32
    return unord32((~o & MASK32) if kind else o), partner


def extremes(S, cls_a, cls_b=None, a_off=0, b_off=0, both_sides=False, n_nodes=None, keys=None):
    """S: dense scores (torch tensor or nested lists).  cls_b None: symmetric mode — S is [N][N], only i < j is read, both nodes of a pair
    are updated.  Otherwise S is [Na][Nb], every pair updates node a_off + i, and node b_off + j too with both_sides.
    -> [best_pos, best_neg, worst_pos]: three lists of n_nodes Python ints (keys); `keys` accumulates into an earlier result."""
    rows = S.tolist() if hasattr(S, "tolist") else S
    ca = [int(c) for c in cls_a]
    sym = cls_b is None
    cb = ca if sym else [int(c) for c in cls_b]
    if sym:
        b_off = a_off
    if n_nodes is None:
        n_nodes = max(a_off + len(ca), (b_off + len(cb)) if (sym or both_sides) else 0)
    out = keys if keys is not None else [[0] * n_nodes for _ in range(3)]

    def update(x, partner, s, mate):
        if mate:
            out[0][x] = max(out[0][x], key(s, partner))
            out[2][x] = max(out[2][x], key(s, partner, lowest=True))
        else:
            out[1][x] = max(out[1][x], key(s, partner))
    for i in range(len(ca)):
        for j in range(i + 1 if sym else 0, len(cb)):
            s = rows[i][j]
            if math.isnan(s):
                continue
            mate = ca[i] == cb[j] and ca[i] >= 0
            update(a_off + i, b_off + j, s, mate)
            if sym or both_sides:
                update(b_off + j, a_off + i, s, mate)
    return out


def decoded(keys):
    """-> (pos_score, pos_index, neg_score, neg_index, weak_score, weak_index) as lists"""
    out = []
    for kind, ks in ((0, keys[0]), (0, keys[1]), (1, keys[2])):
        d = [decode(k, kind) for k in ks]
        out += [[x[0] for x in d], [x[1] for x in d]]
    return tuple(out)


def _ord_t(s):
    u = (s + 0.0).contiguous().view(torch.int32).long() & MASK32
    return torch.where((u & 0x80000000) != 0, ~u & MASK32, u ^ 0x80000000)


def extremes_torch(S, cls):
    """symmetric mode with torch ops: S [N, N] fp32 (the upper triangle is read) -> three int64 [N] tensors holding the keys' 64 bits"""
    n = S.shape[0]
    up = torch.ones(n, n, dtype=torch.bool).triu(1)
    full = torch.where(up, S, S.t())
    valid = ~torch.isnan(full) & ~torch.eye(n, dtype=torch.bool)
    c = cls.long()
    mate = (c[:, None] == c[None, :]) & (c[:, None] >= 0)
    o = _ord_t(full)
    low = MASK32 - torch.arange(n)[None, :].expand(n, n)
    out = []
    for ok, oo in ((valid & mate, o), (valid & ~mate, o), (valid & mate, ~o & MASK32)):
        # (the two halves separately: the 64-bit key does not fit a signed comparison)
        hi = torch.where(ok, oo, torch.full_like(oo, -1))
        top = hi.max(dim=1, keepdim=True).values
        lo = torch.where(ok & (hi == top), low, torch.full_like(low, -1)).max(dim=1).values
        has = ok.any(dim=1)
        k = (top[:, 0] << 32) | lo
        out.append(torch.where(has, k, torch.zeros_like(k)))
    return out


def as_unsigned(t):
    """int64 tensor holding key bits -> list of Python ints in [0, 2^64)"""
    return [v & (2 ** 64 - 1) for v in t.tolist()]


def class_patterns(n, seed):
    """the class vectors of the tests: all one class, all distinct, classes of 3 with singletons, and negative (distractor) classes"""
    g = torch.Generator().manual_seed(seed)
    threes = torch.arange(n) // 3
    threes = torch.where(torch.arange(n) % 7 == 6, 1000 + torch.arange(n), threes)          # every seventh item is a singleton
    neg = threes.clone()
    neg[torch.arange(n) % 5 == 1] = -1
    neg[torch.arange(n) % 11 == 3] = -4
    pats = {"one": torch.zeros(n, dtype=torch.int64), "distinct": torch.arange(n), "threes": threes, "negative": neg}
    return {k: v[torch.randperm(n, generator=g)] for k, v in pats.items()}
