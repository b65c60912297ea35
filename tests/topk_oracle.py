"""Host restatement of the match top-K stack for the tests: the order-preserving score key, the packed list entry, the exact best-K of
a running list and a score chunk, the exact candidate set of the filter epilogue, the layout of the running state, the re-scoring with
its certificate, and the rounding bound of the real-valued re-scoring test.  Plain numpy: no device code, nothing of the library.

Order everywhere: key descending (= score descending, -0.0 below +0.0), ties by ascending gallery index.  The order is stated here with
an explicit lexsort over (key, index), NOT by sorting packed entries, so that the packing itself is under test.

The kernels keep a running list across chunks by letting a later chunk's score in only when its key is STRICTLY above the current K-th
key.  That equals the best K of (list ∪ chunk) under the order above whenever the chunk's indices are all higher than the list's —
chunks visited in ascending order, which is how every caller walks the gallery and how the GPU tests feed their chunks.

Rounding bound of pfr_topk_rescore (rescore_bound)
--------------------------------------------------
The kernel computes a dot product of two fp32 rows of length D as follows (csrc/pfr_match.hip, rescore_kernel): lane l of a wave owns the
16-byte pieces l, l + 64, ... of the row, i.e. ceil(D / 256) pieces of four elements, and folds them into ONE accumulator with
sequential fmas — m_lane = 4 * ceil(D / 256) of them (D / 64 when D is a multiple of 256).  A fma rounds once, so the product x_i * y_i
that enters at step s carries the rounding of steps s .. m_lane: at most m_lane roundings.  The 64 lane sums are then added by a
butterfly of six shuffle-add levels: six more roundings on the path of every term.  With g_scale the sum is multiplied once by the
gallery row's factor: one more.  Every term therefore passes through at most
    m = 4 * ceil(D / 256) + 6 + (1 if g_scale else 0)
roundings to nearest with unit roundoff u = 2^-24, each a factor (1 + d), |d| <= u, and (Higham, Accuracy and Stability of Numerical
Algorithms, Lemma 3.1)
    | fl(score) - score | <= gamma_m * |scale| * sum_i |x_i * y_i|,      gamma_m = m * u / (1 - m * u).
An underflowing partial result adds at most 2^-149 per rounding; m * 2^-149 is added so that the bound holds for every input.  The bound
is about the kernel's fp32 arithmetic on the fp32 inputs it is given: the reference evaluates the same fp32 inputs in float64 (whose own
error, about D * 2^-53 * sum |x_i y_i|, is eight orders of magnitude below and is added as well).  For D = 512: m = 14 (15 with g_scale),
gamma_m = 8.3e-7 — "a small multiple of 2^-24 * sum |x_i y_i|".
Two entries whose float64 scores differ by less than the sum of their two bounds may legitimately come out in either order; any
other swap is an error of the kernel."""
import numpy as np

U32 = np.uint32
U64 = np.uint64
SEL_CAP = 1536      # csrc/pfr_match.hip: direct-collect capacity of the row select
SEL_EQCAP = 1024    # csrc/pfr_match.hip: capacity of the tie buffer (more entries tied with the K-th key set flag bit 0)
FLAG_TIES = 1       # pfr_topk_flags bit 0
FLAG_OVERFLOW = 2   # pfr_topk_flags bit 1: a candidate list held more than `cap` entries


# ------------------------------------------------------------------------------------------------ key and entry
def fkey(x):
    """order-preserving float32 -> uint32 key (csrc/pfr_common.h): negative floats have every bit flipped, others the sign bit set"""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(U32)
    return np.where(u & U32(0x80000000), ~u, u | U32(0x80000000)).astype(U32)


def fkey_inv(k):
    k = np.asarray(k, dtype=U32)
    u = np.where(k & U32(0x80000000), k & U32(0x7FFFFFFF), ~k).astype(U32)
    return np.ascontiguousarray(u).view(np.float32)


def pack(key, idx):
    """list entry (key << 32) | ~idx: as unsigned 64-bit numbers, descending = key descending, then index ascending"""
    lo = (~np.asarray(idx, dtype=np.int64)) & np.int64(0xFFFFFFFF)
    return (np.asarray(key, dtype=U64) << U64(32)) | lo.astype(U64)


def unpack(e):
    """-> (key uint32, index int64 in [0, 2^32))"""
    e = np.asarray(e, dtype=U64)
    return (e >> U64(32)).astype(U32), ((~e) & U64(0xFFFFFFFF)).astype(np.int64)


def _best(key, idx, K):
    """the best K of the (key, idx) pairs, key descending and index ascending (stated by lexsort, not by the packing)"""
    order = np.lexsort((idx, -key.astype(np.int64)))[:K]
    return key[order], idx[order]


def best_entries(entry_arrays, K):
    """best K of the union of packed entry arrays -> (packed entries [<= K], thrk: key of the K-th, 0 while fewer than K exist)"""
    e = np.concatenate([np.asarray(a, dtype=U64).ravel() for a in entry_arrays]) if entry_arrays else np.zeros(0, U64)
    key, idx = unpack(e)
    key, idx = _best(key, idx, K)
    return pack(key, idx), (U32(key[K - 1]) if len(key) == K else U32(0))


def topk_exact(scores, col0, K, self_idx=None, seed=None):
    """scores [rows][n] float32 of one chunk (gallery index of column j = col0 + j); self_idx [rows] (gallery index each row must
    skip, -1 none) or None; seed: per row the packed running list so far, or None.
    -> (per row the packed best-K entries of seed ∪ chunk, thrk uint32 [rows])"""
    scores = np.asarray(scores, dtype=np.float32)
    rows, n = scores.shape
    out, thr = [], np.zeros(rows, U32)
    gidx = col0 + np.arange(n, dtype=np.int64)
    for r in range(rows):
        keep = np.ones(n, bool) if self_idx is None else gidx != int(self_idx[r])
        ent = [pack(fkey(scores[r][keep]), gidx[keep])]
        if seed is not None:
            ent.append(seed[r])
        e, t = best_entries(ent, K)
        out.append(e)
        thr[r] = t
    return out, thr


def filter_set(scores, thr_keys, col0, exclude_self):
    """per row the sorted packed entries of the chunk with key > thr_keys[row] (strict), skipping gallery index == row when exclude_self"""
    scores = np.asarray(scores, dtype=np.float32)
    rows, n = scores.shape
    gidx = col0 + np.arange(n, dtype=np.int64)
    out = []
    for r in range(rows):
        k = fkey(scores[r])
        m = k > U32(thr_keys[r])
        if exclude_self:
            m &= gidx != r
        out.append(np.sort(pack(k[m], gidx[m])))
    return out


def finish_exact(entries, K):
    """what pfr_topk_finish must write for one row: (scores float32 [K], idx int32 [K]), padded with (-inf, -1)"""
    key, idx = unpack(entries)
    sc = np.full(K, -np.inf, np.float32)
    ix = np.full(K, -1, np.int32)
    sc[:len(key)] = fkey_inv(key)
    ix[:len(key)] = idx.astype(np.int64).astype(np.int32)
    return sc, ix


# ------------------------------------------------------------------------------------------------ running-state layout
class StateLayout:
    """cur u64 [rows][K] | cur_n i32 [rows] | flags (64 bytes, the first int is the flag word) | thrk u32 [rows] | ccnt i32 [rows]
    (csrc/pfr_common.h).  `total_bytes` is what the library reports for (rows, K): a layout change fails here."""

    def __init__(self, rows, K, total_bytes):
        self.rows, self.K = rows, K
        self.off_cur = 0
        self.off_cur_n = rows * K * 8
        self.off_flags = self.off_cur_n + rows * 4
        self.off_thrk = self.off_flags + 64
        self.off_ccnt = self.off_thrk + rows * 4
        self.total = self.off_ccnt + rows * 4
        assert self.total == int(total_bytes), f"running-state layout changed: {self.total} bytes here, {total_bytes} in the library"

    def read(self, buf):
        """buf: uint8 [total] (numpy) -> dict of copies"""
        b = np.ascontiguousarray(np.asarray(buf, dtype=np.uint8))
        assert b.size == self.total
        r, K = self.rows, self.K
        return {
            "cur": b[self.off_cur:self.off_cur_n].view(U64).reshape(r, K).copy(),
            "cur_n": b[self.off_cur_n:self.off_flags].view(np.int32).copy(),
            "flags": int(b[self.off_flags:self.off_flags + 4].view(np.int32)[0]),
            "flag_pad": b[self.off_flags + 4:self.off_thrk].copy(),
            "thrk": b[self.off_thrk:self.off_ccnt].view(U32).copy(),
            "ccnt": b[self.off_ccnt:self.total].view(np.int32).copy(),
        }

    def write(self, cur=None, cur_n=None, flags=0, thrk=None, ccnt=None):
        """-> uint8 [total]; parts not given are zero (the state right after pfr_topk_reset)"""
        b = np.zeros(self.total, np.uint8)
        r, K = self.rows, self.K
        if cur is not None:
            b[self.off_cur:self.off_cur_n] = np.ascontiguousarray(np.asarray(cur, dtype=U64).reshape(r, K)).view(np.uint8).ravel()
        if cur_n is not None:
            b[self.off_cur_n:self.off_flags] = np.ascontiguousarray(np.asarray(cur_n, dtype=np.int32)).view(np.uint8)
        b[self.off_flags:self.off_flags + 4] = np.array([flags], np.int32).view(np.uint8)
        if thrk is not None:
            b[self.off_thrk:self.off_ccnt] = np.ascontiguousarray(np.asarray(thrk, dtype=U32)).view(np.uint8)
        if ccnt is not None:
            b[self.off_ccnt:self.total] = np.ascontiguousarray(np.asarray(ccnt, dtype=np.int32)).view(np.uint8)
        return b

    def entries(self, st):
        """per row the valid part of the running list of a read() result"""
        return [st["cur"][r, :st["cur_n"][r]] for r in range(self.rows)]


# ------------------------------------------------------------------------------------------------ re-scoring
def rescore_exact(q, g, g_scale, cand, cand_scores, K):
    """pfr_topk_rescore(_cert) by definition, in float64 (exact for the integer-valued rows of the exact tests, whose dots fit fp32).
    q [rows][D], g [G][D], g_scale [G] or None, cand [rows][KC] int (-1: no candidate), cand_scores [rows][KC] or None.
    -> (scores float32 [rows][K], idx int32 [rows][K], cert float32 [rows][2] or None, dots float64 [rows][KC] (nan where -1))
    cert[r][0] = max |score - cand_score| over the valid candidates; cert[r][1] = K-th best score - cand_score of the LAST candidate,
    +inf when the last candidate is -1 or fewer than K candidates are valid."""
    q = np.asarray(q, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    cand = np.asarray(cand, dtype=np.int64)
    rows, KC = cand.shape
    sc = np.full((rows, K), -np.inf, np.float32)
    ix = np.full((rows, K), -1, np.int32)
    cert = None if cand_scores is None else np.zeros((rows, 2), np.float32)
    dots = np.full((rows, KC), np.nan)
    for r in range(rows):
        v = cand[r] >= 0
        c = cand[r][v]
        d = g[c] @ q[r]
        if g_scale is not None:
            d = d * np.asarray(g_scale, dtype=np.float64)[c]
        dots[r, v] = d
        d32 = d.astype(np.float32)
        key, idx = _best(fkey(d32), c, K)
        sc[r, :len(key)] = fkey_inv(key)
        ix[r, :len(key)] = idx
        if cert is not None:
            cs = np.asarray(cand_scores, dtype=np.float32)[r]
            cert[r, 0] = np.max(np.abs(d32 - cs[v])) if v.any() else 0.0
            full = cand[r, KC - 1] >= 0 and len(key) == K
            cert[r, 1] = (sc[r, K - 1] - cs[KC - 1]) if full else np.inf
    return sc, ix, cert, dots


def rescore_bound(q_row, g_rows, g_scale=None):
    """per candidate the bound on |kernel score - exact score| derived in the module docstring.  q_row [D], g_rows [n][D] float32 values,
    g_scale [n] or None"""
    q_row = np.asarray(q_row, dtype=np.float64)
    g_rows = np.asarray(g_rows, dtype=np.float64)
    D = q_row.shape[0]
    m = 4 * ((D + 255) // 256) + 6 + (0 if g_scale is None else 1)
    u = 2.0 ** -24
    gamma = m * u / (1 - m * u)
    s = np.abs(g_rows * q_row).sum(axis=1)
    if g_scale is not None:
        s = s * np.abs(np.asarray(g_scale, dtype=np.float64))
    return gamma * s + m * 2.0 ** -149 + D * 2.0 ** -53 * s


def rescore_real_case(with_scale):
    """the one real-valued re-scoring case (fixed seed): rows = 4, D = 512, G = 600, KC = 130.  Without a scale the rows are
    normalised in fp32; with one the gallery rows stay raw and g_scale = 1 / |g| in fp32.
    -> (q f32 [4][512], g f32 [600][512], g_scale f32 [600] or None, cand int32 [4][130])"""
    rs = np.random.RandomState(20261 + int(with_scale))
    rows, D, G, KC = 4, 512, 600, 130
    q = rs.standard_normal((rows, D)).astype(np.float32)
    g = rs.standard_normal((G, D)).astype(np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    inv = (1.0 / np.linalg.norm(g.astype(np.float64), axis=1)).astype(np.float32)
    if with_scale:
        scale = inv
    else:
        g = (g * inv[:, None]).astype(np.float32)
        scale = None
    cand = np.stack([rs.permutation(G)[:KC] for _ in range(rows)]).astype(np.int32)
    return q, g, scale, cand


def check_order_within_bound(got_idx, cand_row, dots64, bound):
    """One row of the real-valued test.  got_idx [K]: the kernel's ranking; cand_row [KC] (all valid); dots64 / bound [KC]: float64
    score and rounding bound of every candidate.  Asserts: every returned index is a candidate, none twice; a returned entry may
    stand before a better one (float64) only if they differ by less than the sum of their bounds; and no candidate left out beats a
    returned one by that much or more (no entry skipped)."""
    pos = {int(c): i for i, c in enumerate(cand_row)}
    got = [int(i) for i in got_idx]
    assert len(set(got)) == len(got) and all(i in pos for i in got), "returned an index twice or one that is no candidate"
    d = np.array([dots64[pos[i]] for i in got])
    b = np.array([bound[pos[i]] for i in got])
    # suffix maximum of (d_j - b_j): entry i must satisfy d_i + b_i > d_j - b_j for every later j
    for i in range(len(got) - 1):
        j = i + 1 + int(np.argmax(d[i + 1:] - b[i + 1:]))
        assert d[i] + b[i] > d[j] - b[j] or d[i] >= d[j], f"rank {i} (index {got[i]}, {d[i]!r}) before rank {j} ({d[j]!r}): outside the rounding bound"
    rest = [c for c in pos if c not in set(got)]
    if rest:
        worst = int(np.argmin(d + b))
        for c in rest:
            assert dots64[pos[c]] - bound[pos[c]] < d[worst] + b[worst] or dots64[pos[c]] <= d[worst], \
                f"candidate {c} ({dots64[pos[c]]!r}) was skipped although it beats the returned {got[worst]} ({d[worst]!r})"
