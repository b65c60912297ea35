"""The match top-K kernels through the C ABI against tests/topk_oracle.py: pfr_topk_update (row select), pfr_topk_merge (wave and block
merge), the filter epilogue of pfr_match_scores_filter / _i8, pfr_match_scores_i8 and pfr_topk_rescore / _cert.

Every expectation is exact (indices and score bits) except the one real-valued re-scoring case, which is held to the rounding bound
derived in topk_oracle's docstring.  GEMM scores are exact by construction: embedding entries are integers in [-3, 3] (products and sums
are integers far below 2^24, exact in fp32 in any summation order; exact in bf16 operands), int8 rows carry power-of-two scales.
Integer scores give long tie runs, which is wanted.  Thresholds are set through the public calls (pfr_topk_reset + pfr_topk_update on a
hand-made score chunk); thrk / ccnt / cur_n are read back with the oracle's layout reader.  Caller-owned outputs are filled with a
sentinel and followed by a guard region; what a call must not touch has to keep the sentinel.  Every filter case computes the launch it
expects from the dispatch rule and the device's CU count and asserts pfr_debug_last_conv_kernel (family 11) against it.

Tie flag (bit 0 of pfr_topk_flags) contract, DESIGN.md §Match: with more than 1024 entries tied at the K-th key the returned scores
are still the exact top-K scores and every returned index carries its returned score; only WHICH of the tied indices fill the last
places is unspecified.  With at most 1024 such ties the flag stays clear and the lowest indices win."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import topk_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256                               # guard elements behind every caller-owned buffer
CAND_SENT = 0x5A5A5A5A5A5A5A5A            # candidate slots (as int64)
F_SENT = 12345.678                        # float outputs
I_SENT = -777                             # index outputs
CUR_SENT = np.uint64(0x7777777777777777)  # running-list slots beyond the valid count
PFR_CK_MATCH_FILTER = 11


def L():
    from pets_face_recognition_amd._hip import lib
    return lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ceil(a, b):
    return (a + b - 1) // b


class Guarded:
    """device buffer of `shape` filled with a sentinel, with GUARD more sentinel elements behind it"""

    def __init__(self, shape, dtype, sentinel):
        self.shape, self.n, self.sent = tuple(shape), int(np.prod(shape)), sentinel
        self.flat = torch.full((self.n + GUARD,), sentinel, dtype=dtype, device=DEV)

    @property
    def ptr(self):
        return self.flat.data_ptr()

    @property
    def view(self):
        return self.flat[:self.n].view(self.shape)

    def numpy(self):
        torch.cuda.synchronize()
        assert bool((self.flat[self.n:] == self.sent).all()), "guard region behind the buffer was written"
        return self.view.cpu().numpy()


class State:
    """running top-K state, reset; 256 guard bytes behind it"""

    def __init__(self, rows, K):
        self.rows, self.K = rows, K
        self.nbytes = int(L().pfr_topk_state_bytes(rows, K))
        self.lay = O.StateLayout(rows, K, self.nbytes)
        self.buf = torch.full((self.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        L().pfr_topk_reset(self.ptr, rows, K, _st())

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def read(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        assert (b[self.nbytes:] == 0xA5).all(), "bytes behind the running state were written"
        st = self.lay.read(b[:self.nbytes])
        assert not st["flag_pad"].any()
        return st

    def poke(self, offset, arr):
        raw = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).ravel().copy())
        self.buf[offset:offset + raw.numel()].copy_(raw)

    def update(self, scores, n, col0, self_idx=None):
        """scores: device float32 [rows][ld]"""
        L().pfr_topk_update(scores.data_ptr(), self.rows, scores.shape[1], n, col0, self.K, self.ptr,
                            0 if self_idx is None else self_idx.data_ptr(), _st())

    def flags(self):
        flag = ctypes.c_int(-1)
        L().pfr_topk_flags(self.ptr, self.rows, self.K, ctypes.addressof(flag), _st())
        return flag.value

    def finish(self):
        sc = Guarded((self.rows, self.K), torch.float32, F_SENT)
        ix = Guarded((self.rows, self.K), torch.int32, I_SENT)
        L().pfr_topk_finish(self.ptr, self.rows, self.K, sc.ptr, ix.ptr, _st())
        return sc.numpy(), ix.numpy()

    def check(self, want_entries, want_thrk, flags=0):
        """list, counts, thresholds and pfr_topk_finish against the oracle's entries"""
        st = self.read()
        assert st["cur_n"].tolist() == [len(e) for e in want_entries]
        for r, e in enumerate(want_entries):
            assert np.array_equal(st["cur"][r, :len(e)], e), f"row {r}: running list differs"
        assert np.array_equal(st["thrk"], want_thrk)
        assert st["flags"] == flags == self.flags()
        sc, ix = self.finish()
        for r, e in enumerate(want_entries):
            wsc, wix = O.finish_exact(e, self.K)
            assert np.array_equal(sc[r].view(np.uint32), wsc.view(np.uint32)) and np.array_equal(ix[r], wix), f"row {r}: finish"
        return st


def _chunk(scores, ld=None):
    """host [rows][n] -> device [rows][ld] with +inf in the padding columns (never read)"""
    rows, n = scores.shape
    ld = ld or _ceil(n, 4) * 4
    out = np.full((rows, ld), np.inf, np.float32)
    out[:, :n] = scores
    return torch.from_numpy(out).to(DEV)


# ================================================================================================ a. pfr_topk_update
@pytest.mark.parametrize("K", [1, 10, 257, 512])
def test_update_chunk_sequence_is_exact(K):
    """n = 5 (list not full for K > 5), 3000 (radix select, 0 < have < K), 2048 ascending and all above the threshold (radix select
    with a full list), 1537 / 1536 all above (SEL_CAP boundary), 4099 with ld = 4100 (n % 4 tail, +inf padding never read); a large odd
    col0; self_idx at the first column, at the tail column, at the best score, in no chunk, and -1."""
    rows, rs, c0 = 8, np.random.RandomState(100 + K), 1000003
    sizes = [5, 3000, 2048, 1537, 1536, 4099]
    starts = np.cumsum([c0] + sizes)[:-1]
    chunks = [rs.randint(-50, 51, (rows, 5)), rs.randint(-50, 51, (rows, 3000)),
              100 + 0.5 * np.arange(2048)[None, :] + np.arange(rows)[:, None],
              5000 + rs.randint(0, 40, (rows, 1537)), 9000 + rs.randint(0, 40, (rows, 1536)), rs.randint(8990, 9060, (rows, 4099))]
    chunks = [c.astype(np.float32) for c in chunks]
    self_idx = np.array([-1, starts[1], starts[5] + 4098, 7, starts[2] + 2047, starts[0], -1, starts[4] + 700], np.int64)
    for r, s in enumerate(self_idx):            # the skipped column would be the row's best: skipping it must matter
        for c, a in zip(chunks, starts):
            if a <= s < a + c.shape[1]:
                c[r, s - a] = 1e6
    sidx = torch.tensor(self_idx, dtype=torch.int32, device=DEV)
    state, seed = State(rows, K), None
    for c, a in zip(chunks, starts):
        state.update(_chunk(c, 4100 if c.shape[1] == 4099 else None), c.shape[1], int(a), sidx)
        seed, thr = O.topk_exact(c, int(a), K, self_idx=self_idx, seed=seed)
        st = state.check(seed, thr)
        assert not st["ccnt"].any()
    assert all(float(O.fkey_inv(O.unpack(e)[0])[0]) < 1e6 for e in seed)


@pytest.mark.parametrize("seeded", [False, True], ids=["first_chunk", "full_list"])
@pytest.mark.parametrize("K", [10, 257])
def test_update_ties_at_the_kth_value(K, seeded):
    """n = 3000 (radix select: first chunk below the pivot size, or a later chunk with more than 1536 winners): 4 scores above a run of T
    tied scores that holds the K-th place.  T <= 1024 (1024, 3K, 1000): flag clear, lowest indices win.  T > 1024 (1025, 2000): flag
    bit 0, exact scores, every index carries its score."""
    n, rs = 3000, np.random.RandomState(K)

    def rows_of(counts):
        s = np.zeros((len(counts), n), np.float32)
        for r, T in enumerate(counts):
            p = rs.permutation(n)
            s[r, p[:4]] = 2.0
            s[r, p[4:4 + T]] = 1.0
        return s

    for counts, flagged in (([1024, 3 * K, 1000], False), ([1025, 2000], True)):
        s = rows_of(counts)
        rows = len(counts)
        state, seed, col0 = State(rows, K), None, 0
        if seeded:
            low = np.full((rows, K), -5.0, np.float32)
            state.update(_chunk(low), K, 0)
            seed, _ = O.topk_exact(low, 0, K)
            col0 = K
        state.update(_chunk(s), n, col0)
        want, thr = O.topk_exact(s, col0, K, seed=seed)
        if not flagged:
            state.check(want, thr)
            continue
        st = state.read()
        assert st["flags"] & O.FLAG_TIES and state.flags() & O.FLAG_TIES
        assert np.array_equal(st["thrk"], thr) and st["cur_n"].tolist() == [K] * rows
        sc, ix = state.finish()
        for r in range(rows):
            wsc, wix = O.finish_exact(want[r], K)
            assert np.array_equal(sc[r].view(np.uint32), wsc.view(np.uint32)), "flagged: the scores are still the exact top-K scores"
            assert len(set(ix[r].tolist())) == K and ix[r].min() >= col0 and ix[r].max() < col0 + n
            assert np.array_equal(s[r, ix[r] - col0], sc[r]), "flagged: every returned index carries its returned score"
            assert np.array_equal(ix[r, :4], wix[:4]), "entries above the tied run are not affected"


# ================================================================================================ b. pfr_topk_merge
def _merge_case(K, have, cs, cap, seed_no):
    """rows = len(cs); every row gets a running list of `have` entries (indices from 10000) through pfr_topk_update, then cs[r] candidates
    written straight into cand / ccnt.  Integer scores in [0, 30]: candidates tie running entries; candidate indices lie below the
    running ones on even rows (win ties) and above on odd rows (lose ties)."""
    lib, rows, rs = L(), len(cs), np.random.RandomState(seed_no)
    state = State(rows, K)
    base = rs.randint(0, 31, (rows, have)).astype(np.float32)
    state.update(_chunk(base), have, 10000)
    seed, thr0 = O.topk_exact(base, 10000, K)
    st0 = state.check(seed, thr0)
    if have < K:
        state.poke(state.lay.off_cur, np.where(np.arange(K)[None, :] < have, st0["cur"], CUR_SENT))
    cand = Guarded((rows, cap), torch.int64, CAND_SENT)
    host = np.full((rows, cap), CAND_SENT, np.uint64)
    ents = []
    for r, c in enumerate(cs):
        m = min(c, cap)
        idx = (0 if r % 2 == 0 else 20000) + rs.permutation(5000)[:m]
        # rows 5 and up: every candidate is below the whole running list, so the running list's LAST entry decides the result (it is
        # element c + have - 1 of the merge: the one a hand-off past 256 elements to the wave kernel would lose)
        sc = rs.randint(0, 31, m) if r < 5 else rs.randint(-40, -9, m)
        ents.append(O.pack(O.fkey(sc.astype(np.float32)), idx))
        host[r, :m] = ents[r]
    cand.view.copy_(torch.from_numpy(host.view(np.int64)))
    state.poke(state.lay.off_ccnt, np.array(cs, np.int32))
    lib.pfr_topk_merge(cand.ptr, cap, rows, K, state.ptr, _st())
    st = state.read()
    over = any(c > cap for c in cs)
    assert st["flags"] == (O.FLAG_OVERFLOW if over else 0) == state.flags()
    assert not st["ccnt"].any(), "every merged row leaves ccnt = 0"
    for r, c in enumerate(cs):
        want, thr = O.best_entries([seed[r], ents[r]], K)
        keep = len(want)
        assert keep == min(K, have + min(c, cap)) == st["cur_n"][r], r
        assert np.array_equal(st["cur"][r, :keep], want), f"row {r} (c = {c}, have = {have})"
        assert st["thrk"][r] == thr and (keep == K or thr == 0), r
        assert (st["cur"][r, keep:] == CUR_SENT).all(), f"row {r}: list written beyond the {keep} kept entries"
    assert np.array_equal(cand.numpy().view(np.uint64), host), "the candidate buffer is an input"


@pytest.mark.parametrize("K,have,cs,cap", [
    (100, 100, [1, 0, 155, 156, 0, 157, 400], 1536),     # wave kernel up to c + have = 256, block kernel from 257, in ONE launch; rows % 4 != 0
    (256, 256, [1, 0, 5, 300, 1536], 1536),              # c + have > 256 always: block kernel
    (300, 300, [1, 100, 0, 1536], 1536),                 # K > 256: no wave launch
    (100, 40, [10, 59, 60, 61, 0, 216, 217], 1536),      # lists not full: thrk stays 0 below K entries; 256 / 257 again with have = 40
    (100, 100, [64, 3, 0, 64], 64),                      # c == cap: no flag
    (100, 100, [65, 3, 64], 64),                         # c == cap + 1: flag bit 1, the first cap entries merged
    (100, 100, [1536, 7], 1536),
    (100, 100, [1537, 7], 1536),
    (512, 512, [1536, 1], 1536),                         # cap + K = 2048: the whole sort buffer
], ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_merge_is_exact(K, have, cs, cap):
    _merge_case(K, have, cs, cap, seed_no=K + have + cap + len(cs))


# ================================================================================================ c. the filter epilogue
KINDS = {"f32": 0, "bf16": 1, "i8": 2}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _expected_launch(kind, Q, n, order):
    """the dispatch rule of pfr_match_scores_filter(_i8) / launch_filter_k restated -> (id, big tile?, several tiles per workgroup?, slots)"""
    big = kind != "f32" and _ceil(Q, 256) * _ceil(n, 256) >= 160
    B = 256 if big else 128
    tm, tn = _ceil(Q, B), _ceil(n, B)
    slots = _cus() * (1 if big else 2)
    multi = tm * tn > slots
    qg = 0
    if multi and slots % 8 == 0 and order:
        wpx, qg = slots // 8, 1
        while qg * 2 <= 8 and qg * 2 <= tm and wpx % (qg * 2) == 0:
            qg *= 2
    ident = (PFR_CK_MATCH_FILTER << 24) | (4 if big else 0) | 8 | (16 if multi else 0) | (32 if qg else 0) | (KINDS[kind] << 6) | (qg << 8)
    return ident, big, multi, slots


def _dims(kind):
    """(row length, leading constant part): D = 64, Dp = 128; the first quarter of a row is constant (2 in the gallery, the row's bias
    in a query), so score = bias * 2 * (D / 4) + noise and a row's sign pattern is chosen by its bias"""
    D = 128 if kind == "i8" else 64
    return D, D // 4


@functools.lru_cache(maxsize=4)
def _noise(kind, Q, n, seed):
    """integer embeddings (random part) and their exact dot products"""
    D, lead = _dims(kind)
    rs = np.random.RandomState(seed)
    q = rs.randint(-3, 4, (Q, D)).astype(np.int8)
    g = rs.randint(-3, 4, (n, D)).astype(np.int8)
    q[:, :lead], g[:, :lead] = 0, 2
    dots = q.astype(np.float64) @ g.astype(np.float64).T          # integers: exact
    return q, g, dots


def _scales(kind, Q, n):
    if kind != "i8":
        return None, None
    return (2.0 ** -(np.arange(Q) % 3)).astype(np.float32), (2.0 ** -(4 + np.arange(n) % 2)).astype(np.float32)


def _exact_scores(kind, acc, sq, sg):
    """acc: exact integer dots (float64) -> the fp32 scores as the library defines them"""
    s = acc.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), acc)
    return s if kind != "i8" else (s * sq[:, None]) * sg[None, :]


def _dev_rows(kind, x):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(DEV) if kind == "i8" else t.to(DEV, torch.float32 if kind == "f32" else torch.bfloat16)


def _run_filter(kind, q, g, sq, sg, Q, n, col0, state, cand, cap, excl):
    """q, g (and scales) device tensors; g / sg start at the chunk's first row -> launch id"""
    D = q.shape[1]
    if kind == "i8":
        L().pfr_match_scores_filter_i8(q.data_ptr(), sq.data_ptr(), g.data_ptr(), sg.data_ptr(), Q, n, D, col0, state.K, state.ptr, cand.ptr,
                                       cap, int(excl), _st())
    else:
        L().pfr_match_scores_filter(q.data_ptr(), g.data_ptr(), KINDS[kind], Q, n, D, col0, state.K, state.ptr, cand.ptr, cap, int(excl), _st())
    return L().pfr_debug_last_conv_kernel()


def _threshold_state(Q, thr):
    """running state whose thrk is fkey(thr[r]) (K = 1, one hand-made score per row), or all 0 = lists not full (thr None: K = 2)"""
    if thr is None:
        state = State(Q, 2)
        state.update(_chunk(np.zeros((Q, 1), np.float32)), 1, 0)
        want = np.zeros(Q, np.uint32)
    else:
        state = State(Q, 1)
        state.update(_chunk(np.asarray(thr, np.float32).reshape(Q, 1)), 1, 0)
        want = O.fkey(np.asarray(thr, np.float32))
    st = state.read()
    assert np.array_equal(st["thrk"], want) and not st["ccnt"].any()
    return state, want


def _pick_thresholds(scores, dense_rows=32, dense=0.06, sparse=0.003):
    """row r: the m-th largest score of the row (a value that OCCURS: the strict compare must keep its ties out); odd rows sit 2^-12
    above it (between two score values).  The first `dense_rows` rows let `dense` of the chunk through, the rest `sparse`."""
    Q, n = scores.shape
    thr = np.empty(Q, np.float32)
    for r in range(Q):
        m = max(2, int(n * (dense if r < dense_rows else sparse))) + r % 3
        thr[r] = np.partition(scores[r], n - m)[n - m] + (2.0 ** -12 if r % 2 else 0.0)
    return thr


def _check_candidates(state, cand, want, cap, ccnt_before=None):
    """every row's cand[r][:ccnt[r]] as a set == the exact set: nothing missing, nothing extra, nothing twice; the slots behind keep the
    sentinel.  An overflowing row (more than cap): ccnt is the true count, the cap stored entries are distinct members."""
    st = state.read()
    got = cand.numpy().view(np.uint64)
    for r, w in enumerate(want):
        c = int(st["ccnt"][r])
        assert c == len(w), f"row {r}: ccnt {c}, exact set has {len(w)}"
        row = got[r, :min(c, cap)]
        if c <= cap:
            assert np.array_equal(np.sort(row), w), f"row {r}: candidate set differs ({c} entries)"
        else:
            assert len(np.unique(row)) == cap and np.isin(row, w).all(), f"row {r}: overflowing list holds duplicates or strangers"
        assert (got[r, min(c, cap):] == np.uint64(CAND_SENT)).all(), f"row {r}: slots behind the list were written"
    return st


def _biased(kind, Q, n, seed, bias):
    """-> host q, g (int8 values), exact fp32 scores, scales"""
    D, lead = _dims(kind)
    q, g, dots = _noise(kind, Q, n, seed)
    q = q.copy()
    q[:, :lead] = np.asarray(bias, np.int8).reshape(-1, 1)
    sq, sg = _scales(kind, Q, n)
    return q, g, _exact_scores(kind, dots + 2.0 * lead * np.asarray(bias, np.float64).reshape(-1, 1), sq, sg), sq, sg


def _bias_of(pattern, Q):
    if pattern == "pos":
        return np.full(Q, 3)
    if pattern == "neg":
        return np.full(Q, -3)
    return np.where(np.arange(Q) % 32 == 7, -3, 3)      # one_neg: one row of every 32-row group is negative


def _filter_pattern_case(kind, Q, n, pattern, order=None, cap=1536, col0=1000003, want_form=None):
    lib = L()
    old = ctypes.c_int(0)
    lib.pfr_get_tuning(b"match_order", ctypes.addressof(old))
    try:
        if order is not None:
            lib.pfr_set_tuning(b"match_order", order)
        knob = ctypes.c_int(0)
        lib.pfr_get_tuning(b"match_order", ctypes.addressof(knob))
        want_id, big, multi, slots = _expected_launch(kind, Q, n, knob.value)
        if want_form is not None:
            assert (big, multi) == want_form, f"shape no longer reaches the intended launch form on {_cus()} CUs"
        q, g, scores, sq, sg = _biased(kind, Q, n, 7, _bias_of("pos" if pattern == "zero" else pattern, Q))
        thr = None if pattern == "zero" else _pick_thresholds(scores)
        if pattern == "pos":
            assert (thr > 0).all()
        elif pattern == "neg":
            assert (thr < 0).all()
        elif pattern == "one_neg":
            neg = np.arange(Q) % 32 == 7
            assert (thr[neg] < 0).all() and (thr[~neg] > 0).all()
        state, tk = _threshold_state(Q, thr)
        want = O.filter_set(scores, tk, col0, False)
        if thr is not None:
            assert all(np.any(scores[r] == thr[r]) for r in range(0, Q, 2)), "even rows: the threshold is a score of the chunk"
            if pattern == "pos" and n > 4096:      # winner density: a tile above the deferred queue's capacity and one below it
                B, fqcap = (256, 512) if big else (128, 256)
                per_tile = np.zeros((_ceil(Q, B), _ceil(n, B)), np.int64)
                for r, w in enumerate(want):
                    np.add.at(per_tile[r // B], (O.unpack(w)[1] - col0) // B, 1)
                assert per_tile.max() > fqcap and ((per_tile > 0) & (per_tile <= fqcap)).any()
        cand = Guarded((Q, cap), torch.int64, CAND_SENT)
        dq, dg = _dev_rows(kind, q), _dev_rows(kind, g)
        dsq, dsg = (torch.from_numpy(sq).to(DEV), torch.from_numpy(sg).to(DEV)) if kind == "i8" else (None, None)
        got_id = _run_filter(kind, dq, dg, dsq, dsg, Q, n, col0, state, cand, cap, False)
        assert got_id == want_id, f"launch {got_id:#x}, expected {want_id:#x} from the dispatch rule"
        st = _check_candidates(state, cand, want, cap)
        assert np.array_equal(st["thrk"], tk) and st["flags"] == 0
    finally:
        lib.pfr_set_tuning(b"match_order", old.value)


@pytest.mark.parametrize("pattern", ["pos", "one_neg", "neg", "zero"])
@pytest.mark.parametrize("kind", ["f32", "bf16", "i8"])
def test_filter_128_tile_one_tile_per_workgroup(kind, pattern):
    """Q = 37, n = 300: ragged in both directions (rows past M, the last column tile partial: generic path there, fast path in the
    full tiles of the positive rows)"""
    _filter_pattern_case(kind, 37, 300, pattern, want_form=(False, False))


def _multi128_shape():
    slots = 2 * _cus()
    return 640, (slots // 5 + 3) * 128 - 7          # 5 x (slots / 5 + 3) tiles > slots.  256 CUs: n = 13433


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("pattern", ["pos", "one_neg", "neg"])
def test_filter_128_tile_several_tiles_per_workgroup(pattern, order):
    """f32; L2-blocked and linear tile order must give the same exact sets"""
    Q, n = _multi128_shape()
    _filter_pattern_case("f32", Q, n, pattern, order=order, want_form=(False, True))


def _big_shape(multi):
    """256-tile launches need ceil(Q/256) * ceil(n/256) >= 160; one tile per workgroup needs <= CUs tiles"""
    cus = _cus()
    if not multi:
        return 257, 80 * 256 - 5                   # 2 x 80 = 160 tiles (<= 256 CUs)
    return 513, (max(cus, 160) // 3 + 1) * 256 - 3   # 3 x (CUs / 3 + 1) tiles > CUs.  256 CUs: n = 22013


@pytest.mark.parametrize("pattern", ["pos", "one_neg"])
@pytest.mark.parametrize("kind", ["bf16", "i8"])
def test_filter_256_tile_one_tile_per_workgroup(kind, pattern):
    if _cus() < 160:
        pytest.fail("a 256-tile launch with one tile per workgroup needs at least 160 CUs")
    Q, n = _big_shape(False)
    _filter_pattern_case(kind, Q, n, pattern, want_form=(True, False))


@pytest.mark.parametrize("pattern", ["pos", "one_neg", "neg"])
@pytest.mark.parametrize("kind", ["bf16", "i8"])
def test_filter_256_tile_several_tiles_per_workgroup(kind, pattern):
    Q, n = _big_shape(True)
    _filter_pattern_case(kind, Q, n, pattern, want_form=(True, True))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("where", ["last", "second_to_last"])
def test_filter_drains_the_winner_queues(where, order):
    """Several tiles per workgroup (f32, 128-tile).  In the linear order workgroup 0 runs tile 0 and then tile `slots`, its last.  All
    winners of the chunk sit in ONE tile: the last one (no slot taken before the drain) or the one before (slots taken, entries written
    by the drain).  Every other gallery row is zero and every other query row has a threshold no score reaches."""
    lib = L()
    Q, n = _multi128_shape()
    col0, cap = 4096, 1536
    old = ctypes.c_int(0)
    lib.pfr_get_tuning(b"match_order", ctypes.addressof(old))
    try:
        lib.pfr_set_tuning(b"match_order", order)
        want_id, big, multi, slots = _expected_launch("f32", Q, n, order)
        assert (big, multi) == (False, True)
        tn = _ceil(n, 128)
        tile = slots if where == "last" else 0
        r0, c0 = (tile // tn) * 128, (tile % tn) * 128
        rs = np.random.RandomState(11)
        q = rs.randint(-3, 4, (Q, 64)).astype(np.int8)
        g = np.zeros((n, 64), np.int8)
        g[c0:c0 + 128] = rs.randint(-3, 4, (128, 64))
        scores = (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.float32)
        thr = np.full(Q, 1e6, np.float32)
        thr[r0:r0 + 128] = 80.0 + np.arange(128) % 5
        state, tk = _threshold_state(Q, thr)
        want = O.filter_set(scores, tk, col0, False)
        total = sum(len(w) for w in want)
        assert 32 < total <= 256, "all winners must fit the deferred queue (FQCAP = 256): none takes the immediate path"
        assert all(len(w) == 0 for w in want[:r0] + want[r0 + 128:])
        cand = Guarded((Q, cap), torch.int64, CAND_SENT)
        got_id = _run_filter("f32", _dev_rows("f32", q), _dev_rows("f32", g), None, None, Q, n, col0, state, cand, cap, False)
        assert got_id == want_id
        _check_candidates(state, cand, want, cap)
    finally:
        lib.pfr_set_tuning(b"match_order", old.value)


@pytest.mark.parametrize("pattern", ["zero", "top"])
@pytest.mark.parametrize("kind", ["f32", "bf16", "i8"])
def test_filter_exclude_self(kind, pattern):
    """Q = 300, chunk = gallery rows 90 .. 289 of a self-match (gallery row i = query row i): the diagonal enters the chunk at query
    row 90, crosses the row-tile boundaries 128 and 256 and the column-tile boundary 128 (row 218) and leaves it at row 290.  A row's own
    score is its best; it must stay out, and only it."""
    Q, n, col0, cap = 300, 200, 90, 1536
    D, lead = _dims(kind)
    rs = np.random.RandomState(5)
    q = rs.randint(-3, 4, (Q, D)).astype(np.int8)
    g = q[col0:col0 + n].copy()
    sq, sg = _scales(kind, Q, Q)
    sg = sq[col0:col0 + n].copy() if kind == "i8" else None
    scores = _exact_scores(kind, q.astype(np.float64) @ g.astype(np.float64).T, sq, sg)
    thr = None if pattern == "zero" else np.sort(scores, axis=1)[:, -6].copy()      # self is among the 5 above it
    state, tk = _threshold_state(Q, thr)
    want = O.filter_set(scores, tk, col0, True)
    loose = O.filter_set(scores, tk, col0, False)
    assert [len(a) - len(b) for a, b in zip(loose, want)] == [1 if col0 <= r < col0 + n else 0 for r in range(Q)]
    cand = Guarded((Q, cap), torch.int64, CAND_SENT)
    dsq, dsg = (torch.from_numpy(sq).to(DEV), torch.from_numpy(sg).to(DEV)) if kind == "i8" else (None, None)
    got_id = _run_filter(kind, _dev_rows(kind, q), _dev_rows(kind, g), dsq, dsg, Q, n, col0, state, cand, cap, True)
    assert got_id == _expected_launch(kind, Q, n, 1)[0]
    _check_candidates(state, cand, want, cap)


@pytest.mark.parametrize("kind", ["f32", "i8"])
def test_filter_overflow_keeps_count_and_bounds(kind):
    """cap = 64: even rows let all 300 scores in, odd rows a few.  ccnt is the true count, the 64 stored entries are distinct members,
    the neighbouring rows' slots and the guard stay intact, and pfr_topk_merge raises flag bit 1."""
    Q, n, cap, col0 = 37, 300, 64, 1000
    q, g, scores, sq, sg = _biased(kind, Q, n, 9, np.full(Q, 3))
    thr = _pick_thresholds(scores, dense_rows=0, sparse=0.03)
    thr[::2] = -1e6
    state, tk = _threshold_state(Q, thr)
    seed = state.lay.entries(state.read())
    want = O.filter_set(scores, tk, col0, False)
    assert all(len(w) == n for w in want[::2]) and all(0 < len(w) <= cap for w in want[1::2])
    cand = Guarded((Q, cap), torch.int64, CAND_SENT)
    dsq, dsg = (torch.from_numpy(sq).to(DEV), torch.from_numpy(sg).to(DEV)) if kind == "i8" else (None, None)
    _run_filter(kind, _dev_rows(kind, q), _dev_rows(kind, g), dsq, dsg, Q, n, col0, state, cand, cap, False)
    st = _check_candidates(state, cand, want, cap)
    assert st["flags"] == 0
    L().pfr_topk_merge(cand.ptr, cap, Q, 1, state.ptr, _st())
    st = state.read()
    assert st["flags"] == O.FLAG_OVERFLOW == state.flags() and not st["ccnt"].any()
    for r in range(1, Q, 2):
        e, t = O.best_entries([seed[r], want[r]], 1)
        assert np.array_equal(st["cur"][r], e) and st["thrk"][r] == t
    cand.numpy()


@pytest.mark.parametrize("kind", ["f32", "bf16", "i8"])
def test_filter_twice_merge_finish_equals_exact_topk(kind):
    """The schedule of the match with merge_every = 2: a materialised first chunk (int8: pfr_match_scores_i8, compared bit for bit,
    ld > n, padding untouched) through pfr_topk_update, two filter chunks, ONE merge, finish == the exact top-K of the whole gallery."""
    Q, K, cap = 130, 10, 1536
    sizes = [300, 300, 212]
    n = sum(sizes)
    q, g, scores, sq, sg = _biased(kind, Q, n, 13, np.where(np.arange(Q) % 3 == 0, -1, 2))
    dq, dg = _dev_rows(kind, q), _dev_rows(kind, g)
    dsq, dsg = (torch.from_numpy(sq).to(DEV), torch.from_numpy(sg).to(DEV)) if kind == "i8" else (None, None)
    state = State(Q, K)
    if kind == "i8":
        out = Guarded((Q, 304), torch.float32, F_SENT)
        L().pfr_match_scores_i8(dq.data_ptr(), dsq.data_ptr(), dg.data_ptr(), dsg.data_ptr(), Q, 300, q.shape[1], out.ptr, 304, _st())
        mat = out.numpy()
        assert np.array_equal(mat[:, :300].view(np.uint32), scores[:, :300].view(np.uint32)), "materialised int8 scores: bits differ"
        assert (mat[:, 300:] == np.float32(F_SENT)).all(), "score padding was written"
        state.update(out.view, 300, 0)
    else:
        state.update(_chunk(scores[:, :300]), 300, 0)
    seed, thr = O.topk_exact(scores[:, :300], 0, K)
    state.check(seed, thr)
    cand = Guarded((Q, cap), torch.int64, CAND_SENT)
    want = [np.zeros(0, np.uint64)] * Q
    for a, m in ((300, 300), (600, 212)):
        _run_filter(kind, dq, dg[a:], dsq, None if dsg is None else dsg[a:], Q, m, a, state, cand, cap, False)
        new = O.filter_set(scores[:, a:a + m], thr, a, False)
        want = [np.sort(np.concatenate([w, x])) for w, x in zip(want, new)]
        _check_candidates(state, cand, want, cap)
    L().pfr_topk_merge(cand.ptr, cap, Q, K, state.ptr, _st())
    whole, thr_w = O.topk_exact(scores, 0, K)
    st = state.check(whole, thr_w)
    assert not st["ccnt"].any()
    cand.numpy()


# ================================================================================================ d. pfr_topk_rescore / _cert
def _rescore(q, g, scale, cand, cand_scores, K):
    """-> (scores, idx, cert or None) as numpy, outputs poisoned and guarded"""
    rows, KC = cand.shape
    D = q.shape[1]
    dq, dg, dc = torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV), torch.from_numpy(cand.astype(np.int32)).to(DEV)
    ds = None if scale is None else torch.from_numpy(scale).to(DEV)
    sc = Guarded((rows, K), torch.float32, F_SENT)
    ix = Guarded((rows, K), torch.int32, I_SENT)
    sp = 0 if ds is None else ds.data_ptr()
    if cand_scores is None:
        L().pfr_topk_rescore(dq.data_ptr(), dg.data_ptr(), sp, rows, D, dc.data_ptr(), KC, K, sc.ptr, ix.ptr, _st())
        return sc.numpy(), ix.numpy(), None
    dcs = torch.from_numpy(cand_scores).to(DEV)
    cert = Guarded((rows, 2), torch.float32, F_SENT)
    L().pfr_topk_rescore_cert(dq.data_ptr(), dg.data_ptr(), sp, rows, D, dc.data_ptr(), dcs.data_ptr(), KC, K, sc.ptr, ix.ptr, cert.ptr, _st())
    return sc.numpy(), ix.numpy(), cert.numpy()


@pytest.mark.parametrize("D", [4, 64, 512])
@pytest.mark.parametrize("KC", [5, 16, 130, 512])
def test_rescore_exact_on_integer_rows(KC, D):
    """integer rows: exact fp32 dots (|dot| <= 9 * 512), long tie runs.  K in {1, KC}, g_scale null and a power-of-two vector; rows with
    trailing -1, -1 in the middle, -1 as the last candidate only, and no valid candidate at all."""
    rows, G, rs = 6, 700, np.random.RandomState(KC * 1000 + D)
    q = rs.randint(-3, 4, (rows, D)).astype(np.float32)
    g = rs.randint(-3, 4, (G, D)).astype(np.float32)
    cand = np.stack([rs.permutation(G)[:KC] for _ in range(rows)]).astype(np.int64)
    cand[1, KC - KC // 3 - 1:] = -1                   # trailing
    cand[2, 1:KC - 1:3] = -1                          # in the middle, last one valid
    cand[3, :] = -1                                   # nothing valid
    cand[4, KC - 1] = -1                              # only the last
    for scale in (None, (2.0 ** -(np.arange(G) % 4)).astype(np.float32)):
        _, _, _, dots = O.rescore_exact(q, g, scale, cand, None, 1)
        # selection scores: the exact score moved by a multiple of 1/8 (exact arithmetic), arbitrary where there is no candidate
        cs = (np.nan_to_num(dots, nan=3.0) + rs.randint(-16, 17, cand.shape) / 8.0).astype(np.float32)
        for K in sorted({1, KC}):
            wsc, wix, wcert, _ = O.rescore_exact(q, g, scale, cand, cs, K)
            for with_cert in (False, True):
                sc, ix, cert = _rescore(q, g, scale, cand, cs if with_cert else None, K)
                assert np.array_equal(ix, wix), (K, scale is not None)
                assert np.array_equal(sc.view(np.uint32), wsc.view(np.uint32))
                if with_cert:
                    assert np.array_equal(cert.view(np.uint32), wcert.view(np.uint32)), (cert, wcert)
                    assert np.isposinf(cert[[3, 4], 1]).all() and (K > 1 or np.isfinite(cert[[0, 2], 1]).all())


@pytest.mark.parametrize("with_scale", [False, True])
def test_rescore_real_valued_within_derived_bound(with_scale):
    """normalised random rows, D = 512, against float64: every score within topk_oracle.rescore_bound, order swaps only inside twice
    that bound, no entry skipped (tests/test_topk_oracle_host.py shows that the seed pins the order)."""
    q, g, scale, cand = O.rescore_real_case(with_scale)
    KC = cand.shape[1]
    _, _, _, dots = O.rescore_exact(q, g, scale, cand, None, KC)
    for K in (10, KC):
        sc, ix, _ = _rescore(q, g, scale, cand.astype(np.int64), None, K)
        for r in range(q.shape[0]):
            b = O.rescore_bound(q[r], g[cand[r]], None if scale is None else scale[cand[r]])
            O.check_order_within_bound(ix[r], cand[r], dots[r], b)
            pos = {int(c): i for i, c in enumerate(cand[r])}
            at = np.array([pos[int(i)] for i in ix[r]])
            err = np.abs(sc[r].astype(np.float64) - dots[r][at])
            print(f"rescore real scale={with_scale} K={K} row={r}: max err {err.max():.3e}, bound {b[at].min():.3e}")
            assert np.all(err <= b[at]), (err.max(), b[at].min())
