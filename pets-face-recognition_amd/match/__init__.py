"""Embedding match: cosine scores, running top-K, candR@K (Recall@K) — the evaluation half of the FE hot path.

Reference call sites: /root/reference/engine/controller.py:60-65,77-90,143-160 (pair scores + per-query ranking),
configs/dog_fe/fe_dogs_config.py:89-93 (`similarity_f`), generate_tsv.py:91-125 (query-vs-gallery top-100).

CUDA tensors run on the gfx950 kernels (normalise → MFMA GEMM per gallery chunk → radix-select/threshold top-K merge,
optional exact fp32 re-scoring of the candidate lists); CPU tensors use plain torch (the reference's own device
behaviour, used by the CPU plumbing config).  Ordering everywhere: score descending, ties → lower index.
"""
import collections
import ctypes

import torch

from .._hip import lib, dtype_id, PfrError
from .._hip import ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


class PreparedGallery:
    """An L2-normalised gallery kept on the device for MANY query batches (generate_tsv.py:91-125 loops over query cards; a served
    gallery answers query batch after query batch): the bf16 GEMM operand and, for the exact re-scoring, the fp32 copy.  Reuse is
    EXPLICIT — the caller builds the handle with `prepare_gallery(g)` and passes it to `cosine_topk` in place of `g`; nothing is keyed
    on tensor identity or version counters (writes through raw pointers — every kernel of this library — are invisible to them), so a
    gallery buffer that was refilled needs a new handle.  1 M x 512: 1 GB (bf16) + 2 GB (fp32).
    int8 (`compute_dtype=torch.int8`): `gn` holds the int8 rows [G, Dp] of `quantize_rows` (Dp = D rounded up to 128) and `qscale` their
    fp32 scales [G]; 1 M x 512: 0.5 GB + 4 MB (+ 2 GB fp32 with rescore)."""

    def __init__(self, gn, gn32, compute_dtype, rescore, normalized, qscale=None, dim=None):
        self.gn, self.gn32, self.gscale = gn, gn32, None
        self.qscale = qscale        # int8 only: per-row scales of the int8 rows (gscale means the inverse norms of borrowed raw rows)
        self.compute_dtype, self.rescore, self.normalized = compute_dtype, rescore, normalized
        self.shape, self.device = (gn.shape[0], gn.shape[1] if dim is None else dim), gn.device

    def __len__(self):
        return self.shape[0]


def _prep_rows(x32, T, rescore, normalize, borrow=False):
    """rows of an fp32 matrix -> (GEMM operand in T, fp32 rows for the re-scoring or None[, their per-row scale]).
    borrow=True (one-shot match): the re-scoring reads the caller's RAW rows times 1 / |row| instead of a normalised fp32 copy
    (1 M x 512: 2 GB less written); -> (operand, raw rows, inverse norms)"""
    D = x32.shape[1]
    if normalize and T == torch.bfloat16 and D % 4 == 0 and D <= 2048:
        # one pass per matrix: bf16 GEMM operand + (when re-scoring) the fp32 copy or the inverse norms
        xb = torch.empty(x32.shape, dtype=torch.bfloat16, device=x32.device)
        if borrow and rescore:
            inv = torch.empty(x32.shape[0], dtype=torch.float32, device=x32.device)
            lib.pfr_l2norm_dual(x32.data_ptr(), xb.data_ptr(), 0, inv.data_ptr(), x32.shape[0], D, 1e-12, _stream())
            return xb, x32, inv
        xf = torch.empty(x32.shape, dtype=torch.float32, device=x32.device) if rescore else None
        lib.pfr_l2norm_dual(x32.data_ptr(), xb.data_ptr(), 0 if xf is None else xf.data_ptr(), 0, x32.shape[0], D, 1e-12, _stream())
        return (xb, xf, None) if borrow else (xb, xf)
    if borrow:
        return _prep_rows(x32, T, rescore, normalize) + (None,)
    if normalize:
        xn, _, _ = ops.l2norm_fwd(x32, T)
        xf = ops.l2norm_fwd(x32, torch.float32)[0] if rescore else None
        return xn, xf
    # rows are used as given (card centroids)
    return (x32 if T == torch.float32 else ops.cast(x32, T)), x32


def quantize_rows(x, normalize=True, return_rows=False):
    """The int8 operand of the match: per row x̂ = x / max(|x|, 1e-12) (or x itself with normalize=False), m = max |x̂_i|,
    q_i = round_half_even(x̂_i · (127 / m)), scale = m / 127 (an all-zero row with scale 0 when 127 / m is +inf); the exact definition is
    at pfr_quantize_rows_i8 in include/pfr_hip.h.  x [rows, D] on the device (D % 4 == 0, D <= 2048).
    → (int8 [rows, Dp] with Dp = D rounded up to a multiple of 128, zero padded; fp32 scale [rows]) [+ the fp32 rows x̂ [rows, D]]."""
    if not x.is_cuda:
        raise PfrError("quantize_rows: the int8 operand is made on the device (gfx950)")
    x32 = x.float().contiguous()
    rows, D = x32.shape
    if D % 4 or D > 2048:
        raise PfrError(f"quantize_rows: D={D} must be a multiple of 4 and <= 2048")
    Dp = (D + 127) // 128 * 128
    q8 = torch.empty((rows, Dp), dtype=torch.int8, device=x.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x.device)
    xf = torch.empty((rows, D), dtype=torch.float32, device=x.device) if return_rows else None
    if rows:
        lib.pfr_quantize_rows_i8(x32.data_ptr(), q8.data_ptr(), Dp, sc.data_ptr(), 0 if xf is None else xf.data_ptr(), 0, rows, D,
                                 int(bool(normalize)), 1e-12, _stream())
    return (q8, sc, xf) if return_rows else (q8, sc)


def _prep_rows_i8(x32, rescore, normalize, borrow=False):
    """int8 counterpart of _prep_rows: → ((int8 rows, scales), fp32 rows for the re-scoring or None[, inverse norms of borrowed raw rows])"""
    rows, D = x32.shape
    if D % 4 or D > 2048:
        raise PfrError(f"cosine_topk(int8): D={D} must be a multiple of 4 and <= 2048")
    Dp = (D + 127) // 128 * 128
    q8 = torch.empty((rows, Dp), dtype=torch.int8, device=x32.device)
    sc = torch.empty(rows, dtype=torch.float32, device=x32.device)
    xf = inv = None
    if rescore and borrow and normalize:     # the re-scoring reads the caller's raw rows times their inverse norms (as bf16 does)
        inv = torch.empty(rows, dtype=torch.float32, device=x32.device)
    elif rescore and normalize:
        xf = torch.empty((rows, D), dtype=torch.float32, device=x32.device)
    lib.pfr_quantize_rows_i8(x32.data_ptr(), q8.data_ptr(), Dp, sc.data_ptr(), 0 if xf is None else xf.data_ptr(),
                             0 if inv is None else inv.data_ptr(), rows, D, int(bool(normalize)), 1e-12, _stream())
    if rescore and not normalize:
        xf = x32                              # rows are used as given (the scores are defined on them)
    if inv is not None:
        xf = x32
    return ((q8, sc), xf, inv) if borrow else ((q8, sc), xf)


def prepare_gallery(g, compute_dtype=torch.bfloat16, rescore=None, normalize=True):
    """Normalise a gallery once for many `cosine_topk(q, handle, k)` calls (same compute_dtype / rescore / normalize as those calls)."""
    if not g.is_cuda:
        raise PfrError("prepare_gallery: the gallery handle is a device object (CPU tensors go to cosine_topk directly)")
    T = compute_dtype
    if rescore is None:
        rescore = T != torch.float32
    if T == torch.int8:
        g32 = g.float().contiguous()
        (g8, gs), gn32 = _prep_rows_i8(g32, rescore, normalize)
        if gn32 is not None and gn32.data_ptr() == g32.data_ptr() and g32.data_ptr() == g.data_ptr():
            gn32 = gn32.clone()     # (normalize=False: the handle owns its rows, the caller may refill the buffer)
        return PreparedGallery(g8, gn32, T, bool(rescore), bool(normalize), qscale=gs, dim=g.shape[1])
    gn, gn32 = _prep_rows(g.float().contiguous(), T, rescore, normalize)
    return PreparedGallery(gn, gn32, T, bool(rescore), bool(normalize))


#: default candidate slack of the certified int8 selection (compute_dtype=torch.int8), measured on the GPU: profiles/match_int8.txt
_I8_SLACK = 128

#: what the last certified `cosine_topk` call on this process did: queries, candidates per query, the largest selection-score error measured,
#: queries re-matched with a wider candidate list, queries re-matched exactly in fp32
last_match_stats = {}
_CERT_SAFETY = 2.0     # a query is certified when its gap is at least this many times the LARGEST selection error measured on any candidate


def cosine_topk(q, g, k, compute_dtype=torch.bfloat16, chunk=131072, exclude_self=False, rescore=None, slack=None,
                normalize=True, fused_filter=True, merge_every=2, seed_cols="auto", certify=None):
    """Top-k gallery rows per query by cosine similarity.  q [Q,D], g [G,D] (any scale; rows are L2-normalised here) or a
    `prepare_gallery(g)` handle (the gallery's normalisation is then not repeated per call).
    → (scores [Q,k] fp32 cosine, idx [Q,k] int32, −1 / −inf padded when fewer than k exist).
    exclude_self: q and g are the same set, the diagonal is skipped (the reference excludes the query itself).
    rescore (default: True for bf16): candidates are selected on bf16-input scores with `slack` extra entries, then
    re-scored exactly in fp32 and re-sorted, so that the final order is the fp32 order.
    certify (default: with rescore): the selection is CHECKED instead of trusted.  Every gallery row outside a query's candidate list has a
    selection score of at most the list's last one, so it can belong to the exact top-k only if its selection error exceeds
    gap = (k-th best fp32 score) − (last selection score).  The re-scoring measures the selection error on every candidate (Q x kc samples of
    the same data); a query whose gap is below twice the largest error seen is matched again with a four times wider slack, and in fp32
    (exactly the reference's arithmetic) if it fails again.  With the check the default slack is max(28, k / 4) instead of max(28, 1.5 k):
    1.5 ms less at 10 k x 1 M x 512 (13.5 instead of 15.0 ms on the box that measured it), same results; `last_match_stats` records what the
    check did.
    compute_dtype=torch.int8: the selection runs on per-row scalar-quantised rows (`quantize_rows`) on the int8 MFMA; the selection score is
    ((float) Σ q_a,i q_b,i · s_a) · s_b (include/pfr_hip.h).  rescore and certify default to True and give the same exact top-k as bf16; the
    int8 selection error is about 4x the bf16 one, so the default slack is wider: max(_I8_SLACK, k / 4).  The lists hold at most 512 entries:
    from k = 512 - _I8_SLACK on the slack shrinks, at k = 512 there is none and every query that is not certified is re-matched in fp32.
    rescore=False returns the top-k by the selection score itself (approximate; a 1 M x 512 handle then holds 0.5 GB + 4 MB)."""
    prepared = g if isinstance(g, PreparedGallery) else None
    if not q.is_cuda:
        if prepared is not None:
            raise PfrError("cosine_topk: a PreparedGallery is a device object; pass the CPU gallery tensor itself")
        return _cosine_topk_torch(q, g, k, exclude_self, normalize)
    Q, D = q.shape
    G = g.shape[0]
    T = compute_dtype
    if rescore is None:
        rescore = T != torch.float32
    if certify is None:
        certify = bool(rescore)
    certify = bool(certify and rescore)
    if prepared is not None and (prepared.compute_dtype != T or prepared.rescore != bool(rescore) or prepared.normalized != bool(normalize)
                                 or prepared.shape[1] != D or prepared.device != q.device):
        raise PfrError("cosine_topk: the PreparedGallery was built for other settings "
                       f"({prepared.compute_dtype}, rescore={prepared.rescore}, normalize={prepared.normalized}, D={prepared.shape[1]}, {prepared.device})")
    if k > 512:
        # the running lists of the top-K kernels hold at most 512 entries per query (pfr_match.hip); silently returning
        # fewer columns, or re-scoring past the candidate list, would be wrong answers
        raise PfrError(f"cosine_topk: k={k} exceeds the 512-entry running list of the gfx950 top-K kernels")
    i8 = T == torch.int8
    if slack is None:
        if i8:
            slack = max(_I8_SLACK, (k + 3) // 4) if certify else max(_I8_SLACK, 2 * k)
        else:
            slack = max(28, (k + 3) // 4) if certify else max(28, k // 2 + k)
    kc = max(k, min(512, k + slack)) if rescore else k
    q32 = q.float().contiguous()
    qn, qn32 = _prep_rows_i8(q32, rescore, normalize) if i8 else _prep_rows(q32, T, rescore, normalize)
    if prepared is not None:
        gn, gn32, gscale = prepared.gn, prepared.gn32, None      # (a handle owns a normalised copy: the caller may refill its buffer)
        if i8:
            gn = (gn, prepared.qscale)
    elif i8:
        gn, gn32, gscale = _prep_rows_i8(g.float().contiguous(), rescore, normalize, borrow=True)
    else:
        gn, gn32, gscale = _prep_rows(g.float().contiguous(), T, rescore, normalize, borrow=True)
    sched = dict(chunk=chunk, exclude_self=exclude_self, fused_filter=fused_filter, merge_every=merge_every, seed_cols=seed_cols)
    if not rescore:
        return _topk_pass(qn, None, gn, None, None, k, k, T, False, **sched)[:2]
    sc, idx, cert = _topk_pass(qn, qn32, gn, gn32, gscale, k, kc, T, certify, **sched)
    if not certify:
        return sc, idx
    # ---- the certificate (see the docstring).  One host synchronisation; the re-matches below run only for the queries that fail.
    eps = cert[:, 0].max()
    bad = (cert[:, 1] < _CERT_SAFETY * eps).nonzero().flatten()
    stats = {"queries": Q, "candidates": kc, "max_selection_error": float(eps), "widened": 0, "exact": 0}
    if bad.numel():
        kc2 = max(k, min(512, k + 4 * slack))
        if kc2 > kc:
            # (with exclude_self the fused filter identifies "self" by row == column: the whole set is matched again, not a subset)
            rows = None if exclude_self else bad
            stats["widened"] = Q if rows is None else int(rows.numel())
            s2, i2, c2 = _topk_pass(qn if rows is None else _take_rows(qn, rows), qn32 if rows is None else qn32[rows], gn, gn32, gscale, k, kc2,
                                    T, True, **sched)
            eps = torch.maximum(eps, c2[:, 0].max())
            still = c2[:, 1] < _CERT_SAFETY * eps
            if rows is None:
                sc, idx, bad = s2, i2, still.nonzero().flatten()
            else:
                sc[rows], idx[rows] = s2, i2
                bad = rows[still]
        if bad.numel():
            # fp32 scores of every pair for these queries: the reference's own arithmetic (utils/calc_scores.py: torch.mm on fp32)
            rows = None if exclude_self else bad
            stats["exact"] = Q if rows is None else int(rows.numel())
            if gscale is None:      # gn32 holds the rows the scores are defined on (normalised, or as given with normalize=False)
                s3, i3 = cosine_topk(qn32 if rows is None else qn32[rows], gn32, k, compute_dtype=torch.float32, chunk=chunk,
                                     exclude_self=exclude_self, normalize=False)
            else:                   # gn32 = the caller's raw rows
                s3, i3 = cosine_topk(q32 if rows is None else q32[rows], gn32, k, compute_dtype=torch.float32, chunk=chunk,
                                     exclude_self=exclude_self, normalize=normalize)
            if rows is None:
                sc, idx = s3, i3
            else:
                sc[rows], idx[rows] = s3, i3
    stats["max_selection_error"] = float(eps)
    last_match_stats.clear()
    last_match_stats.update(stats)
    return sc, idx


def _take_rows(qn, rows):
    return (qn[0][rows], qn[1][rows]) if isinstance(qn, tuple) else qn[rows]


def _topk_pass(qn, qn32, gn, gn32, gscale, k, kc, T, certify, chunk=131072, exclude_self=False, fused_filter=True, merge_every=2,
               seed_cols="auto"):
    """One pass of prepared query rows over the prepared gallery: running top-kc lists per query (selection scores in T), then — with
    qn32 / gn32 — the exact fp32 re-scoring that keeps k.  → (scores [Q,k], idx [Q,k], certificate [Q,2] or None).
    int8 (T = torch.int8): qn and gn are (int8 rows [*, Dp], scales) pairs of quantize_rows; qn32 / gn32 keep the original D."""
    i8 = T == torch.int8
    (qn, qs8), (gn, gs8) = (qn, gn) if i8 else ((qn, None), (gn, None))
    Q, D = qn.shape
    G = gn.shape[0]
    rescore = qn32 is not None
    chunk = min(chunk, G)
    state = torch.empty(lib.pfr_topk_state_bytes(Q, kc), dtype=torch.uint8, device=qn.device)
    self_idx = torch.arange(Q, dtype=torch.int32, device=qn.device) if exclude_self else None
    # Chunks after the first (every running list is full by then) use the GEMM with the top-K filter in its epilogue: the
    # fp32 score chunk is never written.  A candidate-list overflow (adversarially ordered gallery) is flagged on the
    # device and the whole match is redone on the unfused path.
    fused = fused_filter and G > chunk and chunk >= kc + 1 and (i8 or D % (64 if T == torch.bfloat16 else 32) == 0)
    cap = 1536
    cand = torch.empty((Q, cap), dtype=torch.int64, device=qn.device) if fused else None
    sbuf = None
    while True:
        lib.pfr_topk_reset(state.data_ptr(), Q, kc, _stream())
        # gallery segments (first column, columns, filter fused into the GEMM?): the first chunk goes through a materialised fp32 score
        # chunk (its running lists start empty), every later one through the GEMM whose epilogue is the top-K filter.
        # (Round 4 measured a seeded variant — an 8 k-column unfused seed segment, then growing fused segments of the first chunk too:
        #  same results, 20.8 / 19.3 / 18.7 ms for seeds of 8 k / 16 k / 32 k columns against 18.5 ms: the early segments carry several times
        #  the candidates per query and their merges cost more than the unfused first chunk they replace; profiles/r04_match_seed_ab.txt.)
        segs = [(c0, min(chunk, G - c0), bool(fused and c0 > 0)) for c0 in range(0, G, chunk)]
        if seed_cols == "auto":     # (a seed pays once the gallery is several chunks long)
            # (round 6, tools/match_sched_ab.py with the certified 128-entry lists: 131 072-column chunks after a 16 384-column seed 13.4 ms,
            #  65 536 / 32 768 — the round-5 schedule — 13.8, 65 536 / 16 384 13.4-13.7, 262 144 / 32 768 13.7)
            seed_cols = 16384 if (chunk >= 65536 and G >= 262144) else None
        if fused and seed_cols and kc + 1 <= seed_cols < chunk:
            # round 5 (tools/match_seed_ab.py, profiles/r05_ab.txt): an unfused seed of `seed_cols` columns, then fused segments that double
            # up to `chunk`, each of the early ones merged at once (their thresholds are loose).  Round 4 had measured this form SLOWER
            # (20.8 / 19.3 / 18.7 ms for seeds of 8 k / 16 k / 32 k against 18.5): the per-winner atomics of the filter epilogue made the
            # candidate-rich early segments expensive; with the counted epilogue it is 15.2 against 15.5 ms, same results.
            segs, c0, n = [(0, seed_cols, False)], seed_cols, seed_cols
            while c0 < G:
                n = min(max(n, seed_cols) if c0 + n <= chunk else chunk, G - c0)
                segs.append((c0, n, True))
                c0 += n
                n = min(2 * n, chunk)
        ld = (max(n for _, n, f in segs if not f) + 3) // 4 * 4
        if sbuf is None or sbuf.shape[-1] < ld:
            sbuf = torch.empty((Q, 1, 1, ld), dtype=torch.float32, device=qn.device)
        ld = sbuf.shape[-1]
        # the candidate lists of TWO fused chunks are folded into the running lists by one merge (expected candidates per query for two
        # chunks: <= 2 * kc, cap = 1536; an overflow is flagged and the match redone unfused): 18.4 -> 17.9 ms at 10 k x 1 M, same results;
        # every 3 / 4 chunks: 18.3 / 18.7 (the stale threshold lets more candidates through the filter epilogue)
        pending = 0
        for si, (c0, n, seg_fused) in enumerate(segs):
            if seg_fused:
                if i8:
                    lib.pfr_match_scores_filter_i8(qn.data_ptr(), qs8.data_ptr(), gn[c0].data_ptr(), gs8[c0].data_ptr(), Q, n, D, c0, kc,
                                                   state.data_ptr(), cand.data_ptr(), cap, int(exclude_self), _stream())
                else:
                    lib.pfr_match_scores_filter(qn.data_ptr(), gn[c0:c0 + n].data_ptr(), dtype_id(T), Q, n, D, c0, kc, state.data_ptr(),
                                                cand.data_ptr(), cap, int(exclude_self), _stream())
                pending += 1
                if pending >= merge_every or si + 1 == len(segs) or (seed_cols and c0 < 4 * chunk):
                    lib.pfr_topk_merge(cand.data_ptr(), cap, Q, kc, state.data_ptr(), _stream())
                    pending = 0
                continue
            if i8:
                lib.pfr_match_scores_i8(qn.data_ptr(), qs8.data_ptr(), gn[c0].data_ptr(), gs8[c0].data_ptr(), Q, n, D, sbuf.data_ptr(), ld, _stream())
            else:
                ops.conv2d_fwd(qn.view(Q, 1, 1, D), gn[c0:c0 + n].view(n, 1, 1, D), out=sbuf)
            lib.pfr_topk_update(sbuf.data_ptr(), Q, ld, n, c0, kc, state.data_ptr(), 0 if self_idx is None else self_idx.data_ptr(),
                                _stream())
        if not fused:
            break
        flag = ctypes.c_int(0)
        lib.pfr_topk_flags(state.data_ptr(), Q, kc, ctypes.addressof(flag), _stream())
        if not (flag.value & 2):
            break
        fused = False   # candidate buffer overflow: redo without the fused filter
    sc = torch.empty((Q, kc), dtype=torch.float32, device=qn.device)
    idx = torch.empty((Q, kc), dtype=torch.int32, device=qn.device)
    lib.pfr_topk_finish(state.data_ptr(), Q, kc, sc.data_ptr(), idx.data_ptr(), _stream())
    if rescore:
        sc2 = torch.empty((Q, k), dtype=torch.float32, device=qn.device)
        idx2 = torch.empty((Q, k), dtype=torch.int32, device=qn.device)
        gs = 0 if gscale is None else gscale.data_ptr()
        D32 = qn32.shape[1]
        if certify:
            cert = torch.empty((Q, 2), dtype=torch.float32, device=qn.device)
            lib.pfr_topk_rescore_cert(qn32.data_ptr(), gn32.data_ptr(), gs, Q, D32, idx.data_ptr(), sc.data_ptr(), kc, k,
                                      sc2.data_ptr(), idx2.data_ptr(), cert.data_ptr(), _stream())
            return sc2, idx2, cert
        lib.pfr_topk_rescore(qn32.data_ptr(), gn32.data_ptr(), gs, Q, D32, idx.data_ptr(), kc, k, sc2.data_ptr(), idx2.data_ptr(), _stream())
        return sc2, idx2, None
    return sc[:, :k].contiguous(), idx[:, :k].contiguous(), None


def _cosine_topk_torch(q, g, k, exclude_self, normalize=True):
    qn = q / q.norm(dim=1, keepdim=True).clamp_min(1e-8) if normalize else q
    gn = g / g.norm(dim=1, keepdim=True).clamp_min(1e-8) if normalize else g
    sc = qn @ gn.t()
    if exclude_self:
        sc.fill_diagonal_(-float("inf"))
    kk = min(k, sc.shape[1] - (1 if exclude_self else 0))
    order = torch.argsort(sc, dim=1, descending=True, stable=True)[:, :kk]
    return torch.gather(sc, 1, order), order.int()


def recall_at_k(emb, classes, ks=(10, 100), compute_dtype=torch.float32, rerank=None):
    """candR@K of the reference's validation protocol (controller.py:77-90): every embedding queries all the OTHERS;
    a hit at K = some same-class item among the K best; denominator = queries that have a same-class other.
    rerank: None, or a dict of keyword arguments of `match.rerank` (k1, k2, lambda_value, candidates): the K best are then taken from the
    k-reciprocal re-ranked order instead of the cosine order.
    → {k: [hits, denom]}"""
    kmax = min(max(ks), emb.shape[0] - 1)
    if rerank is None:
        _, idx = cosine_topk(emb, emb, kmax, compute_dtype=compute_dtype, exclude_self=True)
    else:
        _, idx = _rerank(emb, kmax, compute_dtype=compute_dtype, **dict(rerank))
    idx = idx.long()
    cls = classes.to(idx.device)
    valid = idx >= 0
    same = (cls[idx.clamp_min(0)] == cls[:, None]) & valid
    counts = torch.bincount(cls - cls.min())
    has = counts[cls - cls.min()] > 1
    out = {}
    for k in ks:
        out[k] = [int((same[:, :k].any(dim=1) & has).sum().item()), int(has.sum().item())]
    return out


def pair_similarity(emb, idx_a, idx_b, eps=1e-8):
    """(cos(emb[a], emb[b]) + 1) / 2 for index pairs — `similarity_f` over `pair_generator.corrected_indices`."""
    ia = torch.as_tensor(idx_a, dtype=torch.int64, device=emb.device).contiguous()
    ib = torch.as_tensor(idx_b, dtype=torch.int64, device=emb.device).contiguous()
    if not emb.is_cuda:
        # CPU tensors: the reference's own call (fe_dogs_config.py:93), bit for bit
        return (torch.nn.functional.cosine_similarity(emb[ia], emb[ib], eps=eps) + 1) / 2
    if ia.numel() and (int(torch.stack([ia.min(), ib.min()]).min()) < 0 or int(torch.stack([ia.max(), ib.max()]).max()) >= emb.shape[0]):
        # the torch indexing of the reference raises here; a device gather would read outside the embedding matrix
        raise IndexError(f"pair index out of range for {emb.shape[0]} embeddings (evaluation truncated by limit_val_batches?)")
    e = emb.float().contiguous()
    out = torch.empty(ia.numel(), dtype=torch.float32, device=emb.device)
    lib.pfr_pair_similarity(e.data_ptr(), e.shape[1], ia.data_ptr(), ib.data_ptr(), ia.numel(), float(eps), out.data_ptr(), _stream())
    return out


def embedding_quality(emb):
    """fp32 [N]: the length |emb_i| of every raw embedding, the per-photo quality score of a MagFace-trained extractor (losses/
    large_margin.py MagFaceProduct).  CUDA rows: the reciprocal of the inverse norms the match's row normalisation writes
    (pfr_l2norm_fwd's inv_norm, so the score is the |x| the training head saw); CPU rows: torch's norm."""
    if emb.dim() != 2:
        raise ValueError(f"embedding_quality: expected [N, D] embeddings, got {tuple(emb.shape)}")
    e = emb.float().contiguous()
    if not e.is_cuda or e.shape[0] == 0:
        return e.norm(dim=1)
    return ops.l2norm_fwd(e, torch.bfloat16)[2].reciprocal()


def quality_report(emb, scores, pair_labels, idx_a, idx_b):
    """{'Quality mean norm', 'Quality AUC'} of validation embeddings and their scored pairs.  'Quality AUC': over the GENUINE pairs
    (pair_labels == 1), the ROC AUC of "the pair's score is above the genuine pairs' median" against the pair's quality min(|a|, |b|),
    i.e. the probability that a high-scoring genuine pair has the higher smaller-norm than a low-scoring one (0.5: the length says
    nothing about which genuine pairs match well; NaN with fewer than two genuine pairs or constant scores).  Host arithmetic."""
    q = embedding_quality(emb).double().cpu()
    out = {'Quality mean norm': float(q.mean()) if q.numel() else float('nan'), 'Quality AUC': float('nan')}
    lab = torch.as_tensor(pair_labels).cpu().reshape(-1) == 1
    ia = torch.as_tensor(idx_a, dtype=torch.int64)[lab]
    ib = torch.as_tensor(idx_b, dtype=torch.int64)[lab]
    s = torch.as_tensor(scores).detach().double().cpu().reshape(-1)[lab]
    if s.numel() < 2:
        return out
    pq = torch.minimum(q[ia], q[ib])
    high = s > s.median()
    n1, n0 = int(high.sum()), int((~high).sum())
    if n1 == 0 or n0 == 0:
        return out
    # Mann-Whitney U of the qualities, ties counted half
    d = pq[high][:, None] - pq[~high][None, :]
    out['Quality AUC'] = float(((d > 0).double().sum() + 0.5 * (d == 0).double().sum()) / (n1 * n0))
    return out


def card_centroids(emb, seg, compute_dtype=torch.float32):
    """Mean of the L2-normalised photo embeddings per card.  emb [P, D]; seg: int64 [ncards+1] row offsets."""
    seg = torch.as_tensor(seg, dtype=torch.int64, device=emb.device).contiguous()
    n = seg.numel() - 1
    if not emb.is_cuda:
        e = emb.float() / emb.float().norm(dim=1, keepdim=True).clamp_min(1e-8)
        return torch.stack([e[seg[i]:seg[i + 1]].mean(0) if seg[i + 1] > seg[i] else torch.zeros(e.shape[1]) for i in range(n)])
    e = emb.float().contiguous()
    out = torch.empty((n, e.shape[1]), dtype=torch.float32, device=emb.device)
    lib.pfr_card_centroids(e.data_ptr(), seg.data_ptr(), n, e.shape[1], 1e-8, out.data_ptr(), 0, 0, _stream())
    return out


#: photo rows of one tile of the max-strategy kernel: a card with more photos is refused (pfr_card_tiles, include/pfr_hip.h)
CARD_MAX_PHOTOS = 128
_STRATEGIES = ("mean", "max")


def _check_strategy(strategy, who):
    if strategy not in _STRATEGIES:
        raise PfrError(f"{who}: unknown strategy {strategy!r}, expected one of {_STRATEGIES}")


def _card_seg(seg, who):
    """int64 [ncards+1] row offsets on the host, checked: non-decreasing, no card above CARD_MAX_PHOTOS photos"""
    seg = torch.as_tensor(seg, dtype=torch.int64).cpu().contiguous()
    if seg.dim() != 1 or seg.numel() < 1:
        raise PfrError(f"{who}: seg must hold ncards+1 row offsets")
    n = seg[1:] - seg[:-1]
    if n.numel() and int(n.min()) < 0:
        raise PfrError(f"{who}: row offsets decrease at card {int((n < 0).nonzero()[0])}")
    if n.numel() and int(n.max()) > CARD_MAX_PHOTOS:
        c = int((n > CARD_MAX_PHOTOS).nonzero()[0])
        raise PfrError(f"{who}: card {c} has {int(n[c])} photos, the max strategy takes at most {CARD_MAX_PHOTOS} per card")
    return seg


def card_tiles(seg):
    """The tile table of pfr_card_tiles (include/pfr_hip.h) for row offsets seg [ncards+1]: whole cards packed greedily into tiles of at
    most 128 photo rows → int32 [ntiles, 4] host records (first card, card count, first row, row count).  Host arithmetic, no device."""
    seg = torch.as_tensor(seg, dtype=torch.int64).cpu().contiguous()
    if seg.dim() != 1 or seg.numel() < 1:
        raise PfrError("card_tiles: seg must hold ncards+1 row offsets")
    n = seg.numel() - 1
    nt = lib.pfr_card_tiles(seg.data_ptr(), n, 0, 0)                   # size query, then fill
    tiles = torch.empty((max(int(nt), 0), 4), dtype=torch.int32)
    if nt > 0:
        nt = lib.pfr_card_tiles(seg.data_ptr(), n, tiles.data_ptr(), int(nt))
    if nt < 0:
        raise PfrError(f"pfr_card_tiles failed (rc={int(nt)}): {lib.pfr_last_error().decode()}")
    return tiles


class _CardSide:
    """one side (query or gallery cards) of the max-strategy kernels on the device: GEMM operand, fp32 rows, offsets and tile table"""

    def __init__(self, emb, seg, T, dev, rescore, who):
        self.seg_h = _card_seg(seg, who)
        self.ncards = self.seg_h.numel() - 1
        x32 = emb.to(dev).float().contiguous()
        if x32.dim() != 2 or x32.shape[0] < int(self.seg_h[-1]):
            raise PfrError(f"{who}: emb must be [P, D] with P >= seg[-1] photo rows")
        self.P, self.D = x32.shape
        if self.P:
            xn, _ = _prep_rows(x32, T, False, True)
            # the fp32 rows of the re-scoring are the fp32 path's own operand rows (the same normalising kernel), so that the scores
            # card_match returns with bf16 are bit for bit the ones it returns with fp32
            xf = None if not rescore else (xn if T == torch.float32 else _prep_rows(x32, torch.float32, False, True)[0])
        else:
            xn, xf = x32.to(T), (x32 if rescore else None)
        self.op = _pad_cols(xn.contiguous(), 32 if T == torch.float32 else 64)
        self.x32 = None if xf is None else _pad_cols(xf.contiguous(), 4)
        self.tiles_h = card_tiles(self.seg_h)
        self.first = self.tiles_h[:, 0].long().contiguous()     # first card of every tile (ascending)
        self.seg = self.seg_h.to(dev)
        self.tiles = self.tiles_h.to(dev)

    def tile_range(self, c0, n):
        """tiles that hold the cards [c0, c0 + n)"""
        t0 = int(torch.searchsorted(self.first, torch.tensor(c0), right=True)) - 1
        t1 = int(torch.searchsorted(self.first, torch.tensor(c0 + n - 1), right=True))
        return max(t0, 0), t1


def _card_max_chunk(qs, gs, T, c0, n, out, ld):
    """out [Q][ld] (n valid columns) = max dots of every query card against the gallery cards [c0, c0 + n)"""
    if qs.P == 0 or gs.P == 0:          # no photo on one side: every pair is −inf (and there may be no D to speak of)
        out.view(-1, ld)[:, :n] = -float("inf")
        return
    t0, t1 = gs.tile_range(c0, n)
    lib.pfr_card_max_scores(qs.op.data_ptr(), qs.seg.data_ptr(), qs.tiles.data_ptr(), qs.tiles_h.shape[0], qs.P, qs.ncards,
                            gs.op.data_ptr(), gs.seg.data_ptr(), gs.tiles.data_ptr() + 16 * t0, t1 - t0, gs.P, dtype_id(T), qs.op.shape[1],
                            c0, n, out.data_ptr(), ld, _stream())


def _card_max_dtype(compute_dtype, who):
    if compute_dtype not in (torch.float32, torch.bfloat16):
        raise PfrError(f"{who}: compute_dtype must be torch.float32 or torch.bfloat16")


def card_max_scores(q_emb, q_seg, g_emb, g_seg, compute_dtype=torch.float32):
    """Max-strategy card scores before the (x + 1) / 2 map (generate_tsv.py:81-88): → fp32 [Q, G], element (i, j) = the largest dot product
    of a unit-normalised photo row of query card i with one of gallery card j; −inf when either card has no photos.
    q_emb [Pq, D], g_emb [Pg, D] photo embeddings (any scale), q_seg [Q+1], g_seg [G+1] row offsets; at most CARD_MAX_PHOTOS photos per card.
    CUDA tensors: ONE pfr_card_max_scores launch — the photo GEMM in compute_dtype with a segmented-max epilogue, the photo x photo score
    matrix is never written.  CPU tensors: chunked fp32 matmul with the same definition."""
    _card_max_dtype(compute_dtype, "card_max_scores")
    if q_emb.dim() != 2 or g_emb.dim() != 2 or (q_emb.shape[0] and g_emb.shape[0] and q_emb.shape[1] != g_emb.shape[1]):
        raise PfrError("card_max_scores: q_emb [Pq, D] and g_emb [Pg, D]")
    if not q_emb.is_cuda:
        return _card_max_scores_torch(q_emb, _card_seg(q_seg, "card_max_scores"), g_emb, _card_seg(g_seg, "card_max_scores"))
    dev = q_emb.device
    qs = _CardSide(q_emb, q_seg, compute_dtype, dev, False, "card_max_scores")
    gs = _CardSide(g_emb, g_seg, compute_dtype, dev, False, "card_max_scores")
    Q, G = qs.ncards, gs.ncards
    ld = (G + 3) // 4 * 4
    out = torch.empty((Q, ld), dtype=torch.float32, device=dev)
    if Q and G:
        _card_max_chunk(qs, gs, compute_dtype, 0, G, out, ld)
    return out[:, :G] if ld == G else out[:, :G].contiguous()


def _card_max_scores_torch(q_emb, q_seg, g_emb, g_seg, chunk=2048):
    """CPU form of card_max_scores: photo scores of `chunk` query rows at a time, max over the columns of every gallery card, then over
    the rows of every query card"""
    unit = lambda x: x.float() / x.float().norm(dim=1, keepdim=True).clamp_min(1e-12)
    Q, G = q_seg.numel() - 1, g_seg.numel() - 1
    out = torch.full((Q, G), -float("inf"))
    Pq, Pg = int(q_seg[-1]), int(g_seg[-1])
    if Q == 0 or G == 0 or Pq == 0 or Pg == 0:
        return out
    q, g = unit(q_emb[:Pq]), unit(g_emb[:Pg])
    qcard = torch.repeat_interleave(torch.arange(Q), q_seg[1:] - q_seg[:-1])
    gcard = torch.repeat_interleave(torch.arange(G), g_seg[1:] - g_seg[:-1])
    base = int(q_seg[0]), int(g_seg[0])
    q, g = q[base[0]:], g[base[1]:]
    for r0 in range(0, q.shape[0], chunk):
        s = q[r0:r0 + chunk] @ g.t()
        cols = torch.full((s.shape[0], G), -float("inf")).scatter_reduce_(1, gcard[None, :].expand(s.shape[0], -1), s, "amax")
        out.scatter_reduce_(0, qcard[r0:r0 + chunk, None].expand(-1, G), cols, "amax")
    return out


def _max_scores_to_similarity(dots):
    """(x + 1) / 2 clamped at 0; a pair without photos (−inf) stays −inf"""
    return torch.where(torch.isinf(dots) & (dots < 0), dots, ((dots + 1) / 2).clamp_min(0))


def _card_match_max(q_emb, q_seg, g_emb, g_seg, k, T, chunk):
    _card_max_dtype(T, "card_match")
    if not q_emb.is_cuda:
        dots = card_max_scores(q_emb, q_seg, g_emb, g_seg)
        kk = min(k, dots.shape[1])
        order = torch.argsort(dots, dim=1, descending=True, stable=True)[:, :kk]
        top = _max_scores_to_similarity(torch.gather(dots, 1, order))
        sc = torch.full((dots.shape[0], k), -float("inf"))          # [Q, k] as on the device: −inf / −1 past the candidates
        idx = torch.full((dots.shape[0], k), -1, dtype=torch.int32)
        sc[:, :kk] = top
        idx[:, :kk] = torch.where(torch.isinf(top), torch.full_like(order, -1), order).int()
        return sc, idx
    if k > 512:
        raise PfrError(f"card_match: k={k} exceeds the 512-entry running list of the gfx950 top-K kernels")
    dev = q_emb.device
    rescore = T != torch.float32
    kc = min(512, k + max(28, k + k // 2)) if rescore else k
    qs = _CardSide(q_emb, q_seg, T, dev, rescore, "card_match")
    gs = _CardSide(g_emb, g_seg, T, dev, rescore, "card_match")
    Q, G = qs.ncards, gs.ncards
    sc = torch.full((Q, k), -float("inf"), dtype=torch.float32, device=dev)
    idx = torch.full((Q, k), -1, dtype=torch.int32, device=dev)
    if Q == 0 or G == 0:
        return sc, idx
    chunk = min(chunk, G)
    ld = (chunk + 3) // 4 * 4
    sbuf = torch.empty((Q, ld), dtype=torch.float32, device=dev)
    state = torch.empty(lib.pfr_topk_state_bytes(Q, kc), dtype=torch.uint8, device=dev)
    lib.pfr_topk_reset(state.data_ptr(), Q, kc, _stream())
    for c0 in range(0, G, chunk):
        n = min(chunk, G - c0)
        _card_max_chunk(qs, gs, T, c0, n, sbuf, ld)
        lib.pfr_topk_update(sbuf.data_ptr(), Q, ld, n, c0, kc, state.data_ptr(), 0, _stream())
    dots = torch.empty((Q, kc), dtype=torch.float32, device=dev)
    cand = torch.empty((Q, kc), dtype=torch.int32, device=dev)
    lib.pfr_topk_finish(state.data_ptr(), Q, kc, dots.data_ptr(), cand.data_ptr(), _stream())
    if rescore:
        # exact fp32 maxima of the candidates, then score descending with ties to the lower card index
        lib.pfr_card_max_rescore(qs.x32.data_ptr(), qs.seg.data_ptr(), Q, gs.x32.data_ptr(), gs.seg.data_ptr(), G, qs.x32.shape[1],
                                 cand.data_ptr(), kc, dots.data_ptr(), _stream())
        by_idx = torch.argsort(torch.where(cand >= 0, cand, torch.full_like(cand, 2 ** 31 - 1)), dim=1, stable=True)
        dots, cand = torch.gather(dots, 1, by_idx), torch.gather(cand, 1, by_idx)
        order = torch.argsort(dots, dim=1, descending=True, stable=True)
        dots, cand = torch.gather(dots, 1, order), torch.gather(cand, 1, order)
    kk = min(k, kc)
    sc[:, :kk] = _max_scores_to_similarity(dots[:, :kk])
    idx[:, :kk] = torch.where(torch.isinf(sc[:, :kk]), torch.full_like(cand[:, :kk], -1), cand[:, :kk])
    return sc, idx


def card_match(q_emb, q_seg, g_emb, g_seg, k=100, compute_dtype=torch.bfloat16, strategy="mean", chunk=131072):
    """Card-vs-card ranking of the reference's inference pipeline (generate_tsv.py:71-88, 91-125, one modality); → (scores [Q,k],
    idx [Q,k]), best first.
    strategy='mean' (generate_tsv.py:71-78): score(card_q, card_g) = clamp(mean over photo pairs of (cos+1)/2, min=0).  The mean over the
    photo cross product equals (⟨centroid_q, centroid_g⟩ + 1)/2, so this is ONE GEMM of card centroids with the running top-k.
    strategy='max' (generate_tsv.py:81-88): score = clamp((maxdot + 1) / 2, min=0) with maxdot the best photo pair's cosine
    (`card_max_scores`).  (x + 1) / 2 is monotone under rounding, so this is the reference's max over pairs of (cos+1)/2; the clamp differs
    from the reference (which does not clamp the max) only where rounding puts a cosine below −1.  A gallery card without photos — or
    every card, for a query card without photos — is no candidate: −inf / −1 at the end of the list.  On the device pfr_card_max_scores
    runs per chunk of `chunk` gallery cards into the running top-k (k <= 512).  torch.float32 is exact.  torch.bfloat16 selects
    kc = min(512, k + max(28, k + k // 2)) cards on bf16-input scores, re-scores them exactly in fp32 (pfr_card_max_rescore), re-sorts with
    ties to the lower index and keeps k: the returned scores are fp32 scores, but the selection is NOT certified — unlike `cosine_topk`,
    nothing checks that no card outside the kc candidates belongs to the exact top k."""
    _check_strategy(strategy, "card_match")
    if strategy == "max":
        return _card_match_max(q_emb, q_seg, g_emb, g_seg, k, compute_dtype, chunk)
    qc = card_centroids(q_emb, q_seg)
    gc = card_centroids(g_emb, g_seg)
    dots, idx = cosine_topk(qc, gc, k, compute_dtype=compute_dtype, normalize=False)
    return ((dots + 1) / 2).clamp_min(0), idx


FUSION_THRESHOLDS = (0.9069641, 0.985643)   # generate_tsv.py:107, indexed by species `type` - 1


def _card_flags(head_seg, body_seg, types, device):
    """flags byte per card: bit 0 = has head vectors, bit 1 = has body vectors, bits 2..7 = species type"""
    hs = torch.as_tensor(head_seg, dtype=torch.int64)
    bs = torch.as_tensor(body_seg, dtype=torch.int64)
    t = torch.as_tensor(types, dtype=torch.int64)
    if not (hs.numel() == bs.numel() == t.numel() + 1):
        raise PfrError("calc_scores: head_seg / body_seg need ncards+1 offsets, types ncards entries")
    if int(t.min()) < 1 or int(t.max()) > 63:
        raise PfrError("calc_scores: species type must be in 1..63")
    f = (hs[1:] > hs[:-1]).long() | ((bs[1:] > bs[:-1]).long() << 1) | (t << 2)
    return f.to(torch.uint8).to(device).contiguous()


def calc_scores(q_head, q_head_seg, q_body, q_body_seg, q_type, g_head, g_head_seg, g_body, g_body_seg, g_type, k=100,
                thresholds=FUSION_THRESHOLDS, chunk=32768, strategy="mean"):
    """Card-vs-card ranking of the reference's inference pipeline WITH its head/body fusion rule
    (generate_tsv.py:91-125 `calc_scores`), on the device.

    Query cards (the reference's `init_db`) and gallery cards (`extra_db`) are given per modality as ragged photo-embedding
    matrices: `*_head [P, D]` + `*_head_seg [ncards+1]` row offsets (an empty range = the card has no head vectors),
    likewise `*_body`; `*_type [ncards]` is the species id (1 or 2).  Per (query card, gallery card) pair:
        skip when types differ                                                               (:100-101)
        s0 = mean-strategy head score if both have head vectors else 0                        (:103-104, :71-78)
        s1 = mean-strategy body score if both have body vectors else 0                        (:105-106)
        skip when s0 + s1 == 0                                                                (:107-108)
        score = s1 if (query has no head vectors or (s0 == 0 and s1 > thresholds[type-1])) else s0   (:109)
    then descending sort, best `k` (=100) gallery cards, and the (top-1, mean of best 3, mean of best 10) columns (:112-123).

    The mean over the photo cross product of (cos+1)/2 is (⟨centroid_q, centroid_g⟩ + 1)/2, so each modality is one fp32
    GEMM of card centroids per gallery chunk; `pfr_card_fuse_scores` applies the rule in place and the running top-k
    kernel keeps the best k.  Ties → lower gallery index (Python's stable `sorted(reverse=True)` keeps dict order).
    strategy='max': s0 and s1 are the max-strategy scores instead (generate_tsv.py:81-88 in place of :71-78) — the two per-modality score
    chunks come from pfr_card_max_scores in fp32 instead of the centroid GEMM; the rule, the flags, the thresholds and the top-k are the
    same.  Its −inf entries (a card without photos of that modality) are exactly the pairs whose flags already zero the modality score.
    → dict(scores [Q,k] fp32, idx [Q,k] int32 (−1 past the end of a short list), count [Q], top1, mean3, mean10 [Q] fp64).
    A query with count 0 gets no row in the reference; with fewer than 3 / 10 entries the reference raises IndexError,
    here the available ones are averaged."""
    _check_strategy(strategy, "calc_scores")
    dev = q_head.device if q_head.numel() else q_body.device
    if dev.type != "cuda":
        raise PfrError("calc_scores runs on the gfx950 device only (tests use oracle/match_ref.py as the CPU checker)")
    if k > 512:
        raise PfrError(f"calc_scores: k={k} exceeds the 512-entry running list of the gfx950 top-K kernels")
    qf = _card_flags(q_head_seg, q_body_seg, q_type, dev)
    gf = _card_flags(g_head_seg, g_body_seg, g_type, dev)
    Q, G = qf.numel(), gf.numel()
    if Q > 65535:
        raise PfrError("calc_scores: split the query cards into blocks of <= 65535")

    def cents(emb, seg, n):
        if emb.numel() == 0:
            return None
        return card_centroids(emb.to(dev), seg)

    def side(emb, seg, n):
        if emb.numel() == 0:
            return None
        return _CardSide(emb, seg, torch.float32, dev, False, "calc_scores")

    if strategy == "max":
        qc = (side(q_head, q_head_seg, Q), side(q_body, q_body_seg, Q))
        gc = (side(g_head, g_head_seg, G), side(g_body, g_body_seg, G))
    else:
        qc = (cents(q_head, q_head_seg, Q), cents(q_body, q_body_seg, Q))
        gc = (cents(g_head, g_head_seg, G), cents(g_body, g_body_seg, G))
    chunk = min(chunk, G)
    ld = (chunk + 3) // 4 * 4
    sb = [torch.zeros((Q, 1, 1, ld), dtype=torch.float32, device=dev) for _ in range(2)]
    state = torch.empty(lib.pfr_topk_state_bytes(Q, k), dtype=torch.uint8, device=dev)
    lib.pfr_topk_reset(state.data_ptr(), Q, k, _stream())
    thr = (ctypes.c_float * len(thresholds))(*thresholds)
    for c0 in range(0, G, chunk):
        n = min(chunk, G - c0)
        for m in range(2):
            if qc[m] is None or gc[m] is None:            # a modality nobody has stays 0 and is masked by the flags
                continue
            if strategy == "max":
                _card_max_chunk(qc[m], gc[m], torch.float32, c0, n, sb[m], ld)
            else:
                D = qc[m].shape[1]
                ops.conv2d_fwd(qc[m].view(Q, 1, 1, D), gc[m][c0:c0 + n].view(n, 1, 1, D), out=sb[m])
        lib.pfr_card_fuse_scores(sb[0].data_ptr(), sb[1].data_ptr(), Q, ld, n, c0, qf.data_ptr(), gf.data_ptr(),
                                 ctypes.addressof(thr), len(thresholds), _stream())
        lib.pfr_topk_update(sb[0].data_ptr(), Q, ld, n, c0, k, state.data_ptr(), 0, _stream())
    sc = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    lib.pfr_topk_finish(state.data_ptr(), Q, k, sc.data_ptr(), idx.data_ptr(), _stream())
    skipped = torch.isinf(sc) & (sc < 0)          # pairs the reference `continue`s sort last; drop them
    idx = torch.where(skipped, torch.full_like(idx, -1), idx)
    count = (~skipped).sum(1)
    s64 = torch.where(skipped, torch.zeros_like(sc), sc).double()
    cs = s64.cumsum(1)

    def mean_first(m):
        m_eff = count.clamp(min=1, max=min(m, k))
        return cs.gather(1, (m_eff - 1)[:, None])[:, 0] / m_eff
    return {"scores": sc, "idx": idx, "count": count, "top1": s64[:, 0], "mean3": mean_first(3), "mean10": mean_first(10)}


def calc_scores_db(init_db, extra_db, device="cuda", k=100, thresholds=FUSION_THRESHOLDS, strategy="mean"):
    """`calc_scores(init_db, extra_db)` with the reference's own argument and return types (generate_tsv.py:91-125):
    both dbs map a card path to {'head_vectors': [tensor], 'body_vectors': [tensor], 'type': int}; → list of
    (query name, top-1 score, mean of best 3, mean of best 10, ','-joined names of the best `k` gallery cards).
    strategy: 'mean' or 'max', as in `calc_scores`."""
    from pathlib import Path
    _check_strategy(strategy, "calc_scores_db")

    def pack(db):
        names, types, head, body, hs, bs = [], [], [], [], [0], [0]
        for f, card in db.items():
            names.append(Path(f).name)
            types.append(int(card['type']))
            head.extend(card['head_vectors'])
            body.extend(card['body_vectors'])
            hs.append(len(head))
            bs.append(len(body))
        cat = lambda v: torch.stack([t.reshape(-1).float() for t in v]).to(device) if v else torch.empty((0, 0), device=device)
        return names, cat(head), hs, cat(body), bs, types

    qn, qh, qhs, qb, qbs, qt = pack(init_db)
    gn, gh, ghs, gb, gbs, gt = pack(extra_db)
    if not qn or not gn:
        return []
    r = calc_scores(qh, qhs, qb, qbs, qt, gh, ghs, gb, gbs, gt, k=k, thresholds=thresholds, strategy=strategy)
    idx, cnt = r["idx"].cpu(), r["count"].cpu()
    top1, m3, m10 = r["top1"].cpu(), r["mean3"].cpu(), r["mean10"].cpu()
    rows = []
    for i, name in enumerate(qn):
        if int(cnt[i]) == 0:
            continue
        rows.append((str(name), float(top1[i]), float(m3[i]), float(m10[i]),
                     ','.join(gn[j] for j in idx[i, :int(cnt[i])].tolist())))
    return rows


TSV_COLUMNS = ('query', 'matched_1', 'matched_3', 'matched_10', 'answer')     # generate_tsv.py:129-135


def create_table(db, device="cuda", k=100, strategy="mean"):
    """`create_table(db)` of the reference (generate_tsv.py:128-142): db maps a folder to (initial_base_dict, extra_base_dict);
    every folder's cards are ranked on the device (calc_scores_db) and the rows are collected into one DataFrame with the
    reference's columns.  `create_table(db).to_csv(path, index=False, sep='\t')` is its TSV (generate_tsv.py:262-264).
    strategy: 'mean' or 'max', as in `calc_scores`."""
    _check_strategy(strategy, "create_table")
    import pandas as pd
    rows = []
    for big_folder in db:
        init_db, extra_db = db[big_folder]
        rows.extend(calc_scores_db(init_db, extra_db, device=device, k=k, strategy=strategy))
    return pd.DataFrame(data=rows, columns=TSV_COLUMNS)


def cosine_topk_sharded(q, g_local, k, g_offset, group=None, **kw):
    """Gallery sharded by rows across the ranks of `group` (each rank holds rows [g_offset, g_offset + len(g_local))),
    queries replicated: local GEMM + top-k per rank, ONE all-gather of the (score, index) lists (k·8 bytes per query
    and rank), merge to the global top-k on every rank.  SURVEY.md §8e."""
    import torch.distributed as dist
    sc, idx = cosine_topk(q, g_local, k, **kw)
    kk = sc.shape[1]
    if kk < k:   # pad short lists so that every rank gathers equal shapes
        pad = k - kk
        sc = torch.cat([sc, torch.full((sc.shape[0], pad), -float("inf"), device=sc.device)], 1)
        idx = torch.cat([idx, torch.full((idx.shape[0], pad), -1, dtype=idx.dtype, device=idx.device)], 1)
    if sc.dtype != torch.float32:
        raise PfrError(f"cosine_topk_sharded: scores must be fp32 for the packed all-gather, got {sc.dtype}")
    if int(g_offset) < 0 or int(g_offset) + int(g_local.shape[0]) >= 2 ** 31:
        raise PfrError(f"cosine_topk_sharded: global gallery rows up to {int(g_offset) + int(g_local.shape[0])} do not fit the int32 "
                       f"index half of the packed (score, index) all-gather")
    gidx = torch.where(idx >= 0, idx + int(g_offset), idx).int()
    world = dist.get_world_size(group)
    # ONE collective: (fp32 score bits, int32 global index) pairs of every rank, [world][Q][k][2] int32
    mine = torch.stack([sc.contiguous().view(torch.int32), gidx], dim=2).contiguous()
    everyone = torch.empty((world,) + tuple(mine.shape), dtype=torch.int32, device=mine.device)
    dist.all_gather(list(everyone.unbind(0)), mine, group=group)     # (views of one buffer: gloo has no all_gather_into_tensor)
    S = everyone[..., 0].contiguous().view(torch.float32).permute(1, 0, 2).reshape(sc.shape[0], world * k)
    I = everyone[..., 1].permute(1, 0, 2).reshape(sc.shape[0], world * k).long()
    # merge: score descending, ties → lower global index
    key_i = torch.where(I >= 0, I, torch.full_like(I, 2 ** 62))
    order = torch.argsort(key_i, dim=1, stable=True)
    S, I = torch.gather(S, 1, order), torch.gather(I, 1, order)
    order = torch.argsort(S, dim=1, descending=True, stable=True)[:, :k]
    return torch.gather(S, 1, order), torch.gather(I, 1, order)


# ---- all-pairs verification ------------------------------------------------------------------------------------------------------
_PAIR_HIST_DTYPES = (torch.float32, torch.bfloat16, torch.int8)


def _hist_range(bins, range):
    """(lo, inv_w) as the fp32 numbers both paths use: inv_w = float32(bins) / (float32(hi) - float32(lo))"""
    lo, hi = torch.tensor(float(range[0]), dtype=torch.float32), torch.tensor(float(range[1]), dtype=torch.float32)
    inv_w = torch.tensor(float(bins), dtype=torch.float32) / (hi - lo)
    if not (bool(torch.isfinite(inv_w)) and float(inv_w) > 0 and bool(torch.isfinite(lo))):
        raise PfrError(f"pair_histogram: bad range {tuple(range)}")
    return float(lo), float(inv_w)


def _pad_cols(x, mult):
    pad = -x.shape[1] % mult
    return x if pad == 0 else torch.nn.functional.pad(x, (0, pad)).contiguous()


def _hist_operand(x, T, normalize):
    """rows -> (GEMM operand of pfr_pair_hist, per-row scales or None): the match's own preparation, columns zero padded to a 128-byte k-step"""
    x32 = x.float().contiguous()
    if T == torch.int8:
        (q8, sc), _ = _prep_rows_i8(x32, False, normalize)
        return q8, sc
    xn, _ = _prep_rows(x32, T, False, normalize)
    return _pad_cols(xn.contiguous(), 32 if T == torch.float32 else 64), None


def pair_histogram(emb, classes, emb_b=None, classes_b=None, bins=4096, range=(-1.0, 1.0), compute_dtype=torch.bfloat16, normalize=True):
    """Genuine / impostor score histograms over EVERY pair: all unordered pairs i < j of `emb` [N, D], or — with `emb_b`, `classes_b` — all
    Na x Nb pairs of the two sets.  The score of a pair is the dot product of the (L2-normalised unless normalize=False) rows in
    `compute_dtype` (torch.float32, torch.bfloat16, or torch.int8: the selection score of `quantize_rows`); it is binned by the rule of
    pfr_pair_hist (include/pfr_hip.h): x = (s - lo) * inv_w in fp32, bin = clamp(floor(x), 0, bins - 1), NaN -> slot `bins`.
    → (hist int64 [2, bins + 1] with hist[1] the same-class pairs, lo, inv_w).
    CUDA tensors: ONE pfr_pair_hist launch, the score matrix is never written.  CPU tensors: chunked fp32 matmul, same bin rule."""
    if compute_dtype not in _PAIR_HIST_DTYPES:
        raise PfrError(f"pair_histogram: compute_dtype must be one of {_PAIR_HIST_DTYPES}")
    bins = int(bins)
    if not 1 <= bins <= 8192:
        raise PfrError(f"pair_histogram: bins={bins} must be in 1..8192")
    if (emb_b is None) != (classes_b is None):
        raise PfrError("pair_histogram: emb_b and classes_b come together")
    if emb.dim() != 2 or classes.numel() != emb.shape[0] or (emb_b is not None and (emb_b.dim() != 2 or emb_b.shape[1] != emb.shape[1]
                                                                                    or classes_b.numel() != emb_b.shape[0])):
        raise PfrError("pair_histogram: emb [N, D] with classes [N] (and emb_b [Nb, D] with classes_b [Nb])")
    lo, inv_w = _hist_range(bins, range)
    if not emb.is_cuda:
        return _pair_histogram_torch(emb, classes, emb_b, classes_b, bins, lo, inv_w, normalize), lo, inv_w
    dev = emb.device
    hist = torch.zeros((2, bins + 1), dtype=torch.int64, device=dev)
    Na, Nb = emb.shape[0], 0 if emb_b is None else emb_b.shape[0]
    if Na == 0 or (emb_b is None and Na == 1) or (emb_b is not None and Nb == 0):
        return hist, lo, inv_w
    a, sa = _hist_operand(emb, compute_dtype, normalize)
    ca = classes.to(device=dev, dtype=torch.int32).contiguous()
    b = sb = cb = None
    if emb_b is not None:
        b, sb = _hist_operand(emb_b.to(dev), compute_dtype, normalize)
        cb = classes_b.to(device=dev, dtype=torch.int32).contiguous()
    ptr = lambda t: 0 if t is None else t.data_ptr()
    lib.pfr_pair_hist(ptr(a), ptr(sa), ptr(ca), Na, ptr(b), ptr(sb), ptr(cb), Nb, dtype_id(compute_dtype), a.shape[1], lo, inv_w, bins,
                      hist.data_ptr(), _stream())
    return hist, lo, inv_w


def _bin_rule_torch(s, lo, inv_w, bins):
    """the bin rule on an fp32 tensor of scores -> int64 slots (NaN -> bins)"""
    x = (s - torch.tensor(lo, dtype=torch.float32)) * torch.tensor(inv_w, dtype=torch.float32)
    slot = torch.floor(x).clamp(0, bins - 1)
    return torch.where(torch.isnan(s), torch.full_like(slot, bins), slot).long()


def _pair_histogram_torch(emb, classes, emb_b, classes_b, bins, lo, inv_w, normalize, chunk=2048):
    def rows(x):
        x = x.float()
        return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else x
    a, ca = rows(emb), classes.long().reshape(-1)
    sym = emb_b is None
    b, cb = (a, ca) if sym else (rows(emb_b), classes_b.long().reshape(-1))
    hist = torch.zeros(2 * (bins + 1), dtype=torch.int64)
    jb = torch.arange(b.shape[0])
    for r0 in range(0, a.shape[0], chunk):
        s = a[r0:r0 + chunk] @ b.t()
        slot = _bin_rule_torch(s, lo, inv_w, bins) + (ca[r0:r0 + chunk, None] == cb[None, :]).long() * (bins + 1)
        if sym:
            slot = slot[torch.arange(r0, r0 + s.shape[0])[:, None] < jb[None, :]]
        hist += torch.bincount(slot.reshape(-1), minlength=2 * (bins + 1))
    return hist.view(2, bins + 1)


# ---- exact retrieval ranks: mAP / CMC / mINP ----------------------------------------------------------------------------------------
def rank_count_max_thr():
    """thresholds per row one pfr_rank_count launch takes (host arithmetic)"""
    return int(lib.pfr_rank_count_max_thr())


def _positive_lists(ca, cb, sym):
    """The positives of every query, without anything Nq x Nb: a stable sort of the gallery classes makes every class one run.
    → (col int64 [Nq, Pmax]: gallery indices of the query's same-class items (itself left out when `sym`), ascending, -1 padded;
       npos int64 [Nq])"""
    Nq, dev = ca.numel(), ca.device
    order = torch.argsort(cb, stable=True)
    scb = cb[order]
    lo = torch.searchsorted(scb, ca, right=False)
    n = torch.searchsorted(scb, ca, right=True) - lo
    npos = n - 1 if sym else n                      # (symmetric: the query is one item of its own run)
    pmax = int(npos.max()) if Nq else 0
    k = torch.arange(pmax, device=dev)[None, :]
    src = k
    if sym:
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.numel(), device=dev)
        src = k + (k >= (inv - lo)[:, None]).long()  # skip the query's own place in the run
    ok = k < npos[:, None]
    pos = (lo[:, None] + src).clamp_max(max(cb.numel() - 1, 0))
    col = torch.where(ok, order[pos] if cb.numel() else pos, torch.full_like(pos, -1))
    return col, npos


def _precede_counts_torch(s, ids, thr, tid, excl, budget=1 << 24):
    """the count of pfr_rank_count on a dense block of scores: s [c, Nb] with column ids [Nb], thresholds thr / tid [c, P], excl [c] or
    None → int64 [c, P]; the compares are the contract's (IEEE: NaN precedes nothing, nothing precedes NaN)"""
    c, Nb = s.shape
    P = thr.shape[1]
    out = torch.zeros((c, P), dtype=torch.int64, device=s.device)
    keep = None if excl is None else (ids[None, :] != excl[:, None])
    pk = max(1, budget // max(1, c * Nb))
    for k0 in range(0, P, pk):
        t, ti = thr[:, k0:k0 + pk, None], tid[:, k0:k0 + pk, None]
        pre = (s[:, None, :] > t) | ((s[:, None, :] == t) & (ids[None, None, :] < ti))
        if keep is not None:
            pre &= keep[:, None, :]
        out[:, k0:k0 + pk] = pre.sum(dim=2)
    return out


def _positive_counts_torch(a, b, col, npos, sym, chunk=256):
    """chunked dense restatement of the device path (any device): per block of query rows one fp32 matmul, the thresholds gathered from it,
    the contract's compares, a sum — no argsort.  a, b: prepared fp32 rows → cnt int64 [Nq, Pmax]"""
    Nq, P = col.shape
    ids = torch.arange(b.shape[0], device=a.device)
    cnt = torch.zeros((Nq, P), dtype=torch.int64, device=a.device)
    if P == 0 or b.shape[0] == 0:
        return cnt
    for r0 in range(0, Nq, chunk):
        s = a[r0:r0 + chunk] @ b.t()
        cc = col[r0:r0 + chunk]
        thr = torch.gather(s, 1, cc.clamp_min(0))
        excl = torch.arange(r0, r0 + s.shape[0], device=a.device) if sym else None
        cnt[r0:r0 + chunk] = _precede_counts_torch(s, ids, thr, cc, excl)
    return cnt


def _ranks_from_counts(cnt, npos):
    """counts [Nq, Pmax] → 1-based ranks, ascending per row, 0 padded (int32)"""
    big = torch.iinfo(torch.int64).max
    ok = torch.arange(cnt.shape[1], device=cnt.device)[None, :] < npos[:, None]
    r = torch.where(ok, cnt.long() + 1, torch.full_like(cnt.long(), big)).sort(dim=1).values
    return torch.where(r == big, torch.zeros_like(r), r).int()


def positive_ranks(emb, classes, emb_b=None, classes_b=None, compute_dtype=torch.float32, normalize=True):
    """The exact rank of every positive of every query among ALL the other items — what mAP, mINP and the CMC curve are made of.
    Symmetric (`emb` [N, D], `classes` [N]): every item queries the N - 1 others, positives = same class, not itself.  Query / gallery
    (`emb_b`, `classes_b`): the rows of `emb` query the rows of `emb_b`, positives = same class in the gallery, nothing is excluded.
    Scores are the dot products of the (L2-normalised unless normalize=False) rows in `compute_dtype` (torch.float32, torch.bfloat16,
    torch.int8), ordered descending with ties to the lower gallery index: rank = 1 + the number of items that precede the positive.
    → (ranks int32 [Nq, Pmax]: 1-based, ascending per row, 0 padded;  npos int32 [Nq]).
    CUDA tensors: pfr_pair_scores_gather gives the positives' own scores, pfr_rank_count counts in the epilogue of the match GEMM (one
    launch per `rank_count_max_thr()` positives of the longest list); no score matrix, no sort.  CPU tensors: chunked dense fp32 matmul
    with the same compares."""
    who = "positive_ranks"
    if compute_dtype not in _PAIR_HIST_DTYPES:
        raise PfrError(f"{who}: compute_dtype must be one of {_PAIR_HIST_DTYPES}")
    if (emb_b is None) != (classes_b is None):
        raise PfrError(f"{who}: emb_b and classes_b come together")
    if emb.dim() != 2 or classes.numel() != emb.shape[0] or (emb_b is not None and (emb_b.dim() != 2 or emb_b.shape[1] != emb.shape[1]
                                                                                    or classes_b.numel() != emb_b.shape[0])):
        raise PfrError(f"{who}: emb [N, D] with classes [N] (and emb_b [Nb, D] with classes_b [Nb])")
    if max(emb.shape[0], 0 if emb_b is None else emb_b.shape[0]) >= 2 ** 31:
        raise PfrError(f"{who}: more than 2^31 - 1 rows")
    dev, sym = emb.device, emb_b is None
    ca = classes.to(dev).long().reshape(-1)
    cb = ca if sym else classes_b.to(dev).long().reshape(-1)
    col, npos = _positive_lists(ca, cb, sym)
    Nq, P = col.shape
    if not emb.is_cuda:
        def rows(x):
            x = x.float()
            return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else x
        a = rows(emb)
        cnt = _positive_counts_torch(a, a if sym else rows(emb_b), col, npos, sym)
        return _ranks_from_counts(cnt, npos), npos.int()
    cnt = torch.zeros((Nq, P), dtype=torch.int32, device=dev)
    Nb = Nq if sym else emb_b.shape[0]
    if Nq and Nb and P:
        a, sa = _hist_operand(emb, compute_dtype, normalize)
        b = sb = None
        if not sym:
            b, sb = _hist_operand(emb_b.to(dev), compute_dtype, normalize)
        ptr = lambda t: 0 if t is None else t.data_ptr()
        T, Dp = dtype_id(compute_dtype), a.shape[1]
        ids = torch.arange(Nb, dtype=torch.int32, device=dev)
        excl = torch.arange(Nq, dtype=torch.int32, device=dev) if sym else None
        col32 = col.int().contiguous()
        thr = torch.zeros((Nq, P), dtype=torch.float32, device=dev)
        lib.pfr_pair_scores_gather(ptr(a), ptr(sa), Nq, ptr(b), ptr(sb), Nb, T, Dp, col32.data_ptr(), P, thr.data_ptr(), _stream())
        cap = rank_count_max_thr()
        for k0 in range(0, P, cap):
            w = min(cap, P - k0)
            tv, ti = thr[:, k0:k0 + w].contiguous(), col32[:, k0:k0 + w].contiguous()
            tc = (npos - k0).clamp(0, w).int().contiguous()
            part = cnt if w == P else torch.zeros((Nq, w), dtype=torch.int32, device=dev)
            lib.pfr_rank_count(ptr(a), ptr(sa), Nq, ptr(b), ptr(sb), ids.data_ptr(), Nb, T, Dp, ptr(excl), tv.data_ptr(), ti.data_ptr(),
                               tc.data_ptr(), w, part.data_ptr(), _stream())
            if part is not cnt:
                cnt[:, k0:k0 + w] = part
    return _ranks_from_counts(cnt, npos), npos.int()


def retrieval_metrics(emb, classes, emb_b=None, classes_b=None, ks=(1, 5, 10), compute_dtype=torch.float32, normalize=True):
    """mAP, mINP, the CMC curve at `ks` and the mean first rank over the queries that have a positive, from `positive_ranks` (same
    arguments).  With r_(1) < … < r_(n) the ranks of a query's n positives: AP = (1 / n) Σ_k k / r_(k), INP = n / r_(n), CMC@K = share of
    queries with r_(1) <= K (engine.metrics.RankStats; float64 sums on the host).
    → {'mAP', 'mINP', 'CMC@K={k}' for k in ks, 'mean_first_rank', 'queries'}; no valid query: NaN metrics and queries = 0.
    Not covered: the camera / junk filtering of the re-ID protocols, and the mAP of a re-ranked order (it needs the re-ranked distance of
    every item, `rerank` scores candidate lists)."""
    from ..engine.metrics import RankStats
    ks = tuple(int(k) for k in ks)
    if any(k < 1 for k in ks):
        raise PfrError(f"retrieval_metrics: ks={ks} must be positive")
    ranks, npos = positive_ranks(emb, classes, emb_b, classes_b, compute_dtype=compute_dtype, normalize=normalize)
    return RankStats(ranks, npos).metrics(ks)


# ---- threshold clustering: range search and single-linkage components ----------------------------------------------------------------
#: edge capacity of the first pfr_pairs_above launch of `pairs_above` (12 bytes per edge); a second launch takes the exact count
PAIRS_ABOVE_DEFAULT_CAP = 1 << 22


def _fp32(x):
    """a Python float rounded once to fp32 (what the kernels compare with)"""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _check_pair_sets(who, emb, emb_b, compute_dtype):
    if compute_dtype not in _PAIR_HIST_DTYPES:
        raise PfrError(f"{who}: compute_dtype must be one of {_PAIR_HIST_DTYPES}")
    if emb.dim() != 2 or (emb_b is not None and (emb_b.dim() != 2 or emb_b.shape[1] != emb.shape[1])):
        raise PfrError(f"{who}: emb [N, D] (and emb_b [Nb, D])")
    if max(emb.shape[0], 0 if emb_b is None else emb_b.shape[0]) >= 2 ** 31:
        raise PfrError(f"{who}: more than 2^31 - 1 rows")


def _pairs_above_torch(emb, emb_b, thr, normalize, max_pairs=None, chunk=2048):
    """chunked fp32 matmul with the comparison rule of pfr_pairs_above (s >= thr in IEEE arithmetic: NaN never qualifies)"""
    def rows(x):
        x = x.float()
        return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else x
    a = rows(emb)
    sym = emb_b is None
    b = a if sym else rows(emb_b)
    jb = torch.arange(b.shape[0])
    ii, jj, ss, total = [], [], [], 0
    for r0 in range(0, a.shape[0], chunk):
        s = a[r0:r0 + chunk] @ b.t()
        ok = s >= thr
        if sym:
            ok &= torch.arange(r0, r0 + s.shape[0])[:, None] < jb[None, :]
        i, j = ok.nonzero(as_tuple=True)
        total += i.numel()
        if max_pairs is not None and total > max_pairs:
            continue                                  # (keep counting: the error names the whole count)
        ii.append(i + r0); jj.append(j); ss.append(s[i, j])
    if max_pairs is not None and total > max_pairs:
        raise PfrError(f"pairs_above: {total} pairs at or above the threshold, max_pairs={max_pairs}")
    cat = lambda ts, dt: torch.cat(ts) if ts else torch.zeros(0, dtype=dt)
    return cat(ii, torch.int64), cat(jj, torch.int64), cat(ss, torch.float32)


def pairs_above(emb, threshold, emb_b=None, compute_dtype=torch.float32, normalize=True, max_pairs=None):
    """Range search (duplicate detection): EVERY pair whose score is at or above `threshold` — all unordered pairs i < j of `emb` [N, D],
    or with `emb_b` all Na x Nb pairs of the two sets.  The score is the dot product of the (L2-normalised unless normalize=False) rows
    in `compute_dtype` (torch.float32, torch.bfloat16, torch.int8), the score of `pair_histogram`; `threshold` is on that dot product and
    is rounded once to fp32.  A pair qualifies iff score >= threshold in IEEE arithmetic (a NaN score never does).
    → (i int64 [E], j int64 [E], score fp32 [E]) sorted by (i, j).
    CUDA tensors: ONE pfr_pairs_above launch (the match GEMM with a compacting-append epilogue, nothing N x N is written) with a default
    capacity; when more pairs qualify, one more launch with the exact count, never a third.  `max_pairs`: a PfrError that names the count
    instead of a larger allocation.  CPU tensors: chunked fp32 matmul, same rule."""
    who = "pairs_above"
    _check_pair_sets(who, emb, emb_b, compute_dtype)
    if max_pairs is not None and int(max_pairs) < 0:
        raise PfrError(f"{who}: max_pairs={max_pairs} must be >= 0")
    max_pairs = None if max_pairs is None else int(max_pairs)
    thr = _fp32(threshold)
    if not emb.is_cuda:
        return _pairs_above_torch(emb, emb_b, thr, normalize, max_pairs)
    dev, sym = emb.device, emb_b is None
    Na, Nb = emb.shape[0], emb.shape[0] if sym else emb_b.shape[0]
    npairs = Na * (Na - 1) // 2 if sym else Na * Nb
    empty = (torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
             torch.zeros(0, dtype=torch.float32, device=dev))
    if npairs == 0:
        return empty
    a, sa = _hist_operand(emb, compute_dtype, normalize)
    b = sb = None
    if not sym:
        b, sb = _hist_operand(emb_b.to(dev), compute_dtype, normalize)
    ptr = lambda t: 0 if t is None else t.data_ptr()
    cap = max(1, min(npairs, PAIRS_ABOVE_DEFAULT_CAP if max_pairs is None else min(PAIRS_ABOVE_DEFAULT_CAP, max_pairs)))
    for attempt in (0, 1):
        ei = torch.empty(cap, dtype=torch.int32, device=dev)
        ej = torch.empty(cap, dtype=torch.int32, device=dev)
        es = torch.empty(cap, dtype=torch.float32, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        lib.pfr_pairs_above(ptr(a), ptr(sa), Na, 0, ptr(b), ptr(sb), 0 if sym else Nb, 0, dtype_id(compute_dtype), a.shape[1], thr,
                            ei.data_ptr(), ej.data_ptr(), es.data_ptr(), cap, count.data_ptr(), 0, 0, 0, _stream())
        n = int(count.item())
        if max_pairs is not None and n > max_pairs:
            raise PfrError(f"{who}: {n} pairs at or above the threshold, max_pairs={max_pairs}")
        if n <= cap:
            break
        if attempt == 1:
            raise PfrError(f"{who}: the second launch counted {n} pairs for a capacity of {cap} (the set is deterministic: a bug)")
        cap = n
    i, j, s = ei[:n].long(), ej[:n].long(), es[:n]
    order = torch.argsort(i * Nb + j)
    return i[order], j[order], s[order]


def _host_components(n, i, j):
    """host union-find (path halving, larger root under the smaller) over the edges (i, j) -> int64 labels [n] = component minimum"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for u, v in zip(i.tolist(), j.tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return torch.tensor([find(x) for x in range(n)], dtype=torch.int64)


def cluster(emb, threshold, compute_dtype=torch.float32, normalize=True, chunk=None):
    """Identity clustering at a threshold: single linkage = the connected components of the graph whose edges are the pairs of
    `pairs_above(emb, threshold, …)` (same score, same rule).  → labels int64 [N]: the smallest index of the item's component.
    CUDA tensors: pfr_pairs_above with the union-find epilogue and NO edge list (one launch, or with `chunk` one launch per (row block,
    column block) of that many rows with node offsets), then pfr_cc_flatten; a non-zero status word of the union-find's loop caps raises a
    PfrError.  CPU tensors: a host union-find over the edges of the CPU `pairs_above`.
    Not covered: a threshold so low that the graph is near complete costs ~N^2 / 2 finds on the device (correct, slow, not measured); only
    single linkage here — `dbscan` is the density-based variant (noise, core points); no average linkage or Chinese whispers."""
    who = "cluster"
    _check_pair_sets(who, emb, None, compute_dtype)
    if chunk is not None and int(chunk) < 1:
        raise PfrError(f"{who}: chunk={chunk} must be >= 1")
    N = emb.shape[0]
    if not emb.is_cuda:
        i, j, _ = _pairs_above_torch(emb, None, _fp32(threshold), normalize)
        return _host_components(N, i, j)
    dev = emb.device
    parent = torch.arange(N, dtype=torch.int32, device=dev)
    if N < 2:
        return parent.long()
    thr = _fp32(threshold)
    a, sa = _hist_operand(emb, compute_dtype, normalize)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _block_launches(lib.pfr_pairs_above, a, sa, N, chunk, (dtype_id(compute_dtype), a.shape[1], thr),
                    (0, 0, 0, 0, 0, parent.data_ptr(), N, status.data_ptr(), _stream()))
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    lib.pfr_cc_flatten(parent.data_ptr(), N, labels.data_ptr(), _stream())
    if int(status.item()) != 0:
        raise PfrError(f"{who}: the union-find gave up on a pair (status {int(status.item())}): a loop reached its iteration cap")
    return labels.long()


def _check_chunk(who, chunk):
    if chunk is not None and int(chunk) < 1:
        raise PfrError(f"{who}: chunk={chunk} must be >= 1")


def _block_launches(fn, a, sa, N, chunk, head, tail, block_head=None):
    """one `fn` launch per (row block, column block) of the upper triangle with node offsets — the blocks of `cluster`; `head` are the
    arguments between b_off and the outputs (dtype, D, thr), `tail` the outputs and what follows them; `block_head(r0, c0)` (c0 None:
    the block's own pairs) gives further arguments behind `head` that depend on the block"""
    step = N if chunk is None else int(chunk)
    sp = lambda r0: 0 if sa is None else sa[r0:].data_ptr()
    more = (lambda r0, c0: ()) if block_head is None else block_head
    for r0 in range(0, N, step):
        nr = min(step, N - r0)
        for c0 in range(r0, N, step):
            if c0 == r0:     # the block's own pairs: symmetric mode
                fn(a[r0:].data_ptr(), sp(r0), nr, r0, 0, 0, 0, 0, *head, *more(r0, None), *tail)
            else:
                fn(a[r0:].data_ptr(), sp(r0), nr, r0, a[c0:].data_ptr(), sp(c0), min(step, N - c0), c0, *head, *more(r0, c0), *tail)


def _neighbor_counts_dev(a, sa, N, T, thr, chunk):
    deg = torch.zeros(N, dtype=torch.int32, device=a.device)
    _block_launches(lib.pfr_neighbor_count, a, sa, N, chunk, (T, a.shape[1], thr), (deg.data_ptr(), N, _stream()))
    return deg


def _unit_rows_f32(emb, normalize):
    x = emb.float()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalize else x


def _neighbor_counts_torch(emb, thr, normalize, chunk=2048):
    """degrees from the chunks of `_pairs_above_torch`'s rule (s >= thr, NaN never, self excluded) -> int64 [N]"""
    a = _unit_rows_f32(emb, normalize)
    N = a.shape[0]
    deg = torch.zeros(N, dtype=torch.int64)
    for r0 in range(0, N, chunk):
        ok = (a[r0:r0 + chunk] @ a.t()) >= thr
        ok &= torch.arange(r0, r0 + ok.shape[0])[:, None] != torch.arange(N)[None, :]
        deg[r0:r0 + ok.shape[0]] = ok.sum(dim=1)
    return deg


def neighbor_counts(emb, threshold, compute_dtype=torch.float32, normalize=True, chunk=None):
    """How crowded is every item's neighbourhood: → int64 [N], the number of OTHER items of `emb` [N, D] whose score with the item is at or
    above `threshold` (the score and the rule of `pairs_above`; the item itself is excluded).  CUDA tensors: pfr_neighbor_count, the match
    GEMM with a degree epilogue (one launch, or with `chunk` one per (row block, column block) as in `cluster`); nothing N x N is written.
    CPU tensors: chunked fp32 matmul, same rule."""
    who = "neighbor_counts"
    _check_pair_sets(who, emb, None, compute_dtype)
    _check_chunk(who, chunk)
    thr = _fp32(threshold)
    if not emb.is_cuda:
        return _neighbor_counts_torch(emb, thr, normalize)
    N = emb.shape[0]
    if N < 2:
        return torch.zeros(N, dtype=torch.int64, device=emb.device)
    a, sa = _hist_operand(emb, compute_dtype, normalize)
    return _neighbor_counts_dev(a, sa, N, dtype_id(compute_dtype), thr, chunk).long()


def _dbscan_torch(emb, thr, min_neighbors, normalize, chunk=2048):
    """the contract of pfr_dbscan_link / pfr_dbscan_labels on the host: degrees, a union-find over the core-core edges, and for every
    non-core item the core neighbour with the largest (score, -index) — -0.0 canonicalised by s + 0.0 — or noise"""
    a = _unit_rows_f32(emb, normalize)
    N = a.shape[0]
    core = _neighbor_counts_torch(emb, thr, normalize, chunk) >= min_neighbors
    idx = torch.arange(N)
    ii, jj = [], []
    best = torch.full((N,), -1, dtype=torch.int64)
    for r0 in range(0, N, chunk):
        s = a[r0:r0 + chunk] @ a.t()
        rows = idx[r0:r0 + s.shape[0]]
        ok = (s >= thr) & (rows[:, None] != idx[None, :]) & core[None, :]          # qualifying pairs whose column is core
        i, j = (ok & core[rows][:, None] & (rows[:, None] < idx[None, :])).nonzero(as_tuple=True)
        ii.append(i + r0); jj.append(j)
        sc = torch.where(ok, s + 0.0, torch.full_like(s, float("-inf")))
        top = sc.max(dim=1, keepdim=True).values
        first = (ok & (sc == top)).int().argmax(dim=1)                              # (argmax of a 0/1 row: the first, i.e. smallest, index)
        has = ok.any(dim=1) & ~core[rows]
        best[rows[has]] = first[has]
    comp = _host_components(N, torch.cat(ii) if ii else torch.zeros(0, dtype=torch.int64), torch.cat(jj) if jj else torch.zeros(0, dtype=torch.int64))
    labels = torch.where(core, comp, torch.full_like(comp, -1))
    border = best >= 0
    labels[border] = comp[best[border]]
    return labels, core


def dbscan(emb, threshold, min_samples=4, compute_dtype=torch.float32, normalize=True, chunk=None, return_core=False):
    """DBSCAN identity clustering at a threshold (the definition of include/pfr_hip.h): an item is CORE when at least `min_samples` items —
    itself included, as in scikit-learn — score at or above `threshold` with it (the score and the rule of `pairs_above`); clusters are the
    connected components of the core items over the qualifying core-core pairs, labelled by their smallest core index; a non-core item with
    a qualifying core neighbour is a BORDER item of the cluster of its highest-scoring core neighbour (ties: the smallest index); every
    other item is NOISE, label -1.  → labels int64 [N] (and the bool core mask [N] with return_core=True).  Unlike single linkage
    (`cluster`), one stray item that scores above the threshold against two animals does not merge them unless it is core itself, and items
    that belong to nothing are not counted as clusters.  `dbscan(x, t, min_samples=1)` equals `cluster(x, t)`: every item is core.
    CUDA tensors: two passes of the match GEMM — pfr_neighbor_count (degree epilogue), then pfr_dbscan_link (union-find over core-core
    pairs, an atomic maximum for the border items) — and pfr_dbscan_labels; nothing N x N and no edge list is written; with `chunk` one
    launch per (row block, column block) for BOTH passes, as in `cluster`; a non-zero status word raises a PfrError.  CPU tensors: chunked
    fp32 matmul and a host union-find, same rule.
    Not covered: two-set DBSCAN, average linkage, HDBSCAN / OPTICS; a near-complete graph is correct and slow, as for `cluster`."""
    who = "dbscan"
    _check_pair_sets(who, emb, None, compute_dtype)
    _check_chunk(who, chunk)
    if isinstance(min_samples, bool) or not isinstance(min_samples, int) or min_samples < 1:
        raise PfrError(f"{who}: min_samples={min_samples!r} must be an int >= 1")
    mn = min_samples - 1
    thr = _fp32(threshold)
    N = emb.shape[0]
    if not emb.is_cuda:
        labels, core = _dbscan_torch(emb, thr, mn, normalize)
        return (labels, core) if return_core else labels
    dev = emb.device
    if N < 2:
        core = torch.full((N,), mn == 0, dtype=torch.bool, device=dev)
        labels = torch.where(core, torch.arange(N, device=dev), torch.full((N,), -1, dtype=torch.int64, device=dev))
        return (labels, core) if return_core else labels
    if mn >= 2 ** 31:
        raise PfrError(f"{who}: min_samples={min_samples} does not fit int32")
    a, sa = _hist_operand(emb, compute_dtype, normalize)
    T = dtype_id(compute_dtype)
    head = (T, a.shape[1], thr)
    deg = _neighbor_counts_dev(a, sa, N, T, thr, chunk)
    parent = torch.arange(N, dtype=torch.int32, device=dev)
    best = torch.zeros(N, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _block_launches(lib.pfr_dbscan_link, a, sa, N, chunk, head, (deg.data_ptr(), mn, parent.data_ptr(), best.data_ptr(), N, status.data_ptr(),
                                                                _stream()))
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    lib.pfr_dbscan_labels(parent.data_ptr(), deg.data_ptr(), best.data_ptr(), mn, N, labels.data_ptr(), _stream())
    if int(status.item()) != 0:
        raise PfrError(f"{who}: the union-find gave up on a pair (status {int(status.item())}): a loop reached its iteration cap")
    return (labels.long(), deg >= mn) if return_core else labels.long()


# ---- open-set identification: best mate / best impostor / weakest mate ---------------------------------------------------------------
#: `class_extremes`: fp32 scores and int64 partner indices [N]; no such pair: index -1, score -inf (weak_score: +inf); weak_* None
#: with weakest=False
Extremes = collections.namedtuple("Extremes", "pos_score pos_index neg_score neg_index weak_score weak_index")


def _check_classes(who, emb, classes, emb_b, classes_b):
    if (emb_b is None) != (classes_b is None):
        raise PfrError(f"{who}: emb_b and classes_b go together")
    for x, c in ((emb, classes), (emb_b, classes_b)):
        if x is None:
            continue
        if not torch.is_tensor(c) or c.dim() != 1 or c.shape[0] != x.shape[0] or c.is_floating_point() or c.dtype == torch.bool:
            raise PfrError(f"{who}: classes must be an integer tensor [N]")
        if c.numel() and (int(c.max()) >= 2 ** 31 or int(c.min()) < -2 ** 31):
            raise PfrError(f"{who}: classes must fit int32")


def _class_extremes_torch(emb, classes, emb_b, classes_b, normalize, weakest, chunk=2048):
    """the contract of pfr_class_extremes on the host, dense fp32 by row chunks: mate iff the classes are equal and not negative, a NaN
    score updates nothing, -0.0 canonicalised by s + 0.0, the highest (weakest: lowest) score and then the smallest partner index"""
    a = _unit_rows_f32(emb, normalize)
    sym = emb_b is None
    b = a if sym else _unit_rows_f32(emb_b, normalize)
    ca = classes.long()
    cb = ca if sym else classes_b.long()
    Na, Nb = a.shape[0], b.shape[0]
    cols = torch.arange(Nb)
    inf = float("inf")
    out = [torch.full((Na,), -inf), torch.full((Na,), -1, dtype=torch.int64), torch.full((Na,), -inf), torch.full((Na,), -1, dtype=torch.int64),
           torch.full((Na,), inf), torch.full((Na,), -1, dtype=torch.int64)]

    def pick(ok, s, lowest, score, index, rows):
        sc = torch.where(ok, -s if lowest else s, torch.full_like(s, -inf))
        top = sc.max(dim=1, keepdim=True).values
        first = (ok & (sc == top)).int().argmax(dim=1)          # (argmax of a 0/1 row: the first, i.e. smallest, index)
        has = ok.any(dim=1)
        score[rows[has]] = s[has, first[has]]
        index[rows[has]] = first[has]
    for r0 in range(0, Na, chunk):
        s = a[r0:r0 + chunk] @ b.t() + 0.0
        rows = torch.arange(r0, r0 + s.shape[0])
        valid = ~torch.isnan(s)
        if sym:
            valid &= rows[:, None] != cols[None, :]
        mate = (ca[rows][:, None] == cb[None, :]) & (ca[rows][:, None] >= 0)
        if Nb:
            pick(valid & mate, s, False, out[0], out[1], rows)
            pick(valid & ~mate, s, False, out[2], out[3], rows)
            if weakest:
                pick(valid & mate, s, True, out[4], out[5], rows)
    return Extremes(*out[:4], *(out[4:] if weakest else (None, None)))


def class_extremes(emb, classes, emb_b=None, classes_b=None, compute_dtype=torch.float32, normalize=True, chunk=None, weakest=True):
    """Per item of `emb` [N, D] the BEST MATE (the highest score against an item of the same class), the BEST IMPOSTOR (the highest score
    against an item of any other class) and — with weakest=True — the WEAKEST MATE (the lowest same-class score), each with the partner's
    index: what open-set identification (`open_set_metrics`), label cleaning (`label_suspects`) and hard-pair mining need, and what
    cannot be had from truncated top-K lists.  `classes` int [N]; a NEGATIVE class is "unlabelled / distractor": no mates, an impostor to
    everyone.  The score is that of `pairs_above` (dot product of the L2-normalised rows in `compute_dtype`); an item is never its own
    mate; a NaN score counts for nothing; ties go to the smallest partner index, -0.0 equals +0.0.  With `emb_b`, `classes_b` the
    result is for the rows of `emb` against the gallery `emb_b` (indices into `emb_b`).
    → Extremes(pos_score, pos_index, neg_score, neg_index, weak_score, weak_index): fp32 / int64 [N]; no such pair: index -1 and score
    -inf (weak_score: +inf); weak_* are None with weakest=False.
    CUDA tensors: pfr_class_extremes, the match GEMM with a class-conditioned atomic-max epilogue (one launch, or with `chunk` one per
    (row block, column block) as in `cluster`; with `emb_b` one per row block), then pfr_extremes_decode; nothing N x N is written.
    CPU tensors: chunked dense fp32 matmul, same contract.  Not covered: more than one extreme per item (`cosine_topk`)."""
    who = "class_extremes"
    _check_pair_sets(who, emb, emb_b, compute_dtype)
    _check_chunk(who, chunk)
    _check_classes(who, emb, classes, emb_b, classes_b)
    if not emb.is_cuda:
        return _class_extremes_torch(emb, classes, emb_b, classes_b, normalize, weakest)
    dev, sym = emb.device, emb_b is None
    N = emb.shape[0]
    nk = 3 if weakest else 2
    keys = torch.zeros(nk, max(N, 1), dtype=torch.int64, device=dev)
    Nb = N if sym else emb_b.shape[0]
    if N and Nb and not (sym and N == 1):
        T = dtype_id(compute_dtype)
        a, sa = _hist_operand(emb, compute_dtype, normalize)
        ca = classes.to(device=dev, dtype=torch.int32).contiguous()
        tail = (keys[0].data_ptr(), keys[1].data_ptr(), keys[2].data_ptr() if weakest else 0, N, _stream())
        if sym:
            _block_launches(lib.pfr_class_extremes, a, sa, N, chunk, (T, a.shape[1]), tail,
                            block_head=lambda r0, c0: (ca[r0:].data_ptr(), 0 if c0 is None else ca[c0:].data_ptr(), 1))
        else:
            b, sb = _hist_operand(emb_b.to(dev), compute_dtype, normalize)
            cb = classes_b.to(device=dev, dtype=torch.int32).contiguous()
            step = N if chunk is None else int(chunk)
            for r0 in range(0, N, step):
                lib.pfr_class_extremes(a[r0:].data_ptr(), 0 if sa is None else sa[r0:].data_ptr(), min(step, N - r0), r0, b.data_ptr(),
                                       0 if sb is None else sb.data_ptr(), Nb, 0, T, a.shape[1], ca[r0:].data_ptr(), cb.data_ptr(), 0, *tail)
    out = []
    for k in range(nk):
        score = torch.empty(N, dtype=torch.float32, device=dev)
        index = torch.empty(N, dtype=torch.int32, device=dev)
        lib.pfr_extremes_decode(keys[k].data_ptr(), N, 1 if k == 2 else 0, score.data_ptr(), index.data_ptr(), _stream())
        out += [score, index.long()]
    return Extremes(*out, *(() if weakest else (None, None)))


def open_set_metrics(emb, classes, fpir=(0.1, 0.01), emb_b=None, classes_b=None, compute_dtype=torch.float32, normalize=True):
    """Open-set identification (engine.metrics.OpenSetStats over `class_extremes`): 'rank1', and per false-positive identification rate f
    'DIR@FPIR={f}' — the share of the probes with a mate whose best mate comes back at rank 1 at or above the threshold that raises a
    false alarm for at most f of the searches without a mate — and 'TH@FPIR={f}', that threshold (on the score).  FNIR = 1 - DIR."""
    from ..engine.metrics import OpenSetStats
    ex = class_extremes(emb, classes, emb_b, classes_b, compute_dtype=compute_dtype, normalize=normalize, weakest=False)
    return OpenSetStats(ex.pos_score, ex.pos_index, ex.neg_score, ex.neg_index).metrics(fpir)


def label_suspects(extremes):
    """Label suspects for dataset cleaning: → int64 indices of the items WITH a mate whose best impostor ranks before their best mate
    (score descending, then index ascending), sorted by neg_score - pos_score descending, then by index."""
    ps, pi = extremes.pos_score.detach().cpu().float(), extremes.pos_index.detach().cpu().long()
    ns, ni = extremes.neg_score.detach().cpu().float(), extremes.neg_index.detach().cpu().long()
    idx = ((pi >= 0) & (ni >= 0) & ((ns > ps) | ((ns == ps) & (ni < pi)))).nonzero(as_tuple=True)[0]
    order = torch.sort(ns[idx] - ps[idx], descending=True, stable=True).indices
    return idx[order]


def cluster_metrics(labels, classes):
    """Clustering against the class labels (engine.metrics.ClusterStats): pairwise precision / recall / F, BCubed precision / recall / F,
    `clusters` and `singletons`, from the contingency counts of the N (cluster, class) pairs in exact int64 arithmetic; nothing
    cluster x class is built.  A ratio with a zero denominator is NaN."""
    from ..engine.metrics import ClusterStats
    return ClusterStats(labels, classes).metrics()


# ---- k-reciprocal re-ranking -----------------------------------------------------------------------------------------------------
#: workspace limit of `rerank` on the device: the sparse V and V' rows take N * (E + E2) * 8 bytes
RERANK_WORKSPACE_BUDGET = 16 << 30
#: the CPU path is dense (an N x N fp32 matrix for V and V'): it refuses larger sets
RERANK_CPU_MAX_ITEMS = 4096


def rerank_row_capacity(k1, k2):
    """(E, E2): the row lengths of the sparse V and V' rows for (k1, k2) — pfr_rerank_row_capacity of include/pfr_hip.h (host arithmetic)"""
    e, e2 = ctypes.c_int(0), ctypes.c_int(0)
    lib.pfr_rerank_row_capacity(int(k1), int(k2), ctypes.addressof(e), ctypes.addressof(e2))
    return e.value, e2.value


def _pad_lists(sc, idx, width):
    """(scores, idx) lists cut or padded (−inf / −1) to `width` columns"""
    sc, idx = sc[:, :width], idx[:, :width].int()
    pad = width - sc.shape[1]
    if pad > 0:
        sc = torch.cat([sc, torch.full((sc.shape[0], pad), -float("inf"), dtype=sc.dtype, device=sc.device)], 1)
        idx = torch.cat([idx, torch.full((idx.shape[0], pad), -1, dtype=torch.int32, device=idx.device)], 1)
    return sc.float().contiguous(), idx.contiguous()


def _unit_rows(x):
    x32 = x.float().contiguous()
    if x32.is_cuda and x32.shape[0]:
        return ops.l2norm_fwd(x32, torch.float32)[0]
    return x32 / x32.norm(dim=1, keepdim=True).clamp_min(1e-12)


def _check_rerank_sizes(k, k1, k2, lambda_value):
    if k > 512:
        raise PfrError(f"rerank: k={k} exceeds the 512-entry running list of the gfx950 top-K kernels")
    if k1 < 1 or k1 + 1 > 512:
        raise PfrError(f"rerank: k1={k1} must be >= 1 and k1 + 1 <= 512 (the neighbour lists are running top-K lists)")
    if k2 < 1:
        raise PfrError(f"rerank: k2={k2} must be >= 1")
    if not 0.0 <= float(lambda_value) <= 1.0:
        raise PfrError(f"rerank: lambda_value={lambda_value} must be in [0, 1]")


def rerank_inputs(emb, k, k1=20, candidates=None, emb_b=None, compute_dtype=torch.bfloat16, neighbors=None):
    """The inputs of the re-ranking contract (include/pfr_hip.h, pfr_rerank_*) from embeddings, through `cosine_topk`:
    → (emb32 [N, D] unit fp32 rows of the set — with emb_b the union, queries first, nbr [N, k1 + 1] int32, rows [R] int32,
       cand [R, kc] int32 in the set's numbering, cand_cos [R, kc] fp32, offset to subtract from returned indices (0, or len(emb))).
    The lists are those of `cosine_topk(emb32, emb32, ·, exclude_self=True, normalize=False)` — with a reduced compute_dtype re-scored exactly
    in fp32 — so the cosines are the fp32 dot products of the rows the weights are computed from."""
    _check_rerank_sizes(k, k1, 1, 0.0)
    Nq = emb.shape[0]
    X = emb if emb_b is None else torch.cat([emb.float(), emb_b.float().to(emb.device)], 0)
    N = X.shape[0]
    dev = X.device
    emb32 = _unit_rows(X)
    others = N - 1 if emb_b is None else N - Nq
    if candidates is not None and candidates > 512:
        raise PfrError(f"rerank: candidates={candidates} exceeds the 512-entry running list of the gfx950 top-K kernels")
    kc = max(0, min(max(k, 100) if candidates is None else int(candidates), 512, others))
    want = min(max(k1, kc) if emb_b is None else k1, N - 1)
    if neighbors is not None:
        sc, idx = neighbors
        if sc.shape[0] != N or idx.shape != sc.shape or sc.shape[1] < want:
            raise PfrError(f"rerank: neighbors must be the (cos, idx) lists [{N}, >= {want}] of cosine_topk(x, x, m, exclude_self=True) "
                           f"on the whole set (queries first, then emb_b)")
        sc, idx = sc.to(dev), idx.to(dev)
    elif want > 0:
        sc, idx = cosine_topk(emb32, emb32, want, compute_dtype=compute_dtype if emb32.is_cuda else torch.float32, exclude_self=True,
                              normalize=False)
    else:
        sc, idx = torch.empty((N, 0), device=dev), torch.empty((N, 0), dtype=torch.int32, device=dev)
    _, nb = _pad_lists(sc, idx, k1)
    nbr = torch.cat([torch.arange(N, dtype=torch.int32, device=dev)[:, None], nb], 1).contiguous()
    if emb_b is None:
        cand_cos, cand = _pad_lists(sc, idx, kc)
        return emb32, nbr, torch.arange(N, dtype=torch.int32, device=dev), cand, cand_cos, 0
    if kc > 0 and Nq > 0:
        gs, gi = cosine_topk(emb32[:Nq], emb32[Nq:], kc, compute_dtype=compute_dtype if emb32.is_cuda else torch.float32, normalize=False)
    else:
        gs, gi = torch.empty((Nq, 0), device=dev), torch.empty((Nq, 0), dtype=torch.int32, device=dev)
    cand_cos, cand = _pad_lists(gs, gi, kc)
    cand = torch.where(cand >= 0, cand + Nq, cand).contiguous()
    return emb32, nbr, torch.arange(Nq, dtype=torch.int32, device=dev), cand, cand_cos, Nq


def rerank_lists(emb32, nbr, rows, cand, cand_cos, k, k1=20, k2=6, lambda_value=0.3):
    """Steps 1-4 of the re-ranking contract (include/pfr_hip.h, pfr_rerank_*) on given lists → (dist [R, k] fp32 ascending, idx [R, k] int32,
    +inf / −1 padded).  CUDA tensors: pfr_rerank_expand → pfr_rerank_average → pfr_rerank_score with sparse rows of E and E2 = k2 · E entries
    (`rerank_row_capacity`).  CPU tensors: a dense torch restatement for at most RERANK_CPU_MAX_ITEMS items."""
    _check_rerank_sizes(k, k1, k2, lambda_value)
    N, D = emb32.shape
    R, kc = cand.shape
    if nbr.shape != (N, k1 + 1) or cand_cos.shape != cand.shape or rows.numel() != R:
        raise PfrError(f"rerank_lists: nbr must be [{N}, {k1 + 1}], cand and cand_cos [R, kc], rows [R]")
    if kc > 512:
        raise PfrError(f"rerank_lists: kc={kc} exceeds the 512-entry running list of the gfx950 top-K kernels")
    dev = emb32.device
    dist = torch.full((R, k), float("inf"), dtype=torch.float32, device=dev)
    out = torch.full((R, k), -1, dtype=torch.int32, device=dev)
    kk = min(k, kc)
    if R == 0 or kk == 0 or N == 0:
        return dist, out
    if not emb32.is_cuda:
        if N > RERANK_CPU_MAX_ITEMS:
            raise PfrError(f"rerank: the CPU path is dense (N x N) and takes at most {RERANK_CPU_MAX_ITEMS} items, got {N}; "
                           f"the sparse path runs on the gfx950 device")
        d, i = _rerank_lists_torch(emb32.float(), nbr, rows, cand, cand_cos.float(), kk, k1, k2, float(lambda_value))
        dist[:, :kk], out[:, :kk] = d, i
        return dist, out
    E, E2 = rerank_row_capacity(k1, k2)
    need = N * (E + E2) * 8
    if need > RERANK_WORKSPACE_BUDGET:
        raise PfrError(f"rerank: the workspace N * (E + E2) * 8 = {N} * ({E} + {E2}) * 8 = {need} bytes exceeds the budget of "
                       f"{RERANK_WORKSPACE_BUDGET} bytes (match.RERANK_WORKSPACE_BUDGET); lower k1 / k2 or split the set")
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()
    e32, nbr, rows, cand = emb32.float().contiguous(), i32(nbr), i32(rows), i32(cand)
    cand_cos = cand_cos.to(device=dev, dtype=torch.float32).contiguous()
    v_idx = torch.empty((N, E), dtype=torch.int32, device=dev)
    v_val = torch.empty((N, E), dtype=torch.float32, device=dev)
    q_idx = torch.empty((N, E2), dtype=torch.int32, device=dev)
    q_val = torch.empty((N, E2), dtype=torch.float32, device=dev)
    v_cnt = torch.empty(N, dtype=torch.int32, device=dev)
    q_cnt = torch.empty(N, dtype=torch.int32, device=dev)
    lib.pfr_rerank_expand(e32.data_ptr(), N, D, nbr.data_ptr(), k1, v_idx.data_ptr(), v_val.data_ptr(), v_cnt.data_ptr(), E, _stream())
    lib.pfr_rerank_average(nbr.data_ptr(), N, k1, k2, v_idx.data_ptr(), v_val.data_ptr(), v_cnt.data_ptr(), E, q_idx.data_ptr(),
                           q_val.data_ptr(), q_cnt.data_ptr(), E2, _stream())
    d = torch.empty((R, kk), dtype=torch.float32, device=dev)
    i = torch.empty((R, kk), dtype=torch.int32, device=dev)
    lib.pfr_rerank_score(q_idx.data_ptr(), q_val.data_ptr(), q_cnt.data_ptr(), N, E2, rows.data_ptr(), R, cand.data_ptr(), cand_cos.data_ptr(),
                         kc, float(lambda_value), kk, d.data_ptr(), i.data_ptr(), _stream())
    if kk == k:
        return d, i
    dist[:, :kk], out[:, :kk] = d, i
    return dist, out


def _rerank_lists_torch(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lam):
    """dense CPU form of the contract in matrix algebra: membership, R, R*, V and V' as N x N matrices (no per-item set logic)"""
    N, K1 = emb32.shape[0], nbr.shape[1]
    kh = round(k1 / 2)
    nb = nbr.long()
    valid = (nb >= 0) & (nb < N)
    rank = valid.cumsum(1) - 1                                     # position among the valid entries of the row
    row_of = torch.arange(N)[:, None].expand_as(nb)

    def member(width):                                             # A[i, j] = j is among the first `width` valid entries of nbr[i]
        A = torch.zeros((N, N), dtype=torch.bool)
        sel = valid & (rank < width)
        A[row_of[sel], nb[sel]] = True
        return A
    A1, Ah = member(k1 + 1), member(kh + 1)
    B1, Bh = A1 & A1.t(), Ah & Ah.t()                              # R(i, k1) and R(i, kh) as rows; both symmetric
    B1f, Bhf = B1.float(), Bh.float()
    inter = B1f @ Bhf                                              # [i, j] = |R(i, k1) ∩ R(j, kh)|  (small integers: exact)
    accept = B1 & (3 * inter > 2 * Bhf.sum(0)[None, :])
    Rs = B1 | ((accept.float() @ Bhf) > 0)
    W = torch.where(Rs, torch.exp(-(2 - 2 * (emb32 @ emb32.t()))), torch.zeros(()))
    V = W / W.sum(1, keepdim=True).clamp_min(1e-30)
    sel = valid & (rank < k2)
    Vq = torch.zeros_like(V)
    for t in range(K1):                                            # (in list order, as the kernel sums)
        s = sel[:, t]
        if bool(s.any()):
            Vq[s] += V[nb[s, t]]
    Vq /= sel.sum(1).clamp_min(1)[:, None]
    R, kc = cand.shape
    rw, c = rows.long(), cand.long()
    ok = (c >= 0) & (c < N) & ((rw >= 0) & (rw < N))[:, None]
    rw, cc = rw.clamp(0, N - 1), c.clamp(0, N - 1)
    dist = torch.empty((R, k), dtype=torch.float32)
    idx = torch.empty((R, k), dtype=torch.int32)
    step = max(1, (1 << 24) // max(1, kc * N))
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        m = torch.minimum(Vq[rw[r0:r1], None, :], Vq[cc[r0:r1]]).sum(2)
        fin = (1 - lam) * (1 - m / (2 - m)) + lam * (2 - 2 * cand_cos[r0:r1])
        fin = torch.where(ok[r0:r1], fin, torch.full_like(fin, float("inf")))
        order = torch.argsort(fin, dim=1, stable=True)[:, :k]
        dist[r0:r1] = torch.gather(fin, 1, order)
        idx[r0:r1] = torch.where(torch.gather(ok[r0:r1], 1, order), torch.gather(c[r0:r1], 1, order), torch.full_like(order, -1)).int()
    return dist, idx


def rerank(emb, k, k1=20, k2=6, lambda_value=0.3, candidates=None, emb_b=None, compute_dtype=torch.bfloat16, neighbors=None):
    """k-reciprocal re-ranking (Zhong et al., CVPR 2017) of the cosine match lists → (dist [R, k] fp32 ascending, idx [R, k] int32; +inf / −1
    padded when fewer than k candidates exist).  dist = (1 − lambda_value) · Jaccard distance of the expanded k-reciprocal neighbour
    encodings + lambda_value · (2 − 2 cos); the exact contract is the comment at pfr_rerank_* in include/pfr_hip.h.
    One set (`emb` [N, D]): all-vs-all, self excluded from the candidates, as in `recall_at_k`.
    With `emb_b` (the gallery): the set is the union, queries first; the output rows are the queries, the candidates each query's
    top-`candidates` gallery rows, and idx is in gallery numbering.
    candidates (default max(k, 100), capped at 512 and at the number of other items): ONLY these are re-ranked.  This equals re-ranking every
    item only when the list covers every other item: an item outside the list that shares neighbours with the query (non-zero overlap)
    could otherwise enter the top k.
    neighbors = (cos, idx): the `cosine_topk(x, x, m, exclude_self=True)` lists of the whole set already computed (m >= k1, and in the
    one-set form m >= candidates: they provide the candidates too).  compute_dtype is passed to `cosine_topk`, whose lists are re-scored
    exactly in fp32.
    Deviation from the published code: its division of the distance matrix by the per-column maximum needs the N x N matrix and is dropped.
    CUDA tensors run the sparse gfx950 kernels (workspace N · (E + E2) · 8 bytes, limited by RERANK_WORKSPACE_BUDGET); CPU tensors a dense
    torch form for at most RERANK_CPU_MAX_ITEMS items."""
    _check_rerank_sizes(k, k1, k2, lambda_value)
    emb32, nbr, rows, cand, cand_cos, off = rerank_inputs(emb, k, k1, candidates, emb_b, compute_dtype, neighbors)
    dist, idx = rerank_lists(emb32, nbr, rows, cand, cand_cos, k, k1, k2, lambda_value)
    if off:
        idx = torch.where(idx >= 0, idx - off, idx)
    return dist, idx


_rerank = rerank      # (recall_at_k has a parameter of this name)
