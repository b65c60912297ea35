"""Cost of the k-reciprocal re-ranking (match.rerank -> pfr_rerank_expand / _average / _score): D = 512, k1 = 20, k2 = 6, 100 candidates per
row, top 10 kept, all-vs-all on a random set and on a clustered set (classes of 20 tight items: large R*).  Per (N, set) these legs run
interleaved round by round in one process:
  sparse   match.rerank_lists on the lists below: the three sparse kernels (what re-ranking ADDS to a match)
  topk     match.cosine_topk(x, x, 100, exclude_self=True) of the same set in bf16 with the exact re-scoring: the first stage that produces
           the lists; `sparse` is reported as a multiple of it
  dense    a dense torch implementation of the same contract on the same card (N x N fp32 matrices for the scores, R*, V and V'; the
           Jaccard overlaps in row chunks), only for N <= --dense-max where N x N fits; once per round
The lists (nbr, cand, cand_cos) are computed once outside the timed windows and shared by `sparse` and `dense`; their results are compared.
Writes profiles/rerank.txt.
    python tools/rerank_bench.py [--sizes 20000 100000] [--dense-max 20000] [--rounds 9] [--steps 10] [--out PATH]
Every leg is timed on the host around `steps` back-to-back calls between two device synchronisations (launch and allocation included: what a
caller pays); the file gives the median, the minimum and the maximum over the rounds."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, K1, K2, KC, K, LAM = 512, 20, 6, 100, 10, 0.3


def make_set(kind, N, dev):
    g = torch.Generator().manual_seed(11)
    if kind == "random":
        return torch.randn(N, D, generator=g).to(dev)
    cls = torch.arange(N) // 20
    return (torch.randn((N + 19) // 20, D, generator=g)[cls] + 0.02 * torch.randn(N, D, generator=g)).to(dev)


def dense_rerank(emb32, nbr, cand, cand_cos, k, k1, k2, lam, row_chunk=64):
    """the contract of include/pfr_hip.h with N x N matrices (all rows are output rows)"""
    N = emb32.shape[0]
    dev = emb32.device
    kh = round(k1 / 2)
    ar = torch.arange(N, device=dev)

    def member(width):              # A[i, j] = j among the first `width` valid entries of nbr[i] (the lists of this tool have no inner padding)
        A = torch.zeros((N, N), dtype=torch.bool, device=dev)
        cols = nbr[:, :width].long()
        ok = cols >= 0
        A[ar[:, None].expand_as(cols)[ok], cols[ok]] = True
        return A
    A1, Ah = member(k1 + 1), member(kh + 1)
    B1, Bh = A1 & A1.t(), Ah & Ah.t()
    del A1, Ah
    B1h, Bhh = B1.to(torch.bfloat16), Bh.to(torch.bfloat16)                 # (0 / 1 and counts <= k1 + 1: exact in bf16 with fp32 accumulation)
    inter = B1h @ Bhh                                                        # |R(j, kh) ∩ R(i, k1)| (Bh is symmetric)
    size = Bh.sum(1)
    accept = B1 & (3 * inter.float() > 2 * size[None, :].float())
    Rs = B1 | ((accept.to(torch.bfloat16) @ Bhh) > 0)
    del B1, Bh, B1h, Bhh, inter, accept
    W = torch.exp(-(2 - 2 * (emb32 @ emb32.t())))
    W = torch.where(Rs, W, torch.zeros((), device=dev))
    del Rs
    V = W / W.sum(1, keepdim=True)
    del W
    Vq = torch.zeros_like(V)
    cnt = torch.zeros(N, device=dev)
    for t in range(k2):
        n = nbr[:, t].long()
        ok = n >= 0
        Vq[ok] += V[n[ok]]
        cnt += ok
    Vq /= cnt.clamp_min(1)[:, None]
    del V
    dist = torch.empty((N, k), dtype=torch.float32, device=dev)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    for r0 in range(0, N, row_chunk):
        c = cand[r0:r0 + row_chunk].long()
        m = torch.minimum(Vq[r0:r0 + row_chunk, None, :], Vq[c.clamp_min(0)]).sum(2)
        fin = (1 - lam) * (1 - m / (2 - m)) + lam * (2 - 2 * cand_cos[r0:r0 + row_chunk])
        fin = torch.where(c >= 0, fin, torch.full_like(fin, float("inf")))
        order = torch.argsort(fin, dim=1, stable=True)[:, :k]
        dist[r0:r0 + row_chunk] = torch.gather(fin, 1, order)
        idx[r0:r0 + row_chunk] = torch.gather(c, 1, order).int()
    return dist, idx


def run(N, kind, args, dev):
    from pets_face_recognition_amd import match
    x = make_set(kind, N, dev)
    emb32, nbr, rows, cand, cand_cos, _ = match.rerank_inputs(x, K, k1=K1, candidates=KC)
    legs = {"sparse": lambda: match.rerank_lists(emb32, nbr, rows, cand, cand_cos, K, K1, K2, LAM),
            "topk": lambda: match.cosine_topk(emb32, emb32, KC, exclude_self=True, normalize=False)}
    if N <= args.dense_max:
        legs["dense"] = lambda: dense_rerank(emb32, nbr, cand, cand_cos, K, K1, K2, LAM)
    outs = {}
    for name, fn in legs.items():           # warm-up of every shape
        outs[name] = fn()
        torch.cuda.synchronize()
    res = {}
    if "dense" in outs:
        (ds, is_), (dd, id_) = outs["sparse"], outs["dense"]
        res["agreement"] = {"same_idx_fraction": round(float((is_ == id_).float().mean()), 6),
                            "max_abs_dist_diff": float((ds - dd).abs()[torch.isfinite(dd)].max())}
    res["changed_rows_fraction"] = round(float((outs["sparse"][1] != cand[:, :K]).any(1).float().mean()), 4)
    del outs
    ms = {n: [] for n in legs}
    order = list(legs)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            steps = 1 if name == "dense" else args.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                legs[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    for n, v in ms.items():
        res[n] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    res["sparse"]["vs_topk"] = round(res["sparse"]["median_ms"] / res["topk"]["median_ms"], 2)
    if "dense" in res:
        res["dense"]["vs_sparse"] = round(res["dense"]["median_ms"] / res["sparse"]["median_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--dense-max", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rerank_bench.py needs an MI355X")
    dev = torch.device("cuda", 0)
    from pets_face_recognition_amd.match import rerank_row_capacity
    E, E2 = rerank_row_capacity(K1, K2)
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "D": D, "k1": K1, "k2": K2, "candidates": KC,
           "k": K, "lambda": LAM, "E": E, "E2": E2, "rounds": args.rounds, "steps_per_round": args.steps, "results": {}}
    lines = [f"# tools/rerank_bench.py  {out['date']}  {out['device']}  all-vs-all, D={D}, k1={K1}, k2={K2}, candidates={KC}, k={K}, "
             f"lambda={LAM} (E={E}, E2={E2}); {args.rounds} interleaved rounds x {args.steps} calls (dense: 1), median (min .. max) ms over the rounds"]
    for N in args.sizes:
        for kind in ("random", "clustered"):
            res = run(N, kind, args, dev)
            out["results"][f"{N}_{kind}"] = res
            lines.append(f"N = {N}  {kind}  (rows whose top {K} changed: {res['changed_rows_fraction']}"
                         + (f"; sparse vs dense: {res['agreement']}" if "agreement" in res else "") + ")")
            for name in ("sparse", "topk", "dense"):
                if name in res:
                    r = res[name]
                    extra = "  ".join(f"{k}={v}" for k, v in r.items() if k not in ("median_ms", "min_ms", "max_ms"))
                    lines.append(f"  {name:7s} {r['median_ms']:10.3f} ({r['min_ms']:10.3f} .. {r['max_ms']:10.3f}) ms  {extra}")
            torch.cuda.empty_cache()
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
