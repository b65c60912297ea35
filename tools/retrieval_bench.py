"""Cost of the exact retrieval ranks behind mAP / CMC / mINP (match.retrieval_metrics -> pfr_pair_scores_gather + pfr_rank_count):
symmetric, D = 512, classes of 5 (4 positives per query), N = 20 000 and 100 000 embeddings, bf16 and int8 operands, on two data sets:
  random      L2-normalised random rows with the same class layout: a positive scores like any other item, so four in five of all
              scores are at or above the weakest of their row's 4 positives and take the slow path of the epilogue
  clustered   tight classes (class centre + 2 % noise): the positives are the best items of their row and almost every score is
              dismissed with one compare
Per (N, dtype) these legs run interleaved round by round in one process:
  metrics_*     match.retrieval_metrics end to end from the fp32 embeddings (operand preparation, positive lists, the threshold gather, the
                count launch, the float64 sums on the host)
  count_*       the pfr_rank_count launch alone with its zeroing (prepared operands, thresholds already gathered)
  gemm_plain    the plain score GEMM of the same FLOPs: N x N scores written as fp32 in column chunks into one reused buffer (int8:
                pfr_match_scores_i8; bf16: pfr_conv2d_fwd as a GEMM, the match's own unfused call) — what the epilogue costs
  torch_dense   the same contract in torch on the same card: row chunks of a @ a.T in bf16, the gathered positives' scores as thresholds,
                the precede compares, a sum per threshold (bf16 rows only; once per round; random rows — its cost does not depend on the data)
slow_share = the share of the N (N - 1) scores with s >= the smallest threshold of their row, from the torch leg's own bf16 scores.
Writes profiles/retrieval.txt.
    python tools/retrieval_bench.py [--sizes 20000 100000] [--rounds 3] [--steps 3] [--out PATH]"""
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

D, PER_CLASS = 512, 5


def make_inputs(N, dev):
    g = torch.Generator().manual_seed(7)
    cls = torch.arange(N) // PER_CLASS
    rnd = torch.randn(N, D, generator=g)
    centres = torch.nn.functional.normalize(torch.randn(int(cls.max()) + 1, D, generator=g), dim=1)
    clu = centres[cls] + 0.02 / D ** 0.5 * torch.randn(N, D, generator=g)       # noise vector of length ~0.02 next to a unit centre
    return rnd.to(dev), clu.to(dev), cls.to(dev)


def torch_dense(ab, col, npos, want_share=False, R=2048):
    """chunked dense counting in torch: -> (cnt int64 [N, P], number of scores at or above their row's smallest threshold)"""
    N, P = col.shape
    dev = ab.device
    ids = torch.arange(N, device=dev)
    cnt = torch.zeros((N, P), dtype=torch.int64, device=dev)
    slow = 0
    for r0 in range(0, N, R):
        s = (ab[r0:r0 + R] @ ab.t()).float()
        cc = col[r0:r0 + R]
        thr = torch.gather(s, 1, cc.clamp_min(0))
        keep = ids[None, :] != torch.arange(r0, r0 + s.shape[0], device=dev)[:, None]
        for k in range(P):
            t, ti = thr[:, k:k + 1], cc[:, k:k + 1]
            pre = ((s > t) | ((s == t) & (ids[None, :] < ti))) & keep & (k < npos[r0:r0 + R, None])
            cnt[r0:r0 + R, k] = pre.sum(dim=1)
        if want_share:
            tmin = torch.where(cc >= 0, thr, torch.full_like(thr, float("inf"))).min(dim=1, keepdim=True).values
            slow += int(((s >= tmin) & keep).sum())
    return cnt, slow


def build_cases(N, dt, dev):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import lib, dtype_id, ops
    rnd, clu, cls = make_inputs(N, dev)
    st = lambda: torch.cuda.current_stream().cuda_stream
    T = dtype_id(dt)
    ids = torch.arange(N, dtype=torch.int32, device=dev)
    col, npos = match._positive_lists(cls, cls, True)
    col32, tc = col.int().contiguous(), npos.int().contiguous()
    P = col.shape[1]
    assert P == PER_CLASS - 1 and P <= match.rank_count_max_thr()
    prepared, thr = {}, {}
    for name, x in (("random", rnd), ("clustered", clu)):
        a, sa = match._hist_operand(x, dt, True)
        t = torch.zeros((N, P), dtype=torch.float32, device=dev)
        lib.pfr_pair_scores_gather(a.data_ptr(), 0 if sa is None else sa.data_ptr(), N, 0, 0, 0, T, a.shape[1], col32.data_ptr(), P,
                                   t.data_ptr(), st())
        prepared[name], thr[name] = (a, sa), t
    cnt = torch.zeros((N, P), dtype=torch.int32, device=dev)

    def count_case(name):
        a, sa = prepared[name]

        def run():
            cnt.zero_()
            lib.pfr_rank_count(a.data_ptr(), 0 if sa is None else sa.data_ptr(), N, 0, 0, ids.data_ptr(), 0, T, a.shape[1], ids.data_ptr(),
                               thr[name].data_ptr(), col32.data_ptr(), tc.data_ptr(), P, cnt.data_ptr(), st())
            return cnt
        return run

    def metrics_case(x):
        return lambda: match.retrieval_metrics(x, cls, compute_dtype=dt)

    a, sa = prepared["random"]
    chunk = 4096
    sbuf = torch.empty((N, 1, 1, chunk), dtype=torch.float32, device=dev)

    def gemm_plain():
        for c0 in range(0, N, chunk):
            n = min(chunk, N - c0)
            if dt == torch.int8:
                lib.pfr_match_scores_i8(a.data_ptr(), sa.data_ptr(), a[c0].data_ptr(), sa[c0].data_ptr(), N, n, a.shape[1], sbuf.data_ptr(),
                                        chunk, st())
            else:
                ops.conv2d_fwd(a.view(N, 1, 1, D), a[c0:c0 + n].view(n, 1, 1, D), out=sbuf)

    cases = {"metrics_random": metrics_case(rnd), "metrics_clustered": metrics_case(clu), "count_random": count_case("random"),
             "count_clustered": count_case("clustered"), "gemm_plain": gemm_plain}
    extra = {}
    if dt == torch.bfloat16:
        cases["torch_dense"] = lambda: torch_dense(prepared["random"][0], col, npos)[0]
        # the slow-path share of both data sets, from the torch leg's own scores (not timed)
        for name in ("random", "clustered"):
            _, slow = torch_dense(prepared[name][0], col, npos, want_share=True)
            extra[f"slow_share_{name}"] = round(slow / (N * (N - 1.0)), 5)
    return cases, extra, (match, cls, dt, clu, cnt, tc)


def run(N, dt, args, dev):
    cases, extra, (match, cls, dt, clu, cnt, tc) = build_cases(N, dt, dev)
    for name, fn in cases.items():          # warm-up of every shape
        out = fn()
        torch.cuda.synchronize()
        if name == "metrics_clustered":
            assert out["queries"] == N and out["mAP"] == 1.0 and out["CMC@K=1"] == 1.0, out
        if name == "count_clustered":       # the bare launch gives the ranks the wrapper reports
            ranks, _ = match.positive_ranks(clu, cls, compute_dtype=dt)
            assert torch.equal(ranks, (out + 1).sort(dim=1).values.int())
    ms = {n: [] for n in cases}
    order = list(cases)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            steps = 1 if name == "torch_dense" else args.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                cases[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    res = {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for n, v in ms.items()}
    flop = 2.0 * N * N * D
    for n in ("count_random", "count_clustered"):
        res[n]["tera_ops"] = round(flop / (res[n]["median_ms"] * 1e-3) / 1e12, 1)
        res[n]["vs_gemm_plain"] = round(res[n]["median_ms"] / res["gemm_plain"]["median_ms"], 3)
    for n in ("metrics_random", "metrics_clustered"):
        res[n]["vs_gemm_plain"] = round(res[n]["median_ms"] / res["gemm_plain"]["median_ms"], 3)
    res["count_random"]["vs_count_clustered"] = round(res["count_random"]["median_ms"] / res["count_clustered"]["median_ms"], 3)
    if "torch_dense" in res:
        for n in ("metrics_random", "metrics_clustered", "count_random", "count_clustered"):
            res["torch_dense"][f"vs_{n}"] = round(res["torch_dense"]["median_ms"] / res[n]["median_ms"], 2)
        res["torch_dense"].update(extra)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retrieval_bench.py needs an MI355X")
    dev = torch.device("cuda", 0)
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "D": D, "per_class": PER_CLASS,
           "rounds": args.rounds, "steps_per_round": args.steps, "results": {}}
    lines = [f"# tools/retrieval_bench.py  {out['date']}  {out['device']}  symmetric, D={D}, classes of {PER_CLASS}; {args.rounds} interleaved "
             f"rounds x {args.steps} calls (torch_dense: 1), median (min) ms; tera_ops = 2 N^2 D / time; vs_* = ratio of medians"]
    for N in args.sizes:
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.int8, "int8")):
            res = run(N, dt, args, dev)
            out["results"][f"{N}_{tag}"] = res
            lines.append(f"N = {N}  {tag}  ({N * (N - 1):.3e} scores, {N * (PER_CLASS - 1)} thresholds)")
            for name, r in res.items():
                extra = "  ".join(f"{k}={v}" for k, v in r.items() if k not in ("median_ms", "min_ms"))
                lines.append(f"  {name:18s} {r['median_ms']:10.3f} ({r['min_ms']:10.3f}) ms  {extra}")
            torch.cuda.empty_cache()
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
