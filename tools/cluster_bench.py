"""Cost of the threshold clustering (match.cluster / match.pairs_above -> pfr_pairs_above): symmetric, D = 512, N = 20 000 and 100 000
embeddings in shuffled order, bf16 and int8 operands, threshold cos >= 0.5.  Per (N, dtype) these legs run interleaved round by round in
one process:
  cluster_5         match.cluster end to end (operand preparation, union launch, flatten, status read) on tight classes of 5
  union_5           the pfr_pairs_above launch with the union-find epilogue alone (plus the reset of the parent array)
  cluster_50        the same on tight classes of 50: 10 x the qualifying pairs, longer hook chains
  union_50
  pairs_above_5     match.pairs_above end to end on the classes of 5 (append epilogue, count read, sort by (i, j))
  pair_hist         pfr_pair_hist on the same operands (4096 bins): the sibling epilogue, as it stands
  gemm_plain        the plain score GEMM of the same FLOPs: N x N/2 scores written as fp32 in column chunks into one reused buffer
                    (int8: pfr_match_scores_i8; bf16: pfr_conv2d_fwd as a GEMM)
  dense_5           the same contract in torch on the same card: row chunks of a @ a[r0:].T >= thr -> nonzero -> host union-find over the
                    edges (bf16 rows only; once per round)
The labels of every leg are checked against the classes before anything is timed.  Writes profiles/cluster.txt.
    python tools/cluster_bench.py [--sizes 20000 100000] [--rounds 3] [--steps 3] [--out PATH]"""
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

D, BINS, THR = 512, 4096, 0.5


def make_inputs(N, per, dev):
    """tight classes of `per` items around random centres, in shuffled order -> (rows, classes, expected labels)"""
    g = torch.Generator().manual_seed(7 + per)
    cls = (torch.arange(N) // per)[torch.randperm(N, generator=g)]
    x = torch.randn((N + per - 1) // per, D, generator=g)[cls] + 0.02 * torch.randn(N, D, generator=g)
    first = torch.full((int(cls.max()) + 1,), N, dtype=torch.int64).scatter_reduce(0, cls, torch.arange(N), "amin")
    return x.to(dev), cls.to(dev), first[cls].to(dev)


def build_cases(N, dt, dev):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import lib, dtype_id, ops
    st = lambda: torch.cuda.current_stream().cuda_stream
    T = dtype_id(dt)
    sets = {per: make_inputs(N, per, dev) for per in (5, 50)}
    prepared = {per: match._hist_operand(sets[per][0], dt, True) for per in sets}
    parent = torch.empty(N, dtype=torch.int32, device=dev)
    fresh = torch.arange(N, dtype=torch.int32, device=dev)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    checks = {}

    def cluster_case(per):
        return lambda: match.cluster(sets[per][0], THR, compute_dtype=dt)

    def union_case(per):
        a, sa = prepared[per]

        def run():
            parent.copy_(fresh)
            lib.pfr_pairs_above(a.data_ptr(), 0 if sa is None else sa.data_ptr(), N, 0, 0, 0, 0, 0, T, a.shape[1], THR, 0, 0, 0, 0, 0,
                                parent.data_ptr(), N, status.data_ptr(), st())
            return parent
        return run

    def union_labels(per):
        union_case(per)()
        lib.pfr_cc_flatten(parent.data_ptr(), N, labels.data_ptr(), st())
        assert int(status) == 0
        return labels.long()

    a, sa = prepared[5]
    cls32 = sets[5][1].int().contiguous()
    lo, inv_w = match._hist_range(BINS, (-1.0, 1.0))
    hist = torch.zeros((2, BINS + 1), dtype=torch.int64, device=dev)

    def pair_hist():
        hist.zero_()
        lib.pfr_pair_hist(a.data_ptr(), 0 if sa is None else sa.data_ptr(), cls32.data_ptr(), N, 0, 0, 0, 0, T, a.shape[1], lo, inv_w, BINS,
                          hist.data_ptr(), st())

    half, chunk = N // 2, 4096
    sbuf = torch.empty((N, 1, 1, chunk), dtype=torch.float32, device=dev)

    def gemm_plain():
        for c0 in range(0, half, chunk):
            n = min(chunk, half - c0)
            if dt == torch.int8:
                lib.pfr_match_scores_i8(a.data_ptr(), sa.data_ptr(), a[c0].data_ptr(), sa[c0].data_ptr(), N, n, a.shape[1], sbuf.data_ptr(),
                                        chunk, st())
            else:
                ops.conv2d_fwd(a.view(N, 1, 1, D), a[c0:c0 + n].view(n, 1, 1, D), out=sbuf)

    cases = {"cluster_5": cluster_case(5), "union_5": union_case(5), "cluster_50": cluster_case(50), "union_50": union_case(50),
             "pairs_above_5": lambda: match.pairs_above(sets[5][0], THR, compute_dtype=dt), "pair_hist": pair_hist,
             "gemm_plain": gemm_plain}
    for per in sets:
        checks[f"cluster_{per}"] = lambda per=per: torch.equal(cluster_case(per)(), sets[per][2])
        checks[f"union_{per}"] = lambda per=per: torch.equal(union_labels(per), sets[per][2])
    checks["pairs_above_5"] = lambda: cases["pairs_above_5"]()[0].numel() == (N // 5) * 10 + (N % 5) * (N % 5 - 1) // 2
    if dt == torch.bfloat16:
        R = 2048

        def dense_5():
            ii, jj = [], []
            for r0 in range(0, N, R):
                ok = (a[r0:r0 + R] @ a[r0:].t()).float() >= THR
                i, j = ok.nonzero(as_tuple=True)
                keep = j > i                                  # (column 0 of the block is row r0: the pairs i < j)
                ii.append(i[keep] + r0); jj.append(j[keep] + r0)
            return match._host_components(N, torch.cat(ii).cpu(), torch.cat(jj).cpu())
        cases["dense_5"] = dense_5
        checks["dense_5"] = lambda: torch.equal(dense_5(), sets[5][2].cpu())
    return cases, checks


def run(N, dt, args):
    cases, checks = build_cases(N, dt, torch.device("cuda", 0))
    for name, fn in cases.items():          # warm-up of every shape, and what the answers must be
        fn()
        torch.cuda.synchronize()
        if name in checks:
            assert checks[name](), name
    ms = {n: [] for n in cases}
    order = list(cases)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            steps = 1 if name == "dense_5" else args.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                cases[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    res = {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for n, v in ms.items()}
    for n in ("union_5", "union_50"):
        res[n]["vs_pair_hist"] = round(res[n]["median_ms"] / res["pair_hist"]["median_ms"], 3)
        res[n]["vs_gemm_plain"] = round(res[n]["median_ms"] / res["gemm_plain"]["median_ms"], 3)
    if "dense_5" in res:
        res["dense_5"]["vs_cluster_5"] = round(res["dense_5"]["median_ms"] / res["cluster_5"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench.py needs an MI355X")
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "D": D, "threshold": THR,
           "rounds": args.rounds, "steps_per_round": args.steps, "results": {}}
    lines = [f"# tools/cluster_bench.py  {out['date']}  {out['device']}  symmetric, D={D}, cos >= {THR}; {args.rounds} interleaved rounds x "
             f"{args.steps} calls (dense_5: 1), median (min) ms"]
    for N in args.sizes:
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.int8, "int8")):
            res = run(N, dt, args)
            out["results"][f"{N}_{tag}"] = res
            lines.append(f"N = {N}  {tag}  ({N * (N - 1) // 2:.3e} pairs)")
            for name, r in res.items():
                extra = "  ".join(f"{k}={v}" for k, v in r.items() if k not in ("median_ms", "min_ms"))
                lines.append(f"  {name:15s} {r['median_ms']:10.3f} ({r['min_ms']:10.3f}) ms  {extra}")
            torch.cuda.empty_cache()
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
