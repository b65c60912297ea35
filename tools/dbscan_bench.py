"""Cost of the DBSCAN clustering (match.dbscan -> pfr_neighbor_count, pfr_dbscan_link, pfr_dbscan_labels): symmetric, D = 512, N = 20 000
and 100 000 embeddings in shuffled order (the sets of tools/cluster_bench.py), bf16 and int8 operands, threshold cos >= 0.5, min_samples 4.
Per (N, dtype) these legs run interleaved round by round in one process:
  dbscan_5          match.dbscan end to end (operand preparation, both GEMM passes, label pass, status read) on tight classes of 5
  count_5           the pfr_neighbor_count launch alone (plus the reset of the degrees)
  link_5            the pfr_dbscan_link launch alone on finished degrees (plus the reset of parent and best)
  dbscan_50, count_50, link_50     the same on tight classes of 50: 10 x the qualifying pairs, longer hook chains
  union_5, union_50 the pfr_pairs_above launch with the union-find epilogue on the same operands (plus the reset of the parent array)
  pair_hist         pfr_pair_hist on the same operands (4096 bins): the sibling epilogue, as it stands
  dense_5           the same contract in torch on the same card: two sweeps of row chunks of a @ a.T >= thr (degrees; then core-core edges
                    and the best core neighbour), a host union-find over the edges (bf16 rows only; once per round)
The labels of every leg are checked against the classes before anything is timed.  Writes profiles/dbscan.txt.
    python tools/dbscan_bench.py [--sizes 20000 100000] [--rounds 3] [--steps 3] [--out PATH]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cluster_bench import make_inputs, D, BINS, THR

MIN_SAMPLES = 4


def build_cases(N, dt, dev):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import lib, dtype_id
    st = lambda: torch.cuda.current_stream().cuda_stream
    T, mn = dtype_id(dt), MIN_SAMPLES - 1
    sets, classes, want, want_deg = {}, {}, {}, {}
    for per in (5, 50):
        x, cls, first = make_inputs(N, per, dev)
        sets[per], classes[per] = x, cls
        want_deg[per] = torch.bincount(cls)[cls] - 1            # every class mate, nobody else
        want[per] = torch.where(want_deg[per] >= mn, first, torch.full_like(first, -1))     # (a short last class has no core: noise)
    prepared = {per: match._hist_operand(sets[per], dt, True) for per in sets}
    deg = {per: torch.zeros(N, dtype=torch.int32, device=dev) for per in sets}
    scratch_deg = torch.zeros(N, dtype=torch.int32, device=dev)
    parent = torch.empty(N, dtype=torch.int32, device=dev)
    fresh = torch.arange(N, dtype=torch.int32, device=dev)
    best = torch.zeros(N, dtype=torch.int64, device=dev)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()

    def count_case(per, out=None):
        a, sa = prepared[per]
        out = scratch_deg if out is None else out

        def run():
            out.zero_()
            lib.pfr_neighbor_count(a.data_ptr(), ptr(sa), N, 0, 0, 0, 0, 0, T, a.shape[1], THR, out.data_ptr(), N, st())
            return out
        return run

    def link_case(per):
        a, sa = prepared[per]

        def run():
            parent.copy_(fresh)
            best.zero_()
            lib.pfr_dbscan_link(a.data_ptr(), ptr(sa), N, 0, 0, 0, 0, 0, T, a.shape[1], THR, deg[per].data_ptr(), mn, parent.data_ptr(),
                                best.data_ptr(), N, status.data_ptr(), st())
            return parent
        return run

    def link_labels(per):
        link_case(per)()
        lib.pfr_dbscan_labels(parent.data_ptr(), deg[per].data_ptr(), best.data_ptr(), mn, N, labels.data_ptr(), st())
        assert int(status) == 0
        return labels.long()

    def union_case(per):
        a, sa = prepared[per]

        def run():
            parent.copy_(fresh)
            lib.pfr_pairs_above(a.data_ptr(), ptr(sa), N, 0, 0, 0, 0, 0, T, a.shape[1], THR, 0, 0, 0, 0, 0, parent.data_ptr(), N,
                                status.data_ptr(), st())
            return parent
        return run

    a, sa = prepared[5]
    cls32 = classes[5].int().contiguous()
    lo, inv_w = match._hist_range(BINS, (-1.0, 1.0))
    hist = torch.zeros((2, BINS + 1), dtype=torch.int64, device=dev)

    def pair_hist():
        hist.zero_()
        lib.pfr_pair_hist(a.data_ptr(), ptr(sa), cls32.data_ptr(), N, 0, 0, 0, 0, T, a.shape[1], lo, inv_w, BINS, hist.data_ptr(), st())

    cases, checks = {}, {}
    for per in sets:
        count_case(per, deg[per])()                              # the finished degrees the link legs read
        cases[f"dbscan_{per}"] = lambda per=per: match.dbscan(sets[per], THR, min_samples=MIN_SAMPLES, compute_dtype=dt)
        cases[f"count_{per}"] = count_case(per)
        cases[f"link_{per}"] = link_case(per)
        cases[f"union_{per}"] = union_case(per)
        checks[f"dbscan_{per}"] = lambda per=per: torch.equal(cases[f"dbscan_{per}"](), want[per])
        checks[f"count_{per}"] = lambda per=per: torch.equal(cases[f"count_{per}"]().long(), want_deg[per]) and \
            torch.equal(deg[per].long(), want_deg[per])
        checks[f"link_{per}"] = lambda per=per: torch.equal(link_labels(per), want[per])
    cases["pair_hist"] = pair_hist
    if dt == torch.bfloat16:
        R = 2048

        def dense_5():
            ar = torch.arange(N, device=dev)
            dg = torch.zeros(N, dtype=torch.int64, device=dev)
            for r0 in range(0, N, R):
                ok = (a[r0:r0 + R] @ a.t()).float() >= THR
                ok[ar[:ok.shape[0]], ar[r0:r0 + R]] = False                      # no self pair
                dg[r0:r0 + R] = ok.sum(dim=1)
            core = dg >= mn
            ii, jj = [], []
            bestc = torch.full((N,), -1, dtype=torch.int64, device=dev)
            for r0 in range(0, N, R):
                s = (a[r0:r0 + R] @ a.t()).float()
                ok = (s >= THR) & core[None, :]
                ok[ar[:ok.shape[0]], ar[r0:r0 + R]] = False
                i, j = (ok & core[r0:r0 + R, None]).nonzero(as_tuple=True)
                keep = j > i + r0
                ii.append(i[keep] + r0); jj.append(j[keep])
                sc = torch.where(ok, s + 0.0, torch.full_like(s, float("-inf")))
                first = (ok & (sc == sc.max(dim=1, keepdim=True).values)).int().argmax(dim=1)
                has = ok.any(dim=1) & ~core[r0:r0 + R]
                bestc[r0:r0 + R] = torch.where(has, first, bestc[r0:r0 + R])
            comp = match._host_components(N, torch.cat(ii).cpu(), torch.cat(jj).cpu())
            core, bestc = core.cpu(), bestc.cpu()
            out = torch.where(core, comp, torch.full_like(comp, -1))
            out[bestc >= 0] = comp[bestc[bestc >= 0]]
            return out
        cases["dense_5"] = dense_5
        checks["dense_5"] = lambda: torch.equal(dense_5(), want[5].cpu())
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
    for per in (5, 50):
        for leg in ("count", "link"):
            res[f"{leg}_{per}"]["vs_union"] = round(res[f"{leg}_{per}"]["median_ms"] / res[f"union_{per}"]["median_ms"], 3)
            res[f"{leg}_{per}"]["vs_pair_hist"] = round(res[f"{leg}_{per}"]["median_ms"] / res["pair_hist"]["median_ms"], 3)
    if "dense_5" in res:
        res["dense_5"]["vs_dbscan_5"] = round(res["dense_5"]["median_ms"] / res["dbscan_5"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dbscan_bench.py needs an MI355X")
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "D": D, "threshold": THR,
           "min_samples": MIN_SAMPLES, "rounds": args.rounds, "steps_per_round": args.steps, "results": {}}
    lines = [f"# tools/dbscan_bench.py  {out['date']}  {out['device']}  symmetric, D={D}, cos >= {THR}, min_samples={MIN_SAMPLES}; "
             f"{args.rounds} interleaved rounds x {args.steps} calls (dense_5: 1), median (min) ms"]
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
