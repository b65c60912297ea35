"""Cost of the open-set extremes (match.class_extremes -> pfr_class_extremes, pfr_extremes_decode): symmetric, D = 512, N = 20 000 and
100 000, bf16 and int8, shuffled tight classes of 5 (tools/cluster_bench.make_inputs), all legs interleaved in one process:
  extremes          the pfr_class_extremes launch alone, all three kinds (plus the reset of the keys)
  extremes_2        the same without worst_pos
  count             the pfr_neighbor_count launch on the same operands at cos >= 0.5 (the same GEMM with the cheapest existing epilogue:
                    the yardstick)
  open_set          match.open_set_metrics end to end (operand preparation, launch, decoding, the host statistics)
  extremes_rand     the launch on RANDOM unit rows with the same classes: every score is near zero, the running maxima keep moving, the
                    filter helps least
  dense             bf16 only: a chunked dense torch implementation of the same contract on the same card (best mate, best impostor and
                    weakest mate with their first indices, nothing else)
The extremes of every leg are checked before anything is timed.  Writes profiles/open_set.txt.
    python tools/open_set_bench.py [--sizes 20000 100000] [--rounds 3] [--steps 3] [--out PATH]"""
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
from cluster_bench import make_inputs, D, THR

PER = 5


def dense_extremes(a, cls, R=2048):
    """the contract on dense chunks of the prepared bf16 operand -> (pos_index, neg_index, weak_index) int64 [N]"""
    N = a.shape[0]
    ar = torch.arange(N, device=a.device)
    out = [torch.full((N,), -1, dtype=torch.int64, device=a.device) for _ in range(3)]
    ninf = float("-inf")
    for r0 in range(0, N, R):
        s = (a[r0:r0 + R] @ a.t()).float() + 0.0
        valid = ~torch.isnan(s)
        valid[ar[:s.shape[0]], ar[r0:r0 + R]] = False                                  # no self pair
        mate = (cls[r0:r0 + R, None] == cls[None, :]) & (cls[r0:r0 + R, None] >= 0)
        for k, (ok, sc) in enumerate(((valid & mate, s), (valid & ~mate, s), (valid & mate, -s))):
            sc = torch.where(ok, sc, torch.full_like(sc, ninf))
            first = (ok & (sc == sc.max(dim=1, keepdim=True).values)).int().argmax(dim=1)
            out[k][r0:r0 + R] = torch.where(ok.any(dim=1), first, out[k][r0:r0 + R])
    return out


def build_cases(N, dt, dev):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import lib, dtype_id
    st = lambda: torch.cuda.current_stream().cuda_stream
    T = dtype_id(dt)
    x, cls, _ = make_inputs(N, PER, dev)
    xr = torch.randn(N, D, generator=torch.Generator().manual_seed(3)).to(dev)
    a, sa = match._hist_operand(x, dt, True)
    r, sr = match._hist_operand(xr, dt, True)
    cls32 = cls.int().contiguous()
    keys = torch.zeros(3, N, dtype=torch.int64, device=dev)
    deg = torch.zeros(N, dtype=torch.int32, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()

    def launch(op, sc, worst=True):
        def run():
            keys.zero_()
            lib.pfr_class_extremes(op.data_ptr(), ptr(sc), N, 0, 0, 0, 0, 0, T, op.shape[1], cls32.data_ptr(), 0, 0, keys[0].data_ptr(),
                                   keys[1].data_ptr(), keys[2].data_ptr() if worst else 0, N, st())
            return keys
        return run

    def count():
        deg.zero_()
        lib.pfr_neighbor_count(a.data_ptr(), ptr(sa), N, 0, 0, 0, 0, 0, T, a.shape[1], THR, deg.data_ptr(), N, st())
        return deg

    def partner(k):
        return (0xFFFFFFFF - (keys[k] & 0xFFFFFFFF)).where(keys[k] != 0, torch.full_like(keys[k], -1))
    same = lambda i: bool(((i >= 0) & (cls[i.clamp_min(0)] == cls)).all())
    other = lambda i: bool(((i >= 0) & (cls[i.clamp_min(0)] != cls)).all())
    full = bool((torch.bincount(cls)[cls] >= 2).all())                                  # (a short last class of one has no mate)
    cases = {"extremes": launch(a, sa), "extremes_2": launch(a, sa, worst=False), "count": count,
             "open_set": lambda: match.open_set_metrics(x, cls, compute_dtype=dt), "extremes_rand": launch(r, sr)}
    checks = {
        "extremes": lambda: (cases["extremes"](), (same(partner(0)) and same(partner(2))) or not full, other(partner(1)))[1:] == (True, True),
        "extremes_2": lambda: (cases["extremes_2"](), not bool(keys[2].any()), other(partner(1)))[1:] == (True, True),
        "count": lambda: torch.equal(count().long(), torch.bincount(cls)[cls] - 1),
        # tight classes: every item with a mate is a rank-1 hit at every rate
        "open_set": lambda: cases["open_set"]()["rank1"] == 1.0,
    }
    if dt == torch.bfloat16:
        cases["dense"] = lambda: dense_extremes(a, cls)

        def dense_ok():   # (torch's bf16 product is rounded to bf16, so ties differ from the kernel's fp32 scores: the classes are checked)
            d = dense_extremes(a, cls)
            return ((same(d[0]) and same(d[2])) or not full) and other(d[1])
        checks["dense"] = dense_ok
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
            steps = 1 if name == "dense" else args.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                cases[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    res = {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for n, v in ms.items()}
    for leg in ("extremes", "extremes_2", "extremes_rand"):
        res[leg]["vs_count"] = round(res[leg]["median_ms"] / res["count"]["median_ms"], 3)
    if "dense" in res:
        res["dense"]["vs_open_set"] = round(res["dense"]["median_ms"] / res["open_set"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_set.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("open_set_bench.py needs an MI355X")
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "D": D, "classes_of": PER,
           "count_threshold": THR, "rounds": args.rounds, "steps_per_round": args.steps, "results": {}}
    lines = [f"# tools/open_set_bench.py  {out['date']}  {out['device']}  symmetric, D={D}, shuffled tight classes of {PER}; count at cos >= {THR}; "
             f"{args.rounds} interleaved rounds x {args.steps} calls (dense: 1), median (min) ms"]
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
