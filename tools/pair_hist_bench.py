"""Cost of the all-pairs verification histogram (match.pair_histogram -> pfr_pair_hist): symmetric, D = 512, 4096 bins, N = 20 000 and
100 000 embeddings, bf16 and int8 operands.  Per (N, dtype) these cases run interleaved round by round in one process:
  hist_random     L2-normalised random rows: impostor cosines spread over ~500 bins around 0
  hist_clustered  1 000 classes in tight clusters, rows sorted by class: neighbouring lanes of a wave hold (nearly) the same score, the
                  contended-bin case of the LDS atomics
  gemm_plain      the parent's plain score GEMM of the same FLOPs: N x N/2 scores written as fp32 in column chunks into one reused buffer
                  (int8: pfr_match_scores_i8; bf16: pfr_conv2d_fwd as a GEMM, the match's own unfused call) — what the epilogue costs
  torch_histc     the torch formulation on the same card: row chunks of a @ a[r0:].T in bf16, then torch.histc per kind over the pairs i < j
                  (bf16 rows only; once per round)
The prepared operands (normalised / quantised rows) are made once outside the timed window: only the pair kernel and its zeroing are timed.
Writes profiles/pair_hist.txt.
    python tools/pair_hist_bench.py [--sizes 20000 100000] [--rounds 3] [--steps 3] [--out PATH]"""
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

D, BINS, NCLS = 512, 4096, 1000


def make_inputs(N, dev):
    g = torch.Generator().manual_seed(7)
    rnd = torch.randn(N, D, generator=g)
    cls = (torch.arange(N) * NCLS // N).int()
    clu = torch.randn(NCLS, D, generator=g)[cls.long()] + 0.02 * torch.randn(N, D, generator=g)
    return rnd.to(dev), clu.to(dev), cls.to(dev)


def build_cases(N, dt, dev):
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import lib, dtype_id, ops
    rnd, clu, cls = make_inputs(N, dev)
    st = lambda: torch.cuda.current_stream().cuda_stream
    lo, inv_w = match._hist_range(BINS, (-1.0, 1.0))
    hist = torch.zeros((2, BINS + 1), dtype=torch.int64, device=dev)
    prepared = {name: match._hist_operand(x, dt, True) for name, x in (("random", rnd), ("clustered", clu))}

    def hist_case(name):
        a, sa = prepared[name]

        def run():
            hist.zero_()
            lib.pfr_pair_hist(a.data_ptr(), 0 if sa is None else sa.data_ptr(), cls.data_ptr(), N, 0, 0, 0, 0, dtype_id(dt), a.shape[1],
                              lo, inv_w, BINS, hist.data_ptr(), st())
            return hist
        return run

    a, sa = prepared["random"]
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

    cases = {"hist_random": hist_case("random"), "hist_clustered": hist_case("clustered"), "gemm_plain": gemm_plain}
    if dt == torch.bfloat16:
        ab = prepared["random"][0]
        R = 2048

        def torch_histc():
            h = torch.zeros((2, BINS), dtype=torch.float64, device=dev)
            for r0 in range(0, N, R):
                s = (ab[r0:r0 + R] @ ab[r0:].t()).float()
                i = torch.arange(r0, r0 + s.shape[0], device=dev)[:, None]
                j = torch.arange(r0, N, device=dev)[None, :]
                same = cls[r0:r0 + R, None] == cls[None, r0:]
                up = i < j
                h[1] += torch.histc(s[up & same], bins=BINS, min=-1.0, max=1.0).double()
                h[0] += torch.histc(s[up & ~same], bins=BINS, min=-1.0, max=1.0).double()
            return h
        cases["torch_histc"] = torch_histc
    return cases


def run(N, dt, args, dev):
    cases = build_cases(N, dt, dev)
    pairs = N * (N - 1) // 2
    for name, fn in cases.items():          # warm-up of every shape, and what the counts must be
        out = fn()
        torch.cuda.synchronize()
        if name.startswith("hist_"):
            assert int(out.sum()) == pairs, (name, int(out.sum()), pairs)
        if name == "torch_histc":
            assert int(out.double().sum()) == pairs
    ms = {n: [] for n in cases}
    order = list(cases)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            steps = 1 if name == "torch_histc" else args.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                cases[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
    res = {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for n, v in ms.items()}
    flop = 2.0 * pairs * D
    for n in ("hist_random", "hist_clustered"):
        res[n]["tera_ops"] = round(flop / (res[n]["median_ms"] * 1e-3) / 1e12, 1)
        res[n]["vs_gemm_plain"] = round(res[n]["median_ms"] / res["gemm_plain"]["median_ms"], 3)
    res["hist_clustered"]["vs_hist_random"] = round(res["hist_clustered"]["median_ms"] / res["hist_random"]["median_ms"], 3)
    if "torch_histc" in res:
        res["torch_histc"]["vs_hist_random"] = round(res["torch_histc"]["median_ms"] / res["hist_random"]["median_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_hist.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_hist_bench.py needs an MI355X")
    dev = torch.device("cuda", 0)
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "D": D, "bins": BINS, "classes": NCLS,
           "rounds": args.rounds, "steps_per_round": args.steps, "results": {}}
    lines = [f"# tools/pair_hist_bench.py  {out['date']}  {out['device']}  symmetric, D={D}, bins={BINS}; {args.rounds} interleaved rounds x "
             f"{args.steps} calls (torch_histc: 1), median (min) ms; tera_ops = N (N - 1) D / time"]
    for N in args.sizes:
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.int8, "int8")):
            res = run(N, dt, args, dev)
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
