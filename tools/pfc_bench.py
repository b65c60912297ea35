"""Cost of the margin head with Partial FC: SoftmaxBasedMetricLearning(nn.Identity(), C, 512, arc_margin=True, sample_rate=r, sparse_grad=s)
at B = 256, D = 512, bf16 compute; one step = zero_grad + head forward + backward + FusedSGD step of the head weight (momentum 0.9,
weight decay 1e-4).  Per class count C (100 000 and 1 000 000) five cases run interleaved round by round in one process, so that box
drift hits all alike:
  r = 1.0             the head as it was: every class scored, dense gradient, dense optimiser step
  r = 0.3 / 0.1 dense   sampled classes, dense [C, D] gradient with zero unsampled rows (any optimiser)
  r = 0.3 / 0.1 sparse  sampled classes, weight.row_grad, pfr_sgd_step_rows on the sampled rows only
Every ratio is against r = 1.0 of the same run.  Peak device memory is taken per case in a pass of its own after the timed rounds
(torch.cuda.max_memory_allocated over a few steps, from an emptied cache; the other cases' modules stay resident and are subtracted as the
baseline before the steps).  The steps train on one fixed batch, so the recorded loss falls towards 0.  Writes profiles/pfc_head.txt.
    python tools/pfc_bench.py [--classes 100000 1000000] [--rounds 6] [--steps 10] [--warmup 5] [--out PATH]"""
import argparse
import datetime
import gc
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, D = 256, 512
CASES = [("full", 1.0, False), ("r0.3_dense", 0.3, False), ("r0.3_sparse", 0.3, True), ("r0.1_dense", 0.1, False), ("r0.1_sparse", 0.1, True)]


def build(C, rate, sparse, dev, emb, label):
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedSGD
    torch.manual_seed(5)
    wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=True, arc_margin=True, sample_rate=rate, sparse_grad=sparse).to(dev).train()
    wrap.add_margin.compute_dtype = torch.bfloat16
    wrap.return_logits = False
    opt = FusedSGD([{"params": list(wrap.add_margin.parameters()), "weight_decay": 1e-4}], 0.01, momentum=0.9)

    def step():
        emb.grad = None
        opt.zero_grad()
        loss = wrap(emb, label)["loss"]
        loss.backward()
        opt.step()
        return loss
    return step


def run(C, args, dev):
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    label = torch.randint(0, C, (B,), generator=g).to(dev)
    steps = {name: build(C, rate, sparse, dev, emb, label) for name, rate, sparse in CASES}
    res = {name: {"sample_rate": rate, "sparse_grad": sparse, "S": int(rate * C) if rate < 1 else C} for name, rate, sparse in CASES}
    for name in steps:
        for _ in range(args.warmup):
            steps[name]()
        torch.cuda.synchronize()
        res[name]["loss"] = round(steps[name]().item(), 4)
    ms = {n: [] for n in steps}
    order = list(steps)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                steps[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    for name in steps:
        res[name]["median_ms"] = round(statistics.median(ms[name]), 4)
        res[name]["min_ms"] = round(min(ms[name]), 4)
        res[name]["vs_full"] = round(res[name]["median_ms"] / statistics.median(ms["full"]), 4)
    # peak memory of a step above what is resident before it (all five modules, their momentum and cached buffers)
    for name in steps:
        torch.cuda.synchronize()
        gc.collect()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(3):
            steps[name]()
        torch.cuda.synchronize()
        res[name]["step_peak_mb_above_resident"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pfc_head.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pfc_bench.py needs an MI355X")
    dev = torch.device("cuda", 0)
    out = {"date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "B": B, "D": D, "dtype": "bf16",
           "step": "zero_grad + head forward + backward + FusedSGD step of the head weight", "rounds": args.rounds,
           "steps_per_round": args.steps, "classes": {}}
    lines = [f"# tools/pfc_bench.py  {out['date']}  {out['device']}  B={B} D={D} bf16; {out['step']}; "
             f"{args.rounds} interleaved rounds x {args.steps} steps, median (min) ms"]
    for C in args.classes:
        res = run(C, args, dev)
        out["classes"][str(C)] = res
        lines.append(f"C = {C}")
        for name, r in res.items():
            lines.append(f"  {name:12s} S={r['S']:>8d}  {r['median_ms']:9.4f} ({r['min_ms']:9.4f}) ms  x{r['vs_full']:.3f} of full  "
                         f"step peak {r['step_peak_mb_above_resident']:9.1f} MB above resident  loss {r['loss']}")
        gc.collect()
        torch.cuda.empty_cache()
    lines.append(json.dumps(out))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
