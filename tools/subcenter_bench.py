"""Cost of the sub-centre head: SoftmaxBasedMetricLearning(nn.Identity(), C, 512, arc_margin=True, sub_centers=K) at B = 256, bf16 compute,
forward + backward, three cases interleaved round by round so that box drift hits all alike:
  C = 10 000, K = 1    the head as it was
  C = 10 000, K = 3    three centres per class: the cosine GEMMs over 30 000 rows, then pool -> row kernel over 10 000 -> scatter
  C = 30 000, K = 1    the same GEMMs as K = 3 with the row kernel over all 30 000 columns and no pool / scatter
The second minus the third is what pooling buys or costs against simply tripling the class count; the per-entry-point device times of
the second case (HIP events around every C-ABI launch, a run of their own) show pool and scatter on their own.
Writes profiles/subcenter_head.txt.    python tools/subcenter_bench.py [--rounds 8] [--steps 20] [--warmup 10] [--out PATH]"""
import argparse
import datetime
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
CASES = [("C10000_K1", 10000, 1), ("C10000_K3", 10000, 3), ("C30000_K1", 30000, 1)]


def pool_scatter_bytes(C, K, elt):
    """bytes the two passes move per step: pool reads B*C*K f32 and writes B*C f32 + B*C bytes; scatter reads B*C gradient elements
    + B*C bytes and writes B*C*K gradient elements"""
    return B * C * K * 4 + B * C * 4 + B * C, B * C * elt + B * C + B * C * K * elt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subcenter_head.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subcenter_bench.py needs an MI355X")
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd._hip.lib import EventTracer, set_tracer
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    steps = {}
    for name, C, K in CASES:
        torch.manual_seed(5)
        wrap = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=True, arc_margin=True, sub_centers=K).to(dev).train()
        wrap.add_margin.compute_dtype = torch.bfloat16
        wrap.return_logits = False
        label = torch.randint(0, C, (B,), generator=g).to(dev)

        def step(wrap=wrap, label=label):
            emb.grad = None
            wrap.add_margin.weight.grad = None
            loss = wrap(emb, label)["loss"]
            loss.backward()
            return loss
        steps[name] = step
    res = {n: {"C": C, "K": K} for n, C, K in CASES}
    for name in steps:
        for _ in range(args.warmup):
            steps[name]()
        torch.cuda.synchronize()
        res[name]["loss"] = round(steps[name]().item(), 5)
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
        res[name]["max_ms"] = round(max(ms[name]), 4)
    # device time per entry point (events around every launch slow the host: a run of its own, after the wall-clock rounds)
    for name in steps:
        tr = EventTracer()
        set_tracer(tr)
        for _ in range(args.steps):
            steps[name]()
        set_tracer(None)
        res[name]["device_us_per_step"] = {k: round(v[1] / args.steps * 1e3, 2) for k, v in sorted(tr.summary().items())}
    pb, sb = pool_scatter_bytes(10000, 3, 2)
    k3 = res["C10000_K3"]["device_us_per_step"]
    lines = [f"# tools/subcenter_bench.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  B={B} D={D} bf16, head forward + backward,",
             f"# {args.rounds} rounds x {args.steps} steps per case, interleaved; wall clock around synchronised windows; device_us_per_step: HIP events per entry point",
             f"# pool moves {pb / 1e6:.1f} MB, scatter {sb / 1e6:.1f} MB per step at C=10000 K=3 (counted from the shapes)"]
    lines += [json.dumps({"case": n, **res[n]}) for n in steps]
    summary = {"K3_minus_K1_ms": round(res["C10000_K3"]["median_ms"] - res["C10000_K1"]["median_ms"], 4),
               "K3_minus_C30000_ms": round(res["C10000_K3"]["median_ms"] - res["C30000_K1"]["median_ms"], 4),
               "pool_us": k3.get("pfr_subcenter_pool"), "scatter_us": k3.get("pfr_subcenter_scatter"),
               "pool_GBps": None if not k3.get("pfr_subcenter_pool") else round(pb / k3["pfr_subcenter_pool"] / 1e3, 1),
               "scatter_GBps": None if not k3.get("pfr_subcenter_scatter") else round(sb / k3["pfr_subcenter_scatter"] / 1e3, 1)}
    lines.append(json.dumps({"summary": summary}))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
