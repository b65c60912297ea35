"""Cost of gradient clipping in the bench.py step (ResNet-50 + ArcFace(10 000), bf16, bs 256, built and stepped as bench.py does):
three variants on one model, interleaved round by round so that box drift hits all of them alike:
  none   opt.step()
  fused  opt.clip_grad_norm_(1.0); opt.step()                         (device norm, coefficient read by the update kernels)
  torch  torch.nn.utils.clip_grad_norm_(params, 1.0); opt.step()      (per-tensor norms, stack, in-place scale of every gradient)
Prints one JSON line: median / min ms per step of each variant and the medians' differences to `none`.
  python tools/clip_bench.py [--rounds 8] [--steps 10] [--warmup 10] [--variant fused]   (--variant: that variant alone, for a trace)"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--variant", default=None, choices=["none", "fused", "torch"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench.py needs an MI355X")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    bargs = argparse.Namespace(arch="resnet50", classes=10000, dtype="bf16", batch=256)
    ml, opt = bench.build(bargs, device)
    params = [p for g in opt.param_groups for p in g["params"]]
    g = torch.Generator(device="cpu").manual_seed(123)
    x = torch.rand(bargs.batch, 3, 224, 224, generator=g).to(device)
    y = torch.randint(0, bargs.classes, (bargs.batch,), generator=g).to(device)

    def step(variant):
        opt.zero_grad()
        out = ml(x, y)
        out["loss"].backward()
        if variant == "fused":
            opt.clip_grad_norm_(args.max_norm)
        elif variant == "torch":
            torch.nn.utils.clip_grad_norm_(params, args.max_norm)
        opt.step()

    variants = [args.variant] if args.variant else ["none", "fused", "torch"]
    for v in variants:
        for _ in range(args.warmup):
            step(v)
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    for r in range(args.rounds):
        order = variants if r % 2 == 0 else variants[::-1]
        for v in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(v)
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) / args.steps * 1e3)
    res = {"workload": f"resnet50+ArcFace(10000) bf16 bs {bargs.batch}, bench.py build(); {args.rounds} interleaved rounds x "
                       f"{args.steps} steps per variant", "max_norm": args.max_norm}
    for v in variants:
        res[v] = {"median_ms": round(statistics.median(ms[v]), 4), "min_ms": round(min(ms[v]), 4),
                  "rounds_ms": [round(t, 3) for t in ms[v]]}
    if "none" in ms:
        for v in variants:
            if v != "none":
                res[f"{v}_minus_none_ms"] = round(res[v]["median_ms"] - res["none"]["median_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
