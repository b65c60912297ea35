"""Cost of a weight average (EMA) in the bench.py step (ResNet-50 + ArcFace(10 000), bf16, bs 256, built and stepped as bench.py
does): three variants on one model, interleaved round by round so that box drift hits all of them alike:
  none      opt.step()
  fused     FusedSGD.attach_average('ema', d); opt.step()                 (the step kernel updates the average: pfr_sgd_step_avg)
  separate  opt.step(); torch._foreach_lerp_(avg, params, 1 - d)          (a second pass over master and average, one launch per tensor)
The fused variant steps a second FusedSGD over the same parameters and groups (its own momentum buffers), so that switching
variants re-packs nothing.  Prints one JSON line: median / min ms per step of each variant and the medians' differences to `none`; --out FILE also
writes it there with a header (profiles/weight_avg.txt is such a file).  Like bench.py this asks for 8 hardware queues where the
environment sets none: compare the `none` leg with `python bench.py` only under the same GPU_MAX_HW_QUEUES.
  python tools/weight_avg_bench.py [--rounds 8] [--steps 10] [--warmup 10] [--variant fused] [--out FILE]   (--variant: that one alone)"""
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
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--variant", default=None, choices=["none", "fused", "separate"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_avg_bench.py needs an MI355X")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    bargs = argparse.Namespace(arch="resnet50", classes=10000, dtype="bf16", batch=256)
    ml, opt = bench.build(bargs, device)
    params = [p for g in opt.param_groups for p in g["params"]]
    opt_ema = type(opt)([dict(g) for g in opt.param_groups], opt.defaults["lr"], momentum=opt.defaults["momentum"])
    opt_ema.attach_average("ema", args.decay)
    avg = [p.detach().clone() for p in params]
    g = torch.Generator(device="cpu").manual_seed(123)
    x = torch.rand(bargs.batch, 3, 224, 224, generator=g).to(device)
    y = torch.randint(0, bargs.classes, (bargs.batch,), generator=g).to(device)

    def step(variant):
        opt.zero_grad()
        out = ml(x, y)
        out["loss"].backward()
        if variant == "fused":
            opt_ema.step()
        else:
            opt.step()
            if variant == "separate":
                with torch.no_grad():
                    torch._foreach_lerp_(avg, [p.detach() for p in params], 1.0 - args.decay)

    variants = [args.variant] if args.variant else ["none", "fused", "separate"]
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
    n_params = sum(p.numel() for p in params)
    res = {"workload": f"resnet50+ArcFace(10000) bf16 bs {bargs.batch}, bench.py build(); {args.rounds} interleaved rounds x "
                       f"{args.steps} steps per variant", "decay": args.decay, "averaged_parameters": n_params}
    for v in variants:
        res[v] = {"median_ms": round(statistics.median(ms[v]), 4), "min_ms": round(min(ms[v]), 4),
                  "rounds_ms": [round(t, 3) for t in ms[v]]}
    if "none" in ms:
        for v in variants:
            if v != "none":
                res[f"{v}_minus_none_ms"] = round(res[v]["median_ms"] - res["none"]["median_ms"], 4)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("# tools/weight_avg_bench.py: an EMA of the weights in the bench.py step, three variants interleaved on one box\n"
                    "# none = opt.step(); fused = pfr_sgd_step_avg inside FusedSGD.step(); separate = opt.step() + torch._foreach_lerp_\n")
            f.write(f"# GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')} (all three variants); FusedSGD only, FusedAdamW's fused step is not measured here\n")
            for v in variants:
                f.write(f"{v:9s} median {res[v]['median_ms']:.4f} ms/step  min {res[v]['min_ms']:.4f}  rounds {res[v]['rounds_ms']}\n")
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
