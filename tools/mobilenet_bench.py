"""MobileNetV2 on the device, measured: writes profiles/mobilenet_v2.txt with two sections.  No threshold is set on any figure: the
file is the record.

  1. Whole step: MobileNetV2 + ArcFace (10 k ids) train step at bs 256, bf16, 224² — fence, N steps, fence (as bench.py times its
     workloads) — with the BatchNorm + ReLU6 prologue fused into the depthwise convolution, interleaved with a run that materialises
     the activated expand tensor with pfr_bn_act_clamp before each depthwise convolution (engine.fuse_prologue = False): what the
     fusion buys.
  2. Depthwise kernels: pfr_dwconv3_fwd (prologue + statistics), pfr_dwconv3_dgrad and pfr_dwconv3_wgrad (prologue) per launch at the
     network's ten depthwise geometries of that batch: time, and bytes moved / time as a fraction of the 5.2 TB/s streaming rate the
     README uses.

python tools/mobilenet_bench.py [--batch 256] [--steps 20] [--reps 20] [--rounds 3]"""
import argparse
import datetime
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 5.2e12
# (input plane, channels, stride) of the depthwise convolutions of torchvision's table at 224²
GEOMS = [(112, 32, 1), (112, 96, 2), (56, 144, 1), (56, 144, 2), (28, 192, 1), (28, 192, 2), (14, 384, 1), (14, 576, 1), (14, 576, 2),
         (7, 960, 1)]


def make_step(args, dev, fuse):
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedSGD
    torch.manual_seed(123)
    backbone = M.mobilenet_v2(compute_dtype=torch.bfloat16)
    backbone.classifier = torch.nn.Sequential(torch.nn.Linear(backbone.last_channel, 512))
    ml = SoftmaxBasedMetricLearning(backbone, 10000, 512, is_focal=True, arc_margin=True)
    ml.add_margin.compute_dtype = torch.bfloat16
    ml = ml.to(dev).train()
    backbone.hip_engine(dev).fuse_prologue = fuse
    p1 = [p for n, p in ml.module.named_parameters() if "classifier" not in n]
    p2 = [p for n, p in ml.module.named_parameters() if "classifier" in n]
    opt = FusedSGD([{"lr": 5e-3, "params": p1}, {"lr": 1e-2, "params": p2},
                    {"lr": 1e-2, "params": list(ml.add_margin.parameters()), "weight_decay": 1e-4}], 0.01, momentum=0.9)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(args.batch, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 10000, (args.batch,), generator=g).to(dev)

    def step():
        opt.zero_grad()
        out = ml(x, y)
        out["loss"].backward()
        opt.step()
        return out["loss"]

    return step


def whole_step(args, dev):
    steps = {"fused": make_step(args, dev, True), "materialised": make_step(args, dev, False)}
    best, loss = {}, {}
    for f in steps.values():
        for _ in range(args.warmup):
            f()
    for _ in range(args.rounds):           # interleaved: both forms alternate on the same box
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                l = f()
            torch.cuda.synchronize()
            best[k] = min(best.get(k, 1e9), (time.perf_counter() - t0) / args.steps)
            loss[k] = float(l.detach())
    return best, loss


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps   # ms


def depthwise(args, dev):
    from pets_face_recognition_amd._hip import lib, PFR_BF16
    rows = []
    N = args.batch
    st = torch.cuda.current_stream().cuda_stream
    for HW, C, s in GEOMS:
        OHW = (HW - 1) // s + 1
        x = torch.randn(N, HW, HW, C, device=dev).bfloat16()
        dy = torch.randn(N, OHW, OHW, C, device=dev).bfloat16()
        wt = (torch.randn(9, C, device=dev) / 3).bfloat16()
        sc, sh = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        dw = torch.empty(C, 9, device=dev)
        rpp = lib.pfr_dwconv3_rows_per_part(PFR_BF16, N, HW, HW, C, s)
        part = torch.empty((N * OHW * OHW + rpp - 1) // rpp, 2, C, device=dev)
        ws = torch.empty(lib.pfr_dwconv3_wgrad_parts(PFR_BF16, N, HW, HW, C, s), 9, C, device=dev)
        ours = {
            "fwd": lambda: lib.pfr_dwconv3_fwd(x.data_ptr(), wt.data_ptr(), y.data_ptr(), PFR_BF16, N, HW, HW, C, s, sc.data_ptr(), sh.data_ptr(),
                                               6.0, part.data_ptr(), st),
            "dgrad": lambda: lib.pfr_dwconv3_dgrad(dy.data_ptr(), wt.data_ptr(), dx.data_ptr(), PFR_BF16, N, HW, HW, C, s, st),
            "wgrad": lambda: lib.pfr_dwconv3_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), PFR_BF16, N, HW, HW, C, s,
                                                   sc.data_ptr(), sh.data_ptr(), 6.0, 0, st),
        }
        for f in ours.values():   # warm-up
            f()
        torch.cuda.synchronize()
        best = {}
        for _ in range(args.rounds):
            for k, f in ours.items():
                best[k] = min(best.get(k, 1e9), _time(f, args.reps))
        nbytes = 2 * (x.numel() + dy.numel())      # every kernel moves one input-sized and one output-sized tensor
        rows.append((HW, C, s, best, nbytes))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mobilenet_v2.txt"))
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"MobileNetV2 on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__} "
             f"(tools/mobilenet_bench.py --batch {args.batch} --steps {args.steps} --reps {args.reps} --rounds {args.rounds})", ""]
    lines.append(f"== Whole step: MobileNetV2 + ArcFace (10 k ids), FusedSGD, bf16, 224², fence / N steps / fence; best of {args.rounds} "
                 "interleaved rounds")
    if args.skip_step:
        lines.append("(skipped)")
    else:
        best, loss = whole_step(args, dev)
        for k in ("fused", "materialised"):
            name = {"fused": "BN + ReLU6 in the depthwise prologue", "materialised": "pfr_bn_act_clamp before each depthwise conv"}[k]
            lines.append(f"bs {args.batch}, {name}: {best[k] * 1e3:.2f} ms/step, {args.batch / best[k]:.0f} img/s (last loss {loss[k]:.4f})")
        lines.append(f"the fusion buys {(best['materialised'] - best['fused']) * 1e3:.2f} ms/step "
                     f"({(best['materialised'] / best['fused'] - 1) * 100:.1f} %)")
    rows = depthwise(args, dev)
    lines += ["", f"== Depthwise 3x3 kernels (csrc/pfr_dwconv3.hip), bs {args.batch}, bf16 NHWC; best of {args.rounds} rounds x {args.reps} "
              "launches; % = (bytes of the input-sized + output-sized tensor) / time / 5.2 TB/s",
              f"{'geometry':>16} {'MB moved':>9} {'fwd ms':>8} {'%':>5} {'dgrad ms':>9} {'%':>5} {'wgrad ms':>9} {'%':>5}"]
    for HW, C, s, b, nbytes in rows:
        pct = lambda k: 100 * nbytes / (b[k] * 1e-3) / HBM
        lines.append(f"{f'{HW}x{HW}x{C} s{s}':>16} {nbytes / 1e6:9.1f} {b['fwd']:8.4f} {pct('fwd'):5.1f} {b['dgrad']:9.4f} {pct('dgrad'):5.1f} "
                     f"{b['wgrad']:9.4f} {pct('wgrad'):5.1f}")
    lines.append("(fwd: prologue + statistics epilogue; wgrad: prologue, both of its launches)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
