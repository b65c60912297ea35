"""ConvNeXt-T on the device, measured: writes profiles/convnext_t.txt with three sections.

  1. Whole step: ConvNeXt-T + ArcFace (10 k ids) train step at bs 128, bf16 — fence, N steps, fence (as bench.py times Swin-T).
  2. Depthwise kernels: forward, data gradient and weight gradient at the four depthwise geometries of that batch, with the
     ratio to the HBM bound (bytes read + written over the 5.2 TB/s streaming rate the README uses).
  3. Baseline: each geometry interleaved on the same box against torch's own F.conv2d(groups=C) forward and backward in
     channels-last bf16 (what the reference's config would run).

python tools/convnext_bench.py [--batch 128] [--steps 20] [--reps 20] [--rounds 5]"""
import argparse
import datetime
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 5.2e12
GEOMS = [(56, 96), (28, 192), (14, 384), (7, 768)]


def whole_step(args, dev):
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedAdamW
    torch.manual_seed(123)
    backbone = M.convnext_tiny(compute_dtype=torch.bfloat16)
    backbone.classifier[2] = torch.nn.Linear(768, 512)
    ml = SoftmaxBasedMetricLearning(backbone, 10000, 512, is_focal=True, arc_margin=True)
    ml.add_margin.compute_dtype = torch.bfloat16
    ml = ml.to(dev).train()
    backbone.hip_engine(dev)
    p1 = [p for n, p in ml.module.named_parameters() if "classifier" not in n]
    p2 = [p for n, p in ml.module.named_parameters() if "classifier" in n]
    opt = FusedAdamW([{"lr": 5e-4, "params": p1}, {"lr": 1e-3, "params": p2},
                      {"lr": 1e-3, "params": list(ml.add_margin.parameters()), "weight_decay": 1e-4}], 1e-3, weight_decay=0.05)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(args.batch, 3, 224, 224, generator=g).to(dev)
    y = torch.randint(0, 10000, (args.batch,), generator=g).to(dev)

    def step():
        opt.zero_grad()
        out = ml(x, y)
        out["loss"].backward()
        opt.step()
        return out["loss"]

    for _ in range(args.warmup):
        loss = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    return dt, float(loss.detach())


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
    for HW, C in GEOMS:
        x = torch.randn(N, HW, HW, C, device=dev).bfloat16()
        dy = torch.randn(N, HW, HW, C, device=dev).bfloat16()
        w = (torch.randn(C, 1, 7, 7, device=dev) / 7)
        wt = w.view(C, 49).t().contiguous().bfloat16()
        bias = torch.zeros(C, device=dev)
        y = torch.empty_like(x)
        dw = torch.empty(C, 49, device=dev)
        db = torch.empty(C, device=dev)
        parts = lib.pfr_dwconv2d_wgrad_parts(PFR_BF16, N, HW, HW, C, 7)
        ws = torch.empty(parts, 50, C, device=dev)
        ours = {
            "fwd": lambda: lib.pfr_dwconv2d_fwd(x.data_ptr(), wt.data_ptr(), bias.data_ptr(), y.data_ptr(), PFR_BF16, N, HW, HW, C, 7, 0, st),
            "dgrad": lambda: lib.pfr_dwconv2d_fwd(dy.data_ptr(), wt.data_ptr(), 0, y.data_ptr(), PFR_BF16, N, HW, HW, C, 7, 1, st),
            "wgrad": lambda: lib.pfr_dwconv2d_wgrad(x.data_ptr(), dy.data_ptr(), ws.data_ptr(), dw.data_ptr(), db.data_ptr(), PFR_BF16, N, HW,
                                                    HW, C, 7, 0, st),
        }
        # torch: channels-last bf16 F.conv2d(groups=C); backward = data + weight + bias gradients in one autograd call
        xt = x.permute(0, 3, 1, 2).detach().requires_grad_()          # NCHW view of NHWC memory = channels_last
        wtt = w.bfloat16().contiguous(memory_format=torch.channels_last).requires_grad_()
        bt = bias.bfloat16().requires_grad_()
        dyt = dy.permute(0, 3, 1, 2)
        yt = [F.conv2d(xt, wtt, bt, padding=3, groups=C)]

        def t_fwd():
            with torch.no_grad():
                F.conv2d(xt, wtt, bt, padding=3, groups=C)

        def t_bwd():
            torch.autograd.grad(yt[0], (xt, wtt, bt), dyt, retain_graph=True)

        theirs = {"fwd": t_fwd, "bwd": t_bwd}
        for f in list(ours.values()) + list(theirs.values()):   # warm-up
            f()
        torch.cuda.synchronize()
        best = {}
        for _ in range(args.rounds):                             # interleaved: ours and torch alternate on the same box
            for k, f in ours.items():
                best["o_" + k] = min(best.get("o_" + k, 1e9), _time(f, args.reps))
            for k, f in theirs.items():
                best["t_" + k] = min(best.get("t_" + k, 1e9), _time(f, args.reps))
        nbytes = 2 * x.numel() * 2                                # one tensor read, one written (fwd, dgrad); two read (wgrad)
        bound_ms = nbytes / HBM * 1e3
        rows.append((HW, C, best, bound_ms))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_t.txt"))
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"ConvNeXt-T on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__} "
             f"(tools/convnext_bench.py --batch {args.batch} --steps {args.steps} --reps {args.reps} --rounds {args.rounds})", ""]
    lines.append("== Whole step: ConvNeXt-T + ArcFace (10 k ids), FusedAdamW, bf16, fence / N steps / fence")
    if args.skip_step:
        lines.append("(skipped)")
    else:
        dt, loss = whole_step(args, dev)
        lines.append(f"bs {args.batch}: {dt * 1e3:.2f} ms/step, {args.batch / dt:.0f} img/s (last loss {loss:.4f})")
    rows = depthwise(args, dev)
    lines += ["", f"== Depthwise 7x7 kernels (csrc/pfr_dwconv.hip), bs {args.batch}, bf16 NHWC; best of {args.rounds} rounds x {args.reps} launches; "
              "HBM bound = (bytes read + written) / 5.2 TB/s",
              f"{'geometry':>12} {'bound ms':>9} {'fwd ms':>8} {'x bound':>8} {'dgrad ms':>9} {'x bound':>8} {'wgrad ms':>9} {'x bound':>8}"]
    for HW, C, b, bound in rows:
        lines.append(f"{f'{HW}x{HW}x{C}':>12} {bound:9.4f} {b['o_fwd']:8.4f} {b['o_fwd'] / bound:8.2f} {b['o_dgrad']:9.4f} "
                     f"{b['o_dgrad'] / bound:8.2f} {b['o_wgrad']:9.4f} {b['o_wgrad'] / bound:8.2f}")
    lines += ["", "== Baseline: torch F.conv2d(groups=C), channels-last bf16, interleaved with the above (backward = data + weight + bias gradient)",
              f"{'geometry':>12} {'torch fwd':>10} {'ours fwd':>9} {'ratio':>6} {'torch bwd':>10} {'ours dgrad+wgrad':>17} {'ratio':>6}"]
    for HW, C, b, bound in rows:
        ob = b["o_dgrad"] + b["o_wgrad"]
        lines.append(f"{f'{HW}x{HW}x{C}':>12} {b['t_fwd']:10.4f} {b['o_fwd']:9.4f} {b['t_fwd'] / b['o_fwd']:6.2f} {b['t_bwd']:10.4f} {ob:17.4f} "
                     f"{b['t_bwd'] / ob:6.2f}")
    lines.append("(ratio > 1: this project's kernel is faster)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
