"""EfficientNet-B2 on the device, measured: writes profiles/efficientnet_b2.txt.  No threshold is set on any figure: the file is the
record.

  1. Whole step: EfficientNet-B2 (the reference's head, stochastic depth 0.2) + ArcFace (10 k ids) train step at bs 256, bf16, 224² —
     fence, N steps, fence (as bench.py times its workloads) — with the BatchNorm + SiLU prologue fused into the depthwise convolution,
     interleaved with a run that materialises the activated expand tensor with pfr_bn_act_silu before each depthwise convolution
     (engine.fuse_prologue = False): what the fusion buys.
  2. Launch classes at the network's geometries of that batch: pfr_dwconvk_fwd (prologue + statistics), pfr_dwconvk_dgrad,
     pfr_dwconvk_wgrad (prologue) for 3x3 and 5x5; the BatchNorm + SiLU forms; the squeeze-and-excitation passes: time, and bytes
     moved / time as a fraction of the 5.2 TB/s streaming rate the README uses.
  3. The same module and step in plain PyTorch eager on the same GPU (backbone under bf16 autocast, torch.optim.SGD; the margin head is the same): the only baseline there is
     (--skip-eager leaves it out; the file is written before this section starts and once more after it).

python tools/efficientnet_bench.py [--batch 256] [--steps 20] [--reps 20] [--rounds 3]"""
import argparse
import datetime
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 5.2e12
# (input plane, channels, kernel, stride) of the depthwise convolutions of B2's table at 224²
GEOMS = [(112, 32, 3, 1), (112, 16, 3, 1), (112, 96, 3, 2), (56, 144, 3, 1), (56, 144, 5, 2), (28, 288, 5, 1), (28, 288, 3, 2),
         (14, 528, 3, 1), (14, 528, 5, 1), (14, 720, 5, 1), (14, 720, 5, 2), (7, 1248, 5, 1), (7, 1248, 3, 1), (7, 2112, 3, 1)]
# (plane, channels, squeeze width) of the depthwise outputs the BatchNorm + SiLU and SE passes run on
PLANES = [(112, 32, 8), (56, 144, 6), (28, 288, 12), (14, 720, 30), (7, 2112, 88)]


def make_step(args, dev, fuse, eager=False):
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedSGD
    torch.manual_seed(123)
    backbone = M.efficientnet_b2(compute_dtype=torch.bfloat16)
    backbone.classifier = torch.nn.Linear(backbone.classifier[1].in_features, 512)
    if eager:     # the module's own torch layers on the device tensor instead of the engine
        fwd_torch, draw = backbone._forward_torch, backbone._draw_sd

        def eager_forward(x, sd=None):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                emb = fwd_torch(x, draw(x.shape[0], x.device) if sd is None else sd)
            return emb.float()

        backbone.forward = eager_forward
    ml = SoftmaxBasedMetricLearning(backbone, 10000, 512, is_focal=True, arc_margin=True)
    ml.add_margin.compute_dtype = torch.bfloat16
    ml = ml.to(dev).train()
    if not eager:
        backbone.hip_engine(dev).fuse_prologue = fuse
    p1 = [p for n, p in ml.module.named_parameters() if "classifier" not in n]
    p2 = [p for n, p in ml.module.named_parameters() if "classifier" in n]
    groups = [{"lr": 5e-3, "params": p1}, {"lr": 1e-2, "params": p2},
              {"lr": 1e-2, "params": list(ml.add_margin.parameters()), "weight_decay": 1e-4}]
    opt = torch.optim.SGD(groups, 0.01, momentum=0.9) if eager else FusedSGD(groups, 0.01, momentum=0.9)
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


SPREAD = {}   # form -> the per-round ms/step, sorted


def spread(k):
    v = SPREAD[k]
    return f"min / median / max over {len(v)} rounds {v[0] * 1e3:.2f} / {v[len(v) // 2] * 1e3:.2f} / {v[-1] * 1e3:.2f} ms"


def timed(steps, args):
    best, loss, runs = {}, {}, {}
    for f in steps.values():
        for _ in range(args.warmup):
            f()
    for _ in range(args.rounds):           # interleaved: the forms alternate on the same box
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                l = f()
            torch.cuda.synchronize()
            runs.setdefault(k, []).append((time.perf_counter() - t0) / args.steps)
            best[k] = min(runs[k])
            loss[k] = float(l.detach())
    SPREAD.update({k: sorted(v) for k, v in runs.items()})
    return best, loss


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps   # ms


def _best(fns, args):
    for f in fns.values():   # warm-up
        f()
    torch.cuda.synchronize()
    best = {}
    for _ in range(args.rounds):
        for k, f in fns.items():
            best[k] = min(best.get(k, 1e9), _time(f, args.reps))
    return best


def depthwise(args, dev):
    from pets_face_recognition_amd._hip import lib, PFR_BF16
    rows = []
    N = args.batch
    st = torch.cuda.current_stream().cuda_stream
    for HW, C, K, s in GEOMS:
        OHW = (HW - 1) // s + 1
        x = torch.randn(N, HW, HW, C, device=dev).bfloat16()
        dy = torch.randn(N, OHW, OHW, C, device=dev).bfloat16()
        wt = (torch.randn(K * K, C, device=dev) / K).bfloat16()
        sc, sh = torch.rand(C, device=dev) + 0.5, torch.rand(C, device=dev)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        dw = torch.empty(C, K * K, device=dev)
        rpp = lib.pfr_dwconvk_rows_per_part(PFR_BF16, N, HW, HW, C, K, s)
        part = torch.empty((N * OHW * OHW + rpp - 1) // rpp, 2, C, device=dev)
        ws = torch.empty(lib.pfr_dwconvk_wgrad_parts(PFR_BF16, N, HW, HW, C, K, s), K * K, C, device=dev)
        P = lambda t: t.data_ptr()
        ours = {
            "fwd": lambda: lib.pfr_dwconvk_fwd(P(x), P(wt), P(y), PFR_BF16, N, HW, HW, C, K, s, 2, P(sc), P(sh), 0.0, P(part), st),
            "dgrad": lambda: lib.pfr_dwconvk_dgrad(P(dy), P(wt), P(dx), PFR_BF16, N, HW, HW, C, K, s, st),
            "wgrad": lambda: lib.pfr_dwconvk_wgrad(P(x), P(dy), P(ws), P(dw), PFR_BF16, N, HW, HW, C, K, s, 2, P(sc), P(sh), 0.0, 0, st),
        }
        rows.append((HW, C, K, s, _best(ours, args), 2 * (x.numel() + dy.numel())))   # one input-sized and one output-sized tensor
    return rows


def elementwise(args, dev):
    """per plane: (name, ms, bytes moved) of the BatchNorm + SiLU forms and the squeeze-and-excitation passes"""
    from pets_face_recognition_amd._hip import lib, PFR_BF16
    N = args.batch
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t: t.data_ptr()
    out = []
    for HW, C, S in PLANES:
        rows = N * HW * HW
        x = torch.randn(rows, C, device=dev).bfloat16()
        g = torch.randn(rows, C, device=dev).bfloat16()
        y = torch.empty_like(x)
        f = torch.rand(4, C, device=dev) + 0.5
        coef = torch.rand(3, C, device=dev)
        part = torch.empty(lib.pfr_colreduce_blocks(C, PFR_BF16, rows), 2, C, device=dev)
        pooled = torch.randn(N, C, device=dev).bfloat16()
        w1, b1, w2, b2 = torch.randn(S, C, device=dev), torch.randn(S, device=dev), torch.randn(C, S, device=dev), torch.randn(C, device=dev)
        pre, gate, dgate, dpool, ws = (torch.empty(N, S, device=dev), torch.rand(N, C, device=dev), torch.empty(N, C, device=dev),
                                       torch.empty(N, C, device=dev), torch.empty(N, S, device=dev))
        dw1, db1, dw2, db2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2)
        T = x.numel() * 2      # bytes of one activation tensor
        fns = {
            "bn_act_silu": (lambda: lib.pfr_bn_act_silu(P(x), P(f[2]), P(f[3]), P(y), PFR_BF16, rows, C, st), 2 * T),
            "bn_bwd_reduce_silu": (lambda: lib.pfr_bn_bwd_reduce_silu(P(g), P(x), P(f[0]), P(f[1]), P(f[2]), P(f[3]), PFR_BF16, rows, C, P(part), st), 2 * T),
            "bn_bwd_apply_silu": (lambda: lib.pfr_bn_bwd_apply_silu(P(g), P(x), P(coef), P(f[2]), P(f[3]), P(y), PFR_BF16, rows, C, st), 3 * T),
            "avgpool (squeeze)": (lambda: lib.pfr_avgpool_fwd(P(x), P(pooled), PFR_BF16, N, HW * HW, C, st), T),
            "se_gate_fwd": (lambda: lib.pfr_se_gate_fwd(P(pooled), P(w1), P(b1), P(w2), P(b2), P(pre), P(gate), PFR_BF16, N, C, S, st), 0),
            "se_scale_fwd": (lambda: lib.pfr_se_scale_fwd(P(x), P(gate), P(y), PFR_BF16, N, HW * HW, C, st), 2 * T),
            "se_scale_bwd_reduce": (lambda: lib.pfr_se_scale_bwd_reduce(P(g), P(x), P(dgate), PFR_BF16, N, HW * HW, C, st), 2 * T),
            "se_gate_bwd": (lambda: lib.pfr_se_gate_bwd(P(dgate), P(pooled), P(pre), P(gate), P(w1), P(w2), P(ws), P(dpool), P(dw1), P(db1),
                                                        P(dw2), P(db2), PFR_BF16, N, C, S, 0, st), 0),
            "se_bwd_apply": (lambda: lib.pfr_se_bwd_apply(P(g), P(gate), P(dpool), P(y), PFR_BF16, N, HW * HW, C, st), 2 * T),
        }
        best = _best({k: v[0] for k, v in fns.items()}, args)
        out.append((HW, C, S, [(k, best[k], fns[k][1]) for k in fns]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "efficientnet_b2.txt"))
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-eager", action="store_true")
    ap.add_argument("--only-depthwise", action="store_true", help="the depthwise table alone (A/B of a variant build loaded with PFR_LIB_PATH)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"EfficientNet-B2 on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__} "
             f"(tools/efficientnet_bench.py --batch {args.batch} --steps {args.steps} --reps {args.reps} --rounds {args.rounds})", ""]

    def write():
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(text)
        return text

    lines.append(f"== Whole step: EfficientNet-B2 + ArcFace (10 k ids), FusedSGD, bf16, 224², stochastic depth 0.2, fence / N steps / fence; "
                 f"best of {args.rounds} interleaved rounds of {args.steps} steps")
    if args.skip_step or args.only_depthwise:
        lines.append("(skipped)")
    else:
        best, loss = timed({"fused": make_step(args, dev, True), "materialised": make_step(args, dev, False)}, args)
        for k in ("fused", "materialised"):
            name = {"fused": "BN + SiLU in the depthwise prologue", "materialised": "pfr_bn_act_silu before each depthwise conv"}[k]
            lines.append(f"bs {args.batch}, {name}: {best[k] * 1e3:.2f} ms/step, {args.batch / best[k]:.0f} img/s; {spread(k)} "
                         f"(last loss {loss[k]:.4f})")
        lines.append(f"the fusion buys {(best['materialised'] - best['fused']) * 1e3:.2f} ms/step "
                     f"({(best['materialised'] / best['fused'] - 1) * 100:.1f} %)")
    print(write(), flush=True)
    n0 = len(lines)
    rows = depthwise(args, dev)
    lines += ["", f"== Depthwise k x k kernels (csrc/pfr_dwconvk.hip), bs {args.batch}, bf16 NHWC, SiLU prologue; best of {args.rounds} rounds x "
              f"{args.reps} launches; % = (bytes of the input-sized + output-sized tensor) / time / 5.2 TB/s",
              f"{'geometry':>20} {'MB moved':>9} {'fwd ms':>8} {'%':>5} {'dgrad ms':>9} {'%':>5} {'wgrad ms':>9} {'%':>5}"]
    for HW, C, K, s, b, nbytes in rows:
        pct = lambda k: 100 * nbytes / (b[k] * 1e-3) / HBM
        lines.append(f"{f'{HW}x{HW}x{C} k{K} s{s}':>20} {nbytes / 1e6:9.1f} {b['fwd']:8.4f} {pct('fwd'):5.1f} {b['dgrad']:9.4f} {pct('dgrad'):5.1f} "
                     f"{b['wgrad']:9.4f} {pct('wgrad'):5.1f}")
    lines.append("(fwd: prologue + statistics epilogue; wgrad: prologue, both of its launches)")
    if args.only_depthwise:
        print(write(), flush=True)
        return
    lines += ["", f"== BatchNorm + SiLU forms (csrc/pfr_elementwise.hip) and squeeze-and-excitation (csrc/pfr_se.hip), bs {args.batch}, bf16; ms per "
              "launch and % of 5.2 TB/s for the activation-sized tensors each pass reads and writes (the gate passes move [N][C] only)"]
    for HW, C, S, items in elementwise(args, dev):
        lines.append(f"{HW}x{HW}x{C}, S = {S}: " + "; ".join(
            f"{k} {ms:.4f}" + (f" ({100 * nb / (ms * 1e-3) / HBM:.0f} %)" if nb else "") for k, ms, nb in items))
    print("\n".join(lines[n0:]), flush=True)
    write()
    lines += ["", f"== The same module and step in plain PyTorch eager on this GPU (bf16 autocast, torch.optim.SGD), best of {args.rounds} rounds"]
    if args.skip_eager:
        lines.append("(skipped)")
    else:
        best, loss = timed({"eager": make_step(args, dev, True, eager=True)}, args)
        lines.append(f"bs {args.batch}, eager: {best['eager'] * 1e3:.2f} ms/step, {args.batch / best['eager']:.0f} img/s; {spread('eager')} "
                     f"(last loss {loss['eager']:.4f})")
    print("\n".join(lines[-2:]), flush=True)
    write()


if __name__ == "__main__":
    main()
