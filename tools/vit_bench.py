"""ViT-B/16 on the device, measured: writes profiles/vit_b_16.txt with three sections.

  (a) Whole step: the model of configs/synthetic/fe_vit_b_16_mi355x.py (ViT-B/16, heads = Linear(768, 512), ArcFace over 10 k ids,
      FusedAdamW) at bs 128, bf16 — fence, N steps, fence.
  (b) The same module in PyTorch eager on the device (bf16 autocast, nn.MultiheadAttention on torch's SDPA, torch.optim.AdamW),
      interleaved with (a): best of the rounds.
  (c) pfr_mha_fwd + pfr_mha_bwd alone at B = 128, 12 heads, S = 197 against F.scaled_dot_product_attention forward + backward on
      the same tensors, interleaved: best of the rounds.

python tools/vit_bench.py [--batch 128] [--steps 10] [--reps 20] [--rounds 3]"""
import argparse
import datetime
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
IDS = 10000


def _groups(ml):
    p1 = [p for n, p in ml.module.named_parameters() if "heads" not in n]
    p2 = [p for n, p in ml.module.named_parameters() if "heads" in n]
    return [{"lr": 5e-4, "params": p1}, {"lr": 1e-3, "params": p2},
            {"lr": 1e-3, "params": list(ml.add_margin.parameters()), "weight_decay": 1e-4}]


def _engine_step(args, dev, x, y):
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.optim import FusedAdamW
    torch.manual_seed(123)
    backbone = M.vit_b_16(compute_dtype=torch.bfloat16)
    backbone.heads = torch.nn.Linear(768, 512)
    ml = SoftmaxBasedMetricLearning(backbone, IDS, 512, is_focal=True, arc_margin=True)
    ml.add_margin.compute_dtype = torch.bfloat16
    ml = ml.to(dev).train()
    backbone.hip_engine(dev)
    opt = FusedAdamW(_groups(ml), 1e-3, weight_decay=0.05)

    def step():
        opt.zero_grad()
        out = ml(x, y)
        out["loss"].backward()
        opt.step()
        return out["loss"]
    return step


def _eager_step(args, dev, x, y):
    """the same module tree run by torch itself (the engine is by-passed: _forward_torch), bf16 autocast, torch's fused AdamW"""
    import pets_face_recognition_amd.models as M
    torch.manual_seed(123)
    backbone = M.vit_b_16()
    backbone.heads = torch.nn.Linear(768, 512)
    backbone = backbone.to(dev).train()
    w = torch.nn.Parameter(torch.randn(IDS, 512, device=dev) * 0.05)
    opt = torch.optim.AdamW([{"params": list(backbone.parameters())}, {"params": [w]}], 1e-3, weight_decay=0.05)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            emb = backbone._forward_torch(x)
        # ArcFace logits + cross entropy in fp32 (the margin head is not what this section compares)
        cos = F.linear(F.normalize(emb.float()), F.normalize(w)).clamp(-1 + 1e-7, 1 - 1e-7)
        phi = torch.cos(torch.acos(cos) + 0.5)
        logits = 64.0 * torch.where(F.one_hot(y, IDS).bool(), phi, cos)
        loss = F.cross_entropy(logits, y)
        loss.backward()
        opt.step()
        return loss
    return step


def _time_steps(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        loss = step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n, float(loss.detach())


def _time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps   # ms


def attention(args, dev):
    from pets_face_recognition_amd._hip import lib, PFR_BF16
    B, heads, S, hd = args.batch, 12, 197, 64
    C = heads * hd
    scale = 1.0 / math.sqrt(hd)
    st = torch.cuda.current_stream().cuda_stream
    qkv = (torch.randn(B, S, 3 * C, device=dev) * 1.2).bfloat16()
    dout = torch.randn(B, S, C, device=dev).bfloat16()
    out = torch.empty(B, S, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, heads, S, device=dev)
    dqkv = torch.empty_like(qkv)

    def o_fwd():
        lib.pfr_mha_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), PFR_BF16, B, S, heads, hd, scale, st)

    def o_bwd():
        lib.pfr_mha_bwd(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), PFR_BF16, B, S, heads, hd, scale, st)

    # torch: the same tensors as [B, heads, S, hd] views (what nn.MultiheadAttention hands to SDPA)
    q, k, v = (t.reshape(B, S, heads, hd).transpose(1, 2).detach().requires_grad_() for t in qkv.split(C, dim=-1))
    do = dout.reshape(B, S, heads, hd).transpose(1, 2)
    keep = [F.scaled_dot_product_attention(q, k, v)]

    def t_fwd():
        with torch.no_grad():
            F.scaled_dot_product_attention(q, k, v)

    def t_fwd_bwd():
        o = F.scaled_dot_product_attention(q, k, v)
        torch.autograd.grad(o, (q, k, v), do)

    for f in (o_fwd, o_bwd, t_fwd, t_fwd_bwd):
        f()
    torch.cuda.synchronize()
    err = ((out.float() - keep[0].transpose(1, 2).reshape(B, S, C).float()).norm() / keep[0].float().norm()).item()
    best = {}
    for _ in range(args.rounds):
        for name, f in (("o_fwd", o_fwd), ("o_bwd", o_bwd), ("t_fwd", t_fwd), ("t_fwd_bwd", t_fwd_bwd)):
            best[name] = min(best.get(name, 1e9), _time(f, args.reps))
    return best, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vit_b_16.txt"))
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"ViT-B/16 on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__} "
             f"(tools/vit_bench.py --batch {args.batch} --steps {args.steps} --reps {args.reps} --rounds {args.rounds})", ""]
    lines.append("== (a) whole step on the HIP engine / (b) the same module in PyTorch eager (bf16 autocast, SDPA): ViT-B/16 + ArcFace "
                 f"({IDS} ids), AdamW, 224x224; fence / N steps / fence, interleaved, best of {args.rounds} rounds")
    if args.skip_step:
        lines.append("(skipped)")
    else:
        g = torch.Generator().manual_seed(1)
        x = torch.rand(args.batch, 3, 224, 224, generator=g).to(dev)
        y = torch.randint(0, IDS, (args.batch,), generator=g).to(dev)
        steps = {"engine": _engine_step(args, dev, x, y), "eager": _eager_step(args, dev, x, y)}
        best, last = {}, {}
        for name, s in steps.items():
            for _ in range(args.warmup):
                s()
        for _ in range(args.rounds):
            for name, s in steps.items():
                dt, last[name] = _time_steps(s, args.steps)
                best[name] = min(best.get(name, 1e9), dt)
        for tag, name in (("(a) HIP engine", "engine"), ("(b) torch eager", "eager")):
            lines.append(f"{tag}: bs {args.batch}: {best[name] * 1e3:.2f} ms/step, {args.batch / best[name]:.0f} img/s (last loss {last[name]:.4f})")
        lines.append(f"engine / eager step time: {best['engine'] / best['eager']:.2f} (< 1: the engine is faster)")
    b, err = attention(args, dev)
    lines += ["", f"== (c) attention alone, B {args.batch}, 12 heads, S 197, head_dim 64, bf16; best of {args.rounds} rounds x {args.reps} launches, interleaved",
              f"pfr_mha_fwd {b['o_fwd']:.4f} ms, pfr_mha_bwd {b['o_bwd']:.4f} ms, fwd+bwd {b['o_fwd'] + b['o_bwd']:.4f} ms",
              f"torch SDPA fwd {b['t_fwd']:.4f} ms, fwd+bwd {b['t_fwd_bwd']:.4f} ms",
              f"ratio torch / ours: fwd {b['t_fwd'] / b['o_fwd']:.2f}, fwd+bwd {b['t_fwd_bwd'] / (b['o_fwd'] + b['o_bwd']):.2f} (> 1: this project's kernel is faster)",
              f"(outputs agree to {err:.2e} relative)"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
