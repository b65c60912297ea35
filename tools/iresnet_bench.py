"""IResNet-50 on the device, measured: writes profiles/iresnet50.txt.  No threshold is set on any figure: the file is the record.

Backbone train step (forward + backward + optimizer step; loss = Σ emb·T with a fixed T, so the margin head is not in the figure) at
bs 128 and 256, 112², bf16, interleaved in one process on the same card:

  engine: models/_iresnet_engine.IResNetEngine (HIP plan) + FusedSGD
  eager:  the same module's torch layers (IResNet._forward_torch) under torch.autocast(bfloat16), channels_last, torch.optim.SGD —
          MIOpen picks its convolutions without its exhaustive search (torch.backends.cudnn.benchmark stays False)

fence, N steps, fence (as bench.py times its workloads); per form the best and the worst of the rounds are reported.  The engine has
one form of the block-entry BatchNorm (materialised: models/_iresnet_engine.py), so there is no prologue A/B to run.

python tools/iresnet_bench.py [--batches 128,256] [--steps 20] [--rounds 3]"""
import argparse
import datetime
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_steps(batch, dev):
    import pets_face_recognition_amd.models as M
    from pets_face_recognition_amd.optim import FusedSGD
    torch.manual_seed(123)
    hip = M.iresnet50(compute_dtype=torch.bfloat16).to(dev).train()
    eager = M.iresnet50()
    eager.load_state_dict(hip.state_dict())
    eager = eager.to(dev).to(memory_format=torch.channels_last).train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(batch, 3, 112, 112, generator=g).to(dev)
    xc = x.contiguous(memory_format=torch.channels_last)
    T = torch.randn(batch, 512, generator=g).to(dev)
    opt_h = FusedSGD(hip.parameters(), 1e-3, momentum=0.9)
    opt_e = torch.optim.SGD([p for p in eager.parameters() if p.requires_grad], 1e-3, momentum=0.9)

    def step_engine():
        opt_h.zero_grad()
        loss = (hip(x) * T).sum()
        loss.backward()
        opt_h.step()
        return loss

    def step_eager():
        opt_e.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            e = eager._forward_torch(xc)
        loss = (e.float() * T).sum()
        loss.backward()
        opt_e.step()
        return loss

    return {"engine": step_engine, "eager": step_eager}


def measure(args, batch, dev):
    steps = make_steps(batch, dev)
    for f in steps.values():
        for _ in range(args.warmup):
            f()
    times, loss = {k: [] for k in steps}, {}
    for _ in range(args.rounds):           # interleaved: both forms alternate on the same box
        for k, f in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                l = f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.steps)
            loss[k] = float(l.detach())
    return times, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,256")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iresnet50.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"IResNet-50 on {torch.cuda.get_device_name(0)}, {datetime.date.today().isoformat()}, torch {torch.__version__} "
             f"(tools/iresnet_bench.py --batches {args.batches} --steps {args.steps} --rounds {args.rounds})", "",
             f"== Backbone train step (forward + backward + SGD step, loss = sum(emb * T)), 112x112, bf16; fence / {args.steps} steps / fence; "
             f"{args.rounds} interleaved rounds: best (worst) of the rounds",
             "engine = IResNetEngine + FusedSGD; eager = the module's torch layers, autocast(bfloat16), channels_last, torch.optim.SGD",
             "block-entry BatchNorm: materialised (the only form built; no prologue A/B)"]
    for batch in [int(b) for b in args.batches.split(",")]:
        times, loss = measure(args, batch, dev)
        for k in ("engine", "eager"):
            lo, hi = min(times[k]), max(times[k])
            lines.append(f"bs {batch}, {k:>6}: {lo * 1e3:8.2f} ms/step ({hi * 1e3:.2f}), {batch / lo:7.0f} img/s (last loss {loss[k]:.4e})")
        lines.append(f"bs {batch}, eager / engine: {min(times['eager']) / min(times['engine']):.2f} x")
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
