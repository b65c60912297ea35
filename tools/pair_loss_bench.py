"""Cost of the pair losses (losses/pair.py), forward + backward, on one card:
  fused   PairLoss on the device: pfr_l2norm_fwd, one forward launch, one backward launch, pfr_l2norm_bwd (csrc/pfr_pairloss.hip)
  chain   the same contract as a chain of torch ops on the same device tensors (losses.pair.pair_loss_torch: normalise, matmul, masks,
          masked logsumexp, mean, and autograd's backward of each), in fp32 and with the normalised rows rounded to bf16 for the matmul
at B = 256 and 1024, D = 512, classes of 4, bf16 (and fp32) compute; and the head with and without the pair term:
  head    SoftmaxBasedMetricLearning(nn.Identity(), 10 000, 512, arc_margin=True), forward + backward
  head+pair  the same with pair_loss=dict(kind=..., weight=0.5)
The legs are interleaved round by round in one process (a round in one order, the next in the reverse), so that drift of the box hits all
alike; every timed window ends in a device synchronise.  Prints one JSON line per (kind, B, dtype): median / min ms per variant, the ratio
chain / fused and what the pair term adds to the head's step.
  python tools/pair_loss_bench.py [--rounds 8] [--steps 50] [--warmup 10]"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, C = 512, 10000
PARAMS = {"supcon": dict(tau=0.1), "circle": dict(m=0.25, gamma=64.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="256,1024")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_loss_bench.py needs an MI355X")
    from pets_face_recognition_amd.losses import SoftmaxBasedMetricLearning
    from pets_face_recognition_amd.losses.pair import PairLoss, pair_loss_torch
    dev = torch.device("cuda", 0)
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator().manual_seed(5)
        emb = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
        label = torch.arange(B).div(4, rounding_mode="floor")[torch.randperm(B, generator=g)].to(dev)      # classes of 4
        for kind, p in PARAMS.items():
            for dt in (torch.bfloat16, torch.float32):
                fused = PairLoss(kind, compute_dtype=dt, **p)
                head = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=True, arc_margin=True).to(dev)
                both = SoftmaxBasedMetricLearning(nn.Identity(), C, D, is_focal=True, arc_margin=True, pair_loss=dict(kind=kind, weight=0.5, **p)).to(dev)
                head.add_margin.compute_dtype = both.add_margin.compute_dtype = dt
                hl = torch.randint(0, C, (B,), generator=g).to(dev)
                params = [emb] + list(head.parameters()) + list(both.parameters())

                def chain_loss():
                    if dt == torch.float32:
                        return pair_loss_torch(emb, label, kind, **p)
                    xn = nn.functional.normalize(emb, dim=1)
                    xb = xn + (xn.to(torch.bfloat16).float() - xn).detach()       # the bf16-rounded rows, straight-through
                    return pair_loss_torch(xb, label, kind, normalize=False, **p)

                def step(v):
                    for q in params:
                        q.grad = None
                    if v == "fused":
                        loss = fused(emb, label)
                    elif v == "chain":
                        loss = chain_loss()
                    elif v == "head":
                        loss = head(emb, hl)["loss"]
                    else:
                        loss = both(emb, hl)["loss"]
                    loss.backward()
                    return loss

                variants = ["fused", "chain", "head", "head+pair"]
                res = {"kind": kind, "B": B, "D": D, "dtype": str(dt).split(".")[1]}
                for v in variants:
                    for _ in range(args.warmup):
                        step(v)
                    torch.cuda.synchronize()
                    res[f"{v}_loss"] = round(step(v).item(), 5)
                ms = {v: [] for v in variants}
                for r in range(args.rounds):
                    for v in (variants if r % 2 == 0 else variants[::-1]):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.steps):
                            step(v)
                        torch.cuda.synchronize()
                        ms[v].append((time.perf_counter() - t0) / args.steps * 1e3)
                for v in variants:
                    res[f"{v}_median_ms"] = round(statistics.median(ms[v]), 4)
                    res[f"{v}_min_ms"] = round(min(ms[v]), 4)
                res["chain_over_fused"] = round(res["chain_median_ms"] / res["fused_median_ms"], 2)
                res["pair_in_head_ms"] = round(res["head+pair_median_ms"] - res["head_median_ms"], 4)
                print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
