"""Cost of the mined pair losses (losses/pair.py, csrc/pfr_pairmine.hip) on one card: forward + backward of batch_hard and
multi_similarity at B = 256, D = 512, classes of 4, without a ring (M = 0) and against a FULL ring of M = 4096 and 65 536 slots, bf16 and
fp32 compute:
  fused     PairMinedLossFunction: pfr_l2norm_fwd, pfr_pair_mined_fwd (one launch for batch_hard, two for multi_similarity),
            pfr_pair_mined_bwd (sparse for batch_hard; dense + the slab sum for multi_similarity), pfr_l2norm_bwd
  chain     the same contract as torch ops on the same device tensors (losses.pair.pair_loss_mem_torch and autograd's backward; bf16: the
            normalised rows rounded to bf16, straight-through)
  circle    the existing Circle kernels (PairLossFunction / PairMemLossFunction) on the same operands: what a one-pass pair loss costs
The legs are interleaved round by round in one process (a round in one order, the next in the reverse); every timed window ends in a
device synchronise.  Prints one JSON line per (M, dtype) and writes them to --out (profiles/pair_mined.txt holds them as a table).
  python tools/pair_mined_bench.py [--rounds 8] [--steps 30] [--warmup 5] [--out FILE]"""
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

B, D = 256, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--memories", default="0,4096,65536")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_mined_bench.py needs an MI355X")
    from pets_face_recognition_amd._hip import ops
    from pets_face_recognition_amd.losses.pair import PairLoss, pair_loss_mem_torch
    dev = torch.device("cuda", 0)
    lines = []
    for M in [int(m) for m in args.memories.split(",")]:
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator().manual_seed(5)
            emb = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
            label = torch.arange(B).div(4, rounding_mode="floor")[torch.randperm(B, generator=g)].to(dev)      # classes of 4
            mods = {k: PairLoss(k, memory=M, compute_dtype=dt).to(dev).eval() for k in ("batch_hard", "multi_similarity", "circle")}
            for i in range(M // B):                                     # a full ring, the same rows in every module's ring
                rows = ops.l2norm_fwd(torch.randn(B, D, generator=g).to(dev), dt)[0]
                lab = label[torch.randperm(B, generator=g).to(dev)]
                for m in mods.values():
                    m.push(rows, lab)
            ref = mods["circle"]
            mem32 = ref.mem.float() if M else torch.zeros(0, D, device=dev)
            ml = ref.mem_label if M else torch.zeros(0, dtype=torch.int64, device=dev)

            def chain_loss(kind):
                xn = nn.functional.normalize(emb, dim=1)
                if dt == torch.bfloat16:
                    xn = xn + (xn.to(torch.bfloat16).float() - xn).detach()
                return pair_loss_mem_torch(xn, label, mem32, ml, kind, normalize=False, **mods[kind].params)

            def step(v):
                emb.grad = None
                what, kind = v.split(":")
                loss = mods[kind](emb, label) if what == "fused" else chain_loss(kind)
                loss.backward()
                return loss

            variants = ["fused:batch_hard", "chain:batch_hard", "fused:multi_similarity", "chain:multi_similarity", "fused:circle"]
            res = {"B": B, "D": D, "M": M, "dtype": str(dt).split(".")[1], "splits": ops.pair_mined_splits(B, M, D)}
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
            for kind in ("batch_hard", "multi_similarity"):
                res[f"{kind}_chain_over_fused"] = round(res[f"chain:{kind}_median_ms"] / res[f"fused:{kind}_median_ms"], 2)
                res[f"{kind}_fused_over_circle"] = round(res[f"fused:{kind}_median_ms"] / res["fused:circle_median_ms"], 2)
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
            del mods, ref, mem32
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
