"""Cost of the pair losses with a cross-batch memory (losses/pair.py, csrc/pfr_pairmem.hip) on one card, at B = 256, D = 512 and a FULL
ring of M = 4096, 16 384 and 65 536 slots, bf16 and fp32 compute, supcon:
  fused     PairMemLossFunction: pfr_l2norm_fwd, pfr_pair_mem_loss_fwd, pfr_pair_mem_loss_bwd (+ the slab sum), pfr_l2norm_bwd, under both
            grid orders (pfr_set_tuning("pair_mem_order", 0 | 1): 0 anchor block fast, 1 the anchor blocks of a partner range on one XCD)
  chain     the same contract as torch ops on the same device tensors (losses.pair.pair_loss_mem_torch and autograd's backward; bf16: the
            normalised rows rounded to bf16, straight-through)
  matmul3   a bare torch bf16 B x (B + M) x D matmul three times: the FLOP yardstick (scores, their recomputation, the second product)
  push      pfr_pair_mem_push of one batch alone
The legs are interleaved round by round in one process (a round in one order, the next in the reverse); every timed window ends in a
device synchronise.  Prints one JSON line per (M, dtype) and writes them to profiles/pair_memory.txt with --out.
  python tools/pair_memory_bench.py [--rounds 8] [--steps 30] [--warmup 5] [--out profiles/pair_memory.txt]"""
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
KIND, P = "supcon", dict(tau=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--memories", default="4096,16384,65536")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_memory_bench.py needs an MI355X")
    from pets_face_recognition_amd._hip import lib, ops
    from pets_face_recognition_amd.losses.pair import PairLoss, pair_loss_mem_torch
    dev = torch.device("cuda", 0)
    lines = []
    for M in [int(m) for m in args.memories.split(",")]:
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator().manual_seed(5)
            emb = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
            label = torch.arange(B).div(4, rounding_mode="floor")[torch.randperm(B, generator=g)].to(dev)      # classes of 4
            fused = PairLoss(KIND, memory=M, compute_dtype=dt, **P).to(dev).eval()      # eval: the ring is read and left alone
            for i in range(M // B):                                                       # a full ring, every class 4 + 4 M / B times
                rows = ops.l2norm_fwd(torch.randn(B, D, generator=g).to(dev), dt)[0]
                fused.push(rows, label[torch.randperm(B, generator=g).to(dev)])
            assert fused.count == M
            mem32, ml = fused.mem.float(), fused.mem_label
            a16, b16 = torch.randn(B, D, device=dev).bfloat16(), torch.randn(B + M, D, device=dev).bfloat16()
            xpush = ops.l2norm_fwd(emb.detach(), dt)[0]

            def chain_loss():
                xn = nn.functional.normalize(emb, dim=1)
                if dt == torch.bfloat16:
                    xn = xn + (xn.to(torch.bfloat16).float() - xn).detach()
                return pair_loss_mem_torch(xn, label, mem32, ml, KIND, normalize=False, **P)

            def step(v):
                emb.grad = None
                if v.startswith("fused"):
                    lib.pfr_set_tuning(b"pair_mem_order", int(v[-1]))
                    loss = fused(emb, label)
                    loss.backward()
                elif v == "chain":
                    loss = chain_loss()
                    loss.backward()
                elif v == "matmul3":
                    loss = None
                    for _ in range(3):
                        a16 @ b16.t()
                else:
                    loss = None
                    ops.pair_mem_push(xpush, label, fused.mem, fused.memT, fused.mem_label, 0)
                return loss

            variants = ["fused_order0", "fused_order1", "chain", "matmul3", "push"]
            res = {"kind": KIND, "B": B, "D": D, "M": M, "dtype": str(dt).split(".")[1], "splits": ops.pair_mem_splits(B, M, D)}
            for v in variants:
                for _ in range(args.warmup):
                    step(v)
                torch.cuda.synchronize()
                out = step(v)
                if out is not None:
                    res[f"{v}_loss"] = round(out.item(), 5)
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
            best = min(res["fused_order0_median_ms"], res["fused_order1_median_ms"])
            res["chain_over_fused"] = round(res["chain_median_ms"] / best, 2)
            res["fused_over_matmul3"] = round(best / res["matmul3_median_ms"], 2)
            lib.pfr_set_tuning(b"pair_mem_order", 1)      # the library's default
            print(json.dumps(res), flush=True)
            lines.append(json.dumps(res))
            del fused, mem32, b16
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
