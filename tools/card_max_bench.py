"""Cost of the max-strategy card matching (match.card_match(strategy='max') -> pfr_card_max_scores): 10 000 query cards x 1 000 000 gallery
cards with 1-5 photos each, D = 512, top 100.  These legs run interleaved round by round in one process:
  mean_bf16    match.card_match(strategy='mean', bf16): centroids + ONE card GEMM with the running top-k (what the repository had)
  max_bf16     match.card_match(strategy='max', bf16): row preparation, photo GEMM with the segmented-max epilogue per gallery chunk, running
               top-k, exact fp32 re-scoring of the candidates
  max_fp32     the same in fp32 (exact selection, no re-scoring)
  max_kernel   pfr_card_max_scores alone over the whole gallery on prepared bf16 rows (no top-k): the kernel against its yardstick
  gemm         the plain bf16 score GEMM of the same FLOPs (photo rows x photo rows) that WRITES its fp32 scores, per chunk of photo columns
  torch_bf16 / torch_fp32
               the baseline a user had to write: chunked photo q @ g.T written out (bf16 rows as prepared above; the scores as torch's bf16
               matmul returns them, or converted to fp32 — scatter_reduce's bf16 atomics turned out slower than the copy), then a
               segmented max with torch indexing (scatter_reduce amax over the columns of every gallery card, then over the rows of every
               query card); chunk boundaries, index maps and buffers prepared outside the timed region, no host synchronisation inside
               it, no top-k
Writes profiles/card_max.txt.     python tools/card_max_bench.py [--q 10000] [--g 1000000] [--rounds 5] [--out PATH]
Every leg is timed on the host around one call between two device synchronisations; the file gives the median, the minimum and the maximum
over the rounds.  Condition: max_bf16 is not slower than the faster torch leg beyond the round-to-round spread reported here."""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D, K = 512, 100


def cards(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    cnt = torch.randint(1, 6, (n,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)])
    gd = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(int(seg[-1]), D, generator=gd, device=dev), seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=10000)
    ap.add_argument("--g", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--photo-chunk", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "card_max.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("card_max_bench.py needs an MI355X")
    dev = torch.device("cuda", 0)
    from pets_face_recognition_amd import match
    from pets_face_recognition_amd._hip import ops
    qe, qseg = cards(args.q, 1, dev)
    ge, gseg = cards(args.g, 2, dev)
    Pq, Pg = qe.shape[0], ge.shape[0]
    bf = torch.bfloat16
    qs = match._CardSide(qe, qseg, bf, dev, False, "bench")
    gs = match._CardSide(ge, gseg, bf, dev, False, "bench")
    card_chunk = 131072
    sbuf = torch.empty((args.q, card_chunk), dtype=torch.float32, device=dev)
    pc = args.photo_chunk
    pbuf = torch.empty((Pq, 1, 1, pc), dtype=torch.float32, device=dev)
    qcard = torch.repeat_interleave(torch.arange(args.q), qseg[1:] - qseg[:-1]).to(dev)
    gcard = torch.repeat_interleave(torch.arange(args.g), gseg[1:] - gseg[:-1]).to(dev)

    def max_kernel():
        for c0 in range(0, args.g, card_chunk):
            match._card_max_chunk(qs, gs, bf, c0, min(card_chunk, args.g - c0), sbuf, card_chunk)

    def gemm():
        for r0 in range(0, Pg, pc):
            n = min(pc, Pg - r0)
            ops.conv2d_fwd(qs.op.view(Pq, 1, 1, D), gs.op[r0:r0 + n].view(n, 1, 1, D), out=pbuf)

    # chunks of whole gallery cards for the baseline (each ends at the last card boundary at or below its first row + pc), the card maps
    # and the result buffers: all prepared once, outside the timed region, as a careful user would
    chunks, c0 = [], 0
    while c0 < args.g:
        c1 = int(torch.searchsorted(gseg, min(int(gseg[c0]) + pc, Pg), right=True)) - 1
        chunks.append((int(gseg[c0]), int(gseg[c1]), c0, c1))
        c0 = c1
    col_idx = [(gcard[r0:r1] - a)[None, :].expand(Pq, -1) for r0, r1, a, b in chunks]
    width = max(b - a for _, _, a, b in chunks)
    row_idx = qcard[:, None].expand(-1, width)
    bufs = {t: (torch.empty((Pq, width), dtype=t, device=dev), torch.empty((args.q, width), dtype=t, device=dev)) for t in (bf, torch.float32)}

    def torch_baseline(sdt):
        cols, outb = bufs[sdt]
        for (r0, r1, a, b), ci in zip(chunks, col_idx):
            s = (qs.op @ gs.op[r0:r1].t()).to(sdt)           # the photo score chunk, written out
            cols.fill_(-float("inf"))
            cols[:, :b - a].scatter_reduce_(1, ci, s, "amax")
            outb.fill_(-float("inf"))
            outb.scatter_reduce_(0, row_idx, cols, "amax")
        return outb

    legs = {"mean_bf16": lambda: match.card_match(qe, qseg, ge, gseg, k=K, compute_dtype=bf),
            "max_bf16": lambda: match.card_match(qe, qseg, ge, gseg, k=K, compute_dtype=bf, strategy="max"),
            "max_fp32": lambda: match.card_match(qe, qseg, ge, gseg, k=K, compute_dtype=torch.float32, strategy="max"),
            "max_kernel": max_kernel, "gemm": gemm, "torch_bf16": lambda: torch_baseline(bf), "torch_fp32": lambda: torch_baseline(torch.float32)}
    for fn in legs.values():                 # warm-up of every shape
        fn()
        torch.cuda.synchronize()
    ms = {n: [] for n in legs}
    order = list(legs)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            legs[name]()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    flops = 2.0 * Pq * Pg * D
    lines = [f"# tools/card_max_bench.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  {args.q} x {args.g} cards, 1-5 photos "
             f"({Pq} x {Pg} photo rows), D={D}, k={K}; {args.rounds} interleaved rounds x 1 call, median (min .. max) ms over the rounds"]
    med = {}
    for n, v in ms.items():
        med[n] = statistics.median(v)
        lines.append(f"{n:11s} {med[n]:10.1f}  ({min(v):.1f} .. {max(v):.1f})" + (f"   {flops / med[n] / 1e9:.0f} TFLOP/s of photo products" if n in ("max_kernel", "gemm") else ""))
    tb = min(("torch_bf16", "torch_fp32"), key=lambda n: med[n])          # the condition is taken against the FASTER baseline
    spread = max(ms["max_bf16"]) - min(ms["max_bf16"]) + max(ms[tb]) - min(ms[tb])
    lines.append(f"max_kernel vs gemm (plain score GEMM that writes its scores): {med['gemm'] / med['max_kernel']:.2f} x its speed "
                 f"(pair_hist reached 0.83 x; context, not a gate)")
    lines.append(f"max_bf16 vs the faster torch baseline ({tb}): {med[tb] / med['max_bf16']:.2f} x faster; condition max_bf16 <= torch + spread "
                 f"({med['max_bf16']:.1f} <= {med[tb]:.1f} + {spread:.1f}): {'met' if med['max_bf16'] <= med[tb] + spread else 'NOT met'}")
    lines.append(f"max_bf16 vs mean_bf16: {med['max_bf16'] / med['mean_bf16']:.1f} x the cost (the mean collapses to one GEMM of {args.q} x {args.g} centroids)")
    lines.append("# epilogue design measured here: two-stage (row, then column) reduction through an LDS table R that aliases the operand tiles, 70 720 bytes per workgroup, 2 workgroups per CU; the other open design, a dense [128][128] table that does not alias (98 KiB, 1 workgroup per CU), was not built")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
