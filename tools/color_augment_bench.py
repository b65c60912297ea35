"""Times the head augmentation pipeline (uniform 224 x 224 uint8 frames → float32 NCHW, batch 256) in three modes, interleaved on
one box: the four further transforms off, flip only, and everything on (flip 0.5, ColorJitter(0.2, 0.2, 0.2, 0.02), grayscale 0.1,
erasing 0.25).  Wall clock of `apply` with a device synchronisation (host record building and upload included, as a training step
sees it) and the device time alone (HIP events around `apply`).  "off" runs twice per round, so the spread between the two legs is
the run-to-run noise the other modes are read against.  Writes profiles/color_augment.txt.

    python tools/color_augment_bench.py [--rounds 9] [--batch 256]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    import torch
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    n, dev = args.batch, "cuda:0"
    x = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device=dev)
    kinds = {'off': {}, 'off (second leg)': {}, 'flip only': dict(p_hflip=0.5),
             'everything on': dict(p_hflip=0.5, color_jitter=(0.2, 0.2, 0.2, 0.02), p_grayscale=0.1, erasing=dict(p=0.25))}
    augs = {k: DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, torch.Generator().manual_seed(3), **kw) for k, kw in kinds.items()}
    dec = {k: (*a.draw(n, 224, 224), a.draw_extra(n, 224, 224)) for k, a in augs.items()}

    def run(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record()
        for _ in range(args.inner):
            augs[k].apply(x, *dec[k])
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / args.inner, e0.elapsed_time(e1) * 1e-3 / args.inner

    wall, devt = {k: [] for k in kinds}, {k: [] for k in kinds}
    for r in range(3 + args.rounds):           # three warm-up rounds, then interleaved measured rounds
        for k in kinds:
            w, d = run(k)
            if r >= 3:
                wall[k].append(w)
                devt[k].append(d)
    mb = n * 224 * 224 * 3 / 1e6
    lines = [f"# tools/color_augment_bench.py on one MI355X: head pipeline, batch {n}, 224 x 224 uint8 frames ({mb:.1f} MB), {args.rounds} interleaved rounds of "
             f"{args.inner} calls after 3 warm-up rounds; median (min .. max) per call",
             "# wall = host record building + upload + launches + synchronisation; events = HIP events around the same calls"]
    for k in kinds:
        w, d = wall[k], devt[k]
        lines.append(f"{k:18s} wall {statistics.median(w) * 1e3:7.3f} ms ({min(w) * 1e3:.3f} .. {max(w) * 1e3:.3f})   events {statistics.median(d) * 1e3:7.3f} ms "
                     f"({min(d) * 1e3:.3f} .. {max(d) * 1e3:.3f})   {n / statistics.median(w):10.0f} img/s")
    text = "\n".join(lines) + "\n"
    print(text)
    open(os.environ.get("PFR_BENCH_OUT") or os.path.join(ROOT, "profiles", "color_augment.txt"), "w").write(text)   # PFR_BENCH_OUT: write somewhere else


if __name__ == "__main__":
    main()
