"""Times the landmark alignment at batch 256 on the ragged frames of tools/ragged_augment_bench.py, legs interleaved in one process:

    warp      pfr_align_warp alone (HIP events around the C-ABI call), matrices already on the device
    align     DeviceAlign end to end: host solve, upload of the tables, the launch; wall clock with a device synchronisation
    fit       pfr_augment_fit in resize mode on the same batch (HIP events): the stage the alignment replaces in a head pipeline
    pillow    Image.transform(PERSPECTIVE, BILINEAR) of the same frames and matrices on 16 worker processes that hold their own frames

Three warm-up rounds, then the measured rounds; median (min .. max).  Writes profiles/align.txt.

    python tools/align_bench.py [--rounds 9] [--batch 256]
"""
import argparse
import datetime
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ragged_augment_bench import _frames  # noqa: E402

OUT = 224
BASE = np.array([[0.3125, 0.36], [0.6875, 0.36], [0.5, 0.72]]) * OUT


def _landmarks(shapes, seed=5):
    """three landmarks per frame: the base triangle rotated (+-20 degrees), scaled so that the crop covers 40..80 % of the shorter side"""
    rs = np.random.RandomState(seed)
    out = []
    for h, w in shapes:
        th, k = np.deg2rad(rs.uniform(-20, 20)), rs.uniform(0.4, 0.8) * min(h, w) / OUT
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out.append((BASE - OUT / 2) @ R.T * k + np.array([w, h]) * (0.5 + rs.uniform(-0.05, 0.05, 2)))
    return np.stack(out)


_WORKER = None


def _worker_init(n):
    global _WORKER
    _WORKER = _frames(n)


def _pil_one(job):
    from PIL import Image
    i, coeffs = job
    return np.asarray(Image.fromarray(_WORKER[i]).transform((OUT, OUT), Image.PERSPECTIVE, coeffs, Image.BILINEAR)).shape


def _pillow_coeffs(minv):
    M = np.asarray(minv, np.float64).reshape(3, 3)
    P = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1.0]]) @ M @ np.array([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1.0]])
    return (P / P[2, 2]).reshape(9)[:8].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    n = args.batch
    frames = _frames(n)
    pool = mp.get_context("spawn").Pool(args.workers, initializer=_worker_init, initargs=(n,))   # before the GPU is initialised
    pool.map(_pil_one, [(0, [1, 0, 0, 0, 1, 0, 0, 0])] * args.workers * 4)

    import torch
    from pets_face_recognition_amd._hip import lib
    from pets_face_recognition_amd.data_loading import pack_frames, DeviceAlign, simple_val_augmentation
    from pets_face_recognition_amd.data_loading import align as A
    dev = "cuda:0"
    packed = pack_frames(frames)
    x = {'data': packed['data'].to(dev), 'shape': packed['shape'], 'shape_host': packed['shape_host']}
    pts = _landmarks(packed['shape_host'])
    al = DeviceAlign(BASE, (OUT, OUT, 3))
    minv, valid = A.solve(pts, BASE)
    assert valid.all()
    minv_d = torch.from_numpy(minv).to(dev)
    fit = simple_val_augmentation()
    jobs = [(i, _pillow_coeffs(minv[i])) for i in range(n)]

    def events(entry, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        orig = getattr(lib, entry)

        def timed(*a):
            e0.record()
            rc = orig(*a)
            e1.record()
            return rc
        setattr(lib, entry, timed)
        try:
            fn()
        finally:
            setattr(lib, entry, orig)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def wall(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def pillow():
        t = time.perf_counter()
        pool.map(_pil_one, jobs, chunksize=4)
        return time.perf_counter() - t

    legs = ('warp', 'align', 'solve', 'fit', 'pillow')
    times = {k: [] for k in legs}
    for r in range(3 + args.rounds):
        t0 = time.perf_counter()
        A.solve(pts, BASE)
        row = {'solve': time.perf_counter() - t0,
               'warp': events('pfr_align_warp', lambda: A.warp(x, minv_d, (OUT, OUT))),
               'align': wall(lambda: al(x, pts)),
               'fit': events('pfr_augment_fit', lambda: fit.fit_apply(x)),
               'pillow': pillow() if r >= 2 else None}
        if r >= 3:
            for k, v in row.items():
                times[k].append(v)
    pool.close()
    pool.join()

    out_mb = n * OUT * OUT * 3 / 1e6
    src_mb = sum(f.size for f in frames) / 1e6
    names = {'warp': 'pfr_align_warp alone (HIP events)', 'align': 'DeviceAlign end to end (host solve + uploads + launch, wall clock)',
             'solve': 'pfr_align_solve alone (host)', 'fit': 'pfr_augment_fit, resize mode, launches alone (HIP events)',
             'pillow': f'Pillow Image.transform(PERSPECTIVE, BILINEAR) on {args.workers} processes'}
    lines = [f"# tools/align_bench.py on one MI355X, {datetime.date.today().isoformat()}: batch {n}, output {OUT}x{OUT}, {args.rounds} interleaved rounds after "
             f"3 warm-up rounds; median (min .. max)",
             f"# ragged frames: sides 64..1400, aspect within 1:3, {src_mb:.0f} MB per batch; the warp writes {out_mb:.1f} MB"]
    for k in legs:
        v = times[k]
        med = statistics.median(v)
        lines.append(f"{names[k]:<78s} {n / med:>9.0f} img/s {med * 1e3:>9.3f} ms ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f})")
    w, f = statistics.median(times['warp']), statistics.median(times['fit'])
    lines.append(f"warp / fit = {w / f:.2f}; the warp's output alone: {out_mb / 1e6 / w:.3f} TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "align.txt"), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
