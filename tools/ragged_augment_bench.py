"""Times the ragged-frame input pipelines at batch 256, interleaved:

    device   simple family (fit resize + colour first) and body family (fit thumbnail_pad + geometry first) on seeded ragged
             frames ALREADY ON THE DEVICE: host planning + upload of the tables + kernels, wall clock with a device synchronisation
             (the upload of the frames themselves is in the end-to-end runs of tools/ragged_e2e.sh, not here)
    pillow   the same two pipelines in Pillow on 16 worker processes that hold their own frames (what the reference's dataloader
             workers do; only indices and decisions go through the pipes)
    uniform  the existing head pipeline on a uniform 224 x 224 uint8 batch

and the fit launches alone (HIP events): bytes moved over time, as a fraction of the streaming-pass HBM rate that
profiles/r06_bn_bench.txt reports (5.2 TB/s, bn_act rows of 100+ MB).  Writes profiles/ragged_augment.txt.

    python tools/ragged_augment_bench.py [--rounds 7] [--batch 256]
"""
import argparse
import multiprocessing as mp
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STREAM_TBS = 5.2


def _frames(n, seed=11):
    """n ragged frames cut from one seeded 1400 x 1400 frame (sides 64..1400, aspect within 1:3)"""
    from pets_face_recognition_amd.data_loading.ragged import seeded_frame, seeded_size
    base = seeded_frame(seed, 1400, 1400)
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = seeded_size(seed * 1000 + i)
        y, x = rs.randint(0, 1400 - h + 1), rs.randint(0, 1400 - w + 1)
        out.append(np.ascontiguousarray(base[y:y + h, x:x + w]))
    return out


_WORKER_FRAMES = None


def _worker_init(n):
    """every Pillow worker holds its own copy of the frames, like a loader worker that reads its own files: jobs carry indices only"""
    global _WORKER_FRAMES
    _WORKER_FRAMES = _frames(n)


def _pil_one(job):
    from PIL import Image, ImageEnhance, ImageOps
    i, family, sharp, contrast, top, left, angle = job
    img = Image.fromarray(_WORKER_FRAMES[i])

    def color(im):
        if sharp:
            im = ImageEnhance.Sharpness(im).enhance(0)
        return ImageOps.autocontrast(im) if contrast else im

    if family == 'simple':
        img = color(img).resize((224, 224), Image.BILINEAR)
        crop, size = 220, 224
    else:
        img.thumbnail((256, 256))
        dw, dh = 256 - img.size[0], 256 - img.size[1]
        img = ImageOps.expand(img, (dw // 2, dh // 2, dw - dw // 2, dh - dh // 2))
        crop, size = 252, 256
    img = img.crop((left, top, left + crop, top + crop)).resize((size, size), Image.BILINEAR)
    img = img.rotate(angle, Image.NEAREST, fillcolor=(0, 0, 0))
    if family == 'body':
        img = color(img)
    return (np.asarray(img).transpose(2, 0, 1).astype(np.float32) / 255).shape


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()
    n = args.batch
    frames = _frames(n)
    # started before the GPU is initialised; the workers never touch it
    pool = mp.get_context("spawn").Pool(args.workers, initializer=_worker_init, initargs=(n,))
    pool.map(_pil_one, [(0, 'simple', 1, 1, 0, 0, 1.0)] * args.workers * 4)

    import torch
    from pets_face_recognition_amd._hip import lib
    from pets_face_recognition_amd.data_loading import (pack_frames, simple_train_augmentation, body_train_augmentation,
                                                        train_augmentation)
    dev = "cuda:0"
    packed = pack_frames(frames)
    x = {'data': packed['data'].to(dev), 'shape': packed['shape']}
    uni = torch.randint(0, 256, (n, 224, 224, 3), dtype=torch.uint8, device=dev)
    augs = {'simple': simple_train_augmentation(torch.Generator().manual_seed(1)),
            'body': body_train_augmentation(torch.Generator().manual_seed(2)),
            'uniform': train_augmentation(torch.Generator().manual_seed(3))}
    dec = {k: a.draw(n, *(a.fit[1] if a.fit else (224, 224))) for k, a in augs.items()}

    def device_run(k):
        torch.cuda.synchronize()
        t = time.perf_counter()
        augs[k].apply(uni if k == 'uniform' else x, *dec[k])
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def pillow_run(k):
        f, a = dec[k]
        jobs = [(i, k, int(f[i, 0]), int(f[i, 1]), int(f[i, 2]), int(f[i, 3]), float(a[i])) for i in range(n)]
        t = time.perf_counter()
        pool.map(_pil_one, jobs, chunksize=4)
        return time.perf_counter() - t

    # the fit launches alone, HIP events around the C-ABI call
    def fit_only(k):
        a = augs[k]
        cf = dec[k][0][:, :2] if k == 'simple' else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        orig = lib.pfr_augment_fit

        def timed(*args):
            e0.record()
            rc = orig(*args)
            e1.record()
            return rc
        lib.pfr_augment_fit = timed
        try:
            a.fit_apply(x, cf)
        finally:
            lib.pfr_augment_fit = orig
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    times = {k: [] for k in ('simple', 'body', 'uniform', 'pillow simple', 'pillow body', 'fit simple', 'fit body')}
    for r in range(3 + args.rounds):           # three warm-up rounds, then interleaved measured rounds
        row = {'simple': device_run('simple'), 'pillow simple': pillow_run('simple') if r >= 2 else None, 'body': device_run('body'),
               'pillow body': pillow_run('body') if r >= 2 else None, 'uniform': device_run('uniform'),
               'fit simple': fit_only('simple'), 'fit body': fit_only('body')}
        if r >= 3:
            for k, v in row.items():
                times[k].append(v)
    pool.close()
    pool.join()

    src_bytes = sum(f.size for f in frames)
    shape = packed['shape'].numpy()
    lines = [f"# tools/ragged_augment_bench.py on one MI355X: batch {n}, {args.rounds} interleaved rounds after 3 warm-up rounds; median (min .. max)",
             f"# ragged frames: sides 64..1400, aspect within 1:3, {src_bytes / 1e6:.0f} MB per batch (mean {src_bytes / n / 1e6:.2f} MB per frame); "
             f"Pillow legs on {args.workers} worker processes"]
    for k in ('simple', 'body', 'uniform', 'pillow simple', 'pillow body'):
        t = times[k]
        med = statistics.median(t)
        what = {'simple': 'device simple family (fit resize 224 + train)', 'body': 'device body family (fit thumbnail_pad 256 + train, geometry first)',
                'uniform': 'device head pipeline, uniform 224x224 frames', 'pillow simple': 'Pillow simple family', 'pillow body': 'Pillow body family'}[k]
        lines.append(f"{what:72s} {n / med:12.0f} img/s   {med * 1e3:9.2f} ms ({min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f})")
    f_s = dec['simple'][0].numpy()
    sharp_bytes = sum(int(shape[i, 0]) * int(shape[i, 1]) * 3 for i in range(n) if f_s[i, 0])
    any_bytes = sum(int(shape[i, 0]) * int(shape[i, 1]) * 3 for i in range(n) if f_s[i, 0] or f_s[i, 1])
    moved = {'fit simple': src_bytes + n * 224 * 224 * 3 + any_bytes + sharp_bytes,          # + the pre pass reads and the blurred copies written
             'fit body': src_bytes + n * 256 * 256 * 3}                                        # + the reduced copies (at most 1/4 of the source each way)
    for k in ('fit simple', 'fit body'):
        med = statistics.median(times[k])
        tbs = moved[k] / med / 1e12
        lines.append(f"{k + ' launches alone (HIP events)':72s} {med * 1e3:9.3f} ms   {moved[k] / 1e6:.0f} MB compulsory -> {tbs:.3f} TB/s = "
                     f"{100 * tbs / STREAM_TBS:.1f} % of the {STREAM_TBS} TB/s streaming-pass rate")
    out = os.path.join(ROOT, "profiles", "ragged_augment.txt")
    text = "\n".join(lines) + "\n"
    print(text)
    open(os.environ.get("PFR_BENCH_OUT") or out, "w").write(text)   # PFR_BENCH_OUT: write somewhere else


if __name__ == "__main__":
    main()
