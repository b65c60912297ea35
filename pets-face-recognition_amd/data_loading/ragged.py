"""Ragged frame batch: N uint8 HWC frames of different sizes in one flat buffer.

    batch['x'] = {'data': uint8 [total_bytes], 'shape': int32 [N, 2], 'shape_host': numpy int32 [N, 2]}

'data' holds the frames back to back, each starting on a 16-byte boundary (so the device kernels can use 16-byte loads);
'shape' holds (H, W) per frame.  It is a plain dict of tensors: `DevicePrefetcher._map`, `Trainer._to_device` and
`Trainer._batch_size` pin, copy and skip over it like any other nested batch.  'shape_host' is the same array as numpy: those
helpers move tensors only, so it stays on the host, where the fit stage plans its sizes and coefficient tables without waiting
for the device ('shape' travels with the batch and is read back only when 'shape_host' is absent).  `ragged_collate` is this project's
counterpart of the reference's `list_img_rec_collate_fn` (/root/reference/data_loading/dataset.py), which keeps the
frames of a batch as a Python list because the detector's raw crops have no common size.
"""
import numpy as np
import torch

ALIGN = 16
MAX_SIDE = 4096


def ragged_offsets(shape):
    """shape int [N, 2] = (H, W) → (int64 [N] byte offset of each frame, total bytes)"""
    shape = np.asarray(shape, dtype=np.int64).reshape(-1, 2)
    nbytes = (shape[:, 0] * shape[:, 1] * 3 + ALIGN - 1) // ALIGN * ALIGN
    off = np.zeros(len(shape), np.int64)
    np.cumsum(nbytes[:-1], out=off[1:])
    return off, int(nbytes.sum())


def pack_frames(frames):
    """list of uint8 [H, W, 3] tensors / arrays → the ragged dict"""
    frames = [torch.as_tensor(f) for f in frames]
    for f in frames:
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise ValueError(f"ragged frame must be uint8 [H, W, 3], got {f.dtype} {tuple(f.shape)}")
    shape = torch.tensor([[f.shape[0], f.shape[1]] for f in frames], dtype=torch.int32).reshape(-1, 2)
    off, total = ragged_offsets(shape.numpy())
    data = torch.zeros(total, dtype=torch.uint8)
    for f, o in zip(frames, off):
        data[o:o + f.numel()] = f.reshape(-1)
    return {'data': data, 'shape': shape, 'shape_host': shape.numpy().copy()}


def unpack_frames(x):
    """the ragged dict → list of uint8 [H, W, 3] views"""
    shape = x['shape'].cpu().numpy()
    off, _ = ragged_offsets(shape)
    return [x['data'][o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(off, shape)]


def ragged_collate(samples):
    """samples: dataset items whose 'x' is a uint8 [H, W, 3] tensor; a 'mask' (uint8 [H, W], the frame's size) is packed the same way
    (data_loading/align.py pack_masks); every other key, the landmarks 'pts' among them, is collated as usual"""
    from torch.utils.data import default_collate
    batch = default_collate([{k: v for k, v in s.items() if k not in ('x', 'mask')} for s in samples])
    batch['x'] = pack_frames([s['x'] for s in samples])
    if 'pts' in batch:
        batch['pts_host'] = batch['pts'].numpy().copy()      # stays on the host like 'shape_host': the solve runs there
    if samples and 'mask' in samples[0]:
        from .align import pack_masks
        batch['mask'] = pack_masks([s['mask'] for s in samples])
    return batch


def is_ragged(x):
    return isinstance(x, dict) and 'data' in x and 'shape' in x


def seeded_size(seed, lo=64, hi=1400, max_aspect=3.0):
    """(H, W) drawn from `seed`: sides in [lo, hi], aspect ratio within 1:max_aspect … max_aspect:1"""
    rs = np.random.RandomState(seed)
    long_side = int(rs.randint(lo, hi + 1))
    short_min = max(lo, int(np.ceil(long_side / max_aspect)))
    short_side = int(rs.randint(short_min, long_side + 1))
    return (long_side, short_side) if rs.randint(2) else (short_side, long_side)


def seeded_frame(seed, H, W):
    """a reproducible uint8 [H, W, 3] frame: a smooth pattern plus noise, clipped to a per-seed range (one in four frames
    has a narrow range, one in eight a flat band) so that autocontrast and the blur have something to do"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    px, py = 5.0 + seed % 11, 4.0 + seed % 7
    base = np.stack([127 + 90 * np.sin(xx / px + c) * np.cos(yy / (py + c)) for c in range(3)], -1)
    noise = rs.randn(H, W, 3) * (3 + 18 * (seed % 3))
    lo, hi = [(0, 255), (30, 200), (5, 250), (60, 140)][seed % 4]
    img = np.clip(base + noise, lo, hi).astype(np.uint8)
    if seed % 8 == 7:
        img[..., 1] = 77
    return img
