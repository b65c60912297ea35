"""Landmark alignment on the device: the reference's `preprocessor/align.py` (fit a homography from three or four landmarks onto
`base_pts`, warp the frame to `dsize`; called by Preproc3/7/9/11 on the raw frame and by PreprocCombined on the masked frame) for a
whole ragged batch of raw frames (data_loading/ragged.py).

    solve(pts, base_pts)            host: landmarks -> inverse maps (pfr_align_solve)
    DeviceAlign(base_pts, dsize)    ragged batch + landmarks [+ masks] -> uint8 [N, h, w, 3] on the device (pfr_align_warp)
    align_torch(...)                the same contract in numpy on CPU tensors, for device='cpu' configs

OpenCV is not available to this project, so bit-identity with a cv2 build cannot be tested and is NOT claimed.  The contract is ours
(include/pfr_hip.h states every operation).  It follows OpenCV's published scheme for warpPerspective(..., INTER_LINEAR,
BORDER_CONSTANT 0): inverse map in fp64, source coordinates quantised to 1/32 pixel, 15-bit integer weights.  It is pinned two ways: a
numpy restatement (tests/align_oracle.py), which the device must equal bit for bit, and Pillow's Image.transform(PERSPECTIVE,
BILINEAR), an independent implementation, which must lie within a derived bound of the restatement (tests/test_align_host.py)."""
import numpy as np
import torch

from .._hip import lib, PfrError
from .ragged import ALIGN, MAX_SIDE, is_ragged, ragged_offsets, unpack_frames

_MODES = {'reference': 0, 'similarity': 1}


def _mode(estimate):
    if estimate not in _MODES:
        raise PfrError(f"align: estimate must be 'reference' or 'similarity', got {estimate!r}")
    return _MODES[estimate]


def _points(pts, base_pts, estimate):
    base = np.ascontiguousarray(np.asarray(base_pts, dtype=np.float64))
    if base.ndim != 2 or base.shape[1] != 2:
        raise PfrError(f"align: base_pts must be [npts, 2] = (x, y), got {base.shape}")
    npts = base.shape[0]
    if estimate == 'reference' and npts not in (3, 4):
        raise PfrError(f"align: estimate='reference' takes 3 or 4 landmarks, got {npts}")
    if estimate == 'similarity' and npts < 2:
        raise PfrError(f"align: estimate='similarity' takes at least 2 landmarks, got {npts}")
    if isinstance(pts, torch.Tensor):
        pts = pts.detach().cpu().numpy()
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float64))
    if pts.ndim != 3 or pts.shape[1:] != (npts, 2):
        raise PfrError(f"align: pts must be [N, {npts}, 2] = (x, y) like base_pts, got {pts.shape}")
    return pts, base


def solve(pts, base_pts, estimate='reference', min_distance=5.0):
    """pts [N, npts, 2] = (x, y) per frame, base_pts [npts, 2] -> (minv float64 [N, 9], valid bool [N]) on the host.  minv is the
    inverse map (output pixel -> source pixel); a frame whose landmarks are not more than min_distance apart, collinear or
    non-finite has valid False and an all-zero matrix."""
    mode = _mode(estimate)
    pts, base = _points(pts, base_pts, estimate)
    n = pts.shape[0]
    minv, valid = np.zeros((n, 9), np.float64), np.zeros(n, np.int32)
    lib.pfr_align_solve(mode, pts.ctypes.data, base.ctypes.data, n, base.shape[0], float(min_distance), minv.ctypes.data, valid.ctypes.data)
    return minv, valid.astype(bool)


def pack_masks(masks):
    """list of uint8 [H, W] masks -> {'data': uint8 [bytes], 'offsets': int64 [N], 'offsets_host': numpy int64 [N]}: the planes back to back, each starting on a
    16-byte boundary.  A zero byte drops the pixel, any other keeps it."""
    masks = [torch.as_tensor(m) for m in masks]
    for m in masks:
        if m.dtype != torch.uint8 or m.dim() != 2:
            raise ValueError(f"mask must be uint8 [H, W], got {m.dtype} {tuple(m.shape)}")
    nbytes = [(m.numel() + ALIGN - 1) // ALIGN * ALIGN for m in masks]
    off = np.zeros(len(masks), np.int64)
    np.cumsum(nbytes[:-1], out=off[1:])
    data = torch.zeros(int(sum(nbytes)), dtype=torch.uint8)
    for m, o in zip(masks, off):
        data[o:o + m.numel()] = m.reshape(-1)
    # 'offsets_host' is the same array as numpy: it stays on the host when the batch moves to the device (like 'shape_host' of the frames)
    return {'data': data, 'offsets': torch.from_numpy(off), 'offsets_host': off.copy()}


def _dsize(dsize):
    d = tuple(int(v) for v in dsize)
    if len(d) == 3 and d[2] == 3:       # the reference's (h, w, c): it hands dsize[:-1][::-1] to OpenCV
        d = d[:2]
    if len(d) != 2 or d[0] < 0 or d[1] < 0 or max(d) > MAX_SIDE:
        raise PfrError(f"align: dsize must be (h, w) or (h, w, 3) with sides up to {MAX_SIDE}, got {dsize!r}")
    return d


def _shapes(x):
    host = x.get('shape_host')
    return np.asarray(host if host is not None else x['shape'].cpu().numpy()).astype(np.int32).reshape(-1, 2)


def _mask_offsets(shape):
    nbytes = (shape[:, 0].astype(np.int64) * shape[:, 1] + ALIGN - 1) // ALIGN * ALIGN
    off = np.zeros(len(shape), np.int64)
    np.cumsum(nbytes[:-1], out=off[1:])
    return off, int(nbytes.sum())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def warp(x, minv, dsize, mask=None):
    """the warp alone: ragged dict on the GPU, minv float64 [N, 9] (host or device), mask as `pack_masks` returns it (its planes
    have the frames' sizes) -> uint8 [N, h, w, 3] on the GPU"""
    oh, ow = _dsize(dsize)
    if not is_ragged(x) or not x['data'].is_cuda or x['data'].dtype != torch.uint8 or x['data'].dim() != 1:
        raise PfrError("align: expects the ragged dict {'data': uint8 [bytes], 'shape': int32 [N, 2]} with 'data' on the GPU")
    data, dev = x['data'].contiguous(), x['data'].device
    shape = _shapes(x)
    n = shape.shape[0]
    if n and (int(shape.min()) < 1 or int(shape.max()) > MAX_SIDE):
        raise PfrError(f"align: frame sides must be 1..{MAX_SIDE}")
    off, total = ragged_offsets(shape)
    if total > data.numel():
        raise PfrError(f"align: 'shape' describes {total} bytes, 'data' holds {data.numel()}")
    minv = torch.as_tensor(minv, dtype=torch.float64).reshape(-1, 9)
    if minv.shape[0] != n:
        raise PfrError(f"align: {minv.shape[0]} matrices for {n} frames")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)
    minv_d = minv.contiguous() if minv.is_cuda else up(minv.numpy())
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    if n == 0 or oh == 0 or ow == 0:
        return out
    off_d, shape_d = up(off), up(shape)
    mdata = moff_d = None
    if mask is not None:
        moff, mtotal = _mask_offsets(shape)
        mdata = mask['data'].to(dev).contiguous()
        # the planes have the frames' sizes, so their offsets follow from 'shape' on the host.  mask['offsets'] must agree with them
        # (another frame order or other plane sizes with the same total would be read at the wrong places): compared where that costs
        # no device round trip, i.e. while the offsets are still on the host
        if mdata.dtype != torch.uint8 or mdata.dim() != 1 or mtotal != mdata.numel():
            raise PfrError("align: the mask planes do not have the frames' sizes (pack_masks of one uint8 [H, W] mask per frame)")
        given = mask.get('offsets_host', mask.get('offsets'))
        if given is not None and not (torch.is_tensor(given) and given.is_cuda):
            if not np.array_equal(np.asarray(given, dtype=np.int64).reshape(-1), moff):
                raise PfrError("align: mask['offsets'] are not the offsets of planes with the frames' sizes, in the frames' order")
        moff_d = up(moff)
    lib.pfr_align_warp(data.data_ptr(), off_d.data_ptr(), shape_d.data_ptr(), minv_d.data_ptr(),
                       mdata.data_ptr() if mdata is not None else None, moff_d.data_ptr() if moff_d is not None else None,
                       n, oh, ow, out.data_ptr(), _stream())
    return out


class DeviceAlign:
    """base_pts [npts, 2] = (x, y) in the aligned crop; dsize (h, w) or the reference's (h, w, c).  jitter > 0 adds seeded Gaussian
    noise of that many pixels to the landmarks before the solve: a training augmentation that a dataset aligned offline cannot
    offer; off by default.  Called with a ragged batch on the GPU, landmarks [N, npts, 2] and optionally masks (`pack_masks`):
    -> (uint8 [N, h, w, 3] on the GPU, valid bool [N] on the host).  Invalid frames come back all zero."""

    def __init__(self, base_pts, dsize, estimate='reference', min_distance=5.0, jitter=0.0, generator=None):
        _mode(estimate)
        self.estimate, self.min_distance, self.jitter, self.generator = estimate, float(min_distance), float(jitter), generator
        self.dsize = _dsize(dsize)
        self.base_pts = _points(np.zeros((0,) + np.asarray(base_pts).shape), base_pts, estimate)[1]
        if self.jitter < 0:
            raise ValueError("DeviceAlign: jitter must be >= 0")
        self.last_pts = None

    def landmarks(self, pts):
        """the landmarks the solve sees: `pts` plus the jitter, float64 [N, npts, 2] on the host"""
        pts, _ = _points(pts, self.base_pts, self.estimate)
        if self.jitter > 0:
            noise = torch.randn(pts.shape, generator=self.generator, dtype=torch.float64).numpy()
            pts = pts + self.jitter * noise
        return pts

    def __call__(self, x, pts, mask=None):
        pts = self.landmarks(pts)
        self.last_pts = pts
        minv, valid = solve(pts, self.base_pts, self.estimate, self.min_distance)
        return warp(x, minv, self.dsize, mask), valid


# ---- the same contract on the host -------------------------------------------------------------------------------------------
def _warp_numpy(frame, m, oh, ow, mask=None):
    """one frame, the contract of include/pfr_hip.h operation by operation (numpy's elementwise operations never fuse a multiply-add)"""
    H, W = frame.shape[:2]
    x = np.arange(ow, dtype=np.float64)[None, :]
    y = np.arange(oh, dtype=np.float64)[:, None]
    with np.errstate(all='ignore'):
        X0, Y0, W0 = np.broadcast_arrays((m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5], (m[6] * x + m[7] * y) + m[8])
        s = np.divide(32.0, W0, out=np.zeros(W0.shape, np.float64), where=W0 != 0)
        fx, fy = X0 * s, Y0 * s
    finite = np.isfinite(fx) & np.isfinite(fy) & bool(np.any(np.asarray(m) != 0))     # all-zero matrix: a rejected frame, zeros
    lo, hi = -2.0 ** 31, 2.0 ** 31 - 1
    X = np.rint(np.clip(np.where(finite, fx, 0.0), lo, hi)).astype(np.int64)
    Y = np.rint(np.clip(np.where(finite, fy, 0.0), lo, hi)).astype(np.int64)
    ix, ax, iy, ay = X >> 5, X & 31, Y >> 5, Y & 31
    src = frame.astype(np.int64)
    acc = np.zeros((oh, ow, 3), np.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            yy, xx = iy + dy, ix + dx
            w = (ax if dx else 32 - ax) * (ay if dy else 32 - ay) * 32
            ok = finite & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
            if mask is not None:
                ok = ok & (mask[yc, xc] != 0)
            acc += np.where(ok, w, 0)[..., None] * src[yc, xc]
    return ((acc + 16384) >> 15).astype(np.uint8)


def align_torch(x, pts, base_pts, dsize, estimate='reference', min_distance=5.0, mask=None):
    """`DeviceAlign(...)(x, pts, mask)` on the host: x is the ragged dict on the CPU (or a list of uint8 [H, W, 3] frames), mask a
    list of uint8 [H, W] planes -> (uint8 [N, h, w, 3] CPU tensor, valid bool [N]).  Same bits as the device."""
    oh, ow = _dsize(dsize)
    frames = unpack_frames(x) if is_ragged(x) else list(x)
    minv, valid = solve(pts, base_pts, estimate, min_distance)
    if minv.shape[0] != len(frames):
        raise PfrError(f"align: {minv.shape[0]} landmark sets for {len(frames)} frames")
    out = np.zeros((len(frames), oh, ow, 3), np.uint8)
    for n, f in enumerate(frames):
        if oh and ow:
            out[n] = _warp_numpy(np.asarray(f), minv[n], oh, ow, None if mask is None else np.asarray(mask[n]))
    return torch.from_numpy(out), valid
