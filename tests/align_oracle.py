"""Numpy restatement of the alignment contract of include/pfr_hip.h (pfr_align_solve / pfr_align_warp): a helper, not a test module.

`warp` is the contract operation by operation: fp64 coordinates with every product and sum rounded on its own (numpy's elementwise
ufuncs never fuse), 1/32-pixel quantisation with np.rint (ties to even), int64 tap arithmetic.  `solve` is an independent solver
(np.linalg.solve / np.linalg.inv) for the comparison with pfr_align_solve.  Frames are uint8 [H, W, 3], matrices fp64 [9] (the INVERSE
map: output pixel -> source pixel)."""
import numpy as np


def coords(minv, oh, ow):
    """-> (X, Y int64 [oh, ow] in 1/32 pixel, finite bool [oh, ow])"""
    m = np.asarray(minv, np.float64).reshape(9)
    x = np.arange(ow, dtype=np.float64)[None, :]
    y = np.arange(oh, dtype=np.float64)[:, None]
    with np.errstate(all='ignore'):
        X0 = (m[0] * x + m[1] * y) + m[2]
        Y0 = (m[3] * x + m[4] * y) + m[5]
        W0 = (m[6] * x + m[7] * y) + m[8]
        X0, Y0, W0 = np.broadcast_arrays(X0, Y0, W0)
        s = np.zeros(W0.shape, np.float64)
        nz = W0 != 0
        s[nz] = 32.0 / W0[nz]
        fx, fy = X0 * s, Y0 * s
    finite = np.isfinite(fx) & np.isfinite(fy) & bool(np.any(m != 0))        # the all-zero matrix marks a rejected frame: zeros
    q = lambda f: np.rint(np.clip(np.where(finite, f, 0.0), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64)
    return q(fx), q(fy), finite


def warp(frame, minv, oh, ow, mask=None):
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    H, W = frame.shape[:2]
    out = np.zeros((oh, ow, 3), np.uint8)
    if oh == 0 or ow == 0:
        return out
    X, Y, finite = coords(minv, oh, ow)
    ix, ax, iy, ay = X >> 5, X & 31, Y >> 5, Y & 31
    acc = np.zeros((oh, ow, 3), np.int64)
    src = frame.astype(np.int64)
    for dy, dx, w in ((0, 0, (32 - ax) * (32 - ay) * 32), (0, 1, ax * (32 - ay) * 32), (1, 0, (32 - ax) * ay * 32), (1, 1, ax * ay * 32)):
        yy, xx = iy + dy, ix + dx
        ok = finite & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        yc, xc = np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)
        if mask is not None:
            ok &= np.asarray(mask)[yc, xc] != 0
        acc += (w * ok)[..., None] * src[yc, xc]
    return ((acc + 16384) >> 15).astype(np.uint8)


def taps_inside(minv, oh, ow, H, W):
    """bool [oh, ow]: all four taps of the pixel lie inside the frame"""
    X, Y, finite = coords(minv, oh, ow)
    ix, iy = X >> 5, Y >> 5
    return finite & (ix >= 0) & (ix + 1 < W) & (iy >= 0) & (iy + 1 < H)


def four_points(pts, base):
    """the reference's 3-point rule (align.py:8-9): the rounded centroid is prepended to both sets"""
    pts, base = np.asarray(pts, np.float64), np.asarray(base, np.float64)
    if len(pts) == 3:
        pts = np.concatenate([np.round(np.mean(pts, axis=0))[None], pts])
        base = np.concatenate([np.round(np.mean(base, axis=0))[None], base])
    return pts, base


def solve(pts, base, mode='reference', min_distance=5.0):
    """pts [npts, 2], base [npts, 2] -> (minv fp64 [9], valid) with numpy's own linear algebra"""
    pts, base = np.asarray(pts, np.float64), np.asarray(base, np.float64)
    zero = np.zeros(9)
    if not (np.isfinite(pts).all() and np.isfinite(base).all()):
        return zero, False
    for i in range(len(pts)):
        for j in range(i + 1, len(pts)):
            if not np.sqrt(((pts[i] - pts[j]) ** 2).sum()) > min_distance:
                return zero, False
    if mode == 'reference':
        p4, b4 = four_points(pts, base)
        A, b = [], []
        for (x, y), (u, v) in zip(p4, b4):
            A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
            b += [u, v]
        A = np.asarray(A, np.float64)
        if np.linalg.matrix_rank(A, tol=1e-10 * np.abs(A).max()) < 8:
            return zero, False
        Hm = np.append(np.linalg.solve(A, np.asarray(b, np.float64)), 1.0).reshape(3, 3)
    else:
        ca, cb = pts - pts.mean(0), base - base.mean(0)
        za, zb = ca[:, 0] + 1j * ca[:, 1], cb[:, 0] + 1j * cb[:, 1]
        saa = (np.abs(za) ** 2).sum()
        if not saa > 0:
            return zero, False
        r = (np.conj(za) * zb).sum() / saa                     # scale * e^{i angle}: least squares over the complex plane
        t = (base.mean(0)[0] + 1j * base.mean(0)[1]) - r * (pts.mean(0)[0] + 1j * pts.mean(0)[1])
        Hm = np.array([[r.real, -r.imag, t.real], [r.imag, r.real, t.imag], [0, 0, 1]])
    minv = np.linalg.inv(Hm).reshape(9)
    return (minv, True) if np.isfinite(minv).all() else (zero, False)


def smooth_frame(seed, H, W, period=24.0):
    """uint8 [H, W, 3]: a smooth seeded pattern (adjacent pixels differ by a few levels)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = rs.uniform(0, 6.28, (3, 2))
    img = np.stack([127.5 + 60 * np.sin(xx / period + ph[c, 0]) + 60 * np.cos(yy / (period * 1.3) + ph[c, 1]) for c in range(3)], -1)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def max_adjacent_step(frame):
    f = frame.astype(np.int64)
    return int(max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max()))


def pillow_coeffs(minv):
    """the matrix in Pillow's pixel-centre convention, T(+1/2) . minv . T(-1/2), normalised -> the 8 PERSPECTIVE coefficients"""
    M = np.asarray(minv, np.float64).reshape(3, 3)
    Tp = np.array([[1, 0, 0.5], [0, 1, 0.5], [0, 0, 1.0]])
    Tm = np.array([[1, 0, -0.5], [0, 1, -0.5], [0, 0, 1.0]])
    P = Tp @ M @ Tm
    P = P / P[2, 2]
    return P.reshape(9)[:8].tolist()


# ---- the cases of the comparison with Pillow (tests/test_align_host.py, tools/make_align_golden.py) ---------------------------------
PILLOW_SEEDS = (11, 12, 13, 14, 15, 16)


def pillow_case(seed, small=False):
    """-> (frame uint8 [H, W, 3], pts [3, 2], base [3, 2], (oh, ow)).  Full size: sides 120..500, a 112 x 112 crop; small (the committed
    golden): sides 40..64, a 32 x 32 crop.  The three landmarks are random: the base triangle under a random rotation (+-25 degrees),
    scale (the crop covers 45..70 % of the shorter side) and shift, each landmark then moved by up to 3 % of the shorter side."""
    rs = np.random.RandomState(1000 + seed)
    lo, hi, o = (40, 64, 32) if small else (120, 500, 112)
    H, W = int(rs.randint(lo, hi + 1)), int(rs.randint(lo, hi + 1))
    base = np.array([[0.3125, 0.36], [0.6875, 0.36], [0.5, 0.72]]) * o
    th, k = np.deg2rad(rs.uniform(-25, 25)), rs.uniform(0.45, 0.70) * min(H, W) / o
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    centre = np.array([W, H]) * (0.5 + rs.uniform(-0.05, 0.05, 2))
    pts = (base - o / 2) @ R.T * k + centre + rs.uniform(-0.03, 0.03, (3, 2)) * min(H, W)
    return smooth_frame(seed, H, W, period=8.0 if small else 24.0), pts, base, (o, o)


def pillow_bound(frame):
    """|restatement - Pillow| <= floor(2 g / 64 + 1), g the frame's largest difference between adjacent pixels: the two differ by at most
    1/64 px per axis of coordinate quantisation, and by rounding where Pillow truncates"""
    return int(np.floor(2.0 * max_adjacent_step(frame) / 64.0 + 1.0))
