"""Host side of the landmark alignment (no GPU): the C-ABI declarations, pfr_align_solve against an independent numpy solver and on its
edge cases, the numpy restatement of the warp contract (tests/align_oracle.py) against Pillow's Image.transform(PERSPECTIVE, BILINEAR)
(committed outputs in tests/golden/align.npz, and live where Pillow imports), align_torch against the restatement bit for bit, the
argument checks of DeviceAlign and the landmarks of the synthetic dataset.

The bound of the comparison with Pillow is derived, not measured: |delta| <= floor(2 g / 64 + 1) with g the frame's largest difference
between adjacent pixels (1/64 px of coordinate quantisation per axis, and rounding where Pillow truncates).  Measured on the twelve cases
of this file: max |delta| = 1 against a bound of 1, shares of compared pixels 0.95 .. 1.00."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_oracle as AO

from pets_face_recognition_amd._hip import PfrError
from pets_face_recognition_amd._hip.lib import lib
from pets_face_recognition_amd.data_loading import align as A
from pets_face_recognition_amd.data_loading import DeviceAlign, pack_frames, SyntheticRecDataset, ragged_collate

BASE3 = np.array([[35.0, 40.0], [77.0, 40.0], [56.0, 81.0]])
BASE4 = np.array([[30.0, 30.0], [82.0, 30.0], [82.0, 82.0], [30.0, 82.0]])


# ---- declarations --------------------------------------------------------------------------------------------------------------
def test_symbols_and_signatures():
    syms = lib.symbols()
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    want = {
        'pfr_align_solve': ([I, P, P, I, I, D, P, P], ['mode', 'pts', 'base', 'N', 'npts', 'min_distance', 'minv', 'valid']),
        'pfr_align_warp': ([P, P, P, P, P, P, I, I, I, P, P],
                           ['data', 'offsets', 'shapes', 'minv', 'mask', 'mask_offsets', 'N', 'out_h', 'out_w', 'out_u8', 'stream']),
    }
    for name, (argtypes, argnames) in want.items():
        assert name in syms, f"{name} is not declared in include/pfr_hip.h"
        restype, got_types, got_names = syms[name]
        assert restype is ctypes.c_int and got_types == argtypes and got_names == argnames
        assert hasattr(lib._dll, name)
    inc = open(os.path.join(ROOT, 'pets-face-recognition_amd', 'csrc', 'pfr_thunks_gen.inc')).read()
    assert 'th_pfr_align_warp' in inc and 'th_pfr_align_solve' not in inc      # the solve takes no stream: no thunk


# ---- the solve -----------------------------------------------------------------------------------------------------------------
def _random_pts(rs, base, n):
    """n landmark sets: the base set under a random rotation / scale / shift, every landmark then moved by up to 6 px"""
    out = []
    for _ in range(n):
        th, k = rs.uniform(-np.pi, np.pi), rs.uniform(0.5, 4.0)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        out.append((base - base.mean(0)) @ R.T * k + rs.uniform(50, 900, 2) + rs.uniform(-6, 6, base.shape))
    return np.stack(out)


def _apply(M, p):
    q = np.asarray(M).reshape(3, 3) @ np.array([p[0], p[1], 1.0])
    return q[:2] / q[2]


@pytest.mark.parametrize('base', [BASE3, BASE4], ids=['3pts', '4pts'])
def test_solve_reference_against_numpy(base):
    pts = _random_pts(np.random.RandomState(5), base, 40)
    minv, valid = A.solve(pts, base)
    assert valid.all() and minv.dtype == np.float64 and minv.shape == (40, 9)
    for n in range(len(pts)):
        ref, ok = AO.solve(pts[n], base)
        assert ok
        assert np.abs(minv[n] - ref).max() <= 1e-9 * np.abs(ref).max()
        fwd = np.linalg.inv(minv[n].reshape(3, 3))
        p4, b4 = AO.four_points(pts[n], base)       # with three landmarks: the rounded centroid in front
        assert len(p4) == 4
        for p, b in zip(p4, b4):
            assert np.abs(_apply(fwd, p) - b).max() <= 1e-9


def test_solve_similarity_against_numpy():
    pts = _random_pts(np.random.RandomState(6), np.concatenate([BASE3, BASE4]), 20)
    base = np.concatenate([BASE3, BASE4])
    minv, valid = A.solve(pts, base, estimate='similarity')
    assert valid.all()
    for n in range(len(pts)):
        ref, ok = AO.solve(pts[n], base, mode='similarity')
        assert ok and np.abs(minv[n] - ref).max() <= 1e-9 * np.abs(ref).max()
        assert minv[n][6:].tolist() == [0.0, 0.0, 1.0]


def test_three_point_rule_rounds_half_to_even():
    # means that end in .5, exactly: x (0 + 10 + 21.5) / 3 = 10.5 -> 10 (down), y (0 + 20 + 14.5) / 3 = 11.5 -> 12 (up)
    pts = np.array([[0.0, 0.0], [10.0, 20.0], [21.5, 14.5]])
    # base: x (1 + 30 + 40.5) / 3 = 23.5 -> 24 (up), y (2 + 3 + 32.5) / 3 = 12.5 -> 12 (down)
    base = np.array([[1.0, 2.0], [30.0, 3.0], [40.5, 32.5]])
    p4, b4 = AO.four_points(pts, base)
    assert p4[0].tolist() == [10.0, 12.0] and b4[0].tolist() == [24.0, 12.0]
    minv, valid = A.solve(pts[None], base)
    assert valid[0]
    assert np.abs(_apply(minv[0], [24.0, 12.0]) - [10.0, 12.0]).max() <= 1e-9        # half-up would have paired (24, 13) with (11, 12)
    for p, b in zip(pts, base):
        assert np.abs(_apply(minv[0], b) - p).max() <= 1e-9
    ref, _ = AO.solve(pts, base)
    assert np.abs(minv[0] - ref).max() <= 1e-9 * np.abs(ref).max()


def test_similarity_recovers_a_known_map_and_never_reflects():
    th, s, t = 0.3, 1.7, np.array([12.5, -4.25])
    R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    pts = np.array([[10.0, 20.0], [60.0, 25.0], [33.0, 70.0], [80.0, 90.0], [5.0, 77.0]])
    base = pts @ R.T + t
    minv, valid = A.solve(pts[None], base, estimate='similarity')
    assert valid[0] and minv[0][6:].tolist() == [0.0, 0.0, 1.0]
    fwd = np.linalg.inv(minv[0].reshape(3, 3))
    assert np.abs(fwd[:2, :2] - R).max() <= 1e-12 and np.abs(fwd[:2, 2] - t).max() <= 1e-12
    # a mirrored target: the best ROTATION is returned, never the reflection that would fit exactly
    mirrored = pts * np.array([-1.0, 1.0]) + np.array([100.0, 0.0])
    minv, valid = A.solve(pts[None], mirrored, estimate='similarity')
    assert valid[0]
    fwd = np.linalg.inv(minv[0].reshape(3, 3))
    assert np.linalg.det(fwd[:2, :2]) > 0 and abs(fwd[0, 0] - fwd[1, 1]) <= 1e-12 and abs(fwd[0, 1] + fwd[1, 0]) <= 1e-12


@pytest.mark.parametrize('name,pts', [
    ('collinear', [[10.0, 10.0], [30.0, 30.0], [70.0, 70.0]]),
    ('coincident', [[10.0, 10.0], [10.0, 10.0], [70.0, 20.0]]),
    ('exactly_min_distance', [[10.0, 10.0], [13.0, 14.0], [70.0, 20.0]]),       # 3-4-5: the reference's test is strict
    ('nan', [[10.0, float('nan')], [40.0, 14.0], [70.0, 90.0]]),
])
def test_solve_rejects(name, pts):
    good = [[20.0, 25.0], [90.0, 30.0], [50.0, 99.0]]
    p = np.array([good, pts, good])
    minv = np.full((3, 9), 7.0)
    valid = np.full(3, 7, np.int32)
    base = np.ascontiguousarray(BASE3)
    rc = lib._dll.pfr_align_solve(0, p.ctypes.data, base.ctypes.data, 3, 3, ctypes.c_double(5.0), minv.ctypes.data, valid.ctypes.data)
    assert rc == 0                                              # an invalid frame is data, not an error
    assert valid.tolist() == [1, 0, 1] and not minv[1].any() and minv[0].any() and np.array_equal(minv[0], minv[2])
    if name == 'exactly_min_distance':
        _, v = A.solve(p, BASE3, min_distance=4.999)
        assert v.all()
    if name in ('coincident', 'exactly_min_distance', 'nan'):
        _, v = A.solve(p[:, :2], BASE3[:2], estimate='similarity')
        assert v.tolist() == [True, False, True]


def test_solve_empty_and_bad_arguments():
    minv, valid = A.solve(np.zeros((0, 3, 2)), BASE3)
    assert minv.shape == (0, 9) and valid.shape == (0,)
    with pytest.raises(PfrError):
        A.solve(np.zeros((1, 3, 2)), BASE3, estimate='affine')
    with pytest.raises(PfrError):
        A.solve(np.zeros((1, 4, 2)), BASE3)
    with pytest.raises(PfrError):
        A.solve(np.zeros((1, 5, 2)), np.zeros((5, 2)))          # the reference mode takes 3 or 4 landmarks


# ---- the restatement against Pillow ---------------------------------------------------------------------------------------------------
def _check_against_pillow(frame, minv, pillow, oh, ow):
    ours = AO.warp(frame, minv, oh, ow)
    inside = AO.taps_inside(minv, oh, ow, frame.shape[0], frame.shape[1])
    # Pillow clamps at the border where the contract blends with zero: border pixels are excluded, and enough must remain
    share = inside.mean()
    delta = int(np.abs(ours.astype(np.int64) - pillow.astype(np.int64))[inside].max())
    bound = AO.pillow_bound(frame)
    print(f"frame {frame.shape[:2]}: max |delta| {delta}, bound {bound}, share compared {share:.3f}")
    assert share >= 0.60
    assert delta <= bound


def test_restatement_against_pillow_golden():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'align.npz'))
    for k, seed in enumerate(AO.PILLOW_SEEDS):
        frame, pts, base, (oh, ow) = AO.pillow_case(seed, small=True)
        assert np.array_equal(frame, g[f'frame{k}']) and np.array_equal(pts, g[f'pts{k}']) and max(frame.shape) <= 64
        assert g[f'pillow{k}'].shape == (32, 32, 3)
        _check_against_pillow(frame, g[f'minv{k}'], g[f'pillow{k}'], oh, ow)
        minv, valid = A.solve(pts[None], base)                  # the library's own matrix gives the same picture
        assert valid[0] and np.array_equal(AO.warp(frame, minv[0], oh, ow), AO.warp(frame, g[f'minv{k}'], oh, ow))


def test_restatement_against_pillow_live():
    Image = pytest.importorskip('PIL.Image')
    for seed in AO.PILLOW_SEEDS:
        frame, pts, base, (oh, ow) = AO.pillow_case(seed)
        assert 120 <= min(frame.shape[:2]) and max(frame.shape[:2]) <= 500
        minv, valid = A.solve(pts[None], base)
        assert valid[0]
        pil = np.asarray(Image.fromarray(frame).transform((ow, oh), Image.PERSPECTIVE, AO.pillow_coeffs(minv[0]), Image.BILINEAR))
        _check_against_pillow(frame, minv[0], pil, oh, ow)


# ---- align_torch ---------------------------------------------------------------------------------------------------------------------
def test_align_torch_equals_the_oracle():
    rs = np.random.RandomState(3)
    frames = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (64, 48), (90, 41))]
    masks = [(rs.rand(*f.shape[:2]) > 0.3).astype(np.uint8) * rs.randint(1, 256, f.shape[:2]).astype(np.uint8) for f in frames]
    base = BASE3 * (40 / 112)
    pts = np.stack([base * 0.8 + rs.uniform(2, 6, 2) + rs.uniform(-1.5, 1.5, (3, 2)) for _ in frames])
    pts[2] = [[5.0, 5.0], [6.0, 6.0], [30.0, 30.0]]                 # rejected: comes back zero
    out, valid = A.align_torch(pack_frames(frames), pts, base, (40, 44, 3), min_distance=5.0)
    outm, _ = A.align_torch(frames, pts, base, (40, 44), mask=masks)
    assert valid.tolist() == [True, True, False] and out.dtype == torch.uint8 and tuple(out.shape) == (3, 40, 44, 3)
    for n, f in enumerate(frames):
        minv, ok = AO.solve(pts[n], base)
        lib_minv, _ = A.solve(pts[n:n + 1], base)
        assert np.array_equal(out[n].numpy(), AO.warp(f, lib_minv[0], 40, 44))
        assert np.array_equal(outm[n].numpy(), AO.warp(f, lib_minv[0], 40, 44, masks[n]))
        assert ok == bool(valid[n])
    assert out[:2].any() and not out[2].any()
    # defined inputs of the contract: NaN, saturation, W0 == 0 on a column and the all-zero matrix
    f = frames[0]
    for m in ([1, 0, 0, 0, 1, 0, 1, 0, -5], [float('nan')] + [1.0] * 8, [1e300, 0, 1e300, 0, 1e300, 1e300, 0, 0, 1], [0.0] * 9,
              [1, 0, -3.4, 0, 1, -3.4, 0, 0, 1]):
        assert np.array_equal(A._warp_numpy(f, np.array(m, np.float64), 9, 11), AO.warp(f, m, 9, 11))


# ---- DeviceAlign ---------------------------------------------------------------------------------------------------------------------
def test_device_align_argument_checks():
    assert DeviceAlign(BASE3, (224, 224, 3)).dsize == (224, 224) and DeviceAlign(BASE3, (100, 120)).dsize == (100, 120)
    assert DeviceAlign(BASE3, [64, 32, 3]).dsize == (64, 32)
    for bad in ((224,), (224, 224, 4), (224, 224, 3, 1), (5000, 10), (-1, 10)):
        with pytest.raises(PfrError):
            DeviceAlign(BASE3, bad)
    with pytest.raises(PfrError):
        DeviceAlign(BASE3, (224, 224), estimate='affine')
    with pytest.raises(PfrError):
        DeviceAlign(np.zeros((5, 2)), (224, 224))                # reference: 3 or 4 landmarks
    with pytest.raises(PfrError):
        DeviceAlign(np.zeros((3, 3)), (224, 224))
    assert DeviceAlign(np.zeros((5, 2)) + BASE3[0], (224, 224), estimate='similarity').base_pts.shape == (5, 2)
    with pytest.raises(ValueError):
        DeviceAlign(BASE3, (224, 224), jitter=-1.0)
    al = DeviceAlign(BASE3, (224, 224))
    for bad in (np.zeros((2, 4, 2)), np.zeros((3, 2)), np.zeros((2, 3, 3))):
        with pytest.raises(PfrError):
            al.landmarks(bad)
    # jitter: seeded, and it moves the landmarks
    pts = np.zeros((4, 3, 2)) + BASE3
    a = DeviceAlign(BASE3, (224, 224), jitter=2.0, generator=torch.Generator().manual_seed(1)).landmarks(pts)
    b = DeviceAlign(BASE3, (224, 224), jitter=2.0, generator=torch.Generator().manual_seed(1)).landmarks(pts)
    assert np.array_equal(a, b) and np.abs(a - pts).max() > 0.1 and np.array_equal(al.landmarks(pts), pts)
    with pytest.raises(ValueError):
        A.pack_masks([torch.zeros(3, 4)])
    pk = A.pack_masks([torch.ones(3, 5, dtype=torch.uint8), torch.ones(4, 4, dtype=torch.uint8)])
    assert pk['offsets'].tolist() == [0, 16] and pk['data'].numel() == 32 and pk['data'].sum() == 31


def test_synthetic_landmarks():
    ds = SyntheticRecDataset(3, 4, 224, seed=2, raw_uint8=True, ragged=True, landmarks=True, masks=True)
    plain = SyntheticRecDataset(3, 4, 224, seed=2, raw_uint8=True, ragged=True)
    for i in range(len(ds)):
        it = ds[i]
        H, W = it['x'].shape[:2]
        p = it['pts'].numpy()
        assert torch.equal(it['x'], plain[i]['x']) and 'pts' not in plain[i]
        assert p.shape == (3, 2) and p.dtype == np.float64 and torch.equal(it['pts'], ds[i]['pts'])
        assert (p[:, 0] >= 0.1 * W).all() and (p[:, 0] <= 0.9 * W).all() and (p[:, 1] >= 0.1 * H).all() and (p[:, 1] <= 0.9 * H).all()
        assert min(np.hypot(*(p[a] - p[b])) for a, b in ((0, 1), (0, 2), (1, 2))) > 5.0
        assert it['mask'].dtype == torch.uint8 and tuple(it['mask'].shape) == (H, W) and 0 < int(it['mask'].sum()) < H * W
    batch = ragged_collate([ds[0], ds[5], ds[7]])
    assert tuple(batch['pts'].shape) == (3, 3, 2) and batch['mask']['offsets'].shape == (3,) and 'data' in batch['x']
    _, valid = A.solve(batch['pts'], ds.base_pts((224, 224)))
    assert valid.all()
    with pytest.raises(ValueError):
        SyntheticRecDataset(3, 4, 224, raw_uint8=True, landmarks=True)


def test_align_config_loads_and_exposes_the_entries(tmp_path, monkeypatch):
    import pets_face_recognition_amd as pfr
    from pets_face_recognition_amd.utils import get_dict_wrapper
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    cfg = get_dict_wrapper(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_align.py"))
    al, tr = cfg['device_align'], cfg['device_train_align']
    assert al.dsize == (224, 224) and al.jitter == 0.0 and tr.jitter == 1.0 and tr.generator is not None
    assert cfg['device_train_augmentation'].fit is None and cfg['device_val_augmentation'].fit is None       # the head pipeline
    batch = next(iter(cfg['val_dataloader']()))
    n = batch['x']['shape'].shape[0]
    assert tuple(batch['pts'].shape) == (n, 3, 2) and batch['pts_host'].shape == (n, 3, 2) and 'mask' not in batch
    out, valid = A.align_torch(batch['x'], batch['pts_host'], al.base_pts, al.dsize)
    assert valid.all() and tuple(out.shape) == (n, 224, 224, 3) and all(o.any() for o in out)
