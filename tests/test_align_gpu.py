"""Landmark alignment on the device: pfr_align_warp, data_loading.align.DeviceAlign and the Controller wiring.

Every comparison is torch.equal against the numpy restatement of the contract (tests/align_oracle.py): no tolerance anywhere in this
file.  The inputs with NaN, saturating entries, W0 == 0 and the all-zero matrix are DEFINED inputs of the contract: every tap is
range-checked before an address is formed from it.  The device frames are cached per case and released when this module is done."""
import ctypes
import functools
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_oracle as AO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PFR_ERR_ARG = -1
IDENT = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]


def _A():
    from pets_face_recognition_amd.data_loading import align
    return align


def _frames(seed, sizes):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]


@functools.lru_cache(maxsize=None)
def _packed(seed, sizes):
    """(frames, the ragged dict on the device) - computed once per case, never modified"""
    from pets_face_recognition_amd.data_loading import pack_frames
    frames = _frames(seed, sizes)
    x = pack_frames(frames)
    return frames, {'data': x['data'].to(DEV), 'shape': x['shape'].to(DEV), 'shape_host': x['shape_host']}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _packed.cache_clear()
    torch.cuda.empty_cache()


def _translate(tx, ty):
    return [1.0, 0, tx, 0, 1.0, ty, 0, 0, 1.0]


def _check(frames, x, minv, oh, ow, masks=None):
    A = _A()
    minv = np.asarray(minv, np.float64).reshape(len(frames), 9)
    got = A.warp(x, minv, (oh, ow), None if masks is None else A.pack_masks(masks))
    want = np.stack([AO.warp(f, m, oh, ow, None if masks is None else masks[n]) for n, (f, m) in enumerate(zip(frames, minv))]) \
        if frames else np.zeros((0, oh, ow, 3), np.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(frames), oh, ow, 3) and got.is_cuda
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return want


SIZES = ((1, 1), (2, 3), (7, 5), (64, 48))


@pytest.mark.parametrize("oh,ow", [(1, 1), (5, 7), (33, 65)])
def test_identity_map_is_the_top_left_crop(oh, ow):
    frames, x = _packed(1, SIZES)          # mixed sizes, odd row pitches, every frame on a 16-byte boundary
    want = _check(frames, x, [IDENT] * 4, oh, ow)
    for n, f in enumerate(frames):
        h, w = min(oh, f.shape[0]), min(ow, f.shape[1])
        crop = np.zeros((oh, ow, 3), np.uint8)
        crop[:h, :w] = f[:h, :w]
        assert np.array_equal(want[n], crop)


def test_random_homographies_from_the_solve():
    A = _A()
    sizes = ((150, 211), (97, 64), (301, 180))
    frames, x = _packed(2, sizes)
    base = np.array([[70.0, 80.0], [154.0, 80.0], [112.0, 162.0]])
    rs = np.random.RandomState(4)
    pts = np.stack([(base - 112) * rs.uniform(0.2, 0.5) + [w / 2, h / 2] + rs.uniform(-4, 4, (3, 2)) for h, w in sizes])
    minv, valid = A.solve(pts, base)
    assert valid.all()
    want = _check(frames, x, minv, 224, 224)
    assert all(w.any() for w in want)
    one_f, one_x = _packed(2, sizes[:1])
    assert np.array_equal(_check(one_f, one_x, minv[:1], 224, 224)[0], want[0])
    # N == 0 and an empty output: no launch, an empty result
    empty = {'data': torch.zeros(0, dtype=torch.uint8, device=DEV), 'shape': torch.zeros((0, 2), dtype=torch.int32, device=DEV),
             'shape_host': np.zeros((0, 2), np.int32)}
    assert tuple(A.warp(empty, np.zeros((0, 9)), (224, 224)).shape) == (0, 224, 224, 3)
    assert tuple(A.warp(one_x, minv[:1], (0, 8)).shape) == (1, 0, 8, 3)


def test_each_edge_is_blended_with_zero():
    sizes = ((9, 13), (16, 16))
    frames, x = _packed(3, sizes)
    seen = set()
    for tx, ty in ((-1.5, 0.25), (0.5, -1.5), (0.5, 0.5), (-0.5, -0.5)):
        m = _translate(tx, ty)
        _check(frames, x, [m, m], 19, 19)
        for f in frames:
            H, W = f.shape[:2]
            X, Y, _ = AO.coords(m, 19, 19)
            ix, iy, inrow, incol = X >> 5, Y >> 5, ((Y >> 5) >= 0) & ((Y >> 5) < H - 1), ((X >> 5) >= 0) & ((X >> 5) < W - 1)
            seen |= {k for k, hit in (('ix=-1', (ix == -1) & inrow), ('ix=W-1', (ix == W - 1) & inrow), ('iy=-1', (iy == -1) & incol),
                                      ('iy=H-1', (iy == H - 1) & incol)) if hit.any()}
    assert seen == {'ix=-1', 'ix=W-1', 'iy=-1', 'iy=H-1'}
    for m in (_translate(10000.0, 0.0), _translate(0.0, -500.0), _translate(-20.0, -20.0)):      # the map leaves the frame entirely
        assert not _check(frames, x, [m, m], 19, 19).any()


def test_negative_coordinates_shift_and_mask_arithmetically():
    frames, x = _packed(3, ((9, 13), (16, 16)))
    m = _translate(-3.4, -3.4)
    X, _, _ = AO.coords(m, 12, 12)
    assert X[0, 0] == -109 and (X[0, 0] >> 5, X[0, 0] & 31) == (-4, 19)        # -108.8 -> -109 = -4 * 32 + 19
    want = _check(frames, x, [m, m], 12, 12)
    assert want.any()


def test_ties_round_half_to_even():
    frames, x = _packed(3, ((9, 13), (16, 16)))
    m = _translate(1.0 / 64.0, 1.0 / 64.0)          # fx = 32 x + 0.5 exactly, for every pixel
    X, _, _ = AO.coords(m, 8, 8)
    assert X[0].tolist() == [32 * k for k in range(8)]      # 32 k + 0.5 -> the even 32 k
    _check(frames, x, [m, m], 8, 8)
    m = _translate(3.0 / 64.0, 3.0 / 64.0)          # fx = 32 x + 1.5 -> 32 x + 2
    assert AO.coords(m, 8, 8)[0][0].tolist() == [32 * k + 2 for k in range(8)]
    _check(frames, x, [m, m], 8, 8)


def _fusions(ma, a, mb, b, mc):
    """(ma * a + mb * b) + mc as the contract evaluates it, and as a compiler that contracts evaluates it in either order:
    fma(ma, a, mb * b) + mc and fma(mb, b, ma * a) + mc.  Exact rational arithmetic, float() = one IEEE rounding."""
    F = Fraction
    pa, pb = float(F(ma) * a), float(F(mb) * b)                      # each product rounded on its own
    unfused = float(F(float(F(pa) + F(pb))) + F(mc))
    fma_a = float(F(float(F(ma) * a + F(pb))) + F(mc))               # the exact product ma * a enters the sum
    fma_b = float(F(float(F(mb) * b + F(pa))) + F(mc))
    return unfused, fma_a, fma_b


def test_unfused_coordinate_arithmetic_at_constructed_pixels():
    """Four matrices, each with one output pixel at which a contracted multiply-add lands in another 1/32 bin than the contract.
    A = double(1000 / 3) and B = -996.828125.  A * 3 is not representable: it rounds UP to 1000 exactly, the exact product is
    1000 - 2^-44.  B * 1 is exact.  Unfused, (A * 3 + B * 1) + 0 = 3.171875 = 101.5 / 32: fx = 101.5, a tie that rounds to the even 102
    (tap 3, weight 6).  fma(A, 3, B * 1) keeps the exact product: 3.171875 - 2^-44, fx < 101.5, rounds to 101 (weight 5).  The other
    fusion order, fma(B, 1, A * 3), rounds A * 3 first and equals the unfused value, so each axis is tested in both operand positions:
        0: X0 = (A x + B y) + 0 at (x, y) = (3, 1)      1: X0 = (B x + A y) + 0 at (1, 3)
        2: Y0 = (A x + B y) + 0 at (3, 1)               3: Y0 = (B x + A y) + 0 at (1, 3)
    The other axis of each matrix is the identity.  Frames 0 / 1 are 0 up to column 3 and 255 from column 4, frames 2 / 3 the same
    over rows: the pixel is (6 * 1024 * 255 + 16384) >> 15 = 48 by the contract, (5 * 1024 * 255 + 16384) >> 15 = 40 contracted."""
    A, B = 1000.0 / 3.0, -996.828125
    assert Fraction(A) * 3 == 1000 - Fraction(1, 2 ** 44)
    unfused, fma_a, fma_b = _fusions(A, 3, B, 1, 0.0)
    assert unfused * 32.0 == 101.5 and fma_b == unfused and fma_a == 3.171875 - 2.0 ** -44 and round(fma_a * 32.0) == 101
    unfused, fma_a, fma_b = _fusions(B, 1, A, 3, 0.0)                # the inexact product in the second position
    assert unfused * 32.0 == 101.5 and fma_a == unfused and round(fma_b * 32.0) == 101
    assert (6 * 1024 * 255 + 16384) >> 15 == 48 and (5 * 1024 * 255 + 16384) >> 15 == 40
    cols = np.zeros((6, 8, 3), np.uint8)
    cols[:, 4:] = 255
    rows = np.zeros((8, 6, 3), np.uint8)
    rows[4:] = 255
    frames = [cols, cols, rows, rows]
    ms = [[A, B, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0], [B, A, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0],
          [1.0, 0.0, 0.0, A, B, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, B, A, 0.0, 0.0, 0.0, 1.0]]
    at = [(1, 3), (3, 1), (1, 3), (3, 1)]                            # (row, column) of the constructed pixel
    for m, (r, c), xy in zip(ms, at, ((102, 32), (102, 96), (96, 102), (32, 102))):          # the tie went to the even 102
        X, Y, _ = AO.coords(m, 4, 4)
        assert (X[r, c], Y[r, c]) == xy
    from pets_face_recognition_amd.data_loading import pack_frames
    x = pack_frames(frames)
    x = {'data': x['data'].to(DEV), 'shape': x['shape'].to(DEV), 'shape_host': x['shape_host']}
    got = _A().warp(x, np.array(ms), (4, 4)).cpu().numpy()
    print("constructed pixels (contract 48, contracted 40):", [got[n][r, c].tolist() for n, (r, c) in enumerate(at)])
    want = _check(frames, x, ms, 4, 4)
    for n, (r, c) in enumerate(at):
        assert want[n][r, c].tolist() == [48, 48, 48]


def test_w0_zero_on_one_column():
    frames, x = _packed(3, ((9, 13), (16, 16)))
    m = [1.0, 0, 0, 0, 1.0, 0, 1.0, 0, -5.0]        # W0 = x - 5: zero on column 5, negative on its near side, positive beyond
    want = _check(frames, x, [m, m], 10, 12)
    for n, f in enumerate(frames):
        assert (want[n][:, 5] == f[0, 0]).all()          # s = 0: fx = fy = 0, source pixel (0, 0)
    assert want[:, :, :5].any() or want[:, :, 6:].any()


def test_saturation_and_non_finite_matrices_give_zeros():
    frames, x = _packed(3, ((9, 13), (16, 16)))
    nan = float('nan')
    for m in ([1e300, 0, 1e300, 0, 1e300, 1e300, 0, 0, 1.0], [-1e300, 0, -1e300, 0, 1.0, 0, 0, 0, 1.0], [nan] * 9,
              [1.0, 0, 0, 0, 1.0, 0, 0, 0, nan], [float('inf'), 0, 0, 0, 1.0, 0, 0, 0, 1.0], [0.0] * 9):
        assert not _check(frames, x, [m, IDENT], 9, 9)[0].any()
    # the clamp itself: 32 * 1e300 saturates at 2^31 - 1, far outside every frame
    X, _, finite = AO.coords([1e300, 0, 1e300, 0, 1.0, 0, 0, 0, 1.0], 2, 2)
    assert finite.all() and X.max() == 2 ** 31 - 1


def test_mask_drops_pixels():
    A = _A()
    sizes = ((9, 13), (16, 16), (40, 33))
    frames, x = _packed(5, sizes)
    rs = np.random.RandomState(9)
    masks = [((rs.rand(h, w) > 0.4) * rs.randint(1, 256, (h, w))).astype(np.uint8) for h, w in sizes]      # non-{0, 1} bytes count as 1
    ms = [_translate(-0.7, 0.3), [0.9, 0.1, 0.5, -0.1, 0.9, 1.0, 0.001, 0, 1.0], [1.3, 0, 2.25, 0, 1.3, 1.75, 0, 0.002, 1.0]]
    want = _check(frames, x, ms, 30, 28, masks)
    pre = [f * (k != 0)[..., None].astype(np.uint8) for f, k in zip(frames, masks)]
    assert np.array_equal(want, np.stack([AO.warp(f, m, 30, 28) for f, m in zip(pre, ms)]))      # = the frame multiplied by the 0/1 mask
    # planes in another frame order: the same total, other offsets - refused, on the host copy of the offsets and on a CPU tensor alike
    from pets_face_recognition_amd._hip import PfrError
    swapped = A.pack_masks([masks[1], masks[0], masks[2]])
    assert swapped['data'].numel() == A.pack_masks(masks)['data'].numel()
    for bad in (swapped, {'data': swapped['data'], 'offsets': swapped['offsets']}):
        with pytest.raises(PfrError):
            A.warp(x, np.array(ms), (30, 28), bad)
    ones = [np.ones((h, w), np.uint8) for h, w in sizes]
    assert torch.equal(A.warp(x, np.array(ms), (30, 28), A.pack_masks(ones)), A.warp(x, np.array(ms), (30, 28)))


def test_argument_errors():
    from pets_face_recognition_amd._hip.lib import lib
    lib._load()
    f = lib._dll.pfr_align_warp
    buf = torch.zeros(64, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert f(p, p, p, p, None, None, 1, 4097, 8, p, None) == PFR_ERR_ARG
    assert f(p, p, p, p, None, None, 1, 8, 4097, p, None) == PFR_ERR_ARG
    assert f(None, p, p, p, None, None, 1, 8, 8, p, None) == PFR_ERR_ARG
    assert f(p, p, p, None, None, None, 1, 8, 8, p, None) == PFR_ERR_ARG
    assert f(p, p, p, p, p, None, 1, 8, 8, p, None) == PFR_ERR_ARG           # a mask without its offsets
    assert f(p, p, p, p, None, None, -1, 8, 8, p, None) == PFR_ERR_ARG
    assert f(None, None, None, None, None, None, 0, 8, 8, None, None) == 0 and f(p, p, p, p, None, None, 1, 0, 8, p, None) == 0
    torch.cuda.synchronize()
    assert not buf.any()


def test_device_align_end_to_end():
    from pets_face_recognition_amd.data_loading import DeviceAlign
    A = _A()
    sizes = ((150, 211), (97, 64), (301, 180))
    frames, x = _packed(2, sizes)
    base = np.array([[22.0, 25.0], [48.0, 25.0], [35.0, 50.0]])
    rs = np.random.RandomState(8)
    pts = np.stack([(base - 35) * rs.uniform(0.8, 1.5) + [w / 2, h / 2] + rs.uniform(-3, 3, (3, 2)) for h, w in sizes])
    pts[1] = [[10.0, 10.0], [12.0, 11.0], [50.0, 60.0]]          # two landmarks 2.2 px apart: rejected
    out, valid = DeviceAlign(base, (70, 72, 3))(x, torch.from_numpy(pts))
    minv, v2 = A.solve(pts, base)
    assert valid.tolist() == [True, False, True] == v2.tolist() and not minv[1].any()
    want = np.stack([AO.warp(f, m, 70, 72) for f, m in zip(frames, minv)])
    assert torch.equal(out.cpu(), torch.from_numpy(want)) and want[0].any() and want[2].any() and not want[1].any()
    sim, vs = DeviceAlign(base, (70, 72), estimate='similarity')(x, pts)
    ms, _ = A.solve(pts, base, estimate='similarity')
    assert torch.equal(sim.cpu(), torch.from_numpy(np.stack([AO.warp(f, m, 70, 72) for f, m in zip(frames, ms)]))) and vs.tolist() == valid.tolist()
    cpu, vc = A.align_torch(frames, pts, base, (70, 72))
    assert torch.equal(out.cpu(), cpu) and vc.tolist() == valid.tolist()
    # jitter: seeded, two calls agree, and the landmarks moved
    a = DeviceAlign(base, (70, 72), jitter=1.5, generator=torch.Generator().manual_seed(3))
    b = DeviceAlign(base, (70, 72), jitter=1.5, generator=torch.Generator().manual_seed(3))
    oa, ob = a(x, pts)[0], b(x, pts)[0]
    assert torch.equal(oa, ob) and np.array_equal(a.last_pts, b.last_pts) and np.abs(a.last_pts - pts).max() > 0.1
    assert not torch.equal(oa, out)


class _Cfg(dict):
    """the config surface the Controller uses: entries as items and as attributes"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


class _Probe(torch.nn.Module):
    """stands in for model + loss: records what a training step hands over, embeds a frame as its mean"""

    def __init__(self):
        super().__init__()
        self.seen = {}

    def forward(self, x, label=None):
        if label is None:
            return x.float().mean((1, 2, 3))
        self.seen = {'n': x.shape[0], 'labels': label.tolist()}
        return {'loss': x.float().sum()}


def _controller(**entries):
    from pets_face_recognition_amd.engine.controller import Controller
    return Controller(_Cfg(model=lambda: torch.nn.Identity(), loss=lambda cfg, m: _Probe(), **entries))


def test_controller_aligns_ragged_batches_with_landmarks():
    from torch.utils.data import DataLoader
    from pets_face_recognition_amd.data_loading import DeviceAlign, SyntheticRecDataset, ragged_collate, val_augmentation
    from pets_face_recognition_amd.data_loading import simple_val_augmentation, unpack_frames
    from pets_face_recognition_amd.engine.trainer import _to_device
    ds = SyntheticRecDataset(3, 4, 64, seed=5, raw_uint8=True, ragged=True, landmarks=True, masks=True)
    ds.item_size = lambda i: (80 + 7 * i, 120 - 5 * i)                     # small frames: the test is about the wiring
    base = ds.base_pts((64, 64))
    ctl = _controller(device_align=DeviceAlign(base, (64, 64, 3)), device_val_augmentation=val_augmentation(),
                      device_train_augmentation=val_augmentation())
    plain = _controller(device_val_augmentation=simple_val_augmentation())
    nb = 0
    for batch in DataLoader(ds, 4, collate_fn=ragged_collate):
        nb += 1
        host_pts = batch['pts_host'].copy()
        batch = _to_device(batch, DEV)
        got = ctl._images(batch, False)
        aligned, valid = DeviceAlign(base, (64, 64, 3))(batch['x'], host_pts, batch['mask'])
        assert valid.all() and ctl.last_align_valid.tolist() == valid.tolist()
        assert tuple(got.shape) == (4, 3, 64, 64) and torch.equal(got, val_augmentation()(aligned))
        frames = [f.cpu().numpy() for f in unpack_frames(batch['x'])]
        minv, _ = _A().solve(host_pts, base)
        want = np.stack([AO.warp(f, m, 64, 64, ds.item_mask(int(i))) for f, m, i in zip(frames, minv, batch['index'].cpu())])
        assert torch.equal(aligned.cpu(), torch.from_numpy(want))
        # a config without device_align, and a batch without landmarks, behave as before
        assert torch.equal(plain._images(batch, False), simple_val_augmentation()(batch['x'])) and plain.last_align_valid is None
        assert torch.equal(plain._images(batch['x'], False), simple_val_augmentation()(batch['x']))
        no_pts = {k: v for k, v in batch.items() if k not in ('pts', 'pts_host')}
        with pytest.raises(Exception):
            ctl._images(no_pts, False)          # ragged frames reach an augmentation without a fit stage: refused as before
    assert nb == 3 and ctl.align_rejected == 0 and plain.align_rejected == 0
    # rejected frames: counted, reported in evaluation, dropped from the training step
    batch = _to_device(next(iter(DataLoader(ds, 4, collate_fn=ragged_collate))), DEV)
    batch['pts_host'][2, 1] = batch['pts_host'][2, 0] + 1.0
    ctl.training_step(dict(batch, label=torch.arange(4, device=DEV)))
    assert ctl.model_loss.seen == {'n': 3, 'labels': [0, 1, 3]} and ctl.align_rejected == 1
    out = ctl.validation_step(batch)
    assert out['align_rejected'] == 1 and out['emb'].shape[0] == 4 and float(out['emb'][2]) == 0.0 and ctl.align_rejected == 2
    assert ctl._align_rejected([out, {'emb': None}]) == {'Align rejected': 1} and ctl._align_rejected([{'emb': None}]) == {}
