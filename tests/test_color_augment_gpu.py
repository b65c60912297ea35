"""Flip / ColorJitter / grayscale / erasing on the device (csrc/pfr_augment_color.hip) against the numpy restatement of Pillow's
arithmetic (tools/color_augment_np.py, pinned to Pillow by tests/test_color_augment_host.py), composed with the existing ops of
oracle/augment_ref.py for the whole pipelines, and against the Pillow-produced cases of tests/golden/color_augment.npz.  Everything
is bit-exact: torch.equal."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import augment_ref as A
from tools import color_augment_np as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "color_augment.npz")
SYNTH = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic")
SIZES = ((61, 47), (48, 52))
FACTORS = (0.0, 1.0, 0.37, 1.73)
HUES = (0.0, 0.02, -0.02, 0.5, -0.5)
ALL = (0.2, 0.2, 0.2, 0.02)


def _frames(n, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 80 * np.sin(xx / 9.0 + seed), 128 + 100 * np.cos(yy / 7.0), 60 + 1.5 * (xx + yy)], -1)
    return np.clip(base[None] + rng.normal(0, 25, (n, h, w, 3)), 0, 255).astype(np.uint8)


def _aug(crop=None, size=None, **kw):
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    return DeviceAugmentation(crop, size, 0.0, 0.0, 0.0, **kw)


def _extra(n, flip=0, gray=0, order=(0, 1, 2, 3), factors=(1.0, 1.0, 1.0), hue=0.0, erase=None):
    """decisions in the layout `draw_extra` returns; scalars / single rows are repeated over the batch"""
    e = {'flip': torch.as_tensor(np.broadcast_to(np.asarray(flip, np.int32), (n,)).copy()),
         'gray': torch.as_tensor(np.broadcast_to(np.asarray(gray, np.int32), (n,)).copy()),
         'order': torch.as_tensor(np.broadcast_to(np.asarray(order, np.int32), (n, 4)).copy()),
         'factors': torch.as_tensor(np.broadcast_to(np.asarray(factors, np.float32), (n, 3)).copy()),
         'hue': torch.as_tensor(np.broadcast_to(np.asarray(hue, np.float32), (n,)).copy()),
         'erase': torch.as_tensor(np.zeros((n, 5), np.int32) if erase is None else np.asarray(erase, np.int32).reshape(n, 5))}
    return e


def _apply(aug, x, extra, flags=None, angles=None):
    n = x.shape[0]
    flags = torch.zeros((n, 4), dtype=torch.int32) if flags is None else torch.as_tensor(flags)
    angles = torch.zeros(n) if angles is None else torch.as_tensor(angles)
    y = aug.apply(torch.from_numpy(x).cuda(), flags, angles, extra)
    torch.cuda.synchronize()
    return y.cpu()


def _ref_color(aug, x, e):
    """flip → ColorJitter → grayscale of every frame, per the restatement"""
    out = []
    for i in range(x.shape[0]):
        order = [int(op) for op in e['order'][i] if aug.ops_mask >> int(op) & 1]
        out.append(R.color_pass(x[i], bool(e['flip'][i]), order, [float(f) for f in e['factors'][i]],
                                R.hue_shift_byte(float(e['hue'][i])), bool(e['gray'][i])))
    return out


def _ref_tensor(imgs, e, value=0.0):
    ys = []
    for i, img in enumerate(imgs):
        on, ii, jj, h, w = (int(v) for v in e['erase'][i])
        y = A.to_tensor(img).numpy()
        ys.append(R.erase(y, ii, jj, h if on else 0, w, value))
    return torch.from_numpy(np.stack(ys))


# ----------------------------------------------------------------------------------------------------------- each op alone
@pytest.mark.parametrize("hw", SIZES)
def test_flip_alone(hw):
    x = _frames(4, *hw, seed=1)
    aug = _aug(p_hflip=0.5)
    e = _extra(4, flip=[1, 0, 1, 1])
    assert torch.equal(_apply(aug, x, e), _ref_tensor(_ref_color(aug, x, e), e))
    assert torch.equal(_apply(aug, x, e)[0], A.to_tensor(x[0][:, ::-1].copy()))


@pytest.mark.parametrize("hw", SIZES)
def test_grayscale_alone(hw):
    x = _frames(4, *hw, seed=2)
    aug = _aug(p_grayscale=0.5)
    e = _extra(4, gray=[0, 1, 1, 0])
    y = _apply(aug, x, e)
    assert torch.equal(y, _ref_tensor(_ref_color(aug, x, e), e))
    assert torch.equal(y[1, 0], y[1, 1]) and torch.equal(y[0], A.to_tensor(x[0]))


@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("op", (0, 1, 2))
def test_each_blend_op_alone_at_the_four_factor_kinds(op, hw):
    """factor 0, 1, inside (0, 1) (truncation only) and above 1 (clip, then truncation) — one sample each"""
    x = _frames(4, *hw, seed=3 + op)
    cj = [0, 0, 0, 0]
    cj[op] = (0.0, 2.0)
    aug = _aug(color_jitter=tuple(cj))
    factors = np.ones((4, 3), np.float32)
    factors[:, op] = FACTORS
    e = _extra(4, factors=factors, order=[(0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 3, 2), (2, 3, 0, 1)])
    assert torch.equal(_apply(aug, x, e), _ref_tensor(_ref_color(aug, x, e), e))


@pytest.mark.parametrize("hw", SIZES)
def test_hue_alone(hw):
    x = _frames(5, *hw, seed=6)
    aug = _aug(color_jitter=(0, 0, 0, 0.5))
    e = _extra(5, hue=HUES)
    y = _apply(aug, x, e)
    assert torch.equal(y, _ref_tensor(_ref_color(aug, x, e), e))
    assert not torch.equal(y[0], A.to_tensor(x[0]))            # the HSV round trip loses bits at a zero shift too, as in Pillow


def test_hue_over_a_million_colours():
    """a 1024 x 1024 frame of 2^20 distinct colours spread over the whole cube (odd multiplier mod 2^24), shifts 0 and 0.31"""
    c = (np.arange(1 << 20, dtype=np.int64) * 6700417) & 0xFFFFFF
    x = np.stack([c >> 16, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(1, 1024, 1024, 3)
    x = np.concatenate([x, x])
    aug = _aug(color_jitter=(0, 0, 0, 0.5))
    e = _extra(2, hue=[0.0, 0.31])
    assert torch.equal(_apply(aug, x, e), _ref_tensor(_ref_color(aug, x, e), e))


@pytest.mark.parametrize("hw", SIZES)
def test_erasing_alone(hw):
    """interior rectangle, one touching the bottom-right corner, a 1 x 1 rectangle, the whole image, none; per-channel value"""
    H, W = hw
    x = _frames(5, H, W, seed=7)
    value = (0.25, 0.5, -1.0)
    aug = _aug(erasing=dict(p=0.5, value=value))
    rects = [(1, 3, 5, 20, 9), (1, H - 7, W - 11, 7, 11), (1, H - 1, W - 1, 1, 1), (1, 0, 0, H, W), (0, 0, 0, 0, 0)]
    e = _extra(5, erase=rects)
    y = _apply(aug, x, e)
    want = torch.stack([A.to_tensor(f) for f in x])
    for n, (on, i, j, h, w) in enumerate(rects):
        if on:
            want[n, :, i:i + h, j:j + w] = torch.tensor(value)[:, None, None]
    assert torch.equal(y, want) and torch.equal(y, _ref_tensor(list(x), e, value))
    aug1 = _aug(erasing=dict(p=0.5, value=0.5))
    assert torch.equal(_apply(aug1, x, e), _ref_tensor(list(x), e, 0.5))


# ------------------------------------------------------------------------------------------------------------- the 24 orders
def test_jitter_in_all_24_orders():
    x = _frames(8, 48, 52, seed=8)
    aug = _aug(color_jitter=(0.5, 0.5, 0.5, 0.1))
    rng = np.random.default_rng(9)
    orders = list(itertools.permutations(range(4)))
    seen = set()
    for k in range(3):
        e = _extra(8, order=orders[8 * k:8 * k + 8], factors=rng.uniform(0.5, 1.5, (8, 3)).astype(np.float32),
                   hue=rng.uniform(-0.1, 0.1, 8).astype(np.float32), flip=rng.integers(0, 2, 8), gray=[0] * 7 + [1])
        y = _apply(aug, x, e)
        assert torch.equal(y, _ref_tensor(_ref_color(aug, x, e), e)), k
        seen.update(tuple(o) for o in e['order'].tolist())
    assert len(seen) == 24


# ------------------------------------------------------------------------------------------------------------ whole pipelines
def _ref_pipeline(aug, x, flags, angles, e, geometry_first):
    """the restatement composed with oracle.augment_ref's sharpness / autocontrast / crop / resize / rotate"""
    crop, out = aug.crop[0], aug.size[0]
    imgs = []
    for i in range(x.shape[0]):
        sharp, contrast, top, left = (int(v) for v in flags[i])
        order = [int(op) for op in e['order'][i] if aug.ops_mask >> int(op) & 1]
        fac, shift = [float(f) for f in e['factors'][i]], R.hue_shift_byte(float(e['hue'][i]))

        def color(im):
            im = R.color_pass(im, False, order, fac, shift, bool(e['gray'][i]))
            im = A.smooth(im) if sharp else im
            return A.autocontrast(im) if contrast else im

        def geometry(im):
            im = A.resize_bilinear(np.ascontiguousarray(im[top:top + crop, left:left + crop]), out, out)
            return A.rotate_nearest(im, float(angles[i]))

        im = R.hflip(x[i]) if e['flip'][i] else x[i]
        imgs.append(color(geometry(im)) if geometry_first else geometry(color(im)))
    return imgs


def _pipeline_case(n, size, crop, out, geometry_first, seed):
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    value = (0.1, 0.2, 0.3)
    aug = DeviceAugmentation((crop, crop), (out, out), 0.5, 0.5, 5.0, torch.Generator().manual_seed(seed),
                             order='geometry_first' if geometry_first else 'color_first', p_hflip=0.5, color_jitter=(0.4, 0.4, 0.4, 0.05),
                             p_grayscale=0.3, erasing=dict(p=1.0, value=value))
    x = _frames(n, size, size, seed)
    flags, angles = aug.draw(n, size, size)
    e = aug.draw_extra(n, size, size)
    # mixed per-sample flags whatever the draw gave
    flags[:, 0] = torch.tensor([1, 0, 1, 0] * 2)[:n]
    flags[:, 1] = torch.tensor([1, 1, 0, 0] * 2)[:n]
    e['flip'] = torch.tensor([1, 0, 0, 1, 1, 0, 1, 0], dtype=torch.int32)[:n]
    e['gray'] = torch.tensor([0, 0, 1, 0, 1, 0, 0, 0], dtype=torch.int32)[:n]
    e['erase'][1::2] = 0
    assert e['erase'][:, 0].any()
    y = _apply(aug, x, e, flags, angles)
    want = _ref_tensor(_ref_pipeline(aug, x, flags.numpy(), angles.numpy(), e, geometry_first), e, value)
    return y, want


def test_whole_pipeline_color_first_224():
    y, want = _pipeline_case(4, 224, 220, 224, False, seed=21)
    assert y.shape == (4, 3, 224, 224) and torch.equal(y, want)


def test_whole_pipeline_geometry_first_64():
    y, want = _pipeline_case(8, 64, 60, 64, True, seed=22)
    assert y.shape == (8, 3, 64, 64) and torch.equal(y, want)


@pytest.mark.parametrize("tag", ("head", "body"))
def test_whole_pipeline_equals_the_pillow_golden(tag):
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    z = np.load(GOLD)
    size, crop, out, geo = (int(v) for v in z[f"{tag}_geom"])
    x, dec, order, erase, want = z[f"{tag}_x"], z[f"{tag}_dec"], z[f"{tag}_order"], z[f"{tag}_erase"], z[f"{tag}_y"]
    n = x.shape[0]
    aug = DeviceAugmentation((crop, crop), (out, out), 0.5, 0.5, 5.0, order='geometry_first' if geo else 'color_first', p_hflip=0.5,
                             color_jitter=ALL, p_grayscale=0.3, erasing=dict(p=0.5, value=0.5))
    flags = torch.from_numpy(dec[:, [2, 3, 4, 5]].astype(np.int32))
    e = _extra(n, flip=dec[:, 0].astype(np.int32), gray=dec[:, 1].astype(np.int32), order=order, factors=dec[:, 8:11].astype(np.float32),
               hue=dec[:, 7].astype(np.float32), erase=erase)
    y = _apply(aug, x, e, flags, dec[:, 6].astype(np.float32))
    assert torch.equal(y, _ref_tensor(list(want), e, 0.5))
    e0 = dict(e, erase=torch.zeros((n, 5), dtype=torch.int32))
    assert torch.equal(_apply(aug, x, e0, flags, dec[:, 6].astype(np.float32)), torch.stack([A.to_tensor(w) for w in want]))


# ------------------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("geo", (False, True))
def test_a_batch_without_new_ops_equals_the_feature_off(geo):
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    kw = dict(order='geometry_first' if geo else 'color_first')
    on = DeviceAugmentation((44, 44), (48, 48), 0.5, 0.5, 5.0, p_hflip=0.5, p_grayscale=0.5, erasing=dict(p=0.5), **kw)
    off = DeviceAugmentation((44, 44), (48, 48), 0.5, 0.5, 5.0, **kw)
    x = _frames(6, 48, 52, seed=30)
    flags, angles = DeviceAugmentation((44, 44), (48, 48), 0.5, 0.5, 5.0, torch.Generator().manual_seed(3), **kw).draw(6, 48, 52)
    base = _apply(off, x, None, flags, angles)
    assert torch.equal(_apply(on, x, _extra(6), flags, angles), base)
    assert torch.equal(_apply(on, x, None, flags, angles), base)
    assert on._color_ws is None                                 # nothing launched, no workspace


def test_solid_and_all_zero_images():
    x = np.zeros((3, 61, 47, 3), np.uint8)
    x[1] = (200, 30, 90)
    x[2] = 255
    aug = _aug(p_hflip=0.5, color_jitter=(0.5, 0.5, 0.5, 0.1), p_grayscale=0.5)
    for order, gray in (((1, 3, 0, 2), 0), ((3, 2, 1, 0), 0), ((0, 1, 2, 3), 1)):
        e = _extra(3, flip=1, gray=gray, order=order, factors=(1.3, 0.6, 1.5), hue=0.07)
        y = _apply(aug, x, e)
        assert torch.isfinite(y).all() and torch.equal(y, _ref_tensor(_ref_color(aug, x, e), e))


def test_contrast_mean_beyond_32_bits():
    """a 4200 x 4100 white frame: the L sum is 255 * 17.2 M > 2^32; with the right mean (255) Contrast leaves white white"""
    from pets_face_recognition_amd._hip import lib
    from pets_face_recognition_amd.data_loading.augment import color_records
    H, W = 4200, 4100
    x = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device='cuda')
    out = torch.zeros_like(x)
    rec, mask = color_records([0], [0], [[0, 1, 2, 3]], [[1.0, 0.5, 1.0]], [0.0], 0b0010)
    assert mask == 6
    ws = torch.empty(lib.pfr_augment_color_ws_bytes(1), dtype=torch.uint8, device='cuda')
    lib.pfr_augment_color(x.data_ptr(), 1, H, W, torch.from_numpy(rec).cuda().data_ptr(), mask, out.data_ptr(), ws.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(ws[:8].view(torch.int64).item()) == 255 * H * W and int(out.min().item()) == 255


def test_call_draws_and_applies_everything():
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    aug = DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, torch.Generator().manual_seed(4), p_hflip=0.5, color_jitter=ALL,
                             erasing=dict(p=0.5, value=2.0))
    y = aug(torch.from_numpy(_frames(8, 224, 224, seed=31)).cuda())
    assert y.shape == (8, 3, 224, 224) and torch.isfinite(y).all()
    erased = (y == 2.0).flatten(1).any(1)
    assert erased.any() and not erased.all() and float(y[~erased].max()) <= 1.0


# --------------------------------------------------------------------------------------------------------------- end to end
def test_main_with_jitter_config(tmp_path):
    """python main.py --config fe_r18_mi355x_jitter.py trains end to end (flip 0.5, ColorJitter(0.2, 0.2, 0.2, 0.02), erasing 0.25)"""
    cfg = os.path.join(SYNTH, "fe_r18_mi355x_jitter.py")
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="3")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", cfg], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(l == l and abs(l) != float("inf") for l in losses)
