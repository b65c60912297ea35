"""Flip / ColorJitter / grayscale / erasing of the device augmentation, host side: the numpy restatement (tools/color_augment_np.py)
against the Pillow-produced tests/golden/color_augment.npz (tools/make_color_augment_golden.py) and, where Pillow imports, against
live Pillow (both HSV conversions over all 2^24 colours); the decision draws, the argument validation and the host record builders of
csrc/pfr_augment_color.hip.  CPU only."""
import math
import os

import numpy as np
import pytest
import torch

from tools import color_augment_np as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "color_augment.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ------------------------------------------------------------------------------------------------- restatement vs the golden
def test_each_op_alone_equals_pillow_golden(gold):
    a, b = gold["a"], gold["b"]
    assert a.shape == (61, 47, 3) and b.shape == (48, 52, 3)
    factors = [float(f) for f in gold["factors"]]
    assert 0.0 in factors and 1.0 in factors and any(0 < f < 1 for f in factors) and any(f > 1 for f in factors)
    for op, fn in enumerate((R.brightness, R.contrast, R.saturation)):
        for k, f in enumerate(factors):
            assert np.array_equal(fn(a, f), gold[f"a_op{op}"][k]), (fn.__name__, f)
    hues = [float(h) for h in gold["hues"]]
    assert 0.0 in hues and 0.5 in hues and -0.5 in hues and any(0 < h < 0.1 for h in hues) and any(-0.1 < h < 0 for h in hues)
    for k, h in enumerate(hues):
        assert np.array_equal(R.hue(a, R.hue_shift_byte(h)), gold["a_op3"][k]), h
    assert np.array_equal(R.luma(a), gold["a_luma"])
    for t, img in (("a", a), ("b", b)):
        assert np.array_equal(R.hflip(img), gold[f"{t}_flip"]) and np.array_equal(R.grayscale(img), gold[f"{t}_gray"])


def test_four_fixed_orders_equal_pillow_golden(gold):
    orders = gold["orders"]
    assert orders[0][0] == 1 and orders[1][3] == 1 and len(orders) == 4          # contrast first, contrast last
    f, shift = [float(v) for v in gold["order_factors"]], R.hue_shift_byte(float(gold["order_hue"]))
    outs = [R.jitter(gold["b"], o, f, shift) for o in orders]
    for k in range(4):
        assert np.array_equal(outs[k], gold["b_orders"][k]), orders[k]
    assert not np.array_equal(outs[0], outs[1])                                  # the order matters


# ------------------------------------------------------------------------------------------------ restatement vs live Pillow
def test_restatement_equals_live_pillow_on_random_images():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageOps
    rng = np.random.default_rng(5)
    for h, w in ((37, 53), (8, 3), (1, 1)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pil = Image.fromarray(img)
        for f in (0, 0.37, 0.8, 1, 1.2, 1.73, 2, float(np.float32(rng.uniform(0, 3)))):
            for fn, E in ((R.brightness, ImageEnhance.Brightness), (R.contrast, ImageEnhance.Contrast), (R.saturation, ImageEnhance.Color)):
                assert np.array_equal(fn(img, f), np.asarray(E(pil).enhance(f))), (fn.__name__, f, h, w)
        assert np.array_equal(R.hflip(img), np.asarray(ImageOps.mirror(pil)))
        assert np.array_equal(R.luma(img), np.asarray(pil.convert("L")))


def test_hsv_conversions_equal_pillow_over_all_colours():
    """Convert.c rgb2hsv_row and hsv2rgb, every one of the 2^24 inputs, both directions"""
    pytest.importorskip("PIL")
    from PIL import Image
    a = np.empty((256, 256, 3), np.uint8)
    a[..., 1] = np.arange(256, dtype=np.uint8)[:, None]
    a[..., 2] = np.arange(256, dtype=np.uint8)[None, :]
    bad_fwd = bad_back = 0
    for r in range(256):
        a[..., 0] = r
        hsv = Image.frombuffer("HSV", (256, 256), a.tobytes(), "raw", "HSV", 0, 1)
        rgb = Image.frombuffer("RGB", (256, 256), a.tobytes(), "raw", "RGB", 0, 1)
        bad_fwd += int((np.asarray(rgb.convert("HSV")) != R.rgb2hsv(a)).any(-1).sum())
        bad_back += int((np.asarray(hsv.convert("RGB")) != R.hsv2rgb(a)).any(-1).sum())
    assert (bad_fwd, bad_back) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- the draws
def _aug(**kw):
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    return DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, torch.Generator().manual_seed(7), **kw)


def test_draw_statistics_of_the_new_decisions():
    n = 20000
    scale, ratio = (0.02, 0.33), (0.3, 3.3)
    aug = _aug(p_hflip=0.5, color_jitter=dict(brightness=0.2, contrast=(0.5, 1.5), saturation=1.5, hue=0.02), p_grayscale=0.1,
               erasing=dict(p=0.25, scale=scale, ratio=ratio, value=0))
    e = aug.draw_extra(n, 224, 224)
    assert e["flip"].shape == (n,) and e["order"].shape == (n, 4) and e["factors"].shape == (n, 3) and e["erase"].shape == (n, 5)
    assert abs(e["flip"].float().mean().item() - 0.5) < 0.02 and abs(e["gray"].float().mean().item() - 0.1) < 0.02
    f = e["factors"]
    for k, (lo, hi) in enumerate(((0.8, 1.2), (0.5, 1.5), (0.0, 2.5))):
        assert f[:, k].min() >= lo and f[:, k].max() <= hi and f[:, k].min() < lo + 0.02 * (hi - lo) and f[:, k].max() > hi - 0.02 * (hi - lo)
        assert abs(f[:, k].mean().item() - (lo + hi) / 2) < 0.02 * (hi - lo)
    assert e["hue"].min() >= -0.02 and e["hue"].max() <= 0.02 and e["hue"].min() < -0.019 and e["hue"].max() > 0.019
    order = e["order"]
    assert (order.sort(dim=1).values == torch.arange(4)).all()
    code = (order * torch.tensor([64, 16, 4, 1])).sum(1)
    counts = torch.unique(code, return_counts=True)[1]
    assert len(counts) == 24 and (counts - n / 24).abs().max() < 6 * math.sqrt(n / 24)
    er = e["erase"]
    on = er[:, 0] == 1
    assert abs(on.float().mean().item() - 0.25) < 0.02 and (er[~on] == 0).all()
    i, j, h, w = (er[on][:, k].double() for k in range(1, 5))
    assert (i >= 0).all() and (j >= 0).all() and (h >= 1).all() and (w >= 1).all() and (i + h <= 224).all() and (j + w <= 224).all()
    # h, w are the rounded sides of an area * aspect draw: half a pixel of slack on each side
    area_lo, area_hi = (h - 0.5) * (w - 0.5) / 224 ** 2, (h + 0.5) * (w + 0.5) / 224 ** 2
    assert (area_hi >= scale[0]).all() and (area_lo <= scale[1]).all()
    assert ((h + 0.5) / (w - 0.5) >= ratio[0]).all() and ((h - 0.5) / (w + 0.5) <= ratio[1]).all()
    assert (h * w / 224 ** 2).mean() > 0.05 and len(torch.unique(i)) > 100 and len(torch.unique(j)) > 50


def test_defaults_leave_the_existing_stream_alone():
    """values printed by the parent commit for seed 1234 (n = 6): `draw` is what it was, and `draw_extra` draws nothing"""
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    pins = (
        ({}, 224, [[1, 0, 4, 2], [0, 0, 2, 2], [1, 0, 3, 3], [1, 0, 2, 2], [0, 0, 1, 0], [0, 0, 3, 4]],
         ['0x1.2a912c0000000p+2', '0x1.3322900000000p+1', '-0x1.ee68980000000p-2', '-0x1.f108500000000p-3', '0x1.6bc4ce0000000p+1',
          '-0x1.bcce0a0000000p+1']),
        (dict(fit=('thumbnail_pad', (256, 256)), order='geometry_first', crop=(252, 252), size=(256, 256)), 256,
         [[0, 0, 0, 2], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 4], [0, 0, 1, 3], [0, 1, 4, 1]],
         ['0x1.5fcf020000000p+1', '0x1.9aa0960000000p+1', '-0x1.1a86a80000000p+1', '0x1.d12e2c0000000p+0', '-0x1.14e5640000000p+1',
          '0x1.913ad80000000p+0']),
    )
    for kw, side, flags, angles in pins:
        g = torch.Generator().manual_seed(1234)
        a = DeviceAugmentation(generator=g, **kw)
        f, ang = a.draw(6, side, side)
        assert f.dtype == torch.int32 and f.shape == (6, 4) and ang.shape == (6,) and ang.dtype == torch.float32
        assert f.tolist() == flags and [float.hex(v) for v in ang.double().tolist()] == angles
        state = g.get_state().clone()
        assert a.draw_extra(6, side, side) is None and torch.equal(g.get_state(), state)
    # with the new ops on, `draw` still draws the same values first
    g = torch.Generator().manual_seed(1234)
    f, ang = DeviceAugmentation(generator=g, p_hflip=0.5, color_jitter=(0.2, 0.2, 0.2, 0.02), erasing={'p': 0.25}).draw(6, 224, 224)
    assert f.tolist() == pins[0][2]


def test_argument_validation():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    for bad in (dict(brightness=-0.1), dict(contrast=-1), dict(saturation=-0.5), dict(hue=-0.1), dict(hue=0.6), dict(hue=(-0.6, 0.1)),
                dict(brightness=(1.2, 0.8)), (0.2, 0.2, 0.2), dict(sharpness=1)):
        with pytest.raises(ValueError):
            DeviceAugmentation(color_jitter=bad)
    for bad in (dict(p_hflip=1.5), dict(p_grayscale=-0.1), dict(erasing=dict(p=2)), dict(erasing=dict(scale=(0.5, 0.1))),
                dict(erasing=dict(ratio=(0, 1))), dict(erasing=dict(value=(1, 2)))):
        with pytest.raises(ValueError):
            DeviceAugmentation(**bad)
    with pytest.raises(PfrError, match="random"):
        DeviceAugmentation(erasing=dict(p=0.5, value='random'))
    with pytest.raises(TypeError):
        DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, None, None, 'color_first', 0.5)      # keyword-only
    a = DeviceAugmentation(color_jitter=(0.2, 0, (0.5, 1.5), 0.5), erasing=dict(p=0.3, value=(0.1, 0.2, 0.3)))
    assert a.ops_mask == 0b1101 and a.jitter[0] == (0.8, 1.2) and a.jitter[1] is None and a.jitter[3] == (-0.5, 0.5)
    assert a.erasing[3].tolist() == pytest.approx([0.1, 0.2, 0.3])
    assert DeviceAugmentation(color_jitter=(0, 0, 0, 0), erasing=dict(p=0)).draw_extra(4, 224, 224) is None


def test_ragged_color_first_refuses_the_new_colour_ops():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    fit = ('resize', (224, 224))
    for kw in (dict(p_hflip=0.5), dict(color_jitter=(0.2, 0.2, 0.2, 0.02)), dict(p_grayscale=0.1)):
        with pytest.raises(PfrError, match="ragged"):
            DeviceAugmentation(fit=fit, **kw)
    DeviceAugmentation(fit=fit, erasing=dict(p=0.25))                                                   # erasing works in every shape
    DeviceAugmentation((252, 252), (256, 256), fit=('thumbnail_pad', (256, 256)), order='geometry_first', p_hflip=0.5,
                       color_jitter=(0.2, 0.2, 0.2, 0.02), p_grayscale=0.1)


# ------------------------------------------------------------------------------------------------------ host record builders
def test_record_builders_equal_a_python_restatement():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.data_loading.augment import color_records, erase_records
    rng = np.random.default_rng(11)
    n = 500
    flip, gray = rng.integers(0, 2, n), rng.integers(0, 2, n)
    order = np.stack([rng.permutation(4) for _ in range(n)])
    factors = rng.uniform(0, 3, (n, 3)).astype(np.float32)
    hue = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    hue[:4] = (0.5, -0.5, 0.0, -0.001)
    for ops_mask in (15, 0b0101, 0b1010, 0):
        rec, mask = color_records(flip, gray, order, factors, hue, ops_mask)
        want = np.zeros((n, 12), np.int32)
        for i in range(n):
            run = [int(op) for op in order[i] if ops_mask >> int(op) & 1]
            want[i, :2] = (flip[i], gray[i])
            want[i, 2:6] = run + [-1] * (4 - len(run))
            want[i, 6:9] = factors[i].view(np.int32)
            want[i, 9] = R.hue_shift_byte(float(hue[i])) if ops_mask & 8 else 0
        assert np.array_equal(rec, want), ops_mask
        assert mask == (1 | 2 | (4 if ops_mask & 2 else 0))
    rec, mask = color_records(np.zeros(3), np.zeros(3), np.tile(np.arange(4), (3, 1)), np.ones((3, 3)), np.zeros(3), 0)
    assert mask == 0 and (rec[:, 2:6] == -1).all()
    with pytest.raises(PfrError, match="permutation"):
        color_records([0], [0], [[0, 1, 1, 3]], [[1, 1, 1]], [0], 15)
    with pytest.raises(PfrError, match="hue"):
        color_records([0], [0], [[0, 1, 2, 3]], [[1, 1, 1]], [0.7], 15)

    H, W = 61, 47
    rects = np.zeros((n, 5), np.int32)
    rects[:, 0] = rng.integers(0, 2, n)
    rects[:, 3], rects[:, 4] = rng.integers(1, H + 1, n), rng.integers(1, W + 1, n)
    rects[:, 1], rects[:, 2] = rng.integers(0, H - rects[:, 3] + 1), rng.integers(0, W - rects[:, 4] + 1)
    value = np.array([0.25, -1.5, 3.0], np.float32)
    rec, area = erase_records(rects, value, H, W)
    want = np.zeros((n, 8), np.int32)
    on = rects[:, 0] == 1
    want[on, :5] = rects[on]
    want[on, 5:] = value.view(np.int32)
    assert np.array_equal(rec, want) and area == int((rects[on, 3] * rects[on, 4]).max())
    assert erase_records(np.zeros((2, 5)), 0.0, H, W)[1] == 0
    for bad in ((1, 60, 0, 2, 1), (1, 0, 46, 1, 2), (1, -1, 0, 1, 1), (1, 0, 0, 0, 5), (1, 0, 0, 62, 1)):
        with pytest.raises(PfrError, match="outside"):
            erase_records([bad], 0.0, H, W)


def test_new_symbols_and_config():
    import re
    from pets_face_recognition_amd._hip.lib import HEADER_PATH, parse_header, lib, _NO_CHECK
    protos, table, hdr = parse_header(), lib.symbols(), open(HEADER_PATH).read()
    for name in ("pfr_augment_color_params", "pfr_augment_color_ws_bytes", "pfr_augment_color", "pfr_augment_erase_params", "pfr_augment_erase",
                 "pfr_augment_geo_color_ws_bytes", "pfr_augment_train_geo_color"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in protos and name in table, name
    assert {"pfr_augment_color_ws_bytes", "pfr_augment_geo_color_ws_bytes"} <= _NO_CHECK
    assert lib.pfr_augment_color_ws_bytes(5) >= 40 and lib.pfr_augment_color_ws_bytes(5) % 256 == 0
    base = lib.pfr_augment_geo_ws_bytes(4, 64, 64)
    assert lib.pfr_augment_geo_color_ws_bytes(4, 70, 80, 64, 64, 2) >= base + 32
    assert lib.pfr_augment_geo_color_ws_bytes(4, 70, 80, 64, 64, 3) >= base + 32 + 4 * 70 * 80 * 3
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "csrc", "build.sh")).read()
    assert "pfr_augment_color" in src
    cfg = open(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", "fe_r18_mi355x_jitter.py")).read()
    assert "p_hflip=0.5" in cfg and "(0.2, 0.2, 0.2, 0.02)" in cfg and "0.25" in cfg
