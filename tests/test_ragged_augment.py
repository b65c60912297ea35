"""Ragged frame batches and the host side of the fit stage (csrc/pfr_augment_fit.hip): container layout, Pillow's size / box /
coefficient arithmetic against tests/golden/ragged_augment.npz (tools/make_ragged_golden.py), the C-ABI surface and the new
configs.  CPU only."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ragged_augment.npz")
FIT_GROUPS = ("rs48", "tp48", "rs_rect", "tp_rect", "rs224", "tp256")
NEW_SYMBOLS = ("pfr_augment_fit_params", "pfr_augment_fit_coeff_ints", "pfr_augment_fit_ws_bytes", "pfr_augment_fit",
               "pfr_augment_train_geo", "pfr_augment_geo_ws_bytes")


def test_ragged_collate_layout_and_alignment():
    from pets_face_recognition_amd.data_loading.ragged import ragged_collate, unpack_frames, ragged_offsets, seeded_frame
    sizes = [(5, 7), (64, 64), (1, 1), (33, 90), (16, 16)]
    samples = [{'x': torch.from_numpy(seeded_frame(i, h, w)), 'label': torch.tensor(i), 'index': torch.tensor(10 + i)}
               for i, (h, w) in enumerate(sizes)]
    b = ragged_collate(samples)
    x = b['x']
    assert set(x) == {'data', 'shape', 'shape_host'} and np.array_equal(x['shape_host'], x['shape'].numpy()) and x['data'].dtype == torch.uint8 and x['data'].dim() == 1
    assert x['shape'].dtype == torch.int32 and x['shape'].tolist() == [list(s) for s in sizes]
    assert b['label'].tolist() == list(range(5)) and b['index'].tolist() == list(range(10, 15))
    off, total = ragged_offsets(x['shape'].numpy())
    assert total == x['data'].numel() and (off % 16 == 0).all() and total % 16 == 0
    for i, (h, w) in enumerate(sizes):
        assert off[i] >= (off[i - 1] + sizes[i - 1][0] * sizes[i - 1][1] * 3 if i else 0)
        assert torch.equal(x['data'][off[i]:off[i] + h * w * 3].reshape(h, w, 3), samples[i]['x'])
    for f, s in zip(unpack_frames(x), samples):
        assert torch.equal(f, s['x'])
    with pytest.raises(ValueError):
        ragged_collate([{'x': torch.zeros(3, 8, 8), 'label': torch.tensor(0)}])


def test_synthetic_dataset_ragged_sizes():
    from pets_face_recognition_amd.data_loading import SyntheticRecDataset
    ds = SyntheticRecDataset(6, 4, 224, seed=3, raw_uint8=True, ragged=True)
    shapes = []
    for i in range(len(ds)):
        x = ds[i]['x']
        assert x.dtype == torch.uint8 and x.dim() == 3 and x.shape[2] == 3
        h, w = x.shape[:2]
        assert 64 <= min(h, w) and max(h, w) <= 1400 and max(h, w) <= 3 * min(h, w)
        shapes.append((h, w))
    assert len(set(shapes)) > 12
    assert torch.equal(ds[5]['x'], SyntheticRecDataset(6, 4, 224, seed=3, raw_uint8=True, ragged=True)[5]['x'])
    assert SyntheticRecDataset(6, 4, 224, seed=3, raw_uint8=True)[5]['x'].shape == (224, 224, 3)     # default: uniform, as before


def _digest(tab):
    return hashlib.sha256(np.ascontiguousarray(tab, dtype='<i4').tobytes()).hexdigest()


def test_fit_params_equal_pillow_derived_golden():
    """pfr_augment_fit_params is host code: sizes, reduce factors, boxes, pad offsets, tap counts and both coefficient tables of every
    golden case equal the values of the Pillow-checked restatement exactly"""
    from pets_face_recognition_amd.data_loading.augment import fit_params
    z = np.load(GOLD)
    for tag in FIT_GROUPS:
        mode = ('resize', 'thumbnail_pad')[int(z[f"{tag}_mode"])]
        canvas = tuple(int(v) for v in z[f"{tag}_canvas"])
        cases, plan, box, want_hash = z[f"{tag}_cases"], z[f"{tag}_plan"], z[f"{tag}_box"], z[f"{tag}_coefhash"]
        rec, coeffs = fit_params(mode, cases[:, 1:3], canvas)
        assert rec.shape == (len(cases), 32)
        assert np.array_equal(rec[:, 0:2], cases[:, 1:3])
        # plan columns: tw th fx fy rb0..3 pad_l pad_t rw rh ksx ksy need_h need_v
        got = np.concatenate([rec[:, 2:10], rec[:, 14:16], rec[:, 22:24], rec[:, [17, 19]], rec[:, 25:27]], axis=1)
        assert np.array_equal(got, plan), (tag, np.argwhere(got != plan)[:5])
        assert np.array_equal(rec[:, 10:14].copy().view(np.float32), box), tag
        assert (rec[:, 20:22] == 0).all() and (rec[:, 24] == int(z[f"{tag}_mode"])).all()
        at = 0
        for i in range(len(cases)):
            tw, th, ksx, ksy = rec[i, 2], rec[i, 3], rec[i, 17], rec[i, 19]
            assert rec[i, 16] == at
            tx = coeffs[at:at + tw * (2 + ksx)]
            at += tw * (2 + ksx)
            assert rec[i, 18] == at
            ty = coeffs[at:at + th * (2 + ksy)]
            at += th * (2 + ksy)
            assert (_digest(tx), _digest(ty)) == tuple(want_hash[i]), (tag, i, cases[i])
        assert at == len(coeffs)


def test_fit_params_refuses_oversize_and_bad_modes():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.data_loading.augment import fit_params
    with pytest.raises(PfrError, match="4096"):
        fit_params('resize', [[4097, 10]], (48, 48))
    with pytest.raises(PfrError, match="100:1"):
        fit_params('thumbnail_pad', [[1000, 4]], (256, 256))
    fit_params('thumbnail_pad', [[300, 2]], (256, 256))          # taller than 100:1, but one pass only: the order cannot matter
    rec, _ = fit_params('thumbnail_pad', [[4096, 4096]], (256, 256))
    assert tuple(rec[0, 2:6]) == (256, 256, 8, 8)


def test_new_symbols_in_header_library_and_table():
    import ctypes
    from pets_face_recognition_amd._hip.lib import LIB_PATH, HEADER_PATH, parse_header, lib, _NO_CHECK
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    table = lib.symbols()
    hdr = open(HEADER_PATH).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in protos and name in table and hasattr(dll, name), name
    for name in ("pfr_augment_fit_coeff_ints", "pfr_augment_fit_ws_bytes", "pfr_augment_geo_ws_bytes"):
        assert name in _NO_CHECK
    assert lib.pfr_augment_fit_ws_bytes(1000, 4) >= 1000 + 4 * 8 * 8 * 4
    assert lib.pfr_augment_geo_ws_bytes(4, 48, 48) >= 2 * 4 * 48 * 48 * 3
    src = open(os.path.join(ROOT, "pets-face-recognition_amd", "csrc", "build.sh")).read()
    assert "pfr_augment_fit" in src


def test_legacy_arguments_keep_their_meaning():
    from pets_face_recognition_amd.data_loading import DeviceAugmentation, train_augmentation, val_augmentation
    from pets_face_recognition_amd._hip import PfrError
    for aug in (DeviceAugmentation(), DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, None), train_augmentation(), val_augmentation()):
        assert aug.fit is None and aug.order == 'color_first'
    a = DeviceAugmentation((220, 220), (224, 224), 0.4, 0.5, 5.0, torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)                       # the decision stream of the head pipeline is what it was
    u = torch.rand((16, 2), generator=g)
    flags, angles = a.draw(16, 224, 224)
    assert torch.equal(flags[:, 0], (u[:, 0] < 0.4).int()) and torch.equal(flags[:, 1], (u[:, 1] < 0.5).int())
    assert torch.equal(flags[:, 2], torch.randint(0, 5, (16,), generator=g).int())
    with pytest.raises(TypeError):
        DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, None, ('resize', (224, 224)))     # keyword-only
    with pytest.raises(PfrError):
        DeviceAugmentation(fit=('stretch', (224, 224)))
    with pytest.raises(PfrError):
        DeviceAugmentation(order='rotation_first')


def test_factories_describe_the_reference_pipelines():
    from pets_face_recognition_amd.data_loading import (simple_train_augmentation, simple_val_augmentation, body_train_augmentation,
                                                        body_val_augmentation)
    s, sv, b, bv = simple_train_augmentation(), simple_val_augmentation(), body_train_augmentation(), body_val_augmentation()
    assert s.fit == ('resize', (224, 224)) and s.order == 'color_first' and s.crop == (220, 220) and s.size == (224, 224)
    assert sv.fit == ('resize', (224, 224)) and sv.crop is None and sv.size is None and sv.p_sharpness == 0 and sv.degrees == 0
    assert b.fit == ('thumbnail_pad', (256, 256)) and b.order == 'geometry_first' and b.crop == (252, 252) and b.size == (256, 256)
    assert (b.p_sharpness, b.p_autocontrast, b.degrees) == (0.1, 0.3, 5.0) == (s.p_sharpness, s.p_autocontrast, s.degrees)
    assert bv.fit == ('thumbnail_pad', (256, 256)) and bv.crop is None and bv.p_autocontrast == 0
    # geometry-first draws the crop and the angle before the colour decisions
    g = torch.Generator().manual_seed(4)
    b.generator = torch.Generator().manual_seed(4)
    flags, angles = b.draw(8, 256, 256)
    assert torch.equal(flags[:, 2], torch.randint(0, 5, (8,), generator=g).int())


@pytest.mark.parametrize("name,size,fit", [("fe_r50_mi355x_pipeline_simple", 224, "resize"), ("fe_r50_mi355x_pipeline_body", 256, "thumbnail_pad")])
def test_new_configs_load_and_expose_the_contract(name, size, fit, tmp_path, monkeypatch):
    import pets_face_recognition_amd as pfr
    from pets_face_recognition_amd.utils import get_dict_wrapper
    pfr.install_reference_aliases()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("PFR_VAL_IDS", "4")
    monkeypatch.setenv("PFR_WORKERS", "0")
    cfg = get_dict_wrapper(os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", name + ".py"))
    for key in ("model", "loss", "optimizer", "train_dataloader", "val_dataloader", "pair_generator", "similarity_f", "n_epochs", "thrs",
                "far_thr", "k", "trainer_kwargs", "output", "device", "distributed_train", "world_size"):
        assert key in cfg, key
    tr, va = cfg['device_train_augmentation'], cfg['device_val_augmentation']
    assert tr.fit == (fit, (size, size)) and va.fit == (fit, (size, size))
    assert tr.order == ('geometry_first' if fit == 'thumbnail_pad' else 'color_first')
    batch = next(iter(cfg['val_dataloader']()))
    assert set(batch['x']) == {'data', 'shape', 'shape_host'} and batch['x']['shape'].shape[1] == 2 and len(batch['label']) == batch['x']['shape'].shape[0]
