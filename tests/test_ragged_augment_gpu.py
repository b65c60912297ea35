"""The fit stage (csrc/pfr_augment_fit.hip) and the geometry-first order (pfr_augment_train_geo) on the device against
tests/golden/ragged_augment.npz, which holds the output of the installed Pillow (tools/make_ragged_golden.py).  Every
comparison is exact: all device arithmetic is integer or table-driven."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "ragged_augment.npz")
DEV = "cuda:0"
FIT_GROUPS = ("rs48", "tp48", "rs_rect", "tp_rect", "rs224", "tp256")


def _ragged(cases):
    from pets_face_recognition_amd.data_loading.ragged import pack_frames, seeded_frame
    x = pack_frames([seeded_frame(int(s), int(h), int(w)) for s, h, w in cases[:, :3]])
    return {'data': x['data'].to(DEV), 'shape': x['shape'].to(DEV), 'shape_host': x['shape_host']}     # as the trainer hands it over


def _fit(z, tag, aug=None):
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    mode = ('resize', 'thumbnail_pad')[int(z[f"{tag}_mode"])]
    canvas = tuple(int(v) for v in z[f"{tag}_canvas"])
    aug = aug or DeviceAugmentation(None, None, 0, 0, 0, fit=(mode, canvas))
    cases = z[f"{tag}_cases"]
    out = aug.fit_apply(_ragged(cases), cases[:, 3:5])
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("tag", FIT_GROUPS)
def test_fit_equals_pillow_golden_byte_for_byte(tag):
    z = np.load(GOLD)
    got, want = _fit(z, tag), z[f"{tag}_out"]
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    print(tag, "cases", len(want), "mismatching", bad, "max |diff|", int(np.abs(got.astype(int) - want).max()))
    assert not bad, (tag, [(i, z[f"{tag}_cases"][i].tolist(), z[f"{tag}_plan"][i].tolist()) for i in bad[:4]])


def test_fit_two_launches_give_identical_bits():
    z = np.load(GOLD)
    for tag in ("rs48", "tp48"):
        assert np.array_equal(_fit(z, tag), _fit(z, tag))


def _geo_inputs(z):
    from pets_face_recognition_amd.data_loading.ragged import seeded_frame
    h, w = (int(v) for v in z["geo_hw"])
    return np.stack([seeded_frame(int(s), h, w) for s in z["geo_seeds"]])


def test_train_geo_equals_pillow_golden():
    """crop → resize → rotate, then sharpness / autocontrast on the rotated image: all four flag combinations at non-zero angles"""
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    z = np.load(GOLD)
    crop, size = int(z["geo_crop"]), int(z["geo_size"])
    dec, angles, want = z["geo_dec"], z["geo_angles"], z["geo_out"]
    assert {(int(a), int(b)) for a, b in dec[:, :2]} == {(0, 0), (1, 0), (0, 1), (1, 1)} and (angles != 0).all()
    aug = DeviceAugmentation((crop, crop), (size, size), order='geometry_first')
    y = aug.apply(torch.from_numpy(_geo_inputs(z)).to(DEV), torch.from_numpy(dec), torch.from_numpy(angles))
    torch.cuda.synchronize()
    y = y.cpu()
    u8 = (y * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(u8, want), [i for i in range(len(want)) if not np.array_equal(u8[i], want[i])]
    assert torch.equal(y, torch.from_numpy(want.transpose(0, 3, 1, 2).copy()).float() / 255)
    y2 = aug.apply(torch.from_numpy(_geo_inputs(z)).to(DEV), torch.from_numpy(dec), torch.from_numpy(angles))
    assert torch.equal(y2.cpu(), y)
    # the colour-first kernel on the same decisions differs wherever a colour op is on (the order is what is tested)
    cf = DeviceAugmentation((crop, crop), (size, size)).apply(torch.from_numpy(_geo_inputs(z)).to(DEV), torch.from_numpy(dec), torch.from_numpy(angles)).cpu()
    for i in range(len(dec)):
        assert torch.equal(cf[i], y[i]) == (not dec[i, :2].any())


def _check_train(y, z, tag):
    y = y.cpu()
    u8 = (y * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    assert torch.equal(y, torch.from_numpy(u8.transpose(0, 3, 1, 2).copy()).float() / 255)
    want, sha = z[f"{tag}_out"], z[f"{tag}_sha"]
    assert len(sha) >= 32 and u8.shape[0] == len(sha)
    assert np.array_equal(u8[:len(want)], want), tag
    got = [hashlib.sha256(u8[i].tobytes()).hexdigest() for i in range(len(sha))]
    assert got == list(sha), (tag, [i for i in range(len(sha)) if got[i] != sha[i]])


def test_simple_family_pipelines_on_a_ragged_batch():
    """simple_fe_dog.py:17-31 at a 48 canvas (crop 44): the colour ops act on the raw frame, in the fit stage"""
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    z = np.load(GOLD)
    cases = z["rs48_cases"]
    flags = np.concatenate([cases[:, 3:5], z["simple48_dec"][:, 2:4]], axis=1).astype(np.int32)
    train = DeviceAugmentation((44, 44), (48, 48), 0.1, 0.3, 5.0, fit=('resize', (48, 48)))
    _check_train(train.apply(_ragged(cases), torch.from_numpy(flags), torch.from_numpy(z["simple48_angles"])), z, "simple48")
    # val: Resize → ToTensor on all frames, without colour ops
    val = DeviceAugmentation(None, None, 0, 0, 0, fit=('resize', (48, 48)))
    y = val(_ragged(cases)).cpu()
    u8 = (y * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
    assert len(cases) >= 32 and torch.equal(y, torch.from_numpy(u8.transpose(0, 3, 1, 2).copy()).float() / 255)
    assert [hashlib.sha256(u8[i].tobytes()).hexdigest() for i in range(len(cases))] == list(z["rs48_plain_sha"])
    keep = [i for i, c in enumerate(cases) if not c[3] and not c[4]]
    assert np.array_equal(u8[keep], z["rs48_out"][keep])


def test_body_family_pipelines_on_a_ragged_batch():
    """body_dog_fe.py:18-33 at a 48 canvas (crop 44): thumbnail + pad, geometry, then the colour ops on the rotated image"""
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    z = np.load(GOLD)
    cases = z["tp48_cases"]
    train = DeviceAugmentation((44, 44), (48, 48), 0.1, 0.3, 5.0, fit=('thumbnail_pad', (48, 48)), order='geometry_first')
    _check_train(train.apply(_ragged(cases), torch.from_numpy(z["body48_dec"]), torch.from_numpy(z["body48_angles"])), z, "body48")
    val = DeviceAugmentation(None, None, 0, 0, 0, fit=('thumbnail_pad', (48, 48)))
    y = val(_ragged(cases)).cpu()
    assert len(cases) >= 32 and torch.equal(y, torch.from_numpy(z["tp48_out"].transpose(0, 3, 1, 2).copy()).float() / 255)


def test_uniform_sized_ragged_batch_equals_the_uniform_path():
    """frames of ONE size: fit=('resize', …) + the train tail == a host-side Pillow resize + the existing uniform pipeline"""
    from PIL import Image
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    from pets_face_recognition_amd.data_loading.ragged import pack_frames, seeded_frame
    frames = [seeded_frame(200 + i, 150, 260) for i in range(12)]
    x = pack_frames(frames)
    rag = DeviceAugmentation((220, 220), (224, 224), 0.0, 0.0, 5.0, torch.Generator().manual_seed(3), fit=('resize', (224, 224)))
    uni = DeviceAugmentation((220, 220), (224, 224), 0.0, 0.0, 5.0, torch.Generator().manual_seed(3))
    flags, angles = uni.draw(12, 224, 224)
    host = np.stack([np.asarray(Image.fromarray(f).resize((224, 224), Image.BILINEAR)) for f in frames])
    want = uni.apply(torch.from_numpy(host).to(DEV), flags, angles)
    got = rag.apply({'data': x['data'].to(DEV), 'shape': x['shape']}, flags, angles)
    assert torch.equal(got, want)
    f2, a2 = rag.draw(12, 224, 224)
    assert torch.equal(f2, flags) and torch.equal(a2, angles)          # same generator seed → same decision stream


def test_oversize_frame_raises():
    from pets_face_recognition_amd._hip import PfrError
    from pets_face_recognition_amd.data_loading import DeviceAugmentation
    x = {'data': torch.zeros(4097 * 2 * 3 + 16, dtype=torch.uint8, device=DEV), 'shape': torch.tensor([[4097, 2]], dtype=torch.int32)}
    with pytest.raises(PfrError, match="4096"):
        DeviceAugmentation(None, None, 0, 0, 0, fit=('resize', (48, 48)))(x)
    with pytest.raises(PfrError, match="fit="):
        DeviceAugmentation()({'data': x['data'], 'shape': torch.tensor([[8, 8]], dtype=torch.int32)})


@pytest.mark.parametrize("name", ["fe_r50_mi355x_pipeline_simple", "fe_r50_mi355x_pipeline_body"])
def test_main_on_the_new_configs(name, tmp_path):
    cfg = os.path.join(ROOT, "pets-face-recognition_amd", "configs", "synthetic", name + ".py")
    env = dict(os.environ, PFR_LIMIT_TRAIN_BATCHES="3", PFR_VAL_IDS="8", PFR_WORKERS="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--config", cfg], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "Completed!" in r.stdout and "Val Recall@K=10" in r.stdout
    losses = [float(l.split("loss")[1]) for l in r.stdout.splitlines() if l.startswith("epoch") and "loss" in l]
    assert losses and all(np.isfinite(l) for l in losses)
