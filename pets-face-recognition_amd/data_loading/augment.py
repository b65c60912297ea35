"""Device-side image augmentation: the reference's `train_augmentation` / `val_augmentation` Compose pipelines applied to a
whole uint8 batch on the GPU.  The ten FE configs of the reference use three pipeline shapes:

    head    (fe_dogs_config.py:17-32, cat_fe_head, masked_head_dog, masked_head_cat) — uniform frames
            train:  ToPILImage → RandomAdjustSharpness(0, 0.1) → RandomAutocontrast(0.3) → RandomCrop((220, 220)) →
                    Resize((224, 224)) → RandomRotation(5) → ToTensor
            val:    ToPILImage → [Resize((224, 224))] → ToTensor
    simple  (simple_fe_dog.py:17-31, simple_fe_cat, no_align_head_dog, no_align_head_cat) — the detector's raw crops, ragged
            train:  RandomAdjustSharpness → RandomAutocontrast → Resize((224, 224)) → RandomCrop(220) → Resize(224) →
                    RandomRotation(5) → ToTensor           (the colour ops act on the RAW frame)
            val:    Resize((224, 224)) → ToTensor
    body    (body_dog_fe.py:18-33, body_cat_fe) — ragged
            train:  Lambda(resize_with_padding) → RandomCrop(252) → Resize(256) → RandomRotation(5) →
                    RandomAdjustSharpness → RandomAutocontrast → ToTensor   (the colour ops see the rotated image)
            val:    Lambda(resize_with_padding) → ToTensor
            resize_with_padding (utils/preprocs.py:42-49) = Image.thumbnail((256, 256)) + centred zero pad to 256 x 256

`DeviceAugmentation(crop, size, p_sharpness, p_autocontrast, degrees)` is the head shape.  `fit=('resize' | 'thumbnail_pad',
(h, w))` puts a fit stage in front that turns a ragged batch (data_loading/ragged.py) into the uniform uint8 canvas
(csrc/pfr_augment_fit.hip); `order='geometry_first'` moves sharpness / autocontrast behind the rotation
(pfr_augment_train_geo).  simple = fit resize + colour first (the colour ops run inside the fit stage, on the raw frame);
body = fit thumbnail_pad + geometry first.

The reference runs these per sample on PIL images in dataloader worker processes; here the dataset hands over raw uint8
HWC frames (what `RecDataset.__getitem__` holds before the transform, data_loading/dataset.py:100-121), the batch is
uploaded once and csrc/pfr_augment.hip produces the float32 NCHW batch `batch['x']` the trainer consumes — same pixels,
bit for bit, as the PIL pipeline given the same random decisions (tests/test_augment_gpu.py, tests/test_ragged_augment_gpu.py).
The decisions themselves are drawn here on the host with the distributions torchvision uses (Bernoulli(p) flags, uniform
integer crop corner, uniform angle); the reference draws them inside worker processes with per-worker seeds, so its stream
is not reproducible and is not part of the contract.  There is no CPU implementation: without the HIP library this module
raises.
"""
import ctypes

import numpy as np
import torch

from .._hip import lib, PfrError
from .ragged import MAX_SIDE, is_ragged, ragged_offsets

_REC = 12
_FIT_REC = 32
_FIT_MODES = {'resize': 0, 'thumbnail_pad': 1}
_R_SHARP, _R_CONTRAST = 20, 21


def _stream():
    return torch.cuda.current_stream().cuda_stream


def fit_params(mode, shape, canvas):
    """host part of the fit stage (no device work): shape int [N, 2] = (H, W) → (records int32 [N, 32], coeffs int32 [K])"""
    shape = np.ascontiguousarray(np.asarray(shape), dtype=np.int32).reshape(-1, 2)
    n = shape.shape[0]
    if n and int(shape.max()) > MAX_SIDE:
        raise PfrError(f"DeviceAugmentation: frame side {int(shape.max())} above {MAX_SIDE}")
    ch, cw = canvas
    k = lib.pfr_augment_fit_coeff_ints(_FIT_MODES[mode], shape.ctypes.data, n, ch, cw)
    if k < 0:
        raise PfrError(f"pfr_augment_fit_coeff_ints failed: {lib.pfr_last_error().decode()}")
    rec = np.zeros((n, _FIT_REC), np.int32)
    coeffs = np.zeros(k, np.int32)
    lib.pfr_augment_fit_params(_FIT_MODES[mode], shape.ctypes.data, n, ch, cw, rec.ctypes.data, coeffs.ctypes.data, k)
    return rec, coeffs


class DeviceAugmentation:
    """crop=None → no random crop (validation); size=None → no resize; p_* = 0 and degrees = 0 switch the others off.
    fit=None: uniform uint8 [N, H, W, 3] batches; fit=(mode, (h, w)): ragged batches, brought to the h x w canvas first.
    order: where sharpness / autocontrast sit relative to crop → resize → rotate."""

    def __init__(self, crop=(220, 220), size=(224, 224), p_sharpness=0.1, p_autocontrast=0.3, degrees=5.0, generator=None, *,
                 fit=None, order='color_first'):
        self.crop = tuple(crop) if crop is not None else None
        self.size = tuple(size) if size is not None else None
        self.p_sharpness, self.p_autocontrast, self.degrees = float(p_sharpness), float(p_autocontrast), float(degrees)
        self.generator = generator
        if fit is not None:
            mode, canvas = fit
            if mode not in _FIT_MODES or len(tuple(canvas)) != 2:
                raise PfrError(f"DeviceAugmentation: fit must be None, ('resize', (h, w)) or ('thumbnail_pad', (h, w)), got {fit!r}")
            fit = (mode, (int(canvas[0]), int(canvas[1])))
        if order not in ('color_first', 'geometry_first'):
            raise PfrError(f"DeviceAugmentation: order must be 'color_first' or 'geometry_first', got {order!r}")
        if fit is not None and fit[0] == 'thumbnail_pad' and order == 'color_first' and (self.p_sharpness > 0 or self.p_autocontrast > 0):
            raise PfrError("DeviceAugmentation: colour ops in front of thumbnail_pad are no pipeline of the reference")
        self.fit, self.order = fit, order
        self._ws = None
        self._fit_ws = None

    def draw(self, n, H, W):
        """→ (flags int32 [n, 4] = (sharpness, autocontrast, top, left), angles float32 [n]) — host tensors, drawn in the
        order the pipeline's transforms run (colour decisions first, or crop and angle first)"""
        g = self.generator
        ch, cw = self.crop if self.crop is not None else (H, W)
        if ch > H or cw > W:
            raise PfrError(f"DeviceAugmentation: crop {ch}x{cw} larger than the {H}x{W} input")
        flags = torch.zeros((n, 4), dtype=torch.int32)

        def color():
            u = torch.rand((n, 2), generator=g)
            flags[:, 0] = (u[:, 0] < self.p_sharpness).int()
            flags[:, 1] = (u[:, 1] < self.p_autocontrast).int()

        if self.order == 'color_first':
            color()
        flags[:, 2] = torch.randint(0, H - ch + 1, (n,), generator=g).int()
        flags[:, 3] = torch.randint(0, W - cw + 1, (n,), generator=g).int()
        angles = torch.empty(n).uniform_(-self.degrees, self.degrees, generator=g) if self.degrees > 0 else torch.zeros(n)
        if self.order == 'geometry_first':
            color()
        return flags, angles

    def fit_apply(self, x, color_flags=None):
        """the fit stage alone: ragged dict on the GPU (+ int [N, 2] sharpness / autocontrast flags, 'resize' only) →
        uint8 [N, h, w, 3]"""
        if self.fit is None:
            raise PfrError("DeviceAugmentation: a ragged batch needs fit=('resize' | 'thumbnail_pad', (h, w))")
        if not is_ragged(x) or not x['data'].is_cuda or x['data'].dtype != torch.uint8 or x['data'].dim() != 1:
            raise PfrError("DeviceAugmentation: expects the ragged dict {'data': uint8 [bytes], 'shape': int32 [N, 2]} with 'data' on the GPU")
        mode, (ch, cw) = self.fit
        data = x['data'].contiguous()
        host = x.get('shape_host')      # the collate's host copy: no device round trip in front of the planning
        shape = np.asarray(host if host is not None else x['shape'].cpu().numpy()).astype(np.int32).reshape(-1, 2)
        N = shape.shape[0]
        off, total = ragged_offsets(shape)
        if total > data.numel():
            raise PfrError(f"DeviceAugmentation: 'shape' describes {total} bytes, 'data' holds {data.numel()}")
        rec, coeffs = fit_params(mode, shape, (ch, cw))
        if color_flags is not None:
            cf = np.asarray(torch.as_tensor(color_flags).numpy(), dtype=np.int32).reshape(N, 2)
            if mode != 'resize' and cf.any():
                raise PfrError("DeviceAugmentation: colour flags in the fit stage are for fit='resize' only")
            rec[:, _R_SHARP], rec[:, _R_CONTRAST] = cf[:, 0], cf[:, 1]
        dev = data.device
        rec_d = torch.from_numpy(rec).pin_memory().to(dev, non_blocking=True)
        coeffs_d = torch.from_numpy(coeffs).pin_memory().to(dev, non_blocking=True)
        off_d = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
        need = lib.pfr_augment_fit_ws_bytes(data.numel(), N)
        if self._fit_ws is None or self._fit_ws.numel() < need or self._fit_ws.device != dev:
            self._fit_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty((N, ch, cw, 3), dtype=torch.uint8, device=dev)
        lib.pfr_augment_fit(data.data_ptr(), off_d.data_ptr(), rec_d.data_ptr(), coeffs_d.data_ptr(), N, ch, cw, out.data_ptr(),
                            self._fit_ws.data_ptr(), _stream())
        return out

    def apply(self, x, flags, angles):
        """x uint8 [N, H, W, 3] on the GPU, or the ragged dict when the pipeline has a fit stage; flags / angles as `draw`
        returns them → float32 [N, 3, out_h, out_w]"""
        if is_ragged(x):
            f = torch.as_tensor(flags).clone().reshape(-1, 4)
            if self.order == 'color_first':
                # simple family: sharpness / autocontrast act on the raw frame, inside the fit stage
                x = self.fit_apply(x, f[:, :2])
                f[:, :2] = 0
            else:
                x = self.fit_apply(x)
            flags = f
        if not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
            raise PfrError("DeviceAugmentation: expects a uint8 [N, H, W, 3] CUDA batch")
        x = x.contiguous()
        N, H, W, _ = x.shape
        ch, cw = self.crop if self.crop is not None else (H, W)
        oh, ow = self.size if self.size is not None else (ch, cw)
        flags = np.ascontiguousarray(torch.as_tensor(flags).numpy(), dtype=np.int32).reshape(N, 4)
        angles = np.ascontiguousarray(torch.as_tensor(angles).numpy(), dtype=np.float32).reshape(N)
        if (flags[:, 2] < 0).any() or (flags[:, 2] + ch > H).any() or (flags[:, 3] < 0).any() or (flags[:, 3] + cw > W).any():
            raise PfrError("DeviceAugmentation: crop window outside the image")
        rec = torch.empty((N, _REC), dtype=torch.int32).pin_memory()
        lib.pfr_augment_params(flags.ctypes.data, angles.ctypes.data, N, ow, oh, rec.data_ptr())
        rec_d = rec.to(x.device, non_blocking=True)
        geo = self.order == 'geometry_first'
        need = lib.pfr_augment_geo_ws_bytes(N, oh, ow) if geo else lib.pfr_augment_ws_bytes(N, H, W)
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        y = torch.empty((N, 3, oh, ow), dtype=torch.float32, device=x.device)
        train = lib.pfr_augment_train_geo if geo else lib.pfr_augment_train
        train(x.data_ptr(), N, H, W, ch, cw, oh, ow, rec_d.data_ptr(), y.data_ptr(), self._ws.data_ptr(), _stream())
        return y

    def __call__(self, x):
        if is_ragged(x):
            if self.fit is None:
                raise PfrError("DeviceAugmentation: a ragged batch needs fit=('resize' | 'thumbnail_pad', (h, w))")
            n, (H, W) = x['shape'].shape[0], self.fit[1]
        else:
            n, H, W = x.shape[0], x.shape[1], x.shape[2]
        flags, angles = self.draw(n, H, W)
        return self.apply(x, flags, angles)


def train_augmentation(generator=None):
    """fe_dogs_config.py:17-26"""
    return DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, generator)


def val_augmentation(size=None):
    """fe_dogs_config.py:28-32 (ToTensor only; six of the ten FE configs add Resize((224, 224)))"""
    return DeviceAugmentation(None, size, 0.0, 0.0, 0.0)


def simple_train_augmentation(generator=None):
    """simple_fe_dog.py:17-26 (also simple_fe_cat, no_align_head_dog, no_align_head_cat): sharpness and autocontrast on the
    raw frame, Resize((224, 224)), RandomCrop(220), Resize(224), RandomRotation(5)"""
    return DeviceAugmentation((220, 220), (224, 224), 0.1, 0.3, 5.0, generator, fit=('resize', (224, 224)))


def simple_val_augmentation():
    """simple_fe_dog.py:27-31: Resize((224, 224)) → ToTensor"""
    return DeviceAugmentation(None, None, 0.0, 0.0, 0.0, fit=('resize', (224, 224)))


def body_train_augmentation(generator=None):
    """body_dog_fe.py:18-27 (also body_cat_fe): resize_with_padding to 256 x 256, RandomCrop(252), Resize(256),
    RandomRotation(5), then sharpness and autocontrast on the rotated image"""
    return DeviceAugmentation((252, 252), (256, 256), 0.1, 0.3, 5.0, generator, fit=('thumbnail_pad', (256, 256)), order='geometry_first')


def body_val_augmentation():
    """body_dog_fe.py:29-33: resize_with_padding → ToTensor"""
    return DeviceAugmentation(None, None, 0.0, 0.0, 0.0, fit=('thumbnail_pad', (256, 256)))
