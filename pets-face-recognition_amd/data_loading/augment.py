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

Four further transforms are keyword-only and off by default (csrc/pfr_augment_color.hip; torchvision's PIL-image semantics, i.e.
Pillow's arithmetic, bit for bit — tests/test_color_augment_gpu.py): `p_hflip` RandomHorizontalFlip, `color_jitter` ColorJitter
(brightness / contrast / saturation / hue in a per-sample random order), `p_grayscale` RandomGrayscale, `erasing` RandomErasing with a
constant or per-channel value.  Their positions are fixed:

    color_first (head), uniform frames:
        ToPILImage → flip → ColorJitter → grayscale → sharpness → autocontrast → crop → resize → rotate → ToTensor → erasing
    geometry_first (body):
        fit → flip → crop → resize → rotate → ColorJitter → grayscale → sharpness → autocontrast → ToTensor → erasing
    ragged color_first (simple): the colour ops act on the raw ragged frame inside the fit stage, which has no flip / jitter /
        grayscale: asking for one of them raises PfrError.  Erasing works in all three shapes.

`draw` keeps drawing what it drew; the new decisions come from `draw_extra` (which draws nothing when all four are off) and go to
`apply(..., extra=...)`.
"""
import ctypes
import math

import numpy as np
import torch

from .._hip import lib, PfrError
from .ragged import MAX_SIDE, is_ragged, ragged_offsets

_REC = 12
_FIT_REC = 32
_FIT_MODES = {'resize': 0, 'thumbnail_pad': 1}
_R_SHARP, _R_CONTRAST = 20, 21
_COLOR_REC = 12
_ERASE_REC = 8
_JITTER_OPS = ('brightness', 'contrast', 'saturation', 'hue')      # op ids 0..3 = torchvision's fn_idx


def _jitter_range(name, value):
    """torchvision ColorJitter._check_input → (lo, hi), or None when the op is off"""
    hue = name == 'hue'
    center, bound = (0.0, (-0.5, 0.5)) if hue else (1.0, (0.0, float('inf')))
    if value is None:
        return None
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        lo, hi = center - float(value), center + float(value)
        if not hue:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
    if not bound[0] <= lo <= hi <= bound[1]:
        raise ValueError(f"{name} values should be between {bound}, but got {(lo, hi)}.")
    return None if lo == hi == center else (lo, hi)


def _parse_jitter(cj):
    """dict or 4-tuple (brightness, contrast, saturation, hue) → [range or None] * 4"""
    if cj is None:
        return [None] * 4
    if isinstance(cj, dict):
        unknown = set(cj) - set(_JITTER_OPS)
        if unknown:
            raise ValueError(f"color_jitter: unknown keys {sorted(unknown)}")
        cj = [cj.get(k, 0) for k in _JITTER_OPS]
    if len(cj) != 4:
        raise ValueError("color_jitter must be a dict or (brightness, contrast, saturation, hue)")
    return [_jitter_range(k, v) for k, v in zip(_JITTER_OPS, cj)]


def _parse_erasing(er):
    """dict p / scale / ratio / value (torchvision RandomErasing's defaults) → (p, scale, ratio, value float32 [3]) or None"""
    if er is None:
        return None
    unknown = set(er) - {'p', 'scale', 'ratio', 'value'}
    if unknown:
        raise ValueError(f"erasing: unknown keys {sorted(unknown)}")
    p, scale, ratio, value = float(er.get('p', 0.5)), tuple(er.get('scale', (0.02, 0.33))), tuple(er.get('ratio', (0.3, 3.3))), er.get('value', 0)
    if isinstance(value, str):
        raise PfrError(f"DeviceAugmentation: erasing value={value!r} (normal noise) is not implemented; give a number or a per-channel 3-tuple")
    value = np.asarray(value, np.float32).reshape(-1)
    if value.size not in (1, 3):
        raise ValueError("erasing: value must be a number or a per-channel 3-tuple")
    if not 0.0 <= p <= 1.0:
        raise ValueError("erasing: p must be in [0, 1]")
    if len(scale) != 2 or len(ratio) != 2 or not 0.0 <= scale[0] <= scale[1] <= 1.0 or not 0.0 < ratio[0] <= ratio[1]:
        raise ValueError("erasing: scale must be 0 <= lo <= hi <= 1 and ratio 0 < lo <= hi")
    return (p, (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1])), np.ascontiguousarray(np.broadcast_to(value, (3,)), np.float32)) if p > 0 else None


def color_records(flip, gray, order, factors, hue, ops_mask):
    """host part of the colour pre-pass (no device work): per-sample decisions → (records int32 [N, 12], launch mask)"""
    flip = np.ascontiguousarray(flip, np.int32).reshape(-1)
    n = flip.shape[0]
    gray = np.ascontiguousarray(gray, np.int32).reshape(n)
    order = np.ascontiguousarray(order, np.int32).reshape(n, 4)
    factors = np.ascontiguousarray(factors, np.float32).reshape(n, 3)
    hue = np.ascontiguousarray(hue, np.float32).reshape(n)
    rec, mask = np.zeros((n, _COLOR_REC), np.int32), np.zeros(1, np.int32)
    lib.pfr_augment_color_params(flip.ctypes.data, gray.ctypes.data, order.ctypes.data, factors.ctypes.data, hue.ctypes.data, int(ops_mask),
                                 n, rec.ctypes.data, mask.ctypes.data)
    return rec, int(mask[0])


def erase_records(rects, value, H, W):
    """host part of the erasing (no device work): rects int [N, 5] = (erase, i, j, h, w) → (records int32 [N, 8], largest area)"""
    rects = np.ascontiguousarray(rects, np.int32).reshape(-1, 5)
    value = np.ascontiguousarray(np.broadcast_to(np.asarray(value, np.float32).reshape(-1), (3,)), np.float32)
    rec, area = np.zeros((rects.shape[0], _ERASE_REC), np.int32), np.zeros(1, np.int32)
    lib.pfr_augment_erase_params(rects.ctypes.data, value.ctypes.data, rects.shape[0], int(H), int(W), rec.ctypes.data, area.ctypes.data)
    return rec, int(area[0])


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
                 fit=None, order='color_first', p_hflip=0.0, color_jitter=None, p_grayscale=0.0, erasing=None):
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
        self.p_hflip, self.p_grayscale = float(p_hflip), float(p_grayscale)
        if not (0.0 <= self.p_hflip <= 1.0 and 0.0 <= self.p_grayscale <= 1.0):
            raise ValueError("DeviceAugmentation: p_hflip and p_grayscale must be in [0, 1]")
        self.jitter = _parse_jitter(color_jitter)                     # [range or None] * 4: brightness, contrast, saturation, hue
        self.ops_mask = sum(1 << k for k, r in enumerate(self.jitter) if r is not None)
        self.erasing = _parse_erasing(erasing)
        if fit is not None and order == 'color_first' and (self.p_hflip > 0 or self.ops_mask or self.p_grayscale > 0):
            raise PfrError("DeviceAugmentation: flip / ColorJitter / grayscale are not available for ragged batches in the color_first order "
                           "(the colour ops of that pipeline act on the raw ragged frame inside the fit stage, which has none of them)")
        self._ws = None
        self._fit_ws = None
        self._color_ws = None

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

    def draw_extra(self, n, H, W):
        """decisions of the flip / ColorJitter / grayscale / erasing transforms for n frames of H x W, drawn in the order the
        transforms run → None when all four are off (nothing is drawn from the generator), else a dict of host tensors:
        'flip' int32 [n], 'order' int32 [n, 4] (a permutation of the op ids brightness 0, contrast 1, saturation 2, hue 3),
        'factors' float32 [n, 3], 'hue' float32 [n], 'gray' int32 [n], 'erase' int32 [n, 5] = (erase, i, j, h, w) in the OUTPUT image"""
        if not (self.p_hflip > 0 or self.ops_mask or self.p_grayscale > 0 or self.erasing is not None):
            return None
        g = self.generator
        e = {'flip': torch.zeros(n, dtype=torch.int32), 'order': torch.arange(4, dtype=torch.int32).repeat(n, 1),
             'factors': torch.ones((n, 3)), 'hue': torch.zeros(n), 'gray': torch.zeros(n, dtype=torch.int32),
             'erase': torch.zeros((n, 5), dtype=torch.int32)}
        if self.p_hflip > 0:
            e['flip'] = (torch.rand(n, generator=g) < self.p_hflip).int()
        if self.ops_mask:
            # ColorJitter.get_params: randperm(4), then a uniform factor for every op that is on
            e['order'] = torch.argsort(torch.rand((n, 4), generator=g), dim=1).int()
            for k, r in enumerate(self.jitter):
                if r is not None:
                    u = torch.empty(n).uniform_(r[0], r[1], generator=g)
                    if k < 3:
                        e['factors'][:, k] = u
                    else:
                        e['hue'] = u
        if self.p_grayscale > 0:
            e['gray'] = (torch.rand(n, generator=g) < self.p_grayscale).int()
        if self.erasing is not None:
            # RandomErasing.get_params on the tensor ToTensor returns: up to 10 attempts, the first rectangle that fits wins
            p, scale, ratio, _ = self.erasing
            ch, cw = self.crop if self.crop is not None else (H, W)
            oh, ow = self.size if self.size is not None else (ch, cw)
            on = torch.rand(n, generator=g) < p
            area = oh * ow * torch.empty((n, 10)).uniform_(scale[0], scale[1], generator=g)
            log_ratio = torch.log(torch.tensor(ratio))
            aspect = torch.exp(torch.empty((n, 10)).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=g))
            h, w = torch.round(torch.sqrt(area * aspect)).long(), torch.round(torch.sqrt(area / aspect)).long()
            ok = (h < oh) & (w < ow)
            first = torch.argmax(ok.int(), dim=1, keepdim=True)
            h, w = h.gather(1, first)[:, 0], w.gather(1, first)[:, 0]
            u = torch.rand((n, 2), generator=g)
            i = torch.minimum((u[:, 0] * (oh - h + 1)).long(), oh - h)
            j = torch.minimum((u[:, 1] * (ow - w + 1)).long(), ow - w)
            on = on & ok.any(dim=1) & (h > 0) & (w > 0)
            e['erase'] = (torch.stack([torch.ones_like(h), i, j, h, w], dim=1) * on[:, None]).int()
        return e

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

    def apply(self, x, flags, angles, extra=None):
        """x uint8 [N, H, W, 3] on the GPU, or the ragged dict when the pipeline has a fit stage; flags / angles as `draw`
        returns them; extra as `draw_extra` returns it (None: none of the four further transforms) → float32 [N, 3, out_h, out_w]"""
        crec, cmask, rects = None, 0, None
        if extra is not None:
            n = len(extra['flip'])
            crec, cmask = color_records(extra['flip'], extra['gray'], extra['order'], extra['factors'], extra['hue'], self.ops_mask)
            rects = np.ascontiguousarray(torch.as_tensor(extra['erase']).numpy(), dtype=np.int32).reshape(n, 5)
            if not rects[:, 0].any():
                rects = None
            if cmask and is_ragged(x) and self.order == 'color_first':
                raise PfrError("DeviceAugmentation: flip / ColorJitter / grayscale are not available for ragged batches in the color_first order")
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
        if cmask:
            if crec.shape[0] != N:
                raise PfrError(f"DeviceAugmentation: extra holds decisions for {crec.shape[0]} samples, the batch has {N}")
            crec_d = torch.from_numpy(crec).pin_memory().to(x.device, non_blocking=True)
        if cmask and not geo:
            # flip → ColorJitter → grayscale into a workspace copy, which the kernels below read as their input
            need = N * H * W * 3 + lib.pfr_augment_color_ws_bytes(N)
            if self._color_ws is None or self._color_ws.numel() < need or self._color_ws.device != x.device:
                self._color_ws = torch.empty(need, dtype=torch.uint8, device=x.device)
            sums = self._color_ws.data_ptr()
            pre = sums + lib.pfr_augment_color_ws_bytes(N)
            lib.pfr_augment_color(x.data_ptr(), N, H, W, crec_d.data_ptr(), cmask, pre, sums, _stream())
            src = pre
        else:
            src = x.data_ptr()
        if geo:
            need = lib.pfr_augment_geo_color_ws_bytes(N, H, W, oh, ow, cmask) if cmask else lib.pfr_augment_geo_ws_bytes(N, oh, ow)
        else:
            need = lib.pfr_augment_ws_bytes(N, H, W)
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        y = torch.empty((N, 3, oh, ow), dtype=torch.float32, device=x.device)
        if geo and cmask:
            lib.pfr_augment_train_geo_color(src, N, H, W, ch, cw, oh, ow, rec_d.data_ptr(), crec_d.data_ptr(), cmask, y.data_ptr(),
                                            self._ws.data_ptr(), _stream())
        else:
            train = lib.pfr_augment_train_geo if geo else lib.pfr_augment_train
            train(src, N, H, W, ch, cw, oh, ow, rec_d.data_ptr(), y.data_ptr(), self._ws.data_ptr(), _stream())
        if rects is not None:
            if rects.shape[0] != N:
                raise PfrError(f"DeviceAugmentation: extra holds decisions for {rects.shape[0]} samples, the batch has {N}")
            value = self.erasing[3] if self.erasing is not None else np.zeros(3, np.float32)
            erec, area = erase_records(rects, value, oh, ow)
            erec_d = torch.from_numpy(erec).pin_memory().to(x.device, non_blocking=True)
            lib.pfr_augment_erase(y.data_ptr(), N, oh, ow, erec_d.data_ptr(), area, _stream())
        return y

    def __call__(self, x):
        if is_ragged(x):
            if self.fit is None:
                raise PfrError("DeviceAugmentation: a ragged batch needs fit=('resize' | 'thumbnail_pad', (h, w))")
            n, (H, W) = x['shape'].shape[0], self.fit[1]
        else:
            n, H, W = x.shape[0], x.shape[1], x.shape[2]
        flags, angles = self.draw(n, H, W)
        return self.apply(x, flags, angles, self.draw_extra(n, H, W))


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
