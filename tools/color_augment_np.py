"""numpy restatement of the colour / flip / erasing transforms the device pipeline adds (csrc/pfr_augment_color.hip), in Pillow's
arithmetic.  TEST INFRASTRUCTURE ONLY: tests/test_color_augment_host.py pins every function below against the Pillow-produced
tests/golden/color_augment.npz (tools/make_color_augment_golden.py) and, where Pillow imports, against live Pillow (the two HSV
conversions over all 2^24 colours); tests/test_color_augment_gpu.py then compares the device against this file.

On PIL images torchvision's transforms are thin calls into Pillow (torchvision/transforms/_functional_pil.py):
    hflip(img)                  = img.transpose(FLIP_LEFT_RIGHT)
    adjust_brightness(img, f)   = ImageEnhance.Brightness(img).enhance(f) = Image.blend(black, img, f)
    adjust_contrast(img, f)     = ImageEnhance.Contrast(img).enhance(f)   = Image.blend(solid grey of int(mean(L) + 0.5), img, f)
    adjust_saturation(img, f)   = ImageEnhance.Color(img).enhance(f)      = Image.blend(L on three channels, img, f)
    adjust_hue(img, h)          = convert('HSV'), H += uint8(h * 255) (wrapping), convert('RGB')
    rgb_to_grayscale(img, 3)    = convert('L') on three channels
    erase(tensor, i, j, h, w, v)  tensor[..., i:i+h, j:j+w] = v           (on the float tensor after ToTensor)
Blend.c: temp = (float)(d + alpha * (i - d)) in float32 (d, i ints; alpha float32); alpha in [0, 1] → (UINT8)temp, else clip to
[0, 255] and truncate.  Convert.c: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; rgb2hsv / hsv2rgb follow colorsys in mixed
float / double arithmetic with truncation (rgb → hsv) or round-half-away (hsv → rgb) to bytes.
"""
import numpy as np

OPS = ('brightness', 'contrast', 'saturation', 'hue')      # ids 0..3 = torchvision's fn_idx in ColorJitter.forward


def hflip(img):
    return np.ascontiguousarray(img[:, ::-1])


def luma(img):
    """convert('L') of an RGB uint8 image [..., 3] → uint8 [...]"""
    a = img.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def grayscale(img):
    return np.repeat(luma(img)[..., None], 3, axis=-1)


def blend(deg, img, factor):
    """Image.blend(deg, img, factor): deg, img uint8 (broadcastable), factor a Python float (cast to float32 as _imaging.c does)"""
    f = np.float32(factor)
    d = deg.astype(np.float32)
    t = d + f * (img.astype(np.float32) - d)        # float32: the product is rounded before the add
    if not (0.0 <= f <= 1.0):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)      # truncation toward zero


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast_mean(img):
    """int(ImageStat.Stat(img.convert('L')).mean[0] + 0.5): integer sum, double division"""
    lum = luma(img)
    return int(float(int(lum.astype(np.int64).sum())) / float(lum.size) + 0.5)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(grayscale(img), img, f)


def rgb2hsv(img):
    """Convert.c rgb2hsv_row; img uint8 [..., 3] → uint8 [..., 3]"""
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc = np.maximum(r, np.maximum(g, b))
    minc = np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    mx = np.where(grey, 1, maxc).astype(np.float32)
    s = cr / mx                                             # float32
    rc = (maxc - r).astype(np.float32) / cr
    gc = (maxc - g).astype(np.float32) / cr
    bc = (maxc - b).astype(np.float32) / cr
    rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == maxc, (bc - gc).astype(np.float64),                      # float - float in float32
                 np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64))   # the literals are doubles
    h = h.astype(np.float32).astype(np.float64)                                # `float h`
    h = np.fmod(h / 6.0 + 1.0, 1.0).astype(np.float32).astype(np.float64)
    uh = np.clip((h * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _cround(x):
    """C round(): half away from zero (the operands here are never negative)"""
    return np.floor(x + 0.5).astype(np.int32)


def hsv2rgb(img):
    """Convert.c hsv2rgb; img uint8 [..., 3] → uint8 [..., 3]"""
    h, s, v = (img[..., c] for c in range(3))
    hf = h.astype(np.float32).astype(np.float64)
    h6 = hf * 6.0 / 255.0
    i = np.floor(h6).astype(np.int32)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    fs = (s.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    vf = v.astype(np.float32).astype(np.float64)
    p = np.clip(_cround(vf * (1.0 - fs)), 0, 255)
    q = np.clip(_cround(vf * (1.0 - fs * f)), 0, 255)
    t = np.clip(_cround(vf * (1.0 - fs * (1.0 - f))), 0, 255)
    vi = v.astype(np.int32)
    k = i % 6
    r = np.choose(k, [vi, q, p, p, t, vi])
    g = np.choose(k, [t, vi, vi, q, p, p])
    b = np.choose(k, [p, p, t, vi, vi, q])
    grey = s == 0
    out = np.stack([np.where(grey, vi, r), np.where(grey, vi, g), np.where(grey, vi, b)], axis=-1)
    return out.astype(np.uint8)


def hue_shift_byte(hue):
    """np.array(hue * 255).astype(np.uint8) of torchvision's adjust_hue: truncation toward zero, then the low byte"""
    return int(float(hue) * 255.0) & 255


def hue(img, shift):
    """shift: the byte `hue_shift_byte` gives (the HSV round trip runs, and loses bits, for a zero shift too)"""
    hsv = rgb2hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv2rgb(hsv)


def jitter(img, order, factors, shift):
    """ColorJitter.forward with fixed decisions: order = op ids in the order they run (an op that is off is left out or < 0),
    factors = (brightness, contrast, saturation) floats, shift = hue byte"""
    for op in order:
        op = int(op)
        if op == 0:
            img = brightness(img, factors[0])
        elif op == 1:
            img = contrast(img, factors[1])
        elif op == 2:
            img = saturation(img, factors[2])
        elif op == 3:
            img = hue(img, shift)
    return img


def color_pass(img, flip=False, order=(), factors=(1.0, 1.0, 1.0), shift=0, gray=False):
    """flip → ColorJitter → grayscale on one uint8 [H, W, 3] frame"""
    if flip:
        img = hflip(img)
    img = jitter(img, order, factors, shift)
    if gray:
        img = grayscale(img)
    return img


def erase(y, i, j, h, w, value):
    """F.erase on a float32 [3, H, W] tensor (numpy); value a number or a per-channel 3-tuple; h = 0 or w = 0: no erase"""
    y = y.copy()
    v = np.broadcast_to(np.asarray(value, np.float32).reshape(-1), (3,)) if np.ndim(value) else np.full(3, value, np.float32)
    if h > 0 and w > 0:
        y[:, i:i + h, j:j + w] = v[:, None, None]
    return y
