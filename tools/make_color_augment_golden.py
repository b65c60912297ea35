"""Writes tests/golden/color_augment.npz: outputs of the real Pillow calls torchvision's PIL-image transforms make for horizontal
flip, ColorJitter (each op alone and four fixed orders), grayscale, and two whole pipelines with every op on, on seeded images with
FIXED decisions.  tests/test_color_augment_host.py pins the numpy restatement (tools/color_augment_np.py) to this file without
Pillow; tests/test_color_augment_gpu.py pins the device to it.  Needs Pillow (12.2 wrote the committed file).

    python tools/make_color_augment_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "color_augment.npz")

FACTORS = (0.0, 1.0, 0.37, 1.73)                   # 0, 1, inside (0, 1), above 1
HUES = (0.0, 0.02, -0.02, 0.5, -0.5)
ORDERS = ((1, 0, 2, 3), (0, 2, 3, 1), (3, 1, 0, 2), (2, 3, 1, 0))      # contrast first, contrast last, two mixed
ORDER_FACTORS = (1.2, 0.8, 1.73)                   # brightness, contrast, saturation
ORDER_HUE = -0.02
ENHANCE = (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)


def seeded_image(seed, h, w):
    """low-frequency colour field + noise, so that hue / saturation see real chroma and the mean is not 127"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([96 + 80 * np.sin(xx / 9.0 + seed), 128 + 100 * np.cos(yy / 7.0), 60 + 1.5 * (xx + yy)], -1)
    return np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def f32(v):
    """the factor as torchvision hands it to Pillow: a float32 draw's .item()"""
    return float(np.float32(v))


def pil_hue(img, hue):
    """torchvision _functional_pil.adjust_hue"""
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.array(hue * 255).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pil_gray(img):
    """torchvision _functional_pil.to_grayscale(img, 3)"""
    g = np.array(img.convert("L"), dtype=np.uint8)
    return Image.fromarray(np.dstack([g, g, g]), "RGB")


def pil_jitter(img, order, factors, hue):
    for op in order:
        img = pil_hue(img, hue) if op == 3 else ENHANCE[op](img).enhance(factors[op])
    return img


def pil_pipeline(arr, d, crop, out, geometry_first):
    """one frame through the whole pipeline with the decisions d → the uint8 image in front of ToTensor"""
    img = Image.fromarray(arr, "RGB")

    def color(im):
        im = pil_jitter(im, d["order"], d["factors"], d["hue"])
        if d["gray"]:
            im = pil_gray(im)
        if d["sharp"]:
            im = ImageEnhance.Sharpness(im).enhance(0)
        if d["contrast"]:
            im = ImageOps.autocontrast(im)
        return im

    def geometry(im):
        im = im.crop((d["left"], d["top"], d["left"] + crop, d["top"] + crop))
        im = im.resize((out, out), Image.BILINEAR)
        return im.rotate(d["angle"], Image.NEAREST, expand=False, center=None, fillcolor=(0, 0, 0))

    if d["flip"]:
        img = ImageOps.mirror(img)
    img = color(geometry(img)) if geometry_first else geometry(color(img))
    return np.asarray(img)


def pipeline_case(z, tag, seed, n, size, crop, out, geometry_first):
    rng = np.random.default_rng(seed)
    x = np.stack([seeded_image(seed + i, size, size) for i in range(n)])
    dec = np.zeros((n, 12), np.float64)       # flip gray sharp contrast top left angle hue | factors[3] | erase on
    order = np.zeros((n, 4), np.int32)
    erase = np.zeros((n, 5), np.int32)
    y = np.zeros((n, out, out, 3), np.uint8)
    for i in range(n):
        d = dict(flip=(i + 1) % 2, gray=int(i % 4 == 3), sharp=int(i % 2 == 0), contrast=int(i % 3 != 1),
                 top=int(rng.integers(0, size - crop + 1)), left=int(rng.integers(0, size - crop + 1)),
                 angle=f32(rng.uniform(-5, 5)), hue=f32(rng.uniform(-0.02, 0.02)),
                 factors=[f32(rng.uniform(0.8, 1.2)) for _ in range(3)], order=[int(v) for v in rng.permutation(4)])
        if n == 1:
            d["flip"], d["sharp"], d["contrast"] = 1, 1, 1
        y[i] = pil_pipeline(x[i], d, crop, out, geometry_first)
        dec[i, :8] = (d["flip"], d["gray"], d["sharp"], d["contrast"], d["top"], d["left"], d["angle"], d["hue"])
        dec[i, 8:11] = d["factors"]
        order[i] = d["order"]
        h, w = int(rng.integers(1, out // 2)), int(rng.integers(1, out // 2))
        erase[i] = (i % 2 == 0 or n == 1, int(rng.integers(0, out - h + 1)), int(rng.integers(0, out - w + 1)), h, w)
    z.update({f"{tag}_x": x, f"{tag}_dec": dec, f"{tag}_order": order, f"{tag}_erase": erase, f"{tag}_y": y,
              f"{tag}_geom": np.array([size, crop, out, int(geometry_first)], np.int32)})


def main():
    z = {"factors": np.array(FACTORS, np.float32), "hues": np.array(HUES, np.float32), "orders": np.array(ORDERS, np.int32),
         "order_factors": np.array(ORDER_FACTORS, np.float32), "order_hue": np.array(ORDER_HUE, np.float32)}
    a, b = seeded_image(1, 61, 47), seeded_image(2, 48, 52)
    z["a"], z["b"] = a, b
    pa, pb = Image.fromarray(a, "RGB"), Image.fromarray(b, "RGB")
    for op, E in enumerate(ENHANCE):
        z[f"a_op{op}"] = np.stack([np.asarray(E(pa).enhance(f32(f))) for f in FACTORS])
    z["a_op3"] = np.stack([np.asarray(pil_hue(pa, f32(h))) for h in HUES])
    z["a_flip"], z["b_flip"] = np.asarray(ImageOps.mirror(pa)), np.asarray(ImageOps.mirror(pb))
    z["a_gray"], z["b_gray"] = np.asarray(pil_gray(pa)), np.asarray(pil_gray(pb))
    z["a_luma"] = np.asarray(pa.convert("L"))
    z["b_orders"] = np.stack([np.asarray(pil_jitter(pb, o, [f32(f) for f in ORDER_FACTORS], f32(ORDER_HUE))) for o in ORDERS])
    pipeline_case(z, "head", 10, 1, 224, 220, 224, False)
    pipeline_case(z, "body", 20, 4, 64, 60, 64, True)
    np.savez_compressed(OUT, **z)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(z)} arrays")


if __name__ == "__main__":
    main()
