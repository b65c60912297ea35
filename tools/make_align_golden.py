"""Writes tests/golden/align.npz: Pillow's Image.transform((w, h), PERSPECTIVE, coeffs, BILINEAR) on the small versions of the cases of
tests/test_align_host.py (frames <= 64 x 64, outputs 32 x 32), so that the comparison of the alignment contract with an independent
implementation also runs where Pillow is absent.  Needs Pillow.   python tools/make_align_golden.py"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_oracle as AO   # noqa: E402


def pillow_warp(frame, minv, oh, ow):
    return np.asarray(Image.fromarray(frame).transform((ow, oh), Image.PERSPECTIVE, AO.pillow_coeffs(minv), Image.BILINEAR))


if __name__ == "__main__":
    out = {}
    for k, seed in enumerate(AO.PILLOW_SEEDS):
        frame, pts, base, (oh, ow) = AO.pillow_case(seed, small=True)
        minv, valid = AO.solve(pts, base)
        assert valid
        out[f"frame{k}"], out[f"pts{k}"], out[f"base{k}"], out[f"minv{k}"] = frame, pts, base, minv
        out[f"pillow{k}"] = pillow_warp(frame, minv, oh, ow)
    import PIL
    out["pillow_version"] = np.array(PIL.__version__)
    path = os.path.join(ROOT, "tests", "golden", "align.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
