"""Builds tests/golden/ragged_augment.npz: the fit stage (ragged frames → uniform canvas) and the geometry-first train
order of data_loading/augment.py, executed with the installed PILLOW (12.2.0, the pin of oracle/augment_ref.py).

    python tools/make_ragged_golden.py

Only seeds, shapes, decisions and expected outputs are stored; the tests regenerate the input frames with
data_loading.ragged.seeded_frame.  Pillow does not expose its size / box / coefficient arithmetic, so this file restates
it in numpy (`plan`, `coeffs`, `reduce_box_average`, `resample`); every restated result is asserted against Pillow's
pixels below before anything is written, and the stored plans and coefficient-table digests come from that checked
restatement.  `resize_with_padding` is the body configs' Lambda: Image.thumbnail to the canvas, then a centred zero pad.
"""
import hashlib
import math
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pets_face_recognition_amd.data_loading.ragged import seeded_frame  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ragged_augment.npz")
PREC = 32 - 8 - 2
RESIZE, THUMBNAIL_PAD = 0, 1
f32 = np.float32


# ------------------------------------------------------------------------------------------- Pillow pipelines
def pil_resize_with_padding(img, canvas_h, canvas_w):
    """thumbnail (BICUBIC, reducing_gap 2.0) to at most canvas_w x canvas_h, then pad to the canvas with zeros:
    floor(delta / 2) on the left / top, the rest on the right / bottom"""
    img = img.copy()
    img.thumbnail((canvas_w, canvas_h))
    dw, dh = canvas_w - img.size[0], canvas_h - img.size[1]
    return ImageOps.expand(img, (dw // 2, dh // 2, dw - dw // 2, dh - dh // 2))


def pil_fit(frame, mode, canvas_h, canvas_w, sharp=0, contrast=0):
    img = Image.fromarray(frame)
    if mode == THUMBNAIL_PAD:
        return np.asarray(pil_resize_with_padding(img, canvas_h, canvas_w))
    if sharp:
        img = ImageEnhance.Sharpness(img).enhance(0)
    if contrast:
        img = ImageOps.autocontrast(img)
    return np.asarray(img.resize((canvas_w, canvas_h), Image.BILINEAR))


def pil_train(canvas, top, left, crop, size, angle, sharp, contrast, order):
    """the tail of the train Compose on a uniform uint8 canvas; order 'color_first' (head / simple family) or
    'geometry_first' (body family: sharpness and autocontrast see the rotated image)"""
    img = Image.fromarray(canvas)
    if order == 'color_first':
        if sharp:
            img = ImageEnhance.Sharpness(img).enhance(0)
        if contrast:
            img = ImageOps.autocontrast(img)
    img = img.crop((left, top, left + crop, top + crop))
    img = img.resize((size, size), Image.BILINEAR)
    img = img.rotate(float(angle), Image.NEAREST, expand=False, center=None, fillcolor=(0, 0, 0))
    if order == 'geometry_first':
        if sharp:
            img = ImageEnhance.Sharpness(img).enhance(0)
        if contrast:
            img = ImageOps.autocontrast(img)
    return np.asarray(img)


# ------------------------------------------------------------------------------------------- restatement
def plan(mode, H, W, canvas_h, canvas_w):
    """sizes, reduce factors, boxes and pad offsets of one frame, in Pillow's own double arithmetic"""
    p = dict(fx=1, fy=1, rbox=(0, 0, W, H), rw=W, rh=H, pad_l=0, pad_t=0)
    if mode == RESIZE:
        p.update(tw=canvas_w, th=canvas_h, box=(0.0, 0.0, float(W), float(H)))
    else:
        x, y = canvas_w, canvas_h
        if x >= W and y >= H:
            tw, th = W, H
        else:
            def round_aspect(number, key):
                return max(min(math.floor(number), math.ceil(number), key=key), 1)
            aspect = W / H
            if x / y >= aspect:
                x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
            else:
                y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
            tw, th = x, y
        box = (0.0, 0.0, float(W), float(H))
        if (tw, th) != (W, H):
            fx = int((box[2] - box[0]) / tw / 2.0) or 1
            fy = int((box[3] - box[1]) / th / 2.0) or 1
            if fx > 1 or fy > 1:
                sx, sy = 1.5 * ((box[2] - box[0]) / tw), 1.5 * ((box[3] - box[1]) / th)     # _get_safe_box, bicubic
                rb = (max(0, int(box[0] - sx)), max(0, int(box[1] - sy)), min(W, math.ceil(box[2] + sx)), min(H, math.ceil(box[3] + sy)))
                box = ((box[0] - rb[0]) / fx, (box[1] - rb[1]) / fy, (box[2] - rb[0]) / fx, (box[3] - rb[1]) / fy)
                p.update(fx=fx, fy=fy, rbox=rb, rw=(rb[2] - rb[0] + fx - 1) // fx, rh=(rb[3] - rb[1] + fy - 1) // fy)
        p.update(tw=tw, th=th, box=box, pad_l=(canvas_w - tw) // 2, pad_t=(canvas_h - th) // 2)
    b = tuple(f32(v) for v in p['box'])                     # the C resize parses the box as four floats
    p['box'] = b
    p['need_h'] = int(p['tw'] != p['rw'] or b[0] != 0 or b[2] != p['tw'])
    p['need_v'] = int(p['th'] != p['rh'] or b[1] != 0 or b[3] != p['th'])
    return p


def _box_mean(ss, n):
    """Reduce.c: (sum + n / 2) / n through a 24-bit reciprocal computed in float32, (UINT32)(2^24 / n) (the 1x2, 2x1, 2x2 and
    4x4 kernels shift instead, which gives the same value because the reciprocal of a power of two is exact)"""
    mult = int(f32(1 << 24) / f32(n))
    return ((ss + n // 2) * mult) >> 24


def reduce_box_average(img, fx, fy, rbox):
    x0, y0, x1, y1 = rbox
    a = img[y0:y1, x0:x1].astype(np.int64)
    H, W = a.shape[:2]
    ow, oh = (W + fx - 1) // fx, (H + fy - 1) // fy
    out = np.zeros((oh, ow, 3), np.uint8)
    for oy in range(oh):
        ny = min(fy, H - oy * fy)
        for ox in range(ow):
            nx = min(fx, W - ox * fx)
            ss = a[oy * fy:oy * fy + ny, ox * fx:ox * fx + nx].sum((0, 1))
            out[oy, ox] = _box_mean(ss, nx * ny)
    return out


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, in0, in1, out_size, bicubic, need):
    """Resample.c precompute_coeffs + normalize_coeffs_8bpc over the box (in0, in1) (float32); a pass Pillow skips
    (`need` false) is the identity table.  → int32 [out, 2 + ksize] rows (first tap, taps, k...)"""
    if not need:
        tab = np.zeros((out_size, 3), np.int32)
        tab[:, 0], tab[:, 1], tab[:, 2] = np.arange(out_size), 1, 1 << PREC
        return tab
    filt, sup = (_bicubic, 2.0) if bicubic else (_bilinear, 1.0)
    scale = float(f32(in1) - f32(in0)) / out_size
    filterscale = max(scale, 1.0)
    support = sup * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    tab = np.zeros((out_size, 2 + ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = float(in0) + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        tab[xx, 0], tab[xx, 1] = xmin, xmax
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            tab[xx, 2 + x] = int(-0.5 + k * (1 << PREC)) if k < 0 else int(0.5 + k * (1 << PREC))
    return tab


def _pass(img, tab):
    out = np.empty((tab.shape[0],) + img.shape[1:], np.uint8)
    a = img.astype(np.int64)
    for yy in range(tab.shape[0]):
        acc = np.full(img.shape[1:], 1 << (PREC - 1), np.int64)
        for t in range(tab[yy, 1]):
            acc += a[tab[yy, 0] + t] * int(tab[yy, 2 + t])
        out[yy] = np.clip(acc >> PREC, 0, 255)
    return out


def restated_fit(frame, mode, canvas_h, canvas_w):
    """(plan, table x, table y, canvas) of one frame without the pre-ops"""
    H, W = frame.shape[:2]
    p = plan(mode, H, W, canvas_h, canvas_w)
    img = frame
    if (p['fx'], p['fy']) != (1, 1):
        img = reduce_box_average(img, p['fx'], p['fy'], p['rbox'])
    assert img.shape[:2] == (p['rh'], p['rw'])
    tx = coeffs(p['rw'], p['box'][0], p['box'][2], p['tw'], mode == THUMBNAIL_PAD, p['need_h'])
    ty = coeffs(p['rh'], p['box'][1], p['box'][3], p['th'], mode == THUMBNAIL_PAD, p['need_v'])
    img = _pass(img.transpose(1, 0, 2), tx).transpose(1, 0, 2)
    img = _pass(img, ty)
    out = np.zeros((canvas_h, canvas_w, 3), np.uint8)
    out[p['pad_t']:p['pad_t'] + p['th'], p['pad_l']:p['pad_l'] + p['tw']] = img
    return p, tx, ty, out


def digest(tab):
    return hashlib.sha256(np.ascontiguousarray(tab, dtype='<i4').tobytes()).hexdigest()


PLAN_COLS = ('tw', 'th', 'fx', 'fy', 'rb0', 'rb1', 'rb2', 'rb3', 'pad_l', 'pad_t', 'rw', 'rh', 'ksx', 'ksy', 'need_h', 'need_v')


def fit_group(out, tag, mode, canvas, cases):
    """cases: (seed, H, W, sharp, contrast).  Runs Pillow, checks the restatement against it, stores the group."""
    ch, cw = canvas
    plans, boxes, hashes, outs = [], [], [], []
    for seed, H, W, sharp, contrast in cases:
        frame = seeded_frame(seed, H, W)
        want = pil_fit(frame, mode, ch, cw, sharp, contrast)
        pre = frame
        if sharp:
            pre = np.asarray(ImageEnhance.Sharpness(Image.fromarray(pre)).enhance(0))
        if contrast:
            pre = np.asarray(ImageOps.autocontrast(Image.fromarray(pre)))
        p, tx, ty, got = restated_fit(pre, mode, ch, cw)
        assert np.array_equal(got, want), (tag, seed, H, W, p)
        plans.append([p['tw'], p['th'], p['fx'], p['fy'], *p['rbox'], p['pad_l'], p['pad_t'], p['rw'], p['rh'],
                      tx.shape[1] - 2, ty.shape[1] - 2, p['need_h'], p['need_v']])
        boxes.append(p['box'])
        hashes.append([digest(tx), digest(ty)])
        outs.append(want)
    out[f'{tag}_mode'] = np.int32(mode)
    out[f'{tag}_canvas'] = np.array(canvas, np.int32)
    out[f'{tag}_cases'] = np.array(cases, np.int32)
    out[f'{tag}_plan'] = np.array(plans, np.int32)
    out[f'{tag}_box'] = np.array(boxes, np.float32)
    out[f'{tag}_coefhash'] = np.array(hashes)
    out[f'{tag}_out'] = np.stack(outs)
    return np.array(plans, np.int32), np.stack(outs)


def train_group(out, tag, canvases, crop, size, order, seed, keep=8):
    """the train tail on the canvases of a fit group, with seeded decisions; the first `keep` results are stored in full,
    all of them as SHA-256 digests"""
    rs = np.random.RandomState(seed)
    n = canvases.shape[0]
    H, W = canvases.shape[1:3]
    dec = np.zeros((n, 4), np.int32)
    dec[:, 0], dec[:, 1] = rs.rand(n) < 0.4, rs.rand(n) < 0.5
    dec[:4, :2] = [(0, 0), (1, 0), (0, 1), (1, 1)]
    if order == 'none':
        dec[:, :2] = 0
    dec[:, 2], dec[:, 3] = rs.randint(0, H - crop + 1, n), rs.randint(0, W - crop + 1, n)
    angles = rs.uniform(-5, 5, n).astype(np.float32)
    angles[np.abs(angles) < 0.25] = 1.5
    res = [pil_train(canvases[i], dec[i, 2], dec[i, 3], crop, size, angles[i], dec[i, 0], dec[i, 1], order) for i in range(n)]
    out[f'{tag}_dec'], out[f'{tag}_angles'] = dec, angles
    out[f'{tag}_crop'], out[f'{tag}_size'] = np.int32(crop), np.int32(size)
    out[f'{tag}_out'] = np.stack(res[:keep])
    out[f'{tag}_sha'] = np.array([hashlib.sha256(r.tobytes()).hexdigest() for r in res])
    return dec


def main():
    out = {}
    rs = np.random.RandomState(2024)

    def bulk(n, lo, hi):
        cases = []
        for i in range(n):
            long_side = int(rs.randint(lo, hi + 1))
            short_side = int(rs.randint(max(lo, -(-long_side // 3)), long_side + 1))
            H, W = (long_side, short_side) if rs.randint(2) else (short_side, long_side)
            cases.append([1000 + i, H, W, int(rs.rand() < 0.35), int(rs.rand() < 0.45)])
        return cases

    # RESIZE to 48x48: 26 seeded frames (scale ratios of 64..1400 → 224) + hand-picked: equal to the canvas (both passes
    # skipped), one axis equal, up-scaling with every pre-op combination, down-scaling with every pre-op combination
    special_rs = [[1, 48, 48, 0, 0], [2, 48, 48, 1, 1], [3, 48, 130, 0, 1], [4, 97, 48, 1, 0],
                  [5, 20, 31, 0, 0], [6, 20, 31, 1, 0], [7, 33, 17, 0, 1], [8, 17, 40, 1, 1],
                  [9, 300, 211, 0, 0], [10, 300, 211, 1, 0], [11, 123, 290, 0, 1], [12, 251, 199, 1, 1]]
    rs48 = special_rs + [[s, h, w, a, b] for s, h, w, a, b in bulk(22, 14, 300)]
    _, c_rs = fit_group(out, 'rs48', RESIZE, (48, 48), rs48)
    # the val pipeline has no colour ops: Pillow's plain resize of ALL rs48 frames, as digests
    out['rs48_plain_sha'] = np.array([hashlib.sha256(pil_fit(seeded_frame(s, h, w), RESIZE, 48, 48).tobytes()).hexdigest()
                                      for s, h, w, _, _ in rs48])
    # THUMBNAIL_PAD to 48x48: equal to the canvas, smaller than the canvas (pad only, odd deltas on both axes), reduce
    # factors (1,1) (2,1) (1,2) (2,2) (3,2), an aspect so extreme that round_aspect clamps a side to 1, edge columns/rows
    special_tp = [[21, 48, 48, 0, 0], [22, 31, 17, 0, 0], [23, 40, 48, 0, 0], [24, 100, 130, 0, 0], [25, 61, 200, 0, 0],
                  [26, 199, 90, 0, 0], [27, 203, 219, 0, 0], [28, 3, 600, 0, 0], [29, 290, 290, 0, 0], [30, 5, 300, 0, 0],
                  [31, 10, 193, 0, 0], [32, 193, 11, 0, 0]]
    tp48 = special_tp + [[s + 500, h, w, 0, 0] for s, h, w, a, b in bulk(22, 14, 300)]
    p_tp, c_tp = fit_group(out, 'tp48', THUMBNAIL_PAD, (48, 48), tp48)
    # non-square canvases, then one case each at the real 224 / 256 canvases with full-size frames
    fit_group(out, 'rs_rect', RESIZE, (64, 96), [[41, 100, 333, 1, 1], [42, 64, 96, 0, 0], [43, 50, 50, 0, 1]])
    p_tr, _ = fit_group(out, 'tp_rect', THUMBNAIL_PAD, (96, 64), [[44, 150, 333, 0, 0], [45, 64, 95, 0, 0], [46, 777, 301, 0, 0], [47, 451, 301, 0, 0]])
    fit_group(out, 'rs224', RESIZE, (224, 224), [[51, 1213, 777, 1, 1]])
    p_256, _ = fit_group(out, 'tp256', THUMBNAIL_PAD, (256, 256), [[52, 935, 1400, 0, 0]])

    # what the case list must contain (checked on the Pillow-verified plans)
    plans = np.concatenate([p_tp, p_tr, p_256])
    factors = {(int(a), int(b)) for a, b in plans[:, 2:4]}
    assert {(1, 1), (2, 1), (1, 2), (2, 2), (3, 2)} <= factors, factors
    tp_cases = np.array(tp48)
    assert any((c[1], c[2]) == (48, 48) for c in tp48) and any((c[1], c[2]) == (48, 48) and not c[3] and not c[4] for c in rs48)
    small = (tp_cases[:, 1] < 48) & (tp_cases[:, 2] < 48)
    assert small.any() and ((48 - tp_cases[small][:, 1]) % 2 == 1).any() and ((48 - tp_cases[small][:, 2]) % 2 == 1).any()
    odd = ((48 - p_tp[:, 0]) % 2 == 1) & ((48 - p_tp[:, 1]) % 2 == 1)
    assert odd.any()
    assert ((p_tp[:, 0] == 1) | (p_tp[:, 1] == 1)).any()
    rs_cases = np.array(rs48)
    up = (rs_cases[:, 1] < 48) & (rs_cases[:, 2] < 48)
    down = (rs_cases[:, 1] > 48) & (rs_cases[:, 2] > 48)
    for sel in (up, down):
        assert {(int(a), int(b)) for a, b in rs_cases[sel][:, 3:5]} == {(0, 0), (1, 0), (0, 1), (1, 1)}

    # train tails: simple family (colour ops already applied to the raw frame in the fit stage; crop 44 → 48 → rotate) and body
    # family (geometry first, then sharpness / autocontrast); plus the two orders on the rectangular canvases' sizes
    train_group(out, 'simple48', c_rs, 44, 48, 'none', 7)
    dec = train_group(out, 'body48', c_tp, 44, 48, 'geometry_first', 8)
    assert {(int(a), int(b)) for a, b in dec[:, :2]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    # geometry-first on uniform frames that are no fit output (dense content up to the border), 8 cases in full
    geo = np.stack([seeded_frame(70 + i, 61, 61) for i in range(8)])
    out['geo_seeds'], out['geo_hw'] = np.arange(70, 78, dtype=np.int32), np.array([61, 61], np.int32)
    train_group(out, 'geo', geo, 57, 48, 'geometry_first', 9, keep=8)

    # Image.resize (Pillow 12.2.0, Image.py: `if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`) resizes an image taller
    # than 100:1 vertically FIRST; the horizontal-first restatement then differs from Pillow, which is why pfr_augment_fit_params
    # refuses such frames when both passes are needed.  Checked here on a 1000 x 4 frame thumbnailed into 256 x 256.
    tall = seeded_frame(90, 1000, 4)
    assert not np.array_equal(restated_fit(tall, THUMBNAIL_PAD, 256, 256)[3], pil_fit(tall, THUMBNAIL_PAD, 256, 256))
    wide = np.ascontiguousarray(tall.transpose(1, 0, 2))
    assert np.array_equal(restated_fit(wide, THUMBNAIL_PAD, 256, 256)[3], pil_fit(wide, THUMBNAIL_PAD, 256, 256))

    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", {k: v.shape for k, v in out.items() if k.endswith('_out')})


if __name__ == "__main__":
    main()
