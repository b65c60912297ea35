"""Independent restatement of the depthwise convolutions (pfr_dwconv.hip 7x7, pfr_dwconv3.hip 3x3, pfr_dwconvk.hip K = 3 | 5) and of layer
scale for the tests: float64 CPU references written as the definition (explicit pad, stride and taps; no F.conv2d, no
F.conv_transpose2d), integer cases whose sums are exact in every number format the kernels use, the named edge regions a mismatch is
reported in, and the comparison the GPU tests assert with.  Generators, seeds, the comparisons and the rounding bound are
tests/conv_oracle.py's.

Layouts: x, y, dy, dx [N][H][W][C]; w, dw [C][K][K] (the kernels read the taps tap-major, [K*K][C]: taps()); padding K/2, so the output
plane of stride s is ((H-1)/s + 1) x ((W-1)/s + 1).  A prologue `act` is (mode, scale[C], shift[C], hi): mode 1 = min(max(scale*x + shift,
0), hi), mode 2 = silu(scale*x + shift); it is applied FIRST and the zero padding second (the padding is of the activated tensor).

Exactness of the integer data (RANGES): operands and taps are integers of magnitude <= amax and <= wmax with K*K*amax*wmax (+ 8 for the
7x7 bias) <= 256, so every expected value AND every partial sum, in any order, is an integer of magnitude <= 256: exact in bf16 (8-bit
significand) and in fp32.  With the clamp prologue (scale in {1, 2}, shift in {1, 2}, hi = 6) the operand is an integer in [0, 6] and
clamp(shift) != 0: a kernel that pads before it activates is wrong at every border pixel.  The weight gradient sums `rows` products of
magnitude <= gmax*amax into fp32: rows*gmax*amax < 2^24.  The builders assert all of this on the data and on the references."""
import functools

import torch

from conv_oracle import rng, _seed, assert_exact, assert_within, rounding_bound, int_prologue  # noqa: F401  (re-exported to the tests)

F64 = torch.float64
HI = 6.0
# K -> magnitudes: x (no prologue) and dy; w (no prologue); w with the clamp prologue (operand <= 6); x under the prologue is [-4, 4]
RANGES = {7: dict(x=2, w=2, wpro=None, bias=8),       # 49 * 2 * 2 + 8 = 204
          5: dict(x=3, w=3, wpro=1, bias=0),          # 25 * 3 * 3 = 225;  25 * 6 * 1 = 150
          3: dict(x=4, w=4, wpro=4, bias=0)}          # 9 * 4 * 4 = 144;   9 * 6 * 4 = 216
XPRO, GMAX, ACCMAX = 4, 2, 16


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def taps(w):
    """[C][K][K] -> the kernels' tap-major [K*K][C]"""
    return w.reshape(w.shape[0], -1).t().contiguous()


# ------------------------------------------------------------------------------------------------ references (the definition, float64)
def dw_activate(x, act):
    x = x.to(F64)
    if act is None:
        return x
    mode, sc, sh, hi = act
    u = x * sc.to(F64) + sh.to(F64)
    if mode == 1:
        return u.clamp(0, hi)
    assert mode == 2
    return u / (1 + torch.exp(-u))


def _padded(a, K):
    N, H, W, C = a.shape
    P = K // 2
    ap = torch.zeros(N, H + 2 * P, W + 2 * P, C, dtype=F64)
    ap[:, P:P + H, P:P + W] = a
    return ap


def _tap(ap, kh, kw, stride, OH, OW):
    return ap[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]


def dw_fwd_ref(x, w, K, stride, act=None, bias=None, drop_tap=None):
    """y[n][oh][ow][c] = bias[c] + sum_{kh,kw} act(x)[n][oh*stride - K/2 + kh][ow*stride - K/2 + kw][c] * w[c][kh][kw]  (outside the image: 0).
    drop_tap = (kh, kw, oh, ow): that tap is left out at that output pixel (a deliberately broken copy for the self-test)."""
    N, H, W, C = x.shape
    OH, OW = out_hw(H, W, stride)
    w = w.to(F64).reshape(C, K, K)
    ap = _padded(dw_activate(x, act), K)
    y = torch.zeros(N, OH, OW, C, dtype=F64)
    for kh in range(K):
        for kw in range(K):
            t = _tap(ap, kh, kw, stride, OH, OW) * w[:, kh, kw]
            if drop_tap is not None and tuple(drop_tap[:2]) == (kh, kw):
                t[:, drop_tap[2], drop_tap[3]] = 0
            y += t
    return y + bias.to(F64) if bias is not None else y


def dw_dgrad_ref(dy, w, in_hw, K, stride):
    """the scatter: dx[n][oh*stride - K/2 + kh][ow*stride - K/2 + kw][c] += dy[n][oh][ow][c] * w[c][kh][kw]  (positions outside the image dropped)"""
    dy = dy.to(F64)
    N, OH, OW, C = dy.shape
    H, W = in_hw
    assert (OH, OW) == out_hw(H, W, stride)
    w = w.to(F64).reshape(C, K, K)
    P = K // 2
    dxp = torch.zeros(N, H + 2 * P, W + 2 * P, C, dtype=F64)
    for kh in range(K):
        for kw in range(K):
            _tap(dxp, kh, kw, stride, OH, OW).add_(dy * w[:, kh, kw])
    return dxp[:, P:P + H, P:P + W].clone()


def dw_wgrad_ref(x, dy, K, stride, act=None, acc=None):
    """dw[c][kh][kw] = sum_{n,oh,ow} dy[n][oh][ow][c] * act(x)[n][oh*stride - K/2 + kh][ow*stride - K/2 + kw][c], dbias[c] = sum dy;
    acc = (dw target, dbias target or None) is added.  -> (dw [C][K][K], dbias [C])"""
    dy = dy.to(F64)
    N, OH, OW, C = dy.shape
    ap = _padded(dw_activate(x, act), K)
    dw = torch.zeros(C, K, K, dtype=F64)
    for kh in range(K):
        for kw in range(K):
            dw[:, kh, kw] = (dy * _tap(ap, kh, kw, stride, OH, OW)).sum((0, 1, 2))
    db = dy.sum((0, 1, 2))
    if acc is not None:
        dw = dw + acc[0].to(F64).reshape(C, K, K)
        if acc[1] is not None:
            db = db + acc[1].to(F64)
    return dw, db


# ------------------------------------------------------------------------------------------------ integer cases (computed once, read-only)
def _ints(g, shape, m):
    return torch.randint(-m, m + 1, tuple(shape), generator=g).to(F64)


def _is_int_le(t, m):
    return bool((t == t.round()).all()) and t.abs().max().item() <= m


@functools.lru_cache(maxsize=None)
def dw_case(shape, K, stride=1, pro=False):
    """integer case of one geometry: operands, the references of forward (with the bias at K = 7), data gradient and weight gradient
    (overwrite and accumulate), and the assertions that make `torch.equal` the right comparison.  pro: the clamp prologue."""
    N, H, W, C = shape
    r = RANGES[K]
    g = rng(_seed("dw", shape, K, stride, pro))
    OH, OW = out_hw(H, W, stride)
    c = dict(shape=shape, K=K, stride=stride, ohw=(OH, OW))
    c["x"] = _ints(g, shape, XPRO if pro else r["x"])
    wmax = r["wpro"] if pro else r["w"]
    assert wmax is not None, "no prologue at K = %d" % K
    c["w"] = _ints(g, (C, K, K), wmax)
    c["bias"] = _ints(g, (C,), r["bias"]) if r["bias"] else None
    c["act"] = None
    if pro:
        sc, sh, _ = int_prologue(g, C, True)
        c["act"] = (1, sc, sh.abs() + (sh == 0) * 2, HI)            # shift in {1, 2}: clamp(shift) != 0
        assert set(c["act"][1].tolist()) <= {1.0, 2.0} and set(c["act"][2].tolist()) <= {1.0, 2.0}
    c["dy"] = _ints(g, (N, OH, OW, C), GMAX)                        # upstream gradient of the weight gradient
    c["dyd"] = _ints(g, (N, OH, OW, C), r["x"])                     # ... and of the data gradient (the wider range)
    c["acc_dw"], c["acc_db"] = _ints(g, (C, K, K), ACCMAX), _ints(g, (C,), ACCMAX)
    a = dw_activate(c["x"], c["act"])
    amax = a.abs().max().item()
    # forward: the same sum over magnitudes bounds every partial sum in any order
    c["y"] = dw_fwd_ref(c["x"], c["w"], K, stride, c["act"], c["bias"])
    A = dw_fwd_ref(a.abs(), c["w"].abs(), K, stride, None, None if c["bias"] is None else c["bias"].abs())
    assert _is_int_le(a, HI if pro else r["x"]) and _is_int_le(A, 256) and _is_int_le(c["y"], 256), ("forward range", shape, K, stride, pro)
    assert torch.equal(c["y"].bfloat16().to(F64), c["y"])
    # data gradient (no prologue: of the operand the kernel convolves)
    c["dx"] = dw_dgrad_ref(c["dyd"], c["w"], (H, W), K, stride)
    Ad = dw_dgrad_ref(c["dyd"].abs(), c["w"].abs(), (H, W), K, stride)
    assert _is_int_le(Ad, 256) and _is_int_le(c["dx"], 256), ("data-gradient range", shape, K, stride, pro)
    assert torch.equal(c["dx"].bfloat16().to(F64), c["dx"])
    # weight gradient: fp32 sums of `rows` products
    rows = N * OH * OW
    assert rows * c["dy"].abs().max().item() * max(amax, 1.0) < 2 ** 24, ("weight-gradient range", shape, K, stride, pro)
    c["dw"], c["db"] = dw_wgrad_ref(c["x"], c["dy"], K, stride, c["act"])
    c["dw_acc"], c["db_acc"] = dw_wgrad_ref(c["x"], c["dy"], K, stride, c["act"], (c["acc_dw"], c["acc_db"]))
    for t in (c["dw"], c["db"], c["dw_acc"], c["db_acc"]):
        assert _is_int_le(t, 2 ** 24 - 1) and torch.equal(t.float().to(F64), t)
    return c


@functools.lru_cache(maxsize=None)
def layer_scale_case(shape, with_rs=True):
    """y = residual + row_scale[n] * gamma[c] * u over [N][HW][C] and its gradients, in integers: u, dz in [-8, 8], residual in [-16, 16],
    gamma in {1, 2}, row_scale in {0, 1, 2}: |y| <= 48, |du| <= 32, |dgamma| <= rows * 128 — exact in bf16 / fp32 in any order"""
    N, HW, C = shape
    g = rng(_seed("layer_scale", shape, with_rs))
    c = dict(shape=shape, u=_ints(g, shape, 8), res=_ints(g, shape, 16), dz=_ints(g, shape, 8))
    c["gamma"] = torch.randint(1, 3, (C,), generator=g).to(F64)
    c["rs"] = torch.tensor({1: [2.0], 2: [0.0, 2.0], 3: [0.0, 1.0, 2.0]}[N], dtype=F64) if with_rs else None
    rs = c["rs"].view(N, 1, 1) if with_rs else torch.ones(N, 1, 1, dtype=F64)
    c["y"] = c["res"] + rs * c["gamma"] * c["u"]
    c["du"] = rs * c["gamma"] * c["dz"]
    c["dgamma"] = (rs * c["dz"] * c["u"]).sum((0, 1))
    c["acc"] = _ints(g, (C,), ACCMAX)
    assert _is_int_le(c["y"], 48) and _is_int_le(c["du"], 32) and N * HW * 128 < 2 ** 24 and _is_int_le(c["dgamma"] + c["acc"], 2 ** 24 - 1)
    return c


# ------------------------------------------------------------------------------------------------ edge regions and the comparison
def dw_edge_regions(shape, tile, K=7, chunk=32):
    """named boolean masks (broadcast views of [N][H][W][C]) over an output where the depthwise kernels go wrong: the image border ring of
    width K/2; with `tile` (the 7x7 kernels' tile width, 7 or 8; None for the untiled kernels) the first / last row and column of every
    tile and the ragged last tile row / column; the last channel chunk; the last sample"""
    N, H, W, C = shape
    P = K // 2
    n = torch.arange(N).view(N, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    w = torch.arange(W).view(1, 1, W, 1)
    ch = torch.arange(C).view(1, 1, 1, C)
    regions = {"border ring": (h < P) | (h >= H - P) | (w < P) | (w >= W - P)}
    if tile:
        regions["tile-border rows"] = (h % tile == 0) | (h % tile == tile - 1)
        regions["tile-border columns"] = (w % tile == 0) | (w % tile == tile - 1)
        ragged = torch.zeros(1, 1, 1, 1, dtype=torch.bool)
        if H % tile:
            ragged = ragged | (h >= H // tile * tile)
        if W % tile:
            ragged = ragged | (w >= W // tile * tile)
        regions["last ragged tile"] = ragged
    regions["last channel chunk"] = ch >= (C - 1) // chunk * chunk
    regions["last sample"] = n == N - 1
    return {k: v.expand(N, H, W, C) for k, v in regions.items()}


def _where(bad, shape, tile, K, chunk):
    first = tuple(bad.nonzero()[0].tolist())
    regions = dw_edge_regions(shape, tile, K, chunk)
    names = [k for k, m in regions.items() if bool(m[first])] or ["interior"]
    counts = {k: int((bad & m).sum()) for k, m in regions.items()}
    return "first mismatch (n, h, w, c) = %s in [%s]; mismatches per region %s" % (first, ", ".join(names), counts)


def dw_assert_exact(got, ref, what, tile=None, K=7, chunk=32):
    """conv_oracle.assert_exact on an [N][H][W][C] output; a failure also names the edge regions of the first mismatch"""
    try:
        assert_exact(got, ref, what)
    except AssertionError as e:
        g = got.detach().cpu()
        want = ref.reshape(g.shape).to(g.dtype)
        raise AssertionError("%s; %s" % (e, _where((g != want) | g.isnan(), tuple(g.shape), tile, K, chunk))) from None


def dw_assert_within(got, ref, bound, what, tile=None, K=7, chunk=32):
    """conv_oracle.assert_within, element by element, with the edge regions of the first element outside its bound"""
    try:
        assert_within(got, ref, bound, what)
    except AssertionError as e:
        g = got.detach().cpu().to(F64)
        bad = ~((g - ref.reshape(g.shape)).abs() <= bound.reshape(g.shape))
        raise AssertionError("%s; %s" % (e, _where(bad, tuple(g.shape), tile, K, chunk))) from None
