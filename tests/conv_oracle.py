"""Independent restatement of the convolution family for the tests: integer data generators whose sums are exact in every number format
the kernels use, float64 CPU references written as the definition (explicit pad, stride and taps; no F.conv2d), the per-element rounding
bound of the real-valued tests, and the comparison the GPU tests assert with.

Exactness of the integer data: x in [-2, 2], w = +-1 at no more than `nnz` (<= 96) positions of a filter's K = R*S*C, so |conv| <= 2*nnz
<= 192; bias in [-8, 8], residual and accumulate target in [-16, 16]: |y| <= 192 + 8 + 16 + 16 = 232 < 256, every partial sum is an
integer below 2^8 (exact in bf16, whose 8-bit significand holds all integers up to 256) and far below 2^24 (exact in fp32), whatever the
summation order, split count or tile.  With a prologue scale in {1, 2}, shift in {-1, 0, 1} the operand is an integer in [-5, 5]: those
cases cap nnz at PRO_NNZ = 40 (5 * 40 + 40 = 240) or store fp32.  Layouts are the library's: x [N][H][W][C], w [Cout][R][S][C]."""
import functools
import zlib

import torch

F64 = torch.float64
NNZ = 96
PRO_NNZ = 40
U_BF16 = 2.0 ** -8     # unit roundoff of bf16 (8-bit significand, round to nearest)
U_F32_OUT = 2.0 ** -23   # the per-rounding factor for fp32 output


# ------------------------------------------------------------------------------------------------ generators
def rng(seed):
    return torch.Generator().manual_seed(int(seed))


def _seed(*key):
    """a fixed seed per case (crc of its description: the same in every process)"""
    return zlib.crc32(repr(key).encode())


def int_x(g, shape, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(F64)


def int_w(g, Cout, R, S, C, nnz=NNZ):
    """+-1 at min(nnz, K) random positions of each filter, 0 elsewhere"""
    K = R * S * C
    n = min(nnz, K)
    w = torch.zeros(Cout, K, dtype=F64)
    for co in range(Cout):
        pos = torch.randperm(K, generator=g)[:n]
        w[co, pos] = torch.randint(0, 2, (n,), generator=g).to(F64) * 2 - 1
    return w.reshape(Cout, R, S, C)


def int_bias(g, Cout):
    return torch.randint(-8, 9, (Cout,), generator=g).to(F64)


def int_res(g, shape):
    return torch.randint(-16, 17, tuple(shape), generator=g).to(F64)


def int_prologue(g, C, relu):
    """(scale in {1, 2}, shift in {-1, 0, 1}, relu)"""
    return (torch.randint(1, 3, (C,), generator=g).to(F64), torch.randint(-1, 2, (C,), generator=g).to(F64), int(relu))


def mask_bytes(g, M, Cout, kpack):
    """random ReLU bit mask in the layout of pfr_bn_act_mask: [M][Cout / kpack] bytes, bit e of byte b = channel b * kpack + e"""
    hi = 1 << kpack
    return torch.randint(0, hi, (M, Cout // kpack), generator=g, dtype=torch.int64).to(torch.uint8)


def mask_bits(mask, kpack):
    """[M][Cout / kpack] bytes -> [M][Cout] of 0.0 / 1.0"""
    sh = torch.arange(kpack, dtype=torch.int64)
    return ((mask.to(torch.int64).unsqueeze(-1) >> sh) & 1).reshape(mask.shape[0], -1).to(F64)


# ------------------------------------------------------------------------------------------------ references (the definition, float64)
def out_hw(H, W, R, S, stride, pad):
    return (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1


def apply_prologue(x, pro):
    if pro is None:
        return x
    sc, sh, relu = pro
    x = x * sc.to(F64) + sh.to(F64)
    return x.clamp_min(0) if relu else x


def _padded(x, R, S, stride, pad, OH, OW):
    """zero border: `pad` rows / columns in front, as many behind as the last tap of the last output needs"""
    N, H, W, C = x.shape
    hb = max(0, (OH - 1) * stride + R - pad - H)
    wb = max(0, (OW - 1) * stride + S - pad - W)
    xp = torch.zeros(N, pad + H + hb, pad + W + wb, C, dtype=F64)
    xp[:, pad:pad + H, pad:pad + W] = x
    return xp


def _tap(xp, r, s, stride, OH, OW):
    return xp[:, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride]


def conv_fwd_ref(x, w, stride=1, pad=0, ohw=None, bias=None, residual=None, res_bits=None, acc=None, out_relu=False, pro=None,
                 drop_tap=None):
    """y[n][oh][ow][co] = sum_{r,s,c} act(x)[n][oh*stride - pad + r][ow*stride - pad + s][c] * w[co][r][s][c]  (outside the image: 0)
    + bias[co] + (res_bits ? residual : 0) + acc, then ReLU.  drop_tap = (r, s, oh, ow): that tap is left out at that output pixel
    (a deliberately broken copy for the self-test of the comparison)."""
    x, w = x.to(F64), w.to(F64)
    N, H, W, C = x.shape
    Cout, R, S, _ = w.shape
    OH, OW = ohw if ohw is not None else out_hw(H, W, R, S, stride, pad)
    xp = _padded(apply_prologue(x, pro), R, S, stride, pad, OH, OW)
    y = torch.zeros(N, OH, OW, Cout, dtype=F64)
    for r in range(R):
        for s in range(S):
            t = _tap(xp, r, s, stride, OH, OW) @ w[:, r, s, :].t()
            if drop_tap is not None and drop_tap[:2] == (r, s):
                t[:, drop_tap[2], drop_tap[3]] = 0
            y += t
    if bias is not None:
        y = y + bias.to(F64)
    if residual is not None:
        res = residual.to(F64).reshape(y.shape)
        y = y + (res * res_bits.reshape(y.shape) if res_bits is not None else res)
    if acc is not None:
        y = y + acc.to(F64).reshape(y.shape)
    return y.clamp_min(0) if out_relu else y


def conv_dgrad_ref(dy, w, in_hw, stride, pad, acc=None):
    """dx[n][oh*stride - pad + r][ow*stride - pad + s][c] += dy[n][oh][ow][co] * w[co][r][s][c]  (positions outside the image dropped)"""
    dy, w = dy.to(F64), w.to(F64)
    N, OH, OW, Cout = dy.shape
    _, R, S, C = w.shape
    H, W = in_hw
    hb = max(0, (OH - 1) * stride + R - pad - H)
    wb = max(0, (OW - 1) * stride + S - pad - W)
    dxp = torch.zeros(N, pad + H + hb, pad + W + wb, C, dtype=F64)
    for r in range(R):
        for s in range(S):
            dxp[:, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride] += dy @ w[:, r, s, :]
    dx = dxp[:, pad:pad + H, pad:pad + W].clone()
    return dx + acc.to(F64) if acc is not None else dx


def conv_wgrad_ref(x, dy, R, S, stride, pad, pro=None, scale=1.0, acc=None):
    """dw[co][r][s][c] = scale * sum_{n,oh,ow} dy[n][oh][ow][co] * act(x)[n][oh*stride - pad + r][ow*stride - pad + s][c]  (+ acc)"""
    x, dy = x.to(F64), dy.to(F64)
    N, OH, OW, Cout = dy.shape
    C = x.shape[-1]
    xp = _padded(apply_prologue(x, pro), R, S, stride, pad, OH, OW)
    dw = torch.zeros(Cout, R, S, C, dtype=F64)
    dyt = dy.reshape(-1, Cout).t()
    for r in range(R):
        for s in range(S):
            dw[:, r, s, :] = dyt @ _tap(xp, r, s, stride, OH, OW).reshape(-1, C)
    dw = dw * scale
    return dw + acc.to(F64) if acc is not None else dw


# ------------------------------------------------------------------------------------------------ cases (computed once, shared, read-only)
@functools.lru_cache(maxsize=None)
def fwd_case(geom, epi="", ohw=None, zero_from=None):
    """integer forward case.  geom = (N, H, W, C, Cout, R, stride, pad); epi: any of the words bias res join acc relu pro prorelu,
    joined by '+'; zero_from: channels >= it are zero (the stem's padding channels).  -> dict of float64 CPU tensors (reference: fwd_ref)."""
    N, H, W, C, Cout, R, stride, pad = geom
    flags = set(filter(None, epi.split("+")))
    g = rng(_seed(geom, epi))
    OH, OW = ohw if ohw is not None else out_hw(H, W, R, R, stride, pad)
    c = {"geom": geom, "ohw": (OH, OW), "flags": flags}
    c["x"] = int_x(g, (N, H, W, C))
    if zero_from is not None:
        c["x"][..., zero_from:] = 0
    has_pro = bool(flags & {"pro", "prorelu"})
    c["w"] = int_w(g, Cout, R, R, C, PRO_NNZ if has_pro else NNZ)
    c["bias"] = int_bias(g, Cout) if "bias" in flags else None
    c["res"] = int_res(g, (N, OH, OW, Cout)) if flags & {"res", "join"} else None
    c["acc"] = int_res(g, (N, OH, OW, Cout)) if "acc" in flags else None
    c["pro"] = int_prologue(g, C, "prorelu" in flags) if has_pro else None
    for kp in (8, 4):
        c["mask%d" % kp] = mask_bytes(g, N * OH * OW, Cout, kp) if "join" in flags and Cout % kp == 0 else None
    c["relu"] = "relu" in flags
    return c


def fwd_ref(c, kpack=8, **kw):
    """the reference of a forward case (kept with the case: computed once, shared by the tests, never modified)"""
    key = ("ref", kpack)
    if not kw and key in c:
        return c[key]
    bits = mask_bits(c["mask%d" % kpack], kpack) if "join" in c["flags"] else None
    N, H, W, C, Cout, R, stride, pad = c["geom"]
    ref = _fwd_ref(c, bits, stride, pad, **kw)
    if not kw:
        c[key] = ref
    return ref


def _fwd_ref(c, bits, stride, pad, **kw):
    return conv_fwd_ref(c["x"], c["w"], stride, pad, c["ohw"], c["bias"], c["res"], bits, c["acc"], c["relu"], c["pro"], **kw)


@functools.lru_cache(maxsize=None)
def dgrad_case(geom, accumulate=False):
    """integer data-gradient case: the nonzero cap holds per INPUT channel (the filter of the data gradient is w[:, :, :, c])"""
    N, H, W, C, Cout, R, stride, pad = geom
    g = rng(_seed(geom, "dgrad"))
    OH, OW = out_hw(H, W, R, R, stride, pad)
    wt = int_w(g, C, R, R, Cout)                              # [C][R][S][Cout]: <= 96 nonzeros per input channel
    c = {"geom": geom, "w": wt.permute(3, 1, 2, 0).contiguous(), "dy": int_x(g, (N, OH, OW, Cout))}
    c["acc"] = int_res(g, (N, H, W, C)) if accumulate else None
    c["ref"] = conv_dgrad_ref(c["dy"], c["w"], (H, W), stride, pad, c["acc"])
    return c


@functools.lru_cache(maxsize=None)
def wgrad_case(geom, pro="", accumulate=False):
    N, H, W, C, Cout, R, stride, pad = geom
    g = rng(_seed(geom, "wgrad", pro))
    OH, OW = out_hw(H, W, R, R, stride, pad)
    c = {"geom": geom, "x": int_x(g, (N, H, W, C)), "dy": int_x(g, (N, OH, OW, Cout))}
    c["pro"] = int_prologue(g, C, pro == "prorelu") if pro else None
    c["acc"] = int_res(g, (Cout, R, R, C)) if accumulate else None
    return c


# ------------------------------------------------------------------------------------------------ rounding bound and comparison
def rounding_bound(values, K, A, out_bf16):
    """|got - ref| <= sum_i u * |v_i| + K * 2^-23 * A + 1e-30 per element, u = 2^-8 for bf16 output and 2^-23 for fp32 output:
    `values` = the exact values the kernel's epilogue rounds to the output format (one entry per rounding: n_r entries), K = the
    reduction length, A = the same convolution over |x|, |w| (the gamma_K bound of a length-K fp32 accumulation, 2^-23 = 2 * 2^-24
    also covering the product rounding of the fp32 path)."""
    u = U_BF16 if out_bf16 else U_F32_OUT
    err = K * 2.0 ** -23 * A + 1e-30
    for v in values:
        err = err + u * v.abs()
    return err


def assert_exact(got, ref, what=""):
    """got: the kernel's output (any dtype / device); ref: float64 — equal after casting ref to got's dtype, NaN never equal"""
    got = got.detach().cpu()
    want = ref.reshape(got.shape).to(got.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | got.isnan()
        idx = bad.nonzero()
        first = tuple(idx[0].tolist())
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r want %r" %
                             (what, int(bad.sum()), bad.numel(), first, got[first].item(), want[first].item()))


def assert_within(got, ref, bound, what=""):
    got = got.detach().cpu().to(F64)
    err = (got - ref.reshape(got.shape)).abs()
    bad = ~(err <= bound.reshape(got.shape))
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements outside the bound, first at %s: err %.3e bound %.3e (worst err / bound %.3f)" %
                             (what, int(bad.sum()), bad.numel(), first, err[first].item(), bound.reshape(got.shape)[first].item(),
                              (err / bound.reshape(got.shape)).nan_to_num(posinf=float("inf")).max().item()))


def edge_regions(ref, mtile=64, ctile=64):
    """named regions of an output [N][OH][OW][Cout] where kernels go wrong"""
    N, OH, OW, Cout = ref.shape
    flat = ref.reshape(-1, Cout)
    M = flat.shape[0]
    return {"first row": ref[:, 0], "last row": ref[:, OH - 1], "first column": ref[:, :, 0], "last column": ref[:, :, OW - 1],
            "last m-tile rows": flat[(M - 1) // mtile * mtile:], "last column-tile channels": flat[:, (Cout - 1) // ctile * ctile:]}


# ------------------------------------------------------------------------------------------------ the geometries of the exact tests
# N, H, W, C, Cout, R, stride, pad — the smallest shapes that still cross each kernel's edges
FWD_GEOMS = [
    (2, 9, 9, 64, 72, 3, 1, 1),       # M = 162: ragged against 64 / 128 / 256 rows; Cout ragged against 64 / 128 / 256 columns
    (1, 9, 11, 32, 200, 3, 1, 1),     # non-square; two ragged column tiles
    (2, 15, 15, 64, 64, 3, 2, 1),     # stride 2, odd extent
    (2, 16, 16, 64, 128, 1, 2, 0),    # strided 1x1
    (2, 12, 12, 8, 64, 7, 2, 3),      # 7x7, C = 8: the k-step-ragged (non-FAST) path in both dtypes
    (3, 5, 5, 24, 40, 3, 1, 1),       # C = 24: non-FAST; Cout % 8 == 0 but < 64
    (37, 1, 1, 512, 100, 1, 1, 0),    # plain GEMM, padded pitch (LDY)
    (1, 3, 3, 128, 64, 3, 1, 1),      # every output pixel touches the border
]
LDY = {(37, 1, 1, 512, 100, 1, 1, 0): 104}
EPI_GEOMS = [(2, 9, 9, 64, 72, 3, 1, 1), (2, 7, 7, 64, 64, 1, 1, 0)]
EPIS = ["bias", "res", "acc", "relu", "bias+res+relu", "pro", "prorelu", "join"]
DGRAD_GEOMS = [
    (3, 9, 9, 32, 64, 3, 1, 1),       # stride 1, 3x3
    (1, 9, 9, 64, 96, 3, 2, 1),       # stride 2 on odd extents: the plain dilated path
    (3, 8, 8, 64, 128, 3, 2, 1),      # stride 2 on even extents: the parity-class path
    (1, 10, 10, 96, 32, 3, 2, 1),
    (3, 8, 8, 64, 128, 1, 2, 0),      # stride-2 1x1: only class (0, 0) has taps
    (1, 10, 10, 8, 64, 7, 2, 3),      # 7x7 stride 2 pad 3 at C = 8
]
SCONV_GEOMS = [(1, 3, 3, 64, 256, 1, 1, 0), (3, 5, 5, 64, 64, 1, 1, 0), (7, 9, 9, 256, 64, 1, 1, 0), (2, 8, 8, 256, 512, 1, 2, 0)]
SCONV_JOIN_GEOMS = [(3, 5, 5, 64, 64, 1, 1, 0), (7, 9, 9, 256, 64, 1, 1, 0)]
SCONV3_GEOMS = [(1, 8, 8, 64, 64, 3, 1, 1), (2, 12, 16, 64, 64, 3, 1, 1), (3, 16, 16, 64, 64, 3, 1, 1)]
STEM_GEOM = (64, 32, 32, 16, 64, 4, 1, 2)      # output 32 x 32 (the 4x4 / pad 2 window of the space-to-depth stem is cut to the input size)
SLIN_GEOMS = [(4096 + 5, 1, 1, 96, 96, 1, 1, 0), (31 * 133, 1, 1, 96, 64, 1, 1, 0), (4100, 1, 1, 192, 576, 1, 1, 0)]
WGRAD_GEOMS = [
    (2, 9, 9, 64, 72, 3, 1, 1),       # M = 162: the k-tail of the M reduction
    (1, 9, 11, 32, 200, 3, 1, 1),
    (2, 15, 15, 64, 64, 3, 2, 1),     # stride 2, odd extent
    (2, 16, 16, 32, 64, 3, 2, 1),     # stride 2, even extent
    (2, 16, 16, 64, 128, 1, 2, 0),
    (2, 12, 12, 8, 64, 7, 2, 3),      # 7x7 at C = 8
    (3, 5, 5, 24, 40, 3, 1, 1),
    (37, 1, 1, 512, 104, 1, 1, 0),    # (Cout raised to the 16-byte chunk the weight gradient requires)
    (1, 3, 3, 128, 64, 3, 1, 1),
    (3, 27, 27, 32, 64, 3, 2, 1),     # M = 588: three splits of >= 256 rows exist
    (1, 1, 1, 64, 64, 1, 1, 0),       # M = 1
]
WGRAD_BIG_GEOM = (2, 9, 9, 64, 256, 3, 1, 1)             # Cout = 256, KK = 576
SWGRAD_GEOM = (16421, 1, 1, 256, 256, 1, 1, 0)           # the fewest rows the streaming kernel pipelines at 256 x 256, plus a ragged tail
WGRAD9_GEOMS = [(2, 7, 7, 64, 64, 3, 1, 1), (2, 9, 9, 64, 64, 3, 1, 1), (1, 12, 16, 64, 128, 3, 1, 1)]
WGRAD_PRO_GEOMS = [(2, 9, 9, 64, 72, 3, 1, 1), (2, 12, 12, 8, 64, 7, 2, 3)]
