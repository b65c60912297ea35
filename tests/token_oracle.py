"""Float64 references and DERIVED per-element bounds for the token kernel family: LayerNorm (pfr_swin.hip), exact GELU (gelu_cdf_pdf of
pfr_common.h, the elementwise kernels and the GEMM epilogues act 2 / act 3), the per-tile column statistics of pfr_gemm_act_colstats, and
the ViT token assembly.  Plain numpy / torch float64, no device code.  Nothing here is fitted to a run: every bound is a sum of named
terms, each a unit roundoff times an operation count times the magnitude it scales.

Unit roundoffs: U = 2^-24 (one fp32 operation, round to nearest), UO = 2^-8 for a bf16 result (8-bit significand: the spacing
at 1 is 2^-7, round to nearest errs by half of it; 2^-9 would refuse correctly rounded values) or 2^-24 for fp32.
Row sums over C are bounded as a chain of chain(C) = min(C, 38) additions: no lane of these kernels adds more than 32 values serially
(four chunks of eight in the chunked kernels, C / 64 <= 32 channels in the generic ones) and the fold over the lanes that share a row
has at most 6 levels.  A chain of C itself would make the bound of a 2048-wide row with a large mean infinite, i.e. no check.

Device-function errors the bounds rely on (AMD's device-library documentation lists rsqrtf and the native reciprocal at 1 ulp and
__expf — exp2 of the argument times log2(e) — at 1 ulp of the exp2 plus the argument rounding; taken here as ASSUMPTIONS, 1 ulp = 2 U):
  rsqrtf(a)                    relative error <= 2 U
  __builtin_amdgcn_rcpf(a)     relative error <= 2 U
  __expf(-t), t >= 0           relative error <= (2 + 2 t) U   (exp2: 2 U; the rounded product t * log2(e) moves the result by <= 2 t U)"""
import math
import zlib

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126            # results below the smallest normal fp32 may be flushed or lose bits


def chain(C):
    return min(int(C), 38)


def out_u(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else U


def kpack(dtype):
    return 8 if dtype == torch.bfloat16 else 4


def rng(*key):
    """a fixed generator per case (crc of its description: the same in every process)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rounded(t, dtype):
    """float64 -> the compute dtype -> float64: what the device reads"""
    return t.to(torch.float32).to(dtype).to(F64)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_ref(x, gamma, beta, eps):
    """x [rows][C] (already rounded to the compute dtype), gamma / beta [C]; all float64.  -> mean, var (biased), rstd, y"""
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    return mean, var, rstd, y


def ln_fwd_bounds(x, gamma, beta, eps, dtype):
    """-> bound_mean [rows], bound_rstd [rows], bound_y [rows][C] for a two-pass fp32 kernel (sum, then sum of squared deviations).
      mean   dm = (L + 2) U mean|x|                      L = chain(C) adds, the rounded 1/C, the product
      var    dv = (L + 6) U (var + dm^2) + dm^2          sum (x - m')^2 = sum (x - m)^2 + C (m' - m)^2 exactly; each deviation and square
                                                         rounded (4 U), chain of L fused adds, the product with 1/C and the add of eps (2 U)
      rstd   relative r = dv / (var + eps); (1 - r)^-1/2 - 1 <= r / (2 (1 - r)); rsqrtf 2 U
      y      the deviation x - m' is off by dm + U (|m| + max|x|) (the mean's own error and one rounding at the operands' magnitude: this
             is the term that keeps a correct kernel inside the bound on a row with a large mean and a tiny spread), scaled by rstd |gamma|;
             the relative error of rstd and two products scale |x - m| rstd |gamma|; the fused multiply-add and the output rounding
             scale |y|."""
    C = x.shape[1]
    mean, var, rstd, y = ln_fwd_ref(x, gamma, beta, eps)
    ax = x.abs()
    L = chain(C)
    dm = (L + 2) * U * ax.mean(1)
    dv = (L + 6) * U * (var + dm * dm) + dm * dm
    r = dv / (var + eps)
    rel = torch.where(r < 1, r / (2 * (1 - r).clamp_min(1e-300)), torch.full_like(r, float("inf"))) + 2 * U
    b_rstd = rstd * rel
    dt = (dm + U * (mean.abs() + ax.max(1).values))[:, None]
    dev_ = (x - mean[:, None]).abs()
    b0 = gamma.abs() * rstd[:, None] * (dt * (1 + rel[:, None]) + dev_ * (rel[:, None] + 2 * U))
    b_y = b0 + (U + out_u(dtype)) * (y.abs() + b0) + TINY
    return dm + TINY, b_rstd, b_y


def ln_bwd_ref(dy, x, mean, rstd, gamma, dres):
    """the backward from the device's STORED mean / rstd (float64 copies), as the kernel takes them.  -> dx, dgamma, dbeta (+ pieces)"""
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    a = g.mean(1, keepdim=True)
    b = (g * xh).mean(1, keepdim=True)
    v = rstd[:, None] * (g - a - xh * b)
    dx = v + dres if dres is not None else v
    return {"dx": dx, "v": v, "xh": xh, "g": g, "a": a, "b": b, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)}


def ln_bwd_bounds(dy, x, mean, rstd, gamma, dres, dtype):
    """-> bound_dx [rows][C], bound_dgamma [C], bound_dbeta [C]  (R = rows: dgamma / dbeta are chains of at most R + 8 adds — per-lane row
    loop, lane-group fold, four waves — whatever the partition into workgroups; the test adds the partial rows in float64)
      xh = (x - mean) rstd   2 U |xh|;   g = dy gamma   U |g|
      a  = mean(g)           da = (L + 2) U mean|g|;      b = mean(g xh)   db = (L + 5) U mean|g xh|,   L = chain(C)
      v  = rstd (g - a - xh b):  rstd (da + |xh| db + 4 U (|g| + |a| + |xh b|)),  + U |v| for the product
      dx = v + dres: U |dx|, output rounding UO |dx|"""
    R, C = x.shape
    r = ln_bwd_ref(dy, x, mean, rstd, gamma, dres)
    xh, g, a, b = r["xh"], r["g"], r["a"], r["b"]
    L = chain(C)
    da = (L + 2) * U * g.abs().mean(1, keepdim=True)
    db = (L + 5) * U * (g * xh).abs().mean(1, keepdim=True)
    b0 = rstd.abs()[:, None] * (da + xh.abs() * db + 4 * U * (g.abs() + a.abs() + (xh * b).abs())) + U * r["v"].abs()
    b_dx = b0 + (U + out_u(dtype)) * (r["dx"].abs() + b0) + TINY
    b_dg = (R + 11) * U * (dy * xh).abs().sum(0) + TINY
    b_db = (R + 8) * U * dy.abs().sum(0) + TINY
    return b_dx, b_dg, b_db


def colsum_bound(stored):
    """column sums of a stored matrix [R][C] accumulated in fp32 in any order: a chain of at most R + 8 adds"""
    return (stored.shape[0] + 8) * U * stored.abs().sum(0) + TINY


# ------------------------------------------------------------------------------------------------ GELU
SQRT1_2 = 0.70710678118654752
INV_SQRT_2PI = 0.3989422804014327
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)     # Abramowitz & Stegun 7.1.26, a1..a5


def gelu_cdf(z):
    return 0.5 * (1.0 + torch.erf(z.to(F64) * math.sqrt(0.5)))


def gelu_pdf(z):
    return torch.exp(-0.5 * z.to(F64) ** 2) * (1.0 / math.sqrt(2 * math.pi))


def gelu_ref(z):
    z = z.to(F64)
    return z * gelu_cdf(z)


def gelu_grad_ref(z):
    """d/dz (z Phi(z)) = Phi(z) + z phi(z)"""
    z = z.to(F64)
    return gelu_cdf(z) + z * gelu_pdf(z)


# absolute error of the kernel's Phi(z) = 1 - p(t) t e^(-z^2/2) / 2, t = 1 / (1 + P |z| / sqrt 2), in units of U (besides the formula's own):
#   Horner evaluation of q(t) = p(t) t, five fused steps on t <= 1: sum_k 2 k |a_k|
#   sensitivity to t (fused multiply-add U + reciprocal 2 U): 3 max|q'(t)| on [0, 1] (q' = a1 + 2 a2 t + ... + 5 a5 t^4, at most 3.5)
#   both scaled by e^(-z^2/2) / 2 <= 1/2;  the exponential: (2 + 2 s + 3 s) U with s = z^2/2 (its own error and the three roundings of
#   the argument) times q e^-s / 2 <= (2 + 5 s) e^-s / 2 < 2;  the two products with 1/2 and e^-s: 1.5;  1 - x: 1
K_HORNER = sum(2 * (k + 1) * abs(a) for k, a in enumerate(AS_A))
K_CDF = 0.5 * (K_HORNER + 3 * 3.5) + 2 + 1.5 + 1
ERF_FORMULA = 1.5e-7                                   # published |error| of 7.1.26 on erf; Phi carries half of it
E_CDF = 0.5 * ERF_FORMULA + K_CDF * U
# z phi(z): the exponential's relative error (2 + 5 s) U, the constant and two products 3 U: |z| phi(z) (5 + 5 s) <= 2.3 for every z
K_ZPDF = 2.3


def gelu_fwd_bound(z, dtype):
    """|y' - z Phi(z)| <= |z| (7.5e-8 + K_CDF 2^-24) + (U + UO) |y|: the formula and its evaluation, the product, the output rounding"""
    z = z.to(F64)
    e = z.abs() * E_CDF
    return e + (U + out_u(dtype)) * (gelu_ref(z).abs() + e) + TINY


def gelu_grad_bound(z):
    """absolute error of the kernel's Phi(z) + z phi(z) before it multiplies the incoming gradient"""
    return E_CDF + K_ZPDF * U + U * gelu_grad_ref(z).abs()


def gelu_bwd_bound(z, dy, dtype):
    """dx = dy (Phi(z) + z phi(z)): |dy| times the derivative's error, the product and the output rounding"""
    z, dy = z.to(F64), dy.to(F64)
    e = dy.abs() * gelu_grad_bound(z)
    return e + (U + out_u(dtype)) * ((dy * gelu_grad_ref(z)).abs() + e) + TINY


def finite_class(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    t = t.to(F64)
    return torch.where(torch.isnan(t), 3, torch.where(t == float("inf"), 1, torch.where(t == float("-inf"), 2, 0)))


# ------------------------------------------------------------------------------------------------ gemm_act: exact operands
QUARTER_NNZ = 24


def gemm_case(M, K, N, act):
    """Operands whose GEMM is exact in every format and order: x in {-2..2}/4, w = +-1 at no more than 24 positions of a row, bias in
    {-8..8}/4: every partial sum is a multiple of 1/4 below 0.5 * 24 + 2 = 14, i.e. an integer below 2^8 quarters — exact in bf16 (8-bit
    significand) and in fp32.  act 2: y2 = x w^T + bias (exact), y = gelu(y2).  act 3: no bias, `z` = a given pre-activation [M][N] of
    bf16-exact values, y = (x w^T) gelu'(z)."""
    g = rng("gemm", M, K, N, act)
    x = torch.randint(-2, 3, (M, K), generator=g).to(F64) / 4
    n = min(QUARTER_NNZ, K)
    w = torch.zeros(N, K, dtype=F64)
    for r in range(N):
        pos = torch.randperm(K, generator=g)[:n]
        w[r, pos] = torch.randint(0, 2, (n,), generator=g).to(F64) * 2 - 1
    c = {"x": x, "w": w, "M": M, "K": K, "N": N, "act": act}
    c["lin"] = x @ w.t()
    if act == 2:
        c["bias"] = torch.randint(-8, 9, (N,), generator=g).to(F64) / 4
        c["y2"] = c["lin"] + c["bias"]
    else:
        c["bias"] = None
        z = rounded(torch.randn(M, N, generator=g, dtype=F64) * 2, torch.bfloat16)
        z.view(-1)[:: max(1, z.numel() // 7)] = 0.0
        c["y2"] = z
    return c


def gemm_act_ref(c, stored_y2):
    """y of a case from the STORED pre-activation (float64 copy of the device's y2 for act 2, the input z for act 3)"""
    return gelu_ref(stored_y2) if c["act"] == 2 else c["lin"] * gelu_grad_ref(stored_y2)


def gemm_act_bound(c, stored_y2, dtype):
    return gelu_fwd_bound(stored_y2, dtype) if c["act"] == 2 else gelu_bwd_bound(stored_y2, c["lin"], dtype)


# ------------------------------------------------------------------------------------------------ per-tile statistics
def tile_stats_ref(stored, mt):
    """stored [M][N] float64 -> (mean [T][N], M2 [T][N], rows [T]) of the row tiles of height mt (the last one ragged)"""
    M = stored.shape[0]
    T = (M + mt - 1) // mt
    mean, m2, rows = [], [], []
    for t in range(T):
        blk = stored[t * mt:min(M, (t + 1) * mt)]
        m = blk.mean(0)
        mean.append(m)
        m2.append(((blk - m) ** 2).sum(0))
        rows.append(blk.shape[0])
    return torch.stack(mean), torch.stack(m2), torch.tensor(rows, dtype=F64)


def tile_stats_bounds(stored, mt, shift_abs=None):
    """The kernel sums d = y - k and d^2 over the n rows of a tile, mean = k + s1 / n, M2 = s2 - s1^2 / n.  The shift k is NOT a value of
    the stored column: the tile kernel takes the first row's accumulator before bias and activation, so |d| <= D = Y + |k| with
    Y = max|y| of the tile's column and |k| = shift_abs [T][N] (without it: a value of the column itself, D = 2 Y).
      mean:  chain of n + 4 adds (rows per lane, lane fold, waves) of |d| <= D, the difference, the division and the final add: (n + 6) U D
      M2:    chain (n + 4) U on s2 <= n D^2; s1^2 / n <= n D^2 with relative error (2 (n + 4) + 3) U; squares 2 U; the subtraction U"""
    M = stored.shape[0]
    T = (M + mt - 1) // mt
    bm, b2 = [], []
    for t in range(T):
        blk = stored[t * mt:min(M, (t + 1) * mt)]
        n = blk.shape[0]
        Y = blk.abs().max(0).values
        D = Y + (shift_abs[t] if shift_abs is not None else Y)
        bm.append((n + 6) * U * D + TINY)
        b2.append((3 * n + 16) * U * n * D * D + TINY)
    return torch.stack(bm), torch.stack(b2)


def tile_merge_bound(stored, mt, shift_abs=None):
    """column sum from the tile means, out = sum_t rows_t mean_t as a fused chain in fp32: the means' own bounds weighted by the rows,
    and (T + 8) U on the chain"""
    mean, _, rows = tile_stats_ref(stored, mt)
    bm, _ = tile_stats_bounds(stored, mt, shift_abs)
    T = mean.shape[0]
    return (rows[:, None] * bm).sum(0) + (T + 8) * U * (rows[:, None] * mean.abs()).sum(0) + TINY


# ------------------------------------------------------------------------------------------------ comparison
def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound over all elements; a NaN or an element outside an infinite-free comparison counts as infinity"""
    got = got.detach().cpu().to(F64).reshape(ref.shape)
    err = (got - ref).abs()
    ratio = err / bound.expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_within(got, ref, bound, what=""):
    """every element inside its bound (NaN never is); -> the worst err / bound"""
    got64 = got.detach().cpu().to(F64).reshape(ref.shape)
    b = bound.expand_as(ref)
    err = (got64 - ref).abs()
    bad = ~(err <= b)
    w = worst_ratio(got64, ref, bound)
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements outside the bound, first at %s: got %r want %r err %.3e bound %.3e (worst err / bound %.3g)"
                             % (what, int(bad.sum()), bad.numel(), first, got64[first].item(), ref[first].item(), err[first].item(),
                                b[first].item(), w))
    return w


# ------------------------------------------------------------------------------------------------ the GPU file's input sets
EPS = 1e-5
LN_CHUNKS = [1, 12, 16, 17, 32, 33, 64, 65, 96, 128, 129, 192, 193, 256]
LN_GENERIC = [100, 36]
LN_BF16_GENERIC_MAX = 2044


def ln_widths(dtype):
    w = [c * kpack(dtype) for c in LN_CHUNKS] + list(LN_GENERIC)
    # (100 and 36 are multiples of the fp32 chunk: there they are two more chunked widths, and 102 and 38 take the generic kernels)
    return w + [LN_BF16_GENERIC_MAX] if dtype == torch.bfloat16 else w + [102, 38]


def ln_geom(C, dtype):
    """restates ln_geom of pfr_swin.hip: (G lanes per row, chunks per lane) or None for the generic kernels"""
    kp = kpack(dtype)
    if C % kp:
        return None
    cpr = C // kp
    G = 16 if cpr <= 16 else (32 if cpr <= 32 else 64)
    cpl = (cpr + G - 1) // G
    return (G, cpl) if cpl <= 4 else None


def ln_batch_rows(C, dtype, rb):
    """rows of one forward workgroup batch, rb * 4 * (64 / G); the generic forward takes four rows per workgroup"""
    g = ln_geom(C, dtype)
    return 4 if g is None else (rb if g[1] == 1 else 2) * 4 * (64 // g[0])


def ln_row_counts(C, dtype, rb):
    b = ln_batch_rows(C, dtype, rb)
    return sorted({1, 3, b - 1, b, b + 1} - {0})


def ln_case(rows, C, dtype, use_res):
    """random rows, then (as far as there are rows) a constant row, a row of mean 1000 and spread 1e-2, a row with one non-zero element;
    gamma with zeros and negative values"""
    g = rng("ln", rows, C, str(dtype), use_res)
    x = torch.randn(rows, C, generator=g, dtype=F64) * 2 + 0.3
    special = [torch.full((C,), 1.75, dtype=F64), 1000 + 1e-2 * torch.randn(C, generator=g, dtype=F64), torch.zeros(C, dtype=F64)]
    special[2][C // 2] = 3.0
    if rows >= 3:      # (one row: a random one; three rows: the three special ones; more: random rows and the special ones at the end)
        for i, s in enumerate(special):
            x[rows - 1 - i] = s
    gamma = torch.randn(C, generator=g, dtype=F64)
    gamma[::5] = 0.0
    beta = torch.randn(C, generator=g, dtype=F64) * 0.1
    c = {"x": rounded(x, dtype), "gamma": rounded(gamma, torch.float32), "beta": rounded(beta, torch.float32),
         "dy": rounded(torch.randn(rows, C, generator=g, dtype=F64), dtype)}
    c["dres"] = rounded(torch.randn(rows, C, generator=g, dtype=F64), dtype) if use_res else None
    return c


def bf16_all_finite():
    """every finite bf16 bit pattern (65 280 values; a multiple of the 8-element chunk) as float64"""
    bits = torch.arange(0, 65536, dtype=torch.int32)
    keep = (bits & 0x7F80) != 0x7F80
    v = (bits[keep].to(torch.int32) << 16).view(torch.float32)
    assert v.numel() == 65280 and v.numel() % 8 == 0
    return v.to(F64)


GELU_F32_POINTS = [0.0, 2.0 ** -126, 1e-30, 1e-3, 5.5, 6.0, 10.0, 38.0, 1e4, float(np.finfo(np.float32).max)]


def gelu_f32_inputs():
    """a dense grid over [-12, 12] and the listed points with both signs (-0 included), padded to a chunk multiple with zeros"""
    grid = torch.linspace(-12, 12, 48001, dtype=F64)
    pts = torch.tensor([s * p for p in GELU_F32_POINTS for s in (1.0, -1.0)], dtype=F64)
    v = rounded(torch.cat([grid, pts]), torch.float32)
    pad = (-v.numel()) % 4
    return torch.cat([v, torch.zeros(pad, dtype=F64)])


def gelu_dy(n, dtype):
    """the fixed gradient set the backward pairs the inputs with: a repeating pattern of magnitudes and signs"""
    pat = torch.tensor([1.0, -1.0, 0.5, -2.0, 3.0, 0.0, -0.125, 7.0, 1e-3, -1e3, 0.75], dtype=F64)
    return rounded(pat.repeat(n // pat.numel() + 1)[:n], dtype)


GEMM_NS = lambda dtype: [kpack(dtype), 64, 72, 136]      # noqa: E731
GEMM_KS = lambda dtype: [kpack(dtype), 96, 104]          # noqa: E731


def gemm_ms(mt):
    return sorted({1, mt - 1, mt, mt + 1, 2 * mt + 3})


SLIN_SHAPE = (4096 + 5, 96, 64)      # the fewest rows the streaming Linear takes (M >= 4096, K = 96, N a multiple of 32), ragged

VIT_B, VIT_S = [1, 3], [1, 2, 17]
VIT_D = lambda dtype: [kpack(dtype), 72, 768]            # noqa: E731
LN_MANY_ROWS = 16384 + 21            # the backward's cap of 1024 workgroups is reached above 16 384 rows
GEMM_REAL_SHAPE = (65, 96, 72)


def gemm_real_case(dtype):
    """the one real-valued gemm_act set (act 2): here the stored pre-activation differs from the accumulator, so an epilogue that takes
    GELU of the unrounded value is visible.  y2 is judged by gemm_real_y2_bound, y per element against GELU of the STORED y2."""
    M, K, N = GEMM_REAL_SHAPE
    g = rng("gemm real", str(dtype))
    x = rounded(torch.randn(M, K, generator=g, dtype=F64), dtype)
    w = rounded(torch.randn(N, K, generator=g, dtype=F64) / K ** 0.5, dtype)
    bias = rounded(torch.randn(N, generator=g, dtype=F64) * 0.1, torch.float32)
    c = {"x": x, "w": w, "bias": bias, "M": M, "K": K, "N": N, "act": 2, "lin": x @ w.t()}
    c["y2_ref"] = c["lin"] + bias
    c["absdot"] = x.abs() @ w.abs().t()
    c["acc32"] = x.numpy().astype(np.float32) @ w.numpy().astype(np.float32).T
    return c


def gemm_real_y2_bound(c, dtype):
    """K 2^-23 sum|x||w| for the length-K fp32 accumulation in any order (products included), the rounding of the accumulator to the output
    format, the add of the bias in fp32 and the rounding of the stored value (second-order terms: the factor 1 + 4 UO)"""
    uo = out_u(dtype)
    return (c["K"] * 2.0 ** -23 * c["absdot"] + uo * c["lin"].abs() + (U + uo) * c["y2_ref"].abs()) * (1 + 4 * uo) + TINY
