// pfr_align.hip — landmark alignment, the reference's preprocessor/align.py on the device: a homography from 3 or 4 landmarks onto
// base_pts (pfr_align_solve, host arithmetic only) and the perspective warp of a ragged batch of raw frames to one uniform uint8
// [N][out_h][out_w][3] batch (pfr_align_warp).
//
// OpenCV is not available to this project, so bit-identity with a cv2 build cannot be tested and is NOT claimed.  The contract is
// ours (include/pfr_hip.h states every operation).  It follows OpenCV's published scheme for warpPerspective(..., INTER_LINEAR,
// BORDER_CONSTANT 0): inverse map in fp64, source coordinates quantised to 1/32 pixel, 15-bit integer weights.  It is pinned two
// ways: a numpy restatement (tests/align_oracle.py), which the device must equal bit for bit, and Pillow's
// Image.transform(PERSPECTIVE, BILINEAR), an independent implementation, which must lie within a derived bound of the restatement.
//
// With exactly four correspondences the reference's RANSAC + refinement has nothing to choose or refine, which is why the exact
// solve is the restatement.
//
//   align_warp_kernel   one thread per output pixel; a wave covers a 16 x 4 patch of the output (a workgroup 32 x 8), so that the
//                       taps of neighbouring lanes share cache lines.  The two taps of a source row are adjacent: one 6-byte run
//                       of byte loads (frames have odd row pitches: no wider load is aligned).  All 3 bytes of a pixel are
//                       written by the thread that owns it.  No LDS, no atomics, no data-dependent loops.
#include "pfr_common.h"
#include <math.h>
#include <string.h>

#define ALIGN_MAX_SIDE 4096
#define ALIGN_PW 16     // patch of one wave
#define ALIGN_PH 4
#define ALIGN_BW 32     // tile of one workgroup: 2 x 2 waves
#define ALIGN_BH 8
#define ALIGN_MAX_Z 65535

// ---- host: the solve ------------------------------------------------------------------------------------------------------
static bool all_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!isfinite(v[i])) return false;
  return true;
}

// H (row major, 3 x 3) → its inverse by the adjugate; false when the determinant is 0 or anything is non-finite
static bool invert3(const double* h, double* inv) {
  const double a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7], i = h[8];
  const double adj[9] = {e * i - f * hh, c * hh - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
                         d * hh - e * g, b * g - a * hh, a * e - b * d};
  const double det = a * adj[0] + b * adj[3] + c * adj[6];
  if (!isfinite(det) || det == 0.0) return false;
  for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
  return all_finite(inv, 9);
}

// the exact homography src → dst through 4 correspondences: 8 x 8 system, partial pivoting, h33 = 1
static bool homography4(const double* src, const double* dst, double* h) {
  double A[8][9];
  double big = 0.0;
  for (int k = 0; k < 4; ++k) {
    const double x = src[2 * k], y = src[2 * k + 1], u = dst[2 * k], v = dst[2 * k + 1];
    const double r0[9] = {x, y, 1, 0, 0, 0, -u * x, -u * y, u};
    const double r1[9] = {0, 0, 0, x, y, 1, -v * x, -v * y, v};
    memcpy(A[2 * k], r0, sizeof r0);
    memcpy(A[2 * k + 1], r1, sizeof r1);
  }
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) big = fmax(big, fabs(A[r][c]));
  if (!isfinite(big)) return false;
  for (int c = 0; c < 8; ++c) {
    int p = c;
    for (int r = c + 1; r < 8; ++r)
      if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    if (!(fabs(A[p][c]) >= 1e-12 * big)) return false;
    if (p != c)
      for (int k = 0; k < 9; ++k) { const double t = A[c][k]; A[c][k] = A[p][k]; A[p][k] = t; }
    for (int r = c + 1; r < 8; ++r) {
      const double f = A[r][c] / A[c][c];
      for (int k = c; k < 9; ++k) A[r][k] -= f * A[c][k];
    }
  }
  for (int r = 7; r >= 0; --r) {
    double s = A[r][8];
    for (int k = r + 1; k < 8; ++k) s -= A[r][k] * h[k];
    h[r] = s / A[r][r];
  }
  h[8] = 1.0;
  if (!all_finite(h, 9)) return false;
  for (int k = 0; k < 4; ++k) {   // the solved map returns the four points to 1e-6 px
    const double x = src[2 * k], y = src[2 * k + 1];
    const double w = h[6] * x + h[7] * y + h[8];
    const double u = (h[0] * x + h[1] * y + h[2]) / w, v = (h[3] * x + h[4] * y + h[5]) / w;
    if (!(fabs(u - dst[2 * k]) <= 1e-6 && fabs(v - dst[2 * k + 1]) <= 1e-6)) return false;
  }
  return true;
}

// least-squares rotation + uniform scale + translation src → dst (2-D closed form; a rotation by construction, never a reflection)
static bool similarity(const double* src, const double* dst, int n, double* h) {
  double ma[2] = {0, 0}, mb[2] = {0, 0};
  for (int k = 0; k < n; ++k) { ma[0] += src[2 * k]; ma[1] += src[2 * k + 1]; mb[0] += dst[2 * k]; mb[1] += dst[2 * k + 1]; }
  ma[0] /= n; ma[1] /= n; mb[0] /= n; mb[1] /= n;
  double saa = 0, dot = 0, cross = 0;
  for (int k = 0; k < n; ++k) {
    const double ax = src[2 * k] - ma[0], ay = src[2 * k + 1] - ma[1], bx = dst[2 * k] - mb[0], by = dst[2 * k + 1] - mb[1];
    saa += ax * ax + ay * ay;
    dot += ax * bx + ay * by;
    cross += ax * by - ay * bx;
  }
  if (!(saa > 0.0) || !isfinite(saa)) return false;
  const double p = dot / saa, q = cross / saa;
  if (!(p * p + q * q > 0.0)) return false;
  const double m[9] = {p, -q, mb[0] - (p * ma[0] - q * ma[1]), q, p, mb[1] - (q * ma[0] + p * ma[1]), 0, 0, 1};
  memcpy(h, m, sizeof m);
  return all_finite(h, 9);
}

static double round_mean3(const double* p, int c) { return nearbyint((p[c] + p[2 + c] + p[4 + c]) / 3.0); }   // ties to even

extern "C" int pfr_align_solve(int mode, const double* pts, const double* base, int N, int npts, double min_distance, double* minv,
                               int* valid) {
  PFR_CHECK_ARG(mode == 0 || mode == 1, "pfr_align_solve: mode %d (0 reference, 1 similarity)", mode);
  PFR_CHECK_ARG(N >= 0 && (mode == 0 ? (npts == 3 || npts == 4) : (npts >= 2 && npts <= 1024)),
                "pfr_align_solve: bad sizes (N=%d, npts=%d; reference takes 3 or 4 points, similarity 2..1024)", N, npts);
  if (N == 0) return PFR_OK;
  PFR_CHECK_ARG(pts && base && minv && valid, "pfr_align_solve: null pointer");
  for (int n = 0; n < N; ++n) {
    const double* p = pts + (size_t)n * npts * 2;
    double* out = minv + (size_t)n * 9;
    bool ok = all_finite(p, npts * 2) && all_finite(base, npts * 2);
    for (int i = 0; ok && i < npts; ++i)
      for (int j = i + 1; ok && j < npts; ++j) {
        const double dx = p[2 * i] - p[2 * j], dy = p[2 * i + 1] - p[2 * j + 1];
        ok = sqrt(dx * dx + dy * dy) > min_distance;      // the reference's assert is strict
      }
    double h[9];
    if (ok && mode == 0) {
      double s4[8], d4[8];
      if (npts == 3) {
        s4[0] = round_mean3(p, 0); s4[1] = round_mean3(p, 1);
        d4[0] = round_mean3(base, 0); d4[1] = round_mean3(base, 1);
        memcpy(s4 + 2, p, 6 * sizeof(double));
        memcpy(d4 + 2, base, 6 * sizeof(double));
      } else {
        memcpy(s4, p, sizeof s4);
        memcpy(d4, base, sizeof d4);
      }
      ok = homography4(s4, d4, h);
    } else if (ok) {
      ok = similarity(p, base, npts, h);
    }
    ok = ok && invert3(h, out);
    if (!ok) memset(out, 0, 9 * sizeof(double));
    valid[n] = ok ? 1 : 0;
  }
  return PFR_OK;
}

// ---- device: the warp -----------------------------------------------------------------------------------------------------
// fp64 coordinate → 1/32-pixel integer: clamp to [-2^31, 2^31 - 1], round to nearest, ties to even (the caller excludes NaN)
__device__ __forceinline__ int align_q(double f) {
  f = fmin(fmax(f, -2147483648.0), 2147483647.0);
  return (int)rint(f);
}

// a value that has been rounded: the empty statement makes it opaque to the optimiser, so a product that went through here exists
// as a double of its own and cannot be contracted into the sum it feeds, under any -ffp-contract setting.  No instruction is emitted.
__device__ __forceinline__ double align_rn(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

__global__ __launch_bounds__(256) void align_warp_kernel(const uint8_t* __restrict__ data, const long* __restrict__ off,
                                                         const int* __restrict__ shapes, const double* __restrict__ minv,
                                                         const uint8_t* __restrict__ mask, const long* __restrict__ moff, int oh, int ow,
                                                         uint8_t* __restrict__ out) {
  const int n = blockIdx.z;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int px = blockIdx.x * ALIGN_BW + (wv & 1) * ALIGN_PW + (lane & (ALIGN_PW - 1));
  const int py = blockIdx.y * ALIGN_BH + (wv >> 1) * ALIGN_PH + (lane >> 4);
  if (px >= ow || py >= oh) return;
  const int H = shapes[2 * n], W = shapes[2 * n + 1];
  const double* m = minv + (size_t)n * 9;
  int X = 0, Y = 0;
  bool finite;
  // the all-zero matrix is pfr_align_solve's mark of a rejected frame: its output is zero (uniform over the workgroup)
  const bool rejected = m[0] == 0.0 && m[1] == 0.0 && m[2] == 0.0 && m[3] == 0.0 && m[4] == 0.0 && m[5] == 0.0 && m[6] == 0.0 &&
                        m[7] == 0.0 && m[8] == 0.0;
  {
    // The contract evaluates every product and every sum of the coordinates as its own IEEE double operation: a fused multiply-add
    // rounds once where the contract rounds twice and can land in another 1/32 bin.  The build compiles with -ffp-contract=fast,
    // under which the code generator fuses a product into the sum it feeds whatever the source says (`#pragma clang fp
    // contract(off)` changed nothing in the ISA of this kernel).  So every product goes through align_rn before it is added.
    const double x = (double)px, y = (double)py;
    const double X0 = (align_rn(m[0] * x) + align_rn(m[1] * y)) + m[2];
    const double Y0 = (align_rn(m[3] * x) + align_rn(m[4] * y)) + m[5];
    const double W0 = (align_rn(m[6] * x) + align_rn(m[7] * y)) + m[8];
    const double s = W0 != 0.0 ? 32.0 / W0 : 0.0;
    const double fx = X0 * s, fy = Y0 * s;
    finite = !rejected && isfinite(fx) && isfinite(fy);
    if (finite) { X = align_q(fx); Y = align_q(fy); }
  }
  int acc[3] = {0, 0, 0};
  if (finite) {
    const int ix = X >> 5, ax = X & 31, iy = Y >> 5, ay = Y & 31;      // |ix|, |iy| <= 2^26: ix + 1 and iy + 1 cannot overflow
    const uint8_t* src = data + off[n];
    const uint8_t* mk = mask ? mask + moff[n] : nullptr;
    const bool c0 = ix >= 0 && ix < W, c1 = ix + 1 >= 0 && ix + 1 < W;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int yy = iy + r;
      if (yy < 0 || yy >= H) continue;          // the range test comes first: no address is formed from yy, ix before it
      const int wy = r ? ay : 32 - ay;
      const long rowpx = (long)yy * W;
      bool t0 = c0, t1 = c1;
      if (mk) {
        if (t0) t0 = mk[rowpx + ix] != 0;
        if (t1) t1 = mk[rowpx + ix + 1] != 0;
      }
      const int w0 = (32 - ax) * wy * 32, w1 = ax * wy * 32;
      if (t0) {
        const uint8_t* p = src + (rowpx + ix) * 3;          // with t1 as well: bytes p[0..5], one 6-byte run
        acc[0] += w0 * p[0]; acc[1] += w0 * p[1]; acc[2] += w0 * p[2];
      }
      if (t1) {
        const uint8_t* p = src + (rowpx + ix + 1) * 3;
        acc[0] += w1 * p[0]; acc[1] += w1 * p[1]; acc[2] += w1 * p[2];
      }
    }
  }
  uint8_t* o = out + (((size_t)n * oh + py) * ow + px) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((acc[c] + 16384) >> 15);     // sum of weights 32768: at most 255
}

extern "C" int pfr_align_warp(const unsigned char* data, const long* offsets, const int* shapes, const double* minv,
                              const unsigned char* mask, const long* mask_offsets, int N, int out_h, int out_w, unsigned char* out_u8,
                              hipStream_t st) {
  PFR_CHECK_ARG(N >= 0 && out_h >= 0 && out_w >= 0 && out_h <= ALIGN_MAX_SIDE && out_w <= ALIGN_MAX_SIDE,
                "pfr_align_warp: bad sizes (N=%d out %dx%d; sides up to %d)", N, out_h, out_w, ALIGN_MAX_SIDE);
  if (N == 0 || out_h == 0 || out_w == 0) return PFR_OK;
  PFR_CHECK_ARG(data && offsets && shapes && minv && out_u8 && (!mask || mask_offsets), "pfr_align_warp: null pointer");
  const dim3 tiles((out_w + ALIGN_BW - 1) / ALIGN_BW, (out_h + ALIGN_BH - 1) / ALIGN_BH);
  for (int n0 = 0; n0 < N; n0 += ALIGN_MAX_Z) {     // the z extent of a grid ends at 65535 frames
    const int nn = N - n0 < ALIGN_MAX_Z ? N - n0 : ALIGN_MAX_Z;
    hipLaunchKernelGGL(align_warp_kernel, dim3(tiles.x, tiles.y, nn), dim3(256), 0, st, data, offsets + n0, shapes + 2 * (size_t)n0,
                       minv + 9 * (size_t)n0, mask, mask ? mask_offsets + n0 : nullptr, out_h, out_w,
                       out_u8 + (size_t)n0 * out_h * out_w * 3);
    PFR_CHECK_LAUNCH();
  }
  return PFR_OK;
}
