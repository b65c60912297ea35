// pfr_dwconv3.hip — depthwise 3x3 convolution on NHWC, padding 1, stride 1 | 2 (forward with the producer's BatchNorm-apply + ReLU6 as a
// prologue and its own BatchNorm statistics as an epilogue, data gradient, weight gradient with the same prologue), for the MobileNetV2
// engine (models/_mobilenet_engine.py).  gfx950, VALU / HBM work: no MFMA, no LDS staging — with 9 taps the halo re-read is left to L2.
//
// Geometry of all three kernels: thread (q, s) = (16-byte channel chunk q of the row, row lane s); a workgroup (256 threads = CW chunk
// columns x RL row lanes, CW = min(C / KPACK, 256)) owns a contiguous range of `rpp` flattened pixel rows and its lanes walk it RL rows
// at a time, so a thread stays on its channels: the 9 taps (and the prologue coefficients) of its KPACK channels sit in registers.  Per
// pixel the 9 (stride-2 data gradient: 4) operand chunks are requested together from CLAMPED coordinates and the taps outside the image
// are zeroed afterwards — after the prologue: the padding is of the activated tensor — so no load sits in a branch.
#include "pfr_common.h"
#include <initializer_list>

struct Dw3Geom {
  int cpr;     // chunks per row (C / KP)
  int cw;      // chunk columns per workgroup
  int rl;      // row lanes per workgroup = 256 / cw
  int gy;      // workgroups along the columns
  long rpp;    // rows per workgroup (the last one may hold fewer)
  int parts;   // workgroups along the rows
};
// `target` workgroups in all, every row lane at least 4 rows
static Dw3Geom dw3_geom(int kp, long rows, int C, int target) {
  Dw3Geom g;
  g.cpr = C / kp;
  g.cw = g.cpr < 256 ? g.cpr : 256;
  g.rl = 256 / g.cw;
  g.gy = (g.cpr + g.cw - 1) / g.cw;
  long want = target / g.gy;
  if (want < 1) want = 1;
  long rpp = (rows + want - 1) / want;
  if (rpp < 4l * g.rl) rpp = 4l * g.rl;
  g.rpp = rpp;
  g.parts = (int)((rows + rpp - 1) / rpp);
  return g;
}

// relu6?(scale * x + shift) of a chunk; hi = +inf when there is no upper clamp
template <int KP>
__device__ __forceinline__ void dw3_activate(float (&v)[KP], const float (&sc)[KP], const float (&sh)[KP], float hi) {
#pragma unroll
  for (int e = 0; e < KP; ++e) v[e] = fminf(fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f), hi);
}

// ------------------------------------------------------------------------------------------------ forward
// stats (STATS): every thread keeps (count, Σd, Σd²) of the STORED y of its rows about its first value, turns them into (mean, M2), and
// lane 0 of each chunk column merges the RL lanes (Chan, fixed order) into the workgroup's partial row [2][C]
template <typename T, bool PRO, bool STATS>
__global__ __launch_bounds__(256) void dwconv3_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
                                                          const float* __restrict__ pro_scale, const float* __restrict__ pro_shift,
                                                          float hi, float* __restrict__ stats, int H, int W, int C, int OH, int OW,
                                                          int stride, int cw, int rl, int cpr, uint32_t rows, uint32_t rpp) {
  constexpr int KP = DT<T>::KPACK;
  __shared__ float red[STATS ? 256 * (2 * KP + 1) : 1];
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  const bool active = s < rl && cglob < cpr;
  const uint32_t rbeg = blockIdx.x * rpp;
  const uint32_t rend = rbeg + rpp < rows ? rbeg + rpp : rows;
  float cnt = 0.f, k[KP], sa[KP], sb[KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) { k[e] = 0.f; sa[e] = 0.f; sb[e] = 0.f; }
  if (active) {
    const int c = cglob * KP;
    float wt[9][KP], sc[KP], sh[KP];
#pragma unroll
    for (int t = 0; t < 9; ++t) Chunk<T>::unpack(ld16(w + (size_t)t * C + c), wt[t]);
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      sc[e] = PRO ? pro_scale[c + e] : 1.f;
      sh[e] = PRO ? pro_shift[c + e] : 0.f;
    }
    const uint32_t plane = (uint32_t)OH * OW;
    for (uint32_t r = rbeg + s; r < rend; r += rl) {
      const uint32_t n = r / plane, rem = r - n * plane;
      const int oh = rem / OW, ow = rem - oh * OW;
      const int ih0 = oh * stride - 1, iw0 = ow * stride - 1;
      u32x4 v[9];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = min(max(ih0 + kh, 0), H - 1), iw = min(max(iw0 + kw, 0), W - 1);
          v[kh * 3 + kw] = ld16(x + (((size_t)n * H + ih) * W + iw) * C + c);
        }
      float acc[KP];
#pragma unroll
      for (int e = 0; e < KP; ++e) acc[e] = 0.f;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = ih0 + kh, iw = iw0 + kw;
          const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
          float f[KP];
          Chunk<T>::unpack(v[kh * 3 + kw], f);
          if (PRO) dw3_activate<KP>(f, sc, sh, hi);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[e] = fmaf(ok ? f[e] : 0.f, wt[kh * 3 + kw][e], acc[e]);
        }
      const u32x4 out = Chunk<T>::pack(acc);
      st16(y + (size_t)r * C + c, out);
      if (STATS) {
        float yr[KP];
        Chunk<T>::unpack(out, yr);
        if (cnt == 0.f) {
#pragma unroll
          for (int e = 0; e < KP; ++e) k[e] = yr[e];
        }
        cnt += 1.f;
#pragma unroll
        for (int e = 0; e < KP; ++e) {
          const float d = yr[e] - k[e];
          sa[e] += d;
          sb[e] = fmaf(d, d, sb[e]);
        }
      }
    }
  }
  if (!STATS) return;
  float* mine = red + threadIdx.x * (2 * KP + 1);
  const float cn = cnt > 0.f ? cnt : 1.f;
  mine[0] = cnt;
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    mine[1 + e] = k[e] + sa[e] / cn;
    mine[1 + KP + e] = sb[e] - sa[e] * sa[e] / cn;
  }
  __syncthreads();
  if (s != 0 || cglob >= cpr) return;
  float nt = 0.f;
  for (int j = 0; j < rl; ++j) nt += red[(j * cw + col) * (2 * KP + 1)];
  float* out_row = stats + (size_t)blockIdx.x * 2 * C + cglob * KP;
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    float a = 0.f;
    for (int j = 0; j < rl; ++j) {
      const float* o = red + (j * cw + col) * (2 * KP + 1);
      a = fmaf(o[0], o[1 + e], a);
    }
    const float mean = a / nt;
    float m2 = 0.f;
    for (int j = 0; j < rl; ++j) {
      const float* o = red + (j * cw + col) * (2 * KP + 1);
      const float d = o[1 + e] - mean;
      m2 += o[1 + KP + e] + o[0] * d * d;
    }
    out_row[e] = mean;
    out_row[C + e] = m2;
  }
}

// ------------------------------------------------------------------------------------------------ data gradient
// gather per dx pixel: dx[h][w] = Σ dy[oh][ow] w[kh][kw] over the taps with oh * stride - 1 + kh = h.  Stride 1: the 9 taps (oh = h + 1 - kh).
// Stride 2: per direction candidate A = (oh = (h + 1) / 2, kh = 0 for odd h, 1 for even h) and candidate B = (oh - 1, kh = 2, odd h
// only), so 4 loads per pixel and a parity select of the tap — an input row or column past the last output pixel simply finds no
// candidate inside [0, OH) x [0, OW)
template <typename T, int STRIDE>
__global__ __launch_bounds__(256) void dwconv3_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx, int H,
                                                            int W, int C, int OH, int OW, int cw, int rl, int cpr, uint32_t rows,
                                                            uint32_t rpp) {
  constexpr int KP = DT<T>::KPACK;
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  if (s >= rl || cglob >= cpr) return;
  const int c = cglob * KP;
  const uint32_t rbeg = blockIdx.x * rpp;
  const uint32_t rend = rbeg + rpp < rows ? rbeg + rpp : rows;
  float wt[9][KP];
#pragma unroll
  for (int t = 0; t < 9; ++t) Chunk<T>::unpack(ld16(w + (size_t)t * C + c), wt[t]);
  const uint32_t plane = (uint32_t)H * W;
  for (uint32_t r = rbeg + s; r < rend; r += rl) {
    const uint32_t n = r / plane, rem = r - n * plane;
    const int h = rem / W, wq = rem - h * W;
    float acc[KP];
#pragma unroll
    for (int e = 0; e < KP; ++e) acc[e] = 0.f;
    if constexpr (STRIDE == 1) {
      u32x4 v[9];
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int oh = min(max(h + 1 - kh, 0), OH - 1), ow = min(max(wq + 1 - kw, 0), OW - 1);
          v[kh * 3 + kw] = ld16(dy + (((size_t)n * OH + oh) * OW + ow) * C + c);
        }
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int oh = h + 1 - kh, ow = wq + 1 - kw;
          const bool ok = oh >= 0 && oh < OH && ow >= 0 && ow < OW;
          float f[KP];
          Chunk<T>::unpack(v[kh * 3 + kw], f);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[e] = fmaf(ok ? f[e] : 0.f, wt[kh * 3 + kw][e], acc[e]);
        }
    } else {
      const bool hodd = h & 1, wodd = wq & 1;
      const int oh[2] = {(h + 1) >> 1, ((h + 1) >> 1) - 1}, ow[2] = {(wq + 1) >> 1, ((wq + 1) >> 1) - 1};
      const bool okh[2] = {oh[0] < OH, hodd && oh[1] >= 0 && oh[1] < OH}, okw[2] = {ow[0] < OW, wodd && ow[1] >= 0 && ow[1] < OW};
      u32x4 v[4];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const int ohc = min(max(oh[a], 0), OH - 1), owc = min(max(ow[b], 0), OW - 1);
          v[a * 2 + b] = ld16(dy + (((size_t)n * OH + ohc) * OW + owc) * C + c);
        }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const bool ok = okh[a] && okw[b];
          float f[KP];
          Chunk<T>::unpack(v[a * 2 + b], f);
#pragma unroll
          for (int e = 0; e < KP; ++e) {
            // tap row: candidate A = kh 0 (odd h) | 1 (even h), candidate B = kh 2; columns likewise
            const float w0 = b == 0 ? (wodd ? wt[0][e] : wt[1][e]) : wt[2][e];
            const float w1 = b == 0 ? (wodd ? wt[3][e] : wt[4][e]) : wt[5][e];
            const float w2 = b == 0 ? (wodd ? wt[6][e] : wt[7][e]) : wt[8][e];
            const float ws = a == 0 ? (hodd ? w0 : w1) : w2;
            acc[e] = fmaf(ok ? f[e] : 0.f, ws, acc[e]);
          }
        }
    }
    st16(dx + (size_t)r * C + c, Chunk<T>::pack(acc));
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// workgroup (p, column block) walks the output rows of its range with the 9 sums of every (channel, row lane) in registers (the operand is
// the activated x, recomputed with the forward's prologue), folds the row lanes through LDS tap by tap and leaves ONE partial row set
// part[p][9][C] (tap-major)
template <typename T, bool PRO>
__global__ __launch_bounds__(256) void dwconv3_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                                                            const float* __restrict__ pro_scale, const float* __restrict__ pro_shift,
                                                            float hi, int H, int W, int C, int OH, int OW, int stride, int cw, int rl,
                                                            int cpr, uint32_t rows, uint32_t rpp) {
  constexpr int KP = DT<T>::KPACK;
  __shared__ float red[256 * KP];
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  const bool active = s < rl && cglob < cpr;
  const int c = cglob * KP;
  const uint32_t rbeg = blockIdx.x * rpp;
  const uint32_t rend = rbeg + rpp < rows ? rbeg + rpp : rows;
  float acc[9][KP];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < KP; ++e) acc[t][e] = 0.f;
  if (active) {
    float sc[KP], sh[KP];
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      sc[e] = PRO ? pro_scale[c + e] : 1.f;
      sh[e] = PRO ? pro_shift[c + e] : 0.f;
    }
    const uint32_t plane = (uint32_t)OH * OW;
    for (uint32_t r = rbeg + s; r < rend; r += rl) {
      const uint32_t n = r / plane, rem = r - n * plane;
      const int oh = rem / OW, ow = rem - oh * OW;
      const int ih0 = oh * stride - 1, iw0 = ow * stride - 1;
      u32x4 v[9];
      const u32x4 vg = ld16(dy + (size_t)r * C + c);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = min(max(ih0 + kh, 0), H - 1), iw = min(max(iw0 + kw, 0), W - 1);
          v[kh * 3 + kw] = ld16(x + (((size_t)n * H + ih) * W + iw) * C + c);
        }
      float g[KP];
      Chunk<T>::unpack(vg, g);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = ih0 + kh, iw = iw0 + kw;
          const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
          float f[KP];
          Chunk<T>::unpack(v[kh * 3 + kw], f);
          if (PRO) dw3_activate<KP>(f, sc, sh, hi);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[kh * 3 + kw][e] = fmaf(g[e], ok ? f[e] : 0.f, acc[kh * 3 + kw][e]);
        }
    }
  }
  // fold the row lanes, one tap at a time (fixed order)
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < KP; ++e) red[threadIdx.x * KP + e] = acc[t][e];
    __syncthreads();
    if (s == 0 && cglob < cpr) {
      float* out = part + ((size_t)blockIdx.x * 9 + t) * C + c;
#pragma unroll
      for (int e = 0; e < KP; ++e) {
        float a = 0.f;
        for (int j = 0; j < rl; ++j) a += red[(j * cw + col) * KP + e];
        out[e] = a;
      }
    }
  }
}

// merge of the partial rows: dw in the parameter's own [C][1][3][3] order; block (tap, 64-channel chunk), 4 slices of P
__global__ __launch_bounds__(256) void dwconv3_wgrad_merge_kernel(const float* __restrict__ part, float* __restrict__ dw, int P, int C,
                                                                  int accumulate) {
  __shared__ float red[4][64];
  const int t = blockIdx.x, cl = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  float v = 0.f;
  if (c < C)
    for (int p = s; p < P; p += 4) v += part[((size_t)p * 9 + t) * C + c];
  red[s][cl] = v;
  __syncthreads();
  if (s != 0 || c >= C) return;
  v = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
  float* out = dw + (size_t)c * 9 + t;
  *out = accumulate ? *out + v : v;
}

// ------------------------------------------------------------------------------------------------ entry points
// argument checks in an order that needs no device: geometry first, pointers last
static int dw3_check(const char* fn, std::initializer_list<const void*> ptrs, int dtype, int N, int H, int W, int C, int stride) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", fn);
  if (stride != 1 && stride != 2) {
    pfr_set_error("%s: only stride 1 and 2 are built (got stride = %d)", fn, stride);
    return PFR_ERR_UNSUPPORTED;
  }
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PFR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "%s: empty tensor", fn);
  PFR_CHECK_ARG(C % kp == 0, "%s: C = %d is not a multiple of %d (16-byte channel chunks)", fn, C, kp);
  PFR_CHECK_ARG((long)N * H * W < (1l << 31), "%s: more than 2^31 pixels", fn);
  PFR_CHECK_ARG(pfr_all_dev(ptrs), "%s: not a device pointer (no CPU fallback)", fn);
  return PFR_OK;
}

static inline long dw3_out_rows(int N, int H, int W, int stride) { return (long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1); }

extern "C" long pfr_dwconv3_rows_per_part(int dtype, int N, int H, int W, int C, int stride) {
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  if ((stride != 1 && stride != 2) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % kp) return 0;
  return dw3_geom(kp, dw3_out_rows(N, H, W, stride), C, 2048).rpp;
}

extern "C" int pfr_dwconv3_fwd(const void* x, const void* w, void* y, int dtype, int N, int H, int W, int C, int stride,
                               const float* pro_scale, const float* pro_shift, float pro_hi, float* stats_part, hipStream_t st) {
  PFR_CHECK_ARG(x && w && y, "pfr_dwconv3_fwd: null pointer");
  PFR_CHECK_ARG(!pro_scale == !pro_shift, "pfr_dwconv3_fwd: pro_scale and pro_shift come together");
  if (int rc = dw3_check("pfr_dwconv3_fwd", {x, w, y, pro_scale, pro_shift, stats_part}, dtype, N, H, W, C, stride)) return rc;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long rows = (long)N * OH * OW;
  const Dw3Geom g = dw3_geom(dtype == PFR_BF16 ? 8 : 4, rows, C, 2048);
  const float hi = pro_hi > 0.f ? pro_hi : __builtin_inff();
  const dim3 grid((unsigned)g.parts, (unsigned)g.gy);
#define PFR_DW3_FWD(TT, PRO, ST)                                                                                                          \
  hipLaunchKernelGGL((dwconv3_fwd_kernel<TT, PRO, ST>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)w, (TT*)y, pro_scale, pro_shift, \
                     hi, stats_part, H, W, C, OH, OW, stride, g.cw, g.rl, g.cpr, (uint32_t)rows, (uint32_t)g.rpp)
#define PFR_DW3_FWD4(TT)                                                          \
  do {                                                                            \
    if (pro_scale) { if (stats_part) PFR_DW3_FWD(TT, true, true); else PFR_DW3_FWD(TT, true, false); }    \
    else { if (stats_part) PFR_DW3_FWD(TT, false, true); else PFR_DW3_FWD(TT, false, false); }           \
  } while (0)
  if (dtype == PFR_BF16) PFR_DW3_FWD4(bf16_t); else PFR_DW3_FWD4(float);
#undef PFR_DW3_FWD4
#undef PFR_DW3_FWD
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_dwconv3_dgrad(const void* dy, const void* w, void* dx, int dtype, int N, int H, int W, int C, int stride, hipStream_t st) {
  PFR_CHECK_ARG(dy && w && dx, "pfr_dwconv3_dgrad: null pointer");
  if (int rc = dw3_check("pfr_dwconv3_dgrad", {dy, w, dx}, dtype, N, H, W, C, stride)) return rc;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long rows = (long)N * H * W;
  const Dw3Geom g = dw3_geom(dtype == PFR_BF16 ? 8 : 4, rows, C, 2048);
  const dim3 grid((unsigned)g.parts, (unsigned)g.gy);
#define PFR_DW3_DG(TT, S)                                                                                                                \
  hipLaunchKernelGGL((dwconv3_dgrad_kernel<TT, S>), grid, dim3(256), 0, st, (const TT*)dy, (const TT*)w, (TT*)dx, H, W, C, OH, OW, g.cw, \
                     g.rl, g.cpr, (uint32_t)rows, (uint32_t)g.rpp)
  if (dtype == PFR_BF16) { if (stride == 1) PFR_DW3_DG(bf16_t, 1); else PFR_DW3_DG(bf16_t, 2); }
  else { if (stride == 1) PFR_DW3_DG(float, 1); else PFR_DW3_DG(float, 2); }
#undef PFR_DW3_DG
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// partial row sets of the weight gradient (part_ws: fp32 [parts][9][C]); 0 for a geometry that is not built
extern "C" int pfr_dwconv3_wgrad_parts(int dtype, int N, int H, int W, int C, int stride) {
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  if ((stride != 1 && stride != 2) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % kp) return 0;
  return dw3_geom(kp, dw3_out_rows(N, H, W, stride), C, 1024).parts;
}

extern "C" int pfr_dwconv3_wgrad(const void* x, const void* dy, float* part_ws, float* dw, int dtype, int N, int H, int W, int C,
                                 int stride, const float* pro_scale, const float* pro_shift, float pro_hi, int accumulate,
                                 hipStream_t st) {
  PFR_CHECK_ARG(x && dy && part_ws && dw, "pfr_dwconv3_wgrad: null pointer");
  PFR_CHECK_ARG(!pro_scale == !pro_shift, "pfr_dwconv3_wgrad: pro_scale and pro_shift come together");
  if (int rc = dw3_check("pfr_dwconv3_wgrad", {x, dy, part_ws, dw, pro_scale, pro_shift}, dtype, N, H, W, C, stride)) return rc;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long rows = (long)N * OH * OW;
  const Dw3Geom g = dw3_geom(dtype == PFR_BF16 ? 8 : 4, rows, C, 1024);
  const float hi = pro_hi > 0.f ? pro_hi : __builtin_inff();
  const dim3 grid((unsigned)g.parts, (unsigned)g.gy);
#define PFR_DW3_WG(TT, PRO)                                                                                                                 \
  hipLaunchKernelGGL((dwconv3_wgrad_kernel<TT, PRO>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)dy, part_ws, pro_scale, pro_shift, hi, \
                     H, W, C, OH, OW, stride, g.cw, g.rl, g.cpr, (uint32_t)rows, (uint32_t)g.rpp)
  if (dtype == PFR_BF16) { if (pro_scale) PFR_DW3_WG(bf16_t, true); else PFR_DW3_WG(bf16_t, false); }
  else { if (pro_scale) PFR_DW3_WG(float, true); else PFR_DW3_WG(float, false); }
#undef PFR_DW3_WG
  PFR_CHECK_LAUNCH();
  hipLaunchKernelGGL(dwconv3_wgrad_merge_kernel, dim3(9, (unsigned)((C + 63) / 64)), dim3(256), 0, st, part_ws, dw, g.parts, C, accumulate);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
