// pfr_dwconv.hip — depthwise 7x7 convolution on NHWC (forward = data gradient with mirrored taps, weight / bias gradient) and
// layer scale with per-sample stochastic depth, for the ConvNeXt engine (models/_convnext_engine.py).  gfx950, VALU / HBM work: no MFMA.
//
// Geometry of the depthwise kernels: a workgroup (256 threads) owns a TW x TW output tile (TW = 7 when the plane is a multiple of 7 —
// ConvNeXt's 56 / 28 / 14 / 7 — else 8) of a 32-channel chunk.  The haloed (TW+6)^2 x 32 input tile is staged in LDS with 16-byte loads
// (zero outside the plane / past C); thread (c = tid % 32, r = tid / 32) computes output row r of channel c with that channel's 49 taps in
// registers: per tap row it reads TW+6 inputs from LDS for 7*TW FMAs.  32-channel chunks divide every ConvNeXt width (96 .. 768) exactly.
#include "pfr_common.h"
#include <initializer_list>

#define DW_K 7
#define DW_CC 32   // channels per workgroup
#define DW_RS 8    // row slots per workgroup (256 threads / 32 channels)

// stage a PH x PW pixel window (top-left at (gh0, gw0) of image n) of DW_CC channels from c0 into LDS [pixel][32]
template <typename T>
__device__ __forceinline__ void dw_stage(const T* __restrict__ src, T* __restrict__ dst, int n, int gh0, int gw0, int PH, int PW, int H,
                                         int W, int C, int c0) {
  constexpr int KP = DT<T>::KPACK;
  constexpr int CPP = DW_CC / KP;
  const int items = PH * PW * CPP;
  for (int i = threadIdx.x; i < items; i += 256) {
    const int p = i / CPP, q = i - p * CPP;
    const int py = p / PW, px = p - py * PW;
    const int gh = gh0 + py, gw = gw0 + px, c = c0 + q * KP;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (gh >= 0 && gh < H && gw >= 0 && gw < W && c < C) v = ld16(src + (((size_t)n * H + gh) * W + gw) * C + c);
    st16(dst + p * DW_CC + q * KP, v);
  }
}

template <typename T, int TW>
__global__ __launch_bounds__(256) void dwconv7_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bias,
                                                          T* __restrict__ y, int H, int W, int C, int tiles_w, int tiles_img, int flip) {
  constexpr int PW = TW + DW_K - 1;
  __shared__ __attribute__((aligned(16))) T tile[PW * PW * DW_CC];
  const int n = blockIdx.x / tiles_img, tr = blockIdx.x - n * tiles_img;
  const int th = tr / tiles_w, tw = tr - th * tiles_w;
  const int h0 = th * TW, w0 = tw * TW, c0 = blockIdx.y * DW_CC;
  dw_stage<T>(x, tile, n, h0 - 3, w0 - 3, PW, PW, H, W, C, c0);
  const int cl = threadIdx.x & (DW_CC - 1), r = threadIdx.x >> 5;
  const int c = c0 + cl;
  const bool active = r < TW && c < C && h0 + r < H;
  float wt[DW_K * DW_K];
#pragma unroll
  for (int t = 0; t < DW_K * DW_K; ++t) wt[t] = active ? to_f32(w[(size_t)(flip ? DW_K * DW_K - 1 - t : t) * C + c]) : 0.f;
  __syncthreads();
  if (!active) return;
  float acc[TW];
  const float b = bias ? bias[c] : 0.f;
#pragma unroll
  for (int j = 0; j < TW; ++j) acc[j] = b;
#pragma unroll
  for (int kh = 0; kh < DW_K; ++kh) {
    const T* row = tile + (r + kh) * PW * DW_CC + cl;
    float in[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) in[j] = to_f32(row[j * DW_CC]);
#pragma unroll
    for (int kw = 0; kw < DW_K; ++kw)
#pragma unroll
      for (int j = 0; j < TW; ++j) acc[j] = fmaf(in[j + kw], wt[kh * DW_K + kw], acc[j]);
  }
  T* out = y + (((size_t)n * H + h0 + r) * W + w0) * C + c;
#pragma unroll
  for (int j = 0; j < TW; ++j)
    if (w0 + j < W) out[(size_t)j * C] = from_f32<T>(acc[j]);
}

// weight / bias gradient: workgroup (p, chunk) walks tiles p, p + P, ... of its channel chunk with the 49 + 1 sums of every (channel, row
// slot) in registers, folds the 8 row slots through LDS at the end and leaves ONE partial row set part[p][50][C] (tap-major, row 49 = bias)
template <typename T, int TW>
__global__ __launch_bounds__(256) void dwconv7_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                                                            int ntiles, int H, int W, int C, int tiles_w, int tiles_img) {
  constexpr int PW = TW + DW_K - 1;
  constexpr int NT = DW_K * DW_K + 1;
  constexpr int TILE_B = (PW * PW + TW * TW) * DW_CC * (int)sizeof(T);
  constexpr int RED_B = 4 * NT * DW_CC * (int)sizeof(float);
  __shared__ __attribute__((aligned(16))) char smem[TILE_B > RED_B ? TILE_B : RED_B];
  T* xt = reinterpret_cast<T*>(smem);
  T* gt = xt + PW * PW * DW_CC;
  const int c0 = blockIdx.y * DW_CC;
  const int cl = threadIdx.x & (DW_CC - 1), r = threadIdx.x >> 5;
  float acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = 0.f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = tile / tiles_img, tr = tile - n * tiles_img;
    const int th = tr / tiles_w, tw = tr - th * tiles_w;
    const int h0 = th * TW, w0 = tw * TW;
    __syncthreads();
    dw_stage<T>(x, xt, n, h0 - 3, w0 - 3, PW, PW, H, W, C, c0);
    dw_stage<T>(dy, gt, n, h0, w0, TW, TW, H, W, C, c0);
    __syncthreads();
    if (r < TW) {
      float g[TW];
#pragma unroll
      for (int j = 0; j < TW; ++j) {
        g[j] = to_f32(gt[(r * TW + j) * DW_CC + cl]);
        acc[NT - 1] += g[j];
      }
#pragma unroll
      for (int kh = 0; kh < DW_K; ++kh) {
        const T* row = xt + (r + kh) * PW * DW_CC + cl;
        float in[PW];
#pragma unroll
        for (int j = 0; j < PW; ++j) in[j] = to_f32(row[j * DW_CC]);
#pragma unroll
        for (int kw = 0; kw < DW_K; ++kw)
#pragma unroll
          for (int j = 0; j < TW; ++j) acc[kh * DW_K + kw] = fmaf(g[j], in[j + kw], acc[kh * DW_K + kw]);
      }
    }
  }
  // fold the row slots: 8 -> 4 -> 2 -> 1
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int half = DW_RS / 2; half >= 1; half >>= 1) {
    __syncthreads();
    if (r >= half && r < 2 * half) {
#pragma unroll
      for (int t = 0; t < NT; ++t) red[((r - half) * NT + t) * DW_CC + cl] = acc[t];
    }
    __syncthreads();
    if (r < half) {
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] += red[(r * NT + t) * DW_CC + cl];
    }
  }
  if (r == 0 && c0 + cl < C) {
    float* out = part + (size_t)blockIdx.x * NT * C + c0 + cl;
#pragma unroll
    for (int t = 0; t < NT; ++t) out[(size_t)t * C] = acc[t];
  }
}

// merge of the partial rows: dw in the parameter's own [C][1][7][7] order, dbias [C]; block (t, 64-channel chunk), 4 slices of P
__global__ __launch_bounds__(256) void dwconv7_wgrad_merge_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                  float* __restrict__ dbias, int P, int C, int accumulate) {
  constexpr int NT = DW_K * DW_K + 1;
  __shared__ float red[4][64];
  const int t = blockIdx.x, cl = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  float v = 0.f;
  if (c < C)
    for (int p = s; p < P; p += 4) v += part[((size_t)p * NT + t) * C + c];
  red[s][cl] = v;
  __syncthreads();
  if (s != 0 || c >= C) return;
  v = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
  float* out = t < NT - 1 ? dw + (size_t)c * (NT - 1) + t : (dbias ? dbias + c : nullptr);
  if (out) *out = accumulate ? *out + v : v;
}

static inline int dw_tile(int H, int W) { return (H % 7 == 0 && W % 7 == 0) ? 7 : 8; }

static int dw_check(const char* fn, std::initializer_list<const void*> ptrs, int dtype, int N, int H, int W, int C, int K) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", fn);
  if (K != DW_K) {
    pfr_set_error("%s: only K = 7 is built (got K = %d)", fn, K);
    return PFR_ERR_UNSUPPORTED;
  }
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PFR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "%s: empty tensor", fn);
  PFR_CHECK_ARG(C % kp == 0, "%s: C = %d is not a multiple of %d (16-byte channel chunks)", fn, C, kp);
  PFR_CHECK_ARG(pfr_all_dev(ptrs), "%s: not a device pointer (no CPU fallback)", fn);
  return PFR_OK;
}

extern "C" int pfr_dwconv2d_fwd(const void* x, const void* w, const float* bias, void* y, int dtype, int N, int H, int W, int C, int K,
                                int flip, hipStream_t st) {
  PFR_CHECK_ARG(x && w && y, "pfr_dwconv2d_fwd: null pointer");
  if (int rc = dw_check("pfr_dwconv2d_fwd", {x, w, bias, y}, dtype, N, H, W, C, K)) return rc;
  const int TW = dw_tile(H, W);
  const int tw = (W + TW - 1) / TW, thh = (H + TW - 1) / TW;
  const long nt = (long)N * tw * thh;
  PFR_CHECK_ARG(nt < (1l << 31), "pfr_dwconv2d_fwd: too many tiles");
  const dim3 grid((unsigned)nt, (unsigned)((C + DW_CC - 1) / DW_CC));
#define PFR_DW_FWD(TT, TWV) \
  hipLaunchKernelGGL((dwconv7_fwd_kernel<TT, TWV>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)w, bias, (TT*)y, H, W, C, tw, tw * thh, flip)
  if (dtype == PFR_BF16) {
    if (TW == 7) PFR_DW_FWD(bf16_t, 7); else PFR_DW_FWD(bf16_t, 8);
  } else {
    if (TW == 7) PFR_DW_FWD(float, 7); else PFR_DW_FWD(float, 8);
  }
#undef PFR_DW_FWD
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// partial row sets of the weight gradient (part_ws: fp32 [parts][50][C]); ~1024 workgroups over all channel chunks, every one at least a tile
extern "C" int pfr_dwconv2d_wgrad_parts(int dtype, int N, int H, int W, int C, int K) {
  (void)dtype;
  if (K != DW_K || N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  const int TW = dw_tile(H, W);
  const long nt = (long)N * ((W + TW - 1) / TW) * ((H + TW - 1) / TW);
  const int nch = (C + DW_CC - 1) / DW_CC;
  long P = 1024 / nch;
  if (P < 1) P = 1;
  if (P > nt) P = nt;
  return (int)P;
}

extern "C" int pfr_dwconv2d_wgrad(const void* x, const void* dy, float* part_ws, float* dw, float* dbias, int dtype, int N, int H, int W,
                                  int C, int K, int accumulate, hipStream_t st) {
  PFR_CHECK_ARG(x && dy && part_ws && dw, "pfr_dwconv2d_wgrad: null pointer");
  if (int rc = dw_check("pfr_dwconv2d_wgrad", {x, dy, part_ws, dw, dbias}, dtype, N, H, W, C, K)) return rc;
  const int TW = dw_tile(H, W);
  const int tw = (W + TW - 1) / TW, thh = (H + TW - 1) / TW;
  const long nt = (long)N * tw * thh;
  PFR_CHECK_ARG(nt < (1l << 31), "pfr_dwconv2d_wgrad: too many tiles");
  const int P = pfr_dwconv2d_wgrad_parts(dtype, N, H, W, C, K);
  const dim3 grid((unsigned)P, (unsigned)((C + DW_CC - 1) / DW_CC));
#define PFR_DW_WG(TT, TWV) \
  hipLaunchKernelGGL((dwconv7_wgrad_kernel<TT, TWV>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)dy, part_ws, (int)nt, H, W, C, tw, tw * thh)
  if (dtype == PFR_BF16) {
    if (TW == 7) PFR_DW_WG(bf16_t, 7); else PFR_DW_WG(bf16_t, 8);
  } else {
    if (TW == 7) PFR_DW_WG(float, 7); else PFR_DW_WG(float, 8);
  }
#undef PFR_DW_WG
  PFR_CHECK_LAUNCH();
  hipLaunchKernelGGL(dwconv7_wgrad_merge_kernel, dim3(DW_K * DW_K + 1, (unsigned)((C + 63) / 64)), dim3(256), 0, st, part_ws, dw, dbias, P, C,
                     accumulate);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ------------------------------------------------------------------------------------------------ layer scale (+ stochastic depth)
// y = residual + row_scale[n] * gamma[c] * u over [N][HW][C]; row_scale (fp32 [N], 0 or 1/(1-p)) may be NULL
template <typename T>
__global__ void layer_scale_fwd_kernel(const T* __restrict__ u, const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                       const T* __restrict__ residual, T* __restrict__ y, size_t nchunks, int CH, size_t chunks_per_n) {
  constexpr int KP = DT<T>::KPACK;
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < nchunks; i += stride) {
    const int c = (int)(i % CH) * KP;
    const float rs = row_scale ? row_scale[i / chunks_per_n] : 1.f;
    float a[KP], r[KP];
    Chunk<T>::unpack(ld16(u + i * KP), a);
    Chunk<T>::unpack(ld16(residual + i * KP), r);
#pragma unroll
    for (int k = 0; k < KP; ++k) r[k] = fmaf(rs * gamma[c + k], a[k], r[k]);
    st16(y + i * KP, Chunk<T>::pack(r));
  }
}

// du = row_scale * gamma * dz; part[b][C] = sum over the rows of workgroup b of row_scale * dz * u.  Thread (chunk column q, row slot s):
// the workgroup walks its row range RPI rows at a time, so a thread stays on its channels and sums in registers.
template <typename T>
__global__ __launch_bounds__(256) void layer_scale_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ u, const float* __restrict__ gamma,
                                                              const float* __restrict__ row_scale, T* __restrict__ du,
                                                              float* __restrict__ part, long rows, int HW, int C, int CH, int RPI, long rpb) {
  constexpr int KP = DT<T>::KPACK;
  extern __shared__ float lsred[];   // [RPI][C]
  const int q = threadIdx.x % CH, s = threadIdx.x / CH;
  float sum[KP], gm[KP];
#pragma unroll
  for (int k = 0; k < KP; ++k) sum[k] = 0.f;
  if (s < RPI) {
#pragma unroll
    for (int k = 0; k < KP; ++k) gm[k] = gamma[q * KP + k];
    const long r0 = (long)blockIdx.x * rpb;
    const long r1 = r0 + rpb < rows ? r0 + rpb : rows;
    for (long row = r0 + s; row < r1; row += RPI) {
      const float rs = row_scale ? row_scale[row / HW] : 1.f;
      const size_t off = (size_t)row * C + (size_t)q * KP;
      float g[KP], a[KP];
      Chunk<T>::unpack(ld16(dz + off), g);
      Chunk<T>::unpack(ld16(u + off), a);
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        const float sg = rs * g[k];
        sum[k] = fmaf(sg, a[k], sum[k]);
        g[k] = sg * gm[k];
      }
      st16(du + off, Chunk<T>::pack(g));
    }
#pragma unroll
    for (int k = 0; k < KP; ++k) lsred[s * C + q * KP + k] = sum[k];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float v = 0.f;
    for (int j = 0; j < RPI; ++j) v += lsred[j * C + c];
    part[(size_t)blockIdx.x * C + c] = v;
  }
}

__global__ void layer_scale_merge_kernel(const float* __restrict__ part, float* __restrict__ dgamma, int P, int C, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float v = 0.f;
  for (int p = 0; p < P; ++p) v += part[(size_t)p * C + c];
  dgamma[c] = accumulate ? dgamma[c] + v : v;
}

static int ls_check(const char* fn, std::initializer_list<const void*> ptrs, int dtype, int N, int HW, int C) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", fn);
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PFR_CHECK_ARG(N > 0 && HW > 0 && C > 0, "%s: empty tensor", fn);
  PFR_CHECK_ARG(C % kp == 0 && C / kp <= 256, "%s: C = %d must be a multiple of %d and at most %d", fn, C, kp, 256 * kp);
  PFR_CHECK_ARG(pfr_all_dev(ptrs), "%s: not a device pointer (no CPU fallback)", fn);
  return PFR_OK;
}

extern "C" int pfr_layer_scale_fwd(const void* u, const float* gamma, const float* row_scale, const void* residual, void* y, int dtype,
                                   int N, int HW, int C, hipStream_t st) {
  PFR_CHECK_ARG(u && gamma && residual && y, "pfr_layer_scale_fwd: null pointer");
  if (int rc = ls_check("pfr_layer_scale_fwd", {u, gamma, row_scale, residual, y}, dtype, N, HW, C)) return rc;
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  const int CH = C / kp;
  const size_t cpn = (size_t)HW * CH, nch = cpn * N;
  unsigned blocks = (unsigned)((nch + 255) / 256);
  if (blocks > 8192) blocks = 8192;
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(layer_scale_fwd_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)u, gamma, row_scale,
                       (const bf16_t*)residual, (bf16_t*)y, nch, CH, cpn);
  else
    hipLaunchKernelGGL(layer_scale_fwd_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)u, gamma, row_scale,
                       (const float*)residual, (float*)y, nch, CH, cpn);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// partial rows of the layer-scale gradient (dgamma_part: fp32 [parts][C])
extern "C" int pfr_layer_scale_bwd_parts(int N, int HW, int C) {
  (void)C;
  long nb = ((long)N * HW + 31) / 32;
  if (nb > 1024) nb = 1024;
  return (int)(nb < 1 ? 1 : nb);
}

// dgamma may be NULL: the caller merges dgamma_part itself (pfr_colsum_final_batch); otherwise the merge runs here and honours `accumulate`
extern "C" int pfr_layer_scale_bwd(const void* dz, const void* u, const float* gamma, const float* row_scale, void* du, float* dgamma_part,
                                   float* dgamma, int dtype, int N, int HW, int C, int accumulate, hipStream_t st) {
  PFR_CHECK_ARG(dz && u && gamma && du && dgamma_part, "pfr_layer_scale_bwd: null pointer");
  if (int rc = ls_check("pfr_layer_scale_bwd", {dz, u, gamma, row_scale, du, dgamma_part, dgamma}, dtype, N, HW, C)) return rc;
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  const int CH = C / kp, RPI = 256 / CH;
  const long rows = (long)N * HW;
  const int P = pfr_layer_scale_bwd_parts(N, HW, C);
  const long rpb = (rows + P - 1) / P;
  const size_t shb = (size_t)RPI * C * sizeof(float);
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(layer_scale_bwd_kernel<bf16_t>, dim3(P), dim3(256), shb, st, (const bf16_t*)dz, (const bf16_t*)u, gamma, row_scale,
                       (bf16_t*)du, dgamma_part, rows, HW, C, CH, RPI, rpb);
  else
    hipLaunchKernelGGL(layer_scale_bwd_kernel<float>, dim3(P), dim3(256), shb, st, (const float*)dz, (const float*)u, gamma, row_scale,
                       (float*)du, dgamma_part, rows, HW, C, CH, RPI, rpb);
  PFR_CHECK_LAUNCH();
  if (dgamma) {
    hipLaunchKernelGGL(layer_scale_merge_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, dgamma_part, dgamma, P, C, accumulate);
    PFR_CHECK_LAUNCH();
  }
  return PFR_OK;
}
