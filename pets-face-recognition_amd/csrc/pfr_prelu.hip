// PReLU forms of the BatchNorm apply / backward (IResNet: nn.PReLU(C) after nn.BatchNorm2d; a learnable slope per channel).
//   u = scale[c]*x + shift[c], s = slope[c]
//   forward   y  = u > 0 ? u : s*u
//   backward  g  = dout * (u > 0 ? 1 : s);  partials of (Σg, Σg·x̂) for pfr_bn_bwd_finalize and of Σ dout*min(u, 0), the slope
//             gradient (0 at u == 0: torch's convention);  dx = coef0*g + coef1*x + coef2
// u and the mask are recomputed from the BatchNorm input x: no activation and no mask tensor is read.  Memory-bound kernels in the
// form of the ReLU6 / SiLU kernels of pfr_elementwise.hip: thread = (16-byte channel chunk, row lane), 256 threads, several rows per
// thread in flight, deterministic partials without atomics.  Every pointer is checked to be device memory before a launch.
#include "pfr_common.h"

extern "C" int pfr_colreduce_blocks(int C, int dtype, long rows);   // pfr_elementwise.hip

namespace {

struct PreluGeom {
  int cw;      // chunk columns handled per block (power of two <= 256)
  int rl;      // row lanes per block = 256 / cw
  int cpr;     // chunks per row (C / KP)
  int gy;      // blocks along columns
  int gx;      // blocks along rows
};
// elementwise kernels: as many row blocks as fill the device, at least 4 rows per lane; the reduce takes gx from
// pfr_colreduce_blocks so that its partial rows are the ones pfr_bn_bwd_finalize is told about
PreluGeom prelu_geom(int C, int kp, size_t rows, size_t target) {
  PreluGeom g;
  g.cpr = C / kp;
  int cw = 1;
  while (cw < g.cpr && cw < 256) cw <<= 1;
  g.cw = cw;
  g.rl = 256 / cw;
  g.gy = (g.cpr + cw - 1) / cw;
  size_t want = target / g.gy;
  const size_t maxb = (rows + g.rl * 4 - 1) / (g.rl * 4);
  if (want > maxb) want = maxb;
  if (want < 1) want = 1;
  g.gx = (int)want;
  return g;
}

int prelu_check(const char* fn, int dtype, long rows, int C) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", fn);
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PFR_CHECK_ARG(rows > 0 && C > 0 && C % kp == 0, "%s: C %% %d != 0 or empty tensor", fn, kp);
  return PFR_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_act_prelu_kernel(const T* __restrict__ x, const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ slope, T* __restrict__ y, size_t rows, int C, int cw,
                                                           int rl, int cpr) {
  constexpr int KP = DT<T>::KPACK;
  const int col = threadIdx.x % cw, rlane = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  if (cglob >= cpr) return;
  float A[KP], B[KP], S[KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    A[e] = a[cglob * KP + e];
    B[e] = b[cglob * KP + e];
    S[e] = slope[cglob * KP + e];
  }
  auto body = [&](u32x4 v, size_t row) {
    float f[KP];
    Chunk<T>::unpack(v, f);
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      const float u = fmaf(f[e], A[e], B[e]);
      f[e] = u > 0.f ? u : S[e] * u;
    }
    st16(y + row * C + cglob * KP, Chunk<T>::pack(f));
  };
  const size_t step = (size_t)gridDim.x * rl;
  size_t r = (size_t)blockIdx.x * rl + rlane;
  for (; r + 3 * step < rows; r += 4 * step) {   // four rows per thread in flight
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = ld16_nt(x + (r + u * step) * C + cglob * KP);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) body(v[u], r + u * step);
  }
  for (; r < rows; r += step) body(ld16(x + r * C + cglob * KP), r);
}

// part: [gx][2][C] rows (Σg, Σg·x̂) of row block b — pfr_bn_bwd_finalize's layout — followed by [gx][C] rows Σ dout*min(u, 0)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_prelu_kernel(const T* __restrict__ dout, const T* __restrict__ x,
                                                                  const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const float* __restrict__ slope, float* __restrict__ part, size_t rows,
                                                                  int C, int cw, int rl, int cpr) {
  constexpr int KP = DT<T>::KPACK;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // [rl][cw][3*KP]
  const int col = threadIdx.x % cw, rlane = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  float v[3][KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) { v[0][e] = 0.f; v[1][e] = 0.f; v[2][e] = 0.f; }
  if (cglob < cpr) {
    float mu[KP], is[KP], sc[KP], sh[KP], sl[KP];
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      mu[e] = mean[cglob * KP + e];
      is[e] = invstd[cglob * KP + e];
      sc[e] = scale[cglob * KP + e];
      sh[e] = shift[cglob * KP + e];
      sl[e] = slope[cglob * KP + e];
    }
    auto body = [&](u32x4 vg, u32x4 vx) {
      float g[KP], xv[KP];
      Chunk<T>::unpack(vg, g);
      Chunk<T>::unpack(vx, xv);
#pragma unroll
      for (int e = 0; e < KP; ++e) {
        const float u = fmaf(xv[e], sc[e], sh[e]);
        const float gg = u > 0.f ? g[e] : g[e] * sl[e];
        v[0][e] += gg;
        v[1][e] = fmaf(gg, (xv[e] - mu[e]) * is[e], v[1][e]);
        v[2][e] = fmaf(g[e], fminf(u, 0.f), v[2][e]);
      }
    };
    const size_t step = (size_t)gridDim.x * rl;
    size_t r = (size_t)blockIdx.x * rl + rlane;
    for (; r + 3 * step < rows; r += 4 * step) {
      u32x4 vg[4], vx[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t off = (r + u * step) * C + cglob * KP;
        vg[u] = ld16_nt(dout + off);
        vx[u] = ld16_nt(x + off);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) body(vg[u], vx[u]);
    }
    for (; r < rows; r += step) {
      const size_t off = r * C + cglob * KP;
      body(ld16(dout + off), ld16(x + off));
    }
  }
  // over the row lanes, in lane order (deterministic)
  float* mine = lds + ((size_t)rlane * cw + col) * (3 * KP);
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int e = 0; e < KP; ++e) mine[q * KP + e] = v[q][e];
  __syncthreads();
  if (rlane == 0 && cglob < cpr) {
    float* bn_row = part + (size_t)blockIdx.x * 2 * C;
    float* sl_row = part + (size_t)gridDim.x * 2 * C + (size_t)blockIdx.x * C;
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int e = 0; e < KP; ++e) {
        float acc = 0.f;
        for (int r = 0; r < rl; ++r) acc += lds[((size_t)r * cw + col) * (3 * KP) + q * KP + e];
        if (q < 2) bn_row[(size_t)q * C + cglob * KP + e] = acc;
        else sl_row[cglob * KP + e] = acc;
      }
  }
}

// dslope[c] (+)= Σ_i rows[i][c]; block: 16 channels x 16 part lanes, the lanes summed in lane order
__global__ __launch_bounds__(256) void prelu_slope_finalize_kernel(const float* __restrict__ rows, int nparts, int C,
                                                                   float* __restrict__ dslope, int accumulate) {
  __shared__ float l[16][17];
  const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  float a = 0.f;
  if (c < C)
    for (int i = pl; i < nparts; i += 16) a += rows[(size_t)i * C + c];
  l[pl][cl] = a;
  __syncthreads();
  if (pl == 0 && c < C) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += l[i][cl];
    dslope[c] = accumulate ? dslope[c] + s : s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_prelu_kernel(const T* __restrict__ dout, const T* __restrict__ x,
                                                                 const float* __restrict__ coef, const float* __restrict__ scale,
                                                                 const float* __restrict__ shift, const float* __restrict__ slope,
                                                                 T* __restrict__ dx, size_t rows, int C, int cw, int rl, int cpr) {
  constexpr int KP = DT<T>::KPACK;
  const int col = threadIdx.x % cw, rlane = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  if (cglob >= cpr) return;
  float cg[KP], cx[KP], c0[KP], sc[KP], sh[KP], sl[KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    const int c = cglob * KP + e;
    cg[e] = coef[c];
    cx[e] = coef[C + c];
    c0[e] = coef[2 * C + c];
    sc[e] = scale[c];
    sh[e] = shift[c];
    sl[e] = slope[c];
  }
  auto body = [&](u32x4 vg, u32x4 vx, size_t off) {
    float g[KP], xv[KP];
    Chunk<T>::unpack(vg, g);
    Chunk<T>::unpack(vx, xv);
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      const float u = fmaf(xv[e], sc[e], sh[e]);
      const float gg = u > 0.f ? g[e] : g[e] * sl[e];
      xv[e] = fmaf(cg[e], gg, fmaf(cx[e], xv[e], c0[e]));
    }
    st16(dx + off, Chunk<T>::pack(xv));
  };
  const size_t step = (size_t)gridDim.x * rl;
  size_t r = (size_t)blockIdx.x * rl + rlane;
  for (; r + 3 * step < rows; r += 4 * step) {   // four rows per thread in flight (dx may alias dout: loads precede stores)
    u32x4 vg[4], vx[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const size_t off = (r + u * step) * C + cglob * KP;
      vg[u] = ld16_nt(dout + off);
      vx[u] = ld16_nt(x + off);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 4; ++u) body(vg[u], vx[u], (r + u * step) * C + cglob * KP);
  }
  for (; r < rows; r += step) {
    const size_t off = r * C + cglob * KP;
    body(ld16(dout + off), ld16(x + off), off);
  }
}

}  // namespace

extern "C" int pfr_bn_act_prelu(const void* x, const float* scale, const float* shift, const float* slope, void* y, int dtype, long rows,
                                int C, hipStream_t st) {
  PFR_CHECK_ARG(x && scale && shift && slope && y, "pfr_bn_act_prelu: null pointer");
  if (int rc = prelu_check("pfr_bn_act_prelu", dtype, rows, C)) return rc;
  PFR_CHECK_ARG(pfr_all_dev({x, scale, shift, slope, y}), "pfr_bn_act_prelu: not a device pointer (no CPU fallback)");
  const PreluGeom g = prelu_geom(C, dtype == PFR_BF16 ? 8 : 4, (size_t)rows, 512);
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(bn_act_prelu_kernel<bf16_t>, dim3(g.gx, g.gy), dim3(256), 0, st, (const bf16_t*)x, scale, shift, slope, (bf16_t*)y, (size_t)rows, C, g.cw, g.rl, g.cpr);
  else
    hipLaunchKernelGGL(bn_act_prelu_kernel<float>, dim3(g.gx, g.gy), dim3(256), 0, st, (const float*)x, scale, shift, slope, (float*)y, (size_t)rows, C, g.cw, g.rl, g.cpr);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_bn_bwd_reduce_prelu(const void* dout, const void* x, const float* mean, const float* invstd, const float* scale,
                                       const float* shift, const float* slope, int dtype, long rows, int C, float* part, hipStream_t st) {
  PFR_CHECK_ARG(dout && x && mean && invstd && scale && shift && slope && part, "pfr_bn_bwd_reduce_prelu: null pointer");
  if (int rc = prelu_check("pfr_bn_bwd_reduce_prelu", dtype, rows, C)) return rc;
  PFR_CHECK_ARG(pfr_all_dev({dout, x, mean, invstd, scale, shift, slope, part}), "pfr_bn_bwd_reduce_prelu: not a device pointer (no CPU fallback)");
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PreluGeom g = prelu_geom(C, kp, (size_t)rows, 512);
  g.gx = pfr_colreduce_blocks(C, dtype, rows);      // the partial-row count the caller sized `part` and pfr_bn_bwd_finalize with
  PFR_CHECK_ARG(g.gx >= 1, "pfr_bn_bwd_reduce_prelu: no row blocks");
  const size_t shb = (size_t)256 * 3 * kp * sizeof(float);
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(bn_bwd_reduce_prelu_kernel<bf16_t>, dim3(g.gx, g.gy), dim3(256), shb, st, (const bf16_t*)dout, (const bf16_t*)x, mean, invstd, scale, shift, slope, part, (size_t)rows, C, g.cw, g.rl, g.cpr);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_prelu_kernel<float>, dim3(g.gx, g.gy), dim3(256), shb, st, (const float*)dout, (const float*)x, mean, invstd, scale, shift, slope, part, (size_t)rows, C, g.cw, g.rl, g.cpr);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_prelu_slope_finalize(const float* part, int nparts, int C, float* dslope, int accumulate, hipStream_t st) {
  PFR_CHECK_ARG(part && dslope, "pfr_prelu_slope_finalize: null pointer");
  PFR_CHECK_ARG(nparts > 0 && C > 0, "pfr_prelu_slope_finalize: nparts and C must be positive");
  PFR_CHECK_ARG(pfr_all_dev({part, dslope}), "pfr_prelu_slope_finalize: not a device pointer (no CPU fallback)");
  hipLaunchKernelGGL(prelu_slope_finalize_kernel, dim3((C + 15) / 16), dim3(256), 0, st, part + (size_t)nparts * 2 * C, nparts, C, dslope, accumulate);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_bn_bwd_apply_prelu(const void* dout, const void* x, const float* coef, const float* scale, const float* shift,
                                      const float* slope, void* dx, int dtype, long rows, int C, hipStream_t st) {
  PFR_CHECK_ARG(dout && x && coef && scale && shift && slope && dx, "pfr_bn_bwd_apply_prelu: null pointer");
  if (int rc = prelu_check("pfr_bn_bwd_apply_prelu", dtype, rows, C)) return rc;
  PFR_CHECK_ARG(pfr_all_dev({dout, x, coef, scale, shift, slope, dx}), "pfr_bn_bwd_apply_prelu: not a device pointer (no CPU fallback)");
  const PreluGeom g = prelu_geom(C, dtype == PFR_BF16 ? 8 : 4, (size_t)rows, 256);
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(bn_bwd_apply_prelu_kernel<bf16_t>, dim3(g.gx, g.gy), dim3(256), 0, st, (const bf16_t*)dout, (const bf16_t*)x, coef, scale, shift, slope, (bf16_t*)dx, (size_t)rows, C, g.cw, g.rl, g.cpr);
  else
    hipLaunchKernelGGL(bn_bwd_apply_prelu_kernel<float>, dim3(g.gx, g.gy), dim3(256), 0, st, (const float*)dout, (const float*)x, coef, scale, shift, slope, (float*)dx, (size_t)rows, C, g.cw, g.rl, g.cpr);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
