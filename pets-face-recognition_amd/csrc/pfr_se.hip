// pfr_se.hip — squeeze-and-excitation of the MBConv block (torchvision ops/misc.py SqueezeExcitation with SiLU / Sigmoid) and the
// per-sample ("row" mode) stochastic depth on the project BatchNorm, for the EfficientNet engine (models/_efficientnet_engine.py).
// gfx950, VALU / HBM work.  Activations NHWC [N][HW][C] in fp32 or bf16, C a multiple of the 16-byte chunk; everything of size [N][C]
// or [N][S] that the gate produces is fp32, and the two 1x1 convolutions read their fp32 master weights as they stand ([S][C] and
// [C][S]): the squeeze width S is any positive integer (8, 4, 6, 12, 22, 30, 52, 88 in B2), so they cannot be 16-byte-chunk GEMMs, and
// they are a few kFLOP per sample.  The squeeze itself is pfr_avgpool_fwd.  Deterministic: wave reductions are fixed shuffle trees,
// sums over N and over HW run in a fixed order, no atomics.
#include "pfr_common.h"
#include <initializer_list>

__device__ __forceinline__ float se_sigmoid(float u) { return __builtin_amdgcn_rcpf(1.f + __expf(-u)); }
__device__ __forceinline__ float se_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ gate
// workgroup = sample n.  Phase 1: wave per squeeze channel s (lanes over C, shuffle tree): pre[n][s] = b1[s] + Σ_c w1[s][c] pooled[n][c].
// Phase 2: silu(pre[n][:]) staged in LDS once per tile of 1024 squeeze channels (one tile for every S of the network), then thread per
// channel c: gate[n][c] = σ(b2[c] + Σ_s w2[c][s] silu(pre[n][s])); with more than one tile the running sum waits in gate[n][c]
template <typename T>
__global__ __launch_bounds__(256) void se_gate_fwd_kernel(const T* __restrict__ pooled, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* __restrict__ pre, float* __restrict__ gate,
                                                          int C, int S) {
  __shared__ float h[1024];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const T* p = pooled + (size_t)n * C;
  for (int s = wv; s < S; s += 4) {
    float v = 0.f;
    for (int c = lane; c < C; c += 64) v = fmaf(w1[(size_t)s * C + c], (float)p[c], v);
    v = se_wave_sum(v);
    if (lane == 0) pre[(size_t)n * S + s] = v + b1[s];
  }
  __threadfence_block();
  __syncthreads();
  for (int s0 = 0; s0 < S; s0 += 1024) {
    const int ns = S - s0 < 1024 ? S - s0 : 1024;
    __syncthreads();
    for (int s = threadIdx.x; s < ns; s += 256) {
      const float u = pre[(size_t)n * S + s0 + s];
      h[s] = u * se_sigmoid(u);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {     // a thread keeps its channels over the tiles
      float z = s0 == 0 ? b2[c] : gate[(size_t)n * C + c];
      for (int s = 0; s < ns; ++s) z = fmaf(w2[(size_t)c * S + s0 + s], h[s], z);
      gate[(size_t)n * C + c] = s0 + ns == S ? se_sigmoid(z) : z;
    }
  }
}

// backward of the gate, workgroup = sample n.  dz[n][c] = dgate g (1 - g).  Phase 1: wave per s: dpre[n][s] = silu'(pre) Σ_c dz[n][c] w2[c][s]
// (into the workspace).  Phase 2: thread per c: dpooled[n][c] = Σ_s dpre[n][s] w1[s][c]
__global__ __launch_bounds__(256) void se_gate_bwd_kernel(const float* __restrict__ dgate, const float* __restrict__ pre,
                                                          const float* __restrict__ gate, const float* __restrict__ w1,
                                                          const float* __restrict__ w2, float* __restrict__ dpre,
                                                          float* __restrict__ dpooled, int C, int S) {
  const int n = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* dg = dgate + (size_t)n * C;
  const float* g = gate + (size_t)n * C;
  for (int s = wv; s < S; s += 4) {
    float v = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float gc = g[c];
      v = fmaf(dg[c] * gc * (1.f - gc), w2[(size_t)c * S + s], v);
    }
    v = se_wave_sum(v);
    if (lane == 0) {
      const float u = pre[(size_t)n * S + s], sg = se_sigmoid(u);
      dpre[(size_t)n * S + s] = v * sg * fmaf(u, 1.f - sg, 1.f);
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float v = 0.f;
    for (int s = 0; s < S; ++s) v = fmaf(dpre[(size_t)n * S + s], w1[(size_t)s * C + c], v);
    dpooled[(size_t)n * C + c] = v;
  }
}

// the four parameter gradients, one thread per element, the sum over N in ascending order:
//   dw2[c][s] = Σ_n dz[n][c] silu(pre[n][s]),  dw1[s][c] = Σ_n dpre[n][s] pooled[n][c],  db2[c] = Σ_n dz[n][c],  db1[s] = Σ_n dpre[n][s]
template <typename T>
__global__ __launch_bounds__(256) void se_param_grad_kernel(const float* __restrict__ dgate, const T* __restrict__ pooled,
                                                            const float* __restrict__ pre, const float* __restrict__ gate,
                                                            const float* __restrict__ dpre, float* __restrict__ dw1,
                                                            float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2,
                                                            int N, int C, int S, int accumulate) {
  const long CS = (long)C * S;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  float v = 0.f;
  float* out;
  if (i < CS) {
    const int c = (int)(i / S), s = (int)(i - (long)c * S);
    for (int n = 0; n < N; ++n) {
      const float gc = gate[(size_t)n * C + c], u = pre[(size_t)n * S + s];
      v = fmaf(dgate[(size_t)n * C + c] * gc * (1.f - gc), u * se_sigmoid(u), v);
    }
    out = dw2 + i;
  } else if (i < 2 * CS) {
    i -= CS;
    const int s = (int)(i / C), c = (int)(i - (long)s * C);
    for (int n = 0; n < N; ++n) v = fmaf(dpre[(size_t)n * S + s], (float)pooled[(size_t)n * C + c], v);
    out = dw1 + i;
  } else if (i < 2 * CS + C) {
    const int c = (int)(i - 2 * CS);
    for (int n = 0; n < N; ++n) {
      const float gc = gate[(size_t)n * C + c];
      v += dgate[(size_t)n * C + c] * gc * (1.f - gc);
    }
    out = db2 + c;
  } else if (i < 2 * CS + C + S) {
    const int s = (int)(i - 2 * CS - C);
    for (int n = 0; n < N; ++n) v += dpre[(size_t)n * S + s];
    out = db1 + s;
  } else {
    return;
  }
  *out = accumulate ? *out + v : v;
}

// ------------------------------------------------------------------------------------------------ per-sample element-wise passes
// one 16-byte chunk per thread and iteration over [N][HW][C]:
//   MODE 0  y = x * g[n][c]                                  (pfr_se_scale_fwd)
//   MODE 1  y = x * g[n][c] + q[n][c] / HW                   (pfr_se_bwd_apply: x = dy, g = gate, q = dpooled)
//   MODE 2  y = r + rs[n] * (g[c] * x + q[c])                (pfr_bn_residual_rows: g = a, q = b, r = residual)
//   MODE 3  y = rs[n] * x                                    (pfr_row_scale)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void se_rows_kernel(const T* __restrict__ x, const float* __restrict__ g, const float* __restrict__ q,
                                                      const T* __restrict__ r, const float* __restrict__ rs, T* __restrict__ y,
                                                      uint32_t total, uint32_t cpr, uint32_t HW, int C, float inv_hw) {
  constexpr int KP = DT<T>::KPACK;
  const uint32_t step = gridDim.x * 256u;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += step) {
    const uint32_t row = i / cpr, col = i - row * cpr, n = row / HW;
    const size_t off = (size_t)row * C + col * KP;
    float f[KP];
    Chunk<T>::unpack(ld16(x + off), f);
    if constexpr (MODE == 0 || MODE == 1) {
      const float* gp = g + (size_t)n * C + col * KP;
#pragma unroll
      for (int e = 0; e < KP; ++e) f[e] *= gp[e];
      if constexpr (MODE == 1) {
        const float* qp = q + (size_t)n * C + col * KP;
#pragma unroll
        for (int e = 0; e < KP; ++e) f[e] = fmaf(qp[e], inv_hw, f[e]);
      }
    } else if constexpr (MODE == 2) {
      float rv[KP];
      Chunk<T>::unpack(ld16(r + off), rv);
      const float sc = rs[n];
#pragma unroll
      for (int e = 0; e < KP; ++e) f[e] = fmaf(sc, fmaf(g[col * KP + e], f[e], q[col * KP + e]), rv[e]);
    } else {
      const float sc = rs[n];
#pragma unroll
      for (int e = 0; e < KP; ++e) f[e] *= sc;
    }
    st16(y + off, Chunk<T>::pack(f));
  }
}

// dgate[n][c] = Σ_hw dy[n][hw][c] a[n][hw][c]: workgroup (n, column block), thread (chunk column, row lane) over the sample's rows,
// the row lanes folded through LDS in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void se_scale_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ a, float* __restrict__ dgate,
                                                                  int HW, int C, int cw, int rl, int cpr) {
  constexpr int KP = DT<T>::KPACK;
  __shared__ float red[256 * KP];
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col, n = blockIdx.x;
  float acc[KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) acc[e] = 0.f;
  if (s < rl && cglob < cpr) {
    for (int hw = s; hw < HW; hw += rl) {
      const size_t off = ((size_t)n * HW + hw) * C + cglob * KP;
      float f[KP], v[KP];
      Chunk<T>::unpack(ld16(dy + off), f);
      Chunk<T>::unpack(ld16(a + off), v);
#pragma unroll
      for (int e = 0; e < KP; ++e) acc[e] = fmaf(f[e], v[e], acc[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < KP; ++e) red[threadIdx.x * KP + e] = acc[e];
  __syncthreads();
  if (s != 0 || cglob >= cpr) return;
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    float v = 0.f;
    for (int j = 0; j < rl; ++j) v += red[(j * cw + col) * KP + e];
    dgate[(size_t)n * C + cglob * KP + e] = v;
  }
}

// ------------------------------------------------------------------------------------------------ entry points
static int se_check(const char* fn, std::initializer_list<const void*> ptrs, int dtype, long N, long HW, long C) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", fn);
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PFR_CHECK_ARG(N > 0 && HW > 0 && C > 0, "%s: empty tensor", fn);
  PFR_CHECK_ARG(C % kp == 0, "%s: C = %ld is not a multiple of %d (16-byte channel chunks)", fn, C, kp);
  // the element-wise kernels walk the chunks with a 32-bit index and a stride of at most 8192 * 256: the index must not wrap
  PFR_CHECK_ARG(N * HW * (C / kp) < (1l << 32) - (1l << 21) && N * HW < (1l << 31), "%s: more than 2^32 - 2^21 chunks", fn);
  PFR_CHECK_ARG(pfr_all_dev(ptrs), "%s: not a device pointer (no CPU fallback)", fn);
  return PFR_OK;
}

extern "C" int pfr_se_gate_fwd(const void* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* pre,
                               float* gate, int dtype, int N, int C, int S, hipStream_t st) {
  PFR_CHECK_ARG(pooled && w1 && b1 && w2 && b2 && pre && gate, "pfr_se_gate_fwd: null pointer");
  PFR_CHECK_ARG(S > 0, "pfr_se_gate_fwd: S must be positive");
  if (int rc = se_check("pfr_se_gate_fwd", {pooled, w1, b1, w2, b2, pre, gate}, dtype, N, 1, C)) return rc;
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(se_gate_fwd_kernel<bf16_t>, dim3((unsigned)N), dim3(256), 0, st, (const bf16_t*)pooled, w1, b1, w2, b2, pre, gate, C, S);
  else
    hipLaunchKernelGGL(se_gate_fwd_kernel<float>, dim3((unsigned)N), dim3(256), 0, st, (const float*)pooled, w1, b1, w2, b2, pre, gate, C, S);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_se_gate_bwd(const float* dgate, const void* pooled, const float* pre, const float* gate, const float* w1,
                               const float* w2, float* dpre_ws, float* dpooled, float* dw1, float* db1, float* dw2, float* db2, int dtype,
                               int N, int C, int S, int accumulate, hipStream_t st) {
  PFR_CHECK_ARG(dgate && pooled && pre && gate && w1 && w2 && dpre_ws && dpooled && dw1 && db1 && dw2 && db2, "pfr_se_gate_bwd: null pointer");
  PFR_CHECK_ARG(S > 0, "pfr_se_gate_bwd: S must be positive");
  if (int rc = se_check("pfr_se_gate_bwd", {dgate, pooled, pre, gate, w1, w2, dpre_ws, dpooled, dw1, db1, dw2, db2}, dtype, N, 1, C)) return rc;
  hipLaunchKernelGGL(se_gate_bwd_kernel, dim3((unsigned)N), dim3(256), 0, st, dgate, pre, gate, w1, w2, dpre_ws, dpooled, C, S);
  PFR_CHECK_LAUNCH();
  const long total = 2l * C * S + C + S;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(se_param_grad_kernel<bf16_t>, grid, dim3(256), 0, st, dgate, (const bf16_t*)pooled, pre, gate, dpre_ws, dw1, db1, dw2, db2, N, C, S, accumulate);
  else
    hipLaunchKernelGGL(se_param_grad_kernel<float>, grid, dim3(256), 0, st, dgate, (const float*)pooled, pre, gate, dpre_ws, dw1, db1, dw2, db2, N, C, S, accumulate);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

template <int MODE>
static int se_rows_launch(const void* x, const float* g, const float* q, const void* r, const float* rs, void* y, int dtype, int N, int HW,
                          int C, hipStream_t st) {
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  const uint32_t cpr = (uint32_t)(C / kp), total = (uint32_t)((long)N * HW * cpr);
  unsigned blocks = (total + 255u) / 256u;
  if (blocks > 8192u) blocks = 8192u;
  const float inv = 1.f / (float)HW;
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL((se_rows_kernel<bf16_t, MODE>), dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, g, q, (const bf16_t*)r, rs, (bf16_t*)y, total, cpr, (uint32_t)HW, C, inv);
  else
    hipLaunchKernelGGL((se_rows_kernel<float, MODE>), dim3(blocks), dim3(256), 0, st, (const float*)x, g, q, (const float*)r, rs, (float*)y, total, cpr, (uint32_t)HW, C, inv);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_se_scale_fwd(const void* a, const float* gate, void* y, int dtype, int N, int HW, int C, hipStream_t st) {
  PFR_CHECK_ARG(a && gate && y, "pfr_se_scale_fwd: null pointer");
  if (int rc = se_check("pfr_se_scale_fwd", {a, gate, y}, dtype, N, HW, C)) return rc;
  return se_rows_launch<0>(a, gate, nullptr, nullptr, nullptr, y, dtype, N, HW, C, st);
}

extern "C" int pfr_se_bwd_apply(const void* dy, const float* gate, const float* dpooled, void* da, int dtype, int N, int HW, int C,
                                hipStream_t st) {
  PFR_CHECK_ARG(dy && gate && dpooled && da, "pfr_se_bwd_apply: null pointer");
  if (int rc = se_check("pfr_se_bwd_apply", {dy, gate, dpooled, da}, dtype, N, HW, C)) return rc;
  return se_rows_launch<1>(dy, gate, dpooled, nullptr, nullptr, da, dtype, N, HW, C, st);
}

extern "C" int pfr_bn_residual_rows(const void* z, const float* a, const float* b, const void* residual, const float* row_scale, void* y,
                                    int dtype, int N, int HW, int C, hipStream_t st) {
  PFR_CHECK_ARG(z && a && b && residual && row_scale && y, "pfr_bn_residual_rows: null pointer");
  if (int rc = se_check("pfr_bn_residual_rows", {z, a, b, residual, row_scale, y}, dtype, N, HW, C)) return rc;
  return se_rows_launch<2>(z, a, b, residual, row_scale, y, dtype, N, HW, C, st);
}

extern "C" int pfr_row_scale(const void* x, const float* row_scale, void* y, int dtype, int N, int HW, int C, hipStream_t st) {
  PFR_CHECK_ARG(x && row_scale && y, "pfr_row_scale: null pointer");
  if (int rc = se_check("pfr_row_scale", {x, row_scale, y}, dtype, N, HW, C)) return rc;
  return se_rows_launch<3>(x, nullptr, nullptr, nullptr, row_scale, y, dtype, N, HW, C, st);
}

extern "C" int pfr_se_scale_bwd_reduce(const void* dy, const void* a, float* dgate, int dtype, int N, int HW, int C, hipStream_t st) {
  PFR_CHECK_ARG(dy && a && dgate, "pfr_se_scale_bwd_reduce: null pointer");
  if (int rc = se_check("pfr_se_scale_bwd_reduce", {dy, a, dgate}, dtype, N, HW, C)) return rc;
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  const int cpr = C / kp, cw = cpr < 256 ? cpr : 256, rl = 256 / cw, gy = (cpr + cw - 1) / cw;
  const dim3 grid((unsigned)N, (unsigned)gy);
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(se_scale_bwd_reduce_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)dy, (const bf16_t*)a, dgate, HW, C, cw, rl, cpr);
  else
    hipLaunchKernelGGL(se_scale_bwd_reduce_kernel<float>, grid, dim3(256), 0, st, (const float*)dy, (const float*)a, dgate, HW, C, cw, rl, cpr);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
