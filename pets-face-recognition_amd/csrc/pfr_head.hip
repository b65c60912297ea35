// pfr_head.hip — the ArcFace / CosFace cosine-margin head with softmax cross-entropy (focal) loss.
//
// Reference semantics (file:line in /root/reference):
//   losses/large_margin.py:69-84  ArcMarginProduct.forward  — cos = normalize(x)·normalize(W)ᵀ ; sine = sqrt(1−cos²) ;
//        phi = cos·cos m − sine·sin m ; hard: where(cos > cos(π−m), phi, cos − sin(π−m)·m) ; easy: where(cos > 0, phi, cos) ;
//        out = s·(onehot·phi + (1−onehot)·cos)
//   losses/large_margin.py:30-40  AddMarginProduct.forward  — phi = cos − m
//   losses/losses.py:22-28        FocalLoss.forward         — logp = CE(·,'none') ; p = exp(−logp) ; mean((1−p)^γ·logp)
//   F.normalize: x / max(‖x‖₂, 1e-12)
//
// Kernels here: row L2-normalisation (forward: writes the compute-dtype x̂ and, for the weight, also x̂ᵀ; backward:
// dx = (dx̂ − x̂·(x̂·dx̂))/‖x‖) with wave-shuffle reductions, and ONE fused row kernel for
// margin → scale → log-softmax → loss → ∂loss/∂cos (the three B×C temporaries of the reference never exist).  The criterion of that
// kernel is a template switch: plain / focal CE, focal CE of alpha·logits (learnable alpha; its gradient is a column kernel of its
// own), nn.CrossEntropyLoss with class weights and label smoothing; the loss reduction (mean / sum / weighted mean) stays on the device.
// The two cosine GEMMs and their gradients run on the MFMA implicit-GEMM kernels (pfr_igemm.hip / pfr_wgrad.hip).
#include "pfr_common.h"

// one wave per row; D arbitrary
template <typename TI, typename TOo>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const TI* __restrict__ x, TOo* __restrict__ xn, TOo* __restrict__ xnT,
                                                         float* __restrict__ inv_norm, int rows, int D, int ldt, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const TI* xr = x + (size_t)row * D;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float v = to_f32(xr[d]);
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  const float inv = 1.f / fmaxf(sqrtf(ss), eps);
  if (lane == 0) inv_norm[row] = inv;
  for (int d = lane; d < D; d += 64) {
    const TOo o = from_f32<TOo>(to_f32(xr[d]) * inv);
    xn[(size_t)row * D + d] = o;
    if (xnT) xnT[(size_t)d * ldt + row] = o;
  }
}

extern "C" int pfr_l2norm_dual(const float* x, void* xn_bf16, float* xn_f32, float* inv_norm, int rows, int D, float eps, hipStream_t st);
extern "C" int pfr_l2norm_fwd(const void* x, int in_dtype, void* xn, void* xnT, int out_dtype, float* inv_norm, int rows,
                              int D, int ldt, float eps, hipStream_t st) {
  PFR_CHECK_ARG(x && xn && inv_norm, "pfr_l2norm_fwd: null pointer");
  // fp32 rows without the transposed copy: the register-resident float4 kernel of the match (one read of x, all loads in flight)
  if (in_dtype == PFR_F32 && !xnT && D % 4 == 0 && D <= 2048 && rows > 0 && (out_dtype == PFR_F32 || out_dtype == PFR_BF16))
    return pfr_l2norm_dual((const float*)x, out_dtype == PFR_BF16 ? xn : nullptr, out_dtype == PFR_F32 ? (float*)xn : nullptr, inv_norm, rows, D, eps, st);
  const dim3 grid((rows + 3) / 4), block(256);
  if (ldt <= 0) ldt = rows;
#define L2N(TI, TOo) hipLaunchKernelGGL((l2norm_fwd_kernel<TI, TOo>), grid, block, 0, st, (const TI*)x, (TOo*)xn, (TOo*)xnT, inv_norm, rows, D, ldt, eps)
  if (in_dtype == PFR_F32 && out_dtype == PFR_F32) L2N(float, float);
  else if (in_dtype == PFR_F32 && out_dtype == PFR_BF16) L2N(float, bf16_t);
  else if (in_dtype == PFR_BF16 && out_dtype == PFR_BF16) L2N(bf16_t, bf16_t);
  else if (in_dtype == PFR_BF16 && out_dtype == PFR_F32) L2N(bf16_t, float);
  else { pfr_set_error("pfr_l2norm_fwd: bad dtypes"); return PFR_ERR_UNSUPPORTED; }
#undef L2N
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// gallery / query preparation of the match: ONE pass over fp32 rows (float4 loads kept in registers) writes the normalised
// row in bf16 (GEMM operand) AND in fp32 (exact re-scoring operand).  D % 4 == 0, D <= 2048.
// NK = 16-byte-x4 chunks per lane (2 for D <= 512, 8 up to 2048): the loads are unconditional (clamped index, zeroed by a select) so
// that they are all in flight together — a load in a branch is followed by a full wait, i.e. one memory round trip per chunk
template <int NK>
__global__ __launch_bounds__(256) void l2norm_dual_kernel(const float* __restrict__ x, bf16_t* __restrict__ xb, float* __restrict__ xf,
                                                          float* __restrict__ inv_norm, int rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
  const int n4 = D >> 2;
  f32x4 v[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) v[k] = xr[min(lane + 64 * k, n4 - 1)];
  __builtin_amdgcn_sched_barrier(0);
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (lane + 64 * k >= n4) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) ss = fmaf(v[k][e], v[k][e], ss);
  }
  ss = wave_sum(ss);
  const float inv = 1.f / fmaxf(sqrtf(ss), eps);
  if (lane == 0 && inv_norm) inv_norm[row] = inv;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = lane + 64 * k;
    if (i < n4) {
      f32x4 o = v[k] * inv;
      if (xf) reinterpret_cast<f32x4*>(xf + (size_t)row * D)[i] = o;
      if (xb) {
        bf16x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (bf16_t)o[e];
        reinterpret_cast<bf16x4*>(xb + (size_t)row * D)[i] = b;
      }
    }
  }
}
extern "C" int pfr_l2norm_dual(const float* x, void* xn_bf16, float* xn_f32, float* inv_norm, int rows, int D, float eps,
                               hipStream_t st) {
  PFR_CHECK_ARG(x && (xn_bf16 || xn_f32) && rows > 0, "pfr_l2norm_dual: null pointer");
  PFR_CHECK_ARG(D % 4 == 0 && D <= 2048, "pfr_l2norm_dual: D must be a multiple of 4 and <= 2048");
  if (D <= 512) hipLaunchKernelGGL(l2norm_dual_kernel<2>, dim3((rows + 3) / 4), dim3(256), 0, st, x, (bf16_t*)xn_bf16, xn_f32, inv_norm, rows, D, eps);
  else hipLaunchKernelGGL(l2norm_dual_kernel<8>, dim3((rows + 3) / 4), dim3(256), 0, st, x, (bf16_t*)xn_bf16, xn_f32, inv_norm, rows, D, eps);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// int8 selection operand of the gallery match (the quantiser's definition: include/pfr_hip.h at pfr_quantize_rows_i8).  One pass per row
// as l2norm_dual (float4 loads kept in registers, the same norm arithmetic): x̂ = x · inv (normalize) or x, then m = max |x̂_i| (a wave
// maximum: exact), q_i = rint(x̂_i · (127 / m)), s = m / 127.  Writes the int8 row with leading dimension ldq (columns D .. ldq zero), the
// scale, and optionally the fp32 row x̂ and the inverse norm.
template <int NK>
__global__ __launch_bounds__(256) void quantize_rows_i8_kernel(const float* __restrict__ x, int8_t* __restrict__ q, int ldq, float* __restrict__ scale,
                                                               float* __restrict__ xf, float* __restrict__ inv_norm, int rows, int D, int normalize,
                                                               float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
  const int n4 = D >> 2;
  f32x4 v[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) v[k] = xr[min(lane + 64 * k, n4 - 1)];
  __builtin_amdgcn_sched_barrier(0);
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (lane + 64 * k >= n4) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) ss = fmaf(v[k][e], v[k][e], ss);
  }
  if (normalize) {
    ss = wave_sum(ss);
    const float inv = 1.f / fmaxf(sqrtf(ss), eps);
    if (lane == 0 && inv_norm) inv_norm[row] = inv;
#pragma unroll
    for (int k = 0; k < NK; ++k) v[k] = v[k] * inv;
  }
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(v[k][e]));
  m = wave_max(m);
  const float r = 127.f / m;
  const bool live = r < INFINITY;          // m == 0 (or so small that 127 / m overflows): an all-zero row with scale 0
  const float rq = live ? r : 0.f;
  if (lane == 0) scale[row] = live ? m / 127.f : 0.f;
  uint32_t* qr = reinterpret_cast<uint32_t*>(q + (size_t)row * ldq);
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = lane + 64 * k;
    if (i < n4) {
      if (xf) reinterpret_cast<f32x4*>(xf + (size_t)row * D)[i] = v[k];
      uint32_t w = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) w |= (uint32_t)(uint8_t)(int8_t)(int)rintf(v[k][e] * rq) << (8 * e);
      qr[i] = w;
    }
  }
  for (int i = n4 + lane; i < (ldq >> 2); i += 64) qr[i] = 0u;
}
extern "C" int pfr_quantize_rows_i8(const float* x, void* q, int ldq, float* scale, float* xn_f32, float* inv_norm, int rows, int D, int normalize,
                                    float eps, hipStream_t st) {
  PFR_CHECK_ARG(x && q && scale && rows > 0, "pfr_quantize_rows_i8: null pointer");
  PFR_CHECK_ARG(D > 0 && D % 4 == 0 && D <= 2048 && ldq >= D && ldq % 4 == 0,
                "pfr_quantize_rows_i8: D must be a multiple of 4 and <= 2048, ldq >= D a multiple of 4");
  if (D <= 512) hipLaunchKernelGGL(quantize_rows_i8_kernel<2>, dim3((rows + 3) / 4), dim3(256), 0, st, x, (int8_t*)q, ldq, scale, xn_f32, inv_norm, rows, D, normalize, eps);
  else hipLaunchKernelGGL(quantize_rows_i8_kernel<8>, dim3((rows + 3) / 4), dim3(256), 0, st, x, (int8_t*)q, ldq, scale, xn_f32, inv_norm, rows, D, normalize, eps);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// dx = inv_norm · (dxn − xn · (xn·dxn)) ; xn is the normalised row recomputed in fp32 from x and inv_norm
template <typename TI, typename TOo>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const TI* __restrict__ x, const float* __restrict__ inv_norm,
                                                         const float* __restrict__ dxn, TOo* __restrict__ dx, int rows, int D,
                                                         int accumulate) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float inv = inv_norm[row];
  const TI* xr = x + (size_t)row * D;
  const float* gr = dxn + (size_t)row * D;
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot = fmaf(to_f32(xr[d]) * inv, gr[d], dot);
  dot = wave_sum(dot);
  for (int d = lane; d < D; d += 64) {
    float v = inv * (gr[d] - to_f32(xr[d]) * inv * dot);
    if (accumulate) v += to_f32(dx[(size_t)row * D + d]);
    dx[(size_t)row * D + d] = from_f32<TOo>(v);
  }
}

extern "C" int pfr_l2norm_bwd(const void* x, int in_dtype, const float* inv_norm, const float* dxn, void* dx, int out_dtype,
                              int rows, int D, int accumulate, hipStream_t st) {
  PFR_CHECK_ARG(x && inv_norm && dxn && dx, "pfr_l2norm_bwd: null pointer");
  const dim3 grid((rows + 3) / 4), block(256);
#define L2B(TI, TOo) hipLaunchKernelGGL((l2norm_bwd_kernel<TI, TOo>), grid, block, 0, st, (const TI*)x, inv_norm, dxn, (TOo*)dx, rows, D, accumulate)
  if (in_dtype == PFR_F32 && out_dtype == PFR_F32) L2B(float, float);
  else if (in_dtype == PFR_BF16 && out_dtype == PFR_BF16) L2B(bf16_t, bf16_t);
  else if (in_dtype == PFR_BF16 && out_dtype == PFR_F32) L2B(bf16_t, float);
  else if (in_dtype == PFR_F32 && out_dtype == PFR_BF16) L2B(float, bf16_t);
  else { pfr_set_error("pfr_l2norm_bwd: bad dtypes"); return PFR_ERR_UNSUPPORTED; }
#undef L2B
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ------------------------------------------------------------------------------------------------
struct MarginParams {
  float s, cos_m, sin_m, th, mm, m;
  int mode;  // 0 = ArcFace hard margin, 1 = ArcFace easy margin, 2 = CosFace (cos − m), 3 = no margin
  float gamma;
};

__device__ __forceinline__ float block_reduce_max(float v, float* sh) {
  v = wave_max(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fmaxf(r, sh[i]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float block_reduce_sum(float v, float* sh) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += sh[i];
  __syncthreads();
  return r;
}

// The criterion of the row kernel, a compile-time switch (CRIT_PLAIN is the code every FE config of the reference runs):
//   CRIT_PLAIN  focal / plain cross-entropy of the margin logits l                      (losses/losses.py:22-28 with alpha=None)
//   CRIT_ALPHA  the same on z = alpha·l, alpha a learnable [C] vector                   (losses/losses.py:13-24 with alpha=True)
//   CRIT_WCE    nn.CrossEntropyLoss(weight=w, label_smoothing=e) on l (torch semantics):
//               row = (1−e)·w_t·(lse − l_t) + (e/C)·(W·lse − Σ_c w_c·l_c), W = Σ_c w_c ; 'mean' divides Σ rows by Σ_i w_{t_i}
//               ∂row/∂l_c = S·softmax(l)_c − (1−e)·w_t·[c==t] − (e/C)·w_c, S = (1−e)·w_t + (e/C)·W
enum { CRIT_PLAIN = 0, CRIT_ALPHA = 1, CRIT_WCE = 2 };
struct CritParams {
  const float* alpha;       // [C], CRIT_ALPHA
  const float* weight;      // [C] or null (= all ones), CRIT_WCE
  float smoothing;          // e, CRIT_WCE
  float* row_stats;         // [B][4] or null: {lse, gradient factor of the row (focal f / S), target margin logit l_t, w_t}
  const float* gscale_dev2; // second device-side factor of the gradient scale (1 / Σ w_t of the weighted mean) or null
};

// one block per sample row: 256 threads, or 1024 for long rows (three dependent passes over the row — at 10 000 classes and
// one wave per SIMD each pass is ~40 exposed memory round trips: 30 us with 256 threads)
template <typename TG, int CRIT>
__global__ __launch_bounds__(1024) void margin_ce_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                        MarginParams mp, float* __restrict__ logits, float* __restrict__ loss_rows,
                                                        TG* __restrict__ dcos, int C, int ldc, float gscale,
                                                        const float* __restrict__ gscale_dev, CritParams cp) {
  __shared__ float sh[16];
  if (gscale_dev) gscale *= gscale_dev[0];
  if (CRIT == CRIT_WCE && cp.gscale_dev2) gscale *= cp.gscale_dev2[0];
  const int row = blockIdx.x;
  const int nt = blockDim.x;
  const float* cr = cosv + (size_t)row * ldc;
  const int t = (int)label[row];
  // target logit and d(phi)/d(cos)
  const float ct = cr[t];
  float phi, dphi;
  if (mp.mode == 2) {
    phi = ct - mp.m;
    dphi = 1.f;
  } else if (mp.mode == 3) {
    phi = ct;
    dphi = 1.f;
  } else {
    const float sine = sqrtf(fmaxf(1.f - ct * ct, 0.f));  // reference is NaN for |cos| > 1 (rounding); clamped here
    const float ph = ct * mp.cos_m - sine * mp.sin_m;
    const float dph = mp.cos_m + (sine > 0.f ? mp.sin_m * ct / sine : 0.f);
    const bool take = mp.mode == 1 ? (ct > 0.f) : (ct > mp.th);
    phi = take ? ph : (mp.mode == 1 ? ct : ct - mp.mm);
    dphi = take ? dph : 1.f;
  }
  const float lt = mp.s * phi;
  if constexpr (CRIT == CRIT_PLAIN) {
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      mx = fmaxf(mx, l);
    }
    mx = block_reduce_max(mx, sh);
    float se = 0.f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      se += expf(l - mx);
    }
    se = block_reduce_sum(se, sh);
    const float lse = mx + logf(se);
    const float logp = lse - lt;  // cross-entropy of this row
    const float pt = expf(-logp);
    float f = 1.f, lossv = logp;
    if (mp.gamma != 0.f) {
      const float om = fmaxf(1.f - pt, 0.f);
      lossv = powf(om, mp.gamma) * logp;
      f = powf(om, mp.gamma) + mp.gamma * logp * pt * powf(om, mp.gamma - 1.f);
    }
    if (threadIdx.x == 0 && loss_rows) loss_rows[row] = lossv;
    if (threadIdx.x == 0 && cp.row_stats) reinterpret_cast<f32x4*>(cp.row_stats)[row] = f32x4{lse, f, lt, 1.f};
    const float gs = gscale * f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      if (logits) logits[(size_t)row * C + j] = l;
      if (dcos) {
        const float p = expf(l - lse);
        float d = (j == t) ? (p - 1.f) * dphi : p;
        dcos[(size_t)row * ldc + j] = from_f32<TG>(d * mp.s * gs);
      }
    }
  } else if constexpr (CRIT == CRIT_ALPHA) {
    // z = alpha·l: the maximum, the sum and the target all in z (alpha may be negative or > 1); the logits written stay l
    const float zt = cp.alpha[t] * lt;
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float z = cp.alpha[j] * ((j == t) ? lt : mp.s * cr[j]);
      mx = fmaxf(mx, z);
    }
    mx = block_reduce_max(mx, sh);
    float se = 0.f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float z = cp.alpha[j] * ((j == t) ? lt : mp.s * cr[j]);
      se += expf(z - mx);
    }
    se = block_reduce_sum(se, sh);
    const float lse = mx + logf(se);
    const float logp = lse - zt;
    const float pt = expf(-logp);
    float f = 1.f, lossv = logp;
    if (mp.gamma != 0.f) {
      const float om = fmaxf(1.f - pt, 0.f);
      lossv = powf(om, mp.gamma) * logp;
      f = powf(om, mp.gamma) + mp.gamma * logp * pt * powf(om, mp.gamma - 1.f);
    }
    if (threadIdx.x == 0 && loss_rows) loss_rows[row] = lossv;
    if (threadIdx.x == 0 && cp.row_stats) reinterpret_cast<f32x4*>(cp.row_stats)[row] = f32x4{lse, f, lt, 1.f};
    const float gs = gscale * f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      if (logits) logits[(size_t)row * C + j] = l;
      if (dcos) {
        const float a = cp.alpha[j];
        const float p = expf(a * l - lse);
        float d = (j == t) ? (p - 1.f) * dphi : p;   // dz / f, then dl = alpha·dz
        dcos[(size_t)row * ldc + j] = from_f32<TG>(a * d * mp.s * gs);
      }
    }
  } else {
    const float e = cp.smoothing, wt = cp.weight ? cp.weight[t] : 1.f;
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      mx = fmaxf(mx, l);
    }
    mx = block_reduce_max(mx, sh);
    // the smoothing term rides in the pass of the exponentials: Σ w_c·l_c (and W = Σ w_c when there are weights)
    float se = 0.f, swl = 0.f, sw = 0.f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      se += expf(l - mx);
      if (e != 0.f) {
        if (cp.weight) {
          const float w = cp.weight[j];
          swl = fmaf(w, l, swl);
          sw += w;
        } else {
          swl += l;
        }
      }
    }
    se = block_reduce_sum(se, sh);
    float W = (float)C;
    if (e != 0.f) {
      swl = block_reduce_sum(swl, sh);
      if (cp.weight) W = block_reduce_sum(sw, sh);
    }
    const float lse = mx + logf(se);
    const float hard = (1.f - e) * wt, soft = e / (float)C;
    float lossv = hard * (lse - lt), S = hard;
    if (e != 0.f) {
      lossv += soft * (W * lse - swl);
      S += soft * W;
    }
    if (threadIdx.x == 0 && loss_rows) loss_rows[row] = lossv;
    if (threadIdx.x == 0 && cp.row_stats) reinterpret_cast<f32x4*>(cp.row_stats)[row] = f32x4{lse, S, lt, wt};
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : mp.s * cr[j];
      if (logits) logits[(size_t)row * C + j] = l;
      if (dcos) {
        float d = S * expf(l - lse);
        if (e != 0.f) d -= soft * (cp.weight ? cp.weight[j] : 1.f);
        if (j == t) d = (d - hard) * dphi;
        dcos[(size_t)row * ldc + j] = from_f32<TG>(d * mp.s * gscale);
      }
    }
  }
}

static void margin_params(MarginParams& mp, int mode, float s, float m, float gamma) {
  mp.s = s; mp.m = m; mp.mode = mode; mp.gamma = gamma;
  mp.cos_m = (float)cos((double)m);
  mp.sin_m = (float)sin((double)m);
  mp.th = (float)cos(M_PI - (double)m);
  mp.mm = (float)(sin(M_PI - (double)m) * (double)m);
}

template <int CRIT>
static void launch_margin_ce(const float* cosv, const int64_t* label, int B, int C, int ldc, const MarginParams& mp, float grad_scale,
                             const float* grad_scale_dev, float* logits, float* loss_rows, void* dcos, int dcos_dtype, const CritParams& cp,
                             hipStream_t st) {
  const int nt = C >= 4096 ? 1024 : 256;
  if (dcos_dtype == PFR_BF16)
    hipLaunchKernelGGL((margin_ce_kernel<bf16_t, CRIT>), dim3(B), dim3(nt), 0, st, cosv, label, mp, logits, loss_rows, (bf16_t*)dcos, C, ldc, grad_scale, grad_scale_dev, cp);
  else
    hipLaunchKernelGGL((margin_ce_kernel<float, CRIT>), dim3(B), dim3(nt), 0, st, cosv, label, mp, logits, loss_rows, (float*)dcos, C, ldc, grad_scale, grad_scale_dev, cp);
}

extern "C" int pfr_margin_ce(const float* cosv, const int64_t* label, int B, int C, int ldc, int mode, float s, float m,
                             float gamma, float grad_scale, const float* grad_scale_dev, float* logits, float* loss_rows, void* dcos,
                             int dcos_dtype, hipStream_t st) {
  PFR_CHECK_ARG(cosv && label && B > 0 && C > 0, "pfr_margin_ce: bad args");
  PFR_CHECK_ARG(mode >= 0 && mode <= 3, "pfr_margin_ce: bad margin mode %d", mode);
  MarginParams mp;
  margin_params(mp, mode, s, m, gamma);
  if (ldc <= 0) ldc = C;
  launch_margin_ce<CRIT_PLAIN>(cosv, label, B, C, ldc, mp, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, CritParams{}, st);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_margin_ce_ex(const float* cosv, const int64_t* label, int B, int C, int ldc, int mode, float s, float m, float gamma,
                                const float* alpha, const float* class_weight, float label_smoothing, float grad_scale,
                                const float* grad_scale_dev, const float* grad_scale_dev2, float* logits, float* loss_rows, float* row_stats,
                                void* dcos, int dcos_dtype, hipStream_t st) {
  PFR_CHECK_ARG(cosv && label, "pfr_margin_ce_ex: null pointer");
  PFR_CHECK_ARG(B > 0 && C > 0 && (ldc <= 0 || ldc >= C), "pfr_margin_ce_ex: bad shape B=%d C=%d ldc=%d", B, C, ldc);
  PFR_CHECK_ARG(mode >= 0 && mode <= 3, "pfr_margin_ce_ex: bad margin mode %d", mode);
  PFR_CHECK_ARG(label_smoothing >= 0.f && label_smoothing <= 1.f, "pfr_margin_ce_ex: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  PFR_CHECK_ARG(dcos_dtype == PFR_F32 || dcos_dtype == PFR_BF16, "pfr_margin_ce_ex: bad dcos dtype %d", dcos_dtype);
  const bool wce = class_weight || label_smoothing != 0.f;
  if (alpha && wce) { pfr_set_error("pfr_margin_ce_ex: alpha excludes class_weight / label_smoothing"); return PFR_ERR_UNSUPPORTED; }
  if (wce && gamma != 0.f) { pfr_set_error("pfr_margin_ce_ex: focal gamma excludes class_weight / label_smoothing"); return PFR_ERR_UNSUPPORTED; }
  PFR_CHECK_ARG(wce || !grad_scale_dev2, "pfr_margin_ce_ex: grad_scale_dev2 belongs to the weighted mean only");
  MarginParams mp;
  margin_params(mp, mode, s, m, gamma);
  if (ldc <= 0) ldc = C;
  CritParams cp{alpha, class_weight, label_smoothing, row_stats, grad_scale_dev2};
  if (alpha) launch_margin_ce<CRIT_ALPHA>(cosv, label, B, C, ldc, mp, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, cp, st);
  else if (wce) launch_margin_ce<CRIT_WCE>(cosv, label, B, C, ldc, mp, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, cp, st);
  else launch_margin_ce<CRIT_PLAIN>(cosv, label, B, C, ldc, mp, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, cp, st);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// dalpha_c = gscale · Σ_i dz_ic · l_ic, dz_ic = f_i · (softmax(z_i)_c − [c == t_i]) recomputed from cos, alpha and the row statistics of
// margin_ce_kernel<CRIT_ALPHA> (dz itself is never stored).  A workgroup owns 64 consecutive classes: lane = class (coalesced reads of
// cos), wave w walks rows w, w + nw, ... in that order, the nw partial sums meet in LDS and wave 0 adds them in wave order: no
// atomics, the same bits every run.
__global__ __launch_bounds__(1024) void alpha_grad_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                          const float* __restrict__ alpha, const float* __restrict__ row_stats,
                                                          float* __restrict__ dalpha, int B, int C, int ldc, float s, float gscale,
                                                          const float* __restrict__ gscale_dev) {
  __shared__ float part[16][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool live = c < C;
  const int cc = live ? c : C - 1;
  const float a = alpha[cc];
  float acc = 0.f;
  for (int i = w; i < B; i += nw) {
    const f32x4 st = reinterpret_cast<const f32x4*>(row_stats)[i];   // {lse, f, l_t, -}
    const float l = (cc == (int)label[i]) ? st[2] : s * cosv[(size_t)i * ldc + cc];
    const float p = expf(a * l - st[0]);
    const float dz = st[1] * ((cc == (int)label[i]) ? p - 1.f : p);
    acc = fmaf(dz, l, acc);
  }
  part[w][lane] = acc;
  __syncthreads();
  if (w == 0 && live) {
    float r = part[0][lane];
    for (int k = 1; k < nw; ++k) r += part[k][lane];
    if (gscale_dev) gscale *= gscale_dev[0];
    dalpha[c] = r * gscale;
  }
}
extern "C" int pfr_alpha_grad(const float* cosv, const int64_t* label, const float* alpha, const float* row_stats, int B, int C, int ldc,
                              float s, float grad_scale, const float* grad_scale_dev, float* dalpha, hipStream_t st) {
  PFR_CHECK_ARG(cosv && label && alpha && row_stats && dalpha, "pfr_alpha_grad: null pointer");
  PFR_CHECK_ARG(B > 0 && C > 0 && (ldc <= 0 || ldc >= C), "pfr_alpha_grad: bad shape B=%d C=%d ldc=%d", B, C, ldc);
  if (ldc <= 0) ldc = C;
  const int nt = B >= 64 ? 1024 : 256;
  hipLaunchKernelGGL(alpha_grad_kernel, dim3((C + 63) / 64), dim3(nt), 0, st, cosv, label, alpha, row_stats, dalpha, B, C, ldc, s, grad_scale, grad_scale_dev);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// mean of a small fp32 vector (the per-row losses) → scalar
__global__ void mean_kernel(const float* __restrict__ x, float* __restrict__ out, int n) {
  __shared__ float sh[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += x[i];
  a = block_reduce_sum(a, sh);
  if (threadIdx.x == 0) out[0] = a / n;
}
extern "C" int pfr_mean(const float* x, float* out, int n, hipStream_t st) {
  PFR_CHECK_ARG(x && out && n > 0, "pfr_mean: bad args");
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, st, x, out, n);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// the criterion's reduction of the per-row losses without a host round trip: out_loss = Σ rows / d and out_inv_denom = 1 / d with
// d = n ('mean' of the focal criteria), 1 ('sum') or Σ_i w_{t_i} (nn.CrossEntropyLoss(weight=, reduction='mean'); w_t is row_stats[i][3])
__global__ void loss_reduce_kernel(const float* __restrict__ x, const float* __restrict__ row_stats, float* __restrict__ out,
                                   float* __restrict__ out_inv, int n, int reduction) {
  __shared__ float sh[4];
  float a = 0.f, d = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    a += x[i];
    if (reduction == 2) d += row_stats[4 * (size_t)i + 3];
  }
  a = block_reduce_sum(a, sh);
  if (reduction == 2) d = block_reduce_sum(d, sh);
  else d = reduction == 0 ? (float)n : 1.f;
  if (threadIdx.x == 0) {
    out[0] = a / d;
    if (out_inv) out_inv[0] = 1.f / d;
  }
}
extern "C" int pfr_loss_reduce(const float* loss_rows, const float* row_stats, int n, int reduction, float* out_loss, float* out_inv_denom,
                               hipStream_t st) {
  PFR_CHECK_ARG(loss_rows && out_loss && n > 0, "pfr_loss_reduce: bad args");
  PFR_CHECK_ARG(reduction >= 0 && reduction <= 2, "pfr_loss_reduce: bad reduction mode %d", reduction);
  PFR_CHECK_ARG(reduction != 2 || row_stats, "pfr_loss_reduce: the weighted mean needs row_stats");
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, st, loss_rows, row_stats, out_loss, out_inv_denom, n, reduction);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// standalone backward of the margin: dcos = s·dlogits (·dphi/dcos on the target column)  — used when
// ArcMarginProduct / AddMarginProduct run as separate modules (losses/large_margin.py:30-40,69-84)
template <typename TG>
__global__ __launch_bounds__(256) void margin_bwd_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                         MarginParams mp, const float* __restrict__ dlogits,
                                                         TG* __restrict__ dcos, int C, int ldc) {
  const int row = blockIdx.x;
  const int t = (int)label[row];
  const float ct = cosv[(size_t)row * ldc + t];
  float dphi = 1.f;
  if (mp.mode == 0 || mp.mode == 1) {
    const float sine = sqrtf(fmaxf(1.f - ct * ct, 0.f));
    const float dph = mp.cos_m + (sine > 0.f ? mp.sin_m * ct / sine : 0.f);
    const bool take = mp.mode == 1 ? (ct > 0.f) : (ct > mp.th);
    dphi = take ? dph : 1.f;
  }
  for (int j = threadIdx.x; j < C; j += 256) {
    float d = dlogits[(size_t)row * C + j] * mp.s;
    if (j == t) d *= dphi;
    dcos[(size_t)row * ldc + j] = from_f32<TG>(d);
  }
}
extern "C" int pfr_margin_bwd(const float* cosv, const int64_t* label, int B, int C, int ldc, int mode, float s, float m,
                              const float* dlogits, void* dcos, int dcos_dtype, hipStream_t st) {
  PFR_CHECK_ARG(cosv && label && dlogits && dcos, "pfr_margin_bwd: null pointer");
  MarginParams mp;
  mp.s = s; mp.m = m; mp.mode = mode; mp.gamma = 0.f;
  mp.cos_m = (float)cos((double)m);
  mp.sin_m = (float)sin((double)m);
  mp.th = (float)cos(M_PI - (double)m);
  mp.mm = (float)(sin(M_PI - (double)m) * (double)m);
  if (ldc <= 0) ldc = C;
  if (dcos_dtype == PFR_BF16)
    hipLaunchKernelGGL(margin_bwd_kernel<bf16_t>, dim3(B), dim3(256), 0, st, cosv, label, mp, dlogits, (bf16_t*)dcos, C, ldc);
  else
    hipLaunchKernelGGL(margin_bwd_kernel<float>, dim3(B), dim3(256), 0, st, cosv, label, mp, dlogits, (float*)dcos, C, ldc);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ---- sub-centre heads (Deng et al., ECCV 2020): K centres per class, weight row c*K + k, so the K sub-cosines of a class are
// contiguous in a cosine row.  Two streaming passes around the unchanged row kernel: the pool takes the class cosine as the maximum
// of its K sub-cosines (and remembers which one), the scatter routes d loss / d cos back to that sub-centre alone.
// A lane owns whole classes: K contiguous floats in, K contiguous elements out; with K = 2 or 4 and aligned rows those are one
// 8- / 16-byte access.  grid.y = rows, grid.x = class chunks, sized so that B = 256 alone gives ~2048 workgroups.
template <typename T, int N>
struct alignas(sizeof(T) * N) SubPack {
  T v[N];
};

// KT: compile-time K (0 = run-time K, 1..16); VEC: the lane's K elements move as one SubPack (host checked the alignment)
template <int KT, bool VEC>
__global__ __launch_bounds__(256) void subcenter_pool_kernel(const float* __restrict__ cos_sub, int C, int Krt, int ld_sub,
                                                             float* __restrict__ cosv, int ldc, uint8_t* __restrict__ arg,
                                                             const int64_t* __restrict__ label, int32_t* __restrict__ count) {
  const int K = KT ? KT : Krt;
  const int row = blockIdx.y;
  const float* src = cos_sub + (size_t)row * ld_sub;
  float* dst = cosv + (size_t)row * ldc;
  uint8_t* adst = arg + (size_t)row * C;
  const int t = label ? (int)label[row] : -1;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < ldc; c += gridDim.x * 256) {
    if (c >= C) {   // the GEMMs of the backward read the padded width
      dst[c] = 0.f;
      continue;
    }
    float best;
    int a = 0;
    if constexpr (VEC) {
      const SubPack<float, KT> p = *reinterpret_cast<const SubPack<float, KT>*>(src + (size_t)c * KT);
      best = p.v[0];
#pragma unroll
      for (int k = 1; k < KT; ++k)
        if (p.v[k] > best) { best = p.v[k]; a = k; }
    } else {
      const float* s = src + (size_t)c * K;
      best = s[0];
      for (int k = 1; k < K; ++k) {
        const float v = s[k];
        if (v > best) { best = v; a = k; }   // strict: the lowest k wins a tie
      }
    }
    dst[c] = best;
    adst[c] = (uint8_t)a;
    if (count && c == t) atomicAdd(&count[(size_t)c * K + a], 1);   // one lane per row; integer adds: the same bits every run
  }
}

extern "C" int pfr_subcenter_pool(const float* cos_sub, int B, int C, int K, int ld_sub, float* cosv, int ldc, uint8_t* arg,
                                  const int64_t* label, int32_t* count, hipStream_t st) {
  PFR_CHECK_ARG(cos_sub && cosv && arg, "pfr_subcenter_pool: null pointer");
  PFR_CHECK_ARG(K >= 1 && K <= 16, "pfr_subcenter_pool: K=%d outside 1..16", K);
  PFR_CHECK_ARG(B > 0 && C > 0 && ldc >= C && (long long)ld_sub >= (long long)C * K, "pfr_subcenter_pool: bad shape B=%d C=%d K=%d ld_sub=%d ldc=%d",
                B, C, K, ld_sub, ldc);
  PFR_CHECK_ARG(B <= 65535, "pfr_subcenter_pool: B=%d above 65535 rows", B);
  PFR_CHECK_ARG(!count == !label, "pfr_subcenter_pool: count and label go together");
  const int chunks = (ldc + 255) / 256;
  const int per_row = 2048 / B > 1 ? 2048 / B : 1;
  const dim3 grid(chunks < per_row ? chunks : per_row, B), block(256);
  const bool al = ((uintptr_t)cos_sub % (4 * (size_t)K)) == 0 && ld_sub % K == 0;
#define SCP(KT, VEC) hipLaunchKernelGGL((subcenter_pool_kernel<KT, VEC>), grid, block, 0, st, cos_sub, C, K, ld_sub, cosv, ldc, arg, label, count)
  if (K == 2 && al) SCP(2, true);
  else if (K == 4 && al) SCP(4, true);
  else if (K == 2) SCP(2, false);
  else if (K == 3) SCP(3, false);
  else if (K == 4) SCP(4, false);
  else SCP(0, false);
#undef SCP
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// dcos_sub[b][c*K + k] = (k == arg[b][c]) ? dcos[b][c] : 0 over the whole [B, ld_sub] buffer: lanes past the last class write the pad
// columns, so nothing clears the buffer first
template <typename TG, int KT, bool VEC>
__global__ __launch_bounds__(256) void subcenter_scatter_kernel(const TG* __restrict__ dcos, const uint8_t* __restrict__ arg, int C, int Krt,
                                                                int ldc, TG* __restrict__ dcos_sub, int ld_sub) {
  const int K = KT ? KT : Krt;
  const int row = blockIdx.y;
  const TG* src = dcos + (size_t)row * ldc;
  const uint8_t* asrc = arg + (size_t)row * C;
  TG* dst = dcos_sub + (size_t)row * ld_sub;
  const int nc = (ld_sub + K - 1) / K;   // classes, then whole or partial groups of pad columns
  const TG zero = from_f32<TG>(0.f);
  for (int c = blockIdx.x * 256 + threadIdx.x; c < nc; c += gridDim.x * 256) {
    const bool live = c < C;
    const TG d = live ? src[c] : zero;
    const int a = live ? (int)asrc[c] : -1;
    if constexpr (VEC) {   // ld_sub is a multiple of K: every group is whole
      SubPack<TG, KT> p;
#pragma unroll
      for (int k = 0; k < KT; ++k) p.v[k] = k == a ? d : zero;
      *reinterpret_cast<SubPack<TG, KT>*>(dst + (size_t)c * KT) = p;
    } else {
      const size_t col0 = (size_t)c * K;
      for (int k = 0; k < K; ++k)
        if (col0 + k < (size_t)ld_sub) dst[col0 + k] = k == a ? d : zero;
    }
  }
}

template <typename TG>
static void launch_subcenter_scatter(const void* dcos, const uint8_t* arg, int B, int C, int K, int ldc, void* dcos_sub, int ld_sub,
                                     hipStream_t st) {
  const int chunks = ((ld_sub + K - 1) / K + 255) / 256;
  const int per_row = 2048 / B > 1 ? 2048 / B : 1;
  const dim3 grid(chunks < per_row ? chunks : per_row, B), block(256);
  const bool al = ((uintptr_t)dcos_sub % (sizeof(TG) * (size_t)K)) == 0 && ld_sub % K == 0;
#define SCS(KT, VEC) hipLaunchKernelGGL((subcenter_scatter_kernel<TG, KT, VEC>), grid, block, 0, st, (const TG*)dcos, arg, C, K, ldc, (TG*)dcos_sub, ld_sub)
  if (K == 2 && al) SCS(2, true);
  else if (K == 4 && al) SCS(4, true);
  else if (K == 2) SCS(2, false);
  else if (K == 3) SCS(3, false);
  else if (K == 4) SCS(4, false);
  else SCS(0, false);
#undef SCS
}

extern "C" int pfr_subcenter_scatter(const void* dcos, int dtype, const uint8_t* arg, int B, int C, int K, int ldc, void* dcos_sub,
                                     int ld_sub, hipStream_t st) {
  PFR_CHECK_ARG(dcos && arg && dcos_sub, "pfr_subcenter_scatter: null pointer");
  PFR_CHECK_ARG(K >= 1 && K <= 16, "pfr_subcenter_scatter: K=%d outside 1..16", K);
  PFR_CHECK_ARG(B > 0 && C > 0 && ldc >= C && (long long)ld_sub >= (long long)C * K, "pfr_subcenter_scatter: bad shape B=%d C=%d K=%d ldc=%d ld_sub=%d",
                B, C, K, ldc, ld_sub);
  PFR_CHECK_ARG(B <= 65535, "pfr_subcenter_scatter: B=%d above 65535 rows", B);
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "pfr_subcenter_scatter: bad dtype %d", dtype);
  if (dtype == PFR_BF16) launch_subcenter_scatter<bf16_t>(dcos, arg, B, C, K, ldc, dcos_sub, ld_sub, st);
  else launch_subcenter_scatter<float>(dcos, arg, B, C, K, ldc, dcos_sub, ld_sub, st);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ---- adaptive margins: AdaFace (Kim et al., CVPR 2022: the margin is a function of the sample's feature norm) and CurricularFace
// (Huang et al., CVPR 2020: hard negatives are re-weighted by t + cos, t an EMA of the target cosines).  Neither is in the reference.
// One small launch (margin_prepare_kernel) turns the batch into the per-row margins / the scalar t and moves the module's EMA buffers on
// the device; the row kernel below is margin_ce_kernel with the margin kind as a second compile-time switch.  What a step used
// (state_used, row_margin) is a per-call copy: the backward of a step never reads the buffers a later forward may have moved.
// MagFace (Meng et al., CVPR 2021; not in the reference either) is the third kind: the margin is a function of the row's length like
// AdaFace's, but the length is trained: the row kernel also writes d loss / d |x| (dnorm), which pfr_l2norm_bwd_radial adds to the
// tangent embedding gradient.  It has an entry point of its own (pfr_margin_ce_magface): the two above keep their argument lists.
enum { MK_ADAFACE = 0, MK_CURRICULAR = 1, MK_MAGFACE = 2 };
struct AdaptiveParams {
  float s, m, eps, gamma;
  float cos_m, sin_m, th, mm;   // CurricularFace: ArcFace's hard margin on the target
  // MagFace only: easy / hard fallback, the regulariser's gradient scale (lambda_g / B or lambda_g), {g, dg/d|x|} per row, the output
  int easy = 0;
  float reg_scale = 0.f;
  const float* row_reg = nullptr;
  float* dnorm = nullptr;
};

// 256 threads, fixed tree: the same bits every launch
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// one workgroup; sums in fp64 (B values: the cost is the launch), results rounded to fp32 once.
// AdaFace: a = clip(1 / inv_norm, 1e-3, 100); mean, then the centred squares (two passes); EMA of both into state0 / state1 when
//   `update` (state1 keeps its value at B = 1: the unbiased deviation is undefined); row_margin[b] = {g_ang, g_add} from the buffers
//   after the update; state_used = {batch_mean, batch_std}.
// CurricularFace: t <- momentum * mean_b clamp(cos[b][label_b], -1, 1) + (1 - momentum) * t when `update`; state_used = {t, 0}.
template <int KIND>
__global__ __launch_bounds__(256) void margin_prepare_kernel(const float* __restrict__ inv_norm, const float* __restrict__ cosv,
                                                             const int64_t* __restrict__ label, int B, int ldc, float m, float h,
                                                             float momentum, float eps, int update, float* __restrict__ state0,
                                                             float* __restrict__ state1, float* __restrict__ row_margin,
                                                             float* __restrict__ state_used) {
  __shared__ double sh[256];
  const double mom = (double)momentum;
  if constexpr (KIND == MK_ADAFACE) {
    double bm = (double)state0[0], bs = (double)state1[0];   // read before the barriers below, written after them
    if (update) {
      double a = 0.0;
      for (int i = threadIdx.x; i < B; i += 256) a += fmin(fmax(1.0 / (double)inv_norm[i], 1e-3), 100.0);
      const double mu = block_sum_f64(a, sh) / (double)B;
      bm = (double)(float)(mom * mu + (1.0 - mom) * bm);
      if (B > 1) {
        double q = 0.0;
        for (int i = threadIdx.x; i < B; i += 256) {
          const double d = fmin(fmax(1.0 / (double)inv_norm[i], 1e-3), 100.0) - mu;
          q = fma(d, d, q);
        }
        const double sigma = sqrt(block_sum_f64(q, sh) / (double)(B - 1));
        bs = (double)(float)(mom * sigma + (1.0 - mom) * bs);
      }
      if (threadIdx.x == 0) {
        state0[0] = (float)bm;
        state1[0] = (float)bs;
      }
    }
    if (threadIdx.x == 0) {
      state_used[0] = (float)bm;
      state_used[1] = (float)bs;
    }
    for (int i = threadIdx.x; i < B; i += 256) {
      const double a = fmin(fmax(1.0 / (double)inv_norm[i], 1e-3), 100.0);
      const double k = fmin(fmax((double)h * (a - bm) / (bs + (double)eps), -1.0), 1.0);
      row_margin[2 * (size_t)i] = (float)(-(double)m * k);
      row_margin[2 * (size_t)i + 1] = (float)((double)m + (double)m * k);
    }
  } else {
    double t = (double)state0[0];
    if (update) {
      double a = 0.0;
      for (int i = threadIdx.x; i < B; i += 256) a += (double)fminf(fmaxf(cosv[(size_t)i * ldc + (int)label[i]], -1.f), 1.f);
      const double mu = block_sum_f64(a, sh) / (double)B;
      t = (double)(float)(mom * mu + (1.0 - mom) * t);
      if (threadIdx.x == 0) state0[0] = (float)t;
    }
    if (threadIdx.x == 0) {
      state_used[0] = (float)t;
      state_used[1] = 0.f;
    }
  }
}

extern "C" int pfr_margin_prepare(int kind, const float* inv_norm, const float* cosv, const int64_t* label, int B, int ldc, float m, float h,
                                  float momentum, float eps, int update, float* state0, float* state1, float* row_margin, float* state_used,
                                  hipStream_t st) {
  PFR_CHECK_ARG(kind == MK_ADAFACE || kind == MK_CURRICULAR, "pfr_margin_prepare: bad margin kind %d", kind);
  PFR_CHECK_ARG(B > 0, "pfr_margin_prepare: bad shape B=%d", B);
  PFR_CHECK_ARG(state0 && state_used, "pfr_margin_prepare: null pointer");
  PFR_CHECK_ARG(momentum >= 0.f && momentum <= 1.f, "pfr_margin_prepare: momentum %g outside [0, 1]", (double)momentum);
  if (kind == MK_ADAFACE) {
    PFR_CHECK_ARG(inv_norm && state1 && row_margin, "pfr_margin_prepare: null pointer (AdaFace reads inv_norm, writes batch_std and row_margin)");
    hipLaunchKernelGGL(margin_prepare_kernel<MK_ADAFACE>, dim3(1), dim3(256), 0, st, inv_norm, cosv, label, B, ldc, m, h, momentum, eps, update,
                       state0, state1, row_margin, state_used);
  } else {
    PFR_CHECK_ARG(cosv && label && ldc > 0, "pfr_margin_prepare: null pointer (CurricularFace reads the target cosines)");
    hipLaunchKernelGGL(margin_prepare_kernel<MK_CURRICULAR>, dim3(1), dim3(256), 0, st, inv_norm, cosv, label, B, ldc, m, h, momentum, eps, update,
                       state0, state1, row_margin, state_used);
  }
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// What a row needs once: the target's margin value phi and d phi / d cos, and two numbers (a, b) for the per-entry work.
//   AdaFace:        a, b = the clamp's edges -1 + eps, 1 - eps;  acosf / cosf / sinf run here, once per row
//   CurricularFace: a = t, b = cos(theta + m) of the target (the threshold of a hard negative)
template <int KIND>
__device__ __forceinline__ void adaptive_row(float craw, int row, const AdaptiveParams& ap, const float* __restrict__ row_margin,
                                             const float* __restrict__ state_used, float& phi, float& dphi, float& a, float& b) {
  if constexpr (KIND == MK_ADAFACE) {
    a = -1.f + ap.eps;
    b = 1.f - ap.eps;
    const float ct = fminf(fmaxf(craw, a), b);
    const float g_ang = row_margin[2 * (size_t)row], g_add = row_margin[2 * (size_t)row + 1];
    const float theta = acosf(ct);
    const float lo = ap.eps, hi = 3.14159265358979f - ap.eps;
    const float tp = theta + g_ang;
    const float tc = fminf(fmaxf(tp, lo), hi);
    phi = cosf(tc) - g_add;
    const bool flat = tp < lo || tp > hi || craw < a || craw > b;   // a clip or the clamp is active: no gradient
    dphi = flat ? 0.f : sinf(tc) / sqrtf(fmaxf(1.f - ct * ct, 0.f));  // sin(theta) >= sqrt(2 eps) > 0 inside the clamp
  } else if constexpr (KIND == MK_MAGFACE) {
    // the row's own margin m and d m / d |x| (pfr_magface_prepare); cosf / sinf run here, once per row
    const float m = row_margin[2 * (size_t)row], slope = row_margin[2 * (size_t)row + 1];
    const float cm = cosf(m), sm = sinf(m);
    const float ct = fminf(fmaxf(craw, -1.f), 1.f);
    const float sine = sqrtf(fmaxf(1.f - ct * ct, 0.f));
    const float ph = ct * cm - sine * sm;
    const float dph = cm + (sine > 0.f ? sm * ct / sine : 0.f);
    const bool take = ap.easy ? (ct > 0.f) : (ct > -cm);          // cos(pi - m) = -cos m
    phi = take ? ph : (ap.easy ? ct : ct - m * sm);
    dphi = (craw < -1.f || craw > 1.f) ? 0.f : (take ? dph : 1.f);
    // d phi / d m: -sin(theta + m) under the margin, the derivative of -m sin m on the hard fallback
    const float dpm = take ? -(ct * sm + sine * cm) : (ap.easy ? 0.f : -(sm + m * cm));
    a = dpm * slope;    // d phi / d |x|
    b = 0.f;
  } else {
    const float ct = fminf(fmaxf(craw, -1.f), 1.f);
    const float sine = sqrtf(fmaxf(1.f - ct * ct, 0.f));
    const float ph = ct * ap.cos_m - sine * ap.sin_m;
    const float dph = ap.cos_m + (sine > 0.f ? ap.sin_m * ct / sine : 0.f);
    const bool take = ct > ap.th;
    phi = take ? ph : ct - ap.mm;
    dphi = (craw < -1.f || craw > 1.f) ? 0.f : (take ? dph : 1.f);
    a = state_used[0];
    b = ph;
  }
}
// a negative's value on the cosine side (the logit is s times it) ...
template <int KIND>
__device__ __forceinline__ float adaptive_neg(float c, float a, float b) {
  if constexpr (KIND == MK_ADAFACE) return fminf(fmaxf(c, a), b);
  const float cc = fminf(fmaxf(c, -1.f), 1.f);
  if constexpr (KIND == MK_MAGFACE) return cc;
  return cc > b ? cc * (a + cc) : cc;
}
// ... and its derivative
template <int KIND>
__device__ __forceinline__ float adaptive_dneg(float c, float a, float b) {
  if constexpr (KIND == MK_ADAFACE) return (c < a || c > b) ? 0.f : 1.f;
  if (c < -1.f || c > 1.f) return 0.f;
  if constexpr (KIND == MK_MAGFACE) return 1.f;
  return c > b ? fmaf(2.f, c, a) : 1.f;
}

// margin_ce_kernel (same passes, same row_stats / gscale conventions, same dcos dtypes) with the margin kind as a compile-time switch.
// MagFace: thread 0 also writes dnorm[row] = (d loss / d l_t) * s * d phi / d |x| + the regulariser's lambda_g * g'(a) with its own
// scale (it is a mean over B whatever the criterion divides by): the target's softmax value is one more expf per row.
template <typename TG, int CRIT, int KIND>
__global__ __launch_bounds__(1024) void margin_ce_adaptive_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                                 AdaptiveParams ap, const float* __restrict__ row_margin,
                                                                 const float* __restrict__ state_used, float* __restrict__ logits,
                                                                 float* __restrict__ loss_rows, TG* __restrict__ dcos, int C, int ldc,
                                                                 float gscale, const float* __restrict__ gscale_dev, CritParams cp) {
  static_assert(CRIT == CRIT_PLAIN || CRIT == CRIT_WCE, "the learnable alpha is not fused with the adaptive margins");
  __shared__ float sh[16];
  float rscale = 0.f;
  if constexpr (KIND == MK_MAGFACE) rscale = gscale_dev ? ap.reg_scale * gscale_dev[0] : ap.reg_scale;
  if (gscale_dev) gscale *= gscale_dev[0];
  if (CRIT == CRIT_WCE && cp.gscale_dev2) gscale *= cp.gscale_dev2[0];
  const int row = blockIdx.x;
  const int nt = blockDim.x;
  const float* cr = cosv + (size_t)row * ldc;
  const int t = (int)label[row];
  float phi, dphi, ma, mb;
  adaptive_row<KIND>(cr[t], row, ap, row_margin, state_used, phi, dphi, ma, mb);
  const float lt = ap.s * phi;
  if constexpr (CRIT == CRIT_PLAIN) {
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : ap.s * adaptive_neg<KIND>(cr[j], ma, mb);
      mx = fmaxf(mx, l);
    }
    mx = block_reduce_max(mx, sh);
    float se = 0.f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : ap.s * adaptive_neg<KIND>(cr[j], ma, mb);
      se += expf(l - mx);
    }
    se = block_reduce_sum(se, sh);
    const float lse = mx + logf(se);
    const float logp = lse - lt;
    const float pt = expf(-logp);
    float f = 1.f, lossv = logp;
    if (ap.gamma != 0.f) {
      const float om = fmaxf(1.f - pt, 0.f);
      lossv = powf(om, ap.gamma) * logp;
      f = powf(om, ap.gamma) + ap.gamma * logp * pt * powf(om, ap.gamma - 1.f);
    }
    if (threadIdx.x == 0 && loss_rows) loss_rows[row] = lossv;
    if (threadIdx.x == 0 && cp.row_stats) reinterpret_cast<f32x4*>(cp.row_stats)[row] = f32x4{lse, f, lt, 1.f};
    const float gs = gscale * f;
    if constexpr (KIND == MK_MAGFACE) {
      if (threadIdx.x == 0 && ap.dnorm) {
        float r = (expf(lt - lse) - 1.f) * ap.s * gs * ma;
        if (ap.row_reg) r = fmaf(rscale, ap.row_reg[2 * (size_t)row + 1], r);
        ap.dnorm[row] = r;
      }
    }
    for (int j = threadIdx.x; j < C; j += nt) {
      const float c = cr[j];
      const float l = (j == t) ? lt : ap.s * adaptive_neg<KIND>(c, ma, mb);
      if (logits) logits[(size_t)row * C + j] = l;
      if (dcos) {
        const float p = expf(l - lse);
        const float d = (j == t) ? (p - 1.f) * dphi : p * adaptive_dneg<KIND>(c, ma, mb);
        dcos[(size_t)row * ldc + j] = from_f32<TG>(d * ap.s * gs);
      }
    }
  } else {
    const float e = cp.smoothing, wt = cp.weight ? cp.weight[t] : 1.f;
    float mx = -INFINITY;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : ap.s * adaptive_neg<KIND>(cr[j], ma, mb);
      mx = fmaxf(mx, l);
    }
    mx = block_reduce_max(mx, sh);
    float se = 0.f, swl = 0.f, sw = 0.f;
    for (int j = threadIdx.x; j < C; j += nt) {
      const float l = (j == t) ? lt : ap.s * adaptive_neg<KIND>(cr[j], ma, mb);
      se += expf(l - mx);
      if (e != 0.f) {
        if (cp.weight) {
          const float w = cp.weight[j];
          swl = fmaf(w, l, swl);
          sw += w;
        } else {
          swl += l;
        }
      }
    }
    se = block_reduce_sum(se, sh);
    float W = (float)C;
    if (e != 0.f) {
      swl = block_reduce_sum(swl, sh);
      if (cp.weight) W = block_reduce_sum(sw, sh);
    }
    const float lse = mx + logf(se);
    const float hard = (1.f - e) * wt, soft = e / (float)C;
    float lossv = hard * (lse - lt), S = hard;
    if (e != 0.f) {
      lossv += soft * (W * lse - swl);
      S += soft * W;
    }
    if (threadIdx.x == 0 && loss_rows) loss_rows[row] = lossv;
    if (threadIdx.x == 0 && cp.row_stats) reinterpret_cast<f32x4*>(cp.row_stats)[row] = f32x4{lse, S, lt, wt};
    if constexpr (KIND == MK_MAGFACE) {
      if (threadIdx.x == 0 && ap.dnorm) {
        float d = S * expf(lt - lse) - hard;
        if (e != 0.f) d -= soft * wt;
        float r = d * ap.s * gscale * ma;
        if (ap.row_reg) r = fmaf(rscale, ap.row_reg[2 * (size_t)row + 1], r);
        ap.dnorm[row] = r;
      }
    }
    for (int j = threadIdx.x; j < C; j += nt) {
      const float c = cr[j];
      const float l = (j == t) ? lt : ap.s * adaptive_neg<KIND>(c, ma, mb);
      if (logits) logits[(size_t)row * C + j] = l;
      if (dcos) {
        float d = S * expf(l - lse);
        if (e != 0.f) d -= soft * (cp.weight ? cp.weight[j] : 1.f);
        d = (j == t) ? (d - hard) * dphi : d * adaptive_dneg<KIND>(c, ma, mb);
        dcos[(size_t)row * ldc + j] = from_f32<TG>(d * ap.s * gscale);
      }
    }
  }
}

static void adaptive_params(AdaptiveParams& ap, float s, float m, float eps, float gamma) {
  ap.s = s; ap.m = m; ap.eps = eps; ap.gamma = gamma;
  ap.cos_m = (float)cos((double)m);
  ap.sin_m = (float)sin((double)m);
  ap.th = (float)cos(M_PI - (double)m);
  ap.mm = (float)(sin(M_PI - (double)m) * (double)m);
}

template <int CRIT, int KIND>
static void launch_margin_ce_adaptive(const float* cosv, const int64_t* label, int B, int C, int ldc, const AdaptiveParams& ap,
                                      const float* row_margin, const float* state_used, float grad_scale, const float* grad_scale_dev,
                                      float* logits, float* loss_rows, void* dcos, int dcos_dtype, const CritParams& cp, hipStream_t st) {
  const int nt = C >= 4096 ? 1024 : 256;
  if (dcos_dtype == PFR_BF16)
    hipLaunchKernelGGL((margin_ce_adaptive_kernel<bf16_t, CRIT, KIND>), dim3(B), dim3(nt), 0, st, cosv, label, ap, row_margin, state_used, logits, loss_rows, (bf16_t*)dcos, C, ldc, grad_scale, grad_scale_dev, cp);
  else
    hipLaunchKernelGGL((margin_ce_adaptive_kernel<float, CRIT, KIND>), dim3(B), dim3(nt), 0, st, cosv, label, ap, row_margin, state_used, logits, loss_rows, (float*)dcos, C, ldc, grad_scale, grad_scale_dev, cp);
}

extern "C" int pfr_margin_ce_adaptive(const float* cosv, const int64_t* label, int B, int C, int ldc, int kind, float s, float m, float eps,
                                      float gamma, const float* class_weight, float label_smoothing, const float* row_margin,
                                      const float* state_used, float grad_scale, const float* grad_scale_dev, const float* grad_scale_dev2,
                                      float* logits, float* loss_rows, float* row_stats, void* dcos, int dcos_dtype, hipStream_t st) {
  PFR_CHECK_ARG(cosv && label, "pfr_margin_ce_adaptive: null pointer");
  PFR_CHECK_ARG(B > 0 && C > 0 && (ldc <= 0 || ldc >= C), "pfr_margin_ce_adaptive: bad shape B=%d C=%d ldc=%d", B, C, ldc);
  PFR_CHECK_ARG(kind == MK_ADAFACE || kind == MK_CURRICULAR, "pfr_margin_ce_adaptive: bad margin kind %d", kind);
  PFR_CHECK_ARG(kind == MK_ADAFACE ? row_margin != nullptr : state_used != nullptr,
                "pfr_margin_ce_adaptive: null pointer (AdaFace reads row_margin, CurricularFace state_used: pfr_margin_prepare writes both)");
  PFR_CHECK_ARG(kind != MK_ADAFACE || (eps > 0.f && eps < 1.f), "pfr_margin_ce_adaptive: eps %g outside (0, 1)", (double)eps);
  PFR_CHECK_ARG(label_smoothing >= 0.f && label_smoothing <= 1.f, "pfr_margin_ce_adaptive: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  PFR_CHECK_ARG(dcos_dtype == PFR_F32 || dcos_dtype == PFR_BF16, "pfr_margin_ce_adaptive: bad dcos dtype %d", dcos_dtype);
  const bool wce = class_weight || label_smoothing != 0.f;
  if (wce && gamma != 0.f) { pfr_set_error("pfr_margin_ce_adaptive: focal gamma excludes class_weight / label_smoothing"); return PFR_ERR_UNSUPPORTED; }
  PFR_CHECK_ARG(wce || !grad_scale_dev2, "pfr_margin_ce_adaptive: grad_scale_dev2 belongs to the weighted mean only");
  AdaptiveParams ap;
  adaptive_params(ap, s, m, eps, gamma);
  if (ldc <= 0) ldc = C;
  CritParams cp{nullptr, class_weight, label_smoothing, row_stats, grad_scale_dev2};
#define MCA(CRIT, KIND) launch_margin_ce_adaptive<CRIT, KIND>(cosv, label, B, C, ldc, ap, row_margin, state_used, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, cp, st)
  if (kind == MK_ADAFACE) { if (wce) MCA(CRIT_WCE, MK_ADAFACE); else MCA(CRIT_PLAIN, MK_ADAFACE); }
  else { if (wce) MCA(CRIT_WCE, MK_CURRICULAR); else MCA(CRIT_PLAIN, MK_CURRICULAR); }
#undef MCA
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// standalone backward of the adaptive margins (the unfused path: the heads as separate modules, or a criterion the row kernel does not
// fuse): dcos = s * dlogits * d l / d cos, the derivatives of adaptive_row / adaptive_dneg
template <typename TG, int KIND>
__global__ __launch_bounds__(256) void margin_bwd_adaptive_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                                  AdaptiveParams ap, const float* __restrict__ row_margin,
                                                                  const float* __restrict__ state_used, const float* __restrict__ dlogits,
                                                                  TG* __restrict__ dcos, int C, int ldc) {
  const int row = blockIdx.x;
  const float* cr = cosv + (size_t)row * ldc;
  const int t = (int)label[row];
  float phi, dphi, ma, mb;
  adaptive_row<KIND>(cr[t], row, ap, row_margin, state_used, phi, dphi, ma, mb);
  for (int j = threadIdx.x; j < C; j += 256) {
    const float d = dlogits[(size_t)row * C + j] * ap.s * ((j == t) ? dphi : adaptive_dneg<KIND>(cr[j], ma, mb));
    dcos[(size_t)row * ldc + j] = from_f32<TG>(d);
  }
}
extern "C" int pfr_margin_bwd_adaptive(const float* cosv, const int64_t* label, int B, int C, int ldc, int kind, float s, float m, float eps,
                                       const float* row_margin, const float* state_used, const float* dlogits, void* dcos, int dcos_dtype,
                                       hipStream_t st) {
  PFR_CHECK_ARG(cosv && label && dlogits && dcos, "pfr_margin_bwd_adaptive: null pointer");
  PFR_CHECK_ARG(B > 0 && C > 0 && (ldc <= 0 || ldc >= C), "pfr_margin_bwd_adaptive: bad shape B=%d C=%d ldc=%d", B, C, ldc);
  PFR_CHECK_ARG(kind == MK_ADAFACE || kind == MK_CURRICULAR, "pfr_margin_bwd_adaptive: bad margin kind %d", kind);
  PFR_CHECK_ARG(kind == MK_ADAFACE ? row_margin != nullptr : state_used != nullptr,
                "pfr_margin_bwd_adaptive: null pointer (AdaFace reads row_margin, CurricularFace state_used: pfr_margin_prepare writes both)");
  PFR_CHECK_ARG(kind != MK_ADAFACE || (eps > 0.f && eps < 1.f), "pfr_margin_bwd_adaptive: eps %g outside (0, 1)", (double)eps);
  PFR_CHECK_ARG(dcos_dtype == PFR_F32 || dcos_dtype == PFR_BF16, "pfr_margin_bwd_adaptive: bad dcos dtype %d", dcos_dtype);
  AdaptiveParams ap;
  adaptive_params(ap, s, m, eps, 0.f);
  if (ldc <= 0) ldc = C;
#define MBA(TG, KIND) hipLaunchKernelGGL((margin_bwd_adaptive_kernel<TG, KIND>), dim3(B), dim3(256), 0, st, cosv, label, ap, row_margin, state_used, dlogits, (TG*)dcos, C, ldc)
  if (kind == MK_ADAFACE) { if (dcos_dtype == PFR_BF16) MBA(bf16_t, MK_ADAFACE); else MBA(float, MK_ADAFACE); }
  else { if (dcos_dtype == PFR_BF16) MBA(bf16_t, MK_CURRICULAR); else MBA(float, MK_CURRICULAR); }
#undef MBA
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ---- MagFace: the per-row margins and regulariser values, the row kernel's entry, the standalone backward, the loss with the
// regulariser, and the embedding backward with the radial term.
// prepare: every row on its own (no sums), fp64 arithmetic on the fp32 |x| = 1 / inv_norm, rounded once
__global__ __launch_bounds__(256) void magface_prepare_kernel(const float* __restrict__ inv_norm, int B, float l_a, float u_a, float l_m,
                                                              float u_m, float* __restrict__ row_margin, float* __restrict__ row_reg) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B) return;
  const float n = 1.f / inv_norm[i];
  const bool inside = n >= l_a && n <= u_a;      // torch.clamp's autograd: the bounds themselves pass the gradient
  const double a = fmin(fmax((double)n, (double)l_a), (double)u_a);
  const double slope = ((double)u_m - (double)l_m) / ((double)u_a - (double)l_a);
  const double ua2 = (double)u_a * (double)u_a;
  reinterpret_cast<f32x2*>(row_margin)[i] = f32x2{(float)(slope * (a - (double)l_a) + (double)l_m), inside ? (float)slope : 0.f};
  reinterpret_cast<f32x2*>(row_reg)[i] = f32x2{(float)(a / ua2 + 1.0 / a), inside ? (float)(1.0 / ua2 - 1.0 / (a * a)) : 0.f};
}

extern "C" int pfr_magface_prepare(const float* inv_norm, int B, float l_a, float u_a, float l_m, float u_m, float* row_margin,
                                   float* row_reg, hipStream_t st) {
  PFR_CHECK_ARG(inv_norm && row_margin && row_reg, "pfr_magface_prepare: null pointer");
  PFR_CHECK_ARG(B > 0, "pfr_magface_prepare: bad shape B=%d", B);
  PFR_CHECK_ARG(l_a > 0.f && u_a > l_a, "pfr_magface_prepare: need 0 < l_a < u_a, got %g, %g", (double)l_a, (double)u_a);
  hipLaunchKernelGGL(magface_prepare_kernel, dim3((B + 255) / 256), dim3(256), 0, st, inv_norm, B, l_a, u_a, l_m, u_m, row_margin, row_reg);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_margin_ce_magface(const float* cosv, const int64_t* label, int B, int C, int ldc, int easy_margin, float s, float gamma,
                                     const float* class_weight, float label_smoothing, const float* row_margin, const float* row_reg,
                                     float reg_scale, float grad_scale, const float* grad_scale_dev, const float* grad_scale_dev2,
                                     float* logits, float* loss_rows, float* row_stats, void* dcos, int dcos_dtype, float* dnorm,
                                     hipStream_t st) {
  PFR_CHECK_ARG(cosv && label && row_margin, "pfr_margin_ce_magface: null pointer (row_margin is what pfr_magface_prepare wrote)");
  PFR_CHECK_ARG(B > 0 && C > 0 && (ldc <= 0 || ldc >= C), "pfr_margin_ce_magface: bad shape B=%d C=%d ldc=%d", B, C, ldc);
  PFR_CHECK_ARG(label_smoothing >= 0.f && label_smoothing <= 1.f, "pfr_margin_ce_magface: label_smoothing %g outside [0, 1]", (double)label_smoothing);
  PFR_CHECK_ARG(dcos_dtype == PFR_F32 || dcos_dtype == PFR_BF16, "pfr_margin_ce_magface: bad dcos dtype %d", dcos_dtype);
  PFR_CHECK_ARG(row_reg || reg_scale == 0.f, "pfr_margin_ce_magface: reg_scale %g without row_reg", (double)reg_scale);
  const bool wce = class_weight || label_smoothing != 0.f;
  if (wce && gamma != 0.f) { pfr_set_error("pfr_margin_ce_magface: focal gamma excludes class_weight / label_smoothing"); return PFR_ERR_UNSUPPORTED; }
  PFR_CHECK_ARG(wce || !grad_scale_dev2, "pfr_margin_ce_magface: grad_scale_dev2 belongs to the weighted mean only");
  AdaptiveParams ap;
  adaptive_params(ap, s, 0.f, 0.f, gamma);
  ap.easy = easy_margin != 0;
  ap.reg_scale = reg_scale;
  ap.row_reg = row_reg;
  ap.dnorm = dnorm;
  if (ldc <= 0) ldc = C;
  CritParams cp{nullptr, class_weight, label_smoothing, row_stats, grad_scale_dev2};
  if (wce) launch_margin_ce_adaptive<CRIT_WCE, MK_MAGFACE>(cosv, label, B, C, ldc, ap, row_margin, nullptr, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, cp, st);
  else launch_margin_ce_adaptive<CRIT_PLAIN, MK_MAGFACE>(cosv, label, B, C, ldc, ap, row_margin, nullptr, grad_scale, grad_scale_dev, logits, loss_rows, dcos, dcos_dtype, cp, st);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// margin_bwd_adaptive_kernel for MagFace, plus dnorm (thread 0)
template <typename TG>
__global__ __launch_bounds__(256) void margin_bwd_magface_kernel(const float* __restrict__ cosv, const int64_t* __restrict__ label,
                                                                 AdaptiveParams ap, const float* __restrict__ row_margin,
                                                                 const float* __restrict__ reg_scale_dev, const float* __restrict__ dlogits,
                                                                 TG* __restrict__ dcos, int C, int ldc) {
  const int row = blockIdx.x;
  const float* cr = cosv + (size_t)row * ldc;
  const int t = (int)label[row];
  float phi, dphi, ma, mb;
  adaptive_row<MK_MAGFACE>(cr[t], row, ap, row_margin, nullptr, phi, dphi, ma, mb);
  if (threadIdx.x == 0 && ap.dnorm) {
    float r = dlogits[(size_t)row * C + t] * ap.s * ma;
    if (ap.row_reg) r = fmaf(reg_scale_dev ? ap.reg_scale * reg_scale_dev[0] : ap.reg_scale, ap.row_reg[2 * (size_t)row + 1], r);
    ap.dnorm[row] = r;
  }
  for (int j = threadIdx.x; j < C; j += 256) {
    const float d = dlogits[(size_t)row * C + j] * ap.s * ((j == t) ? dphi : adaptive_dneg<MK_MAGFACE>(cr[j], ma, mb));
    dcos[(size_t)row * ldc + j] = from_f32<TG>(d);
  }
}
extern "C" int pfr_margin_bwd_magface(const float* cosv, const int64_t* label, int B, int C, int ldc, int easy_margin, float s,
                                      const float* row_margin, const float* row_reg, float reg_scale, const float* reg_scale_dev,
                                      const float* dlogits, void* dcos, int dcos_dtype, float* dnorm, hipStream_t st) {
  PFR_CHECK_ARG(cosv && label && dlogits && dcos && row_margin, "pfr_margin_bwd_magface: null pointer");
  PFR_CHECK_ARG(B > 0 && C > 0 && (ldc <= 0 || ldc >= C), "pfr_margin_bwd_magface: bad shape B=%d C=%d ldc=%d", B, C, ldc);
  PFR_CHECK_ARG(dcos_dtype == PFR_F32 || dcos_dtype == PFR_BF16, "pfr_margin_bwd_magface: bad dcos dtype %d", dcos_dtype);
  PFR_CHECK_ARG(row_reg || reg_scale == 0.f, "pfr_margin_bwd_magface: reg_scale %g without row_reg", (double)reg_scale);
  AdaptiveParams ap;
  adaptive_params(ap, s, 0.f, 0.f, 0.f);
  ap.easy = easy_margin != 0;
  ap.reg_scale = reg_scale;
  ap.row_reg = row_reg;
  ap.dnorm = dnorm;
  if (ldc <= 0) ldc = C;
  if (dcos_dtype == PFR_BF16)
    hipLaunchKernelGGL(margin_bwd_magface_kernel<bf16_t>, dim3(B), dim3(256), 0, st, cosv, label, ap, row_margin, reg_scale_dev, dlogits, (bf16_t*)dcos, C, ldc);
  else
    hipLaunchKernelGGL(margin_bwd_magface_kernel<float>, dim3(B), dim3(256), 0, st, cosv, label, ap, row_margin, reg_scale_dev, dlogits, (float*)dcos, C, ldc);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// loss_reduce_kernel with the regulariser: out = sum(rows) / d + lambda_g * sum_i g(a_i) / (n, or 1 for 'sum'); the same strides and
// the same block_reduce_sum, so the criterion term has pfr_loss_reduce's bits
__global__ void magface_loss_kernel(const float* __restrict__ x, const float* __restrict__ row_stats, const float* __restrict__ row_reg,
                                    float* __restrict__ out, float* __restrict__ out_inv, float* __restrict__ out_reg, int n, int reduction,
                                    float lambda_g) {
  __shared__ float sh[4];
  float a = 0.f, d = 0.f, g = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (x) a += x[i];
    if (x && reduction == 2) d += row_stats[4 * (size_t)i + 3];
    g += row_reg[2 * (size_t)i];
  }
  a = block_reduce_sum(a, sh);
  g = block_reduce_sum(g, sh);
  if (reduction == 2 && x) d = block_reduce_sum(d, sh);
  else d = reduction == 0 ? (float)n : 1.f;
  if (threadIdx.x == 0) {
    const float reg = lambda_g * g / (reduction == 1 ? 1.f : (float)n);
    if (out_reg) out_reg[0] = reg;
    if (x) out[0] = a / d + reg;
    if (x && out_inv) out_inv[0] = 1.f / d;
  }
}
extern "C" int pfr_magface_loss(const float* loss_rows, const float* row_stats, const float* row_reg, int n, int reduction, float lambda_g,
                                float* out_loss, float* out_inv_denom, float* out_reg, hipStream_t st) {
  PFR_CHECK_ARG(row_reg && n > 0 && (loss_rows ? out_loss != nullptr : out_reg != nullptr), "pfr_magface_loss: bad args");
  PFR_CHECK_ARG(reduction >= 0 && reduction <= 2, "pfr_magface_loss: bad reduction mode %d", reduction);
  PFR_CHECK_ARG(reduction != 2 || !loss_rows || row_stats, "pfr_magface_loss: the weighted mean needs row_stats");
  hipLaunchKernelGGL(magface_loss_kernel, dim3(1), dim3(256), 0, st, loss_rows, row_stats, row_reg, out_loss, out_inv_denom, out_reg, n, reduction, lambda_g);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// l2norm_bwd_kernel plus dnorm[row] * x / |x|: one wave per row, the same two passes over the row
template <typename TI, typename TOo>
__global__ __launch_bounds__(256) void l2norm_bwd_radial_kernel(const TI* __restrict__ x, const float* __restrict__ inv_norm,
                                                                const float* __restrict__ dxn, const float* __restrict__ dnorm,
                                                                TOo* __restrict__ dx, int rows, int D, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float inv = inv_norm[row], dn = dnorm[row];
  const TI* xr = x + (size_t)row * D;
  const float* gr = dxn + (size_t)row * D;
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot = fmaf(to_f32(xr[d]) * inv, gr[d], dot);
  dot = wave_sum(dot);
  for (int d = lane; d < D; d += 64) {
    const float xh = to_f32(xr[d]) * inv;
    float v = fmaf(dn, xh, inv * (gr[d] - xh * dot));
    if (accumulate) v += to_f32(dx[(size_t)row * D + d]);
    dx[(size_t)row * D + d] = from_f32<TOo>(v);
  }
}

extern "C" int pfr_l2norm_bwd_radial(const void* x, int in_dtype, const float* inv_norm, const float* dxn, const float* dnorm, void* dx,
                                     int out_dtype, int rows, int D, int accumulate, hipStream_t st) {
  if (!dnorm) return pfr_l2norm_bwd(x, in_dtype, inv_norm, dxn, dx, out_dtype, rows, D, accumulate, st);
  PFR_CHECK_ARG(x && inv_norm && dxn && dx, "pfr_l2norm_bwd_radial: null pointer");
  PFR_CHECK_ARG(rows > 0 && D > 0, "pfr_l2norm_bwd_radial: bad shape rows=%d D=%d", rows, D);
  const dim3 grid((rows + 3) / 4), block(256);
#define L2R(TI, TOo) hipLaunchKernelGGL((l2norm_bwd_radial_kernel<TI, TOo>), grid, block, 0, st, (const TI*)x, inv_norm, dxn, dnorm, (TOo*)dx, rows, D, accumulate)
  if (in_dtype == PFR_F32 && out_dtype == PFR_F32) L2R(float, float);
  else if (in_dtype == PFR_BF16 && out_dtype == PFR_BF16) L2R(bf16_t, bf16_t);
  else if (in_dtype == PFR_BF16 && out_dtype == PFR_F32) L2R(bf16_t, float);
  else if (in_dtype == PFR_F32 && out_dtype == PFR_BF16) L2R(float, bf16_t);
  else { pfr_set_error("pfr_l2norm_bwd_radial: bad dtypes"); return PFR_ERR_UNSUPPORTED; }
#undef L2R
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
