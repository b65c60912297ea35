// pfr_pfc.hip — Partial FC (An et al., CVPR 2022): the margin head scores a sampled subset of the class centres.
//
// Semantics (losses/large_margin.py: _MarginHead.sample): key[c] = 2.0 when class c occurs in the batch's labels, else score[c] (a
// uniform draw in [0, 1)); index = the S classes with the largest key, ties towards the lower class id, ascending;
// local_label[b] = position of label[b] in index.  The head then runs on the S gathered centres as it does on all C.
//
// Kernels here:
//   pfr_pfc_sample          the selection, entirely on the stream: 32-bit order-preserving keys, an 8-bit-digit radix select of the S-th
//                           largest key (integer histograms: order-free, so bit-reproducible), per-block counts of the keys above / equal
//                           to it, an ordered compaction that takes the equal keys in class order until the quota is used, and a binary
//                           search of every label in the sorted result.
//   pfr_l2norm_gather_fwd   ŵ[s] = W[index[s]] / max(|.|, eps) with pfr_l2norm_fwd's arithmetic (both of its kernels), pad rows zeroed.
//   pfr_l2norm_gather_bwd   pfr_l2norm_bwd's arithmetic on the gathered rows, compact [S, D] or scattered into a dense [C, D] buffer whose
//                           rows of the previous index are re-zeroed in the same launch.
//   pfr_sgd_step_rows       SGD with momentum and weight decay on the listed rows only (lazy momentum).
#include "pfr_common.h"

static constexpr int PFC_ITEMS = 4;                     // classes per thread of the count / compaction kernels (consecutive)
static constexpr int PFC_TILE = 256 * PFC_ITEMS;        // classes per block there

static inline long pfc_nblk(long C) { return (C + PFC_TILE - 1) / PFC_TILE; }
// workspace: key u32 [C] | hist u32 [4][256] | blk_gt u32 [nblk] | blk_eq u32 [nblk]
extern "C" long pfr_pfc_sample_ws_bytes(long C) {
  if (C < 1) return 0;
  return (long)sizeof(uint32_t) * (C + 4 * 256 + 2 * pfc_nblk(C));
}

// larger score = larger key; -0.0 orders as +0.0 (torch.sort compares the values)
__device__ __forceinline__ uint32_t pfc_key(float s) { return fkey(s == 0.f ? 0.f : s); }

__global__ __launch_bounds__(256) void pfc_keys_kernel(const float* __restrict__ score, uint32_t* __restrict__ key, int C) {
  const int stride = gridDim.x * blockDim.x;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += stride) key[c] = pfc_key(score[c]);
}

// positives get the maximum key (several rows of one class store the same word); a label outside [0, C) flags nothing
__global__ __launch_bounds__(256) void pfc_flag_kernel(const long long* __restrict__ label, uint32_t* __restrict__ key, int B, int C) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long c = label[b];
  if (c >= 0 && c < C) key[c] = 0xffffffffu;
}

// State of the radix select after `npass` digits, recomputed by every block from the finished histograms (256 threads, 1 KB of LDS): the
// key prefix chosen so far and how many keys of that prefix are still to be taken, largest first.  hist[q] counts digit q of the keys
// whose higher digits equal the prefix.  Every thread returns the same (prefix, rem).
__device__ __forceinline__ void pfc_resolve(const uint32_t* __restrict__ hist, int npass, uint32_t S, uint32_t* sh, uint32_t* sh_out,
                                            uint32_t& prefix, uint32_t& rem) {
  const int t = threadIdx.x;
  prefix = 0;
  rem = S;
  for (int q = 0; q < npass; ++q) {
    const uint32_t h = hist[q * 256 + t];
    // above = number of keys in the bins > t: an inclusive suffix sum minus the own bin
    __syncthreads();
    sh[t] = h;
    __syncthreads();
    uint32_t incl = h;
    for (int o = 1; o < 256; o <<= 1) {
      const uint32_t add = t + o < 256 ? sh[t + o] : 0u;
      __syncthreads();
      incl += add;
      sh[t] = incl;
      __syncthreads();
    }
    const uint32_t above = incl - h;
    if (above < rem && rem <= incl) {       // exactly one bin: the rem-th largest key of this prefix has digit t
      sh_out[0] = t;
      sh_out[1] = rem - above;
    }
    __syncthreads();
    prefix = (prefix << 8) | sh_out[0];
    rem = sh_out[1];
  }
}

// digit `pass` (0 = the top byte) of the keys that match the prefix of the passes before it
__global__ __launch_bounds__(256) void pfc_hist_kernel(const uint32_t* __restrict__ key, uint32_t* __restrict__ hist, int C, uint32_t S, int pass) {
  __shared__ uint32_t sh[256];
  __shared__ uint32_t sh_out[2];
  __shared__ uint32_t loc[256];
  uint32_t prefix, rem;
  pfc_resolve(hist, pass, S, sh, sh_out, prefix, rem);
  loc[threadIdx.x] = 0;
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const int stride = gridDim.x * blockDim.x;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < C; c += stride) {
    const uint32_t k = key[c];
    // (pass 0: every key matches; a shift by 32 is not defined)
    if (pass == 0 || (k >> (shift + 8)) == prefix) atomicAdd(&loc[(k >> shift) & 255u], 1u);
  }
  __syncthreads();
  const uint32_t n = loc[threadIdx.x];
  if (n) atomicAdd(&hist[pass * 256 + threadIdx.x], n);
}

// keys above / equal to the threshold in each tile of PFC_TILE consecutive classes
__global__ __launch_bounds__(256) void pfc_count_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ hist, uint32_t* __restrict__ blk_gt,
                                                        uint32_t* __restrict__ blk_eq, int C, uint32_t S) {
  __shared__ uint32_t sh[256];
  __shared__ uint32_t sh_out[2];
  __shared__ uint32_t tot[2];
  uint32_t thr, quota;
  pfc_resolve(hist, 4, S, sh, sh_out, thr, quota);
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * PFC_TILE + threadIdx.x * PFC_ITEMS;
  uint32_t gt = 0, eq = 0;
#pragma unroll
  for (int e = 0; e < PFC_ITEMS; ++e) {
    if (base + e < C) {
      const uint32_t k = key[base + e];
      gt += k > thr;
      eq += k == thr;
    }
  }
  if (gt) atomicAdd(&tot[0], gt);
  if (eq) atomicAdd(&tot[1], eq);
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_gt[blockIdx.x] = tot[0];
    blk_eq[blockIdx.x] = tot[1];
  }
}

// ordered compaction: class c is taken when key > thr, or key == thr and fewer than `quota` equal keys precede it; its place is the
// number of taken classes before it = (#greater before) + min(#equal before, quota)
__global__ __launch_bounds__(256) void pfc_compact_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ hist,
                                                          const uint32_t* __restrict__ blk_gt, const uint32_t* __restrict__ blk_eq,
                                                          int* __restrict__ index, int C, uint32_t S) {
  __shared__ uint32_t sh[256];
  __shared__ uint32_t sh_out[2];
  __shared__ uint32_t sg[256];
  __shared__ uint32_t se[256];
  uint32_t thr, quota;
  pfc_resolve(hist, 4, S, sh, sh_out, thr, quota);
  const int t = threadIdx.x;
  // taken-before counts of the tiles in front of this one (integer sums: any order gives the same value)
  uint32_t pg = 0, pe = 0;
  for (int j = t; j < (int)blockIdx.x; j += 256) {
    pg += blk_gt[j];
    pe += blk_eq[j];
  }
  const long base = (long)blockIdx.x * PFC_TILE + t * PFC_ITEMS;
  uint32_t k[PFC_ITEMS];
  uint32_t gt = 0, eq = 0;
#pragma unroll
  for (int e = 0; e < PFC_ITEMS; ++e) {
    k[e] = base + e < C ? key[base + e] : 0u;
    if (base + e < C) {
      gt += k[e] > thr;
      eq += k[e] == thr;
    }
  }
  __syncthreads();
  sg[t] = pg;
  se[t] = pe;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
      sg[t] += sg[t + o];
      se[t] += se[t + o];
    }
    __syncthreads();
  }
  const uint32_t front_gt = sg[0], front_eq = se[0];
  __syncthreads();
  // exclusive scan of the per-thread counts inside the tile
  sg[t] = gt;
  se[t] = eq;
  __syncthreads();
  uint32_t ig = gt, ie = eq;
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t ag = t >= o ? sg[t - o] : 0u;
    const uint32_t ae = t >= o ? se[t - o] : 0u;
    __syncthreads();
    ig += ag;
    ie += ae;
    sg[t] = ig;
    se[t] = ie;
    __syncthreads();
  }
  uint32_t g_before = front_gt + ig - gt, e_before = front_eq + ie - eq;
#pragma unroll
  for (int e = 0; e < PFC_ITEMS; ++e) {
    if (base + e < C) {
      const bool is_gt = k[e] > thr, is_eq = k[e] == thr;
      if (is_gt || (is_eq && e_before < quota)) {
        const uint32_t pos = g_before + (e_before < quota ? e_before : quota);
        if (pos < S) index[pos] = (int)(base + e);
      }
      g_before += is_gt;
      e_before += is_eq;
    }
  }
}

// local_label[b] = position of label[b] in the ascending index (-1: not there, i.e. a label outside [0, C))
__global__ __launch_bounds__(256) void pfc_lookup_kernel(const long long* __restrict__ label, const int* __restrict__ index,
                                                         long long* __restrict__ local_label, int B, int S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long c = label[b];
  int lo = 0, hi = S;                    // first position with index[pos] >= c
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long long)index[mid] < c) lo = mid + 1; else hi = mid;
  }
  local_label[b] = (lo < S && (long long)index[lo] == c) ? lo : -1;
}

extern "C" int pfr_pfc_sample(const void* label, int B, const float* score, int C, int S, int* index, void* local_label, void* ws,
                              hipStream_t st) {
  PFR_CHECK_ARG(label && score && index && local_label && ws, "pfr_pfc_sample: null pointer");
  PFR_CHECK_ARG(C >= 1 && S >= 1 && S <= C, "pfr_pfc_sample: need 1 <= S <= C (S = %d, C = %d)", S, C);
  PFR_CHECK_ARG(B >= 1 && B <= S, "pfr_pfc_sample: need 1 <= B <= S so that every positive fits (B = %d, S = %d)", B, S);
  uint32_t* key = reinterpret_cast<uint32_t*>(ws);
  uint32_t* hist = key + C;
  const int nblk = (int)pfc_nblk(C);
  uint32_t* blk_gt = hist + 4 * 256;
  uint32_t* blk_eq = blk_gt + nblk;
  if (hipMemsetAsync(hist, 0, 4 * 256 * sizeof(uint32_t), st) != hipSuccess) {
    pfr_set_error("pfr_pfc_sample: hipMemsetAsync failed");
    return PFR_ERR_HIP;
  }
  const int sblk = nblk < 1024 ? nblk : 1024;   // the grid-stride kernels
  hipLaunchKernelGGL(pfc_keys_kernel, dim3(sblk), dim3(256), 0, st, score, key, C);
  hipLaunchKernelGGL(pfc_flag_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const long long*)label, key, B, C);
  for (int pass = 0; pass < 4; ++pass) hipLaunchKernelGGL(pfc_hist_kernel, dim3(sblk), dim3(256), 0, st, key, hist, C, (uint32_t)S, pass);
  hipLaunchKernelGGL(pfc_count_kernel, dim3(nblk), dim3(256), 0, st, key, hist, blk_gt, blk_eq, C, (uint32_t)S);
  hipLaunchKernelGGL(pfc_compact_kernel, dim3(nblk), dim3(256), 0, st, key, hist, blk_gt, blk_eq, index, C, (uint32_t)S);
  hipLaunchKernelGGL(pfc_lookup_kernel, dim3((B + 255) / 256), dim3(256), 0, st, (const long long*)label, index, (long long*)local_label, B, S);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ------------------------------------------------------------------------------------------------
// gathered normalisation.  One wave per output row s < Spad; rows S .. Spad-1 (the GEMM's padding) are written as zeros, as are the pad
// columns of the transposed copy.  A row id outside [0, C) normalises a zero row.
// DUAL = the arithmetic of l2norm_dual_kernel (what pfr_l2norm_fwd runs for fp32 rows without a transposed copy when D % 4 == 0 and
// D <= 2048: float4 chunks kept in registers); otherwise that of l2norm_fwd_kernel.  Either way a gathered row has the bits of the same
// row of a full normalisation.
template <typename TOo, int NK>
__global__ __launch_bounds__(256) void l2norm_gather_dual_kernel(const float* __restrict__ W, const int* __restrict__ index, TOo* __restrict__ wn,
                                                                 float* __restrict__ inv_norm, int S, int Spad, int C, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= Spad) return;
  const int n4 = D >> 2;
  const int r = s < S ? index[s] : -1;
  if (r < 0 || r >= C) {
    for (int i = lane; i < n4; i += 64) {
      if constexpr (sizeof(TOo) == 2) reinterpret_cast<u32x2*>(wn + (size_t)s * D)[i] = u32x2{0u, 0u};
      else reinterpret_cast<f32x4*>(wn + (size_t)s * D)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (s < S && lane == 0) inv_norm[s] = 1.f / eps;
    return;
  }
  const f32x4* xr = reinterpret_cast<const f32x4*>(W + (size_t)r * D);
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
  if (lane == 0) inv_norm[s] = inv;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int i = lane + 64 * k;
    if (i < n4) {
      f32x4 o = v[k] * inv;
      if constexpr (sizeof(TOo) == 2) {
        bf16x4 b;
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = (bf16_t)o[e];
        reinterpret_cast<bf16x4*>(wn + (size_t)s * D)[i] = b;
      } else {
        reinterpret_cast<f32x4*>(wn + (size_t)s * D)[i] = o;
      }
    }
  }
}

template <typename TOo>
__global__ __launch_bounds__(256) void l2norm_gather_fwd_kernel(const float* __restrict__ W, const int* __restrict__ index, TOo* __restrict__ wn,
                                                                TOo* __restrict__ wnT, float* __restrict__ inv_norm, int S, int Spad, int C,
                                                                int D, int ldt, float eps) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= Spad) return;
  const int r = s < S ? index[s] : -1;
  if (r < 0 || r >= C) {
    for (int d = lane; d < D; d += 64) {
      wn[(size_t)s * D + d] = from_f32<TOo>(0.f);
      if (wnT) wnT[(size_t)d * ldt + s] = from_f32<TOo>(0.f);
    }
    if (s < S && lane == 0) inv_norm[s] = 1.f / eps;
    return;
  }
  const float* xr = W + (size_t)r * D;
  float ss = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float v = to_f32(xr[d]);
    ss = fmaf(v, v, ss);
  }
  ss = wave_sum(ss);
  const float inv = 1.f / fmaxf(sqrtf(ss), eps);
  if (lane == 0) inv_norm[s] = inv;
  for (int d = lane; d < D; d += 64) {
    const TOo o = from_f32<TOo>(to_f32(xr[d]) * inv);
    wn[(size_t)s * D + d] = o;
    if (wnT) wnT[(size_t)d * ldt + s] = o;
  }
}

extern "C" int pfr_l2norm_gather_fwd(const float* W, const int* index, void* wn, void* wnT, int out_dtype, float* inv_norm, int S, int Spad,
                                     int C, int D, int ldt, float eps, hipStream_t st) {
  PFR_CHECK_ARG(W && index && wn && inv_norm, "pfr_l2norm_gather_fwd: null pointer");
  PFR_CHECK_ARG(S >= 1 && S <= C && Spad >= S && D >= 1, "pfr_l2norm_gather_fwd: need 1 <= S <= C, Spad >= S, D >= 1");
  PFR_CHECK_ARG(!wnT || ldt >= Spad, "pfr_l2norm_gather_fwd: the transposed copy needs ldt >= Spad");
  PFR_CHECK_ARG(out_dtype == PFR_F32 || out_dtype == PFR_BF16, "pfr_l2norm_gather_fwd: bad dtype");
  const dim3 grid((Spad + 3) / 4), block(256);
  if (!wnT && D % 4 == 0 && D <= 2048) {
#define L2GD(TOo, NK) hipLaunchKernelGGL((l2norm_gather_dual_kernel<TOo, NK>), grid, block, 0, st, W, index, (TOo*)wn, inv_norm, S, Spad, C, D, eps)
    if (out_dtype == PFR_BF16) { if (D <= 512) L2GD(bf16_t, 2); else L2GD(bf16_t, 8); }
    else { if (D <= 512) L2GD(float, 2); else L2GD(float, 8); }
#undef L2GD
  } else if (out_dtype == PFR_BF16) {
    hipLaunchKernelGGL(l2norm_gather_fwd_kernel<bf16_t>, grid, block, 0, st, W, index, (bf16_t*)wn, (bf16_t*)wnT, inv_norm, S, Spad, C, D, ldt, eps);
  } else {
    hipLaunchKernelGGL(l2norm_gather_fwd_kernel<float>, grid, block, 0, st, W, index, (float*)wn, (float*)wnT, inv_norm, S, Spad, C, D, ldt, eps);
  }
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// position of row id r in the ascending list idx[0..n), or -1
__device__ __forceinline__ int pfc_find(const int* __restrict__ idx, int n, int r) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < r) lo = mid + 1; else hi = mid;
  }
  return (lo < n && idx[lo] == r) ? lo : -1;
}

// rows[s] = inv · (dŵ[s] − ŵ[s] · (ŵ[s]·dŵ[s])) with ŵ recomputed from W[index[s]] and inv (l2norm_bwd_kernel's arithmetic).  One wave per
// job: jobs 0 .. S-1 write a gradient row (compact: row s of out; dense: row index[s] of the [C, D] buffer), jobs S .. S+prevS-1 exist in
// dense mode only and zero row prev[j] of the buffer unless this step's index holds it too (that row is written by its own job: no
// two waves touch one row).
__global__ __launch_bounds__(256) void l2norm_gather_bwd_kernel(const float* __restrict__ W, const int* __restrict__ index, const float* __restrict__ inv_norm,
                                                                const float* __restrict__ dwn, float* __restrict__ out, int S, int C, int D, int dense,
                                                                const int* __restrict__ prev, int prevS) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (job >= S + prevS) return;
  if (job >= S) {
    const int r = prev[job - S];
    if (r < 0 || r >= C || pfc_find(index, S, r) >= 0) return;
    for (int d = lane; d < D; d += 64) out[(size_t)r * D + d] = 0.f;
    return;
  }
  const int r = index[job];
  if (r < 0 || r >= C) return;
  const float inv = inv_norm[job];
  const float* xr = W + (size_t)r * D;
  const float* gr = dwn + (size_t)job * D;
  float* orow = out + (size_t)(dense ? r : job) * D;
  float dot = 0.f;
  for (int d = lane; d < D; d += 64) dot = fmaf(to_f32(xr[d]) * inv, gr[d], dot);
  dot = wave_sum(dot);
  for (int d = lane; d < D; d += 64) {
    float v = inv * (gr[d] - to_f32(xr[d]) * inv * dot);
    orow[d] = from_f32<float>(v);
  }
}

extern "C" int pfr_l2norm_gather_bwd(const float* W, const int* index, const float* inv_norm, const float* dwn, float* out, int S, int C, int D,
                                     int dense, const int* prev_index, int prev_S, hipStream_t st) {
  PFR_CHECK_ARG(W && index && inv_norm && dwn && out, "pfr_l2norm_gather_bwd: null pointer");
  PFR_CHECK_ARG(S >= 1 && S <= C && D >= 1, "pfr_l2norm_gather_bwd: need 1 <= S <= C, D >= 1");
  PFR_CHECK_ARG(prev_S >= 0 && prev_S <= C && (prev_S == 0 || (prev_index && dense)),
                "pfr_l2norm_gather_bwd: a previous index (0 <= prev_S <= C) belongs to the dense mode and must not be null");
  const long jobs = (long)S + prev_S;
  hipLaunchKernelGGL(l2norm_gather_bwd_kernel, dim3((unsigned)((jobs + 3) / 4)), dim3(256), 0, st, W, index, inv_norm, dwn, out, S, C, D, dense, prev_index,
                     prev_S);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ------------------------------------------------------------------------------------------------
// SGD on the listed rows: g = clip(rows * gscale) + wd * w[r]; mom[r] = momentum * mom[r] + g; w[r] -= lr * mom[r] — sgd_kernel's
// arithmetic (pfr_elementwise.hip) with a zero-initialised momentum buffer.  One thread per 16-byte chunk of a row (D % 4 == 0 and
// 16-byte-aligned buffers), else per element.  Nothing outside the listed rows is read or written; a row id outside [0, C) is skipped.
template <bool VEC>
__global__ __launch_bounds__(256) void sgd_rows_kernel(float* __restrict__ p, const int* __restrict__ index, const float* __restrict__ rows,
                                                       float* __restrict__ mom, long total, int C, int D, float lr, float momentum, float wd,
                                                       float gscale, const float* __restrict__ coef, float clipv) {
  const float c = coef ? *coef : 1.f;
  const bool use_mom = momentum != 0.f;
  const int per_row = VEC ? D >> 2 : D;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long s = i / per_row;
    const int j = (int)(i - s * per_row);
    const int r = index[s];
    if (r < 0 || r >= C) continue;
    if constexpr (VEC) {
      f32x4* wp = reinterpret_cast<f32x4*>(p + (size_t)r * D) + j;
      f32x4* mp = reinterpret_cast<f32x4*>(mom + (size_t)r * D) + j;
      f32x4 w = *wp;
      const f32x4 gr = reinterpret_cast<const f32x4*>(rows)[i];
      f32x4 m = {0.f, 0.f, 0.f, 0.f};
      if (use_mom) m = *mp;
      f32x4 b;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float gv = gr[e] * gscale * c;
        if (clipv > 0.f) gv = gv > clipv ? clipv : (gv < -clipv ? -clipv : gv);
        const float d = fmaf(wd, w[e], gv);
        b[e] = use_mom ? fmaf(momentum, m[e], d) : d;
        w[e] = fmaf(-lr, b[e], w[e]);
      }
      if (use_mom) *mp = b;
      *wp = w;
    } else {
      const size_t o = (size_t)r * D + j;
      float w = p[o];
      float gv = rows[i] * gscale * c;
      if (clipv > 0.f) gv = gv > clipv ? clipv : (gv < -clipv ? -clipv : gv);
      const float d = fmaf(wd, w, gv);
      float b = d;
      if (use_mom) {
        b = fmaf(momentum, mom[o], d);
        mom[o] = b;
      }
      p[o] = fmaf(-lr, b, w);
    }
  }
}

extern "C" int pfr_sgd_step_rows(float* p, const int* index, const float* rows, float* mom, int S, int C, int D, float lr, float momentum,
                                 float weight_decay, float grad_scale, const float* clip_coef, float clip_value, hipStream_t st) {
  PFR_CHECK_ARG(p && index && rows && (momentum == 0.f || mom), "pfr_sgd_step_rows: null pointer");
  PFR_CHECK_ARG(S >= 1 && S <= C && D >= 1, "pfr_sgd_step_rows: need 1 <= S <= C, D >= 1");
  PFR_CHECK_ARG(clip_value >= 0.f, "pfr_sgd_step_rows: clip_value must be >= 0 (0 = no clamp)");
  const bool vec = D % 4 == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(mom)) & 15) == 0;
  const long total = vec ? (long)S * (D / 4) : (long)S * D;
  long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (vec)
    hipLaunchKernelGGL(sgd_rows_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, p, index, rows, mom, total, C, D, lr, momentum, weight_decay,
                       grad_scale, clip_coef, clip_value);
  else
    hipLaunchKernelGGL(sgd_rows_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, p, index, rows, mom, total, C, D, lr, momentum, weight_decay,
                       grad_scale, clip_coef, clip_value);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
