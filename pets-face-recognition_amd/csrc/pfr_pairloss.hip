// pfr_pairloss.hip — pair losses on the Gram matrix of the batch itself: supervised contrastive (Khosla et al. 2020, L_out) and Circle
// loss (Sun et al. 2020, per anchor), one forward launch and one backward launch on the L2-normalised rows ê that pfr_l2norm_fwd wrote.
// The contract (sets, formulas, reduction) is the comment at pfr_pair_loss_fwd in include/pfr_hip.h.  Not in the reference.
// What these kernels share with the cross-batch-memory ones (pfr_pairmem.hip) is in pfr_pairloss.h.
//
// Data flow (both kernels): a workgroup of 4 waves owns a block of 32 anchors and walks the batch in tiles of 32 partners.  A score tile
// is ONE 32x32 MFMA accumulator per wave, computed TRANSPOSED: the partner rows are the MFMA "A" operand (accumulator row), the anchor
// rows the "B" operand (accumulator column = lane & 31).  So a lane holds ONE anchor and 16 partners of it per tile:
//   * forward: the online (max, sum) of each log-sum-exp lives in the lane, no cross-lane traffic while the tiles stream; the four waves
//     take different tiles and their states meet once, in LDS, in wave order.  Nothing B x B is written.  The last workgroup to finish
//     (an integer ticket) sums the per-anchor losses in a fixed order: no floating-point atomics, the same bits every call.
//   * backward: G_ij = W_ij + W_ji is formed in the accumulator registers (W_ji needs only anchor j's statistics and the same s_ij) and
//     is, as it stands, the "A" operand of the second product dê[i][d] = sum_j G[i][j] ê[j][d] (an accumulator tile as the next MFMA's
//     operand: the sum runs over the tile's ROW index, so there is no lane movement and no LDS; the k order inside a step is permuted to
//     j = 16 s + 8 (e >> 2) + 4 half + (e & 3) and the other operand, read from êᵀ, follows it).  Every wave recomputes the score tile
//     (D / 16 MFMAs) and owns a slice of D of the [32][D] result in registers; one pass, plain stores.
// Operands come straight from global memory in fragment form (16 bytes per lane per k-step; the whole ê is 0.25-1 MB and lives in L2).
#include "pfr_pairloss.h"


// acc[t][q] = ê[j0[t] + acc_row(q, lane)] . ê[r0 + (lane & 31)] for TP partner tiles against one anchor block
template <typename T, int TP>
__device__ __forceinline__ void pl_scores(const char* xn, int B, int rowbytes, int r0, const int (&j0)[TP], int lane, f32x16 (&acc)[TP]) {
  const int row = lane & 31, half = lane >> 5;
  const int nk = (rowbytes + 31) >> 5;
#pragma unroll
  for (int t = 0; t < TP; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
  // four k-steps per trip, their loads in flight together (a step past the row's end reads zeros)
  for (int s0 = 0; s0 < nk; s0 += 4)
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int boff = (s0 + u) * 32 + half * 16;
    const u32x4 fb = pl_frag(xn, r0 + row, B, rowbytes, boff);
    u32x4 fa[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) fa[t] = pl_frag(xn, j0[t] + row, B, rowbytes, boff);
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      if constexpr (sizeof(T) == 2) {
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[t]), __builtin_bit_cast(bf16x8, fb), acc[t], 0, 0, 0);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[t][e]), __uint_as_float(fb[e]), acc[t], 0, 0, 0);
      }
    }
  }
}


template <typename T, int KIND>
__global__ __launch_bounds__(256) void pair_loss_fwd_kernel(const char* __restrict__ xn, const int64_t* __restrict__ label, int B, int D, float p0,
                                                            float p1, float* __restrict__ stats, float* __restrict__ ell, float* __restrict__ out,
                                                            int* __restrict__ counter) {
  constexpr int TP = 2;
  __shared__ float red[4][PL_NSTAT][32];
  __shared__ float fin[2][4];
  __shared__ int is_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * 32;
  const int rowbytes = D * (int)sizeof(T);
  const int ntiles = (B + 31) >> 5;
  const int i = r0 + (lane & 31);
  const int64_t yi = label[min(i, B - 1)];
  float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f, psum = 0.f;
  int cp = 0, cn = 0;
  for (int tb = wave * TP; tb < ntiles; tb += 4 * TP) {
    int j0[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) j0[t] = (tb + t) * 32;
    f32x16 acc[TP];
    pl_scores<T, TP>(xn, B, rowbytes, r0, j0, lane, acc);
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      float x[16];
      bool k1[16], k2[16];
      float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = j0[t] + acc_row(q, lane);
        const bool in = i < B && j < B && j != i;
        const bool same = label[min(j, B - 1)] == yi;
        float slope;
        pl_logit<KIND>(acc[t][q], same, p0, p1, x[q], slope);
        if constexpr (KIND == PL_SUPCON) {
          k1[q] = in;            // the denominator: every a != i
          k2[q] = false;
          if (in && same) { psum += x[q]; ++cp; }
        } else {
          k1[q] = in && same;    // positives
          k2[q] = in && !same;   // negatives (j != i holds)
          cp += k1[q];
          cn += k2[q];
        }
        t1 = k1[q] ? fmaxf(t1, x[q]) : t1;
        t2 = k2[q] ? fmaxf(t2, x[q]) : t2;
      }
      const float n1 = fmaxf(m1, t1), n2 = fmaxf(m2, t2);
      float a1 = m1 == -INFINITY ? 0.f : s1 * expf(m1 - n1);
      float a2 = m2 == -INFINITY ? 0.f : s2 * expf(m2 - n2);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        a1 += k1[q] ? expf(x[q] - n1) : 0.f;
        if constexpr (KIND == PL_CIRCLE) a2 += k2[q] ? expf(x[q] - n2) : 0.f;
      }
      m1 = n1; s1 = a1; m2 = n2; s2 = a2;
    }
  }
  // the two lane halves hold the same anchor: half 1 into half 0
  pl_merge(m1, s1, __shfl_xor(m1, 32, 64), __shfl_xor(s1, 32, 64));
  pl_merge(m2, s2, __shfl_xor(m2, 32, 64), __shfl_xor(s2, 32, 64));
  psum += __shfl_xor(psum, 32, 64);
  cp += __shfl_xor(cp, 32, 64);
  cn += __shfl_xor(cn, 32, 64);
  if (lane < 32) {
    red[wave][0][lane] = m1; red[wave][1][lane] = s1; red[wave][2][lane] = m2; red[wave][3][lane] = s2;
    red[wave][4][lane] = psum; red[wave][5][lane] = (float)cp; red[wave][6][lane] = (float)cn;   // counts <= B: exact in fp32 below 2^24
  }
  __syncthreads();
  if (tid < 32) {
    for (int w = 1; w < 4; ++w) {   // wave order: fixed
      pl_merge(m1, s1, red[w][0][tid], red[w][1][tid]);
      pl_merge(m2, s2, red[w][2][tid], red[w][3][tid]);
      psum += red[w][4][tid];
      cp += (int)red[w][5][tid];
      cn += (int)red[w][6][tid];
    }
    float st0 = 0.f, st1 = 0.f, st2 = 0.f, l = 0.f;
    bool valid;
    if constexpr (KIND == PL_SUPCON) {
      valid = cp > 0;
      if (valid) {
        st0 = m1 + logf(s1);
        st1 = 1.f / (float)cp;
        st2 = 1.f;
        l = st0 - psum * st1;
      }
    } else {
      valid = cp > 0 && cn > 0;
      if (valid) {
        st0 = m1 + logf(s1);
        st1 = m2 + logf(s2);
        const float z = st0 + st1;
        l = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
        st2 = 1.f / (1.f + expf(-z));
      }
    }
    if (i < B) {
      reinterpret_cast<f32x4*>(stats)[i] = f32x4{st0, st1, st2, valid ? 1.f : 0.f};
      // l_i >= 0 for both kinds (a rounding below 0 is clamped): < 0 marks an invalid anchor until the reduction below
      __hip_atomic_store(ell + i, valid ? fmaxf(l, 0.f) : -1.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __threadfence();   // release: this workgroup's rows before its ticket
    if (tid == 0) is_last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();     // acquire: every workgroup's rows
  // loss = sum over the valid anchors / A: strided partial sums, lane tree, wave order; the same order whichever workgroup is last
  float sum = 0.f, cnt = 0.f;
  for (int r = tid; r < B; r += 256) {
    const float v = __hip_atomic_load(ell + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v >= 0.f) { sum += v; cnt += 1.f; }
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if (lane == 0) { fin[0][wave] = sum; fin[1][wave] = cnt; }
  __syncthreads();
  if (tid == 0) {
    const float S = ((fin[0][0] + fin[0][1]) + fin[0][2]) + fin[0][3];
    const float A = ((fin[1][0] + fin[1][1]) + fin[1][2]) + fin[1][3];
    out[0] = A > 0.f ? S / A : 0.f;
    out[1] = A > 0.f ? 1.f / A : 0.f;
    out[2] = A;
    __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch on this stream
  }
  // ell of an invalid anchor is 0 for the caller
  for (int r = tid; r < B; r += 256) {
    const float v = __hip_atomic_load(ell + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v < 0.f) ell[r] = 0.f;
  }
}


template <typename T, int KIND, int TD>
__global__ __launch_bounds__(256) void pair_loss_bwd_kernel(const char* __restrict__ xn, const T* __restrict__ xnT, int ldt,
                                                            const int64_t* __restrict__ label, int B, int D, float p0, float p1,
                                                            const float* __restrict__ stats, const float* __restrict__ out, float grad_scale,
                                                            const float* __restrict__ grad_scale_dev, float* __restrict__ dxn) {
  constexpr int TP = 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (wave * 32 >= D) return;   // (no barrier below: a wave without a slice of D has nothing to do)
  const int row = lane & 31, half = lane >> 5;
  const int r0 = blockIdx.x * 32;
  const int rowbytes = D * (int)sizeof(T);
  const int ntiles = (B + 31) >> 5;
  const int i = r0 + row;
  const int64_t yi = label[min(i, B - 1)];
  const f32x4 sti = reinterpret_cast<const f32x4*>(stats)[min(i, B - 1)];
  const float scale = grad_scale * (grad_scale_dev ? grad_scale_dev[0] : 1.f) * out[1];
  f32x16 accd[TD];
#pragma unroll
  for (int t = 0; t < TD; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) accd[t][q] = 0.f;
  for (int tb = 0; tb < ntiles; tb += TP) {
    int j0[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) j0[t] = (tb + t) * 32;
    f32x16 g[TP];
    pl_scores<T, TP>(xn, B, rowbytes, r0, j0, lane, g);
#pragma unroll
    for (int t = 0; t < TP; ++t) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = j0[t] + acc_row(q, lane);
        const int jc = min(j, B - 1);
        const bool in = i < B && j < B && j != i;
        const bool same = label[jc] == yi;
        const f32x4 stj = reinterpret_cast<const f32x4*>(stats)[jc];
        float x, slope;
        pl_logit<KIND>(g[t][q], same, p0, p1, x, slope);
        const float w = pl_weight<KIND>(sti, x, slope, same) + pl_weight<KIND>(stj, x, slope, same);
        g[t][q] = in ? w * scale : 0.f;
      }
      if (j0[t] >= B) continue;   // (the odd tail tile of the pair: all zero)
      // dê[i][d] += sum_j G[i][j] ê[j][d]: G's registers are the A fragment, êᵀ[d][j ...] the B fragment in the same k order
#pragma unroll
      for (int td = 0; td < TD; ++td) {
        const int d = (wave + 4 * td) * 32 + row;
        const bool dok = d < D;
        const T* src = xnT + (size_t)(dok ? d : 0) * ldt + j0[t] + 4 * half;
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            float gf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) gf[e] = g[t][8 * s + e];
            const u32x4 fa = Chunk<bf16_t>::pack(gf);
            const u32x2 lo = *reinterpret_cast<const u32x2*>(src + 16 * s);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(src + 16 * s + 8);
            u32x4 fb = u32x4{lo[0], lo[1], hi[0], hi[1]};
            if (!dok) fb = u32x4{0u, 0u, 0u, 0u};
            accd[td] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa), __builtin_bit_cast(bf16x8, fb), accd[td], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int qg = 0; qg < 4; ++qg) {
            f32x4 fb = *reinterpret_cast<const f32x4*>(src + 8 * qg);
            if (!dok) fb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) accd[td] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[t][4 * qg + e], fb[e], accd[td], 0, 0, 0);
          }
        }
      }
    }
  }
#pragma unroll
  for (int td = 0; td < TD; ++td) {
    const int d = (wave + 4 * td) * 32 + row;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = r0 + acc_row(q, lane);
      if (r < B && d < D) dxn[(size_t)r * D + d] = accd[td][q];
    }
  }
}


extern "C" int pfr_pair_loss_fwd(const void* xn, int dtype, const int64_t* label, int B, int D, int kind, float p0, float p1, float* stats,
                                 float* ell, float* out, int* counter, hipStream_t st) {
  const int rc = pl_check("pfr_pair_loss_fwd", xn, dtype, label, B, D, kind, p0, p1);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(stats && ell && out && counter, "pfr_pair_loss_fwd: null pointer");
  const dim3 grid((B + 31) / 32), block(256);
  const float q0 = kind == PL_SUPCON ? 1.f / p0 : p0;
#define PLF(T, K) hipLaunchKernelGGL((pair_loss_fwd_kernel<T, K>), grid, block, 0, st, (const char*)xn, label, B, D, q0, p1, stats, ell, out, counter)
  if (dtype == PFR_BF16) { if (kind == PL_SUPCON) PLF(bf16_t, PL_SUPCON); else PLF(bf16_t, PL_CIRCLE); }
  else { if (kind == PL_SUPCON) PLF(float, PL_SUPCON); else PLF(float, PL_CIRCLE); }
#undef PLF
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_pair_loss_bwd(const void* xn, const void* xnT, int dtype, int ldt, const int64_t* label, int B, int D, int kind, float p0,
                                 float p1, const float* stats, const float* out, float grad_scale, const float* grad_scale_dev, float* dxn,
                                 hipStream_t st) {
  const int rc = pl_check("pfr_pair_loss_bwd", xn, dtype, label, B, D, kind, p0, p1);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(xnT && stats && out && dxn, "pfr_pair_loss_bwd: null pointer");
  PFR_CHECK_ARG(ldt >= (B + 31) / 32 * 32 && ldt % 32 == 0, "pfr_pair_loss_bwd: the transposed copy needs ldt = a multiple of 32 >= B (zero pad columns), got %d", ldt);
  const dim3 grid((B + 31) / 32), block(256);
  const float q0 = kind == PL_SUPCON ? 1.f / p0 : p0;
#define PLB(T, K, TD) hipLaunchKernelGGL((pair_loss_bwd_kernel<T, K, TD>), grid, block, 0, st, (const char*)xn, (const T*)xnT, ldt, label, B, D, q0, p1, stats, out, grad_scale, grad_scale_dev, dxn)
#define PLB2(T, K) do { if (D <= 512) PLB(T, K, 4); else PLB(T, K, 8); } while (0)
  if (dtype == PFR_BF16) { if (kind == PL_SUPCON) PLB2(bf16_t, PL_SUPCON); else PLB2(bf16_t, PL_CIRCLE); }
  else { if (kind == PL_SUPCON) PLB2(float, PL_SUPCON); else PLB2(float, PL_CIRCLE); }
#undef PLB2
#undef PLB
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
