// pfr_pairmem.hip — the pair losses of pfr_pairloss.hip with a cross-batch memory (Wang et al., CVPR 2020): every anchor of the batch also
// pairs with the live slots of a ring of past embeddings, which carry no gradient.  The contract is the comment at pfr_pair_mem_loss_fwd
// in include/pfr_hip.h.  Not in the reference.
//
// The partners of an anchor block are the 32-row tiles of the batch (nb = ceil(B / 32) tiles, the last one ragged) followed by the tiles
// of the live slots (nm = ceil(count / 32), the last one ragged): a tile is either a batch tile or a memory tile, never both.  The grid is
// (anchor blocks) x (S splits of that tile list); split sp owns the tiles [sp nt / S, (sp + 1) nt / S), possibly none.
//   * forward: as pair_loss_fwd_kernel, a lane holds one anchor and its online (max, sum) states while the tiles of the split stream.
//     S = 1: the workgroup finishes its anchors itself.  S > 1: it writes the partial state [8] of each anchor; the last workgroup of the
//     launch (an integer ticket) merges the S states of every anchor IN SPLIT ORDER, finishes the anchors and sums the scalar in a fixed
//     order.  No floating-point atomics.
//   * backward: the four waves of a workgroup score four DIFFERENT tiles, turn the scores into G in the accumulator registers
//     (W_rj + W_jr for a batch partner, W_rk alone for a slot), pack G as the MFMA "A" fragment and hand it to the other waves through LDS
//     (a fragment is lane-resident: lane l of every wave reads what lane l of the producer wrote, no conflicts; two buffers, one barrier
//     per four tiles).  Every wave owns a slice of D and multiplies every G tile with êᵀ or mT for its slice.  S = 1 writes dê, S > 1 a
//     slab per split, and pair_mem_reduce_kernel sums the slabs in split order.
//   * push: rows, transposed columns and labels of a batch into the ring at (head + r) mod M.
#include "pfr_pairloss.h"

#define PM_WS_STATE 8                          // floats per (split, anchor) of the forward workspace
#define PM_SLAB_BUDGET (64ll << 20)            // bytes of backward slabs pfr_pair_mem_splits stays under
#define PM_MAX_SPLITS 4096

// linear block id -> (anchor block, split).  order 0: the anchor block is the fast index.  order 1: workgroups are dealt round-robin over
// the 8 XCDs by linear id, so ids with the same id % 8 share an L2; give every such class a contiguous run of the (split, block) list, so
// that the anchor blocks that read one partner range go through one L2 (a bijection for every grid size)
__device__ __forceinline__ void pm_block(int order, int nblk, int& blk, int& sp) {
  int id = blockIdx.x;
  if (order) {
    const int total = gridDim.x, q = total >> 3, r = total & 7, x = id & 7;
    id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
  }
  blk = id % nblk;
  sp = id / nblk;
}

// acc[q] = partner[j0 + acc_row(q, lane)] . ê[r0 + (lane & 31)]; partner rows >= prows read as zeros whatever the memory holds there
template <typename T>
__device__ __forceinline__ void pm_scores(const char* xn, int B, const char* part, int prows, int rowbytes, int r0, int j0, int lane, f32x16& acc) {
  const int row = lane & 31, half = lane >> 5;
  const int nk = (rowbytes + 31) >> 5;
#pragma unroll
  for (int q = 0; q < 16; ++q) acc[q] = 0.f;
  for (int s0 = 0; s0 < nk; s0 += 4) {
    u32x4 fa[4], fb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int boff = (s0 + u) * 32 + half * 16;
      fb[u] = pl_frag(xn, r0 + row, B, rowbytes, boff);
      fa[u] = pl_frag(part, j0 + row, prows, rowbytes, boff);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (sizeof(T) == 2) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[u]), __builtin_bit_cast(bf16x8, fb[u]), acc, 0, 0, 0);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[u][e]), __uint_as_float(fb[u][e]), acc, 0, 0, 0);
      }
    }
  }
}

// the merged state of an anchor -> its statistics, loss and validity (the arithmetic of pair_loss_fwd_kernel)
template <int KIND>
__device__ __forceinline__ bool pm_finish(float m1, float s1, float m2, float s2, float psum, int cp, int cn, f32x4& st, float& l) {
  st = f32x4{0.f, 0.f, 0.f, 0.f};
  l = 0.f;
  bool valid;
  if constexpr (KIND == PL_SUPCON) {
    valid = cp > 0;
    if (valid) {
      st[0] = m1 + logf(s1);
      st[1] = 1.f / (float)cp;
      st[2] = 1.f;
      l = st[0] - psum * st[1];
    }
  } else {
    valid = cp > 0 && cn > 0;
    if (valid) {
      st[0] = m1 + logf(s1);
      st[1] = m2 + logf(s2);
      const float z = st[0] + st[1];
      l = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
      st[2] = 1.f / (1.f + expf(-z));
    }
  }
  st[3] = valid ? 1.f : 0.f;
  l = fmaxf(l, 0.f);   // l_i >= 0 for both kinds (a rounding below 0 is clamped)
  return valid;
}

__device__ __forceinline__ float pm_ld(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <typename T, int KIND>
__global__ __launch_bounds__(256) void pair_mem_fwd_kernel(const char* __restrict__ xn, const int64_t* __restrict__ label, int B, int D,
                                                           const char* __restrict__ mem, const int64_t* __restrict__ mem_label, int count, float p0,
                                                           float p1, int S, int order, float* __restrict__ ws, float* __restrict__ stats,
                                                           float* __restrict__ ell, float* __restrict__ out, int* __restrict__ counter) {
  __shared__ float red[4][PL_NSTAT][32];
  __shared__ float fin[2][4];
  __shared__ int is_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = (B + 31) >> 5, nm = (count + 31) >> 5, nt = nb + nm;
  int blk, sp;
  pm_block(order, nb, blk, sp);
  const int t_lo = (int)((long long)sp * nt / S), t_hi = (int)((long long)(sp + 1) * nt / S);
  const int r0 = blk * 32;
  const int rowbytes = D * (int)sizeof(T);
  const int i = r0 + (lane & 31);
  const int64_t yi = label[min(i, B - 1)];
  float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f, psum = 0.f;
  int cp = 0, cn = 0;
  for (int t = t_lo + wave; t < t_hi; t += 4) {
    const bool isb = t < nb;
    const char* part = isb ? xn : mem;
    const int64_t* plab = isb ? label : mem_label;
    const int prows = isb ? B : count, j0 = (isb ? t : t - nb) * 32;
    f32x16 acc;
    pm_scores<T>(xn, B, part, prows, rowbytes, r0, j0, lane, acc);
    float x[16];
    bool k1[16], k2[16];
    float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = j0 + acc_row(q, lane);
      const bool in = i < B && j < prows && !(isb && j == i);
      const bool same = plab[min(j, prows - 1)] == yi;
      float slope;
      pl_logit<KIND>(acc[q], same, p0, p1, x[q], slope);
      if constexpr (KIND == PL_SUPCON) {
        k1[q] = in;            // the denominator: every partner
        k2[q] = false;
        if (in && same) { psum += x[q]; ++cp; }
      } else {
        k1[q] = in && same;    // positives
        k2[q] = in && !same;   // negatives
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
  // the two lane halves hold the same anchor: half 1 into half 0
  pl_merge(m1, s1, __shfl_xor(m1, 32, 64), __shfl_xor(s1, 32, 64));
  pl_merge(m2, s2, __shfl_xor(m2, 32, 64), __shfl_xor(s2, 32, 64));
  psum += __shfl_xor(psum, 32, 64);
  cp += __shfl_xor(cp, 32, 64);
  cn += __shfl_xor(cn, 32, 64);
  if (lane < 32) {   // (counts travel as their integer bits: B + count may pass 2^24)
    red[wave][0][lane] = m1; red[wave][1][lane] = s1; red[wave][2][lane] = m2; red[wave][3][lane] = s2;
    red[wave][4][lane] = psum; red[wave][5][lane] = __int_as_float(cp); red[wave][6][lane] = __int_as_float(cn);
  }
  __syncthreads();
  if (tid < 32) {
    for (int w = 1; w < 4; ++w) {   // wave order: fixed
      pl_merge(m1, s1, red[w][0][tid], red[w][1][tid]);
      pl_merge(m2, s2, red[w][2][tid], red[w][3][tid]);
      psum += red[w][4][tid];
      cp += __float_as_int(red[w][5][tid]);
      cn += __float_as_int(red[w][6][tid]);
    }
    if (i < B) {
      if (S == 1) {
        f32x4 st;
        float l;
        const bool valid = pm_finish<KIND>(m1, s1, m2, s2, psum, cp, cn, st, l);
        reinterpret_cast<f32x4*>(stats)[i] = st;
        // < 0 marks an invalid anchor until the reduction below
        __hip_atomic_store(ell + i, valid ? l : -1.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        float* w = ws + ((size_t)sp * B + i) * PM_WS_STATE;
        const float v[PM_WS_STATE] = {m1, s1, m2, s2, psum, __int_as_float(cp), __int_as_float(cn), 0.f};
#pragma unroll
        for (int k = 0; k < PM_WS_STATE; ++k) __hip_atomic_store(w + k, v[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __threadfence();   // release: this workgroup's rows before its ticket
    if (tid == 0) is_last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();     // acquire: every workgroup's rows
  // S > 1: merge the S partial states of every anchor in split order and finish it.  Then loss = sum over the valid anchors / A: strided
  // partial sums, lane tree, wave order; the same order whichever workgroup is last
  float sum = 0.f, cnt = 0.f;
  for (int r = tid; r < B; r += 256) {
    float l;
    bool valid;
    if (S == 1) {
      l = pm_ld(ell + r);
      valid = l >= 0.f;
    } else {
      float a1 = -INFINITY, b1 = 0.f, a2 = -INFINITY, b2 = 0.f, ps = 0.f;
      int np = 0, nn = 0;
      for (int s = 0; s < S; ++s) {
        const float* w = ws + ((size_t)s * B + r) * PM_WS_STATE;
        pl_merge(a1, b1, pm_ld(w + 0), pm_ld(w + 1));
        pl_merge(a2, b2, pm_ld(w + 2), pm_ld(w + 3));
        ps += pm_ld(w + 4);
        np += __float_as_int(pm_ld(w + 5));
        nn += __float_as_int(pm_ld(w + 6));
      }
      f32x4 st;
      valid = pm_finish<KIND>(a1, b1, a2, b2, ps, np, nn, st, l);
      reinterpret_cast<f32x4*>(stats)[r] = st;
    }
    if (valid) { sum += l; cnt += 1.f; }
    ell[r] = valid ? l : 0.f;   // ell of an invalid anchor is 0 for the caller
  }
  sum = wave_sum(sum);
  cnt = wave_sum(cnt);
  if (lane == 0) { fin[0][wave] = sum; fin[1][wave] = cnt; }
  __syncthreads();
  if (tid == 0) {
    const float Ssum = ((fin[0][0] + fin[0][1]) + fin[0][2]) + fin[0][3];
    const float A = ((fin[1][0] + fin[1][1]) + fin[1][2]) + fin[1][3];
    out[0] = A > 0.f ? Ssum / A : 0.f;
    out[1] = A > 0.f ? 1.f / A : 0.f;
    out[2] = A;
    __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch on this stream
  }
}

template <typename T> struct PmFrag;   // G of one tile as MFMA "A" fragments: NQ 16-byte pieces per lane
template <> struct PmFrag<bf16_t> { static constexpr int NQ = 2; };
template <> struct PmFrag<float> { static constexpr int NQ = 4; };

template <typename T, int KIND, int TD>
__global__ __launch_bounds__(256) void pair_mem_bwd_kernel(const char* __restrict__ xn, const T* __restrict__ xnT, int ldt, const int64_t* __restrict__ label,
                                                           int B, int D, const char* __restrict__ mem, const T* __restrict__ memT, int ldm,
                                                           const int64_t* __restrict__ mem_label, int count, float p0, float p1,
                                                           const float* __restrict__ stats, const float* __restrict__ out, float grad_scale,
                                                           const float* __restrict__ grad_scale_dev, int S, int order, float* __restrict__ dst) {
  constexpr int NQ = PmFrag<T>::NQ;
  __shared__ u32x4 gl[2][4][NQ][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = lane & 31, half = lane >> 5;
  const int nb = (B + 31) >> 5, nm = (count + 31) >> 5, nt = nb + nm;
  int blk, sp;
  pm_block(order, nb, blk, sp);
  const int t_lo = (int)((long long)sp * nt / S), t_hi = (int)((long long)(sp + 1) * nt / S);
  const int r0 = blk * 32;
  const int rowbytes = D * (int)sizeof(T);
  const int i = r0 + row;
  const int64_t yi = label[min(i, B - 1)];
  const f32x4 sti = reinterpret_cast<const f32x4*>(stats)[min(i, B - 1)];
  const float scale = grad_scale * (grad_scale_dev ? grad_scale_dev[0] : 1.f) * out[1];
  f32x16 accd[TD];
#pragma unroll
  for (int t = 0; t < TD; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) accd[t][q] = 0.f;
  int buf = 0;
  for (int tg = t_lo; tg < t_hi; tg += 4, buf ^= 1) {
    const int t = tg + wave;
    if (t < t_hi) {   // this wave's tile of the four: scores -> G -> LDS
      const bool isb = t < nb;
      const char* part = isb ? xn : mem;
      const int64_t* plab = isb ? label : mem_label;
      const int prows = isb ? B : count, j0 = (isb ? t : t - nb) * 32;
      f32x16 g;
      pm_scores<T>(xn, B, part, prows, rowbytes, r0, j0, lane, g);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = j0 + acc_row(q, lane);
        const int jc = min(j, prows - 1);
        const bool in = i < B && j < prows && !(isb && j == i);
        const bool same = plab[jc] == yi;
        float x, slope;
        pl_logit<KIND>(g[q], same, p0, p1, x, slope);
        float w = pl_weight<KIND>(sti, x, slope, same);
        if (isb) w += pl_weight<KIND>(reinterpret_cast<const f32x4*>(stats)[jc], x, slope, same);   // W_jr: batch partners are anchors too
        g[q] = in ? w * scale : 0.f;
      }
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float gf[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) gf[e] = g[8 * s + e];
          gl[buf][wave][s][lane] = Chunk<bf16_t>::pack(gf);
        }
      } else {
#pragma unroll
        for (int qg = 0; qg < 4; ++qg)
          gl[buf][wave][qg][lane] = u32x4{__float_as_uint(g[4 * qg]), __float_as_uint(g[4 * qg + 1]), __float_as_uint(g[4 * qg + 2]), __float_as_uint(g[4 * qg + 3])};
      }
    }
    __syncthreads();
    if (wave * 32 < D) {   // (a wave without a slice of D only scores)
      for (int u = 0; u < 4 && tg + u < t_hi; ++u) {
        const int tu = tg + u;
        const bool isb = tu < nb;
        const T* baseT = isb ? xnT : memT;
        const int ld = isb ? ldt : ldm, j0 = (isb ? tu : tu - nb) * 32;
        u32x4 fa[NQ];
#pragma unroll
        for (int s = 0; s < NQ; ++s) fa[s] = gl[buf][u][s][lane];
        // dê[i][d] += sum_j G[i][j] p[j][d]: G's registers are the A fragment, pᵀ[d][j ...] the B fragment in the same k order
#pragma unroll
        for (int td = 0; td < TD; ++td) {
          const int d = (wave + 4 * td) * 32 + row;
          const bool dok = d < D;
          const T* src = baseT + (size_t)(dok ? d : 0) * ld + j0 + 4 * half;
          if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
              const u32x2 lo = *reinterpret_cast<const u32x2*>(src + 16 * s);
              const u32x2 hi = *reinterpret_cast<const u32x2*>(src + 16 * s + 8);
              u32x4 fb = u32x4{lo[0], lo[1], hi[0], hi[1]};
              if (!dok) fb = u32x4{0u, 0u, 0u, 0u};
              accd[td] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[s]), __builtin_bit_cast(bf16x8, fb), accd[td], 0, 0, 0);
            }
          } else {
#pragma unroll
            for (int qg = 0; qg < 4; ++qg) {
              f32x4 fb = *reinterpret_cast<const f32x4*>(src + 8 * qg);
              if (!dok) fb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int e = 0; e < 4; ++e) accd[td] = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(fa[qg][e]), fb[e], accd[td], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  float* o = dst + (size_t)sp * B * D;   // S = 1: dê itself; S > 1: the slab of this split
#pragma unroll
  for (int td = 0; td < TD; ++td) {
    const int d = (wave + 4 * td) * 32 + row;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = r0 + acc_row(q, lane);
      if (r < B && d < D) o[(size_t)r * D + d] = accd[td][q];
    }
  }
}

// dê = slab 0 + slab 1 + ... in split order, four elements per thread (n = B D is a multiple of 8)
__global__ __launch_bounds__(256) void pair_mem_reduce_kernel(const float* __restrict__ ws, size_t n, int S, float* __restrict__ dxn) {
  const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= n) return;
  f32x4 a = *reinterpret_cast<const f32x4*>(ws + e);
  for (int s = 1; s < S; ++s) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(ws + (size_t)s * n + e);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] += b[k];
  }
  *reinterpret_cast<f32x4*>(dxn + e) = a;
}

// ring push: E = the element as an integer of its size.  First the rows (d fast: coalesced into mem), then the columns (r fast:
// consecutive slots of one row of memT, up to the wrap), then the labels
template <typename E>
__global__ __launch_bounds__(256) void pair_mem_push_kernel(const E* __restrict__ xn, const int64_t* __restrict__ label, int B, int D, E* __restrict__ mem,
                                                            E* __restrict__ memT, int ldm, int64_t* __restrict__ mem_label, int M, int head) {
  const size_t n = (size_t)B * D, step = (size_t)gridDim.x * 256, first = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (size_t e = first; e < n; e += step) {
    const int r = (int)(e / D), d = (int)(e % D);
    mem[(size_t)((head + r) % M) * D + d] = xn[e];
  }
  for (size_t e = first; e < n; e += step) {
    const int d = (int)(e / B), r = (int)(e % B);
    memT[(size_t)d * ldm + (head + r) % M] = xn[(size_t)r * D + d];
  }
  for (size_t e = first; e < (size_t)B; e += step) mem_label[(head + (int)e) % M] = label[e];
}

static int pm_check(const char* who, const void* xn, int dtype, const void* label, int B, int D, int kind, float p0, float p1, const void* mem,
                    const void* mem_label, int M, int count, int splits) {
  const int rc = pl_check(who, xn, dtype, label, B, D, kind, p0, p1);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(mem && mem_label, "%s: null pointer", who);
  PFR_CHECK_ARG(M >= 32 && M % 32 == 0 && M < (1 << 24), "%s: the ring needs M = a multiple of 32 with 32 <= M < 2^24, got %d", who, M);
  PFR_CHECK_ARG(count >= 0 && count <= M, "%s: need 0 <= count <= M, got count=%d M=%d", who, count, M);
  PFR_CHECK_ARG(splits >= 0 && splits <= PM_MAX_SPLITS, "%s: splits must be 0 (auto) or in [1, %d], got %d", who, PM_MAX_SPLITS, splits);
  return PFR_OK;
}

// one workgroup per CU of a 256-CU part, at least four tiles (one per wave) a split, the backward slabs within PM_SLAB_BUDGET
extern "C" int pfr_pair_mem_splits(int B, int count, int D) {
  if (B < 1 || count < 0 || D < 1) return 1;
  const long long nb = (B + 31) / 32, nt = nb + (count + 31) / 32;
  long long s = 256 / nb;
  if (s > (nt + 3) / 4) s = (nt + 3) / 4;
  const long long cap = PM_SLAB_BUDGET / ((long long)B * D * 4);
  if (s > cap) s = cap;
  if (s > PM_MAX_SPLITS) s = PM_MAX_SPLITS;
  return s < 1 ? 1 : (int)s;
}

static int pm_order() { return pfr_knob(KNOB_PAIR_MEM_ORDER) ? 1 : 0; }

extern "C" int pfr_pair_mem_loss_fwd(const void* xn, int dtype, const int64_t* label, int B, int D, const void* mem, const int64_t* mem_label, int M,
                                     int count, int kind, float p0, float p1, int splits, float* ws, float* stats, float* ell, float* out,
                                     int* counter, hipStream_t st) {
  const int rc = pm_check("pfr_pair_mem_loss_fwd", xn, dtype, label, B, D, kind, p0, p1, mem, mem_label, M, count, splits);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(stats && ell && out && counter, "pfr_pair_mem_loss_fwd: null pointer");
  const int S = splits ? splits : pfr_pair_mem_splits(B, count, D);
  PFR_CHECK_ARG(S == 1 || ws, "pfr_pair_mem_loss_fwd: workspace required (splits=%d)", S);
  const int nb = (B + 31) / 32;
  PFR_CHECK_ARG((long long)nb * S < (1ll << 31), "pfr_pair_mem_loss_fwd: too many workgroups (%d anchor blocks x %d splits)", nb, S);
  const dim3 grid(nb * S), block(256);
  const float q0 = kind == PL_SUPCON ? 1.f / p0 : p0;
  const int order = pm_order();
#define PMF(T, K) hipLaunchKernelGGL((pair_mem_fwd_kernel<T, K>), grid, block, 0, st, (const char*)xn, label, B, D, (const char*)mem, mem_label, count, q0, p1, S, order, ws, stats, ell, out, counter)
  if (dtype == PFR_BF16) { if (kind == PL_SUPCON) PMF(bf16_t, PL_SUPCON); else PMF(bf16_t, PL_CIRCLE); }
  else { if (kind == PL_SUPCON) PMF(float, PL_SUPCON); else PMF(float, PL_CIRCLE); }
#undef PMF
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_pair_mem_loss_bwd(const void* xn, const void* xnT, int dtype, int ldt, const int64_t* label, int B, int D, const void* mem,
                                     const void* memT, int ldm, const int64_t* mem_label, int M, int count, int kind, float p0, float p1,
                                     const float* stats, const float* out, float grad_scale, const float* grad_scale_dev, int splits, float* ws,
                                     float* dxn, hipStream_t st) {
  const int rc = pm_check("pfr_pair_mem_loss_bwd", xn, dtype, label, B, D, kind, p0, p1, mem, mem_label, M, count, splits);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(xnT && memT && stats && out && dxn, "pfr_pair_mem_loss_bwd: null pointer");
  PFR_CHECK_ARG(ldt >= (B + 31) / 32 * 32 && ldt % 32 == 0, "pfr_pair_mem_loss_bwd: the transposed copy needs ldt = a multiple of 32 >= B (zero pad columns), got %d", ldt);
  PFR_CHECK_ARG(ldm >= M && ldm % 32 == 0, "pfr_pair_mem_loss_bwd: the transposed ring needs ldm = a multiple of 32 >= M (zero beyond count), got %d", ldm);
  const int S = splits ? splits : pfr_pair_mem_splits(B, count, D);
  PFR_CHECK_ARG(S == 1 || ws, "pfr_pair_mem_loss_bwd: workspace required (splits=%d)", S);
  const int nb = (B + 31) / 32;
  PFR_CHECK_ARG((long long)nb * S < (1ll << 31), "pfr_pair_mem_loss_bwd: too many workgroups (%d anchor blocks x %d splits)", nb, S);
  const dim3 grid(nb * S), block(256);
  const float q0 = kind == PL_SUPCON ? 1.f / p0 : p0;
  const int order = pm_order();
  float* dst = S == 1 ? dxn : ws;
#define PMB(T, K, TD) hipLaunchKernelGGL((pair_mem_bwd_kernel<T, K, TD>), grid, block, 0, st, (const char*)xn, (const T*)xnT, ldt, label, B, D, (const char*)mem, (const T*)memT, ldm, mem_label, count, q0, p1, stats, out, grad_scale, grad_scale_dev, S, order, dst)
#define PMB2(T, K) do { if (D <= 512) PMB(T, K, 4); else PMB(T, K, 8); } while (0)
  if (dtype == PFR_BF16) { if (kind == PL_SUPCON) PMB2(bf16_t, PL_SUPCON); else PMB2(bf16_t, PL_CIRCLE); }
  else { if (kind == PL_SUPCON) PMB2(float, PL_SUPCON); else PMB2(float, PL_CIRCLE); }
#undef PMB2
#undef PMB
  PFR_CHECK_LAUNCH();
  if (S > 1) {
    const size_t n = (size_t)B * D;
    hipLaunchKernelGGL(pair_mem_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, (const float*)ws, n, S, dxn);
    PFR_CHECK_LAUNCH();
  }
  return PFR_OK;
}

extern "C" int pfr_pair_mem_push(const void* xn, const int64_t* label, int B, int D, int dtype, void* mem, void* memT, int ldm, int64_t* mem_label,
                                 int M, int head, hipStream_t st) {
  PFR_CHECK_ARG(xn && label && mem && memT && mem_label, "pfr_pair_mem_push: null pointer");
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "pfr_pair_mem_push: the compute dtype is fp32 or bf16 (int8 is not supported)");
  PFR_CHECK_ARG(D >= 8 && D % 8 == 0 && D <= 1024, "pfr_pair_mem_push: D must be a multiple of 8 in [8, 1024], got %d", D);
  PFR_CHECK_ARG(M >= 32 && M % 32 == 0 && M < (1 << 24), "pfr_pair_mem_push: the ring needs M = a multiple of 32 with 32 <= M < 2^24, got %d", M);
  PFR_CHECK_ARG(B >= 1 && B <= M, "pfr_pair_mem_push: need 1 <= B <= M, got B=%d M=%d", B, M);
  PFR_CHECK_ARG(ldm >= M && ldm % 32 == 0, "pfr_pair_mem_push: the transposed ring needs ldm = a multiple of 32 >= M, got %d", ldm);
  PFR_CHECK_ARG(head >= 0 && head < M, "pfr_pair_mem_push: need 0 <= head < M, got head=%d M=%d", head, M);
  const size_t n = (size_t)B * D;
  const dim3 grid((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), block(256);
  if (dtype == PFR_BF16)
    hipLaunchKernelGGL(pair_mem_push_kernel<uint16_t>, grid, block, 0, st, (const uint16_t*)xn, label, B, D, (uint16_t*)mem, (uint16_t*)memT, ldm, mem_label, M, head);
  else
    hipLaunchKernelGGL(pair_mem_push_kernel<uint32_t>, grid, block, 0, st, (const uint32_t*)xn, label, B, D, (uint32_t*)mem, (uint32_t*)memT, ldm, mem_label, M, head);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
