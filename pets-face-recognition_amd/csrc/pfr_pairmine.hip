// pfr_pairmine.hip — the mined pair losses: batch-hard triplet (Hermans et al. 2017) and Multi-Similarity with its miner (Wang et al.,
// CVPR 2019), on the partner list of pfr_pairmem.hip (the batch, then the live slots of an optional ring).  The contract is the comment
// at pfr_pair_mined_fwd in include/pfr_hip.h.  Not in the reference.
//
// Both need what a one-pass kernel cannot give: the hardest positive and the hardest negative of every anchor over ALL partners, before
// any pair is weighed.  So the forward is
//   * phase 1, the extremes: the transposed 32 x 32 score tile of pfr_pairmem.hip (a lane holds one anchor while the tiles of its split
//     stream); per-lane state (min positive, its partner number, max negative, its partner number, |P|, |N|), merged over the lane halves,
//     over the four waves in LDS in wave order, and over the S splits by the last workgroup of the launch (integer ticket).  The merge is
//     a total order (value, then the smaller partner number), so its result does not depend on the order at all.  batch_hard ends here.
//   * phase 2, multi_similarity only: a SECOND LAUNCH on the same stream (a grid-wide dependency is a launch, never a wait) scores the
//     tiles again, gates every pair with pmn_keep against the extremes of its anchor and accumulates the two online log-sum-exps.
// The backward of multi_similarity is the dense kernel of pfr_pairmem.hip with another weight (G in the accumulator, the second MFMA
// against êᵀ / memT, slabs when S > 1); the one of batch_hard is sparse: two weights per anchor, no GEMM.
#include "pfr_pairloss.h"
#include "pfr_scorekey.h"

#define PMN_BATCH_HARD 2
#define PMN_MS 3
#define PMN_STAT 8                             // floats per stats row, and per (split, anchor) of the forward workspace
#define PMN_MAX_SPLITS 4096

struct PmnParams { float a, b, c, d; };        // batch_hard: margin, gamma, -, -;  multi_similarity: alpha, beta, base, epsilon

// linear block id -> (anchor block, split): pm_block of pfr_pairmem.hip
__device__ __forceinline__ void pmn_block(int order, int nblk, int& blk, int& sp) {
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
__device__ __forceinline__ void pmn_scores(const char* xn, int B, const char* part, int prows, int rowbytes, int r0, int j0, int lane, f32x16& acc) {
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

// an extreme and its partner number as ONE 64-bit key, the keys of pfr_scorekey.h (pfr_extremes.hip): the larger key is the harder partner
// (negatives: the higher score; positives: the lower score, the order inverted), then the smaller number; -0.0 is +0.0 in the key; 0 =
// no partner yet (smaller than every key).  A merge is an integer max: a total order, whatever the order of the merges
__device__ __forceinline__ unsigned long long pmn_key(float s, int pn, bool positive) {
  const unsigned ord = db_score_key(s);
  return db_pack_key(positive ? ~ord : ord, pn);
}
__device__ __forceinline__ unsigned long long pmn_umax(unsigned long long x, unsigned long long y) { return x > y ? x : y; }
__device__ __forceinline__ unsigned long long pmn_u64(unsigned lo, unsigned hi) { return ((unsigned long long)hi << 32) | lo; }

// THE mining decision of multi_similarity, for the forward and the backward alike: a negative stays when s + eps > s_p*, a positive when
// s - eps < s_n* (each sum rounded once, never contracted)
__device__ __forceinline__ bool pmn_keep(float s, bool same, float sp, float sn, float eps) {
  return same ? __fsub_rn(s, eps) < sn : __fadd_rn(s, eps) > sp;
}
// the logit of a pair of multi_similarity: -alpha (s - base) for a positive, beta (s - base) for a negative (rounded on its own)
__device__ __forceinline__ float pmn_logit(float s, bool same, const PmnParams& p) {
  return __fmul_rn(same ? -p.a : p.b, __fsub_rn(s, p.c));
}
// d l_i / d s of a pair, given the stats row of its anchor (lo = slots 0-3, hi = slots 4-7)
__device__ __forceinline__ float pmn_weight(const f32x4& lo, const f32x4& hi, float s, bool same, const PmnParams& p) {
  if (hi[3] == 0.f || !pmn_keep(s, same, lo[0], lo[1], p.d)) return 0.f;
  const float x = pmn_logit(s, same, p);
  return same ? -expf(x - hi[0]) : expf(x - hi[1]);
}

__device__ __forceinline__ unsigned pmn_ld(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void pmn_st(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// phase 1: the merged extremes of anchor r -> its stats row; batch_hard: also z, f and l.  -> valid
template <int KIND>
__device__ __forceinline__ bool pmn_finish1(unsigned long long kp, unsigned long long kn, int cp, int cn, const PmnParams& p, unsigned* st, float& l) {
  const bool valid = cp > 0 && cn > 0;
  const float sp = db_key_score(~(unsigned)(kp >> 32)), sn = db_key_score((unsigned)(kn >> 32));
  const int ip = (int)(0xffffffffu - (unsigned)kp), in = (int)(0xffffffffu - (unsigned)kn);
  float z = 0.f, f = 0.f;
  l = 0.f;
  if constexpr (KIND == PMN_BATCH_HARD) {
    if (valid) {
      z = __fadd_rn(__fsub_rn(sn, sp), p.a);
      if (p.b == 0.f) {
        l = fmaxf(z, 0.f);
        f = z > 0.f ? 1.f : 0.f;
      } else {
        const float t = __fmul_rn(p.b, z);
        l = (fmaxf(t, 0.f) + log1pf(expf(-fabsf(t)))) / p.b;
        f = 1.f / (1.f + expf(-t));
      }
    }
  }
  pmn_st(st + 0, valid ? __float_as_uint(sp) : 0u);
  pmn_st(st + 1, valid ? __float_as_uint(sn) : 0u);
  pmn_st(st + 2, valid ? (unsigned)ip : 0xffffffffu);
  pmn_st(st + 3, valid ? (unsigned)in : 0xffffffffu);
  pmn_st(st + 4, __float_as_uint(z));
  pmn_st(st + 5, __float_as_uint(f));
  pmn_st(st + 6, 0u);
  pmn_st(st + 7, __float_as_uint(valid ? 1.f : 0.f));
  return valid;
}

// phase 2: the merged (max, sum) states of the kept positives and negatives of a valid anchor -> L_p, L_n (each log(1 + sum): the state
// merged with the element 0), the kept count and l
__device__ __forceinline__ void pmn_finish2(float m1, float s1, float m2, float s2, int kept, bool valid, const PmnParams& p, unsigned* st, float& l) {
  float Lp = 0.f, Ln = 0.f;
  l = 0.f;
  if (valid) {
    pl_merge(m1, s1, 0.f, 1.f);   // an empty kept set: (0, 1), log 1 = 0 exactly
    pl_merge(m2, s2, 0.f, 1.f);
    Lp = m1 + logf(s1);
    Ln = m2 + logf(s2);
    l = fmaxf(Lp / p.a + Ln / p.b, 0.f);
  }
  pmn_st(st + 4, __float_as_uint(Lp));
  pmn_st(st + 5, __float_as_uint(Ln));
  pmn_st(st + 6, __float_as_uint(valid ? (float)kept : 0.f));
}

// PHASE 1: extremes (and the whole of batch_hard).  PHASE 2 (multi_similarity): the gated log-sum-exps; reads slots 0, 1, 7 of stats as
// phase 1 left them.  `out` is written by the launch that ends the forward of its kind.
template <typename T, int KIND, int PHASE>
__global__ __launch_bounds__(256) void pair_mined_fwd_kernel(const char* __restrict__ xn, const int64_t* __restrict__ label, int B, int D,
                                                             const char* __restrict__ mem, const int64_t* __restrict__ mem_label, int count,
                                                             PmnParams p, int S, int order, unsigned* __restrict__ ws, unsigned* __restrict__ stats,
                                                             float* __restrict__ ell, float* __restrict__ out, int* __restrict__ counter) {
  __shared__ unsigned red[4][6][32];
  __shared__ float fin[2][4];
  __shared__ int is_last;
  constexpr bool ENDS = KIND == PMN_BATCH_HARD || PHASE == 2;   // this launch finishes l_i and the scalar
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = (B + 31) >> 5, nm = (count + 31) >> 5, nt = nb + nm;
  int blk, sp;
  pmn_block(order, nb, blk, sp);
  const int t_lo = (int)((long long)sp * nt / S), t_hi = (int)((long long)(sp + 1) * nt / S);
  const int r0 = blk * 32;
  const int rowbytes = D * (int)sizeof(T);
  const int i = r0 + (lane & 31), ic = min(i, B - 1);
  const int64_t yi = label[ic];
  // phase 1: ka = the key of the hardest positive, kb = of the hardest negative, c1 = |P|, c2 = |N|
  // phase 2: (a, a2) and (b, b2) the online (max, sum) of the kept positives and negatives, c1 = the kept pairs
  float a = -INFINITY, b = -INFINITY, a2 = 0.f, b2 = 0.f;
  unsigned long long ka = 0ull, kb = 0ull;
  int c1 = 0, c2 = 0;
  float spS = 0.f, snS = 0.f;
  bool vi = true;
  if constexpr (PHASE == 2) {
    spS = __uint_as_float(stats[(size_t)ic * PMN_STAT + 0]);
    snS = __uint_as_float(stats[(size_t)ic * PMN_STAT + 1]);
    vi = stats[(size_t)ic * PMN_STAT + 7] != 0u;
  }
  for (int t = t_lo + wave; t < t_hi; t += 4) {
    const bool isb = t < nb;
    const char* part = isb ? xn : mem;
    const int64_t* plab = isb ? label : mem_label;
    const int prows = isb ? B : count, j0 = (isb ? t : t - nb) * 32;
    f32x16 acc;
    pmn_scores<T>(xn, B, part, prows, rowbytes, r0, j0, lane, acc);
    if constexpr (PHASE == 1) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = j0 + acc_row(q, lane);
        const float s = acc[q];
        const bool in = i < B && j < prows && !(isb && j == i) && s == s;   // a NaN score counts for nothing
        const bool same = plab[min(j, prows - 1)] == yi;
        const int pn = isb ? j : B + j;
        const unsigned long long key = pmn_key(s, pn, same);
        c1 += in && same;
        c2 += in && !same;
        ka = pmn_umax(ka, in && same ? key : 0ull);
        kb = pmn_umax(kb, in && !same ? key : 0ull);
      }
    } else {
      float x[16];
      bool k1[16], k2[16];
      float t1 = -INFINITY, t2 = -INFINITY;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = j0 + acc_row(q, lane);
        const float s = acc[q];
        const bool in = vi && i < B && j < prows && !(isb && j == i) && s == s;
        const bool same = plab[min(j, prows - 1)] == yi;
        const bool keep = in && pmn_keep(s, same, spS, snS, p.d);
        x[q] = pmn_logit(s, same, p);
        k1[q] = keep && same;
        k2[q] = keep && !same;
        c1 += keep;
        t1 = k1[q] ? fmaxf(t1, x[q]) : t1;
        t2 = k2[q] ? fmaxf(t2, x[q]) : t2;
      }
      const float n1 = fmaxf(a, t1), n2 = fmaxf(b, t2);
      float e1 = a == -INFINITY ? 0.f : a2 * expf(a - n1);
      float e2 = b == -INFINITY ? 0.f : b2 * expf(b - n2);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        e1 += k1[q] ? expf(x[q] - n1) : 0.f;
        e2 += k2[q] ? expf(x[q] - n2) : 0.f;
      }
      a = n1; a2 = e1; b = n2; b2 = e2;
    }
  }
  // the two lane halves hold the same anchor: half 1 into half 0
  if constexpr (PHASE == 1) {
    ka = pmn_umax(ka, pmn_u64(__shfl_xor((unsigned)ka, 32, 64), __shfl_xor((unsigned)(ka >> 32), 32, 64)));
    kb = pmn_umax(kb, pmn_u64(__shfl_xor((unsigned)kb, 32, 64), __shfl_xor((unsigned)(kb >> 32), 32, 64)));
    c2 += __shfl_xor(c2, 32, 64);
  } else {
    pl_merge(a, a2, __shfl_xor(a, 32, 64), __shfl_xor(a2, 32, 64));
    pl_merge(b, b2, __shfl_xor(b, 32, 64), __shfl_xor(b2, 32, 64));
  }
  c1 += __shfl_xor(c1, 32, 64);
  // the state as six words: phase 1 the two keys (low, high), phase 2 the two (max, sum) pairs; then the counts
  unsigned v[6] = {__float_as_uint(a), __float_as_uint(a2), __float_as_uint(b), __float_as_uint(b2), (unsigned)c1, (unsigned)c2};
  if constexpr (PHASE == 1) { v[0] = (unsigned)ka; v[1] = (unsigned)(ka >> 32); v[2] = (unsigned)kb; v[3] = (unsigned)(kb >> 32); }
  if (lane < 32) {
#pragma unroll
    for (int k = 0; k < 6; ++k) red[wave][k][lane] = v[k];
  }
  __syncthreads();
  if (tid < 32) {
    for (int w = 1; w < 4; ++w) {   // wave order: fixed
      if constexpr (PHASE == 1) {
        ka = pmn_umax(ka, pmn_u64(red[w][0][tid], red[w][1][tid]));
        kb = pmn_umax(kb, pmn_u64(red[w][2][tid], red[w][3][tid]));
        c2 += (int)red[w][5][tid];
      } else {
        pl_merge(a, a2, __uint_as_float(red[w][0][tid]), __uint_as_float(red[w][1][tid]));
        pl_merge(b, b2, __uint_as_float(red[w][2][tid]), __uint_as_float(red[w][3][tid]));
      }
      c1 += (int)red[w][4][tid];
    }
    if (i < B) {
      if (S == 1) {
        unsigned* st = stats + (size_t)i * PMN_STAT;
        float l = 0.f;
        if constexpr (PHASE == 1) pmn_finish1<KIND>(ka, kb, c1, c2, p, st, l);
        else pmn_finish2(a, a2, b, b2, c1, vi, p, st, l);
        if constexpr (ENDS) pmn_st(reinterpret_cast<unsigned*>(ell) + i, __float_as_uint(l));
      } else {
        unsigned* w = ws + ((size_t)sp * B + i) * PMN_STAT;
        unsigned o[6] = {__float_as_uint(a), __float_as_uint(a2), __float_as_uint(b), __float_as_uint(b2), (unsigned)c1, (unsigned)c2};
        if constexpr (PHASE == 1) { o[0] = (unsigned)ka; o[1] = (unsigned)(ka >> 32); o[2] = (unsigned)kb; o[3] = (unsigned)(kb >> 32); }
#pragma unroll
        for (int k = 0; k < 6; ++k) pmn_st(w + k, o[k]);
      }
    }
    __threadfence();   // release: this workgroup's rows before its ticket
    if (tid == 0) is_last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
  }
  __syncthreads();
  if (!is_last) return;
  __threadfence();     // acquire: every workgroup's rows
  // S > 1: merge the S partial states of every anchor and finish it.  Then loss = sum over the valid anchors / A: strided partial sums,
  // lane tree, wave order; the same order whichever workgroup is last
  float sum = 0.f, cnt = 0.f;
  for (int r = tid; r < B; r += 256) {
    unsigned* st = stats + (size_t)r * PMN_STAT;
    float l = 0.f;
    bool valid;
    if (S == 1) {
      valid = pmn_ld(st + 7) != 0u;
      if constexpr (ENDS) l = __uint_as_float(pmn_ld(reinterpret_cast<unsigned*>(ell) + r));
    } else {
      float ma = -INFINITY, mb = -INFINITY, ma2 = 0.f, mb2 = 0.f;
      unsigned long long ja = 0ull, jb = 0ull;
      int n1 = 0, n2 = 0;
      for (int s = 0; s < S; ++s) {   // split order: fixed
        const unsigned* w = ws + ((size_t)s * B + r) * PMN_STAT;
        if constexpr (PHASE == 1) {
          ja = pmn_umax(ja, pmn_u64(pmn_ld(w + 0), pmn_ld(w + 1)));
          jb = pmn_umax(jb, pmn_u64(pmn_ld(w + 2), pmn_ld(w + 3)));
          n2 += (int)pmn_ld(w + 5);
        } else {
          pl_merge(ma, ma2, __uint_as_float(pmn_ld(w + 0)), __uint_as_float(pmn_ld(w + 1)));
          pl_merge(mb, mb2, __uint_as_float(pmn_ld(w + 2)), __uint_as_float(pmn_ld(w + 3)));
        }
        n1 += (int)pmn_ld(w + 4);
      }
      if constexpr (PHASE == 1) {
        valid = pmn_finish1<KIND>(ja, jb, n1, n2, p, st, l);
      } else {
        valid = st[7] != 0u;        // (the previous launch wrote it)
        pmn_finish2(ma, ma2, mb, mb2, n1, valid, p, st, l);
      }
      if constexpr (ENDS) ell[r] = l;
    }
    if (valid) { sum += l; cnt += 1.f; }
  }
  if constexpr (ENDS) {
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
    }
  }
  if (tid == 0) __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch on this stream
}

template <typename T> struct PmnFrag;   // G of one tile as MFMA "A" fragments: NQ 16-byte pieces per lane
template <> struct PmnFrag<bf16_t> { static constexpr int NQ = 2; };
template <> struct PmnFrag<float> { static constexpr int NQ = 4; };

// multi_similarity backward: pair_mem_bwd_kernel of pfr_pairmem.hip with pmn_weight (the four waves score four different tiles, G goes
// through LDS as lane-resident "A" fragments, every wave multiplies every G tile with êᵀ or memT for its slice of D)
template <typename T, int TD>
__global__ __launch_bounds__(256) void pair_mined_ms_bwd_kernel(const char* __restrict__ xn, const T* __restrict__ xnT, int ldt, const int64_t* __restrict__ label,
                                                                int B, int D, const char* __restrict__ mem, const T* __restrict__ memT, int ldm,
                                                                const int64_t* __restrict__ mem_label, int count, PmnParams p,
                                                                const float* __restrict__ stats, const float* __restrict__ out, float grad_scale,
                                                                const float* __restrict__ grad_scale_dev, int S, int order, float* __restrict__ dst) {
  constexpr int NQ = PmnFrag<T>::NQ;
  __shared__ u32x4 gl[2][4][NQ][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row = lane & 31, half = lane >> 5;
  const int nb = (B + 31) >> 5, nm = (count + 31) >> 5, nt = nb + nm;
  int blk, sp;
  pmn_block(order, nb, blk, sp);
  const int t_lo = (int)((long long)sp * nt / S), t_hi = (int)((long long)(sp + 1) * nt / S);
  const int r0 = blk * 32;
  const int rowbytes = D * (int)sizeof(T);
  const int i = r0 + row;
  const int64_t yi = label[min(i, B - 1)];
  const f32x4* st4 = reinterpret_cast<const f32x4*>(stats);
  const f32x4 lo_i = st4[2 * (size_t)min(i, B - 1)], hi_i = st4[2 * (size_t)min(i, B - 1) + 1];
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
      pmn_scores<T>(xn, B, part, prows, rowbytes, r0, j0, lane, g);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int j = j0 + acc_row(q, lane);
        const int jc = min(j, prows - 1);
        const float s = g[q];
        const bool in = i < B && j < prows && !(isb && j == i) && s == s;
        const bool same = plab[jc] == yi;
        float w = pmn_weight(lo_i, hi_i, s, same, p);
        if (isb) w += pmn_weight(st4[2 * (size_t)jc], st4[2 * (size_t)jc + 1], s, same, p);   // W_jr: batch partners are anchors too
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
__global__ __launch_bounds__(256) void pair_mined_reduce_kernel(const float* __restrict__ ws, size_t n, int S, float* __restrict__ dxn) {
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

__device__ __forceinline__ float pmn_elem(const float* p) { return *p; }
__device__ __forceinline__ float pmn_elem(const uint16_t* p) { return __uint_as_float((uint32_t)*p << 16); }

// the weight f_i scale of anchor i and its two partners, only when the row is usable: valid and both partner numbers in [0, B + count)
__device__ __forceinline__ bool pmn_bh_row(const float* stats, int i, int n, float scale, int& ip, int& in, float& w) {
  const float* s = stats + (size_t)i * PMN_STAT;
  ip = __float_as_int(s[2]);
  in = __float_as_int(s[3]);
  w = s[5] * scale;
  return s[7] != 0.f && ip >= 0 && ip < n && in >= 0 && in < n;
}

// batch_hard backward, one workgroup per row r of dê (E = the element as stored: float, or the 16 bits of a bf16):
//   dê_r = (f_r / A) (p[n*_r] - p[p*_r])  +  sum over the anchors i in index order of  +(f_i / A) ê_i where n*_i = r,  -(f_i / A) ê_i where p*_i = r
// fp32 weights, fp32 sums, plain stores, every element of the row written
template <typename E>
__global__ __launch_bounds__(256) void pair_mined_bh_bwd_kernel(const E* __restrict__ xn, int B, int D, const E* __restrict__ mem, int count,
                                                                const float* __restrict__ stats, const float* __restrict__ out, float grad_scale,
                                                                const float* __restrict__ grad_scale_dev, float* __restrict__ dxn) {
  __shared__ float wl[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int n = B + count;
  const float scale = grad_scale * (grad_scale_dev ? grad_scale_dev[0] : 1.f) * out[1];
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int ip, in;
  float w;
  if (pmn_bh_row(stats, r, n, scale, ip, in, w)) {
    const E* pp = ip < B ? xn + (size_t)ip * D : mem + (size_t)(ip - B) * D;
    const E* pq = in < B ? xn + (size_t)in * D : mem + (size_t)(in - B) * D;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int d = tid + 256 * k;
      if (d < D) acc[k] = w * (pmn_elem(pq + d) - pmn_elem(pp + d));
    }
  }
  for (int i0 = 0; i0 < B; i0 += 256) {
    float wi = 0.f;
    if (i0 + tid < B && pmn_bh_row(stats, i0 + tid, n, scale, ip, in, w)) wi = in == r ? w : (ip == r ? -w : 0.f);
    __syncthreads();
    wl[tid] = wi;
    __syncthreads();
    const int m = min(256, B - i0);
    for (int k = 0; k < m; ++k) {   // index order: fixed
      const float wk = wl[k];
      if (wk == 0.f) continue;
      const E* e = xn + (size_t)(i0 + k) * D;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int d = tid + 256 * c;
        if (d < D) acc[c] += wk * pmn_elem(e + d);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = tid + 256 * k;
    if (d < D) dxn[(size_t)r * D + d] = acc[k];
  }
}

static int pmn_check(const char* who, const void* xn, int dtype, const void* label, int B, int D, const void* mem, const void* mem_label, int M,
                     int count, int kind, const float* params, int splits) {
  PFR_CHECK_ARG(xn && label && params, "%s: null pointer", who);
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: the compute dtype is fp32 or bf16 (int8 is not supported)", who);
  PFR_CHECK_ARG(B >= 1 && B < (1 << 24), "%s: need 1 <= B < 2^24, got %d", who, B);
  PFR_CHECK_ARG(D >= 8 && D % 8 == 0 && D <= 1024, "%s: D must be a multiple of 8 in [8, 1024], got %d", who, D);
  PFR_CHECK_ARG(kind == PMN_BATCH_HARD || kind == PMN_MS, "%s: kind must be 2 (batch_hard) or 3 (multi_similarity), got %d", who, kind);
  if (kind == PMN_BATCH_HARD)
    PFR_CHECK_ARG(params[0] >= 0.f && params[1] >= 0.f, "%s: batch_hard needs a margin >= 0 and gamma >= 0, got m=%g gamma=%g", who, (double)params[0], (double)params[1]);
  else
    PFR_CHECK_ARG(params[0] > 0.f && params[1] > 0.f && params[3] >= 0.f && params[2] == params[2],
                  "%s: multi_similarity needs alpha > 0, beta > 0 and epsilon >= 0, got alpha=%g beta=%g base=%g epsilon=%g", who,
                  (double)params[0], (double)params[1], (double)params[2], (double)params[3]);
  if (!mem) {
    PFR_CHECK_ARG(M == 0 && count == 0, "%s: without a ring (mem = NULL) M and count are 0, got M=%d count=%d", who, M, count);
  } else {
    PFR_CHECK_ARG(mem_label, "%s: null pointer", who);
    PFR_CHECK_ARG(M >= 32 && M % 32 == 0 && M < (1 << 24), "%s: the ring needs M = a multiple of 32 with 32 <= M < 2^24, got %d", who, M);
    PFR_CHECK_ARG(count >= 0 && count <= M, "%s: need 0 <= count <= M, got count=%d M=%d", who, count, M);
  }
  PFR_CHECK_ARG(splits >= 0 && splits <= PMN_MAX_SPLITS, "%s: splits must be 0 (auto) or in [1, %d], got %d", who, PMN_MAX_SPLITS, splits);
  return PFR_OK;
}

extern "C" int pfr_pair_mem_splits(int B, int count, int D);   // pfr_pairmem.hip: the same partner list, the same workspaces
extern "C" int pfr_pair_mined_splits(int B, int count, int D) { return pfr_pair_mem_splits(B, count, D); }

extern "C" int pfr_pair_mined_fwd(const void* xn, int dtype, const int64_t* label, int B, int D, const void* mem, const int64_t* mem_label, int M,
                                  int count, int kind, const float* params, int splits, float* ws, float* stats, float* ell, float* out,
                                  int* counter, hipStream_t st) {
  const int rc = pmn_check("pfr_pair_mined_fwd", xn, dtype, label, B, D, mem, mem_label, M, count, kind, params, splits);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(stats && ell && out && counter, "pfr_pair_mined_fwd: null pointer");
  const int S = splits ? splits : pfr_pair_mined_splits(B, count, D);
  PFR_CHECK_ARG(S == 1 || ws, "pfr_pair_mined_fwd: workspace required (splits=%d)", S);
  const int nb = (B + 31) / 32;
  PFR_CHECK_ARG((long long)nb * S < (1ll << 31), "pfr_pair_mined_fwd: too many workgroups (%d anchor blocks x %d splits)", nb, S);
  const dim3 grid(nb * S), block(256);
  const PmnParams p{params[0], params[1], params[2], params[3]};
  const int order = pfr_knob(KNOB_PAIR_MEM_ORDER) ? 1 : 0;
#define PMNF(T, K, PH) hipLaunchKernelGGL((pair_mined_fwd_kernel<T, K, PH>), grid, block, 0, st, (const char*)xn, label, B, D, (const char*)mem, mem_label, count, p, S, order, (unsigned*)ws, (unsigned*)stats, ell, out, counter)
  if (kind == PMN_BATCH_HARD) {
    if (dtype == PFR_BF16) PMNF(bf16_t, PMN_BATCH_HARD, 1); else PMNF(float, PMN_BATCH_HARD, 1);
    PFR_CHECK_LAUNCH();
  } else {
    if (dtype == PFR_BF16) PMNF(bf16_t, PMN_MS, 1); else PMNF(float, PMN_MS, 1);
    PFR_CHECK_LAUNCH();
    if (dtype == PFR_BF16) PMNF(bf16_t, PMN_MS, 2); else PMNF(float, PMN_MS, 2);
    PFR_CHECK_LAUNCH();
  }
#undef PMNF
  return PFR_OK;
}

extern "C" int pfr_pair_mined_bwd(const void* xn, const void* xnT, int dtype, int ldt, const int64_t* label, int B, int D, const void* mem,
                                  const void* memT, int ldm, const int64_t* mem_label, int M, int count, int kind, const float* params,
                                  const float* stats, const float* out, float grad_scale, const float* grad_scale_dev, int splits, float* ws,
                                  float* dxn, hipStream_t st) {
  const int rc = pmn_check("pfr_pair_mined_bwd", xn, dtype, label, B, D, mem, mem_label, M, count, kind, params, splits);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(stats && out && dxn, "pfr_pair_mined_bwd: null pointer");
  if (kind == PMN_BATCH_HARD) {   // sparse: neither the transposed copies nor a workspace
    if (dtype == PFR_BF16)
      hipLaunchKernelGGL(pair_mined_bh_bwd_kernel<uint16_t>, dim3(B), dim3(256), 0, st, (const uint16_t*)xn, B, D, (const uint16_t*)mem, count, stats, out, grad_scale, grad_scale_dev, dxn);
    else
      hipLaunchKernelGGL(pair_mined_bh_bwd_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)xn, B, D, (const float*)mem, count, stats, out, grad_scale, grad_scale_dev, dxn);
    PFR_CHECK_LAUNCH();
    return PFR_OK;
  }
  PFR_CHECK_ARG(xnT && (memT || !mem), "pfr_pair_mined_bwd: null pointer");
  PFR_CHECK_ARG(ldt >= (B + 31) / 32 * 32 && ldt % 32 == 0, "pfr_pair_mined_bwd: the transposed copy needs ldt = a multiple of 32 >= B (zero pad columns), got %d", ldt);
  PFR_CHECK_ARG(!mem || (ldm >= M && ldm % 32 == 0), "pfr_pair_mined_bwd: the transposed ring needs ldm = a multiple of 32 >= M (zero beyond count), got %d", ldm);
  const int S = splits ? splits : pfr_pair_mined_splits(B, count, D);
  PFR_CHECK_ARG(S == 1 || ws, "pfr_pair_mined_bwd: workspace required (splits=%d)", S);
  const int nb = (B + 31) / 32;
  PFR_CHECK_ARG((long long)nb * S < (1ll << 31), "pfr_pair_mined_bwd: too many workgroups (%d anchor blocks x %d splits)", nb, S);
  const dim3 grid(nb * S), block(256);
  const PmnParams p{params[0], params[1], params[2], params[3]};
  const int order = pfr_knob(KNOB_PAIR_MEM_ORDER) ? 1 : 0;
  float* dst = S == 1 ? dxn : ws;
#define PMNB(T, TD) hipLaunchKernelGGL((pair_mined_ms_bwd_kernel<T, TD>), grid, block, 0, st, (const char*)xn, (const T*)xnT, ldt, label, B, D, (const char*)mem, (const T*)memT, ldm, mem_label, count, p, stats, out, grad_scale, grad_scale_dev, S, order, dst)
  if (dtype == PFR_BF16) { if (D <= 512) PMNB(bf16_t, 4); else PMNB(bf16_t, 8); }
  else { if (D <= 512) PMNB(float, 4); else PMNB(float, 8); }
#undef PMNB
  PFR_CHECK_LAUNCH();
  if (S > 1) {
    const size_t n = (size_t)B * D;
    hipLaunchKernelGGL(pair_mined_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, (const float*)ws, n, S, dxn);
    PFR_CHECK_LAUNCH();
  }
  return PFR_OK;
}
