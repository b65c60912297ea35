// pfr_rerank.hip — k-reciprocal re-ranking (Zhong et al., CVPR 2017) of match lists on SPARSE rows: nothing N x N is ever built.
// The contract (sets, weights, local query expansion, Jaccard blend, tie rules) is the comment block at pfr_rerank_* in include/pfr_hip.h.
//
// Three kernels, each ONE 256-thread workgroup per row, every list and set in LDS (32-bit and aligned 64-bit accesses only):
//   rerank_expand_kernel   R(i, k1) by probing the K1-entry rows of the neighbours, the accepted R(j, kh), a bitonic sort that makes the union
//                          sorted and duplicate free, then one wave per member for the fp32 dot product and the Gaussian weight
//   rerank_average_kernel  the k2' member rows concatenated, sorted by (index, source) and summed run by run
//   rerank_score_kernel    row i sorted in LDS; the four waves take candidates in turn, lanes stride over the candidate's row and binary-search
//                          row i; a bitonic sort of (distance key, position) pairs gives the k smallest with ties by position
// Determinism: every sum runs in a fixed order (per-lane strides in ascending position, then the xor butterfly of wave_sum, which gives every
// lane the same bits); there are no atomics.  Every index read from nbr / rows / cand is range-checked before it is used as an address.
#include "pfr_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_MAX_LIST = 512;                 // K1 = k1 + 1 and kc: the limit of the running top-K lists that produce them
constexpr size_t RR_MAX_LDS = 160 * 1024;        // gfx950: 160 KiB per CU

__host__ __device__ inline int rr_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
static inline size_t rr_align16(size_t b) { return (b + 15) & ~(size_t)15; }

// Python's round(k1 / 2): half to even
static inline int rr_kh(int k1) {
  const int m = k1 / 2;
  return (k1 & 1) ? (m & 1 ? m + 1 : m) : m;
}

// ascending in-place sort of P (a power of two) keys in LDS; the caller has synchronised after filling them
template <typename T> __device__ void rr_bitonic(T* a, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < P; t += RR_THREADS) {
        const int u = t ^ j;
        if (u > t) {
          const T x = a[t], y = a[u];
          if ((x > y) == ((t & k) == 0)) { a[t] = y; a[u] = x; }
        }
      }
      __syncthreads();
    }
}

// Ordered compaction over positions [0, n): val(p) >= 0 is kept and handed to out(rank, value) with rank = kept positions before p.
// out must not write what val reads.  scr: 4 ints of LDS.  Returns the number kept (to every thread); ends with a barrier.
template <typename V, typename O> __device__ int rr_compact(int n, int* scr, V val, O out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int base = 0;
  for (int p0 = 0; p0 < n; p0 += RR_THREADS) {
    const int p = p0 + threadIdx.x;
    const int v = p < n ? val(p) : -1;
    const unsigned long long m = __ballot(v >= 0);
    if (lane == 0) scr[w] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int q = 0; q < w; ++q) off += scr[q];
    if (v >= 0) out(off + __popcll(m & ((1ull << lane) - 1ull)), v);
    base += scr[0] + scr[1] + scr[2] + scr[3];
    __syncthreads();
  }
  return base;
}

// ---------------------------------------------------------------------------------------------------------------- steps 1 + 2
struct ExpandParams {
  const float* emb;
  const int* nbr;
  int N, D, K1, kh1, E, P, cap;
  int* v_idx;
  float* v_val;
  int* v_cnt;
};
static size_t expand_lds(int K1, int kh1, int E) {
  // Li, R0, acc [K1] | mem, memI [K1 * kh1] | keys [P] | uniq [E] | wv [E] | scratch [8]
  return rr_align16(sizeof(int) * ((size_t)3 * K1 + (size_t)2 * K1 * kh1 + rr_pow2(E) + (size_t)2 * E + 8));
}

__global__ __launch_bounds__(RR_THREADS) void rerank_expand_kernel(ExpandParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int K1 = p.K1, kh1 = p.kh1, N = p.N;
  int* Li = reinterpret_cast<int*>(smem);
  int* R0 = Li + K1;
  int* acc = R0 + K1;
  int* mem = acc + K1;
  int* memI = mem + K1 * kh1;
  uint32_t* keys = reinterpret_cast<uint32_t*>(memI + K1 * kh1);
  int* uniq = reinterpret_cast<int*>(keys + p.P);
  float* wv = reinterpret_cast<float*>(uniq + p.E);
  int* scr = reinterpret_cast<int*>(wv + p.E);
  const int i = blockIdx.x, tid = threadIdx.x;
  const int* nbr = p.nbr;
  const int* nb_i = nbr + (size_t)i * K1;

  // L_k1(i): the valid entries of row i, in order
  const int ni = rr_compact(K1, scr, [&](int t) { const int e = nb_i[t]; return (unsigned)e < (unsigned)N ? e : -1; },
                            [&](int rk, int v) { Li[rk] = v; });
  // R(i, k1) = { j in L_k1(i) : i in L_k1(j) }  (L_k1(j) is every valid entry of row j; i itself is valid)
  for (int a = tid; a < ni; a += RR_THREADS) acc[a] = 0;
  __syncthreads();
  for (int q = tid; q < ni * K1; q += RR_THREADS) {
    const int a = q / K1, t = q - a * K1;
    if (nbr[(size_t)Li[a] * K1 + t] == i) acc[a] = 1;      // (several threads may store the same 1)
  }
  __syncthreads();
  const int nr = rr_compact(ni, scr, [&](int a) { return acc[a] ? Li[a] : -1; }, [&](int rk, int v) { R0[rk] = v; });

  // R(j, kh) for every j in R(i, k1): slot (a, b) holds the b-th valid entry c of row j when j is among the first kh + 1 valid entries of row c
  for (int q = tid; q < nr * kh1; q += RR_THREADS) {
    const int a = q / kh1, b = q - a * kh1, j = R0[a];
    const int* nb_j = nbr + (size_t)j * K1;
    int c = -1, cnt = 0;
    for (int t = 0; t < K1; ++t) {
      const int e = nb_j[t];
      if ((unsigned)e < (unsigned)N) {
        if (cnt == b) { c = e; break; }
        ++cnt;
      }
    }
    bool rec = false;
    if (c >= 0) {
      const int* nb_c = nbr + (size_t)c * K1;
      cnt = 0;
      for (int t = 0; t < K1; ++t) {
        const int e = nb_c[t];
        if ((unsigned)e < (unsigned)N) {
          if (e == j) { rec = true; break; }
          if (++cnt == kh1) break;
        }
      }
    }
    int inr = 0;
    if (rec)
      for (int s = 0; s < nr; ++s)
        if (R0[s] == c) { inr = 1; break; }
    mem[q] = rec ? c : -1;
    memI[q] = inr;
  }
  __syncthreads();
  // accepted when 3 |R(j, kh) ∩ R(i, k1)| > 2 |R(j, kh)|
  for (int a = tid; a < nr; a += RR_THREADS) {
    int size = 0, inter = 0;
    for (int b = 0; b < kh1; ++b) {
      size += mem[a * kh1 + b] >= 0;
      inter += memI[a * kh1 + b];
    }
    acc[a] = 3 * inter > 2 * size;
  }
  __syncthreads();
  // the union, sorted and duplicate free
  for (int s = tid; s < p.P; s += RR_THREADS) {
    uint32_t v = 0xffffffffu;
    if (s < K1) {
      if (s < nr) v = (uint32_t)R0[s];
    } else if (s < p.E) {
      const int q = s - K1, a = q / kh1;
      if (a < nr && acc[a] && mem[q] >= 0) v = (uint32_t)mem[q];
    }
    keys[s] = v;
  }
  __syncthreads();
  rr_bitonic(keys, p.P);
  const int n = rr_compact(p.P, scr,
                           [&](int s) { const uint32_t k = keys[s]; return (k != 0xffffffffu && (s == 0 || keys[s - 1] != k)) ? (int)k : -1; },
                           [&](int rk, int v) { uniq[rk] = v; });

  // weights: one wave per member, lanes stride over D, then the butterfly; exp(-(2 - 2 dot))
  const int lane = tid & 63, w = tid >> 6;
  const float* ei = p.emb + (size_t)i * p.D;
  for (int s = w; s < n; s += RR_THREADS / 64) {
    const float* ej = p.emb + (size_t)uniq[s] * p.D;
    float part = 0.f;
    for (int d = lane; d < p.D; d += 64) part = fmaf(ei[d], ej[d], part);
    const float dot = wave_sum(part);
    if (lane == 0) wv[s] = expf(-(2.f - 2.f * dot));
  }
  __syncthreads();
  float* tot = reinterpret_cast<float*>(scr + 4);
  if (w == 0) {
    float part = 0.f;
    for (int s = lane; s < n; s += 64) part += wv[s];
    part = wave_sum(part);
    if (lane == 0) *tot = part;
  }
  __syncthreads();
  const float total = *tot;
  int* oi = p.v_idx + (size_t)i * p.cap;
  float* ov = p.v_val + (size_t)i * p.cap;
  for (int s = tid; s < p.cap; s += RR_THREADS) {
    oi[s] = s < n ? uniq[s] : -1;
    ov[s] = s < n ? wv[s] / total : 0.f;
  }
  if (tid == 0) p.v_cnt[i] = n;
}

// ---------------------------------------------------------------------------------------------------------------- step 3
struct AverageParams {
  const int* nbr;
  int N, K1, k2, E, cap, E2, cap2, P2;
  const int* v_idx;
  const float* v_val;
  const int* v_cnt;
  int* q_idx;
  float* q_val;
  int* q_cnt;
};
static size_t average_lds(int k2, int E2) {
  // keys u64 [P2] | vals [E2] | oidx [E2] | oval [E2] | src [k2] | off [k2 + 1] | scratch [8]
  return rr_align16((size_t)8 * rr_pow2(E2) + sizeof(int) * ((size_t)3 * E2 + (size_t)2 * k2 + 1 + 8));
}

__global__ __launch_bounds__(RR_THREADS) void rerank_average_kernel(AverageParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  float* vals = reinterpret_cast<float*>(keys + p.P2);
  int* oidx = reinterpret_cast<int*>(vals + p.E2);
  float* oval = reinterpret_cast<float*>(oidx + p.E2);
  int* src = reinterpret_cast<int*>(oval + p.E2);
  int* off = src + p.k2;
  int* scr = off + p.k2 + 1;
  const int i = blockIdx.x, tid = threadIdx.x;
  // the first k2 valid entries of row i (self first) and where their rows start in the concatenation
  if (tid == 0) {
    const int* nb_i = p.nbr + (size_t)i * p.K1;
    int cnt = 0;
    off[0] = 0;
    for (int t = 0; t < p.K1 && cnt < p.k2; ++t) {
      const int e = nb_i[t];
      if ((unsigned)e < (unsigned)p.N) {
        src[cnt] = e;
        off[cnt + 1] = off[cnt] + min(max(p.v_cnt[e], 0), p.E);
        ++cnt;
      }
    }
    scr[4] = cnt;
  }
  __syncthreads();
  const int k2p = scr[4];
  const int total = off[k2p];
  // key = (index, position in the concatenation): equal indices stay in source order
  for (int s = tid; s < p.P2; s += RR_THREADS) {
    unsigned long long key = ~0ull;
    if (s < total) {
      int m = 0;
      while (off[m + 1] <= s) ++m;
      const size_t at = (size_t)src[m] * p.cap + (s - off[m]);
      vals[s] = p.v_val[at];
      key = ((unsigned long long)(uint32_t)p.v_idx[at] << 32) | (uint32_t)s;
    }
    keys[s] = key;
  }
  __syncthreads();
  rr_bitonic(keys, p.P2);
  const float denom = (float)(k2p > 0 ? k2p : 1);
  const int n = rr_compact(total, scr,
                           [&](int s) { return (s == 0 || (uint32_t)(keys[s - 1] >> 32) != (uint32_t)(keys[s] >> 32)) ? s : -1; },
                           [&](int rk, int s) {
                             const uint32_t id = (uint32_t)(keys[s] >> 32);
                             float a = 0.f;
                             for (int u = s; u < total && (uint32_t)(keys[u] >> 32) == id; ++u) a += vals[(uint32_t)keys[u]];
                             oidx[rk] = (int)id;
                             oval[rk] = a / denom;
                           });
  int* oi = p.q_idx + (size_t)i * p.cap2;
  float* ov = p.q_val + (size_t)i * p.cap2;
  for (int s = tid; s < p.cap2; s += RR_THREADS) {
    oi[s] = s < n ? oidx[s] : -1;
    ov[s] = s < n ? oval[s] : 0.f;
  }
  if (tid == 0) p.q_cnt[i] = n;
}

// ---------------------------------------------------------------------------------------------------------------- step 4
struct ScoreParams {
  const int* q_idx;
  const float* q_val;
  const int* q_cnt;
  int N, cap2, R, kc, k, P;
  const int* rows;
  const int* cand;
  const float* cand_cos;
  float lambda;
  float* dist;
  int* idx;
};
static size_t score_lds(int kc, int cap2) {
  // keys u64 [P] | ri [cap2] | rv [cap2]
  return rr_align16((size_t)8 * rr_pow2(kc) + sizeof(int) * (size_t)2 * cap2);
}

__global__ __launch_bounds__(RR_THREADS) void rerank_score_kernel(ScoreParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
  int* ri = reinterpret_cast<int*>(keys + p.P);
  float* rv = reinterpret_cast<float*>(ri + p.cap2);
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = p.rows[r];
  const bool row_ok = (unsigned)i < (unsigned)p.N;
  const int ni = row_ok ? min(max(p.q_cnt[i], 0), p.cap2) : 0;
  for (int s = tid; s < ni; s += RR_THREADS) {
    ri[s] = p.q_idx[(size_t)i * p.cap2 + s];
    rv[s] = p.q_val[(size_t)i * p.cap2 + s];
  }
  __syncthreads();
  const int* cand = p.cand + (size_t)r * p.kc;
  for (int t = w; t < p.P; t += RR_THREADS / 64) {      // (t is uniform in the wave)
    unsigned long long key = ~0ull;
    const int c = t < p.kc ? cand[t] : -1;
    if (row_ok && (unsigned)c < (unsigned)p.N) {
      const int nc = min(max(p.q_cnt[c], 0), p.cap2);
      const int* ci = p.q_idx + (size_t)c * p.cap2;
      const float* cv = p.q_val + (size_t)c * p.cap2;
      float part = 0.f;
      for (int s = lane; s < nc; s += 64) {
        const int id = ci[s];
        int lo = 0, hi = ni;                                // first position with ri >= id
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (ri[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo < ni && ri[lo] == id) part += fminf(rv[lo], cv[s]);
      }
      const float m = wave_sum(part);
      const float dj = 1.f - m / (2.f - m);
      const float fin = (1.f - p.lambda) * dj + p.lambda * (2.f - 2.f * p.cand_cos[(size_t)r * p.kc + t]);
      key = ((unsigned long long)fkey(fin) << 32) | (uint32_t)t;
    }
    if (lane == 0) keys[t] = key;
  }
  __syncthreads();
  rr_bitonic(keys, p.P);
  for (int t = tid; t < p.k; t += RR_THREADS) {
    const unsigned long long key = keys[t];
    const bool ok = (uint32_t)key != 0xffffffffu;
    p.dist[(size_t)r * p.k + t] = ok ? fkey_inv((uint32_t)(key >> 32)) : INFINITY;
    p.idx[(size_t)r * p.k + t] = ok ? cand[(uint32_t)key] : -1;
  }
}

static std::atomic<unsigned long long> g_lds_done{0};

static int rr_capacity(const char* who, int k1, int k2, int* E, int* E2) {
  PFR_CHECK_ARG(k1 >= 1, "%s: k1=%d must be >= 1", who, k1);
  PFR_CHECK_ARG(k1 + 1 <= RR_MAX_LIST, "%s: k1 + 1 = %d exceeds the %d-entry neighbour lists", who, k1 + 1, RR_MAX_LIST);
  PFR_CHECK_ARG(k2 >= 1, "%s: k2=%d must be >= 1", who, k2);
  const long long e = (long long)(k1 + 1) + (long long)(k1 + 1) * (rr_kh(k1) + 1);
  const long long e2 = e * k2;
  PFR_CHECK_ARG(e2 <= INT_MAX / 8, "%s: row capacity k2 * E = %lld is out of range", who, e2);
  *E = (int)e;
  *E2 = (int)e2;
  return PFR_OK;
}

}  // namespace

extern "C" int pfr_rerank_row_capacity(int k1, int k2, int* E, int* E2) {
  PFR_CHECK_ARG(E && E2, "pfr_rerank_row_capacity: null pointer");
  return rr_capacity("pfr_rerank_row_capacity", k1, k2, E, E2);
}

extern "C" int pfr_rerank_expand(const float* emb32, int N, int D, const int* nbr, int k1, int* v_idx, float* v_val, int* v_cnt, int cap,
                                 hipStream_t stream) {
  int E, E2;
  const int rc = rr_capacity("pfr_rerank_expand", k1, 1, &E, &E2);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(N >= 0 && D >= 1, "pfr_rerank_expand: bad shape N=%d D=%d", N, D);
  PFR_CHECK_ARG(cap >= E, "pfr_rerank_expand: rows of %d entries are smaller than the capacity E=%d of k1=%d", cap, E, k1);
  PFR_CHECK_ARG(emb32 && nbr && v_idx && v_val && v_cnt, "pfr_rerank_expand: null pointer");
  const int K1 = k1 + 1, kh1 = rr_kh(k1) + 1;
  const size_t lds = expand_lds(K1, kh1, E);
  if (lds > RR_MAX_LDS) {
    pfr_set_error("pfr_rerank_expand: k1=%d needs %zu bytes of LDS per row (E=%d), the limit is %zu", k1, lds, E, RR_MAX_LDS);
    return PFR_ERR_UNSUPPORTED;
  }
  PFR_CHECK_ARG(pfr_all_dev({emb32, nbr, v_idx, v_val, v_cnt}), "pfr_rerank_expand: every pointer must be device memory");
  if (N == 0) return PFR_OK;
  PFR_MAX_LDS_ONCE(g_lds_done, (int)RR_MAX_LDS, (const void*)rerank_expand_kernel, (const void*)rerank_average_kernel,
                   (const void*)rerank_score_kernel);
  ExpandParams p;
  p.emb = emb32; p.nbr = nbr; p.N = N; p.D = D; p.K1 = K1; p.kh1 = kh1; p.E = E; p.P = rr_pow2(E); p.cap = cap;
  p.v_idx = v_idx; p.v_val = v_val; p.v_cnt = v_cnt;
  hipLaunchKernelGGL(rerank_expand_kernel, dim3(N), dim3(RR_THREADS), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_rerank_average(const int* nbr, int N, int k1, int k2, const int* v_idx, const float* v_val, const int* v_cnt, int cap,
                                  int* q_idx, float* q_val, int* q_cnt, int cap2, hipStream_t stream) {
  int E, E2;
  const int rc = rr_capacity("pfr_rerank_average", k1, k2, &E, &E2);
  if (rc != PFR_OK) return rc;
  PFR_CHECK_ARG(N >= 0, "pfr_rerank_average: bad N=%d", N);
  PFR_CHECK_ARG(cap >= E, "pfr_rerank_average: input rows of %d entries are smaller than the capacity E=%d of k1=%d", cap, E, k1);
  PFR_CHECK_ARG(cap2 >= E2, "pfr_rerank_average: output rows of %d entries are smaller than the capacity E2=%d of k1=%d, k2=%d", cap2, E2, k1, k2);
  PFR_CHECK_ARG(nbr && v_idx && v_val && v_cnt && q_idx && q_val && q_cnt, "pfr_rerank_average: null pointer");
  const size_t lds = average_lds(k2, E2);
  if (lds > RR_MAX_LDS) {
    pfr_set_error("pfr_rerank_average: k1=%d, k2=%d need %zu bytes of LDS per row (E2=%d), the limit is %zu", k1, k2, lds, E2, RR_MAX_LDS);
    return PFR_ERR_UNSUPPORTED;
  }
  PFR_CHECK_ARG(pfr_all_dev({nbr, v_idx, v_val, v_cnt, q_idx, q_val, q_cnt}), "pfr_rerank_average: every pointer must be device memory");
  if (N == 0) return PFR_OK;
  PFR_MAX_LDS_ONCE(g_lds_done, (int)RR_MAX_LDS, (const void*)rerank_expand_kernel, (const void*)rerank_average_kernel,
                   (const void*)rerank_score_kernel);
  AverageParams p;
  p.nbr = nbr; p.N = N; p.K1 = k1 + 1; p.k2 = k2; p.E = E; p.cap = cap; p.E2 = E2; p.cap2 = cap2; p.P2 = rr_pow2(E2);
  p.v_idx = v_idx; p.v_val = v_val; p.v_cnt = v_cnt; p.q_idx = q_idx; p.q_val = q_val; p.q_cnt = q_cnt;
  hipLaunchKernelGGL(rerank_average_kernel, dim3(N), dim3(RR_THREADS), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_rerank_score(const int* q_idx, const float* q_val, const int* q_cnt, int N, int cap2, const int* rows, int R,
                                const int* cand, const float* cand_cos, int kc, float lambda, int k, float* dist, int* idx,
                                hipStream_t stream) {
  PFR_CHECK_ARG(N >= 0 && R >= 0 && cap2 >= 1, "pfr_rerank_score: bad shape N=%d R=%d cap2=%d", N, R, cap2);
  PFR_CHECK_ARG(kc >= 1 && kc <= RR_MAX_LIST, "pfr_rerank_score: kc=%d must be in 1..%d (the running lists)", kc, RR_MAX_LIST);
  PFR_CHECK_ARG(k >= 1 && k <= kc, "pfr_rerank_score: k=%d must be in 1..kc=%d", k, kc);
  PFR_CHECK_ARG(lambda >= 0.f && lambda <= 1.f, "pfr_rerank_score: lambda must be in [0, 1]");
  PFR_CHECK_ARG(q_idx && q_val && q_cnt && rows && cand && cand_cos && dist && idx, "pfr_rerank_score: null pointer");
  const size_t lds = score_lds(kc, cap2);
  if (lds > RR_MAX_LDS) {
    pfr_set_error("pfr_rerank_score: rows of %d entries need %zu bytes of LDS, the limit is %zu", cap2, lds, RR_MAX_LDS);
    return PFR_ERR_UNSUPPORTED;
  }
  PFR_CHECK_ARG(pfr_all_dev({q_idx, q_val, q_cnt, rows, cand, cand_cos, dist, idx}), "pfr_rerank_score: every pointer must be device memory");
  if (R == 0) return PFR_OK;
  PFR_MAX_LDS_ONCE(g_lds_done, (int)RR_MAX_LDS, (const void*)rerank_expand_kernel, (const void*)rerank_average_kernel,
                   (const void*)rerank_score_kernel);
  ScoreParams p;
  p.q_idx = q_idx; p.q_val = q_val; p.q_cnt = q_cnt; p.N = N; p.cap2 = cap2; p.R = R; p.kc = kc; p.k = k; p.P = rr_pow2(kc);
  p.rows = rows; p.cand = cand; p.cand_cos = cand_cos; p.lambda = lambda; p.dist = dist; p.idx = idx;
  hipLaunchKernelGGL(rerank_score_kernel, dim3(R), dim3(RR_THREADS), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
