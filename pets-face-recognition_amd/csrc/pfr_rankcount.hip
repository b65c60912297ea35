// pfr_rankcount.hip — exact retrieval ranks: the score GEMM of the match with a RANK-COUNTING epilogue (pfr_rank_count) and the gather
// of single scores by the same tile code (pfr_pair_scores_gather); contract in include/pfr_hip.h.  The rank of a positive is a count
// (how many items precede it), so nothing Na x Nb is written and nothing is sorted: every score is compared, where the MFMA left it,
// against the few thresholds of its row.
//
// Schedule (pfr_pairhist.hip's): persistent workgroups walk a queue of 128 x 128 tiles in super-tiles of 16 x 16 tiles; a tile is
// 256 threads = 2 x 2 waves of 64 x 64, 128-byte k-steps staged global -> registers -> swizzled LDS, the next k-step's loads in flight
// under the MFMAs.  Ranks are per row, so every (row, column) tile is visited: there is no triangle to skip.
//
// Count epilogue.  Staged per tile: the column ids, the rows' excluded id, threshold count and (int8) scales, the rows' thresholds
// (value, id) themselves, and tmin = the smallest non-NaN threshold value of each row.  An accumulator register holds 2 rows x 32
// columns of a wave; it enters the slow path only when some lane has s >= tmin[row] (one compare and one wave vote otherwise: a score
// below every threshold of its row precedes none of them, and a NaN score fails the compare as the contract wants).  The slow path
// walks the thresholds of the two rows: one wave vote per threshold, the population counts of its halves are added by ONE lane per row
// to the workgroup-private 32-bit LDS counter of (row, k) — not one atomic per lane, the 32 lanes of a row would hit one address.  A
// tile adds at most 128 to a counter; the counters are flushed after every tile with global integer atomic adds of the non-zero slots
// (thresholds and counters belong to the ROW tile and the tile order interleaves row tiles, so keeping them over tiles buys nothing).
//
// LDS budget: operands 2 x 16 KiB + 6 x 512 B of per-tile vectors = 35 840 B fixed, plus 128 rows x ld x 12 B (threshold value, id,
// counter).  RC_MAX_THR = 64 thresholds per row gives 134 144 B of the CU's 160 KiB (one workgroup per CU); ld <= 30 keeps two
// workgroups per CU, which is what the common case (a handful of positives per query) runs with.  The dynamic size follows ld.
//
// Gather: tile (row tile, k) multiplies the 128 rows of a with the 128 GATHERED rows b[col[row][k]] and keeps the diagonal.  Both
// kernels call rc_tile_gemm — same staging, same k-steps, same MFMA sequence — and rc_score; an accumulator element's value depends on
// its two operand rows and the k order only, not on where in a tile it sits, so the two entry points give the same bits.
#include "pfr_igemm.h"
#include "pfr_pairtile.h"

#define RC_MAX_THR 64       // thresholds per row of one launch
#define RC_FIXED_LDS (2 * RC_T * RC_ROWB + 6 * RC_T * 4)

struct RankCountParams {
  const char* a;
  const char* b;
  const float* a_scale;
  const float* b_scale;
  const int* b_id;
  const int* excl;          // or nullptr
  const float* thr_val;
  const int* thr_id;
  const int* thr_cnt;
  unsigned int* cnt;
  const int* col;           // gather
  float* out;               // gather
  int Na, Nb, ld;
  int rowb;                 // bytes per operand row
  int ntm, ntn, nsn;
  long long nsuper;
};


template <typename T>
__global__ __launch_bounds__(256) void rank_count_kernel(const RankCountParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsA = smem;                                  // [128][128 B]
  char* ldsB = smem + RC_T * RC_ROWB;                 // [128][128 B]
  int* idB = reinterpret_cast<int*>(smem + 2 * RC_T * RC_ROWB);
  int* exA = idB + RC_T;
  int* cntA = exA + RC_T;
  float* scA = reinterpret_cast<float*>(cntA + RC_T);
  float* scB = scA + RC_T;
  float* tmin = scB + RC_T;
  float* thrV = tmin + RC_T;                          // [128][ld]
  int* thrI = reinterpret_cast<int*>(thrV + RC_T * p.ld);
  unsigned int* c = reinterpret_cast<unsigned int*>(thrI + RC_T * p.ld);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int ld = p.ld, slots = RC_T * ld;
  for (int s = tid; s < slots; s += 256) c[s] = 0;
  // (the first tile's barriers order this against the first LDS atomic)

  const int lc = tid & 7, lr = tid >> 3;
  const int nk = p.rowb / RC_ROWB;
  const bool has_excl = p.excl != nullptr;
  const long long total = p.nsuper * (RC_SUPER * RC_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const long long su = t / (RC_SUPER * RC_SUPER);
    const int l = (int)(t % (RC_SUPER * RC_SUPER));
    const int sm = (int)(su / p.nsn), sn = (int)(su % p.nsn);
    const int tm = sm * RC_SUPER + l / RC_SUPER, tn = sn * RC_SUPER + l % RC_SUPER;
    if (tm >= p.ntm || tn >= p.ntn) continue;   // (block-uniform)
    const int row0 = tm * RC_T, col0 = tn * RC_T;

    // operand rows of a ragged last tile are clamped to the last valid row (their scores are masked below)
    const char* ga[4];
    const char* gb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ra = min(row0 + lr + 32 * u, p.Na - 1), rb = min(col0 + lr + 32 * u, p.Nb - 1);
      ga[u] = p.a + (size_t)ra * p.rowb + lc * 16;
      gb[u] = p.b + (size_t)rb * p.rowb + lc * 16;
    }
    f32x16 acc[2][2];
    rc_tile_gemm<T>(ga, gb, nk, ldsA, ldsB, tid, true, acc, [&] {
      if (tid < RC_T) {
        const int ra = min(row0 + tid, p.Na - 1), rb = min(col0 + tid, p.Nb - 1);
        idB[tid] = p.b_id[rb];
        exA[tid] = has_excl ? p.excl[ra] : 0;
        cntA[tid] = row0 + tid < p.Na ? min(max(p.thr_cnt[ra], 0), ld) : 0;   // a row past the end has no thresholds
        if constexpr (sizeof(T) == 1) { scA[tid] = p.a_scale[ra]; scB[tid] = p.b_scale[rb]; }
      }
      // the rows' thresholds: [128][ld] of the tile is one contiguous range of thr_val / thr_id, cut at the last valid row
      const int nvalid = min(RC_T, p.Na - row0) * ld;
      const size_t g0 = (size_t)row0 * ld;
      for (int s = tid; s < nvalid; s += 256) {
        thrV[s] = p.thr_val[g0 + s];
        thrI[s] = p.thr_id[g0 + s];
      }
    });
    // (the staged thresholds are behind the second barrier of the first k-step)
    if (tid < RC_T) {
      float m = __builtin_inff();               // no (non-NaN) threshold: only +inf scores look further, and find nothing to precede
      const int n = cntA[tid];
      for (int k = 0; k < n; ++k) m = fminf(m, thrV[tid * ld + k]);   // fminf drops a NaN threshold (nothing precedes it)
      tmin[tid] = m;
    }
    __syncthreads();

    // ---- rank-count epilogue
    const bool full = row0 + RC_T <= p.Na && col0 + RC_T <= p.Nb;   // no element of the tile is masked by the edges
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cl = wq * 64 + j * 32 + (lane & 31);
      const int idj = idB[cl];
      const bool colok = full || col0 + cl < p.Nb;
      float sb = 0.f;
      if constexpr (sizeof(T) == 1) sb = scB[cl];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wp * 64 + i * 32 + acc_row(r, lane);   // one row per half wave
          float sa = 0.f;
          if constexpr (sizeof(T) == 1) sa = scA[rl];
          const float s = rc_score<T>(acc[i][j][r], sa, sb);
          // (rows past Na have tmin = +inf and no thresholds)
          const bool in = colok && s >= tmin[rl] && !(has_excl && idj == exA[rl]);
          if (__ballot(in) == 0ull) continue;   // (wave-uniform)
          const int n = cntA[rl];
          const int nmax = max(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 32));
          for (int k = 0; k < nmax; ++k) {
            bool pre = false;
            if (in && k < n) {
              const float tv = thrV[rl * ld + k];
              pre = s > tv || (s == tv && idj < thrI[rl * ld + k]);
            }
            const unsigned long long m = __ballot(pre);
            const unsigned int add = __popc((unsigned int)(lane < 32 ? m : m >> 32));
            if ((lane & 31) == 0 && add) atomicAdd(c + rl * ld + k, add);
          }
        }
      }
    }
    // ---- flush the tile's counters (rows past Na were never counted)
    __syncthreads();
    for (int s = tid; s < slots; s += 256) {
      const unsigned int v = c[s];
      if (v) {
        atomicAdd(p.cnt + (size_t)row0 * ld + s, v);
        c[s] = 0;
      }
    }
    // (the next tile's first barrier orders the zeroing and these reads against its staging)
  }
}

template <typename T>
__global__ __launch_bounds__(256) void pair_gather_kernel(const RankCountParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsA = smem;
  char* ldsB = smem + RC_T * RC_ROWB;
  int* colS = reinterpret_cast<int*>(smem + 2 * RC_T * RC_ROWB);
  float* scA = reinterpret_cast<float*>(colS + RC_T);
  float* scB = scA + RC_T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int lc = tid & 7, lr = tid >> 3;
  const int nk = p.rowb / RC_ROWB;
  const int ld = p.ld;
  const long long total = (long long)p.ntm * ld;
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const int tm = (int)(t / ld), k = (int)(t % ld);
    const int row0 = tm * RC_T;
    // row r of the tile meets b row col[row0 + r][k]; an entry outside [0, Nb) is no address (row 0 stands in, the score is dropped)
    const char* ga[4];
    const char* gb[4];
    int any = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int gi = row0 + lr + 32 * u;
      const int ra = min(gi, p.Na - 1);
      int cj = gi < p.Na ? p.col[(size_t)ra * ld + k] : -1;
      if (cj < 0 || cj >= p.Nb) cj = -1;
      any |= cj >= 0;
      ga[u] = p.a + (size_t)ra * p.rowb + lc * 16;
      gb[u] = p.b + (size_t)max(cj, 0) * p.rowb + lc * 16;
    }
    if (!__syncthreads_or(any)) continue;   // (block-uniform) nothing to gather in this tile
    f32x16 acc[2][2];
    rc_tile_gemm<T>(ga, gb, nk, ldsA, ldsB, tid, wp == wq, acc, [&] {
      if (tid < RC_T) {
        const int gi = row0 + tid;
        const int ra = min(gi, p.Na - 1);
        int cj = gi < p.Na ? p.col[(size_t)ra * ld + k] : -1;
        if (cj < 0 || cj >= p.Nb) cj = -1;
        colS[tid] = cj;
        if constexpr (sizeof(T) == 1) { scA[tid] = p.a_scale[ra]; scB[tid] = p.b_scale[max(cj, 0)]; }
      }
    });
    // (the staged columns and scales are behind the second barrier of the first k-step)
    if (wp == wq) {
      // the diagonal of the tile lies in the diagonal 32 x 32 blocks of the waves (0, 0) and (1, 1)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (acc_row(r, lane) != (lane & 31)) continue;
          const int rl = wp * 64 + i * 32 + (lane & 31);
          if (colS[rl] < 0) continue;
          float sa = 0.f, sb = 0.f;
          if constexpr (sizeof(T) == 1) { sa = scA[rl]; sb = scB[rl]; }
          p.out[(size_t)(row0 + rl) * ld + k] = rc_score<T>(acc[i][i][r], sa, sb);
        }
      }
    }
  }
}

static std::atomic<unsigned long long> g_rc_lds_done{0};

extern "C" int pfr_rank_count_max_thr(void) { return RC_MAX_THR; }


extern "C" int pfr_rank_count(const void* a, const float* a_scale, int Na, const void* b, const float* b_scale, const int* b_id, int Nb,
                              int dtype, int D, const int* excl, const float* thr_val, const int* thr_id, const int* thr_cnt, int ld,
                              unsigned int* cnt, hipStream_t stream) {
  int esz = 0;
  if (int rc = rc_check_operands("pfr_rank_count", dtype, D, &esz)) return rc;
  PFR_CHECK_ARG(Na >= 0 && (b == nullptr || Nb >= 0), "pfr_rank_count: negative row count");
  PFR_CHECK_ARG(ld >= 0 && ld <= RC_MAX_THR, "pfr_rank_count: ld=%d thresholds per row, a launch takes at most %d", ld, RC_MAX_THR);
  if (b == nullptr) { b = a; b_scale = a_scale; Nb = Na; }
  if (Na == 0 || Nb == 0 || ld == 0) return PFR_OK;   // nothing to add
  PFR_CHECK_ARG(a && b && b_id && thr_val && thr_id && thr_cnt && cnt, "pfr_rank_count: null pointer");
  PFR_CHECK_ARG(dtype != PFR_I8 || (a_scale && b_scale), "pfr_rank_count: int8 rows need their scales");
  PFR_CHECK_ARG(pfr_all_dev({a, b, a_scale, b_scale, b_id, excl, thr_val, thr_id, thr_cnt, cnt}),
                "pfr_rank_count: every pointer must be device memory");

  RankCountParams p = {};
  p.a = static_cast<const char*>(a); p.b = static_cast<const char*>(b);
  p.a_scale = a_scale; p.b_scale = b_scale; p.b_id = b_id; p.excl = excl;
  p.thr_val = thr_val; p.thr_id = thr_id; p.thr_cnt = thr_cnt; p.cnt = cnt;
  p.Na = Na; p.Nb = Nb; p.ld = ld;
  p.rowb = D * esz;
  p.ntm = (Na + RC_T - 1) / RC_T; p.ntn = (Nb + RC_T - 1) / RC_T;
  p.nsn = (p.ntn + RC_SUPER - 1) / RC_SUPER;
  p.nsuper = (long long)((p.ntm + RC_SUPER - 1) / RC_SUPER) * p.nsn;
  const int lds = RC_FIXED_LDS + RC_T * ld * 12;
  const long long ntiles = (long long)p.ntm * p.ntn;
  const long long wgs = (long long)(2 * lds <= 160 * 1024 ? 2 : 1) * num_cus();
  const unsigned grid = (unsigned)(ntiles < wgs ? ntiles : wgs);
  PFR_MAX_LDS_ONCE(g_rc_lds_done, RC_FIXED_LDS + RC_T * RC_MAX_THR * 12, (const void*)rank_count_kernel<float>,
                   (const void*)rank_count_kernel<bf16_t>, (const void*)rank_count_kernel<int8_t>);
  if (dtype == PFR_F32) hipLaunchKernelGGL(rank_count_kernel<float>, dim3(grid), dim3(256), lds, stream, p);
  else if (dtype == PFR_BF16) hipLaunchKernelGGL(rank_count_kernel<bf16_t>, dim3(grid), dim3(256), lds, stream, p);
  else hipLaunchKernelGGL(rank_count_kernel<int8_t>, dim3(grid), dim3(256), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_pair_scores_gather(const void* a, const float* a_scale, int Na, const void* b, const float* b_scale, int Nb, int dtype,
                                      int D, const int* col, int ld, float* out, hipStream_t stream) {
  int esz = 0;
  if (int rc = rc_check_operands("pfr_pair_scores_gather", dtype, D, &esz)) return rc;
  PFR_CHECK_ARG(Na >= 0 && (b == nullptr || Nb >= 0) && ld >= 0, "pfr_pair_scores_gather: negative size");
  if (b == nullptr) { b = a; b_scale = a_scale; Nb = Na; }
  if (Na == 0 || Nb == 0 || ld == 0) return PFR_OK;
  PFR_CHECK_ARG(a && b && col && out, "pfr_pair_scores_gather: null pointer");
  PFR_CHECK_ARG(dtype != PFR_I8 || (a_scale && b_scale), "pfr_pair_scores_gather: int8 rows need their scales");
  PFR_CHECK_ARG(pfr_all_dev({a, b, a_scale, b_scale, col, out}), "pfr_pair_scores_gather: every pointer must be device memory");

  RankCountParams p = {};
  p.a = static_cast<const char*>(a); p.b = static_cast<const char*>(b);
  p.a_scale = a_scale; p.b_scale = b_scale; p.col = col; p.out = out;
  p.Na = Na; p.Nb = Nb; p.ld = ld;
  p.rowb = D * esz;
  p.ntm = (Na + RC_T - 1) / RC_T;
  const int lds = 2 * RC_T * RC_ROWB + 3 * RC_T * 4;   // 34 304 bytes: under the default limit
  const long long ntiles = (long long)p.ntm * ld;
  const long long wgs = 2LL * num_cus();
  const unsigned grid = (unsigned)(ntiles < wgs ? ntiles : wgs);
  if (dtype == PFR_F32) hipLaunchKernelGGL(pair_gather_kernel<float>, dim3(grid), dim3(256), lds, stream, p);
  else if (dtype == PFR_BF16) hipLaunchKernelGGL(pair_gather_kernel<bf16_t>, dim3(grid), dim3(256), lds, stream, p);
  else hipLaunchKernelGGL(pair_gather_kernel<int8_t>, dim3(grid), dim3(256), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
