// pfr_rankcount.hip — exact retrieval ranks: the score GEMM of the match with a RANK-COUNTING epilogue (pfr_rank_count) and the gather
// of single scores by the same tile code (pfr_pair_scores_gather); contract in include/pfr_hip.h.  The rank of a positive is a count
// (how many items precede it), so nothing Na x Nb is written and nothing is sorted: every score is compared, where the MFMA left it,
// against the few thresholds of its row.
//
// Schedule and tile product: the tile queue of pfr_tilewalk.h and rc_tile_gemm / rc_score of pfr_pairtile.h.  Ranks are per row, so
// every (row, column) tile is visited, also of a set against itself: there is no triangle to skip.
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
#include "pfr_pairtile.h"

#define RC_MAX_THR 64       // thresholds per row of one launch
#define RC_FIXED_LDS (RC_LDS_BASE + 4 * RC_T * 4)

struct RankCountParams {
  PairOperands o;           // (sym = 0: the whole rectangle)
  const int* b_id;
  const int* excl;          // or nullptr
  const float* thr_val;
  const int* thr_id;
  const int* thr_cnt;
  unsigned int* cnt;
  const int* col;           // gather
  float* out;               // gather
  int ld;
};

template <typename T>
__global__ __launch_bounds__(256) void rank_count_kernel(const RankCountParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *ldsA, *ldsB;
  float *scA, *scB;
  int* idB = reinterpret_cast<int*>(rc_carve(smem, ldsA, ldsB, scA, scB));
  int* exA = idB + RC_T;
  int* cntA = exA + RC_T;
  float* tmin = reinterpret_cast<float*>(cntA + RC_T);
  float* thrV = tmin + RC_T;                          // [128][ld]
  int* thrI = reinterpret_cast<int*>(thrV + RC_T * p.ld);
  unsigned int* c = reinterpret_cast<unsigned int*>(thrI + RC_T * p.ld);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int ld = p.ld, slots = RC_T * ld;
  for (int s = tid; s < slots; s += 256) c[s] = 0;
  // (the first tile's barriers order this against the first LDS atomic)

  const int nk = p.o.rowb / RC_ROWB;
  const bool has_excl = p.excl != nullptr;
  const long long total = p.o.nsuper * (RC_SUPER * RC_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    int tm, tn;
    if (!tw_tile(t, p.o.ntm, p.o.ntn, p.o.nsn, 0, tm, tn)) continue;   // (block-uniform)
    const int row0 = tm * RC_T, col0 = tn * RC_T;
    const char* ga[4];
    const char* gb[4];
    rc_operand_rows(p.o.a, p.o.b, p.o.rowb, row0, col0, p.o.Na, p.o.Nb, tid, ga, gb);
    f32x16 acc[2][2];
    rc_tile_gemm<T>(ga, gb, nk, ldsA, ldsB, tid, true, acc, [&] {
      if (tid < RC_T) {
        const int ra = min(row0 + tid, p.o.Na - 1), rb = min(col0 + tid, p.o.Nb - 1);
        idB[tid] = p.b_id[rb];
        exA[tid] = has_excl ? p.excl[ra] : 0;
        cntA[tid] = row0 + tid < p.o.Na ? min(max(p.thr_cnt[ra], 0), ld) : 0;   // a row past the end has no thresholds
      }
      rc_stage_scales<T>(p.o.a_scale, p.o.b_scale, row0, col0, p.o.Na, p.o.Nb, tid, scA, scB);
      // the rows' thresholds: [128][ld] of the tile is one contiguous range of thr_val / thr_id, cut at the last valid row
      const int nvalid = min(RC_T, p.o.Na - row0) * ld;
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
    const bool full = rc_tile_full(false, row0, col0, p.o.Na, p.o.Nb);   // no element of the tile is masked by the edges
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cl = wq * 64 + j * 32 + (lane & 31);
      const int idj = idB[cl];
      const bool colok = full || col0 + cl < p.o.Nb;
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
  char *ldsA, *ldsB;
  float *scA, *scB;
  int* colS = reinterpret_cast<int*>(rc_carve(smem, ldsA, ldsB, scA, scB));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int lc = tid & 7, lr = tid >> 3;
  const int nk = p.o.rowb / RC_ROWB;
  const int ld = p.ld;
  const long long total = (long long)p.o.ntm * ld;
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
      const int ra = min(gi, p.o.Na - 1);
      int cj = gi < p.o.Na ? p.col[(size_t)ra * ld + k] : -1;
      if (cj < 0 || cj >= p.o.Nb) cj = -1;
      any |= cj >= 0;
      ga[u] = p.o.a + (size_t)ra * p.o.rowb + lc * 16;
      gb[u] = p.o.b + (size_t)max(cj, 0) * p.o.rowb + lc * 16;
    }
    if (!__syncthreads_or(any)) continue;   // (block-uniform) nothing to gather in this tile
    f32x16 acc[2][2];
    rc_tile_gemm<T>(ga, gb, nk, ldsA, ldsB, tid, wp == wq, acc, [&] {
      if (tid < RC_T) {
        const int gi = row0 + tid;
        const int ra = min(gi, p.o.Na - 1);
        int cj = gi < p.o.Na ? p.col[(size_t)ra * ld + k] : -1;
        if (cj < 0 || cj >= p.o.Nb) cj = -1;
        colS[tid] = cj;
        if constexpr (sizeof(T) == 1) { scA[tid] = p.o.a_scale[ra]; scB[tid] = p.o.b_scale[max(cj, 0)]; }
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
  const char* who = "pfr_rank_count";
  RankCountParams p = {};
  if (int rc = rc_operands(who, a, a_scale, Na, 0, b, b_scale, Nb, 0, dtype, D, &p.o)) return rc;
  p.o.sym = 0;   // a set against itself is still the whole rectangle
  PFR_CHECK_ARG(p.o.Na >= 0 && p.o.Nb >= 0, "%s: negative row count", who);
  PFR_CHECK_ARG(ld >= 0 && ld <= RC_MAX_THR, "%s: ld=%d thresholds per row, a launch takes at most %d", who, ld, RC_MAX_THR);
  if (ld == 0) return PFR_OK;   // nothing to add
  const int lds = RC_FIXED_LDS + RC_T * ld * 12;
  unsigned grid = 0;
  if (int rc = rc_ready(who, &p.o, dtype, {b_id, excl, thr_val, thr_id, thr_cnt, cnt}, b_id && thr_val && thr_id && thr_cnt && cnt,
                        2 * lds <= 160 * 1024 ? 2 : 1, &grid))
    return rc;
  if (grid == 0) return PFR_OK;
  p.b_id = b_id; p.excl = excl;
  p.thr_val = thr_val; p.thr_id = thr_id; p.thr_cnt = thr_cnt; p.cnt = cnt;
  p.ld = ld;
  PFR_MAX_LDS_ONCE(g_rc_lds_done, RC_FIXED_LDS + RC_T * RC_MAX_THR * 12, (const void*)rank_count_kernel<float>,
                   (const void*)rank_count_kernel<bf16_t>, (const void*)rank_count_kernel<int8_t>);
  RC_LAUNCH(dtype, grid, lds, stream, p, rank_count_kernel);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_pair_scores_gather(const void* a, const float* a_scale, int Na, const void* b, const float* b_scale, int Nb, int dtype,
                                      int D, const int* col, int ld, float* out, hipStream_t stream) {
  const char* who = "pfr_pair_scores_gather";
  RankCountParams p = {};
  if (int rc = rc_operands(who, a, a_scale, Na, 0, b, b_scale, Nb, 0, dtype, D, &p.o)) return rc;
  p.o.sym = 0;
  PFR_CHECK_ARG(p.o.Na >= 0 && p.o.Nb >= 0 && ld >= 0, "%s: negative size", who);
  if (ld == 0) return PFR_OK;
  unsigned grid = 0;
  if (int rc = rc_ready(who, &p.o, dtype, {col, out}, col && out, 2, &grid)) return rc;
  if (grid == 0) return PFR_OK;
  p.col = col; p.out = out;
  p.ld = ld;
  grid = tw_grid((long long)p.o.ntm * ld, 2, num_cus());   // one tile per (row tile, list position)
  RC_LAUNCH(dtype, grid, RC_LDS_BASE + RC_T * 4, stream, p, pair_gather_kernel);   // 34 304 bytes: under the default limit
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
