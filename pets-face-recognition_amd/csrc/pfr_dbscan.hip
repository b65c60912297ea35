// pfr_dbscan.hip — DBSCAN identity clustering on the match GEMM: two passes of the score GEMM of pfr_pairs_above with a DEGREE epilogue
// (pfr_neighbor_count) and a LINK epilogue (pfr_dbscan_link: core-core pairs are united in the lock-free union-find, a border node keeps
// its best core neighbour in a 64-bit max key), and the label pass (pfr_dbscan_labels); contract in include/pfr_hip.h.  Nothing N x N and
// no edge list is written.
//
// Schedule and step 1 of the epilogue are pairs_above_kernel's (pfr_cluster.hip): persistent workgroups (2 per CU) walk the 128 x 128
// tiles in super-tiles of 16 x 16, upper triangle only in symmetric mode; the tile product is rc_tile_gemm / rc_score of pfr_pairtile.h,
// so a score has the bits of pfr_pairs_above and pfr_pair_scores_gather; every lane builds the 64-bit mask of its qualifying registers and
// ONE wave vote ends the wave when nothing qualifies.
//
// Degree epilogue, per wave (its 64 x 64 part of the tile): no atomic per pair.  Lane l holds column (l & 31) of both 32-column halves:
// the column's count is the population count of the lane's mask bits of that half plus the same from the lane 32 away.  For a register
// (i, r) the 32 lanes of one half share the row acc_row(r, lane): the row's count is a wave vote on that bit per column half.  Lane l
// collects the count of local column l and of local row l, and the wave issues TWO atomic instructions: one add per touched column and
// one per touched row.
//
// Link epilogue: every lane walks its own pairs (as the union epilogue of pfr_cluster.hip); deg is read with plain loads (the previous
// launch wrote it).  The border key is (order-preserving uint32 of the score, 0xffffffff - core index): its maximum is "highest score,
// then smallest index" whatever the order of arrival.
#include "pfr_pairtile.h"
#include "pfr_scorekey.h"     // db_score_key: the order-preserving uint32 of a score (shared with pfr_extremes.hip)
#include "pfr_unionfind.h"

#define DB_LDS (2 * RC_T * RC_ROWB + 2 * RC_T * 4)   // 33 792 bytes: under the default limit

struct DbscanParams {
  const char* a;
  const char* b;
  const float* a_scale;
  const float* b_scale;
  int Na, Nb, sym;
  int a_off, b_off;
  int rowb;                 // bytes per operand row
  float thr;
  int* deg;                 // count: accumulated; link: read only
  int min_neighbors;
  int* parent;
  unsigned long long* best;
  int n_nodes, budget;
  int* status;
  int ntm, ntn, nsn;
  long long nsuper;
};

template <typename T, bool LINK>
__global__ __launch_bounds__(256, 2) void dbscan_pass_kernel(const DbscanParams p) {   // (2 workgroups per CU: at most 256 registers)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsA = smem;                                  // [128][128 B]
  char* ldsB = smem + RC_T * RC_ROWB;                 // [128][128 B]
  float* scA = reinterpret_cast<float*>(smem + 2 * RC_T * RC_ROWB);
  float* scB = scA + RC_T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int lc = tid & 7, lr = tid >> 3;
  const int nk = p.rowb / RC_ROWB;
  const long long total = p.nsuper * (RC_SUPER * RC_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const long long su = t / (RC_SUPER * RC_SUPER);
    const int l = (int)(t % (RC_SUPER * RC_SUPER));
    int sm, sn;
    if (p.sym) {
      // super-tile su of the upper triangle, row-major: row r starts at r * ns - r (r - 1) / 2
      const double ns2 = 2.0 * p.nsn + 1.0;
      int r = (int)((ns2 - sqrt(ns2 * ns2 - 8.0 * (double)su)) * 0.5);
      r = r < 0 ? 0 : (r > p.nsn - 1 ? p.nsn - 1 : r);
      while (r > 0 && (long long)r * p.nsn - (long long)r * (r - 1) / 2 > su) --r;
      while ((long long)(r + 1) * p.nsn - (long long)(r + 1) * r / 2 <= su) ++r;
      sm = r;
      sn = r + (int)(su - ((long long)r * p.nsn - (long long)r * (r - 1) / 2));
    } else {
      sm = (int)(su / p.nsn);
      sn = (int)(su % p.nsn);
    }
    const int tm = sm * RC_SUPER + l / RC_SUPER, tn = sn * RC_SUPER + l % RC_SUPER;
    if (tm >= p.ntm || tn >= p.ntn || (p.sym && tn < tm)) continue;   // (block-uniform)
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
      if constexpr (sizeof(T) == 1) {
        if (tid < RC_T) {
          const int ra = min(row0 + tid, p.Na - 1), rb = min(col0 + tid, p.Nb - 1);
          scA[tid] = p.a_scale[ra];
          scB[tid] = p.b_scale[rb];
        }
      }
    });
    // (the staged scales are behind the second barrier of the first k-step; the next tile's first barrier keeps them until every wave
    //  has left this epilogue)

    // ---- 1. the lanes' qualifying masks: bit (j * 2 + i) * 16 + r <-> acc[i][j][r]
    const bool diag = p.sym && tm == tn;
    const bool full = !diag && row0 + RC_T <= p.Na && col0 + RC_T <= p.Nb;   // no element of the tile is masked
    unsigned long long mask = 0ull;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cl = wq * 64 + j * 32 + (lane & 31);
      const int gj = col0 + cl;
      float sb = 0.f;
      if constexpr (sizeof(T) == 1) sb = scB[cl];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wp * 64 + i * 32 + acc_row(r, lane);
          const int gi = row0 + rl;
          float sa = 0.f;
          if constexpr (sizeof(T) == 1) sa = scA[rl];
          const float s = rc_score<T>(acc[i][j][r], sa, sb);
          const bool ok = full || (gi < p.Na && gj < p.Nb && (!diag || gi < gj));
          if (ok && s >= p.thr) mask |= 1ull << ((j * 2 + i) * 16 + r);
        }
      }
    }
    if (__ballot(mask != 0ull) == 0ull) continue;   // (wave-uniform; the epilogue holds no barrier)

    if constexpr (!LINK) {
      // ---- 2. degrees.  Columns: bits [32 j, 32 j + 32) of the mask are the lane's 32 rows of column half j; the lane 32 away holds
      // the other 32 rows of the same column.  Lane l then owns local column l = 32 j + (l & 31).
      unsigned int c0 = (unsigned int)__popc((unsigned int)mask), c1 = (unsigned int)__popc((unsigned int)(mask >> 32));
      c0 += __shfl_xor(c0, 32, 64);
      c1 += __shfl_xor(c1, 32, 64);
      const int ccnt = (int)(lane < 32 ? c0 : c1);
      // Rows: register (i, r) of the lanes 0..31 is local row i * 32 + acc_row(r, 0), of the lanes 32..63 that row + 4; the vote's low
      // and high words are their counts over one column half.  Lane l owns local row l.
      int rcnt = 0;
      // (a rolled loop on purpose: the mask is the only thing indexed, and 64 unrolled votes keep 128 scalar registers alive)
#pragma unroll 1
      for (int k = 0; k < 32; ++k) {                    // k = i * 16 + r
        const unsigned long long v0 = __ballot(((mask >> k) & 1ull) != 0ull);           // column half 0
        const unsigned long long v1 = __ballot(((mask >> (32 + k)) & 1ull) != 0ull);    // column half 1
        const int lo = __popc((unsigned int)v0) + __popc((unsigned int)v1);
        const int hi = __popc((unsigned int)(v0 >> 32)) + __popc((unsigned int)(v1 >> 32));
        const int row = (k >> 4) * 32 + (k & 3) + 8 * ((k & 15) >> 2);
        if (lane == row) rcnt = lo;
        if (lane == row + 4) rcnt = hi;
      }
      // one add per touched column and one per touched row (a count > 0 means a valid element: the node is below its set's size, and
      // a_off + Na, b_off + Nb <= n_nodes is checked on the host)
      if (ccnt > 0) __hip_atomic_fetch_add(p.deg + (p.b_off + col0 + wq * 64 + lane), ccnt, UF_RLX_AGENT);
      if (rcnt > 0) __hip_atomic_fetch_add(p.deg + (p.a_off + row0 + wp * 64 + lane), rcnt, UF_RLX_AGENT);
    } else {
      // ---- 2. this lane's pairs: core-core -> union, core-border -> the border's key, else nothing
      if (mask != 0ull) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if ((unsigned int)(mask >> (32 * j)) == 0u) continue;
          const int cl = wq * 64 + j * 32 + (lane & 31);
          const int v = p.b_off + col0 + cl;            // (< n_nodes: a set bit is a valid column)
          const bool vcore = p.deg[v] >= p.min_neighbors;
          float sb = 0.f;
          if constexpr (sizeof(T) == 1) sb = scB[cl];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              if (!((mask >> ((j * 2 + i) * 16 + r)) & 1ull)) continue;
              const int rl = wp * 64 + i * 32 + acc_row(r, lane);
              const int u = p.a_off + row0 + rl;        // (< n_nodes: a set bit is a valid row)
              const bool ucore = p.deg[u] >= p.min_neighbors;
              if (ucore && vcore) {
                uf_union(p.parent, u, v, p.budget, p.status);
              } else if (ucore || vcore) {
                float sa = 0.f;
                if constexpr (sizeof(T) == 1) sa = scA[rl];
                const unsigned int sk = db_score_key(rc_score<T>(acc[i][j][r], sa, sb));
                const int core = ucore ? u : v, border = ucore ? v : u;
                const unsigned long long key = ((unsigned long long)sk << 32) | (unsigned long long)(0xffffffffu - (unsigned int)core);
                __hip_atomic_fetch_max(p.best + border, key, UF_RLX_AGENT);
              }
            }
          }
        }
      }
    }
  }
}

// One thread per node.  Core: the read-only root walk of cc_flatten_kernel (capped at n_nodes steps, range-checked).  Border: the root
// of the core decoded from best (range-checked before it is used).  Noise: -1.
__global__ __launch_bounds__(256) void dbscan_labels_kernel(const int* parent, const int* deg, const unsigned long long* best,
                                                            int min_neighbors, int n_nodes, int* labels) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= n_nodes) return;
  int cur = x;
  if (deg[x] < min_neighbors) {
    const unsigned long long key = best[x];
    const unsigned int core = 0xffffffffu - (unsigned int)key;
    if (key == 0ull || core >= (unsigned int)n_nodes) {   // no core neighbour (or a key that decodes outside the set: never an index)
      labels[x] = -1;
      return;
    }
    cur = (int)core;
  }
  for (int it = 0; it < n_nodes; ++it) {
    const int q = __hip_atomic_load(const_cast<int*>(parent) + cur, UF_RLX_AGENT);
    if (q == cur || q < 0 || q > cur) break;
    cur = q;
  }
  labels[x] = cur;
}

// the checks and the geometry both GEMM passes share; *run = false: nothing to do
static int db_setup(const char* who, const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb,
                    int b_off, int dtype, int D, float thr, int n_nodes, std::initializer_list<const void*> outs, bool outs_ok,
                    DbscanParams* p, unsigned* grid, bool* run) {
  *run = false;
  int esz = 0;
  if (int rc = rc_check_operands(who, dtype, D, &esz)) return rc;
  const bool sym = b == nullptr;
  if (sym) { b = a; b_scale = a_scale; Nb = Na; b_off = a_off; }
  PFR_CHECK_ARG(Na >= 0 && Nb >= 0 && n_nodes >= 0, "%s: negative size", who);
  PFR_CHECK_ARG(a_off >= 0 && b_off >= 0, "%s: negative offset", who);
  PFR_CHECK_ARG((long long)a_off + Na <= (long long)n_nodes && (long long)b_off + Nb <= (long long)n_nodes,
                "%s: offset + rows pass n_nodes=%d", who, n_nodes);
  if (Na == 0 || Nb == 0 || (sym && Na == 1)) return PFR_OK;   // no pair
  PFR_CHECK_ARG(a && b && outs_ok, "%s: null pointer", who);
  PFR_CHECK_ARG(dtype != PFR_I8 || (a_scale && b_scale), "%s: int8 rows need their scales", who);
  PFR_CHECK_ARG(pfr_all_dev({a, b, a_scale, b_scale}) && pfr_all_dev(outs), "%s: every pointer must be device memory", who);
  *p = DbscanParams{};
  p->a = static_cast<const char*>(a); p->b = static_cast<const char*>(b);
  p->a_scale = a_scale; p->b_scale = b_scale;
  p->Na = Na; p->Nb = Nb; p->sym = sym ? 1 : 0;
  p->a_off = a_off; p->b_off = b_off;
  p->rowb = D * esz;
  p->thr = thr;
  p->n_nodes = n_nodes; p->budget = uf_budget(n_nodes);
  p->ntm = (Na + RC_T - 1) / RC_T; p->ntn = (Nb + RC_T - 1) / RC_T;
  p->nsn = (p->ntn + RC_SUPER - 1) / RC_SUPER;
  const int nsm = (p->ntm + RC_SUPER - 1) / RC_SUPER;
  p->nsuper = sym ? (long long)p->nsn * (p->nsn + 1) / 2 : (long long)nsm * p->nsn;
  const long long ntiles = sym ? (long long)p->ntn * (p->ntn + 1) / 2 : (long long)p->ntm * p->ntn;
  const long long wgs = 2LL * num_cus();
  *grid = (unsigned)(ntiles < wgs ? ntiles : wgs);
  *run = true;
  return PFR_OK;
}

template <bool LINK> static void db_launch(int dtype, unsigned grid, hipStream_t stream, const DbscanParams& p) {
  if (dtype == PFR_F32) hipLaunchKernelGGL((dbscan_pass_kernel<float, LINK>), dim3(grid), dim3(256), DB_LDS, stream, p);
  else if (dtype == PFR_BF16) hipLaunchKernelGGL((dbscan_pass_kernel<bf16_t, LINK>), dim3(grid), dim3(256), DB_LDS, stream, p);
  else hipLaunchKernelGGL((dbscan_pass_kernel<int8_t, LINK>), dim3(grid), dim3(256), DB_LDS, stream, p);
}

extern "C" int pfr_neighbor_count(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb,
                                  int b_off, int dtype, int D, float thr, int* deg, int n_nodes, hipStream_t stream) {
  DbscanParams p;
  unsigned grid = 0;
  bool run = false;
  if (int rc = db_setup("pfr_neighbor_count", a, a_scale, Na, a_off, b, b_scale, Nb, b_off, dtype, D, thr, n_nodes, {deg}, deg != nullptr,
                        &p, &grid, &run))
    return rc;
  if (!run) return PFR_OK;
  p.deg = deg;
  db_launch<false>(dtype, grid, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_dbscan_link(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb,
                               int b_off, int dtype, int D, float thr, const int* deg, int min_neighbors, int* parent,
                               unsigned long long* best, int n_nodes, int* status, hipStream_t stream) {
  PFR_CHECK_ARG(min_neighbors >= 0, "pfr_dbscan_link: min_neighbors=%d must be >= 0", min_neighbors);
  DbscanParams p;
  unsigned grid = 0;
  bool run = false;
  if (int rc = db_setup("pfr_dbscan_link", a, a_scale, Na, a_off, b, b_scale, Nb, b_off, dtype, D, thr, n_nodes,
                        {deg, parent, best, status}, deg && parent && best && status, &p, &grid, &run))
    return rc;
  if (!run) return PFR_OK;
  p.deg = const_cast<int*>(deg);
  p.min_neighbors = min_neighbors;
  p.parent = parent; p.best = best; p.status = status;
  db_launch<true>(dtype, grid, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_dbscan_labels(const int* parent, const int* deg, const unsigned long long* best, int min_neighbors, int n_nodes,
                                 int* labels, hipStream_t stream) {
  PFR_CHECK_ARG(n_nodes >= 0, "pfr_dbscan_labels: negative size");
  PFR_CHECK_ARG(min_neighbors >= 0, "pfr_dbscan_labels: min_neighbors=%d must be >= 0", min_neighbors);
  if (n_nodes == 0) return PFR_OK;
  PFR_CHECK_ARG(parent && deg && best && labels, "pfr_dbscan_labels: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({parent, deg, best, labels}), "pfr_dbscan_labels: every pointer must be device memory");
  hipLaunchKernelGGL(dbscan_labels_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, stream, parent, deg, best, min_neighbors,
                     n_nodes, labels);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
