// pfr_cluster.hip — threshold clustering: the score GEMM of the match with a THRESHOLD epilogue (pfr_pairs_above: a compacting append
// of the qualifying pairs and / or a lock-free union-find on a parent array), the same union over an explicit edge list (pfr_cc_union)
// and the flatten pass that turns the forest into canonical labels (pfr_cc_flatten); contract in include/pfr_hip.h.
//
// Schedule and tile product: the tile queue of pfr_tilewalk.h (2 persistent workgroups per CU) and rc_tile_gemm / rc_score of
// pfr_pairtile.h — the code pfr_pair_scores_gather runs — so a score has the gather's bits.
//
// Epilogue, per wave (its 64 x 64 part of the tile = 64 accumulator registers per lane):
//   1. every lane builds the 64-bit mask of its qualifying registers (valid element, RC_VALID of pfr_pairtile.h, and s >= thr); ONE wave
//      vote; nothing qualifies (almost every tile of a realistic threshold): the wave is done.
//   2. edges: the lanes' population counts, an inclusive wave scan, ONE agent-scope add of the wave's total to *count by the last lane
//      (reserve per wave, never per lane); every lane then writes its own pairs at base + its exclusive prefix + 0, 1, ...
//      while the position is below cap.
//   3. unions: every lane unites its own pairs one after the other (uf_union below).
//
// Union-find: uf_find / uf_union / uf_budget of pfr_unionfind.h (shared with pfr_dbscan.hip; the invariants and the loop cap are there).
#include "pfr_pairtile.h"
#include "pfr_unionfind.h"

struct ClusterParams {
  PairOperands o;
  float thr;
  int* edge_i;
  int* edge_j;
  float* edge_s;
  unsigned long long cap;
  unsigned long long* count;
  int* parent;
  int n_nodes, budget;
  int* status;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void pairs_above_kernel(const ClusterParams p) {   // (2 workgroups per CU: at most 256 registers)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *ldsA, *ldsB;
  float *scA, *scB;
  rc_carve(smem, ldsA, ldsB, scA, scB);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int nk = p.o.rowb / RC_ROWB;
  const long long total = p.o.nsuper * (RC_SUPER * RC_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    int tm, tn;
    if (!tw_tile(t, p.o.ntm, p.o.ntn, p.o.nsn, p.o.sym, tm, tn)) continue;   // (block-uniform)
    const int row0 = tm * RC_T, col0 = tn * RC_T;
    const char* ga[4];
    const char* gb[4];
    rc_operand_rows(p.o.a, p.o.b, p.o.rowb, row0, col0, p.o.Na, p.o.Nb, tid, ga, gb);
    f32x16 acc[2][2];
    rc_tile_gemm<T>(ga, gb, nk, ldsA, ldsB, tid, true, acc,
                    [&] { rc_stage_scales<T>(p.o.a_scale, p.o.b_scale, row0, col0, p.o.Na, p.o.Nb, tid, scA, scB); });

    // ---- 1. the lanes' qualifying masks: bit (j * 2 + i) * 16 + r <-> acc[i][j][r]
    const bool diag = rc_tile_diag(p.o.sym, tm, tn);
    const bool full = rc_tile_full(diag, row0, col0, p.o.Na, p.o.Nb);
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
          const bool ok = RC_VALID(full, diag, gi, gj, p.o.Na, p.o.Nb);
          if (ok && s >= p.thr) mask |= 1ull << ((j * 2 + i) * 16 + r);
        }
      }
    }
    if (__ballot(mask != 0ull) == 0ull) continue;   // (wave-uniform; the epilogue holds no barrier)

    // ---- 2. reserve the wave's positions: one add
    unsigned long long pos = 0ull;
    if (p.edge_i) {
      const unsigned int mine = (unsigned int)__popcll(mask);
      unsigned int incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      unsigned long long base = 0ull;
      if (lane == 63) base = __hip_atomic_fetch_add(p.count, (unsigned long long)incl, UF_RLX_AGENT);
      base = __shfl(base, 63, 64);
      pos = base + (incl - mine);
    }

    // ---- 3. this lane's pairs
    if (mask != 0ull) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int cl = wq * 64 + j * 32 + (lane & 31);
        const int v = p.o.b_off + col0 + cl;
        float sb = 0.f;
        if constexpr (sizeof(T) == 1) sb = scB[cl];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (!((mask >> ((j * 2 + i) * 16 + r)) & 1ull)) continue;
            const int rl = wp * 64 + i * 32 + acc_row(r, lane);
            const int u = p.o.a_off + row0 + rl;
            if (p.edge_i) {
              if (pos < p.cap) {
                p.edge_i[pos] = u;
                p.edge_j[pos] = v;
                if (p.edge_s) {
                  float sa = 0.f;
                  if constexpr (sizeof(T) == 1) sa = scA[rl];
                  p.edge_s[pos] = rc_score<T>(acc[i][j][r], sa, sb);
                }
              }
              ++pos;
            }
            if (p.parent && u < p.n_nodes && v < p.n_nodes) uf_union(p.parent, u, v, p.budget, p.status);   // (u, v >= 0: checked offsets)
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void cc_union_kernel(int* parent, int n_nodes, const int* edge_i, const int* edge_j, long long E,
                                                       int budget, int* status) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
    const int u = edge_i[e], v = edge_j[e];
    if (u < 0 || v < 0 || u >= n_nodes || v >= n_nodes || u == v) continue;
    uf_union(parent, u, v, budget, status);
  }
}

// Read-only walk to the root (no halving: the kernel writes labels only).  An entry outside [0, x] ends the walk where it stands.
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, int n_nodes, int* labels) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= n_nodes) return;
  int cur = x;
  for (int it = 0; it < n_nodes; ++it) {
    const int q = __hip_atomic_load(parent + cur, UF_RLX_AGENT);
    if (q == cur || q < 0 || q > cur) break;
    cur = q;
  }
  __hip_atomic_store(labels + x, cur, UF_RLX_AGENT);
}

extern "C" int pfr_pairs_above(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb,
                               int b_off, int dtype, int D, float thr, int* edge_i, int* edge_j, float* edge_s, long cap,
                               unsigned long long* count, int* parent, int n_nodes, int* status, hipStream_t stream) {
  const char* who = "pfr_pairs_above";
  ClusterParams p = {};
  if (int rc = rc_operands(who, a, a_scale, Na, a_off, b, b_scale, Nb, b_off, dtype, D, &p.o)) return rc;
  PFR_CHECK_ARG(p.o.Na >= 0 && p.o.Nb >= 0, "%s: negative row count", who);
  PFR_CHECK_ARG(p.o.a_off >= 0 && p.o.b_off >= 0, "%s: negative offset", who);
  PFR_CHECK_ARG(p.o.a_off <= INT_MAX - p.o.Na && p.o.b_off <= INT_MAX - p.o.Nb, "%s: offset + rows pass 2^31 - 1", who);
  PFR_CHECK_ARG(edge_i || parent, "%s: neither an edge list nor a parent array", who);
  PFR_CHECK_ARG(!edge_i || (edge_j && count && cap >= 0), "%s: an edge list needs edge_j, count and cap >= 0", who);
  PFR_CHECK_ARG(edge_i || (!edge_j && !edge_s), "%s: edge_j / edge_s without edge_i", who);
  PFR_CHECK_ARG(!parent || (status && n_nodes >= 0), "%s: a parent array needs status and n_nodes >= 0", who);
  unsigned grid = 0;
  if (int rc = rc_ready(who, &p.o, dtype, {edge_i, edge_j, edge_s, count, parent, status}, true, 2, &grid)) return rc;
  if (grid == 0) return PFR_OK;   // no pair
  p.thr = thr;
  p.edge_i = edge_i; p.edge_j = edge_j; p.edge_s = edge_s; p.cap = edge_i ? (unsigned long long)cap : 0ull; p.count = count;
  p.parent = parent; p.n_nodes = parent ? n_nodes : 0; p.budget = uf_budget(p.n_nodes); p.status = status;
  RC_LAUNCH(dtype, grid, RC_LDS_BASE, stream, p, pairs_above_kernel);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_cc_union(int* parent, int n_nodes, const int* edge_i, const int* edge_j, long E, int* status, hipStream_t stream) {
  PFR_CHECK_ARG(n_nodes >= 0 && E >= 0, "pfr_cc_union: negative size");
  if (E == 0 || n_nodes == 0) return PFR_OK;
  PFR_CHECK_ARG(parent && edge_i && edge_j && status, "pfr_cc_union: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({parent, edge_i, edge_j, status}), "pfr_cc_union: every pointer must be device memory");
  const long long blocks = ((long long)E + 255) / 256, wgs = 8LL * num_cus();
  hipLaunchKernelGGL(cc_union_kernel, dim3((unsigned)(blocks < wgs ? blocks : wgs)), dim3(256), 0, stream, parent, n_nodes, edge_i, edge_j,
                     (long long)E, uf_budget(n_nodes), status);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_cc_flatten(int* parent, int n_nodes, int* labels, hipStream_t stream) {
  PFR_CHECK_ARG(n_nodes >= 0, "pfr_cc_flatten: negative size");
  if (n_nodes == 0) return PFR_OK;
  PFR_CHECK_ARG(parent && labels, "pfr_cc_flatten: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({parent, labels}), "pfr_cc_flatten: every pointer must be device memory");
  hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, stream, parent, n_nodes, labels);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
