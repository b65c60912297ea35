// pfr_cluster.hip — threshold clustering: the score GEMM of the match with a THRESHOLD epilogue (pfr_pairs_above: a compacting append
// of the qualifying pairs and / or a lock-free union-find on a parent array), the same union over an explicit edge list (pfr_cc_union)
// and the flatten pass that turns the forest into canonical labels (pfr_cc_flatten); contract in include/pfr_hip.h.
//
// Schedule (pfr_pairhist.hip's): persistent workgroups (2 per CU) walk a queue of 128 x 128 tiles in super-tiles of 16 x 16 tiles;
// symmetric mode enumerates the super-tiles of the upper triangle only and skips the tiles below the diagonal.  The tile product is
// rc_tile_gemm / rc_score of pfr_pairtile.h — the code pfr_pair_scores_gather runs — so a score has the gather's bits.
//
// Epilogue, per wave (its 64 x 64 part of the tile = 64 accumulator registers per lane):
//   1. every lane builds the 64-bit mask of its qualifying registers (valid element and s >= thr); ONE wave vote; nothing qualifies
//      (almost every tile of a realistic threshold): the wave is done.
//   2. edges: the lanes' population counts, an inclusive wave scan, ONE agent-scope add of the wave's total to *count by the last lane
//      (reserve per wave, never per lane); every lane then writes its own pairs at base + its exclusive prefix + 0, 1, ...
//      while the position is below cap.
//   3. unions: every lane unites its own pairs one after the other (uf_union below).
//
// Union-find: uf_find / uf_union / uf_budget of pfr_unionfind.h (shared with pfr_dbscan.hip; the invariants and the loop cap are there).
#include "pfr_pairtile.h"
#include "pfr_unionfind.h"

#define CL_LDS (2 * RC_T * RC_ROWB + 2 * RC_T * 4)   // 33 792 bytes: under the default limit

struct ClusterParams {
  const char* a;
  const char* b;
  const float* a_scale;
  const float* b_scale;
  int Na, Nb, sym;
  int a_off, b_off;
  int rowb;                 // bytes per operand row
  float thr;
  int* edge_i;
  int* edge_j;
  float* edge_s;
  unsigned long long cap;
  unsigned long long* count;
  int* parent;
  int n_nodes, budget;
  int* status;
  int ntm, ntn, nsn;
  long long nsuper;
};

template <typename T>
__global__ __launch_bounds__(256, 2) void pairs_above_kernel(const ClusterParams p) {   // (2 workgroups per CU: at most 256 registers)
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
        const int v = p.b_off + col0 + cl;
        float sb = 0.f;
        if constexpr (sizeof(T) == 1) sb = scB[cl];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (!((mask >> ((j * 2 + i) * 16 + r)) & 1ull)) continue;
            const int rl = wp * 64 + i * 32 + acc_row(r, lane);
            const int u = p.a_off + row0 + rl;
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
  int esz = 0;
  if (int rc = rc_check_operands("pfr_pairs_above", dtype, D, &esz)) return rc;
  const bool sym = b == nullptr;
  if (sym) { b = a; b_scale = a_scale; Nb = Na; b_off = a_off; }
  PFR_CHECK_ARG(Na >= 0 && Nb >= 0, "pfr_pairs_above: negative row count");
  PFR_CHECK_ARG(a_off >= 0 && b_off >= 0, "pfr_pairs_above: negative offset");
  PFR_CHECK_ARG(a_off <= INT_MAX - Na && b_off <= INT_MAX - Nb, "pfr_pairs_above: offset + rows pass 2^31 - 1");
  PFR_CHECK_ARG(edge_i || parent, "pfr_pairs_above: neither an edge list nor a parent array");
  PFR_CHECK_ARG(!edge_i || (edge_j && count && cap >= 0), "pfr_pairs_above: an edge list needs edge_j, count and cap >= 0");
  PFR_CHECK_ARG(edge_i || (!edge_j && !edge_s), "pfr_pairs_above: edge_j / edge_s without edge_i");
  PFR_CHECK_ARG(!parent || (status && n_nodes >= 0), "pfr_pairs_above: a parent array needs status and n_nodes >= 0");
  if (Na == 0 || Nb == 0 || (sym && Na == 1)) return PFR_OK;   // no pair
  PFR_CHECK_ARG(a && b, "pfr_pairs_above: null pointer");
  PFR_CHECK_ARG(dtype != PFR_I8 || (a_scale && b_scale), "pfr_pairs_above: int8 rows need their scales");
  PFR_CHECK_ARG(pfr_all_dev({a, b, a_scale, b_scale, edge_i, edge_j, edge_s, count, parent, status}),
                "pfr_pairs_above: every pointer must be device memory");

  ClusterParams p = {};
  p.a = static_cast<const char*>(a); p.b = static_cast<const char*>(b);
  p.a_scale = a_scale; p.b_scale = b_scale;
  p.Na = Na; p.Nb = Nb; p.sym = sym ? 1 : 0;
  p.a_off = a_off; p.b_off = b_off;
  p.rowb = D * esz;
  p.thr = thr;
  p.edge_i = edge_i; p.edge_j = edge_j; p.edge_s = edge_s; p.cap = edge_i ? (unsigned long long)cap : 0ull; p.count = count;
  p.parent = parent; p.n_nodes = parent ? n_nodes : 0; p.budget = uf_budget(p.n_nodes); p.status = status;
  p.ntm = (Na + RC_T - 1) / RC_T; p.ntn = (Nb + RC_T - 1) / RC_T;
  p.nsn = (p.ntn + RC_SUPER - 1) / RC_SUPER;
  const int nsm = (p.ntm + RC_SUPER - 1) / RC_SUPER;
  p.nsuper = sym ? (long long)p.nsn * (p.nsn + 1) / 2 : (long long)nsm * p.nsn;
  const long long ntiles = sym ? (long long)p.ntn * (p.ntn + 1) / 2 : (long long)p.ntm * p.ntn;
  const long long wgs = 2LL * num_cus();
  const unsigned grid = (unsigned)(ntiles < wgs ? ntiles : wgs);
  if (dtype == PFR_F32) hipLaunchKernelGGL(pairs_above_kernel<float>, dim3(grid), dim3(256), CL_LDS, stream, p);
  else if (dtype == PFR_BF16) hipLaunchKernelGGL(pairs_above_kernel<bf16_t>, dim3(grid), dim3(256), CL_LDS, stream, p);
  else hipLaunchKernelGGL(pairs_above_kernel<int8_t>, dim3(grid), dim3(256), CL_LDS, stream, p);
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
