// pfr_unionfind.h — the lock-free union-find of the clustering epilogues (pfr_cluster.hip, pfr_dbscan.hip): ONE definition of the find,
// the union and the loop cap.
//
// Union-find.  parent[x] <= x always: a root is the smallest id of its tree, a hook puts the larger root under the smaller, a path
// halving replaces a parent by the grandparent.  All three only ever lower an entry, so every walk strictly descends and the structure
// has no cycle at any instant, whatever the interleaving.  Every access is an agent-scope relaxed atomic (load or compare-exchange):
// the L2s of the XCDs are not coherent for plain stores, atomics execute at the memory side.  No ordering between different entries is
// needed: an entry read late is merely an older ancestor.  Every loop counts down a budget of 6 * n_nodes + 64 iterations and every
// value read from parent is range-checked before it is used as an index: a bug ends in *status != 0, not in a hang or a stray access.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#define UF_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ void uf_flag(int* status) { __hip_atomic_store(status, 1, UF_RLX_AGENT); }

// Root of x with path halving, at most `budget` iterations (counted down in place).  -1: budget spent or an entry outside [0, x].
__device__ __forceinline__ int uf_find(int* parent, int x, int& budget) {
  while (budget > 0) {
    --budget;
    const int p = __hip_atomic_load(parent + x, UF_RLX_AGENT);
    if (p == x) return x;
    if (p < 0 || p > x) return -1;
    const int gp = __hip_atomic_load(parent + p, UF_RLX_AGENT);
    if (gp < 0 || gp > p) return -1;
    if (gp != p) {
      int expect = p;   // halving: parent[x] = grandparent, unless somebody lowered it meanwhile (then theirs stands)
      __hip_atomic_compare_exchange_strong(parent + x, &expect, gp, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    x = gp;
  }
  return -1;
}

// Unites the trees of u and v (both in [0, n_nodes), u != v is not required) within `budget` = uf_budget(n_nodes) loop iterations.
// Why that is enough: S = (place of the u walk) + (place of the v walk) <= 2 (n - 1) at the start.  A find iteration that does not
// return lowers S, a failed hook lowers S (the value read back lies below the lost root), and each of the <= 1 + (failed hooks) rounds
// adds the two returning iterations: at most S + 2 (1 + S) < 6 n iterations in a correct forest.
static inline int uf_budget(int n_nodes) { return n_nodes < (INT_MAX - 64) / 6 ? 6 * n_nodes + 64 : INT_MAX; }

__device__ __forceinline__ void uf_union(int* parent, int u, int v, int budget, int* status) {
  while (true) {
    const int ru = uf_find(parent, u, budget);
    const int rv = ru < 0 ? -1 : uf_find(parent, v, budget);
    if (ru < 0 || rv < 0) { uf_flag(status); return; }
    if (ru == rv) return;
    const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    int expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    // hi is no root any more: `expect` is its new parent (below hi); go on from there
    if (expect < 0 || expect > hi || --budget <= 0) { uf_flag(status); return; }
    u = expect;
    v = lo;
  }
}
