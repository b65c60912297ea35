// pfr_extremes.hip — open-set identification on the match GEMM: per node the BEST MATE (highest same-class score), the BEST IMPOSTOR
// (highest other-class score) and the WEAKEST MATE (lowest same-class score), each with its partner, as 64-bit atomic-max keys
// (pfr_class_extremes), and their decoding (pfr_extremes_decode); contract in include/pfr_hip.h.  Nothing N x N is written.
//
// Schedule and tile product: the tile queue of pfr_tilewalk.h (2 persistent workgroups per CU) and rc_tile_gemm / rc_score of
// pfr_pairtile.h, so a score has the bits of pfr_pair_scores_gather.  Next to the int8 scales the tile stages, per row and per column,
// the class id (a negative class becomes a value no other side can equal) and the FILTER value: the score of the node's current
// best_neg key, read once per tile with an agent-scope relaxed load (-inf while the key is 0).  Keys only grow, so a stale value only
// lets too much through.
//
// Epilogue, per wave (its 64 x 64 part of the tile):
//   1. Two lane masks (bit (j * 2 + i) * 16 + r <-> acc[i][j][r]): mN, the scores that reach the filter value of their row or of their
//      column (a NaN reaches nothing), and mM, the mate pairs.  Mate pairs are NOT filtered: they are few (classes are small against the
//      set) and feed two kinds.  ONE wave vote ends the wave when both masks are empty everywhere — the common case after the first tiles.
//   2. Otherwise the registers are walked unrolled; a register nobody kept costs one vote.  For a kept register the lane builds the keys
//      of its two columns; ROWS: the 32 lanes of a half share acc_row(r, lane), so a five-step butterfly of 64-bit maxima leaves the
//      row's key in every lane of the half and lane l collects the key of local row l; COLUMNS: the lane's running maximum over its 32
//      registers, then the maximum with the lane 32 away, lane l owns local column l.  The wave then issues at most one atomic-max
//      instruction per kind for its rows and one for its columns: one atomic per touched row or column, per kind, per wave and tile.
// Correctness rests on neither step: the maximum is idempotent and commutative, the filter and the reduction only remove atomics that
// could not change the result.
#include <climits>
#include "pfr_pairtile.h"
#include "pfr_scorekey.h"

#define EX_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define EX_LDS (RC_LDS_BASE + 4 * RC_T * 4)   // operands, scales, classes, filter values: 35 840 bytes, under the default limit

typedef unsigned long long ex_u64;

struct ExtremesParams {
  PairOperands o;
  const int* cls_a;
  const int* cls_b;
  int cols;                 // the column side has outputs (symmetric mode or both_sides)
  ex_u64* best_pos;
  ex_u64* best_neg;
  ex_u64* worst_pos;        // may be null
};

// the filter value of a node: the score its best_neg key holds now (-inf: no key yet, or a key that holds no number)
__device__ __forceinline__ float ex_filter(const ex_u64* key) {
  const ex_u64 k = __hip_atomic_load(const_cast<ex_u64*>(key), EX_RLX_AGENT);
  const float f = db_key_score((unsigned int)(k >> 32));
  return (k == 0ull || f != f) ? -INFINITY : f;
}

__device__ __forceinline__ ex_u64 ex_max(ex_u64 x, ex_u64 y) { return x > y ? x : y; }

// the maximum over the 32 lanes of each wave half, in every lane of the half
__device__ __forceinline__ ex_u64 ex_half_max(ex_u64 k) {
#pragma unroll
  for (int m = 1; m < 32; m <<= 1) k = ex_max(k, (ex_u64)__shfl_xor(k, m, 64));
  return k;
}

template <typename T>
__global__ __launch_bounds__(256, 2) void class_extremes_kernel(const ExtremesParams p) {   // (2 workgroups per CU: at most 256 registers)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *ldsA, *ldsB;
  float *scA, *scB;
  int* clsA = reinterpret_cast<int*>(rc_carve(smem, ldsA, ldsB, scA, scB));
  int* clsB = clsA + RC_T;
  float* tnA = reinterpret_cast<float*>(clsB + RC_T);
  float* tnB = tnA + RC_T;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int nk = p.o.rowb / RC_ROWB;
  const bool worst = p.worst_pos != nullptr;
  const long long total = p.o.nsuper * (RC_SUPER * RC_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    int tm, tn;
    if (!tw_tile(t, p.o.ntm, p.o.ntn, p.o.nsn, p.o.sym, tm, tn)) continue;   // (block-uniform)
    const int row0 = tm * RC_T, col0 = tn * RC_T;
    const char* ga[4];
    const char* gb[4];
    rc_operand_rows(p.o.a, p.o.b, p.o.rowb, row0, col0, p.o.Na, p.o.Nb, tid, ga, gb);
    // what this thread stages: threads 0..127 the tile's rows, threads 128..255 its columns (clamped like the operands: every index is
    // inside its set); scA | scB, clsA | clsB and tnA | tnB are contiguous, so the slot is [tid] of the first.  Plain values, captured by
    // value: a capture by reference of the parameter block would put it on the stack.
    const bool st_rows = tid < RC_T;
    const int st_r = st_rows ? min(row0 + tid, p.o.Na - 1) : min(col0 + tid - RC_T, p.o.Nb - 1);
    const int* st_cls = st_rows ? p.cls_a : p.cls_b;
    const float* st_scale = st_rows ? p.o.a_scale : p.o.b_scale;
    const ex_u64* st_key = p.best_neg + ((st_rows ? p.o.a_off : p.o.b_off) + st_r);
    const bool st_filter = st_rows || p.cols != 0;    // (no output on the column side: nothing reaches its filter value)
    const int st_neg = st_rows ? INT_MIN : INT_MIN + 1;   // a distractor row equals no column, a distractor column no row
    f32x16 acc[2][2];
    rc_tile_gemm<T>(ga, gb, nk, ldsA, ldsB, tid, true, acc, [=] {
      if constexpr (sizeof(T) == 1) scA[tid] = st_scale[st_r];
      const int c = st_cls[st_r];
      clsA[tid] = c < 0 ? st_neg : c;
      tnA[tid] = st_filter ? ex_filter(st_key) : INFINITY;
    });
    // (the staged values are behind the second barrier of the first k-step; the next tile's first barrier keeps them until every wave
    //  has left this epilogue)

    // ---- 1. the lanes' masks: bit (j * 2 + i) * 16 + r <-> acc[i][j][r]
    const bool diag = rc_tile_diag(p.o.sym, tm, tn);
    const bool full = rc_tile_full(diag, row0, col0, p.o.Na, p.o.Nb);
    const int cl0 = wq * 64 + (lane & 31), cl1 = cl0 + 32;
    const int cb0 = clsB[cl0], cb1 = clsB[cl1];
    const float tc0 = tnB[cl0], tc1 = tnB[cl1];
    float sb0 = 0.f, sb1 = 0.f;
    if constexpr (sizeof(T) == 1) { sb0 = scB[cl0]; sb1 = scB[cl1]; }
    ex_u64 mN = 0ull, mM = 0ull;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        // registers r = 4 q .. 4 q + 3 are four consecutive rows: one 16-byte LDS read per staged array
        const int base = wp * 64 + i * 32 + 8 * q + 4 * (lane >> 5);
        const int4 c4 = *reinterpret_cast<const int4*>(clsA + base);
        const float4 t4 = *reinterpret_cast<const float4*>(tnA + base);
        const int ca[4] = {c4.x, c4.y, c4.z, c4.w};
        const float tr[4] = {t4.x, t4.y, t4.z, t4.w};
        float sa[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (sizeof(T) == 1) {
          const float4 s4 = *reinterpret_cast<const float4*>(scA + base);
          sa[0] = s4.x; sa[1] = s4.y; sa[2] = s4.z; sa[3] = s4.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * q + e;
          const float s0 = rc_score<T>(acc[i][0][r], sa[e], sb0), s1 = rc_score<T>(acc[i][1][r], sa[e], sb1);
          if (s0 >= tr[e] || s0 >= tc0) mN |= 1ull << (i * 16 + r);
          if (s1 >= tr[e] || s1 >= tc1) mN |= 1ull << ((2 + i) * 16 + r);
          if (ca[e] == cb0) mM |= 1ull << (i * 16 + r);
          if (ca[e] == cb1) mM |= 1ull << ((2 + i) * 16 + r);
        }
      }
    }
    if (!full) {   // (block-uniform) a ragged or diagonal tile: drop what is outside the sets, the diagonal and the lower triangle
      const ex_u64 ok = rc_valid_mask(false, diag, row0, col0, p.o.Na, p.o.Nb, wp, wq, lane);
      mN &= ok;
      mM &= ok;
    }
    if (__ballot((mN | mM) != 0ull) == 0ull) continue;   // (wave-uniform; the epilogue holds no barrier)

    // ---- 2. keys of the kept registers, reduced inside the wave.  Lane l collects local row l (rP, rN, rW) and, at the end, local
    // column l; cX[j] is the lane's running maximum for its column of half j.
    ex_u64 rP = 0ull, rN = 0ull, rW = 0ull;
    ex_u64 cP[2] = {0ull, 0ull}, cN[2] = {0ull, 0ull}, cW[2] = {0ull, 0ull};
    const int ubase = p.o.a_off + row0 + wp * 64, vbase = p.o.b_off + col0 + wq * 64;
    // (the lane id behind an empty statement the compiler may not move: what step 2 derives from it — 64 lane comparisons, the row
    //  offsets — is otherwise computed once before the tile loop and kept in registers across the GEMM, which spilled)
    int ln = lane;
    asm volatile("" : "+v"(ln));
    // bit k = i * 16 + r of word j <-> acc[i][j][r]
    const unsigned int keep[2] = {(unsigned int)(mN | mM), (unsigned int)((mN | mM) >> 32)};
    const unsigned int mate[2] = {(unsigned int)mM, (unsigned int)(mM >> 32)};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = i * 16 + r;
        if (__ballot((((keep[0] | keep[1]) >> k) & 1u) != 0u) == 0ull) continue;   // (wave-uniform: nobody kept this register)
        const int rl = i * 32 + acc_row(r, ln);
        const int u = ubase + rl;                     // (< n_nodes where a bit is set: a set bit is a valid row and a valid column)
        float sa = 0.f;
        if constexpr (sizeof(T) == 1) sa = scA[wp * 64 + rl];
        ex_u64 kP = 0ull, kN = 0ull, kW = 0ull;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (!((keep[j] >> k) & 1u)) continue;
          const float s = rc_score<T>(acc[i][j][r], sa, j ? sb1 : sb0);
          if (!(s == s)) continue;                    // a NaN score updates nothing
          const unsigned int o = db_score_key(s);
          const int v = vbase + j * 32 + (ln & 31);
          if ((mate[j] >> k) & 1u) {
            kP = ex_max(kP, db_pack_key(o, v));
            cP[j] = ex_max(cP[j], db_pack_key(o, u));
            if (worst) {
              kW = ex_max(kW, db_pack_key(~o, v));
              cW[j] = ex_max(cW[j], db_pack_key(~o, u));
            }
          } else {
            kN = ex_max(kN, db_pack_key(o, v));
            cN[j] = ex_max(cN[j], db_pack_key(o, u));
          }
        }
        // rows: lanes 0..31 share local row R, lanes 32..63 local row R + 4 (a kind nobody has a key for costs one vote)
        const int R = i * 32 + acc_row(r, 0);
        if (__ballot(kP != 0ull) != 0ull) {
          kP = ex_half_max(kP);
          const ex_u64 lo = __shfl(kP, 0, 64), hi = __shfl(kP, 32, 64);
          if (ln == R) rP = lo;
          if (ln == R + 4) rP = hi;
        }
        if (__ballot(kN != 0ull) != 0ull) {
          kN = ex_half_max(kN);
          const ex_u64 lo = __shfl(kN, 0, 64), hi = __shfl(kN, 32, 64);
          if (ln == R) rN = lo;
          if (ln == R + 4) rN = hi;
        }
        if (__ballot(kW != 0ull) != 0ull) {
          kW = ex_half_max(kW);
          const ex_u64 lo = __shfl(kW, 0, 64), hi = __shfl(kW, 32, 64);
          if (ln == R) rW = lo;
          if (ln == R + 4) rW = hi;
        }
      }
    }
    // one atomic maximum per touched row and kind (a non-zero key means a valid element: the node is below its set's size, and
    // a_off + Na <= n_nodes is checked on the host)
    if (rP != 0ull) __hip_atomic_fetch_max(p.best_pos + (ubase + lane), rP, EX_RLX_AGENT);
    if (rN != 0ull) __hip_atomic_fetch_max(p.best_neg + (ubase + lane), rN, EX_RLX_AGENT);
    if (rW != 0ull) __hip_atomic_fetch_max(p.worst_pos + (ubase + lane), rW, EX_RLX_AGENT);   // (non-zero only with worst_pos)
    if (p.cols) {
      // columns: the lane 32 away holds the other 32 rows of the same columns; lane l then owns local column l = 32 j + (l & 31)
      // (b_off + Nb <= n_nodes is checked on the host when this side is written)
      const ex_u64 p0 = ex_max(cP[0], (ex_u64)__shfl_xor(cP[0], 32, 64)), p1 = ex_max(cP[1], (ex_u64)__shfl_xor(cP[1], 32, 64));
      const ex_u64 n0 = ex_max(cN[0], (ex_u64)__shfl_xor(cN[0], 32, 64)), n1 = ex_max(cN[1], (ex_u64)__shfl_xor(cN[1], 32, 64));
      const ex_u64 kp = lane < 32 ? p0 : p1, kn = lane < 32 ? n0 : n1;
      if (kp != 0ull) __hip_atomic_fetch_max(p.best_pos + (vbase + lane), kp, EX_RLX_AGENT);
      if (kn != 0ull) __hip_atomic_fetch_max(p.best_neg + (vbase + lane), kn, EX_RLX_AGENT);
      if (worst) {
        const ex_u64 w0 = ex_max(cW[0], (ex_u64)__shfl_xor(cW[0], 32, 64)), w1 = ex_max(cW[1], (ex_u64)__shfl_xor(cW[1], 32, 64));
        const ex_u64 kw = lane < 32 ? w0 : w1;
        if (kw != 0ull) __hip_atomic_fetch_max(p.worst_pos + (vbase + lane), kw, EX_RLX_AGENT);
      }
    }
  }
}

// One thread per key.  kind 0: a max-key; kind 1: a min-key (the stored ord is complemented).  Key 0, or a key whose partner would be
// 2^31 or more, is "no such pair": index -1, score -inf (kind 0) or +inf (kind 1).
__global__ __launch_bounds__(256) void extremes_decode_kernel(const ex_u64* keys, int n, int kind, float* score, int* index) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  const ex_u64 key = keys[x];
  const unsigned int partner = 0xffffffffu - (unsigned int)key;
  if (key == 0ull || partner >= 0x80000000u) {
    score[x] = kind ? INFINITY : -INFINITY;
    index[x] = -1;
    return;
  }
  const unsigned int o = (unsigned int)(key >> 32);
  score[x] = db_key_score(kind ? ~o : o);
  index[x] = (int)partner;
}

extern "C" int pfr_class_extremes(const void* a, const float* a_scale, int Na, int a_off, const void* b, const float* b_scale, int Nb,
                                  int b_off, int dtype, int D, const int* cls_a, const int* cls_b, int both_sides,
                                  unsigned long long* best_pos, unsigned long long* best_neg, unsigned long long* worst_pos, int n_nodes,
                                  hipStream_t stream) {
  const char* who = "pfr_class_extremes";
  ExtremesParams p{};
  PairOperands& o = p.o;
  if (int rc = rc_operands(who, a, a_scale, Na, a_off, b, b_scale, Nb, b_off, dtype, D, &o)) return rc;
  if (o.sym) cls_b = cls_a;
  const bool cols = o.sym || both_sides != 0;
  PFR_CHECK_ARG(o.Na >= 0 && o.Nb >= 0 && n_nodes >= 0, "%s: negative size", who);
  PFR_CHECK_ARG(o.a_off >= 0 && o.b_off >= 0, "%s: negative offset", who);
  PFR_CHECK_ARG((long long)o.a_off + o.Na <= (long long)n_nodes, "%s: a_off + Na passes n_nodes=%d", who, n_nodes);
  PFR_CHECK_ARG(!cols || (long long)o.b_off + o.Nb <= (long long)n_nodes, "%s: b_off + Nb passes n_nodes=%d", who, n_nodes);
  PFR_CHECK_ARG((long long)o.b_off + o.Nb <= (long long)INT_MAX, "%s: b_off + Nb passes 2^31 - 1", who);
  unsigned grid = 0;
  if (int rc = rc_ready(who, &o, dtype, {cls_a, cls_b, best_pos, best_neg, worst_pos}, cls_a && cls_b && best_pos && best_neg, 2, &grid))
    return rc;
  if (grid == 0) return PFR_OK;   // no pair
  p.cls_a = cls_a; p.cls_b = cls_b;
  p.cols = cols ? 1 : 0;
  p.best_pos = best_pos; p.best_neg = best_neg; p.worst_pos = worst_pos;
  RC_LAUNCH(dtype, grid, EX_LDS, stream, p, class_extremes_kernel);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_extremes_decode(const unsigned long long* keys, int n, int kind, float* score, int* index, hipStream_t stream) {
  const char* who = "pfr_extremes_decode";
  PFR_CHECK_ARG(n >= 0, "%s: negative size", who);
  PFR_CHECK_ARG(kind == 0 || kind == 1, "%s: kind=%d must be 0 (max-key) or 1 (min-key)", who, kind);
  if (n == 0) return PFR_OK;
  PFR_CHECK_ARG(keys && score && index, "%s: null pointer", who);
  PFR_CHECK_ARG(pfr_all_dev({keys, score, index}), "%s: every pointer must be device memory", who);
  hipLaunchKernelGGL(extremes_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, keys, n, kind, score, index);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
