// pfr_pairtile.h — the 128 x 128 score tile of the pair entry points (pfr_rank_count, pfr_pair_scores_gather, pfr_pairs_above,
// pfr_class_extremes; pfr_neighbor_count / pfr_dbscan_link use its k-loop, score and dtype check only): ONE definition of the operand block, the operand-row setup, the staging, the
// 128-byte k-steps, the MFMA sequence, the score expression, the valid-element mask and the host side every entry point shares, so that
// the entry points agree bit for bit on the same operand bits (an accumulator element depends on its two operand rows and the k order
// only).  The tile queue they walk is pfr_tilewalk.h.  pfr_pairhist.hip and pfr_cardmax.hip keep private copies of the walk and of the
// k-loop, pfr_dbscan.hip of the walk and the setup: converted to this header they gave the same results 3-4 % (dbscan: about 1 %)
// slower (profiles/pairtile_refactor.txt).
//
// A tile: 256 threads = 2 x 2 waves of 64 x 64 (2 x 2 accumulators of 32 x 32), 128-byte k-steps staged global -> registers -> swizzled
// LDS (the v2 operand layout of pfr_mma.h), the next k-step's global loads in flight under the MFMAs of the current one.  Wave (wp, wq)
// = (wave >> 1, wave & 1); accumulator register acc[i][j][r] of a lane is the element (wp * 64 + i * 32 + acc_row(r, lane),
// wq * 64 + j * 32 + (lane & 31)) of the tile, and bit (j * 2 + i) * 16 + r of the 64-bit lane masks below.
//
// The device functions are __forceinline__ and take plain values or references to register arrays: a parameter block passed by
// reference ends up on the stack.
#pragma once
#include "pfr_igemm.h"
#include "pfr_tilewalk.h"

// The score and what an epilogue does with it are separately rounded fp32 operations.  The build sets -ffp-contract=fast, which lets the
// backend fuse ANY multiply with a following add (no pragma and no __fmul_rn stops that: the int8 score's second product was seen
// contracted with the histogram bin rule's subtraction into one v_fma_f32).  rc_opaque hides a value's origin from the combiner: an
// empty asm statement, no instruction.
__device__ __forceinline__ float rc_opaque(float v) {
  asm("" : "+v"(v));
  return v;
}

#define RC_ROWB 128         // LDS operand row: one 128-byte k-step (KCH = 8)
#define RC_LDS_BASE (2 * RC_T * RC_ROWB + 2 * RC_T * 4)   // operand tiles + int8 scales: 33 792 bytes, under the default limit

// What every pair kernel is launched with: the two row sets (b == a in symmetric mode, aliased on the host), their int8 scales, the
// node offsets of the entry points that write per node, and the geometry of the walk.
struct PairOperands {
  const char* a;
  const char* b;
  const float* a_scale;
  const float* b_scale;
  int Na, Nb, sym;
  int a_off, b_off;
  int rowb;                 // bytes per operand row
  int ntm, ntn, nsn;        // (TileWalk)
  long long nsuper;
};

// the head of the dynamic LDS: ldsA [128][128 B], ldsB [128][128 B], scA [128], scB [128]; -> what follows (RC_LDS_BASE bytes in)
__device__ __forceinline__ char* rc_carve(char* smem, char*& ldsA, char*& ldsB, float*& scA, float*& scB) {
  ldsA = smem;
  ldsB = smem + RC_T * RC_ROWB;
  scA = reinterpret_cast<float*>(smem + 2 * RC_T * RC_ROWB);
  scB = scA + RC_T;
  return smem + RC_LDS_BASE;
}

// This thread's four operand row pointers (at its 16-byte chunk of k-step 0).  Operand rows of a ragged last tile are clamped to the
// last valid row (their scores are masked in the epilogue).
__device__ __forceinline__ void rc_operand_rows(const char* a, const char* b, int rowb, int row0, int col0, int Na, int Nb, int tid,
                                                const char* (&ga)[4], const char* (&gb)[4]) {
  const int lc = tid & 7, lr = tid >> 3;              // this thread's 16-byte chunk and first row of the staged k-step
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int ra = min(row0 + lr + 32 * u, Na - 1), rb = min(col0 + lr + 32 * u, Nb - 1);
    ga[u] = a + (size_t)ra * rowb + lc * 16;
    gb[u] = b + (size_t)rb * rowb + lc * 16;
  }
}

// stage the int8 scales of the tile's rows and columns (threads 0..127; clamped like the operands); part of a kernel's stage lambda
template <typename T>
__device__ __forceinline__ void rc_stage_scales(const float* a_scale, const float* b_scale, int row0, int col0, int Na, int Nb, int tid,
                                                float* scA, float* scB) {
  if constexpr (sizeof(T) == 1) {
    if (tid < RC_T) {
      scA[tid] = a_scale[min(row0 + tid, Na - 1)];
      scB[tid] = b_scale[min(col0 + tid, Nb - 1)];
    }
  }
}

// the score of the contract from an accumulator register
template <typename T> __device__ __forceinline__ float rc_score(float acc, float sa, float sb) {
  if constexpr (sizeof(T) == 1) return rc_opaque(((float)__float_as_int(acc) * sa) * sb);
  else return acc;
}

// One 128 x 128 tile product over the whole row: ga / gb are this thread's four operand row pointers (at its 16-byte chunk of k-step 0).
// `stage` runs once, between the two barriers of the first k-step (the previous tile's LDS reads are done, nothing of this tile's
// epilogue has started): what it stages is behind the second barrier, and the next tile's first barrier keeps it until every wave has
// left this tile's epilogue.  do_mma == false (wave-uniform): the wave only stages.
template <typename T, typename Stage>
__device__ __forceinline__ void rc_tile_gemm(const char* (&ga)[4], const char* (&gb)[4], int nk, char* ldsA, char* ldsB, int tid,
                                             bool do_mma, f32x16 (&acc)[2][2], Stage stage) {
  const int lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int lc = tid & 7, lr = tid >> 3;
  u32x4 va[4], vb[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) { va[u] = ld16(ga[u]); vb[u] = ld16(gb[u]); }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  for (int ks = 0; ks < nk; ++ks) {
    __syncthreads();   // the previous k-step's (or tile's epilogue's) LDS reads are done
    if (ks == 0) stage();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = lr + 32 * u;
      const int off = r * RC_ROWB + ((lc ^ row_swizzle<8>(r)) << 4);
      st16(ldsA + off, va[u]);
      st16(ldsB + off, vb[u]);
    }
    __syncthreads();
    if (ks + 1 < nk) {
#pragma unroll
      for (int u = 0; u < 4; ++u) { va[u] = ld16(ga[u] + (ks + 1) * RC_ROWB); vb[u] = ld16(gb[u] + (ks + 1) * RC_ROWB); }
    }
    if (do_mma) mma_kstep_sw<T, 8, 2, 2>(ldsA + wp * 64 * RC_ROWB, ldsB + wq * 64 * RC_ROWB, lane, acc);
  }
}

// ---- which elements of a tile count
// diag: a tile on the diagonal of a symmetric walk keeps i < j only; full: no element of the tile is masked (block-uniform, both)
__device__ __forceinline__ bool rc_tile_diag(int sym, int tm, int tn) { return sym && tm == tn; }
__device__ __forceinline__ bool rc_tile_full(bool diag, int row0, int col0, int Na, int Nb) {
  return !diag && row0 + RC_T <= Na && col0 + RC_T <= Nb;
}
// element (gi, gj): inside both sets and, on a diagonal tile, above the diagonal.  An expression macro: as a bool-returning
// __forceinline__ function with this text, inside the threshold loop of pairs_above_kernel<float>, the kernel went from 168 to 207
// registers and from 3 waves per SIMD to 2 (measured with -Rpass-analysis=kernel-resource-usage; the cause was not looked for further).
#define RC_VALID(full, diag, gi, gj, Na, Nb) ((full) || ((gi) < (Na) && (gj) < (Nb) && (!(diag) || (gi) < (gj))))

// the lane's 64-bit mask of valid accumulator registers
__device__ __forceinline__ unsigned long long rc_valid_mask(bool full, bool diag, int row0, int col0, int Na, int Nb, int wp, int wq,
                                                            int lane) {
  unsigned long long ok = 0ull;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gj = col0 + wq * 64 + j * 32 + (lane & 31);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gi = row0 + wp * 64 + i * 32 + acc_row(r, lane);
        if (RC_VALID(full, diag, gi, gj, Na, Nb)) ok |= 1ull << ((j * 2 + i) * 16 + r);
      }
    }
  }
  return ok;
}

// ---- host side
static inline int rc_check_operands(const char* who, int dtype, int D, int* esz) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16 || dtype == PFR_I8, "%s: bad dtype %d", who, dtype);
  *esz = dtype == PFR_F32 ? 4 : (dtype == PFR_BF16 ? 2 : 1);
  if (dtype == PFR_I8)
    PFR_CHECK_ARG(D > 0 && D % 128 == 0 && D <= 1040, "%s: int8 rows need Dp %% 128 == 0 and Dp <= 1040 (exact int32 -> float), got %d", who, D);
  else
    PFR_CHECK_ARG(D > 0 && D % (128 / *esz) == 0 && D <= 65536, "%s: D=%d must be a multiple of %d (128-byte k-steps)", who, D, 128 / *esz);
  return PFR_OK;
}

// First half of an entry point: the dtype / D check and the operand block with the symmetric aliasing done (b == nullptr: one set
// against itself, o->b / b_scale / Nb / b_off are a's).  The entry's own checks follow and read the aliased values from *o.
static inline int rc_operands(const char* who, const void* a, const float* a_scale, int Na, int a_off, const void* b,
                              const float* b_scale, int Nb, int b_off, int dtype, int D, PairOperands* o) {
  int esz = 0;
  if (int rc = rc_check_operands(who, dtype, D, &esz)) return rc;
  const bool sym = b == nullptr;
  *o = PairOperands{};
  o->a = static_cast<const char*>(a); o->b = sym ? o->a : static_cast<const char*>(b);
  o->a_scale = a_scale; o->b_scale = sym ? a_scale : b_scale;
  o->Na = Na; o->Nb = sym ? Na : Nb; o->sym = sym ? 1 : 0;
  o->a_off = a_off; o->b_off = sym ? a_off : b_off;
  o->rowb = D * esz;
  return PFR_OK;
}

// Second half: *grid = 0 and PFR_OK when there is no pair (nothing to launch); else the null / scale / device-pointer checks of the
// operands and of the entry's other pointers (`others`; others_ok: the required ones are there), the walk's geometry and the grid of
// persistent workgroups, wg_per_cu per compute unit.
static inline int rc_ready(const char* who, PairOperands* o, int dtype, std::initializer_list<const void*> others, bool others_ok,
                           int wg_per_cu, unsigned* grid) {
  *grid = 0;
  if (o->Na == 0 || o->Nb == 0 || (o->sym && o->Na == 1)) return PFR_OK;   // no pair
  PFR_CHECK_ARG(o->a && o->b && others_ok, "%s: null pointer", who);
  PFR_CHECK_ARG(dtype != PFR_I8 || (o->a_scale && o->b_scale), "%s: int8 rows need their scales", who);
  PFR_CHECK_ARG(pfr_all_dev({o->a, o->b, o->a_scale, o->b_scale}) && pfr_all_dev(others), "%s: every pointer must be device memory", who);
  const TileWalk w = tw_from_rows(o->Na, o->Nb, o->sym != 0);
  o->ntm = w.ntm; o->ntn = w.ntn; o->nsn = w.nsn; o->nsuper = w.nsuper;
  *grid = tw_grid(tw_ntiles(w, o->sym != 0), wg_per_cu, num_cus());
  return PFR_OK;
}

// the three-dtype launch of kernel<T, ...>(p): 256 threads, `lds` bytes of dynamic LDS
#define RC_LAUNCH(dtype, grid, lds, stream, p, kernel, ...)                                                               \
  do {                                                                                                                    \
    if ((dtype) == PFR_F32) hipLaunchKernelGGL((kernel<float, ##__VA_ARGS__>), dim3(grid), dim3(256), lds, stream, p);      \
    else if ((dtype) == PFR_BF16) hipLaunchKernelGGL((kernel<bf16_t, ##__VA_ARGS__>), dim3(grid), dim3(256), lds, stream, p); \
    else hipLaunchKernelGGL((kernel<int8_t, ##__VA_ARGS__>), dim3(grid), dim3(256), lds, stream, p);                        \
  } while (0)
