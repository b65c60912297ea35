// pfr_pairtile.h — the 128 x 128 score tile of the pair entry points (pfr_rank_count, pfr_pair_scores_gather, pfr_pairs_above): ONE
// definition of the staging, the 128-byte k-steps, the MFMA sequence and the score expression, so that the entry points that include it
// agree bit for bit on the same operand bits (an accumulator element depends on its two operand rows and the k order only).
#pragma once
#include "pfr_igemm.h"

// see ph_opaque (pfr_pairhist.hip): keeps -ffp-contract=fast from fusing the int8 score's second product into whatever follows
__device__ __forceinline__ float rc_opaque(float v) {
  asm("" : "+v"(v));
  return v;
}

#define RC_T 128            // tile rows / columns
#define RC_SUPER 16         // super-tile edge in tiles
#define RC_ROWB 128         // LDS operand row: one 128-byte k-step (KCH = 8)

// the score of the contract from an accumulator register
template <typename T> __device__ __forceinline__ float rc_score(float acc, float sa, float sb) {
  if constexpr (sizeof(T) == 1) return rc_opaque(((float)__float_as_int(acc) * sa) * sb);
  else return acc;
}

// One 128 x 128 tile product over the whole row: ga / gb are this thread's four operand row pointers (at its 16-byte chunk of k-step 0).
// `stage` runs once, between the two barriers of the first k-step (the previous tile's LDS reads are done, nothing of this tile's
// epilogue has started).  do_mma == false (wave-uniform): the wave only stages.
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

static inline int rc_check_operands(const char* who, int dtype, int D, int* esz) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16 || dtype == PFR_I8, "%s: bad dtype %d", who, dtype);
  *esz = dtype == PFR_F32 ? 4 : (dtype == PFR_BF16 ? 2 : 1);
  if (dtype == PFR_I8)
    PFR_CHECK_ARG(D > 0 && D % 128 == 0 && D <= 1040, "%s: int8 rows need Dp %% 128 == 0 and Dp <= 1040 (exact int32 -> float), got %d", who, D);
  else
    PFR_CHECK_ARG(D > 0 && D % (128 / *esz) == 0 && D <= 65536, "%s: D=%d must be a multiple of %d (128-byte k-steps)", who, D, 128 / *esz);
  return PFR_OK;
}
