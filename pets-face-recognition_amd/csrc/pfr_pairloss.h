// pfr_pairloss.h — what the pair-loss kernels on the batch (pfr_pairloss.hip) and the ones with a cross-batch memory (pfr_pairmem.hip)
// share: the operand fragment load, the logit of a pair, the merge of two online (max, sum) states, the gradient weight and the
// argument check.  The contract is the comment at pfr_pair_loss_fwd in include/pfr_hip.h.
#pragma once
#include "pfr_common.h"
#include "pfr_mma.h"

#define PL_SUPCON 0
#define PL_CIRCLE 1
#define PL_NSTAT 7   // per-anchor running state: m1, s1, m2, s2, sum of positive logits, |P|, |N|

// 16 bytes of row `row` at byte offset `boff`; zeros (and an in-range address) where the row or the offset is outside the matrix
__device__ __forceinline__ u32x4 pl_frag(const char* xn, int row, int rows, int rowbytes, int boff) {
  const bool ok = row < rows && boff < rowbytes;
  u32x4 v = ld16(xn + (size_t)min(row, rows - 1) * rowbytes + (ok ? boff : 0));
  if (!ok) v = u32x4{0u, 0u, 0u, 0u};
  return v;
}

// the logit of a pair and the factor d logit / d s that the gradient uses (circle: alpha is a constant there).  The last product is
// rounded on its own (__fmul_rn: no contraction into the caller's x - lse), so that the forward and the backward see the same logit bits
// and exp(x - lse) of a lone element is exactly 1
template <int KIND>
__device__ __forceinline__ void pl_logit(float s, bool same, float p0, float p1, float& x, float& slope) {
  if constexpr (KIND == PL_SUPCON) {      // p0 = 1 / tau
    x = __fmul_rn(s, p0);
    slope = p0;
  } else {                                // p0 = m, p1 = gamma
    if (same) {
      const float a = fmaxf(0.f, 1.f + p0 - s);
      slope = -p1 * a;
      x = __fmul_rn(slope, s - (1.f - p0));
    } else {
      const float a = fmaxf(0.f, s + p0);
      slope = p1 * a;
      x = __fmul_rn(slope, s - p0);
    }
  }
}

// (m, s) <- (m, s) merged with (m2, s2); an empty state is (-inf, 0) and stays NaN-free
__device__ __forceinline__ void pl_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  const float a = m == -INFINITY ? 0.f : s * expf(m - mn);
  const float b = m2 == -INFINITY ? 0.f : s2 * expf(m2 - mn);
  m = mn;
  s = a + b;
}

// W_ij * A (the factor 1 / A is in `scale`): anchor statistics st = {lse (supcon) | lse_p, 1 / |P| | lse_n, 1 | sigma(z), valid}
template <int KIND>
__device__ __forceinline__ float pl_weight(const f32x4& st, float x, float slope, bool same) {
  float w;
  if constexpr (KIND == PL_SUPCON) w = (expf(x - st[0]) - (same ? st[1] : 0.f)) * slope;
  else w = st[2] * expf(x - (same ? st[0] : st[1])) * slope;
  return st[3] != 0.f ? w : 0.f;
}

static inline int pl_check(const char* who, const void* xn, int dtype, const void* label, int B, int D, int kind, float p0, float p1) {
  PFR_CHECK_ARG(xn && label, "%s: null pointer", who);
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: the compute dtype is fp32 or bf16 (int8 is not supported)", who);
  PFR_CHECK_ARG(B >= 1 && B < (1 << 24), "%s: need 1 <= B < 2^24, got %d", who, B);
  PFR_CHECK_ARG(D >= 8 && D % 8 == 0 && D <= 1024, "%s: D must be a multiple of 8 in [8, 1024], got %d", who, D);
  PFR_CHECK_ARG(kind == PL_SUPCON || kind == PL_CIRCLE, "%s: kind must be 0 (supcon) or 1 (circle), got %d", who, kind);
  if (kind == PL_SUPCON) PFR_CHECK_ARG(p0 > 0.f, "%s: supcon needs a temperature > 0, got %g", who, (double)p0);
  else PFR_CHECK_ARG(p1 > 0.f && p0 >= 0.f && p0 < 1.f, "%s: circle needs gamma > 0 and 0 <= m < 1, got m=%g gamma=%g", who, (double)p0, (double)p1);
  return PFR_OK;
}
