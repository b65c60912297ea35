// pfr_mha.hip — fused multi-head self-attention over the WHOLE token sequence (Vision Transformer), forward and backward, and the
// small token kernels of the ViT engine (class token + position embedding, class-token row gather / scatter).
//
// qkv [B][S][3·heads·64] (q | k | v, each (head, d): the row layout of nn.MultiheadAttention's in_proj and of pfr_window_attn_*),
// out [B][S][heads·64], lse fp32 [B][heads][S].  head_dim = 64, 1 <= S <= 257 (pfr_mha_supported).  The B·heads·S² scores never reach
// memory.
//
// bf16 (the hot path): ONE workgroup per (batch, head).  The head's K and V rows (backward: Q, K, V and dO) are staged in LDS once,
// rows S … Sp−1 (Sp = S rounded up to the 32-key tile) ZERO-FILLED — never read from what follows in memory, which is the next batch
// element — as two [Sp][32 d] sub-panels per operand in the 64-byte-row, XOR-swizzled layout of the window-attention kernels
// (pfr_swin.hip: conflict free for the ds_read_b128 row fragments and the transposing ds_read_b64_tr_b16 fragments alike).  Products
// are v_mfma_f32_32x32x16_bf16 in the orientation of those kernels: an accumulator holds its COLUMN on the lane (lane & 31) and its
// rows in the 16 registers, so a score tile is already the B operand of the product that sums over its rows — no shuffles, no LDS
// round trip — and the per-column softmax statistics are one scalar per lane.
//   forward:  a wave owns 64 query rows (two column halves sharing every K / V fragment) and walks the key tiles with a running
//             maximum and sum (flash form: the rescale of Oᵀ is one multiply per register with the lane's own factor); padding key
//             rows get −inf before the maximum; P is rounded to bf16 for P·V; the division by the sum comes last.
//   backward: recompute form, P = exp(s·scale − lse), D = rowsum(dO ∘ O).  Phase A (a wave owns 32 queries, walks the keys):
//             dQ = dS·K·scale.  Phase B (a wave owns 32 keys, walks the queries, scores in the transposed orientation so that the
//             reduction index — the queries — is again the register index): dV = Pᵀ·dO, dK = dSᵀ·Q·scale.  Every output row is
//             complete inside its wave: no atomics, no second pass, bit-reproducible.  S and dP are computed in both phases (28
//             instead of 20 MFMAs per 32x32 tile pair) — the price of keeping the reduction off the lanes in both.
// fp32 (the parity gate): plain FMA kernels, one wave per output row, scores of the row in registers / per-wave LDS.
// Rows at or beyond S are never stored.
#include "pfr_common.h"
#include <math.h>

typedef short mha_s16x4 __attribute__((ext_vector_type(4)));

#define MHA_HD 64
#define MHA_MAXS 257
#define MHA_RS 64      // bytes per row of a [Sp][32 d] bf16 sub-panel
#define MHA_MAXC 5     // 64-key chunks of the fp32 kernels: ceil(MHA_MAXS / 64)

static inline int mha_sp(int S) { return (S + 31) / 32 * 32; }

extern "C" int pfr_mha_supported(int dtype, int S, int heads, int head_dim) {
  return (dtype == PFR_F32 || dtype == PFR_BF16) && head_dim == MHA_HD && S >= 1 && S <= MHA_MAXS && heads >= 1 && heads <= 1024;
}

// ------------------------------------------------------------------------------------------------ bf16 fragments
__device__ __forceinline__ int mha_swz(int row, int chunk) { return chunk ^ ((row >> 2) & 3); }
__device__ __forceinline__ int mha_accrow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// operand with the reduction over d: row (token) = 32·tile + lane&31, d = 32·(ks4>>1) + 16·(ks4&1) + 8·(lane>>5) … +7
__device__ __forceinline__ bf16x8 mha_rowfrag(const char* pan, int Sp, int tile, int ks4, int lane) {
  const int row = (lane & 31) + 32 * tile;
  const char* sub = pan + (size_t)(ks4 >> 1) * Sp * MHA_RS;
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(sub + row * MHA_RS + mha_swz(row, 2 * (ks4 & 1) + (lane >> 5)) * 16));
}
// A operand [M = d (32 of sub-panel dt)][K = token] from the [token][d] sub-panel: reduction slot e ↔ token
// 32·tile + 16·t + 8·(e>>2) + 4·(lane>>5) + (e&3) — the accumulator-row order of mha_accfrag
__device__ __forceinline__ bf16x8 mha_trfrag(const char* pan, int Sp, int dt, int tile, int t, int lane) {
  const char* sub = pan + (size_t)dt * Sp * MHA_RS;
  const int g = lane >> 4, s4 = lane & 15;
  const int row = 32 * tile + 16 * t + (g >> 1) * 4 + (s4 >> 2), ch = 2 * (g & 1) + ((s4 & 3) >> 1), off = (s4 & 1) * 8;
  const char* a = sub + row * MHA_RS + mha_swz(row, ch) * 16 + off;
  const char* b = sub + (row + 8) * MHA_RS + mha_swz(row + 8, ch) * 16 + off;
  mha_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mha_s16x4 __attribute__((address_space(3)))*)(a));
  mha_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mha_s16x4 __attribute__((address_space(3)))*)(b));
  u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
  u32x4 u = {l2[0], l2[1], h2[0], h2[1]};
  return __builtin_bit_cast(bf16x8, u);
}
__device__ __forceinline__ bf16x8 mha_accfrag(const f32x16& v, int t) {   // accumulator rows 8t … 8t+7 → bf16 B operand
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (bf16_t)v[8 * t + e];
  return f;
}
__device__ __forceinline__ f32x16 mha_mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }

// rows 0 … S−1 of one operand (64 d = 128 bytes each, `rowstride` elements apart) into its two sub-panels; rows S … Sp−1 are zeros.
// Eight consecutive lanes read one row.  The load is unconditional from a clamped row of the SAME batch element, the zero a select.
__device__ __forceinline__ void mha_load_panel(char* pan, const bf16_t* base, size_t rowstride, int S, int Sp, int tid, int nthreads) {
  for (int idx = tid; idx < Sp * 8; idx += nthreads) {
    const int row = idx >> 3, c8 = idx & 7;
    u32x4 v = ld16(base + (size_t)min(row, S - 1) * rowstride + c8 * 8);
    if (row >= S) v = u32x4{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4*>(pan + (size_t)(c8 >> 2) * Sp * MHA_RS + row * MHA_RS + mha_swz(row, c8 & 3) * 16) = v;
  }
}
// a row fragment straight from memory (zeros for a row at or beyond S)
__device__ __forceinline__ bf16x8 mha_gfrag(const bf16_t* base, size_t rowstride, int row, int S, int ks4, int lane) {
  u32x4 v = ld16(base + (size_t)min(row, S - 1) * rowstride + 16 * ks4 + 8 * (lane >> 5));
  if (row >= S) v = u32x4{0u, 0u, 0u, 0u};
  return __builtin_bit_cast(bf16x8, v);
}
// Oᵀ-style accumulator (rows d = 32·dt + accrow, column = token on the lane) → 4 consecutive d per register quad, 8-byte stores
__device__ __forceinline__ void mha_store_acc(const f32x16& acc, float mul, bf16_t* rowptr, int dt, int lane) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    bf16x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (bf16_t)(acc[4 * g + e] * mul);
    *reinterpret_cast<bf16x4*>(rowptr + 32 * dt + 8 * g + 4 * (lane >> 5)) = v;
  }
}

// ------------------------------------------------------------------------------------------------ bf16 forward
#define MHA_FWD_WAVES 4
__global__ __launch_bounds__(MHA_FWD_WAVES * 64) void mha_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                                          float* __restrict__ lse, int S, int Sp, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) char mha_smem[];
  char* lk = mha_smem;
  char* lv = mha_smem + (size_t)Sp * 2 * MHA_RS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int C = heads * MHA_HD;
  const size_t rs = 3 * (size_t)C;
  const bf16_t* base = qkv + (size_t)b * S * rs + h * MHA_HD;
  mha_load_panel(lk, base + C, rs, S, Sp, tid, MHA_FWD_WAVES * 64);
  mha_load_panel(lv, base + 2 * C, rs, S, Sp, tid, MHA_FWD_WAVES * 64);
  __syncthreads();
  const int nkt = Sp >> 5, nqb = (S + 63) >> 6;
#pragma unroll 1
  for (int qb = wave; qb < nqb; qb += MHA_FWD_WAVES) {
    bf16x8 qf[2][4];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[qh][ks] = mha_gfrag(base, rs, 64 * qb + 32 * qh + (lane & 31), S, ks, lane);
    f32x16 oacc[2][2];
    float m[2], l[2];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      m[qh] = -INFINITY;
      l[qh] = 0.f;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[qh][dt][e] = 0.f;
    }
#pragma unroll 1
    for (int jt = 0; jt < nkt; ++jt) {
      f32x16 s[2];
#pragma unroll
      for (int qh = 0; qh < 2; ++qh)
#pragma unroll
        for (int e = 0; e < 16; ++e) s[qh][e] = 0.f;
      // Sᵀ[j][i] = K·Qᵀ
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = mha_rowfrag(lk, Sp, jt, ks, lane);
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) s[qh] = mha_mfma(kf, qf[qh][ks], s[qh]);
      }
      const bool last = 32 * (jt + 1) > S;   // the only tile with padding keys (it always holds a real one: Sp − S < 32)
#pragma unroll
      for (int qh = 0; qh < 2; ++qh) {
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          float v = s[qh][e] * scale;
          if (last && 32 * jt + mha_accrow(e, lane) >= S) v = -INFINITY;
          s[qh][e] = v;
          mx = fmaxf(mx, v);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m[qh], mx);            // finite from the first tile on: key 0 is real
        const float alpha = __expf(m[qh] - mn);       // first tile: exp(−inf) = 0 on an all-zero accumulator
        float sum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pv = __expf(s[qh][e] - mn);
          s[qh][e] = pv;
          sum += pv;
        }
        sum += __shfl_xor(sum, 32, 64);
        l[qh] = fmaf(l[qh], alpha, sum);
        m[qh] = mn;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) oacc[qh][dt][e] *= alpha;
      }
      // Oᵀ[d][i] += Σ_j Vᵀ[d][j]·Pᵀ[j][i]
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 p0 = mha_accfrag(s[0], t), p1 = mha_accfrag(s[1], t);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const bf16x8 vf = mha_trfrag(lv, Sp, dt, jt, t, lane);
          oacc[0][dt] = mha_mfma(vf, p0, oacc[0][dt]);
          oacc[1][dt] = mha_mfma(vf, p1, oacc[1][dt]);
        }
      }
    }
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
      const int i = 64 * qb + 32 * qh + (lane & 31);
      if (i < S) {
        const float inv = 1.f / l[qh];
        bf16_t* orow = out + ((size_t)b * S + i) * C + h * MHA_HD;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) mha_store_acc(oacc[qh][dt], inv, orow, dt, lane);
        if (lse && lane < 32) lse[((size_t)b * heads + h) * S + i] = m[qh] + logf(l[qh]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ bf16 backward
#define MHA_BWD_WAVES 8
__global__ __launch_bounds__(MHA_BWD_WAVES * 64) void mha_bwd_bf16_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ out,
                                                                          const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                          bf16_t* __restrict__ dqkv, int S, int Sp, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) char mha_smem[];
  const size_t pb = (size_t)Sp * 2 * MHA_RS;
  char* lq = mha_smem;
  char* lk = lq + pb;
  char* lv = lk + pb;
  char* lg = lv + pb;
  float* lse_s = reinterpret_cast<float*>(lg + pb);   // [Sp]: +inf for padding rows (P = exp(s − inf) = 0)
  float* d_s = lse_s + Sp;                            // [Sp]: D = rowsum(dO ∘ O), 0 for padding rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int C = heads * MHA_HD;
  const size_t rs = 3 * (size_t)C;
  const bf16_t* base = qkv + (size_t)b * S * rs + h * MHA_HD;
  const bf16_t* gbase = dout + (size_t)b * S * C + h * MHA_HD;
  const bf16_t* obase = out + (size_t)b * S * C + h * MHA_HD;
  bf16_t* dbase = dqkv + (size_t)b * S * rs + h * MHA_HD;
  constexpr int NT = MHA_BWD_WAVES * 64;
  mha_load_panel(lq, base, rs, S, Sp, tid, NT);
  mha_load_panel(lk, base + C, rs, S, Sp, tid, NT);
  mha_load_panel(lv, base + 2 * C, rs, S, Sp, tid, NT);
  mha_load_panel(lg, gbase, (size_t)C, S, Sp, tid, NT);
  for (int i = tid; i < Sp; i += NT) {
    float dsum = 0.f, lv_ = INFINITY;
    if (i < S) {
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8) {
        float fo[8], fg[8];
        Chunk<bf16_t>::unpack(ld16(obase + (size_t)i * C + c8 * 8), fo);
        Chunk<bf16_t>::unpack(ld16(gbase + (size_t)i * C + c8 * 8), fg);
#pragma unroll
        for (int e = 0; e < 8; ++e) dsum = fmaf(fo[e], fg[e], dsum);
      }
      lv_ = lse[((size_t)b * heads + h) * S + i];
    }
    d_s[i] = dsum;
    lse_s[i] = lv_;
  }
  __syncthreads();
  const int nt = Sp >> 5;
  // ---- phase A: dQ.  Rows j = keys, columns i = queries (the forward's orientation)
#pragma unroll 1
  for (int it = wave; it < nt; it += MHA_BWD_WAVES) {
    const int i = 32 * it + (lane & 31);
    const float li = lse_s[i], di = d_s[i];
    bf16x8 qf[4], gf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qf[ks] = mha_rowfrag(lq, Sp, it, ks, lane);
      gf[ks] = mha_rowfrag(lg, Sp, it, ks, lane);
    }
    f32x16 dq[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) dq[dt][e] = 0.f;
#pragma unroll 1
    for (int jt = 0; jt < nt; ++jt) {
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mha_mfma(mha_rowfrag(lk, Sp, jt, ks, lane), qf[ks], s);      // Sᵀ = K·Qᵀ
        dp = mha_mfma(mha_rowfrag(lv, Sp, jt, ks, lane), gf[ks], dp);    // dPᵀ = V·dOᵀ
      }
      const bool last = 32 * (jt + 1) > S;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float pv = __expf(fmaf(s[e], scale, -li));
        if (last && 32 * jt + mha_accrow(e, lane) >= S) pv = 0.f;
        s[e] = pv * (dp[e] - di);                                        // dSᵀ = Pᵀ ∘ (dPᵀ − D_i)
      }
      // dQᵀ[d][i] += Σ_j Kᵀ[d][j]·dSᵀ[j][i]
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 df = mha_accfrag(s, t);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) dq[dt] = mha_mfma(mha_trfrag(lk, Sp, dt, jt, t, lane), df, dq[dt]);
      }
    }
    if (i < S) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) mha_store_acc(dq[dt], scale, dbase + (size_t)i * rs, dt, lane);
    }
  }
  // ---- phase B: dK, dV.  Rows i = queries, columns j = keys: the reduction index of both products is the register index
#pragma unroll 1
  for (int jt = wave; jt < nt; jt += MHA_BWD_WAVES) {
    const int j = 32 * jt + (lane & 31);
    const bool jok = j < S;
    bf16x8 kf[4], vf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      kf[ks] = mha_rowfrag(lk, Sp, jt, ks, lane);
      vf[ks] = mha_rowfrag(lv, Sp, jt, ks, lane);
    }
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 16; ++e) { dk[dt][e] = 0.f; dv[dt][e] = 0.f; }
#pragma unroll 1
    for (int it = 0; it < nt; ++it) {
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        s = mha_mfma(mha_rowfrag(lq, Sp, it, ks, lane), kf[ks], s);      // S = Q·Kᵀ
        dp = mha_mfma(mha_rowfrag(lg, Sp, it, ks, lane), vf[ks], dp);    // dP = dO·Vᵀ
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_s + 32 * it + 8 * g + 4 * (lane >> 5));
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(d_s + 32 * it + 8 * g + 4 * (lane >> 5));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pv = jok ? __expf(fmaf(s[4 * g + e], scale, -l4[e])) : 0.f;
          s[4 * g + e] = pv;
          dp[4 * g + e] = pv * (dp[4 * g + e] - d4[e]);
        }
      }
      // dVᵀ[d][j] += Σ_i dOᵀ[d][i]·P[i][j],  dKᵀ[d][j] += Σ_i Qᵀ[d][i]·dS[i][j]
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const bf16x8 pf = mha_accfrag(s, t), df = mha_accfrag(dp, t);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          dv[dt] = mha_mfma(mha_trfrag(lg, Sp, dt, it, t, lane), pf, dv[dt]);
          dk[dt] = mha_mfma(mha_trfrag(lq, Sp, dt, it, t, lane), df, dk[dt]);
        }
      }
    }
    if (jok) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        mha_store_acc(dk[dt], scale, dbase + (size_t)j * rs + C, dt, lane);
        mha_store_acc(dv[dt], 1.f, dbase + (size_t)j * rs + 2 * C, dt, lane);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ fp32 (parity gate)
// One wave per output row; lane = key (scores, 64-key chunks) and then lane = d (the 64 outputs of the row).
__device__ __forceinline__ float mha_dot64(const float* __restrict__ a_lds, const float* __restrict__ row) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < MHA_HD; d += 4) {
    const f32x4 k4 = *reinterpret_cast<const f32x4*>(row + d);
    acc = fmaf(a_lds[d], k4[0], acc);
    acc = fmaf(a_lds[d + 1], k4[1], acc);
    acc = fmaf(a_lds[d + 2], k4[2], acc);
    acc = fmaf(a_lds[d + 3], k4[3], acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void mha_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                          int S, int heads, float scale) {
  __shared__ __attribute__((aligned(16))) float qs[4][MHA_HD];
  __shared__ float ps[4][MHA_MAXC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int i = blockIdx.y * 4 + wave;
  const bool valid = i < S;
  const int C = heads * MHA_HD;
  const size_t rs = 3 * (size_t)C;
  const float* base = qkv + (size_t)b * S * rs + h * MHA_HD;
  qs[wave][lane] = base[(size_t)(valid ? i : S - 1) * rs + lane];
  __syncthreads();
  float s[MHA_MAXC];
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < MHA_MAXC; ++c) {
    const int j = lane + 64 * c;
    float v = -INFINITY;                               // padding key columns
    if (j < S) v = mha_dot64(qs[wave], base + C + (size_t)j * rs) * scale;
    s[c] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < MHA_MAXC; ++c) {
    const float pv = (lane + 64 * c < S) ? expf(s[c] - mx) : 0.f;
    ps[wave][lane + 64 * c] = pv;
    sum += pv;
  }
  sum = wave_sum(sum);
  __syncthreads();
  float o = 0.f;
  for (int j = 0; j < S; ++j) o = fmaf(ps[wave][j], base[2 * C + (size_t)j * rs + lane], o);
  if (valid) {
    out[((size_t)b * S + i) * C + h * MHA_HD + lane] = o / sum;
    if (lse && lane == 0) lse[((size_t)b * heads + h) * S + i] = mx + logf(sum);
  }
}

// dQ: one wave per query row
__global__ __launch_bounds__(256) void mha_bwd_q_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                            const float* __restrict__ dout, const float* __restrict__ lse,
                                                            float* __restrict__ dqkv, int S, int heads, float scale) {
  __shared__ __attribute__((aligned(16))) float qs[4][MHA_HD], gs[4][MHA_HD];
  __shared__ float ds[4][MHA_MAXC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int i = blockIdx.y * 4 + wave;
  const bool valid = i < S;
  const int ic = valid ? i : S - 1;
  const int C = heads * MHA_HD;
  const size_t rs = 3 * (size_t)C;
  const float* base = qkv + (size_t)b * S * rs + h * MHA_HD;
  const size_t orow = ((size_t)b * S + ic) * C + h * MHA_HD + lane;
  const float g = dout[orow];
  qs[wave][lane] = base[(size_t)ic * rs + lane];
  gs[wave][lane] = g;
  const float di = wave_sum(g * out[orow]);
  const float li = lse[((size_t)b * heads + h) * S + ic];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < MHA_MAXC; ++c) {
    const int j = lane + 64 * c;
    float v = 0.f;
    if (j < S) {
      const float sc = mha_dot64(qs[wave], base + C + (size_t)j * rs);
      const float dp = mha_dot64(gs[wave], base + 2 * C + (size_t)j * rs);
      v = expf(fmaf(sc, scale, -li)) * (dp - di);
    }
    ds[wave][j] = v;
  }
  __syncthreads();
  float dq = 0.f;
  for (int j = 0; j < S; ++j) dq = fmaf(ds[wave][j], base[C + (size_t)j * rs + lane], dq);
  if (valid) dqkv[((size_t)b * S + i) * rs + h * MHA_HD + lane] = dq * scale;
}

// dK, dV: one wave per key row
__global__ __launch_bounds__(256) void mha_bwd_kv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                             const float* __restrict__ dout, const float* __restrict__ lse,
                                                             float* __restrict__ dqkv, int S, int heads, float scale) {
  __shared__ __attribute__((aligned(16))) float ks[4][MHA_HD], vs[4][MHA_HD];
  __shared__ float ps[4][MHA_MAXC * 64], ds[4][MHA_MAXC * 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
  const int j = blockIdx.y * 4 + wave;
  const bool valid = j < S;
  const int jc = valid ? j : S - 1;
  const int C = heads * MHA_HD;
  const size_t rs = 3 * (size_t)C;
  const float* base = qkv + (size_t)b * S * rs + h * MHA_HD;
  const float* gbase = dout + (size_t)b * S * C + h * MHA_HD;
  const float* obase = out + (size_t)b * S * C + h * MHA_HD;
  ks[wave][lane] = base[C + (size_t)jc * rs + lane];
  vs[wave][lane] = base[2 * C + (size_t)jc * rs + lane];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < MHA_MAXC; ++c) {
    const int i = lane + 64 * c;
    float pv = 0.f, dv = 0.f;
    if (i < S) {
      const float* grow = gbase + (size_t)i * C;
      const float* orow = obase + (size_t)i * C;
      const float sc = mha_dot64(ks[wave], base + (size_t)i * rs);
      const float dp = mha_dot64(vs[wave], grow);
      float di = 0.f;
#pragma unroll
      for (int d = 0; d < MHA_HD; d += 4) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(grow + d), o4 = *reinterpret_cast<const f32x4*>(orow + d);
        di = fmaf(g4[0], o4[0], di); di = fmaf(g4[1], o4[1], di); di = fmaf(g4[2], o4[2], di); di = fmaf(g4[3], o4[3], di);
      }
      pv = expf(fmaf(sc, scale, -lse[((size_t)b * heads + h) * S + i]));
      dv = pv * (dp - di);
    }
    ps[wave][i] = pv;
    ds[wave][i] = dv;
  }
  __syncthreads();
  float dk = 0.f, dvv = 0.f;
  for (int i = 0; i < S; ++i) {
    dvv = fmaf(ps[wave][i], gbase[(size_t)i * C + lane], dvv);
    dk = fmaf(ds[wave][i], base[(size_t)i * rs + lane], dk);
  }
  if (valid) {
    dqkv[((size_t)b * S + j) * rs + C + h * MHA_HD + lane] = dk * scale;
    dqkv[((size_t)b * S + j) * rs + 2 * C + h * MHA_HD + lane] = dvv;
  }
}

// ------------------------------------------------------------------------------------------------ entry points
static int mha_check(const char* who, int dtype, int B, int S, int heads, int head_dim) {
  PFR_CHECK_ARG(pfr_mha_supported(dtype, S, heads, head_dim),
                "%s: unsupported shape (dtype %d, S %d, heads %d, head_dim %d): head_dim must be %d and 1 <= S <= %d", who, dtype, S, heads,
                head_dim, MHA_HD, MHA_MAXS);
  PFR_CHECK_ARG(B > 0 && (long)B * heads <= 0x7fffffffL, "%s: bad batch size %d", who, B);
  return PFR_OK;
}

extern "C" int pfr_mha_fwd(const void* qkv, void* out, float* lse, int dtype, int B, int S, int heads, int head_dim, float scale,
                           hipStream_t st) {
  if (int rc = mha_check("pfr_mha_fwd", dtype, B, S, heads, head_dim)) return rc;
  PFR_CHECK_ARG(qkv && out, "pfr_mha_fwd: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({qkv, out, lse}), "pfr_mha_fwd: not a device pointer");
  if (dtype == PFR_BF16) {
    const int Sp = mha_sp(S);
    const size_t lds = (size_t)Sp * 2 * MHA_RS * 2;
    static std::atomic<unsigned long long> attr{0};
    PFR_MAX_LDS_ONCE(attr, 160 * 1024, (const void*)mha_fwd_bf16_kernel);
    hipLaunchKernelGGL(mha_fwd_bf16_kernel, dim3((unsigned)(B * heads)), dim3(MHA_FWD_WAVES * 64), lds, st, (const bf16_t*)qkv, (bf16_t*)out,
                       lse, S, Sp, heads, scale);
  } else {
    hipLaunchKernelGGL(mha_fwd_f32_kernel, dim3((unsigned)(B * heads), (unsigned)((S + 3) / 4)), dim3(256), 0, st, (const float*)qkv,
                       (float*)out, lse, S, heads, scale);
  }
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_mha_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv, int dtype, int B, int S,
                           int heads, int head_dim, float scale, hipStream_t st) {
  if (int rc = mha_check("pfr_mha_bwd", dtype, B, S, heads, head_dim)) return rc;
  PFR_CHECK_ARG(qkv && out && dout && lse && dqkv, "pfr_mha_bwd: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({qkv, out, dout, lse, dqkv}), "pfr_mha_bwd: not a device pointer");
  if (dtype == PFR_BF16) {
    const int Sp = mha_sp(S);
    const size_t lds = (size_t)Sp * 2 * MHA_RS * 4 + (size_t)Sp * 8;
    static std::atomic<unsigned long long> attr{0};
    PFR_MAX_LDS_ONCE(attr, 160 * 1024, (const void*)mha_bwd_bf16_kernel);
    hipLaunchKernelGGL(mha_bwd_bf16_kernel, dim3((unsigned)(B * heads)), dim3(MHA_BWD_WAVES * 64), lds, st, (const bf16_t*)qkv,
                       (const bf16_t*)out, (const bf16_t*)dout, lse, (bf16_t*)dqkv, S, Sp, heads, scale);
  } else {
    const dim3 grid((unsigned)(B * heads), (unsigned)((S + 3) / 4));
    hipLaunchKernelGGL(mha_bwd_q_f32_kernel, grid, dim3(256), 0, st, (const float*)qkv, (const float*)out, (const float*)dout, lse,
                       (float*)dqkv, S, heads, scale);
    hipLaunchKernelGGL(mha_bwd_kv_f32_kernel, grid, dim3(256), 0, st, (const float*)qkv, (const float*)out, (const float*)dout, lse,
                       (float*)dqkv, S, heads, scale);
  }
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ------------------------------------------------------------------------------------------------ ViT token kernels
// tok[b][0] = class_token + pos[0];  tok[b][s] = patches[b][s−1] + pos[s]   (class_token / pos: the fp32 master parameters)
template <typename T>
__global__ void vit_tokens_fwd_kernel(const T* __restrict__ patches, const float* __restrict__ cls, const float* __restrict__ pos,
                                      T* __restrict__ tok, int B, int S, int D) {
  constexpr int KP = DT<T>::KPACK;
  const int dc = D / KP;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * S * dc) return;
  const int c = (int)(idx % dc);
  const int s = (int)((idx / dc) % S);
  const size_t b = idx / ((size_t)dc * S);
  float f[KP];
  if (s == 0) {
#pragma unroll
    for (int e = 0; e < KP; ++e) f[e] = cls[c * KP + e];
  } else {
    Chunk<T>::unpack(ld16(patches + (b * (S - 1) + (s - 1)) * D + c * KP), f);
  }
#pragma unroll
  for (int e = 0; e < KP; ++e) f[e] += pos[(size_t)s * D + c * KP + e];
  st16(tok + (b * S + s) * D + c * KP, Chunk<T>::pack(f));
}
// dpatches[b][s−1] = dtok[b][s];  dpos[s] = Σ_b dtok[b][s];  dcls = Σ_b dtok[b][0]   (sums over b in ascending order)
template <typename T>
__global__ void vit_tokens_bwd_kernel(const T* __restrict__ dtok, T* __restrict__ dpatches, float* __restrict__ dpos,
                                      float* __restrict__ dcls, int B, int S, int D) {
  constexpr int KP = DT<T>::KPACK;
  const int dc = D / KP;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= S * dc) return;
  const int c = idx % dc, s = idx / dc;
  float acc[KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) acc[e] = 0.f;
  for (size_t b = 0; b < (size_t)B; ++b) {
    const u32x4 v = ld16(dtok + (b * S + s) * D + c * KP);
    float f[KP];
    Chunk<T>::unpack(v, f);
#pragma unroll
    for (int e = 0; e < KP; ++e) acc[e] += f[e];
    if (s > 0) st16(dpatches + (b * (S - 1) + (s - 1)) * D + c * KP, v);
  }
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    dpos[(size_t)s * D + c * KP + e] = acc[e];
    if (s == 0) dcls[c * KP + e] = acc[e];
  }
}
// y[b] = x[b][0]
template <typename T>
__global__ void vit_cls_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int S, int D) {
  constexpr int KP = DT<T>::KPACK;
  const int dc = D / KP;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * dc) return;
  const size_t b = idx / dc;
  const int c = (int)(idx % dc);
  st16(y + b * D + c * KP, ld16(x + b * S * D + c * KP));
}
// dx[b][0] = dy[b], dx[b][s > 0] = 0
template <typename T>
__global__ void vit_cls_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int B, int S, int D) {
  constexpr int KP = DT<T>::KPACK;
  const int dc = D / KP;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * S * dc) return;
  const int c = (int)(idx % dc);
  const int s = (int)((idx / dc) % S);
  const size_t b = idx / ((size_t)dc * S);
  u32x4 v = {0u, 0u, 0u, 0u};
  if (s == 0) v = ld16(dy + b * D + c * KP);
  st16(dx + (b * S + s) * D + c * KP, v);
}

static int vit_check(const char* who, int dtype, int B, int S, int D) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", who);
  PFR_CHECK_ARG(B > 0 && S >= 1 && D > 0 && D % (dtype == PFR_BF16 ? 8 : 4) == 0, "%s: bad shape (B %d, S %d, D %d; D must be a multiple of %d)",
                who, B, S, D, dtype == PFR_BF16 ? 8 : 4);
  PFR_CHECK_ARG((size_t)B * S * (D / 4) < 0x7fffffffull * 256, "%s: tensor too large", who);
  return PFR_OK;
}
#define VIT_LAUNCH(KERNEL, TT, n, ...)                                                                                        \
  do {                                                                                                                        \
    hipLaunchKernelGGL(KERNEL<TT>, dim3((unsigned)(((n) + 255) / 256)), dim3(256), 0, st, __VA_ARGS__);                       \
    PFR_CHECK_LAUNCH();                                                                                                       \
  } while (0)

extern "C" int pfr_vit_tokens_fwd(const void* patches, const float* class_token, const float* pos, void* tok, int dtype, int B, int S, int D,
                                  hipStream_t st) {
  if (int rc = vit_check("pfr_vit_tokens_fwd", dtype, B, S, D)) return rc;
  PFR_CHECK_ARG((patches || S == 1) && class_token && pos && tok, "pfr_vit_tokens_fwd: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({patches, class_token, pos, tok}), "pfr_vit_tokens_fwd: not a device pointer");
  const size_t n = (size_t)B * S * (D / (dtype == PFR_BF16 ? 8 : 4));
  if (dtype == PFR_BF16) {
    VIT_LAUNCH(vit_tokens_fwd_kernel, bf16_t, n, (const bf16_t*)patches, class_token, pos, (bf16_t*)tok, B, S, D);
  } else {
    VIT_LAUNCH(vit_tokens_fwd_kernel, float, n, (const float*)patches, class_token, pos, (float*)tok, B, S, D);
  }
  return PFR_OK;
}
extern "C" int pfr_vit_tokens_bwd(const void* dtok, void* dpatches, float* dpos, float* dclass_token, int dtype, int B, int S, int D,
                                  hipStream_t st) {
  if (int rc = vit_check("pfr_vit_tokens_bwd", dtype, B, S, D)) return rc;
  PFR_CHECK_ARG(dtok && (dpatches || S == 1) && dpos && dclass_token, "pfr_vit_tokens_bwd: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({dtok, dpatches, dpos, dclass_token}), "pfr_vit_tokens_bwd: not a device pointer");
  const size_t n = (size_t)S * (D / (dtype == PFR_BF16 ? 8 : 4));
  if (dtype == PFR_BF16) {
    VIT_LAUNCH(vit_tokens_bwd_kernel, bf16_t, n, (const bf16_t*)dtok, (bf16_t*)dpatches, dpos, dclass_token, B, S, D);
  } else {
    VIT_LAUNCH(vit_tokens_bwd_kernel, float, n, (const float*)dtok, (float*)dpatches, dpos, dclass_token, B, S, D);
  }
  return PFR_OK;
}
extern "C" int pfr_vit_cls_fwd(const void* x, void* y, int dtype, int B, int S, int D, hipStream_t st) {
  if (int rc = vit_check("pfr_vit_cls_fwd", dtype, B, S, D)) return rc;
  PFR_CHECK_ARG(x && y, "pfr_vit_cls_fwd: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({x, y}), "pfr_vit_cls_fwd: not a device pointer");
  const size_t n = (size_t)B * (D / (dtype == PFR_BF16 ? 8 : 4));
  if (dtype == PFR_BF16) {
    VIT_LAUNCH(vit_cls_fwd_kernel, bf16_t, n, (const bf16_t*)x, (bf16_t*)y, B, S, D);
  } else {
    VIT_LAUNCH(vit_cls_fwd_kernel, float, n, (const float*)x, (float*)y, B, S, D);
  }
  return PFR_OK;
}
extern "C" int pfr_vit_cls_bwd(const void* dy, void* dx, int dtype, int B, int S, int D, hipStream_t st) {
  if (int rc = vit_check("pfr_vit_cls_bwd", dtype, B, S, D)) return rc;
  PFR_CHECK_ARG(dy && dx, "pfr_vit_cls_bwd: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({dy, dx}), "pfr_vit_cls_bwd: not a device pointer");
  const size_t n = (size_t)B * S * (D / (dtype == PFR_BF16 ? 8 : 4));
  if (dtype == PFR_BF16) {
    VIT_LAUNCH(vit_cls_bwd_kernel, bf16_t, n, (const bf16_t*)dy, (bf16_t*)dx, B, S, D);
  } else {
    VIT_LAUNCH(vit_cls_bwd_kernel, float, n, (const float*)dy, (float*)dx, B, S, D);
  }
  return PFR_OK;
}
