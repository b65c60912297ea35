// pfr_pairhist.hip — all-pairs verification: the score GEMM of the match with a HISTOGRAM epilogue (pfr_pair_hist, include/pfr_hip.h).
// The N x N (or Na x Nb) score matrix is never written: every score is binned where the MFMA left it, per kind (genuine / impostor),
// into a workgroup-private LDS table that is flushed into the caller's 64-bit table.
//
// Schedule: persistent workgroups (2 per CU) walk a queue of 128 x 128 tiles in super-tiles of 16 x 16 tiles (what the chip works on at any
// time is a few MB of rows); symmetric mode enumerates the super-tiles of the upper triangle only and skips the tiles below the diagonal.
// A tile: 256 threads = 2 x 2 waves of 64 x 64 (2 x 2 accumulators of 32 x 32), 128-byte k-steps staged global -> registers -> swizzled LDS
// (the v2 operand layout of pfr_mma.h), the next k-step's global loads in flight under the MFMAs of the current one.
//
// Epilogue, per accumulator register: slot = kind * (bins + 1) + bin, one LDS atomic add per lane (masked lanes skip it).  Straight-line
// code: a wave-uniform fast path (all 64 lanes hold one slot -> one lane adds 64) was measured and lost on every realistic input — its
// readfirstlane / compare / branch per register cost 12-20 % of the kernel at N = 100 000 — and won only on identical rows
// (profiles/pair_hist.txt).
//
// Flush rule: the LDS counters are 32-bit.  A tile adds at most 128 * 128 = 2^14 to any of them and a workgroup flushes (64-bit global
// atomic adds of the non-zero slots, then zeroes them) after at most PH_FLUSH_TILES = 2^16 tiles: no LDS counter can pass 2^30.
#include "pfr_igemm.h"

// The score and the bin rule are defined as separately rounded fp32 operations.  The build sets -ffp-contract=fast, which lets the backend
// fuse ANY multiply with a following add (no pragma and no __fmul_rn stops that: the int8 score's second product was seen contracted with
// the bin rule's subtraction into one v_fma_f32).  ph_opaque hides a value's origin from the combiner: an empty asm statement, no instruction.
__device__ __forceinline__ float ph_opaque(float v) {
  asm("" : "+v"(v));
  return v;
}

#define PH_T 128            // tile rows / columns
#define PH_SUPER 16         // super-tile edge in tiles
#define PH_FLUSH_TILES 65536
#define PH_ROWB 128         // LDS operand row: one 128-byte k-step (KCH = 8)

struct PairHistParams {
  const char* a;
  const char* b;
  const float* a_scale;
  const float* b_scale;
  const int* a_cls;
  const int* b_cls;
  int Na, Nb, sym;
  int rowb;                 // bytes per operand row
  float lo, inv_w;
  int bins;
  int ntm, ntn, nsm, nsn;   // tiles / super-tiles per dimension
  long long nsuper;
  unsigned long long* hist;
};

// bin rule of include/pfr_hip.h (two separately rounded operations, floor, clamp; NaN -> slot `bins`)
__device__ __forceinline__ int ph_slot(float s, float lo, float inv_w, int bins) {
  const float x = (s - lo) * inv_w;
  const float t = floorf(x);
  const int bin = (int)fminf(fmaxf(t, 0.f), (float)(bins - 1));
  return s != s ? bins : bin;
}

__device__ __forceinline__ void ph_flush(unsigned int* h, unsigned long long* hist, int slots, int tid) {
  __syncthreads();
  for (int s = tid; s < slots; s += 256) {
    const unsigned int v = h[s];
    if (v) {
      atomicAdd(hist + s, (unsigned long long)v);
      h[s] = 0;
    }
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void pair_hist_kernel(const PairHistParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsA = smem;                                  // [128][128 B]
  char* ldsB = smem + PH_T * PH_ROWB;                 // [128][128 B]
  int* clsA = reinterpret_cast<int*>(smem + 2 * PH_T * PH_ROWB);
  int* clsB = clsA + PH_T;
  float* scA = reinterpret_cast<float*>(clsB + PH_T);
  float* scB = scA + PH_T;
  unsigned int* h = reinterpret_cast<unsigned int*>(scB + PH_T);   // [2][bins + 1]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int slots = 2 * (p.bins + 1);
  for (int s = tid; s < slots; s += 256) h[s] = 0;
  // (the first tile's barriers order this against the first LDS atomic)

  const int lc = tid & 7, lr = tid >> 3;              // this thread's 16-byte chunk and first row of the staged k-step
  const int nk = p.rowb / PH_ROWB;
  int since_flush = 0;
  const long long total = p.nsuper * (PH_SUPER * PH_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const long long su = t / (PH_SUPER * PH_SUPER);
    const int l = (int)(t % (PH_SUPER * PH_SUPER));
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
    const int tm = sm * PH_SUPER + l / PH_SUPER, tn = sn * PH_SUPER + l % PH_SUPER;
    if (tm >= p.ntm || tn >= p.ntn || (p.sym && tn < tm)) continue;   // (block-uniform)
    const int row0 = tm * PH_T, col0 = tn * PH_T;

    // operand rows of a ragged last tile are clamped to the last valid row (their scores are masked below)
    const char* ga[4];
    const char* gb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ra = min(row0 + lr + 32 * u, p.Na - 1), rb = min(col0 + lr + 32 * u, p.Nb - 1);
      ga[u] = p.a + (size_t)ra * p.rowb + lc * 16;
      gb[u] = p.b + (size_t)rb * p.rowb + lc * 16;
    }
    u32x4 va[4], vb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { va[u] = ld16(ga[u]); vb[u] = ld16(gb[u]); }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    for (int ks = 0; ks < nk; ++ks) {
      __syncthreads();   // the previous k-step's (or tile's epilogue's) LDS reads are done
      if (ks == 0 && tid < PH_T) {
        const int ra = min(row0 + tid, p.Na - 1), rb = min(col0 + tid, p.Nb - 1);
        clsA[tid] = p.a_cls[ra];
        clsB[tid] = p.b_cls[rb];
        if constexpr (sizeof(T) == 1) { scA[tid] = p.a_scale[ra]; scB[tid] = p.b_scale[rb]; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = lr + 32 * u;
        const int off = r * PH_ROWB + ((lc ^ row_swizzle<8>(r)) << 4);
        st16(ldsA + off, va[u]);
        st16(ldsB + off, vb[u]);
      }
      __syncthreads();
      if (ks + 1 < nk) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { va[u] = ld16(ga[u] + (ks + 1) * PH_ROWB); vb[u] = ld16(gb[u] + (ks + 1) * PH_ROWB); }
      }
      mma_kstep_sw<T, 8, 2, 2>(ldsA + wp * 64 * PH_ROWB, ldsB + wq * 64 * PH_ROWB, lane, acc);
    }

    // ---- histogram epilogue
    const bool diag = p.sym && tm == tn;
    const bool full = !diag && row0 + PH_T <= p.Na && col0 + PH_T <= p.Nb;   // no element of the tile is masked
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cl = wq * 64 + j * 32 + (lane & 31);
      const int gj = col0 + cl;
      const int cb = clsB[cl];
      float sb = 0.f;
      if constexpr (sizeof(T) == 1) sb = scB[cl];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rl = wp * 64 + i * 32 + acc_row(r, lane);
          const int gi = row0 + rl;
          float s;
          if constexpr (sizeof(T) == 1) s = ph_opaque(((float)__float_as_int(acc[i][j][r]) * scA[rl]) * sb);
          else s = acc[i][j][r];
          int slot = ph_slot(s, p.lo, p.inv_w, p.bins) + (clsA[rl] == cb ? p.bins + 1 : 0);
          if (!full && !(gi < p.Na && gj < p.Nb && (!diag || gi < gj))) slot = -1;
          if (slot >= 0) atomicAdd(h + slot, 1u);
        }
      }
    }
    if (++since_flush == PH_FLUSH_TILES) {
      ph_flush(h, p.hist, slots, tid);
      since_flush = 0;
    }
  }
  ph_flush(h, p.hist, slots, tid);
}

static std::atomic<unsigned long long> g_ph_lds_done{0};

extern "C" int pfr_pair_hist(const void* a, const float* a_scale, const int* a_cls, int Na, const void* b, const float* b_scale,
                             const int* b_cls, int Nb, int dtype, int D, float lo, float inv_w, int bins, unsigned long long* hist,
                             hipStream_t stream) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16 || dtype == PFR_I8, "pfr_pair_hist: bad dtype %d", dtype);
  PFR_CHECK_ARG(bins >= 1 && bins <= 8192, "pfr_pair_hist: bins=%d must be in 1..8192", bins);
  PFR_CHECK_ARG(inv_w > 0.f && inv_w <= 3.0e38f && lo == lo && fabsf(lo) <= 3.0e38f, "pfr_pair_hist: lo / inv_w must be finite, inv_w > 0");
  PFR_CHECK_ARG(Na >= 0 && (b == nullptr || Nb >= 0), "pfr_pair_hist: negative row count");
  const int esz = dtype == PFR_F32 ? 4 : (dtype == PFR_BF16 ? 2 : 1);
  if (dtype == PFR_I8)
    PFR_CHECK_ARG(D > 0 && D % 128 == 0 && D <= 1040, "pfr_pair_hist: int8 rows need Dp %% 128 == 0 and Dp <= 1040 (exact int32 -> float), got %d", D);
  else
    PFR_CHECK_ARG(D > 0 && D % (128 / esz) == 0 && D <= 65536, "pfr_pair_hist: D=%d must be a multiple of %d (128-byte k-steps)", D, 128 / esz);
  const bool sym = b == nullptr;
  if (sym) { b = a; b_scale = a_scale; b_cls = a_cls; Nb = Na; }
  if (Na == 0 || Nb == 0 || (sym && Na == 1)) return PFR_OK;   // no pair: nothing is added
  PFR_CHECK_ARG(a && b && a_cls && b_cls && hist, "pfr_pair_hist: null pointer");
  PFR_CHECK_ARG(dtype != PFR_I8 || (a_scale && b_scale), "pfr_pair_hist: int8 rows need their scales");
  PFR_CHECK_ARG(pfr_all_dev({a, b, a_scale, b_scale, a_cls, b_cls, hist}), "pfr_pair_hist: every pointer must be device memory");

  PairHistParams p;
  p.a = static_cast<const char*>(a); p.b = static_cast<const char*>(b);
  p.a_scale = a_scale; p.b_scale = b_scale; p.a_cls = a_cls; p.b_cls = b_cls;
  p.Na = Na; p.Nb = Nb; p.sym = sym ? 1 : 0;
  p.rowb = D * esz;
  p.lo = lo; p.inv_w = inv_w; p.bins = bins; p.hist = hist;
  p.ntm = (Na + PH_T - 1) / PH_T; p.ntn = (Nb + PH_T - 1) / PH_T;
  p.nsm = (p.ntm + PH_SUPER - 1) / PH_SUPER; p.nsn = (p.ntn + PH_SUPER - 1) / PH_SUPER;
  p.nsuper = sym ? (long long)p.nsn * (p.nsn + 1) / 2 : (long long)p.nsm * p.nsn;
  const long long ntiles = sym ? (long long)p.ntn * (p.ntn + 1) / 2 : (long long)p.ntm * p.ntn;
  const long long slots = 2LL * num_cus();
  const unsigned grid = (unsigned)(ntiles < slots ? ntiles : slots);
  const int lds = 2 * PH_T * PH_ROWB + 4 * PH_T * 4 + 2 * (bins + 1) * 4;   // <= 100 360 bytes
  PFR_MAX_LDS_ONCE(g_ph_lds_done, 2 * PH_T * PH_ROWB + 4 * PH_T * 4 + 2 * 8193 * 4, (const void*)pair_hist_kernel<float>,
                   (const void*)pair_hist_kernel<bf16_t>, (const void*)pair_hist_kernel<int8_t>);
  if (dtype == PFR_F32) hipLaunchKernelGGL(pair_hist_kernel<float>, dim3(grid), dim3(256), lds, stream, p);
  else if (dtype == PFR_BF16) hipLaunchKernelGGL(pair_hist_kernel<bf16_t>, dim3(grid), dim3(256), lds, stream, p);
  else hipLaunchKernelGGL(pair_hist_kernel<int8_t>, dim3(grid), dim3(256), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
