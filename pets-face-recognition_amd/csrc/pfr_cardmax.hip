// pfr_cardmax.hip — max-strategy card matching (generate_tsv.py:81-88): the photo x photo score GEMM of the match with a SEGMENTED-MAX
// epilogue (pfr_card_tiles, pfr_card_max_scores, pfr_card_max_rescore; contracts in include/pfr_hip.h).  The photo score matrix is never
// written: every score is folded where the MFMA left it into the maximum of its (query card, gallery card) pair.
//
// Tiling: pfr_card_tiles packs WHOLE cards into tiles of at most 128 photo rows, on both axes.  A card pair therefore lives in exactly one
// (row tile, column tile) and its output element is written by exactly one workgroup with a plain store — no global atomics.
//
// Schedule (pfr_pairhist.hip): persistent workgroups (2 per CU) walk a queue of 128 x 128 tiles in super-tiles of 16 x 16 tiles; a tile is
// 256 threads = 2 x 2 waves of 64 x 64, 128-byte k-steps staged global -> registers -> swizzled LDS, the next k-step's loads in flight under
// the MFMAs of the current one.
//
// Epilogue, two stages (row, then column):
//   maps   per tile and axis, in LDS: rank[row] = the row's card among the tile's NON-EMPTY cards (-1 for the rows past the tile's row
//          count: they never enter a maximum), start[rank] / card[rank] = first local row and global index of that card.  Built from the
//          segment offsets with two wave ballots per axis.
//   rows   a lane's 32 accumulator rows of one column come in ascending order: it folds the runs of equal row card in registers and sends
//          one LDS atomic max per run into R[row card][column] (order-preserving u32 keys).
//   cols   one thread per (row card, column card): max of R over the column card's columns -> out.
// R is [128][128] u32 = 64 KiB in the worst case (single-photo cards) and ALIASES the operand tiles (32 KiB, dead after the last k-step); only
// the rows of the tile's own row cards are initialised.  With the maps a workgroup takes 70 720 bytes: two fit the 160 KiB of a CU, which this
// kernel needs because a tile's k-steps are not double buffered in LDS (the second workgroup's MFMAs cover the first one's staging).
// The other open design, a table that does not alias (98 KiB, one workgroup per CU), gives up that overlap and was not built
// (measurements of this one: profiles/card_max.txt).
#include "pfr_igemm.h"

#define CM_T 128            // tile rows / columns
#define CM_SUPER 16         // super-tile edge in tiles
#define CM_ROWB 128         // LDS operand row: one 128-byte k-step (KCH = 8)
#define CM_KEY_NINF 0x007fffffu   // fkey(-inf)
#define CM_ECH (CM_T * CM_T) // column cards per chunk of the empty-card pass (their flags take R's 64 KiB)

// ---- pfr_card_tiles (host only) -------------------------------------------------------------------------------------------------
extern "C" long pfr_card_tiles(const long* seg, int ncards, int* tiles, int cap) {
  PFR_CHECK_ARG(seg && ncards >= 0 && cap >= 0, "pfr_card_tiles: bad args");
  PFR_CHECK_ARG(seg[0] >= 0, "pfr_card_tiles: negative offset");
  if (ncards == 0) return 0;
  long nt = 0;
  int first = 0, end = 0;     // the open tile holds the cards [first, end) + the empty cards that follow, `rows` photo rows
  long rows = 0;
  auto emit = [&](int c0, int c1, long r) {
    if (tiles && nt < cap) {
      tiles[4 * nt] = c0; tiles[4 * nt + 1] = c1 - c0; tiles[4 * nt + 2] = (int)seg[c0]; tiles[4 * nt + 3] = (int)r;
    }
    ++nt;
  };
  for (int c = 0; c < ncards; ++c) {
    const long n = seg[c + 1] - seg[c];
    PFR_CHECK_ARG(n >= 0, "pfr_card_tiles: offsets decrease at card %d", c);
    PFR_CHECK_ARG(seg[c + 1] <= 0x7fffffffL, "pfr_card_tiles: more than 2^31 - 1 photo rows");
    if (n > CM_T) {
      pfr_set_error("pfr_card_tiles: card %d has %ld photos, a tile holds at most %d", c, n, CM_T);
      return PFR_ERR_UNSUPPORTED;
    }
    if (n == 0) continue;     // goes with the next non-empty card (or, trailing, with the last tile)
    if (rows + n > CM_T) {
      emit(first, end, rows);
      first = end;
      rows = 0;
    }
    rows += n;
    end = c + 1;
  }
  emit(first, ncards, rows);
  PFR_CHECK_ARG(!tiles || nt <= cap, "pfr_card_tiles: %ld tiles do not fit cap=%d", nt, cap);
  return nt;
}

// ---- pfr_card_max_scores --------------------------------------------------------------------------------------------------------
struct CardMaxParams {
  const char* q;
  const char* g;
  const long* qseg;
  const long* gseg;
  const int* qtiles;
  const int* gtiles;
  int Pq, Pg, Qcards;
  int rowb;                 // bytes per operand row
  int col0, n, ld;
  int ntm, ntn, nsn;        // tiles / super-tiles
  long long nsuper;
  float* out;
};

struct CardMaxMaps {        // one axis of a tile
  int rank[CM_T];           // local row -> non-empty card of the tile, -1 past the tile's rows
  int flag[CM_T];           // a non-empty card starts at this local row
  int at[CM_T];             //   ... its global index
  int card[CM_T];           // non-empty card -> global index
  int start[CM_T + 4];      // non-empty card -> first local row; start[count] = rows of the tile
  int count;
  int pad[3];
};

// wave-wide: ranks of the rows and the compacted card lists from the start flags
__device__ __forceinline__ void cm_ranks(CardMaxMaps& m, int nr, int lane) {
  const int f0 = m.flag[lane], f1 = m.flag[lane + 64];
  const unsigned long long b0 = __ballot(f0 != 0), b1 = __ballot(f1 != 0);
  const unsigned long long upto = (2ull << lane) - 1ull;     // bits 0..lane
  const int n0 = __popcll(b0);
  const int r0 = __popcll(b0 & upto) - 1, r1 = n0 + __popcll(b1 & upto) - 1;
  m.rank[lane] = lane < nr ? r0 : -1;
  m.rank[lane + 64] = lane + 64 < nr ? r1 : -1;
  if (f0) { m.card[r0] = m.at[lane]; m.start[r0] = lane; }
  if (f1) { m.card[r1] = m.at[lane + 64]; m.start[r1] = lane + 64; }
  if (lane == 0) {
    m.count = n0 + __popcll(b1);
    m.start[m.count] = nr;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void card_max_kernel(const CardMaxParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* ldsA = smem;                                  // [128][128 B]
  char* ldsB = smem + CM_T * CM_ROWB;                 // [128][128 B]
  uint32_t* R = reinterpret_cast<uint32_t*>(smem);    // [row cards][128] keys — aliases the operand tiles
  CardMaxMaps* maps = reinterpret_cast<CardMaxMaps*>(smem + CM_T * CM_T * 4);
  CardMaxMaps& mA = maps[0];
  CardMaxMaps& mB = maps[1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wp = wave >> 1, wq = wave & 1;
  const int lc = tid & 7, lr = tid >> 3;              // this thread's 16-byte chunk and first row of the staged k-step
  const int nk = p.rowb / CM_ROWB;
  const long long total = p.nsuper * (CM_SUPER * CM_SUPER);
  for (long long t = blockIdx.x; t < total; t += gridDim.x) {
    const long long su = t / (CM_SUPER * CM_SUPER);
    const int l = (int)(t % (CM_SUPER * CM_SUPER));
    const int tm = (int)(su / p.nsn) * CM_SUPER + l / CM_SUPER, tn = (int)(su % p.nsn) * CM_SUPER + l % CM_SUPER;
    if (tm >= p.ntm || tn >= p.ntn) continue;         // (block-uniform, as every `continue` below)
    const int cA0 = p.qtiles[4 * tm], ncA = p.qtiles[4 * tm + 1], row0 = p.qtiles[4 * tm + 2], nrA = min(p.qtiles[4 * tm + 3], CM_T);
    const int cB0 = p.gtiles[4 * tn], ncB = p.gtiles[4 * tn + 1], colr0 = p.gtiles[4 * tn + 2], nrB = min(p.gtiles[4 * tn + 3], CM_T);
    if (cB0 + ncB <= p.col0 || cB0 >= p.col0 + p.n || ncA <= 0 || ncB <= 0) continue;   // no card of the tile is in the window

    // ---- maps
    __syncthreads();          // the previous tile's epilogue is done with the maps and with R
    if (tid < CM_T) { mA.flag[tid] = 0; mB.flag[tid] = 0; }
    __syncthreads();
    for (int c = tid; c < ncA; c += 256) {
      const long s = p.qseg[cA0 + c];
      const unsigned at = (unsigned)(s - row0);
      if (p.qseg[cA0 + c + 1] > s && at < (unsigned)CM_T) { mA.flag[at] = 1; mA.at[at] = cA0 + c; }
    }
    for (int c = tid; c < ncB; c += 256) {
      const long s = p.gseg[cB0 + c];
      const unsigned at = (unsigned)(s - colr0);
      if (p.gseg[cB0 + c + 1] > s && at < (unsigned)CM_T) { mB.flag[at] = 1; mB.at[at] = cB0 + c; }
    }
    __syncthreads();
    if (wave == 0) cm_ranks(mA, nrA, lane);
    else if (wave == 1) cm_ranks(mB, nrB, lane);
    __syncthreads();
    const int na = mA.count, nb = mB.count;

    if (nrA > 0 && nrB > 0) {
      // operand rows past the tile's row count are clamped to its last row (their scores never enter a maximum: rank -1 / column mask)
      const char* ga[4];
      const char* gb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int ra = min(row0 + min(lr + 32 * u, nrA - 1), p.Pq - 1), rb = min(colr0 + min(lr + 32 * u, nrB - 1), p.Pg - 1);
        ga[u] = p.q + (size_t)ra * p.rowb + lc * 16;
        gb[u] = p.g + (size_t)rb * p.rowb + lc * 16;
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
        __syncthreads();   // the previous k-step's LDS reads are done
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int r = lr + 32 * u;
          const int off = r * CM_ROWB + ((lc ^ row_swizzle<8>(r)) << 4);
          st16(ldsA + off, va[u]);
          st16(ldsB + off, vb[u]);
        }
        __syncthreads();
        if (ks + 1 < nk) {
#pragma unroll
          for (int u = 0; u < 4; ++u) { va[u] = ld16(ga[u] + (ks + 1) * CM_ROWB); vb[u] = ld16(gb[u] + (ks + 1) * CM_ROWB); }
        }
        mma_kstep_sw<T, 8, 2, 2>(ldsA + wp * 64 * CM_ROWB, ldsB + wq * 64 * CM_ROWB, lane, acc);
      }

      // ---- R = -inf over the tile's row cards (the operand tiles are dead)
      __syncthreads();
      {
        u32x4 k4;
        k4[0] = k4[1] = k4[2] = k4[3] = CM_KEY_NINF;
        for (int i = tid; i < na * (CM_T / 4); i += 256) st16(R + 4 * i, k4);
      }
      __syncthreads();

      // ---- rows: runs of equal row card folded in registers, one LDS atomic max per run
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = wq * 64 + j * 32 + (lane & 31);
        const bool cok = col < nrB;
        int cur = -1;
        float m = -INFINITY;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rk = mA.rank[wp * 64 + i * 32 + acc_row(r, lane)];
            const float v = acc[i][j][r];
            if (rk != cur) {
              if (cur >= 0 && cok) atomicMax(R + cur * CM_T + col, fkey(m));
              cur = rk;
              m = v;
            } else {
              m = fmaxf(m, v);
            }
          }
        }
        if (cur >= 0 && cok) atomicMax(R + cur * CM_T + col, fkey(m));
      }
      __syncthreads();

      // ---- cols: thread (a, b) takes the max over the columns of column card b; consecutive threads write consecutive gallery cards
      int bw = 1;
      while (bw < nb) bw <<= 1;
      const int b = tid & (bw - 1);
      if (b < nb) {
        const int c0 = mB.start[b], c1 = mB.start[b + 1];
        const int cB = mB.card[b];
        const bool inwin = cB >= p.col0 && cB < p.col0 + p.n;
        for (int a = tid / bw; a < na; a += 256 / bw) {
          uint32_t k = CM_KEY_NINF;
          for (int c = c0; c < c1; ++c) k = max(k, R[a * CM_T + c]);
          const int cA = mA.card[a];
          if (inwin && cA < p.Qcards) p.out[(size_t)cA * p.ld + (cB - p.col0)] = fkey_inv(k);
        }
      }
    }

    // ---- a tile that holds empty cards: their rows / columns are -inf
    // Emptiness is decided once per card, not per cell: the column cards' flags are staged in LDS (R is dead by now; chunks of CM_ECH cards,
    // a tile may hold any number of empty cards), a wave takes a row card, reads its two offsets and its lanes walk the staged flags.
    if (na != ncA || nb != ncB) {
      int* emptyB = reinterpret_cast<int*>(R);
      for (int b0 = 0; b0 < ncB; b0 += CM_ECH) {
        const int nbc = min(CM_ECH, ncB - b0);
        __syncthreads();      // the column stage's reads of R (or the previous chunk's reads of the flags) are done
        for (int b = tid; b < nbc; b += 256) emptyB[b] = p.gseg[cB0 + b0 + b + 1] == p.gseg[cB0 + b0 + b];
        __syncthreads();
        for (int a = wave; a < ncA; a += 4) {
          const int cA = cA0 + a;
          if (cA >= p.Qcards) break;
          const bool ea = p.qseg[cA + 1] == p.qseg[cA];
          for (int b = lane; b < nbc; b += 64) {
            const int cB = cB0 + b0 + b;
            if ((ea || emptyB[b]) && cB >= p.col0 && cB < p.col0 + p.n) p.out[(size_t)cA * p.ld + (cB - p.col0)] = -INFINITY;
          }
        }
      }
    }
  }
}

static std::atomic<unsigned long long> g_cm_lds_done{0};

extern "C" int pfr_card_max_scores(const void* q, const long* q_seg, const int* q_tiles, int n_qtiles, int Pq, int Qcards, const void* g,
                                   const long* g_seg, const int* g_tiles, int n_gtiles, int Pg, int dtype, int D, int col0, int n,
                                   float* out, int ld, hipStream_t stream) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "pfr_card_max_scores: bad dtype %d", dtype);
  const int esz = dtype == PFR_F32 ? 4 : 2;
  PFR_CHECK_ARG(D > 0 && D % (128 / esz) == 0 && D <= 65536, "pfr_card_max_scores: D=%d must be a multiple of %d (128-byte k-steps)", D, 128 / esz);
  PFR_CHECK_ARG(n_qtiles >= 0 && n_gtiles >= 0 && Pq >= 0 && Pg >= 0 && Qcards >= 0, "pfr_card_max_scores: negative count");
  PFR_CHECK_ARG(col0 >= 0 && n >= 0 && ld >= n && (long long)col0 + n <= 0x7fffffffLL, "pfr_card_max_scores: bad window col0=%d n=%d ld=%d", col0, n, ld);
  if (n_qtiles == 0 || n_gtiles == 0 || n == 0 || Qcards == 0) return PFR_OK;
  PFR_CHECK_ARG(q_seg && g_seg && q_tiles && g_tiles && out, "pfr_card_max_scores: null pointer");
  PFR_CHECK_ARG((Pq == 0 || q) && (Pg == 0 || g), "pfr_card_max_scores: null pointer");
  PFR_CHECK_ARG(pfr_all_dev({q, q_seg, q_tiles, g, g_seg, g_tiles, out}), "pfr_card_max_scores: every pointer must be device memory");

  CardMaxParams p;
  p.q = static_cast<const char*>(q); p.g = static_cast<const char*>(g);
  p.qseg = q_seg; p.gseg = g_seg; p.qtiles = q_tiles; p.gtiles = g_tiles;
  // (with no photo rows on a side every tile of it has a row count of 0 and nothing is read)
  p.Pq = Pq > 0 ? Pq : 1; p.Pg = Pg > 0 ? Pg : 1; p.Qcards = Qcards;
  p.rowb = D * esz;
  p.col0 = col0; p.n = n; p.ld = ld; p.out = out;
  p.ntm = n_qtiles; p.ntn = n_gtiles;
  const int nsm = (p.ntm + CM_SUPER - 1) / CM_SUPER;
  p.nsn = (p.ntn + CM_SUPER - 1) / CM_SUPER;
  p.nsuper = (long long)nsm * p.nsn;
  const long long ntiles = (long long)p.ntm * p.ntn, slots = 2LL * num_cus();
  const unsigned grid = (unsigned)(ntiles < slots ? ntiles : slots);
  const int lds = CM_T * CM_T * 4 + 2 * (int)sizeof(CardMaxMaps);
  PFR_MAX_LDS_ONCE(g_cm_lds_done, lds, (const void*)card_max_kernel<float>, (const void*)card_max_kernel<bf16_t>);
  if (Pq == 0 || Pg == 0) {
    // (the operand pointer may be NULL: no tile has rows, the kernel only writes -inf)
    if (!p.q) p.q = reinterpret_cast<const char*>(q_seg);
    if (!p.g) p.g = reinterpret_cast<const char*>(g_seg);
  }
  if (dtype == PFR_F32) hipLaunchKernelGGL(card_max_kernel<float>, dim3(grid), dim3(256), lds, stream, p);
  else hipLaunchKernelGGL(card_max_kernel<bf16_t>, dim3(grid), dim3(256), lds, stream, p);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// ---- pfr_card_max_rescore -------------------------------------------------------------------------------------------------------
// One wave per (query card, candidate) pair.  The photo rows of the two cards are the A and B rows of v_mfma_f32_32x32x2_f32, read straight
// from global memory in the k order of the fp32 tile kernel above (k-group of 8: lanes 0-31 elements 0..3, lanes 32-63 elements 4..7, one
// MFMA per element): the same instructions on the same values in the same order, so the maxima are the bits pfr_card_max_scores(PFR_F32)
// writes.  Cards above 32 photos take several 32 x 32 blocks.
__global__ __launch_bounds__(256) void card_max_rescore_kernel(const float* __restrict__ q, const long* __restrict__ qseg,
                                                               const float* __restrict__ g, const long* __restrict__ gseg, int Gcards,
                                                               int D, const int* __restrict__ cand, int kc, float* __restrict__ out,
                                                               long long npairs) {
  const int lane = threadIdx.x & 63;
  const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= npairs) return;                         // (wave-uniform; the kernel has no barrier)
  const int row = lane & 31, half = lane >> 5;
  const int c = cand[pair];
  float best = -INFINITY;
  if (c >= 0 && c < Gcards) {
    const long a0 = qseg[pair / kc], a1 = qseg[pair / kc + 1], b0 = gseg[c], b1 = gseg[c + 1];
    for (long ab = a0; ab < a1; ab += 32) {
      const int na = (int)min(32L, a1 - ab);
      const float* pa = q + (size_t)(ab + min(row, na - 1)) * D;
      for (long bb = b0; bb < b1; bb += 32) {
        const int nb = (int)min(32L, b1 - bb);
        const float* pb = g + (size_t)(bb + min(row, nb - 1)) * D;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int k = 0; k < D; k += 8) {
          const int off = k + half * 4;
          f32x4 xa = {0.f, 0.f, 0.f, 0.f}, xb = {0.f, 0.f, 0.f, 0.f};
          if (off < D) {
            xa = *reinterpret_cast<const f32x4*>(pa + off);
            xb = *reinterpret_cast<const f32x4*>(pb + off);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[e], xb[e], acc, 0, 0, 0);
        }
        if (row < nb) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (acc_row(r, lane) < na) best = fmaxf(best, acc[r]);
        }
      }
    }
  }
  best = wave_max(best);
  if (lane == 0) out[pair] = best;
}

extern "C" int pfr_card_max_rescore(const float* q, const long* q_seg, int Q, const float* g, const long* g_seg, int Gcards, int D,
                                    const int* cand, int kc, float* out, hipStream_t stream) {
  PFR_CHECK_ARG(Q >= 0 && Gcards >= 0 && kc >= 0 && kc <= 512, "pfr_card_max_rescore: bad sizes (kc <= 512)");
  PFR_CHECK_ARG(D > 0 && D % 4 == 0, "pfr_card_max_rescore: D=%d must be a multiple of 4 (16-byte chunks)", D);
  if (Q == 0 || kc == 0) return PFR_OK;
  PFR_CHECK_ARG(q_seg && g_seg && cand && out, "pfr_card_max_rescore: null pointer");
  PFR_CHECK_ARG((reinterpret_cast<size_t>(q) & 15) == 0 && (reinterpret_cast<size_t>(g) & 15) == 0, "pfr_card_max_rescore: rows must be 16-byte aligned");
  PFR_CHECK_ARG(pfr_all_dev({q, q_seg, g, g_seg, cand, out}), "pfr_card_max_rescore: every pointer must be device memory");
  const long long npairs = (long long)Q * kc;
  hipLaunchKernelGGL(card_max_rescore_kernel, dim3((unsigned)((npairs + 3) / 4)), dim3(256), 0, stream, q, q_seg, g, g_seg, Gcards, D, cand,
                     kc, out, npairs);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
