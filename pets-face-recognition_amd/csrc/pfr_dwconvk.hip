// pfr_dwconvk.hip — depthwise K x K convolution on NHWC, K = 3 | 5, padding K/2, stride 1 | 2 (forward with the producer's BatchNorm
// apply + activation as a prologue and its own BatchNorm statistics as an epilogue, data gradient, weight gradient with the same
// prologue), for the EfficientNet engine (models/_efficientnet_engine.py).  gfx950, VALU / HBM work: no MFMA.
//
// The geometry is pfr_dwconv3.hip's: thread (q, s) = (16-byte channel chunk q of the row, row lane s); a workgroup (256 threads = CW
// chunk columns x RL row lanes) owns a contiguous range of flattened pixel rows and its lanes walk it RL rows at a time, so a thread
// stays on its channels.  Prologue (pro_act): 0 = the operand is x; 1 = min(max(s x + t, 0), hi) — at K = 3 the arithmetic and its
// order are pfr_dwconv3_fwd's, the results equal it bit for bit; 2 = silu(s x + t), the sigmoid in fp32.  Taps outside the image are
// zeroed after the prologue (the padding is of the activated tensor) and every load comes from clamped coordinates: none sits in a branch.
//
// The halo at 25 taps: still left to the caches, no LDS staging.  Reasons: (i) the row lanes of a workgroup are consecutive pixels of
// a plane row, so the 25 requests of a pixel meet lines its neighbours in the SAME workgroup asked for — the re-reads are served by the
// CU's vector L1 and the XCD's L2, and HBM sees each x line once per XCD; (ii) EfficientNet's 5x5 planes are 28² ... 7² at bs 256: a
// staged (T+4)² tile of a plane that small carries 2.5-6x halo and needs a barrier per tile, which is how the staged 7x7 kernel of
// pfr_dwconv.hip ended at 11-15x its HBM bound while the unstaged 3x3 kernel reaches 22-66 % of the streaming rate; (iii) the 25 taps
// stay in registers as 25 PACKED chunks (100 VGPRs in either dtype, unpacked at use), and the loads are issued one tap row (K chunks)
// at a time.  Not measured against a staged form.
//
// Registers and occupancy (vgpr_count of the code object, -O3, scratch 0 everywhere): every K = 3 and every fp32 kernel stays at or
// under 256, two waves per SIMD.  The bf16 K = 5 kernels do not, except the data gradient (252 / 152) and the forward without
// prologue and statistics (252): forward with statistics 281 (no prologue) / 299 (clamp) / 340 (SiLU), without statistics 269 / 312,
// weight gradient 260 / 310 / 440.  With __launch_bounds__(256, 1) the compiler may take the whole 512-entry file, so these run ONE
// wave per SIMD — the engine's default training path at 5x5 bf16 (forward with statistics, no prologue: 281; weight gradient: 260)
// among them.  PFR_DWK_MIN_WAVES (below; build.sh's variant builds) is the second argument of the launch bounds.  With 2 the
// compiler caps these kernels at 256 registers and spills 28-724 bytes per lane to scratch; measured with the SiLU prologue
// (profiles/efficientnet_b2_minwaves2.txt against profiles/efficientnet_b2.txt, bs 256 bf16) the 5x5 forward is then 2.1-2.6x and
// the weight gradient 1.4-2.4x SLOWER (28²x288: 0.65 → 1.63 ms, 0.91 → 2.16 ms), the data gradients and the 3x3 weight gradient are unchanged and the
// 3x3 forward, which does not spill, is 6-17 % slower: the default stays 1.  The prologue-free 5x5 forms (104 / 28 bytes of scratch at 2) were not timed separately, and a smaller live set
// that fits 256 registers without scratch (fewer taps resident, or two passes over the tap rows) was not tried.
//
// Measured (profiles/efficientnet_b2.txt): the 5x5 forward with the SiLU prologue runs at 4-14 % of the streaming rate, its data
// gradient at 14-30 %, the 3x3 forms at 12-50 % / 25-64 %.  What bounds the 5x5 kernels is NOT established: no counter run was made.
// Candidates: the vector ALU (unpack, select, FMA and, with a prologue, one exponential per tap), or, at one wave per SIMD with 25
// dependent 16-byte loads per pixel, load latency that nothing hides.  The spill A/B above does not separate the two.
#include "pfr_common.h"
#include <initializer_list>

// minimum waves per SIMD the compiler has to leave room for (second argument of __launch_bounds__); 2 lost its A/B, see the header:
// PFR_BUILD_TAG=mw2 PFR_EXTRA_FLAGS="-DPFR_DWK_MIN_WAVES=2" build.sh, then tools/efficientnet_bench.py --only-depthwise with PFR_LIB_PATH
#ifndef PFR_DWK_MIN_WAVES
#define PFR_DWK_MIN_WAVES 1
#endif

struct DwkGeom {
  int cpr;     // chunks per row (C / KP)
  int cw;      // chunk columns per workgroup
  int rl;      // row lanes per workgroup = 256 / cw
  int gy;      // workgroups along the columns
  long rpp;    // rows per workgroup (the last one may hold fewer)
  int parts;   // workgroups along the rows
};
// `target` workgroups in all, every row lane at least 4 rows (pfr_dwconv3.hip's rule)
static DwkGeom dwk_geom(int kp, long rows, int C, int target) {
  DwkGeom g;
  g.cpr = C / kp;
  g.cw = g.cpr < 256 ? g.cpr : 256;
  g.rl = 256 / g.cw;
  g.gy = (g.cpr + g.cw - 1) / g.cw;
  long want = target / g.gy;
  if (want < 1) want = 1;
  long rpp = (rows + want - 1) / want;
  if (rpp < 4l * g.rl) rpp = 4l * g.rl;
  g.rpp = rpp;
  g.parts = (int)((rows + rpp - 1) / rpp);
  return g;
}

// the prologue of a chunk: ACT 1 = relu6-style clamp (hi = +inf: none), ACT 2 = silu
template <int KP, int ACT>
__device__ __forceinline__ void dwk_activate(float (&v)[KP], const float (&sc)[KP], const float (&sh)[KP], float hi) {
  if constexpr (ACT == 1) {
#pragma unroll
    for (int e = 0; e < KP; ++e) v[e] = fminf(fmaxf(fmaf(v[e], sc[e], sh[e]), 0.f), hi);
  } else if constexpr (ACT == 2) {
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      const float u = fmaf(v[e], sc[e], sh[e]);
      v[e] = u * __builtin_amdgcn_rcpf(1.f + __expf(-u));
    }
  }
}

// ------------------------------------------------------------------------------------------------ forward
// stats (STATS): every thread keeps (count, Σd, Σd²) of the STORED y of its rows about its first value, turns them into (mean, M2), and
// lane 0 of each chunk column merges the RL lanes (Chan, fixed order) into the workgroup's partial row [2][C]
template <typename T, int K, int ACT, bool STATS>
__global__ __launch_bounds__(256, PFR_DWK_MIN_WAVES) void dwconvk_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w, T* __restrict__ y,
                                                          const float* __restrict__ pro_scale, const float* __restrict__ pro_shift,
                                                          float hi, float* __restrict__ stats, int H, int W, int C, int OH, int OW,
                                                          int stride, int cw, int rl, int cpr, uint32_t rows, uint32_t rpp) {
  constexpr int KP = DT<T>::KPACK, P = K / 2;
  __shared__ float red[STATS ? 256 * (2 * KP + 1) : 1];
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  const bool active = s < rl && cglob < cpr;
  const uint32_t rbeg = blockIdx.x * rpp;
  const uint32_t rend = rbeg + rpp < rows ? rbeg + rpp : rows;
  float cnt = 0.f, k[KP], sa[KP], sb[KP];
#pragma unroll
  for (int e = 0; e < KP; ++e) { k[e] = 0.f; sa[e] = 0.f; sb[e] = 0.f; }
  if (active) {
    const int c = cglob * KP;
    u32x4 wt[K * K];
    float sc[KP], sh[KP];
#pragma unroll
    for (int t = 0; t < K * K; ++t) wt[t] = ld16(w + (size_t)t * C + c);
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      sc[e] = ACT ? pro_scale[c + e] : 1.f;
      sh[e] = ACT ? pro_shift[c + e] : 0.f;
    }
    const uint32_t plane = (uint32_t)OH * OW;
    for (uint32_t r = rbeg + s; r < rend; r += rl) {
      const uint32_t n = r / plane, rem = r - n * plane;
      const int oh = rem / OW, ow = rem - oh * OW;
      const int ih0 = oh * stride - P, iw0 = ow * stride - P;
      float acc[KP];
#pragma unroll
      for (int e = 0; e < KP; ++e) acc[e] = 0.f;
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        u32x4 v[K];
        const int ihc = min(max(ih0 + kh, 0), H - 1);
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int iwc = min(max(iw0 + kw, 0), W - 1);
          v[kw] = ld16(x + (((size_t)n * H + ihc) * W + iwc) * C + c);
        }
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int ih = ih0 + kh, iw = iw0 + kw;
          const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
          float f[KP], wf[KP];
          Chunk<T>::unpack(v[kw], f);
          Chunk<T>::unpack(wt[kh * K + kw], wf);
          dwk_activate<KP, ACT>(f, sc, sh, hi);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[e] = fmaf(ok ? f[e] : 0.f, wf[e], acc[e]);
        }
      }
      const u32x4 out = Chunk<T>::pack(acc);
      st16(y + (size_t)r * C + c, out);
      if (STATS) {
        float yr[KP];
        Chunk<T>::unpack(out, yr);
        if (cnt == 0.f) {
#pragma unroll
          for (int e = 0; e < KP; ++e) k[e] = yr[e];
        }
        cnt += 1.f;
#pragma unroll
        for (int e = 0; e < KP; ++e) {
          const float d = yr[e] - k[e];
          sa[e] += d;
          sb[e] = fmaf(d, d, sb[e]);
        }
      }
    }
  }
  if (!STATS) return;
  float* mine = red + threadIdx.x * (2 * KP + 1);
  const float cn = cnt > 0.f ? cnt : 1.f;
  mine[0] = cnt;
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    mine[1 + e] = k[e] + sa[e] / cn;
    mine[1 + KP + e] = sb[e] - sa[e] * sa[e] / cn;
  }
  __syncthreads();
  if (s != 0 || cglob >= cpr) return;
  float nt = 0.f;
  for (int j = 0; j < rl; ++j) nt += red[(j * cw + col) * (2 * KP + 1)];
  float* out_row = stats + (size_t)blockIdx.x * 2 * C + cglob * KP;
#pragma unroll
  for (int e = 0; e < KP; ++e) {
    float a = 0.f;
    for (int j = 0; j < rl; ++j) {
      const float* o = red + (j * cw + col) * (2 * KP + 1);
      a = fmaf(o[0], o[1 + e], a);
    }
    const float mean = a / nt;
    float m2 = 0.f;
    for (int j = 0; j < rl; ++j) {
      const float* o = red + (j * cw + col) * (2 * KP + 1);
      const float d = o[1 + e] - mean;
      m2 += o[1 + KP + e] + o[0] * d * d;
    }
    out_row[e] = mean;
    out_row[C + e] = m2;
  }
}

// ------------------------------------------------------------------------------------------------ data gradient
// gather per dx pixel: dx[h][w] = Σ dy[oh][ow] w[kh][kw] over the taps with oh * stride - P + kh = h.  Stride 1: the K² taps (oh = h + P - kh).
// Stride 2: per direction the candidates j = 0 .. (K+1)/2 - 1 are kh = par + 2j with par = (h + P) & 1 and oh = (h + P - par)/2 - j
// (K = 5: three rows for even h, two for odd h; K = 3: one or two), so ((K+1)/2)² loads per pixel and a parity select of the packed
// tap — a candidate whose tap index is past K or whose output pixel is outside [0, OH) x [0, OW) contributes 0
template <typename T, int K, int STRIDE>
__global__ __launch_bounds__(256, PFR_DWK_MIN_WAVES) void dwconvk_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ w, T* __restrict__ dx, int H,
                                                            int W, int C, int OH, int OW, int cw, int rl, int cpr, uint32_t rows,
                                                            uint32_t rpp) {
  constexpr int KP = DT<T>::KPACK, P = K / 2, NC = (K + 1) / 2;
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  if (s >= rl || cglob >= cpr) return;
  const int c = cglob * KP;
  const uint32_t rbeg = blockIdx.x * rpp;
  const uint32_t rend = rbeg + rpp < rows ? rbeg + rpp : rows;
  u32x4 wt[K * K];
#pragma unroll
  for (int t = 0; t < K * K; ++t) wt[t] = ld16(w + (size_t)t * C + c);
  const uint32_t plane = (uint32_t)H * W;
  for (uint32_t r = rbeg + s; r < rend; r += rl) {
    const uint32_t n = r / plane, rem = r - n * plane;
    const int h = rem / W, wq = rem - h * W;
    float acc[KP];
#pragma unroll
    for (int e = 0; e < KP; ++e) acc[e] = 0.f;
    if constexpr (STRIDE == 1) {
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        u32x4 v[K];
        const int oh = h + P - kh, ohc = min(max(oh, 0), OH - 1);
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int owc = min(max(wq + P - kw, 0), OW - 1);
          v[kw] = ld16(dy + (((size_t)n * OH + ohc) * OW + owc) * C + c);
        }
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int ow = wq + P - kw;
          const bool ok = oh >= 0 && oh < OH && ow >= 0 && ow < OW;
          float f[KP], wf[KP];
          Chunk<T>::unpack(v[kw], f);
          Chunk<T>::unpack(wt[kh * K + kw], wf);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[e] = fmaf(ok ? f[e] : 0.f, wf[e], acc[e]);
        }
      }
    } else {
      const int ph = (h + P) & 1, pw = (wq + P) & 1;
      const int ohb = (h + P - ph) >> 1, owb = (wq + P - pw) >> 1;
#pragma unroll
      for (int a = 0; a < NC; ++a) {
        u32x4 v[NC];
        const int oh = ohb - a, ohc = min(max(oh, 0), OH - 1);
        const bool okh = oh >= 0 && oh < OH && ph + 2 * a < K;
#pragma unroll
        for (int b = 0; b < NC; ++b) {
          const int owc = min(max(owb - b, 0), OW - 1);
          v[b] = ld16(dy + (((size_t)n * OH + ohc) * OW + owc) * C + c);
        }
#pragma unroll
        for (int b = 0; b < NC; ++b) {
          const int ow = owb - b;
          const bool ok = okh && ow >= 0 && ow < OW && pw + 2 * b < K;
          // the tap (ph + 2a, pw + 2b): the four parity cases as compile-time indices (an index past K is never selected with ok)
          const int kh0 = 2 * a, kh1 = 2 * a + 1 < K ? 2 * a + 1 : K - 1;
          const int kw0 = 2 * b, kw1 = 2 * b + 1 < K ? 2 * b + 1 : K - 1;
          const u32x4 w0 = pw ? wt[kh0 * K + kw1] : wt[kh0 * K + kw0];
          const u32x4 w1 = pw ? wt[kh1 * K + kw1] : wt[kh1 * K + kw0];
          const u32x4 ws = ph ? w1 : w0;
          float f[KP], wf[KP];
          Chunk<T>::unpack(v[b], f);
          Chunk<T>::unpack(ws, wf);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[e] = fmaf(ok ? f[e] : 0.f, wf[e], acc[e]);
        }
      }
    }
    st16(dx + (size_t)r * C + c, Chunk<T>::pack(acc));
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// workgroup (p, column block) walks the output rows of its range with the K² sums of every (channel, row lane) in registers (the operand
// is the activated x, recomputed with the forward's prologue), folds the row lanes through LDS tap by tap and leaves ONE partial row
// set part[p][K²][C] (tap-major)
template <typename T, int K, int ACT>
__global__ __launch_bounds__(256, PFR_DWK_MIN_WAVES) void dwconvk_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ part,
                                                            const float* __restrict__ pro_scale, const float* __restrict__ pro_shift,
                                                            float hi, int H, int W, int C, int OH, int OW, int stride, int cw, int rl,
                                                            int cpr, uint32_t rows, uint32_t rpp) {
  constexpr int KP = DT<T>::KPACK, P = K / 2;
  __shared__ float red[256 * KP];
  const int col = threadIdx.x % cw, s = threadIdx.x / cw;
  const int cglob = blockIdx.y * cw + col;
  const bool active = s < rl && cglob < cpr;
  const int c = cglob * KP;
  const uint32_t rbeg = blockIdx.x * rpp;
  const uint32_t rend = rbeg + rpp < rows ? rbeg + rpp : rows;
  float acc[K * K][KP];
#pragma unroll
  for (int t = 0; t < K * K; ++t)
#pragma unroll
    for (int e = 0; e < KP; ++e) acc[t][e] = 0.f;
  if (active) {
    float sc[KP], sh[KP];
#pragma unroll
    for (int e = 0; e < KP; ++e) {
      sc[e] = ACT ? pro_scale[c + e] : 1.f;
      sh[e] = ACT ? pro_shift[c + e] : 0.f;
    }
    const uint32_t plane = (uint32_t)OH * OW;
    for (uint32_t r = rbeg + s; r < rend; r += rl) {
      const uint32_t n = r / plane, rem = r - n * plane;
      const int oh = rem / OW, ow = rem - oh * OW;
      const int ih0 = oh * stride - P, iw0 = ow * stride - P;
      float g[KP];
      Chunk<T>::unpack(ld16(dy + (size_t)r * C + c), g);
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        u32x4 v[K];
        const int ihc = min(max(ih0 + kh, 0), H - 1);
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int iwc = min(max(iw0 + kw, 0), W - 1);
          v[kw] = ld16(x + (((size_t)n * H + ihc) * W + iwc) * C + c);
        }
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const int ih = ih0 + kh, iw = iw0 + kw;
          const bool ok = ih >= 0 && ih < H && iw >= 0 && iw < W;
          float f[KP];
          Chunk<T>::unpack(v[kw], f);
          dwk_activate<KP, ACT>(f, sc, sh, hi);
#pragma unroll
          for (int e = 0; e < KP; ++e) acc[kh * K + kw][e] = fmaf(g[e], ok ? f[e] : 0.f, acc[kh * K + kw][e]);
        }
      }
    }
  }
  // fold the row lanes, one tap at a time (fixed order)
#pragma unroll
  for (int t = 0; t < K * K; ++t) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < KP; ++e) red[threadIdx.x * KP + e] = acc[t][e];
    __syncthreads();
    if (s == 0 && cglob < cpr) {
      float* out = part + ((size_t)blockIdx.x * (K * K) + t) * C + c;
#pragma unroll
      for (int e = 0; e < KP; ++e) {
        float a = 0.f;
        for (int j = 0; j < rl; ++j) a += red[(j * cw + col) * KP + e];
        out[e] = a;
      }
    }
  }
}

// merge of the partial rows: dw in the parameter's own [C][1][K][K] order; block (tap, 64-channel chunk), 4 slices of P
__global__ __launch_bounds__(256) void dwconvk_wgrad_merge_kernel(const float* __restrict__ part, float* __restrict__ dw, int P, int C,
                                                                  int KK, int accumulate) {
  __shared__ float red[4][64];
  const int t = blockIdx.x, cl = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  float v = 0.f;
  if (c < C)
    for (int p = s; p < P; p += 4) v += part[((size_t)p * KK + t) * C + c];
  red[s][cl] = v;
  __syncthreads();
  if (s != 0 || c >= C) return;
  v = (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
  float* out = dw + (size_t)c * KK + t;
  *out = accumulate ? *out + v : v;
}

// ------------------------------------------------------------------------------------------------ entry points
// argument checks in an order that needs no device: geometry first, pointers last
static int dwk_check(const char* fn, std::initializer_list<const void*> ptrs, int dtype, int N, int H, int W, int C, int K, int stride) {
  PFR_CHECK_ARG(dtype == PFR_F32 || dtype == PFR_BF16, "%s: dtype must be fp32 or bf16", fn);
  if ((K != 3 && K != 5) || (stride != 1 && stride != 2)) {
    pfr_set_error("%s: only K = 3 | 5 and stride 1 | 2 are built (got K = %d, stride = %d)", fn, K, stride);
    return PFR_ERR_UNSUPPORTED;
  }
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  PFR_CHECK_ARG(N > 0 && H > 0 && W > 0 && C > 0, "%s: empty tensor", fn);
  PFR_CHECK_ARG(C % kp == 0, "%s: C = %d is not a multiple of %d (16-byte channel chunks)", fn, C, kp);
  PFR_CHECK_ARG((long)N * H * W < (1l << 31), "%s: more than 2^31 pixels", fn);
  PFR_CHECK_ARG(pfr_all_dev(ptrs), "%s: not a device pointer (no CPU fallback)", fn);
  return PFR_OK;
}

static int dwk_check_pro(const char* fn, int pro_act, const float* pro_scale, const float* pro_shift) {
  PFR_CHECK_ARG(pro_act >= 0 && pro_act <= 2, "%s: pro_act is 0 (none), 1 (clamp) or 2 (silu), got %d", fn, pro_act);
  PFR_CHECK_ARG(pro_act == 0 || (pro_scale && pro_shift), "%s: pro_act %d needs pro_scale and pro_shift", fn, pro_act);
  return PFR_OK;
}

static inline long dwk_out_rows(int N, int H, int W, int stride) { return (long)N * ((H - 1) / stride + 1) * ((W - 1) / stride + 1); }
static inline bool dwk_geom_ok(int dtype, int N, int H, int W, int C, int K, int stride) {
  const int kp = dtype == PFR_BF16 ? 8 : 4;
  return (K == 3 || K == 5) && (stride == 1 || stride == 2) && (dtype == PFR_F32 || dtype == PFR_BF16) && N > 0 && H > 0 && W > 0 &&
         C > 0 && C % kp == 0;
}

extern "C" long pfr_dwconvk_rows_per_part(int dtype, int N, int H, int W, int C, int K, int stride) {
  if (!dwk_geom_ok(dtype, N, H, W, C, K, stride)) return 0;
  return dwk_geom(dtype == PFR_BF16 ? 8 : 4, dwk_out_rows(N, H, W, stride), C, 2048).rpp;
}

extern "C" int pfr_dwconvk_fwd(const void* x, const void* w, void* y, int dtype, int N, int H, int W, int C, int K, int stride,
                               int pro_act, const float* pro_scale, const float* pro_shift, float pro_hi, float* stats_part,
                               hipStream_t st) {
  PFR_CHECK_ARG(x && w && y, "pfr_dwconvk_fwd: null pointer");
  if (int rc = dwk_check_pro("pfr_dwconvk_fwd", pro_act, pro_scale, pro_shift)) return rc;
  if (int rc = dwk_check("pfr_dwconvk_fwd", {x, w, y, pro_scale, pro_shift, stats_part}, dtype, N, H, W, C, K, stride)) return rc;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long rows = (long)N * OH * OW;
  const DwkGeom g = dwk_geom(dtype == PFR_BF16 ? 8 : 4, rows, C, 2048);
  const float hi = pro_hi > 0.f ? pro_hi : __builtin_inff();
  const dim3 grid((unsigned)g.parts, (unsigned)g.gy);
#define PFR_DWK_FWD(TT, KK, ACT, ST)                                                                                                  \
  hipLaunchKernelGGL((dwconvk_fwd_kernel<TT, KK, ACT, ST>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)w, (TT*)y, pro_scale,    \
                     pro_shift, hi, stats_part, H, W, C, OH, OW, stride, g.cw, g.rl, g.cpr, (uint32_t)rows, (uint32_t)g.rpp)
#define PFR_DWK_FWD_S(TT, KK, ACT) do { if (stats_part) PFR_DWK_FWD(TT, KK, ACT, true); else PFR_DWK_FWD(TT, KK, ACT, false); } while (0)
#define PFR_DWK_FWD_A(TT, KK)                          \
  do {                                                 \
    if (pro_act == 0) PFR_DWK_FWD_S(TT, KK, 0);        \
    else if (pro_act == 1) PFR_DWK_FWD_S(TT, KK, 1);   \
    else PFR_DWK_FWD_S(TT, KK, 2);                     \
  } while (0)
  if (dtype == PFR_BF16) { if (K == 3) PFR_DWK_FWD_A(bf16_t, 3); else PFR_DWK_FWD_A(bf16_t, 5); }
  else { if (K == 3) PFR_DWK_FWD_A(float, 3); else PFR_DWK_FWD_A(float, 5); }
#undef PFR_DWK_FWD_A
#undef PFR_DWK_FWD_S
#undef PFR_DWK_FWD
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_dwconvk_dgrad(const void* dy, const void* w, void* dx, int dtype, int N, int H, int W, int C, int K, int stride,
                                 hipStream_t st) {
  PFR_CHECK_ARG(dy && w && dx, "pfr_dwconvk_dgrad: null pointer");
  if (int rc = dwk_check("pfr_dwconvk_dgrad", {dy, w, dx}, dtype, N, H, W, C, K, stride)) return rc;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long rows = (long)N * H * W;
  const DwkGeom g = dwk_geom(dtype == PFR_BF16 ? 8 : 4, rows, C, 2048);
  const dim3 grid((unsigned)g.parts, (unsigned)g.gy);
#define PFR_DWK_DG(TT, KK, S)                                                                                                            \
  hipLaunchKernelGGL((dwconvk_dgrad_kernel<TT, KK, S>), grid, dim3(256), 0, st, (const TT*)dy, (const TT*)w, (TT*)dx, H, W, C, OH, OW,   \
                     g.cw, g.rl, g.cpr, (uint32_t)rows, (uint32_t)g.rpp)
#define PFR_DWK_DG_S(TT, KK) do { if (stride == 1) PFR_DWK_DG(TT, KK, 1); else PFR_DWK_DG(TT, KK, 2); } while (0)
  if (dtype == PFR_BF16) { if (K == 3) PFR_DWK_DG_S(bf16_t, 3); else PFR_DWK_DG_S(bf16_t, 5); }
  else { if (K == 3) PFR_DWK_DG_S(float, 3); else PFR_DWK_DG_S(float, 5); }
#undef PFR_DWK_DG_S
#undef PFR_DWK_DG
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

// partial row sets of the weight gradient (part_ws: fp32 [parts][K²][C]); 0 for a geometry that is not built
extern "C" int pfr_dwconvk_wgrad_parts(int dtype, int N, int H, int W, int C, int K, int stride) {
  if (!dwk_geom_ok(dtype, N, H, W, C, K, stride)) return 0;
  return dwk_geom(dtype == PFR_BF16 ? 8 : 4, dwk_out_rows(N, H, W, stride), C, 1024).parts;
}

extern "C" int pfr_dwconvk_wgrad(const void* x, const void* dy, float* part_ws, float* dw, int dtype, int N, int H, int W, int C, int K,
                                 int stride, int pro_act, const float* pro_scale, const float* pro_shift, float pro_hi, int accumulate,
                                 hipStream_t st) {
  PFR_CHECK_ARG(x && dy && part_ws && dw, "pfr_dwconvk_wgrad: null pointer");
  if (int rc = dwk_check_pro("pfr_dwconvk_wgrad", pro_act, pro_scale, pro_shift)) return rc;
  if (int rc = dwk_check("pfr_dwconvk_wgrad", {x, dy, part_ws, dw, pro_scale, pro_shift}, dtype, N, H, W, C, K, stride)) return rc;
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  const long rows = (long)N * OH * OW;
  const DwkGeom g = dwk_geom(dtype == PFR_BF16 ? 8 : 4, rows, C, 1024);
  const float hi = pro_hi > 0.f ? pro_hi : __builtin_inff();
  const dim3 grid((unsigned)g.parts, (unsigned)g.gy);
#define PFR_DWK_WG(TT, KK, ACT)                                                                                                         \
  hipLaunchKernelGGL((dwconvk_wgrad_kernel<TT, KK, ACT>), grid, dim3(256), 0, st, (const TT*)x, (const TT*)dy, part_ws, pro_scale,      \
                     pro_shift, hi, H, W, C, OH, OW, stride, g.cw, g.rl, g.cpr, (uint32_t)rows, (uint32_t)g.rpp)
#define PFR_DWK_WG_A(TT, KK)                        \
  do {                                              \
    if (pro_act == 0) PFR_DWK_WG(TT, KK, 0);        \
    else if (pro_act == 1) PFR_DWK_WG(TT, KK, 1);   \
    else PFR_DWK_WG(TT, KK, 2);                     \
  } while (0)
  if (dtype == PFR_BF16) { if (K == 3) PFR_DWK_WG_A(bf16_t, 3); else PFR_DWK_WG_A(bf16_t, 5); }
  else { if (K == 3) PFR_DWK_WG_A(float, 3); else PFR_DWK_WG_A(float, 5); }
#undef PFR_DWK_WG_A
#undef PFR_DWK_WG
  PFR_CHECK_LAUNCH();
  hipLaunchKernelGGL(dwconvk_wgrad_merge_kernel, dim3((unsigned)(K * K), (unsigned)((C + 63) / 64)), dim3(256), 0, st, part_ws, dw, g.parts,
                     C, K * K, accumulate);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
