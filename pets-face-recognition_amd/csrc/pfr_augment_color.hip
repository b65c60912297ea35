// pfr_augment_color.hip — horizontal flip, ColorJitter, grayscale (uint8 pre-pass) and RandomErasing (float32 post-pass) of the
// device augmentation pipeline, bit-exact with the Pillow arithmetic torchvision's PIL-image transforms run.
//
// torchvision calls replaced (torchvision/transforms/_functional_pil.py; the restatement the tests pin is tools/color_augment_np.py):
//   RandomHorizontalFlip      img.transpose(FLIP_LEFT_RIGHT)
//   ColorJitter               randperm(4) order of  ImageEnhance.Brightness / Contrast / Color (.enhance(f) = Image.blend(degenerate,
//                             img, f), Blend.c: (float)(d + f * (i - d)), truncated; clipped first when f is outside [0, 1]) and
//                             adjust_hue (convert('HSV'), H += uint8(hue * 255), convert('RGB'); Convert.c rgb2hsv_row / hsv2rgb)
//   RandomGrayscale           convert('L') on three channels, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
//   RandomErasing             tensor[..., i:i+h, j:j+w] = value  after ToTensor
// The pre-pass is pointwise except for Contrast's degenerate image, a solid grey of int(mean(L) + 0.5) of the image AS IT STANDS when
// Contrast's turn comes.  So: pass A applies the ops in front of Contrast to every pixel and reduces the integer sum of L per image
// (a flip does not change a sum, so pass A ignores it); pass B applies flip and all ops with the grey level known and stores.  No
// intermediate image is written: one read (+ one for pass A) and one write of the uint8 batch.
// The library is built with -ffp-contract=fast; every product that feeds an add is pinned in a register by an empty asm statement
// (as pfr_augment_dev.h does) so that no fma forms where Pillow rounds twice.
#include "pfr_common.h"
#include "pfr_augment_dev.h"
#include <math.h>
#include <string.h>

#define AUGC_REC 12     // ints per colour record: flip, gray, order[4] (op ids in run order, -1 = none), factor bits b / c / s, hue byte, pad[2]
#define AUGE_REC 8      // ints per erase record: on, i, j, h, w, value bits of the three channels
#define AUGC_PX 4       // pixels per thread: 12 contiguous bytes (a pixel is 3 bytes; a wave covers 768 contiguous bytes of a row)

// ---- host: decision records -----------------------------------------------------------------------------------------------
static int f2bits(float f) {
  int b;
  memcpy(&b, &f, 4);
  return b;
}

extern "C" int pfr_augment_color_params(const int* flip, const int* gray, const int* order, const float* factors, const float* hue,
                                        int ops_mask, int N, int* records, int* mask_out) {
  PFR_CHECK_ARG(flip && gray && order && factors && hue && records && mask_out && N > 0, "pfr_augment_color_params: bad args");
  PFR_CHECK_ARG(ops_mask >= 0 && ops_mask < 16, "pfr_augment_color_params: ops_mask %d outside [0, 15]", ops_mask);
  int mask = 0;
  for (int i = 0; i < N; ++i) {
    int* r = records + (size_t)i * AUGC_REC;
    for (int j = 0; j < AUGC_REC; ++j) r[j] = 0;
    r[0] = flip[i] != 0;
    r[1] = gray[i] != 0;
    int seen = 0, k = 0;
    for (int j = 0; j < 4; ++j) {
      const int op = order[i * 4 + j];
      PFR_CHECK_ARG(op >= 0 && op < 4 && !(seen >> op & 1), "pfr_augment_color_params: order of sample %d is no permutation of 0..3", i);
      seen |= 1 << op;
      if (ops_mask >> op & 1) r[2 + k++] = op;
    }
    for (; k < 4; ++k) r[2 + k] = -1;
    for (int j = 0; j < 3; ++j) {
      const float f = factors[i * 3 + j];
      PFR_CHECK_ARG(!(ops_mask >> j & 1) || (f >= 0.0f && f < 1e30f), "pfr_augment_color_params: factor %g of sample %d", (double)f, i);
      r[6 + j] = f2bits(f);
    }
    if (ops_mask & 8) {
      PFR_CHECK_ARG(hue[i] >= -0.5f && hue[i] <= 0.5f, "pfr_augment_color_params: hue %g of sample %d outside [-0.5, 0.5]", (double)hue[i], i);
      r[9] = (int)((double)hue[i] * 255.0) & 255;      // np.array(hue * 255).astype(np.uint8): truncate, keep the low byte
    }
    if (r[0]) mask |= 1;
    if (r[1] || ops_mask) mask |= 2;
    if (ops_mask & 2) mask |= 4;
  }
  *mask_out = mask;
  return PFR_OK;
}

extern "C" int pfr_augment_erase_params(const int* rects, const float* value, int N, int H, int W, int* records, int* max_area) {
  PFR_CHECK_ARG(rects && value && records && max_area && N > 0 && H > 0 && W > 0, "pfr_augment_erase_params: bad args");
  int area = 0;
  for (int i = 0; i < N; ++i) {
    const int* q = rects + (size_t)i * 5;
    int* r = records + (size_t)i * AUGE_REC;
    for (int j = 0; j < AUGE_REC; ++j) r[j] = 0;
    if (!q[0]) continue;
    PFR_CHECK_ARG(q[1] >= 0 && q[2] >= 0 && q[3] > 0 && q[4] > 0 && q[3] <= H - q[1] && q[4] <= W - q[2],
                  "pfr_augment_erase_params: rectangle (%d, %d, %d, %d) of sample %d outside the %dx%d image", q[1], q[2], q[3], q[4], i, H, W);
    r[0] = 1;
    for (int j = 1; j < 5; ++j) r[j] = q[j];
    for (int j = 0; j < 3; ++j) r[5 + j] = f2bits(value[j]);
    if (q[3] * q[4] > area) area = q[3] * q[4];
  }
  *max_area = area;
  return PFR_OK;
}

// ---- device: Pillow's pixel arithmetic -------------------------------------------------------------------------------------------
__device__ __forceinline__ int augc_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// Blend.c: (float)(d + f * (i - d)); f in [0, 1] → truncate, else clip to [0, 255] and truncate
__device__ __forceinline__ int augc_blend(int d, int i, float f, bool clip) {
  float prod = f * (float)(i - d);
  asm volatile("" : "+v"(prod));
  float t = (float)d + prod;
  if (clip) t = fminf(fmaxf(t, 0.0f), 255.0f);
  return (int)t;
}

__device__ __forceinline__ int augc_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Convert.c rgb2hsv_row → hue byte += shift → Convert.c hsv2rgb (floats and doubles where the C has them)
__device__ __forceinline__ void augc_hue_px(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    double hd = (double)h / 6.0 + 1.0;                 // fmod(h / 6 + 1, 1) for h / 6 + 1 in [5/6, 11/6]: exact
    if (hd >= 1.0) hd -= 1.0;
    h = (float)hd;
    uh = augc_clip8((int)((double)h * 255.0));
    us = augc_clip8((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 255;
  if (us == 0) {
    r = g = b = uv;
    return;
  }
  const double h6 = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const double f = (double)(float)(h6 - (double)(float)i);
  const double fs = (double)(float)((double)(float)us / 255.0);
  const double v = (double)uv;
  double a = fs * f, omf = 1.0 - f;
  asm volatile("" : "+v"(a), "+v"(omf));
  double c = fs * omf;
  asm volatile("" : "+v"(c));
  double pp = v * (1.0 - fs), qq = v * (1.0 - a), tt = v * (1.0 - c);
  asm volatile("" : "+v"(pp), "+v"(qq), "+v"(tt));
  const int p = augc_clip8((int)floor(pp + 0.5)), q = augc_clip8((int)floor(qq + 0.5)), t = augc_clip8((int)floor(tt + 0.5));
  switch (i % 6) {
    case 0: r = uv; g = t; b = p; break;
    case 1: r = q; g = uv; b = p; break;
    case 2: r = p; g = uv; b = t; break;
    case 3: r = p; g = q; b = uv; break;
    case 4: r = t; g = p; b = uv; break;
    default: r = uv; g = p; b = q; break;
  }
}

// the jitter ops of one image on the AUGC_PX pixels of a thread, in the record's order.  SUM: stop in front of Contrast and
// return true when the image has one (the caller then sums L); grey = Contrast's level otherwise.  The order is uniform over the
// workgroup (one image per blockIdx.y), so the branches are scalar.
template <bool SUM>
__device__ __forceinline__ bool augc_jitter(int (&r)[AUGC_PX], int (&g)[AUGC_PX], int (&b)[AUGC_PX], const int* __restrict__ rec, int grey) {
  const int ord = (rec[2] & 15) | (rec[3] & 15) << 4 | (rec[4] & 15) << 8 | (rec[5] & 15) << 12;     // -1 → 15
  const int shift = rec[9];
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const int op = ord >> (4 * k) & 15;
    if (op > 3) break;
    if (op == 3) {
#pragma unroll
      for (int j = 0; j < AUGC_PX; ++j) augc_hue_px(r[j], g[j], b[j], shift);
      continue;
    }
    if (SUM && op == 1) return true;
    const float f = __int_as_float(rec[6 + op]);
    const bool clip = !(f >= 0.0f && f <= 1.0f);
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j) {
      const int l = op == 2 ? augc_luma(r[j], g[j], b[j]) : 0;
      const int d = op == 0 ? 0 : (op == 1 ? grey : l);
      r[j] = augc_blend(d, r[j], f, clip);
      g[j] = augc_blend(d, g[j], f, clip);
      b[j] = augc_blend(d, b[j], f, clip);
    }
  }
  return false;
}

// one thread = AUGC_PX consecutive pixels of one row (the last chunk of a row may hold fewer); grid (chunks of an image / 256, N).
// mask: 1 honour the flip flags, 2 honour the jitter / grayscale part of the records.
// SUM (pass A): sums[n] += L of every pixel as it stands in front of Contrast; nothing is stored.
// !SUM (pass B): out = flip → jitter (grey from sums[n]) → grayscale of x.  out may be x when mask has no flip (pointwise, in place).
template <bool SUM>
__global__ __launch_bounds__(256) void aug_color_kernel(const uint8_t* x, uint8_t* out, int H, int W, const int* __restrict__ crec,
                                                        unsigned long long* sums, int mask) {
  const int n = blockIdx.y;
  const int* rec = crec + (size_t)n * AUGC_REC;
  const bool color = (mask & 2) != 0;
  bool has_contrast = false;
  if (color)
    for (int k = 0; k < 4; ++k) has_contrast |= rec[2 + k] == 1;
  if (SUM && !has_contrast) return;
  const int cw = (W + AUGC_PX - 1) / AUGC_PX;
  const int chunk = blockIdx.x * 256 + threadIdx.x;
  const bool live = chunk < H * cw;
  const int yy = live ? chunk / cw : 0, x0 = live ? (chunk - yy * cw) * AUGC_PX : 0;
  const int npx = live ? min(AUGC_PX, W - x0) : 0;
  const size_t img = (size_t)n * H * W * 3, rowo = img + (size_t)yy * W * 3;
  int r[AUGC_PX], g[AUGC_PX], b[AUGC_PX];
#pragma unroll
  for (int j = 0; j < AUGC_PX; ++j) r[j] = g[j] = b[j] = 0;
  if (npx == AUGC_PX) {
    uint32_t w[3];
    __builtin_memcpy(w, x + rowo + (size_t)x0 * 3, 12);
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j) {
      r[j] = (w[(3 * j) >> 2] >> (((3 * j) & 3) * 8)) & 255;
      g[j] = (w[(3 * j + 1) >> 2] >> (((3 * j + 1) & 3) * 8)) & 255;
      b[j] = (w[(3 * j + 2) >> 2] >> (((3 * j + 2) & 3) * 8)) & 255;
    }
  } else {
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j)
      if (j < npx) {
        const uint8_t* p = x + rowo + (size_t)(x0 + j) * 3;
        r[j] = p[0];
        g[j] = p[1];
        b[j] = p[2];
      }
  }
  int grey = 0;
  if (!SUM && has_contrast) {
    // int(ImageStat.Stat(L).mean[0] + 0.5): integer sum, double division
    grey = (int)((double)sums[n] / (double)((long long)H * W) + 0.5);
  }
  if (color) augc_jitter<SUM>(r, g, b, rec, grey);
  if (SUM) {
    int s = 0;
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j)
      if (j < npx) s += augc_luma(r[j], g[j], b[j]);
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    // 256 threads x 4 pixels x 255 fits an int; the per-image total (255 * H * W) may not: 64-bit combine
    if (threadIdx.x == 0) atomicAdd(&sums[n], (unsigned long long)(part[0] + part[1] + part[2] + part[3]));
    return;
  }
  if (!live) return;
  if (color && rec[1]) {
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j) r[j] = g[j] = b[j] = augc_luma(r[j], g[j], b[j]);
  }
  const bool flip = (mask & 1) && rec[0];
  if (npx == AUGC_PX) {
    // a flipped chunk lands on AUGC_PX consecutive pixels too, in reverse order
    uint32_t w[3] = {0, 0, 0};
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j) {
      const int rr = flip ? r[AUGC_PX - 1 - j] : r[j], gg = flip ? g[AUGC_PX - 1 - j] : g[j], bb = flip ? b[AUGC_PX - 1 - j] : b[j];
      w[(3 * j) >> 2] |= (uint32_t)rr << (((3 * j) & 3) * 8);
      w[(3 * j + 1) >> 2] |= (uint32_t)gg << (((3 * j + 1) & 3) * 8);
      w[(3 * j + 2) >> 2] |= (uint32_t)bb << (((3 * j + 2) & 3) * 8);
    }
    const int xd = flip ? W - x0 - AUGC_PX : x0;
    __builtin_memcpy(out + rowo + (size_t)xd * 3, w, 12);
  } else {
#pragma unroll
    for (int j = 0; j < AUGC_PX; ++j)
      if (j < npx) {
        const int xd = flip ? W - 1 - (x0 + j) : x0 + j;
        uint8_t* p = out + rowo + (size_t)xd * 3;
        p[0] = (uint8_t)r[j];
        p[1] = (uint8_t)g[j];
        p[2] = (uint8_t)b[j];
      }
  }
}

// y float32 [N][3][H][W]; one thread per pixel of the largest rectangle of the batch
__global__ __launch_bounds__(256) void aug_erase_kernel(float* __restrict__ y, int H, int W, const int* __restrict__ erec) {
  const int n = blockIdx.y;
  const int* r = erec + (size_t)n * AUGE_REC;
  if (!r[0]) return;
  const int i = r[1], j = r[2], h = r[3], w = r[4];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (w <= 0 || p >= h * w) return;
  const int yy = i + p / w, xx = j + p % w;
  if (yy < 0 || yy >= H || xx < 0 || xx >= W) return;
  const size_t plane = (size_t)H * W;
  float* yo = y + (size_t)n * 3 * plane + (size_t)yy * W + xx;
#pragma unroll
  for (int c = 0; c < 3; ++c) yo[c * plane] = __int_as_float(r[5 + c]);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------
extern "C" long pfr_augment_color_ws_bytes(int N) { return ((long)N * 8 + 255) & ~255L; }

extern "C" int pfr_augment_color(const unsigned char* x, int N, int H, int W, const int* color_records, int mask, unsigned char* out,
                                 void* ws, hipStream_t st) {
  PFR_CHECK_ARG(x && color_records && out && ws, "pfr_augment_color: null pointer");
  PFR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * ((W + AUGC_PX - 1) / AUGC_PX) < (1LL << 31) - 256,
                "pfr_augment_color: bad sizes (N=%d %dx%d)", N, H, W);
  PFR_CHECK_ARG(mask > 0 && mask < 8, "pfr_augment_color: mask %d outside [1, 7]", mask);
  PFR_CHECK_ARG(!(mask & 1) || (const unsigned char*)out != x, "pfr_augment_color: a flip cannot run in place");
  const int chunks = H * ((W + AUGC_PX - 1) / AUGC_PX);
  const dim3 grid((chunks + 255) / 256, N);
  unsigned long long* sums = (unsigned long long*)ws;
  if ((mask & 6) == 6) {
    if (hipMemsetAsync(sums, 0, (size_t)N * 8, st) != hipSuccess) {
      pfr_set_error("pfr_augment_color: hipMemsetAsync failed");
      return PFR_ERR_HIP;
    }
    hipLaunchKernelGGL(aug_color_kernel<true>, grid, dim3(256), 0, st, x, out, H, W, color_records, sums, mask);
    PFR_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(aug_color_kernel<false>, grid, dim3(256), 0, st, x, out, H, W, color_records, sums, mask);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}

extern "C" int pfr_augment_erase(float* y, int N, int H, int W, const int* erase_records, int max_area, hipStream_t st) {
  PFR_CHECK_ARG(y && erase_records, "pfr_augment_erase: null pointer");
  PFR_CHECK_ARG(N > 0 && N <= 65535 && H > 0 && W > 0 && max_area >= 0 && (long long)max_area <= (long long)H * W,
                "pfr_augment_erase: bad sizes (N=%d %dx%d max_area=%d)", N, H, W, max_area);
  if (max_area == 0) return PFR_OK;
  hipLaunchKernelGGL(aug_erase_kernel, dim3((max_area + 255) / 256, N), dim3(256), 0, st, y, H, W, erase_records);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
