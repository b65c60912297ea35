// pfr_augment_dev.h — device functions shared by the augmentation kernels (pfr_augment.hip, pfr_augment_fit.hip): Pillow's
// ImageFilter.SMOOTH pixel, the ImageOps.autocontrast LUT entry, the wave-wide min / max of the lo / hi search.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define AUG_PREC 22     // Resample.c PRECISION_BITS = 32 - 8 - 2
#define AUG_SLABS 8     // row slabs per image in the pre passes (one workgroup each); lo/hi partials are merged by the consumer

// the colour pre-pass (pfr_augment_color.hip), which the geometry-first pipeline of pfr_augment.hip runs between its own kernels
extern "C" long pfr_augment_color_ws_bytes(int N);
extern "C" int pfr_augment_color(const unsigned char* x, int N, int H, int W, const int* color_records, int mask, unsigned char* out,
                                 void* ws, hipStream_t st);

__device__ __forceinline__ int wave_min_i(int v) {
  for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// ImageFilter.SMOOTH at byte i of an HWC uint8 image with rowb bytes per row; the caller guarantees an interior pixel
// (the 1-pixel frame is copied, Filter.c)
__device__ __forceinline__ int aug_smooth_px(const uint8_t* __restrict__ src, int i, int rowb) {
  int s = 4 * src[i];
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
    for (int dx = -3; dx <= 3; dx += 3) s += src[i + dy * rowb + dx];
  const int v = (2 * s + 13) / 26;          // = (UINT8)(S/13 + 0.5) of Filter.c (S/13 + 0.5 is never within 0.038 of an integer)
  return v > 255 ? 255 : v;
}

// ImageOps.autocontrast's LUT entry in Python-double arithmetic.  The reference rounds the product before the add; the
// library is built with -ffp-contract=fast (which ignores contraction pragmas), so the products are pinned in registers by
// empty asm statements to keep the compiler from forming an fma.
__device__ __forceinline__ uint8_t autocontrast_lut(int ix, int lo, int hi) {
  if (hi <= lo) return (uint8_t)ix;
  const double scale = 255.0 / (double)(hi - lo);
  double offset = (double)(-lo) * scale;
  double prod = (double)ix * scale;
  asm volatile("" : "+v"(offset), "+v"(prod));
  const int v = (int)(prod + offset);
  return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// the per-band LUT of image n from the slab partials of aug_pre_kernel (256 threads)
__device__ __forceinline__ void aug_build_lut(uint8_t (*lut)[256], const int* __restrict__ lohi, int n) {
  for (int i = threadIdx.x; i < 768; i += 256) {
    const int c = i >> 8;
    int lo = 255, hi = 0;
#pragma unroll
    for (int sl = 0; sl < AUG_SLABS; ++sl) {
      lo = min(lo, lohi[(n * AUG_SLABS + sl) * 8 + 2 * c]);
      hi = max(hi, lohi[(n * AUG_SLABS + sl) * 8 + 2 * c + 1]);
    }
    lut[c][i & 255] = autocontrast_lut(i & 255, lo, hi);
  }
  __syncthreads();
}
