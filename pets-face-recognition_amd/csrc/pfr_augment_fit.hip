// pfr_augment_fit.hip — the FIRST operation of the reference's simple / no-align and body Compose pipelines on the device:
// a ragged batch of uint8 HWC frames (data_loading/ragged.py) → one uniform uint8 [N][canvas_h][canvas_w][3] canvas,
// bit-exact with Pillow.
//
//   mode RESIZE          Resize((224, 224)) of configs/dog_fe/simple_fe_dog.py:17-31 = Image.resize((w, h), BILINEAR), no reducing_gap;
//                        RandomAdjustSharpness(0) / RandomAutocontrast act on the RAW frame first (per-image flags): the resampler reads
//                        through the autocontrast LUT from the blurred or the original frame, so the colour ops cost no pass of their own
//                        beyond the blur / lo-hi search that the head pipeline has as well
//   mode THUMBNAIL_PAD   Lambda(resize_with_padding) of configs/dog_fe/body_dog_fe.py:18-33 = Image.thumbnail((w, h), BICUBIC,
//                        reducing_gap=2.0) + centred zero pad (ImageOps.expand): aspect-preserved size (round_aspect), integer box
//                        pre-reduction (Reduce.c, factor = int(extent / size / 2) per axis), bicubic resize over the rescaled box
//
// Sizes, boxes and the 22-bit fixed-point coefficient tables are HOST arithmetic in Pillow's own double / float operations
// (pfr_augment_fit_params: Image.thumbnail / Image.resize / _get_safe_box, Resample.c precompute_coeffs + normalize_coeffs_8bpc);
// the device does integer work only, without atomics: the output is bit-reproducible.
//   fit_pre      RESIZE images with a flag: blurred copy and per-band lo / hi of the raw frame (the arithmetic of aug_pre_kernel)
//   fit_reduce   THUMBNAIL_PAD images with a factor > 1: box average into the workspace
//   fit_resample one workgroup per 8 x 32 tile of one image's canvas: the horizontal taps of the source rows the tile needs go to
//                an LDS strip as 8-bit values (Pillow's horizontal pass), up to 32 rows at a time; the vertical taps read the strip.
//                The source row segments of a strip are staged in LDS with aligned 16-byte loads first; the taps read LDS.
#include "pfr_common.h"
#include "pfr_augment_dev.h"
#include <math.h>
#include <string.h>
#include <vector>

#define FIT_REC 32      // ints per image record, see pfr_hip.h
#define FIT_TH 8
#define FIT_TW 32
#define FIT_ROWS 32     // source rows per LDS strip
#define FIT_STAGE 32768  // bytes of LDS for the source row segments of one strip
#define FIT_MAX_SIDE 4096
enum { FIT_RESIZE = 0, FIT_THUMBNAIL_PAD = 1 };
enum { R_H, R_W, R_TW, R_TH, R_FX, R_FY, R_RB0, R_RB1, R_RB2, R_RB3, R_BOX0, R_BOX1, R_BOX2, R_BOX3, R_PADL, R_PADT, R_COX, R_KSX, R_COY,
       R_KSY, R_SHARP, R_CONTRAST, R_RW, R_RH, R_MODE, R_NEEDH, R_NEEDV };

// ---- host: Pillow's size / box arithmetic -------------------------------------------------------------------------------
static int round_aspect(double number, bool x_axis, double aspect, int other) {
  // max(min(floor(number), ceil(number), key=key), 1); min() keeps the first of two equal keys
  const long lo = (long)floor(number), hi = (long)ceil(number);
  auto key = [&](long n) {
    if (x_axis) return fabs(aspect - (double)n / (double)other);        // abs(aspect - n / y)
    return n == 0 ? 0.0 : fabs(aspect - (double)other / (double)n);     // 0 if n == 0 else abs(aspect - x / n)
  };
  const long pick = key(hi) < key(lo) ? hi : lo;
  return (int)(pick > 1 ? pick : 1);
}

static double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
static double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

static int fit_ksize(float in0, float in1, int out_size, bool bicubic, bool need) {
  if (!need) return 1;
  double filterscale = (double)(in1 - in0) / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil((bicubic ? 2.0 : 1.0) * filterscale) * 2 + 1;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc over the box (in0, in1); a pass Pillow skips is the identity table
// (one tap of weight 1.0: (v << 22 + (1 << 21)) >> 22 == v).  tab: [out][2 + ksize] = (first tap, taps, k...)
static void fit_coeffs(int in_size, float in0, float in1, int out_size, bool bicubic, bool need, int ksize, int* tab) {
  memset(tab, 0, (size_t)out_size * (2 + ksize) * sizeof(int));
  if (!need) {
    for (int xx = 0; xx < out_size; ++xx) { tab[xx * 3] = xx; tab[xx * 3 + 1] = 1; tab[xx * 3 + 2] = 1 << AUG_PREC; }
    return;
  }
  double scale = (double)(in1 - in0) / out_size, filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = (bicubic ? 2.0 : 1.0) * filterscale, ss = 1.0 / filterscale;
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = in0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double t = (x + xmin - center + 0.5) * ss;
      const double w = bicubic ? bicubic_filter(t) : bilinear_filter(t);
      k[x] = w;
      ww += w;
    }
    int* row = tab + (size_t)xx * (2 + ksize);
    row[0] = xmin;
    row[1] = xmax;
    for (int x = 0; x < xmax; ++x) {
      const double v = ww != 0.0 ? k[x] / ww : k[x];
      row[2 + x] = v < 0 ? (int)(-0.5 + v * (1 << AUG_PREC)) : (int)(0.5 + v * (1 << AUG_PREC));
    }
  }
}

static int f2i(float f) { int i; memcpy(&i, &f, 4); return i; }

// everything of one record but the coefficient offsets; → false with the error set
static bool fit_plan(int mode, int H, int W, int ch, int cw, int* r) {
  for (int j = 0; j < FIT_REC; ++j) r[j] = 0;
  if (H < 1 || W < 1 || H > FIT_MAX_SIDE || W > FIT_MAX_SIDE) {
    pfr_set_error("pfr_augment_fit_params: frame %dx%d outside 1..%d", H, W, FIT_MAX_SIDE);
    return false;
  }
  int tw = cw, th = ch, fx = 1, fy = 1, rb[4] = {0, 0, W, H};
  double box[4] = {0.0, 0.0, (double)W, (double)H};
  if (mode == FIT_THUMBNAIL_PAD) {
    // Image.thumbnail: preserve_aspect_ratio
    if (cw >= W && ch >= H) {
      tw = W; th = H;
    } else {
      const double aspect = (double)W / (double)H;
      if ((double)cw / (double)ch >= aspect) tw = round_aspect(ch * aspect, true, aspect, ch);
      else th = round_aspect(cw / aspect, false, aspect, cw);
    }
    if (tw != W || th != H) {
      // Image.resize(reducing_gap=2.0)
      fx = (int)((box[2] - box[0]) / tw / 2.0);
      fy = (int)((box[3] - box[1]) / th / 2.0);
      if (fx < 1) fx = 1;
      if (fy < 1) fy = 1;
      if (fx > 1 || fy > 1) {
        const double sx = 1.5 * ((box[2] - box[0]) / tw), sy = 1.5 * ((box[3] - box[1]) / th);   // _get_safe_box, bicubic support 2.0 - 0.5
        rb[0] = (int)(box[0] - sx) > 0 ? (int)(box[0] - sx) : 0;
        rb[1] = (int)(box[1] - sy) > 0 ? (int)(box[1] - sy) : 0;
        rb[2] = (int)ceil(box[2] + sx) < W ? (int)ceil(box[2] + sx) : W;
        rb[3] = (int)ceil(box[3] + sy) < H ? (int)ceil(box[3] + sy) : H;
        const double b0 = box[0], b1 = box[1], b2 = box[2], b3 = box[3];
        box[0] = (b0 - rb[0]) / fx; box[1] = (b1 - rb[1]) / fy; box[2] = (b2 - rb[0]) / fx; box[3] = (b3 - rb[1]) / fy;
      }
    }
    r[R_PADL] = (cw - tw) / 2;     // delta >= 0: floor division
    r[R_PADT] = (ch - th) / 2;
  }
  const int rw = (rb[2] - rb[0] + fx - 1) / fx, rh = (rb[3] - rb[1] + fy - 1) / fy;
  const float fb[4] = {(float)box[0], (float)box[1], (float)box[2], (float)box[3]};   // the C resize parses the box as four floats
  r[R_H] = H; r[R_W] = W; r[R_TW] = tw; r[R_TH] = th; r[R_FX] = fx; r[R_FY] = fy;
  for (int j = 0; j < 4; ++j) { r[R_RB0 + j] = rb[j]; r[R_BOX0 + j] = f2i(fb[j]); }
  r[R_RW] = rw; r[R_RH] = rh; r[R_MODE] = mode;
  r[R_NEEDH] = tw != rw || fb[0] != 0.0f || fb[2] != (float)tw;
  r[R_NEEDV] = th != rh || fb[1] != 0.0f || fb[3] != (float)th;
  // Image.resize (Pillow 12.2.0 Image.py): `if self.size[1] > self.size[0] * 100 and size[1] < self.size[1]` resizes vertically FIRST;
  // with both passes needed the 8-bit intermediate differs from the horizontal-first order implemented here (tools/make_ragged_golden.py
  // checks the divergence against Pillow)
  if (rh > rw * 100 && th < rh && r[R_NEEDH] && r[R_NEEDV]) {
    pfr_set_error("pfr_augment_fit_params: frame %dx%d: Pillow resizes images taller than 100:1 in the other pass order; unsupported", H, W);
    return false;
  }
  const bool bic = mode == FIT_THUMBNAIL_PAD;
  r[R_KSX] = fit_ksize(fb[0], fb[2], tw, bic, r[R_NEEDH]);
  r[R_KSY] = fit_ksize(fb[1], fb[3], th, bic, r[R_NEEDV]);
  return true;
}

static bool fit_args_ok(int mode, const int* shapes, int N, int ch, int cw) {
  if (!((mode == FIT_RESIZE || mode == FIT_THUMBNAIL_PAD) && shapes && N > 0 && N <= 65535 && ch > 0 && cw > 0 && ch <= FIT_MAX_SIDE &&
        cw <= FIT_MAX_SIDE)) {
    pfr_set_error("pfr_augment_fit: bad args (mode %d, N %d, canvas %dx%d)", mode, N, ch, cw);
    return false;
  }
  return true;
}

extern "C" long pfr_augment_fit_coeff_ints(int mode, const int* shapes, int N, int canvas_h, int canvas_w) {
  if (!fit_args_ok(mode, shapes, N, canvas_h, canvas_w)) return -1;
  long total = 0;
  int r[FIT_REC];
  for (int i = 0; i < N; ++i) {
    if (!fit_plan(mode, shapes[2 * i], shapes[2 * i + 1], canvas_h, canvas_w, r)) return -1;
    total += (long)r[R_TW] * (2 + r[R_KSX]) + (long)r[R_TH] * (2 + r[R_KSY]);
  }
  return total;
}

extern "C" int pfr_augment_fit_params(int mode, const int* shapes, int N, int canvas_h, int canvas_w, int* records, int* coeffs,
                                      long coeff_capacity) {
  PFR_CHECK_ARG(records && coeffs, "pfr_augment_fit_params: null pointer");
  if (!fit_args_ok(mode, shapes, N, canvas_h, canvas_w)) return PFR_ERR_ARG;
  long at = 0;
  for (int i = 0; i < N; ++i) {
    int* r = records + (size_t)i * FIT_REC;
    if (!fit_plan(mode, shapes[2 * i], shapes[2 * i + 1], canvas_h, canvas_w, r)) return PFR_ERR_UNSUPPORTED;
    const long nx = (long)r[R_TW] * (2 + r[R_KSX]), ny = (long)r[R_TH] * (2 + r[R_KSY]);
    if (at + nx + ny > coeff_capacity || at + nx + ny > 0x7fffffffL) {
      pfr_set_error("pfr_augment_fit_params: coefficient tables need more than %ld ints (pfr_augment_fit_coeff_ints)", coeff_capacity);
      return PFR_ERR_ARG;
    }
    float b[4];
    memcpy(b, r + R_BOX0, 16);
    const bool bic = mode == FIT_THUMBNAIL_PAD;
    r[R_COX] = (int)at;
    fit_coeffs(r[R_RW], b[0], b[2], r[R_TW], bic, r[R_NEEDH], r[R_KSX], coeffs + at);
    at += nx;
    r[R_COY] = (int)at;
    fit_coeffs(r[R_RH], b[1], b[3], r[R_TH], bic, r[R_NEEDV], r[R_KSY], coeffs + at);
    at += ny;
  }
  return PFR_OK;
}

// ---- device ---------------------------------------------------------------------------------------------------------------
// blurred copy (sharp) and per-band lo / hi (contrast) of one row slab of one RESIZE frame: aug_pre_kernel for ragged frames
__global__ __launch_bounds__(1024) void fit_pre_kernel(const uint8_t* __restrict__ data, const long* __restrict__ off,
                                                       const int* __restrict__ rec, uint8_t* __restrict__ img_ws, int* __restrict__ lohi) {
  const int n = blockIdx.x;
  const int* r = rec + n * FIT_REC;
  const int sharp = r[R_SHARP], contrast = r[R_CONTRAST];
  if (r[R_MODE] != FIT_RESIZE || (!sharp && !contrast)) return;
  const int H = r[R_H], W = r[R_W];
  const uint8_t* src = data + off[n];
  uint8_t* dst = img_ws + off[n];
  int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
  const int rowb = W * 3;
  const int rows = (H + AUG_SLABS - 1) / AUG_SLABS, r0 = blockIdx.y * rows, r1 = min(H, r0 + rows);
  for (int yy = r0; yy < r1; ++yy) {
    const bool yin = yy > 0 && yy < H - 1 && H >= 3 && W >= 3;
    for (int xb = threadIdx.x; xb < rowb; xb += 1024) {
      const int xx = xb / 3, c = xb - xx * 3, i = yy * rowb + xb;
      int v = src[i];
      if (sharp) {
        if (yin && xx > 0 && xx < W - 1) v = aug_smooth_px(src, i, rowb);
        dst[i] = (uint8_t)v;
      }
      lo[c] = min(lo[c], v);
      hi[c] = max(hi[c], v);
    }
  }
  if (!contrast) return;
  __shared__ int red[16][6];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int a = wave_min_i(lo[c]), b = wave_max_i(hi[c]);
    if (lane == 0) { red[wv][2 * c] = a; red[wv][2 * c + 1] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    int v = red[0][threadIdx.x];
    for (int w = 1; w < 16; ++w) v = (threadIdx.x & 1) ? max(v, red[w][threadIdx.x]) : min(v, red[w][threadIdx.x]);
    lohi[(n * AUG_SLABS + blockIdx.y) * 8 + threadIdx.x] = v;
  }
}

// Reduce.c for 8-bit bands: (sum + count / 2) / count through the 24-bit reciprocal (UINT32)(2^24 / count) computed in float
// (division_UINT32; the 1x2 / 2x1 / 2x2 / 4x4 shift kernels give the same value), edge columns / rows averaged over what is there
__global__ __launch_bounds__(256) void fit_reduce_kernel(const uint8_t* __restrict__ data, const long* __restrict__ off,
                                                         const int* __restrict__ rec, uint8_t* __restrict__ img_ws) {
  const int n = blockIdx.y;
  const int* r = rec + n * FIT_REC;
  const int fx = r[R_FX], fy = r[R_FY];
  if (fx == 1 && fy == 1) return;
  const int W = r[R_W], x0 = r[R_RB0], y0 = r[R_RB1], bw = r[R_RB2] - x0, bh = r[R_RB3] - y0, rw = r[R_RW], rh = r[R_RH];
  const uint8_t* src = data + off[n];
  uint8_t* dst = img_ws + off[n];
  for (int p = blockIdx.x * 256 + threadIdx.x; p < rw * rh; p += gridDim.x * 256) {
    const int oy = p / rw, ox = p - oy * rw;
    const int nx = min(fx, bw - ox * fx), ny = min(fy, bh - oy * fy);
    uint32_t ss[3] = {0, 0, 0};
    for (int dy = 0; dy < ny; ++dy) {
      const uint8_t* row = src + ((size_t)(y0 + oy * fy + dy) * W + x0 + ox * fx) * 3;
      for (int dx = 0; dx < nx; ++dx) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ss[c] += row[dx * 3 + c];
      }
    }
    const uint32_t cnt = (uint32_t)(nx * ny), mult = (uint32_t)(16777216.0f / (float)cnt);
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[(size_t)p * 3 + c] = (uint8_t)(((ss[c] + cnt / 2) * mult) >> 24);
  }
}

__global__ __launch_bounds__(256) void fit_resample_kernel(const uint8_t* __restrict__ data, const long* __restrict__ off,
                                                           const int* __restrict__ rec, const int* __restrict__ coeffs,
                                                           const uint8_t* __restrict__ img_ws, const int* __restrict__ lohi, int ch, int cw,
                                                           uint8_t* __restrict__ out) {
  __shared__ uint8_t lut[3][256];
  __shared__ uint8_t strip[FIT_ROWS][FIT_TW * 3];
  __shared__ uint4 stage[FIT_STAGE / 16];
  __shared__ int srec[FIT_REC];
  const int n = blockIdx.y;
  if (threadIdx.x < FIT_REC) srec[threadIdx.x] = rec[n * FIT_REC + threadIdx.x];   // the record is read once per workgroup
  __syncthreads();
  const int tw = srec[R_TW], th = srec[R_TH], pad_l = srec[R_PADL], pad_t = srec[R_PADT], rw = srec[R_RW];
  const int ksx = srec[R_KSX], ksy = srec[R_KSY];
  const bool resize = srec[R_MODE] == FIT_RESIZE, contrast = resize && srec[R_CONTRAST];
  const bool from_ws = resize ? srec[R_SHARP] != 0 : (srec[R_FX] > 1 || srec[R_FY] > 1);
  const uint8_t* src = (from_ws ? img_ws : data) + off[n];
  const int* cx = coeffs + srec[R_COX];
  const int* cy = coeffs + srec[R_COY];
  if (contrast) aug_build_lut(lut, lohi, n);

  const int tiles_x = (cw + FIT_TW - 1) / FIT_TW;
  const int ty0 = (blockIdx.x / tiles_x) * FIT_TH, tx0 = (blockIdx.x % tiles_x) * FIT_TW;
  const int lx = threadIdx.x % FIT_TW, ly = threadIdx.x / FIT_TW;
  const int px = tx0 + lx, py = ty0 + ly, ox = px - pad_l, oy = py - pad_t;
  const bool in_canvas = px < cw && py < ch;
  const bool col_ok = px < cw && ox >= 0 && ox < tw, row_ok = py < ch && oy >= 0 && oy < th;
  // target rows / columns of this tile (uniform over the workgroup) → the source rows and the source row segment its taps touch
  const int oy_lo = max(ty0 - pad_t, 0), oy_hi = min(min(ty0 + FIT_TH, ch) - pad_t, th);
  const int ox_lo = max(tx0 - pad_l, 0), ox_hi = min(min(tx0 + FIT_TW, cw) - pad_l, tw);
  int acc[3] = {1 << (AUG_PREC - 1), 1 << (AUG_PREC - 1), 1 << (AUG_PREC - 1)};
  if (oy_lo < oy_hi && ox_lo < ox_hi) {
    const int r0 = cy[(size_t)oy_lo * (2 + ksy)];
    const int* klast = cy + (size_t)(oy_hi - 1) * (2 + ksy);
    const int r1 = klast[0] + klast[1];
    const int xs0 = cx[(size_t)ox_lo * (2 + ksx)];
    const int* kxl = cx + (size_t)(ox_hi - 1) * (2 + ksx);
    const int seg0 = xs0 * 3, segb = (kxl[0] + kxl[1] - xs0) * 3;      // the tile's bytes of every source row
    // a row segment is contiguous: it goes to LDS in aligned 16-byte pieces (the piece that holds its first byte up to the piece that
    // holds its last; frames start on 16-byte boundaries and are padded to 16 bytes, so both stay inside the frame's bytes), `nvec`
    // pieces per row at most.  Segments too long for the stage buffer (down-scaling beyond ~100x) are read from memory tap by tap.
    const int nvec = (segb + 15 + 15) >> 4;
    const int rows_staged = min(FIT_ROWS, (FIT_STAGE / 16) / nvec);
    const int rstep = rows_staged > 0 ? rows_staged : FIT_ROWS;
    const int* kx = cx + (size_t)(col_ok ? ox : ox_lo) * (2 + ksx);
    const int x0 = kx[0], nx = kx[1];
    const int* ky = cy + (size_t)(row_ok ? oy : oy_lo) * (2 + ksy);
    const int y0 = ky[0], ny = ky[1];
    for (int rc = r0; rc < r1; rc += rstep) {
      if (rows_staged > 0) {
        for (int idx = threadIdx.x; idx < rstep * nvec; idx += 256) {
          const int rr = idx / nvec, v = idx - rr * nvec;
          const int first = (rc + rr) * rw * 3 + seg0, m = first & 15;
          if (rc + rr < r1 && v < ((m + segb + 15) >> 4)) stage[idx] = *(const uint4*)(src + (first - m) + v * 16);
        }
        __syncthreads();
      }
      // horizontal pass of source rows rc .. rc + rstep for the tile's columns, to 8 bits
      if (col_ok) {
        for (int rr = ly; rr < rstep && rc + rr < r1; rr += FIT_TH) {
          const int first = (rc + rr) * rw * 3 + seg0;
          const uint8_t* row = rows_staged > 0 ? (const uint8_t*)stage + rr * nvec * 16 + (first & 15) + (x0 - xs0) * 3
                                               : src + ((size_t)(rc + rr) * rw + x0) * 3;
          int a[3] = {1 << (AUG_PREC - 1), 1 << (AUG_PREC - 1), 1 << (AUG_PREC - 1)};
          for (int t = 0; t < nx; ++t) {
            const int k = kx[2 + t];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              int v = row[t * 3 + c];
              if (contrast) v = lut[c][v];
              a[c] += v * k;
            }
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int v = a[c] >> AUG_PREC;
            strip[rr][lx * 3 + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
          }
        }
      }
      __syncthreads();
      if (col_ok && row_ok) {
        const int t0 = max(0, rc - y0), t1 = min(ny, rc + rstep - y0);
        for (int t = t0; t < t1; ++t) {
          const int k = ky[2 + t];
          const uint8_t* s = &strip[y0 + t - rc][lx * 3];
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] += s[c] * k;
        }
      }
      __syncthreads();
    }
  }
  if (!in_canvas) return;
  uint8_t* o = out + (((size_t)n * ch + py) * cw + px) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = acc[c] >> AUG_PREC;
    o[c] = (col_ok && row_ok) ? (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)) : (uint8_t)0;   // ImageOps.expand: zero border
  }
}

// ws: the lo / hi partials [N][AUG_SLABS][8] first, then (256-byte aligned) an image area laid out like `data`
static size_t fit_lohi_bytes(int N) { return ((size_t)N * AUG_SLABS * 8 * sizeof(int) + 255) & ~(size_t)255; }

extern "C" long pfr_augment_fit_ws_bytes(long total_bytes, int N) { return (long)fit_lohi_bytes(N) + total_bytes + 256; }

extern "C" int pfr_augment_fit(const unsigned char* data, const long* offsets, const int* records, const int* coeffs, int N, int canvas_h,
                               int canvas_w, unsigned char* out_u8, void* ws, hipStream_t st) {
  PFR_CHECK_ARG(data && offsets && records && coeffs && out_u8 && ws, "pfr_augment_fit: null pointer");
  PFR_CHECK_ARG(N > 0 && N <= 65535 && canvas_h > 0 && canvas_w > 0 && canvas_h <= FIT_MAX_SIDE && canvas_w <= FIT_MAX_SIDE,
                "pfr_augment_fit: bad sizes (N=%d canvas %dx%d)", N, canvas_h, canvas_w);
  PFR_CHECK_ARG(((uintptr_t)data & 15) == 0 && ((uintptr_t)ws & 15) == 0, "pfr_augment_fit: data and ws must be 16-byte aligned");
  int* lohi = (int*)ws;
  uint8_t* img_ws = (uint8_t*)ws + fit_lohi_bytes(N);
  hipLaunchKernelGGL(fit_pre_kernel, dim3(N, AUG_SLABS), dim3(1024), 0, st, data, offsets, records, img_ws, lohi);
  PFR_CHECK_LAUNCH();
  hipLaunchKernelGGL(fit_reduce_kernel, dim3(64, N), dim3(256), 0, st, data, offsets, records, img_ws);
  PFR_CHECK_LAUNCH();
  const int tiles = ((canvas_w + FIT_TW - 1) / FIT_TW) * ((canvas_h + FIT_TH - 1) / FIT_TH);
  hipLaunchKernelGGL(fit_resample_kernel, dim3(tiles, N), dim3(256), 0, st, data, offsets, records, coeffs, img_ws, lohi, canvas_h, canvas_w,
                     out_u8);
  PFR_CHECK_LAUNCH();
  return PFR_OK;
}
