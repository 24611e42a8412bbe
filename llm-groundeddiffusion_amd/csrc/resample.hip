// Pillow's Image.resize for 8-bit RGB images on the device (include/lgd_hip.h states the contract): [ext] Pillow
// src/libImaging/Resample.c — precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc and
// ImagingResampleVertical_8bpc as ImagingResampleInner chains them (horizontal pass first, an 8-bit image between the
// two, a pass whose size does not change left out).
//
//  * lgd_resample_plan is host code: the fp64 weights of one axis, normalised and rounded to 22 fractional bits.  This
//    file is compiled with floating-point contraction off so that every product and sum rounds where Pillow's do.
//  * resample_pass_kernel is one pass with the output form folded in: one thread per output pixel (three channels, the
//    coefficients read once), a workgroup covers 256 pixels of one output row.  In the vertical pass the window and the
//    coefficients are the same for the whole workgroup; in the horizontal pass neighbouring lanes read overlapping
//    windows of one input row.  Sums are int32, as Pillow's.  No atomics; every output element has one owner.
//  * lgd_resample_u8 launches the horizontal pass into the caller's scratch and the vertical pass from it; when only one
//    axis changes size that pass writes the output itself, and when none does the output form is applied to the input.
//  * lgd_resample_canvas_u8 is the same chain with the LAST pass instantiated with CANVAS: its grid covers a CH x CW
//    canvas, one thread per canvas pixel; a thread inside the H x W image computes its pixel as above, one outside stores
//    the pad value.  Lanes of a wave hold neighbouring pixels of one canvas row, so each of a lane's three stores is one
//    contiguous run per wave (256 B of fp32 per plane); whether a row lies below the image is the same for a whole
//    workgroup, and only the one wave that straddles the image's right edge diverges.  The dense instantiations carry none
//    of this: lgd_resample_u8 launches the kernels it launched before the canvas form existed.
#include "common.h"
#include "contract.h"

#include <math.h>

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr int MAX_SIDE = 16384, MAX_N = 65535;
constexpr int PASS_THREADS = 256;

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  if (x < 1.0) return 1.0 - x;
  return 0.0;
}

double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

// support0 of a filter code, 0 for an unknown one
double support_of(int filter) {
  switch (filter) {
    case LGD_FILTER_BILINEAR: return 1.0;
    case LGD_FILTER_BICUBIC: return 2.0;
    case LGD_FILTER_LANCZOS: return 3.0;
  }
  return 0.0;
}

double weight_of(int filter, double x) {
  switch (filter) {
    case LGD_FILTER_BILINEAR: return bilinear_filter(x);
    case LGD_FILTER_BICUBIC: return bicubic_filter(x);
  }
  return lanczos_filter(x);
}

// the row width 2 ceil(support) + 1 of an axis (in, out >= 1, a known filter)
int width_of(int in, int out, int filter) {
  double filterscale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)ceil(support_of(filter) * filterscale) * 2 + 1;
}

enum { AXIS_NONE = 0, AXIS_H = 1, AXIS_V = 2 };

struct PassArgs {
  const uint8_t* src;     // [N][in_h][in_w][3]
  void* dst;              // uint8 [N][out_h][out_w][3], or fp32 / fp16 [N][3][out_h][out_w]
  const int32_t* coef;    // [out][ksize] of the axis this pass resamples
  const int32_t* bounds;  // [out][2] = {first input index, taps}
  int ksize, in_h, in_w, out_h, out_w;
  float r, m0, m1, m2, s0, s1, s2;
  int cv_h, cv_w;  // CANVAS only: dst is [N][3][cv_h][cv_w] (uint8: [N][cv_h][cv_w][3]), the image at its top left
  float pad;       // CANVAS only: every element outside the out_h x out_w image
};

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PRECISION_BITS, 0), 255); }

template <int FORM>
__device__ __forceinline__ float form_of(int v, float r, float m, float s) {
  if (FORM == LGD_RESAMPLE_AFFINE) return ((float)v * r - m) / s;
  return (float)v / 255.f * 2.f - 1.f;
}

template <int AXIS, int FORM, typename T, bool CANVAS>
__global__ __launch_bounds__(PASS_THREADS) void resample_pass_kernel(const PassArgs a) {
  const int xx = blockIdx.x * PASS_THREADS + threadIdx.x, yy = blockIdx.y, n = blockIdx.z;
  const int rows = CANVAS ? a.cv_h : a.out_h, row_w = CANVAS ? a.cv_w : a.out_w;  // of dst; the grid covers them
  if (xx >= row_w) return;
  const bool inside = !CANVAS || (xx < a.out_w && yy < a.out_h);
  int v0 = 0, v1 = 0, v2 = 0;
  if (!inside) {
    // a pad pixel reads neither the source nor the tables (their rows end at the image)
  } else if (AXIS == AXIS_NONE) {
    const uint8_t* p = a.src + (((long)n * a.in_h + yy) * a.in_w + xx) * 3;
    v0 = p[0], v1 = p[1], v2 = p[2];
  } else {
    // the window is clamped into the input whatever the table holds: a wrong table gives wrong pixels, not a fault
    const int o = AXIS == AXIS_H ? xx : yy, in = AXIS == AXIS_H ? a.in_w : a.in_h;
    const int first = min(max(a.bounds[2 * o], 0), in - 1);
    const int taps = min(min(max(a.bounds[2 * o + 1], 0), a.ksize), in - first);
    const int32_t* k = a.coef + (long)o * a.ksize;
    const long step = AXIS == AXIS_H ? 3 : (long)a.in_w * 3;
    const uint8_t* p = AXIS == AXIS_H ? a.src + (((long)n * a.in_h + yy) * a.in_w + first) * 3
                                      : a.src + (((long)n * a.in_h + first) * a.in_w + xx) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
#pragma unroll 1
    for (int t = 0; t < taps; ++t, p += step) {
      const int kt = k[t];
      s0 += kt * (int)p[0], s1 += kt * (int)p[1], s2 += kt * (int)p[2];
    }
    v0 = clip8(s0), v1 = clip8(s1), v2 = clip8(s2);
  }
  if (FORM == LGD_RESAMPLE_U8) {
    if (!inside) v0 = v1 = v2 = (int)a.pad;  // an integral byte: the host refused anything else
    uint8_t* d = static_cast<uint8_t*>(a.dst) + (((long)n * rows + yy) * row_w + xx) * 3;
    d[0] = (uint8_t)v0, d[1] = (uint8_t)v1, d[2] = (uint8_t)v2;
  } else {
    const long plane = (long)rows * row_w;
    T* d = static_cast<T*>(a.dst) + (long)n * 3 * plane + (long)yy * row_w + xx;
    d[0] = (T)(inside ? form_of<FORM>(v0, a.r, a.m0, a.s0) : a.pad);
    d[plane] = (T)(inside ? form_of<FORM>(v1, a.r, a.m1, a.s1) : a.pad);
    d[2 * plane] = (T)(inside ? form_of<FORM>(v2, a.r, a.m2, a.s2) : a.pad);
  }
}

template <int AXIS, bool CANVAS>
void launch_pass_as(const PassArgs& a, int N, int form, int out_f16, hipStream_t st) {
  const int rows = CANVAS ? a.cv_h : a.out_h, row_w = CANVAS ? a.cv_w : a.out_w;
  const dim3 grid((unsigned)((row_w + PASS_THREADS - 1) / PASS_THREADS), (unsigned)rows, (unsigned)N);
  const dim3 block(PASS_THREADS);
  if (form == LGD_RESAMPLE_U8)
    hipLaunchKernelGGL((resample_pass_kernel<AXIS, LGD_RESAMPLE_U8, uint8_t, CANVAS>), grid, block, 0, st, a);
  else if (form == LGD_RESAMPLE_AFFINE && !out_f16)
    hipLaunchKernelGGL((resample_pass_kernel<AXIS, LGD_RESAMPLE_AFFINE, float, CANVAS>), grid, block, 0, st, a);
  else if (form == LGD_RESAMPLE_AFFINE)
    hipLaunchKernelGGL((resample_pass_kernel<AXIS, LGD_RESAMPLE_AFFINE, half_t, CANVAS>), grid, block, 0, st, a);
  else if (!out_f16)
    hipLaunchKernelGGL((resample_pass_kernel<AXIS, LGD_RESAMPLE_UNIT, float, CANVAS>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((resample_pass_kernel<AXIS, LGD_RESAMPLE_UNIT, half_t, CANVAS>), grid, block, 0, st, a);
}

// canvas: only the pass that writes `out` is asked for it; the pass into scratch is always dense
template <int AXIS>
void launch_pass(const PassArgs& a, int N, int form, int out_f16, bool canvas, hipStream_t st) {
  if (canvas)
    launch_pass_as<AXIS, true>(a, N, form, out_f16, st);
  else
    launch_pass_as<AXIS, false>(a, N, form, out_f16, st);
}

}  // namespace

extern "C" int lgd_resample_plan(int in, int out, int filter, int32_t* coef, int32_t* bounds, int* width) {
  if (in <= 0 || out <= 0 || support_of(filter) == 0.0) return LGD_ERR_ARG;
  if ((coef == nullptr) != (bounds == nullptr) || (!coef && !width)) return LGD_ERR_ARG;
  if (lgd_contract::misaligned(coef, 4) || lgd_contract::misaligned(bounds, 4) || lgd_contract::misaligned(width, 4))
    return LGD_ERR_ARG;
  if (in > MAX_SIDE || out > MAX_SIDE) return LGD_ERR_UNSUPPORTED;
  const int ksize = width_of(in, out, filter);
  if (width) *width = ksize;
  if (!coef) return LGD_OK;
  if (lgd_contract::overlaps(coef, (int64_t)out * ksize * 4, bounds, (int64_t)out * 8)) return LGD_ERR_ARG;
  // precompute_coeffs with the box (0, in)
  double scale, filterscale;
  filterscale = scale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = support_of(filter) * filterscale;
  const double ss = 1.0 / filterscale;
  double* kk = new double[ksize];
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    int x;
    for (x = 0; x < xmax; ++x) {
      const double w = weight_of(filter, (x + xmin - center + 0.5) * ss);
      kk[x] = w;
      ww += w;
    }
    for (x = 0; x < xmax; ++x)
      if (ww != 0.0) kk[x] /= ww;
    for (; x < ksize; ++x) kk[x] = 0;
    // normalize_coeffs_8bpc
    int32_t* k = coef + (long)xx * ksize;
    for (x = 0; x < ksize; ++x)
      k[x] = kk[x] < 0 ? (int)(-0.5 + kk[x] * (1 << PRECISION_BITS)) : (int)(0.5 + kk[x] * (1 << PRECISION_BITS));
    bounds[xx * 2] = xmin;
    bounds[xx * 2 + 1] = xmax;
  }
  delete[] kk;
  return LGD_OK;
}

namespace {

// Both entries: canvas = false is lgd_resample_u8 (CH, CW and pad are H, W and 0 and are not read by a kernel).
int resample_run(const uint8_t* src, int N, int h, int w, int H, int W, int filter, const int32_t* coef_x,
                 const int32_t* bounds_x, int width_x, int rows_x, const int32_t* coef_y, const int32_t* bounds_y,
                 int width_y, int rows_y, uint8_t* scratch, int form, int out_f16, float r, float m0, float m1, float m2,
                 float s0, float s1, float s2, void* out, bool canvas, int CH, int CW, float pad, void* stream) {
  using lgd_contract::misaligned;
  using lgd_contract::overlaps;
  if (!src || !out) return LGD_ERR_ARG;
  if (N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return LGD_ERR_ARG;
  if (support_of(filter) == 0.0) return LGD_ERR_ARG;
  if (form != LGD_RESAMPLE_U8 && form != LGD_RESAMPLE_AFFINE && form != LGD_RESAMPLE_UNIT) return LGD_ERR_ARG;
  if (out_f16 != 0 && out_f16 != 1) return LGD_ERR_ARG;
  if (canvas) {
    if (CH < H || CW < W || !isfinite(pad)) return LGD_ERR_ARG;
    if (form == LGD_RESAMPLE_U8 && !(pad >= 0.f && pad <= 255.f && pad == (float)(int)pad)) return LGD_ERR_ARG;
  }
  if (N > MAX_N || h > MAX_SIDE || w > MAX_SIDE || H > MAX_SIDE || W > MAX_SIDE) return LGD_ERR_UNSUPPORTED;
  if (canvas && (CH > MAX_SIDE || CW > MAX_SIDE)) return LGD_ERR_UNSUPPORTED;
  const bool need_h = W != w, need_v = H != h;
  if (need_h) {
    if (!coef_x || !bounds_x || misaligned(coef_x, 4) || misaligned(bounds_x, 4)) return LGD_ERR_ARG;
    if (width_x != width_of(w, W, filter) || rows_x != W) return LGD_ERR_ARG;
  }
  if (need_v) {
    if (!coef_y || !bounds_y || misaligned(coef_y, 4) || misaligned(bounds_y, 4)) return LGD_ERR_ARG;
    if (width_y != width_of(h, H, filter) || rows_y != H) return LGD_ERR_ARG;
  }
  if (need_h && need_v && !scratch) return LGD_ERR_ARG;
  const int64_t in_bytes = (int64_t)N * h * w * 3, mid_bytes = (int64_t)N * h * W * 3;
  const int elem = form == LGD_RESAMPLE_U8 ? 1 : (out_f16 ? 2 : 4);
  const int64_t out_bytes = (int64_t)N * CH * CW * 3 * elem;
  if (misaligned(out, elem)) return LGD_ERR_ARG;
  if (overlaps(out, out_bytes, src, in_bytes)) return LGD_ERR_ARG;
  if (need_h && need_v && (overlaps(out, out_bytes, scratch, mid_bytes) || overlaps(scratch, mid_bytes, src, in_bytes)))
    return LGD_ERR_ARG;
  if (need_h && (overlaps(out, out_bytes, coef_x, (int64_t)W * width_x * 4) || overlaps(out, out_bytes, bounds_x, (int64_t)W * 8)))
    return LGD_ERR_ARG;
  if (need_v && (overlaps(out, out_bytes, coef_y, (int64_t)H * width_y * 4) || overlaps(out, out_bytes, bounds_y, (int64_t)H * 8)))
    return LGD_ERR_ARG;
  (void)hipGetLastError();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  PassArgs a;
  a.r = r, a.m0 = m0, a.m1 = m1, a.m2 = m2, a.s0 = s0, a.s1 = s1, a.s2 = s2;
  a.src = src, a.in_h = h, a.in_w = w;
  a.coef = nullptr, a.bounds = nullptr, a.ksize = 0;
  a.cv_h = CH, a.cv_w = CW, a.pad = pad;
  if (need_h) {
    a.coef = coef_x, a.bounds = bounds_x, a.ksize = width_x;
    a.out_h = h, a.out_w = W;
    a.dst = need_v ? static_cast<void*>(scratch) : out;
    launch_pass<AXIS_H>(a, N, need_v ? LGD_RESAMPLE_U8 : form, out_f16, canvas && !need_v, st);
    a.src = scratch, a.in_w = W;
  }
  if (need_v) {
    a.coef = coef_y, a.bounds = bounds_y, a.ksize = width_y;
    a.out_h = H, a.out_w = W, a.dst = out;
    launch_pass<AXIS_V>(a, N, form, out_f16, canvas, st);
  }
  if (!need_h && !need_v) {
    a.out_h = H, a.out_w = W, a.dst = out;
    launch_pass<AXIS_NONE>(a, N, form, out_f16, canvas, st);
  }
  return lgd_check_launch();
}

}  // namespace

extern "C" int lgd_resample_u8(const uint8_t* src, int N, int h, int w, int H, int W, int filter, const int32_t* coef_x,
                               const int32_t* bounds_x, int width_x, int rows_x, const int32_t* coef_y,
                               const int32_t* bounds_y, int width_y, int rows_y, uint8_t* scratch, int form,
                               int out_f16, float r, float m0, float m1, float m2, float s0, float s1, float s2,
                               void* out, void* stream) {
  return resample_run(src, N, h, w, H, W, filter, coef_x, bounds_x, width_x, rows_x, coef_y, bounds_y, width_y, rows_y,
                      scratch, form, out_f16, r, m0, m1, m2, s0, s1, s2, out, false, H, W, 0.f, stream);
}

extern "C" int lgd_resample_canvas_u8(const uint8_t* src, int N, int h, int w, int H, int W, int filter,
                                      const int32_t* coef_x, const int32_t* bounds_x, int width_x, int rows_x,
                                      const int32_t* coef_y, const int32_t* bounds_y, int width_y, int rows_y,
                                      uint8_t* scratch, int form, int out_f16, float r, float m0, float m1, float m2,
                                      float s0, float s1, float s2, void* out, int CH, int CW, float pad, void* stream) {
  return resample_run(src, N, h, w, H, W, filter, coef_x, bounds_x, width_x, rows_x, coef_y, bounds_y, width_y, rows_y,
                      scratch, form, out_f16, r, m0, m1, m2, s0, s1, s2, out, true, CH, CW, pad, stream);
}
