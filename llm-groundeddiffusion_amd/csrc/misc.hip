// Small HBM/latency-bound pieces of the denoising loop: boundary convolutions (4 <-> C channels,
// NCHW fp32 <-> channels-last fp16), elementwise gradient helpers, and the fused per-step update
// (classifier-free guidance + DDIM + frozen-mask blend).
#include "common.h"
#include "contract.h"
#include "../../include/lgd_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// conv_in: NCHW fp32 (B,Cin<=8,L,L) -> [B][L*L][Cout] fp16.   w: [Cout][9*Cin] (ky,kx,ci).
// Workgroup = 32 pixels; weights transposed into LDS as [k][Cout] so that lanes run over output
// channels (coalesced stores, conflict-free LDS reads); the 9*Cin input patch of a pixel is
// broadcast.
// ---------------------------------------------------------------------------------------------
constexpr int CI_PIX = 32;
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x,
                                                       const half_t* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       half_t* __restrict__ y, int B, int Cin,
                                                       int L, int Cout) {
  extern __shared__ __attribute__((aligned(16))) char dyn_smem[];
  const int K = 9 * Cin;
  half_t* wT = reinterpret_cast<half_t*>(dyn_smem);                 // [K][Cout]
  float* patch = reinterpret_cast<float*>(dyn_smem + (size_t)((K * Cout * 2 + 15) & ~15));  // [32][K]
  const int HW = L * L;
  const long pix0 = (long)blockIdx.x * CI_PIX;
  for (int i = threadIdx.x; i < K * Cout; i += 256) {
    int co = i / K, k = i - co * K;
    wT[k * Cout + co] = w[i];
  }
  for (int i = threadIdx.x; i < CI_PIX * K; i += 256) {
    int p = i / K, k = i - p * K;
    long pix = pix0 + p;
    float v = 0.f;
    if (pix < (long)B * HW) {
      int b = (int)(pix / HW), rem = (int)(pix - (long)b * HW);
      int oy = rem / L, ox = rem - oy * L;
      int tap = k / Cin, ci = k - tap * Cin;
      int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
      if (iy >= 0 && iy < L && ix >= 0 && ix < L) v = x[(((long)b * Cin + ci) * L + iy) * L + ix];
    }
    patch[i] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int pp = wid; pp < CI_PIX; pp += 4) {
    long pix = pix0 + pp;
    if (pix >= (long)B * HW) break;
    const float* pt = patch + pp * K;
    for (int co = lane; co < Cout; co += 64) {
      float acc = bias ? bias[co] : 0.f;
      for (int k = 0; k < K; ++k) acc += pt[k] * (float)wT[k * Cout + co];
      y[pix * Cout + co] = (half_t)acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// conv_out: [B][L*L][Cin] fp16 -> NCHW fp32 (B,Cout<=8,L,L), 3x3 pad 1.  w: [Cout][9*Cin].
// One wave per output pixel; the 9*Cin reduction is spread over the lanes in 8-channel vectors and
// closed with shuffles.  Also used as conv_in's input gradient with flipped/transposed weights.
// ---------------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void conv_out_kernel(const half_t* __restrict__ x,
                                                        const half_t* __restrict__ w,
                                                        const float* __restrict__ bias,
                                                        float* __restrict__ y, int B, int Cin, int L,
                                                        float out_scale) {
  const int lane = threadIdx.x & 63;
  const long pix = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int HW = L * L;
  if (pix >= (long)B * HW) return;
  const int b = (int)(pix / HW), rem = (int)(pix - (long)b * HW);
  const int oy = rem / L, ox = rem - oy * L;
  const int vpt = Cin / 8;  // vectors per tap
  const int nvec = 9 * vpt;
  float acc[COUT];
#pragma unroll
  for (int c = 0; c < COUT; ++c) acc[c] = 0.f;
  for (int v = lane; v < nvec; v += 64) {
    int tap = v / vpt, cv = v - tap * vpt;
    int iy = oy + tap / 3 - 1, ix = ox + tap % 3 - 1;
    if (iy < 0 || iy >= L || ix < 0 || ix >= L) continue;
    half8_t hx = *reinterpret_cast<const half8_t*>(x + ((long)b * HW + iy * L + ix) * Cin + cv * 8);
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
      half8_t hw = *reinterpret_cast<const half8_t*>(w + (long)c * 9 * Cin + tap * Cin + cv * 8);
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += (float)hx[e] * (float)hw[e];
      acc[c] += s;
    }
  }
#pragma unroll
  for (int c = 0; c < COUT; ++c) acc[c] = wave_sum(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < COUT; ++c)
      y[(((long)b * COUT + c) * L + oy) * L + ox] = (acc[c] + (bias ? bias[c] : 0.f)) * out_scale;
  }
}

// NCHW fp32 (B, C <= 8, HW) -> channels-last fp16 [B*HW][8]: channels 0..C-1 = fp16(x), C..2C-1 = fp16(x - fp16(x))
// when they fit, the rest zero: the 4-channel latents become an
// 8-channel map, the narrowest the implicit-GEMM convolution takes (one 16-byte vector per pixel and tap), so that
// conv_in runs on the matrix cores (K = 72) instead of conv_in_kernel's LDS-bound scalar loop.
__global__ __launch_bounds__(256) void nchw_to_nhwc8_kernel(const float* __restrict__ x, half_t* __restrict__ y,
                                                             int C, long HW, long total) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const long b = i / HW, p = i - b * HW;
    half8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < C) {
        const float v = x[(b * C + c) * HW + p];
        const half_t hi = (half_t)v;
        o[c] = hi;
        // the spare channels carry the rounding remainder (the filter is duplicated over them by the caller):
        // hi + lo reproduces the fp32 latent to 2^-22, so the fp16 operand format costs conv_in no input precision
        if (2 * C <= 8 && c + C < 8) o[c + C] = (half_t)(v - (float)hi);
      }
    reinterpret_cast<half8_t*>(y)[i] = o;
  }
}

// ---------------------------------------------------------------------------------------------
// elementwise helpers (16-byte vectors, grid-stride)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_kernel(const half_t* a, const half_t* b, half_t* y,
                                                   long nvec) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < nvec; i += gridDim.x * 256L) {
    half8_t x0 = reinterpret_cast<const half8_t*>(a)[i];
    half8_t x1 = reinterpret_cast<const half8_t*>(b)[i];
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)x0[e] + (float)x1[e]);
    reinterpret_cast<half8_t*>(y)[i] = o;
  }
}
__global__ __launch_bounds__(256) void scale_kernel(const half_t* a, half_t* y, float alpha,
                                                     long nvec) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < nvec; i += gridDim.x * 256L) {
    half8_t x0 = reinterpret_cast<const half8_t*>(a)[i];
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)x0[e] * alpha);
    reinterpret_cast<half8_t*>(y)[i] = o;
  }
}

// y = x * sigmoid(1.702 x): the "quick GELU" of the CLIP text encoder's MLP ([ext] transformers CLIPMLP).
__global__ __launch_bounds__(256) void quick_gelu_kernel(const half_t* a, half_t* y, long nvec) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < nvec; i += gridDim.x * 256L) {
    half8_t x0 = reinterpret_cast<const half8_t*>(a)[i];
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (float)x0[e];
      o[e] = (half_t)(x / (1.f + __expf(-1.702f * x)));
    }
    reinterpret_cast<half8_t*>(y)[i] = o;
  }
}

// GEGLU forward on a stored pre-activation (the grad-enabled guidance pass keeps h for backward;
// the no-grad pass uses the fused GEMM epilogue instead).  h packed [16 value | 16 gate] blocks.
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const half_t* __restrict__ h,
                                                         half_t* __restrict__ y, long rows, int n) {
  const long nvec_row = n / 8;
  const long total = rows * nvec_row;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    long r = i / nvec_row;
    int j = (int)(i - r * nvec_row) * 8;
    long base = r * 2L * n + (j / 16) * 32 + (j % 16);
    half8_t v = *reinterpret_cast<const half8_t*>(h + base);
    half8_t g = *reinterpret_cast<const half8_t*>(h + base + 16);
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)v[e] * gelu_f((float)g[e]));
    *reinterpret_cast<half8_t*>(y + r * (long)n + j) = o;
  }
}

// GEGLU backward.  h packed as [.. 16 value | 16 gate ..] blocks (the layout the GEMM epilogue
// consumes); y[j] = v[j]*gelu(g[j]);  gv = gy*gelu(g), gg = gy*v*gelu'(g).
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const half_t* __restrict__ h,
                                                         const half_t* __restrict__ gy,
                                                         half_t* __restrict__ gh, long rows, int n) {
  const long nvec_row = n / 8;
  const long total = rows * nvec_row;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    long r = i / nvec_row;
    int j = (int)(i - r * nvec_row) * 8;           // output column (multiple of 8, inside a 16-block)
    long base = r * 2L * n + (j / 16) * 32 + (j % 16);
    half8_t v = *reinterpret_cast<const half8_t*>(h + base);
    half8_t g = *reinterpret_cast<const half8_t*>(h + base + 16);
    half8_t dy = *reinterpret_cast<const half8_t*>(gy + r * (long)n + j);
    half8_t ov, og;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float gf = (float)g[e], d = (float)dy[e];
      ov[e] = (half_t)(d * gelu_f(gf));
      og[e] = (half_t)(d * (float)v[e] * gelu_grad_f(gf));
    }
    *reinterpret_cast<half8_t*>(gh + base) = ov;
    *reinterpret_cast<half8_t*>(gh + base + 16) = og;
  }
}

__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const half_t* __restrict__ gy,
                                                              half_t* __restrict__ gx, int B, int H,
                                                              int W, int C) {
  const long nvec = C / 8;
  const long total = (long)B * H * W * nvec;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    long pix = i / nvec;
    int cv = (int)(i - pix * nvec);
    int b = (int)(pix / (H * W)), rem = (int)(pix - (long)b * H * W);
    int y = rem / W, x = rem - y * W;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        long src = ((long)b * 2 * H + 2 * y + dy) * 2 * W + 2 * x + dx;
        half8_t v = *reinterpret_cast<const half8_t*>(gy + src * C + cv * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
      }
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)acc[e];
    *reinterpret_cast<half8_t*>(gx + pix * C + cv * 8) = o;
  }
}

// Row softmax of scale*x (fp16 in/out, fp32 math), one wave per row; used by the single-head
// 512-channel attention of the VAE decoder mid block (the flash kernel covers head dims <= 160).
// (x and y may be the same buffer: every lane rewrites only elements it has read itself)
__global__ __launch_bounds__(256) void softmax_rows_kernel(const half_t* x, half_t* y, long rows, int n,
                                                            float scale) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const half_t* xr = x + row * n;
  half_t* yr = y + row * n;
  const int nvec = n / 8;
  float mx = -1.0e30f;
  for (int v = lane; v < nvec; v += 64) {
    half8_t h = *reinterpret_cast<const half8_t*>(xr + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, (float)h[e] * scale);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int v = lane; v < nvec; v += 64) {
    half8_t h = *reinterpret_cast<const half8_t*>(xr + v * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += __expf((float)h[e] * scale - mx);
  }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int v = lane; v < nvec; v += 64) {
    half8_t h = *reinterpret_cast<const half8_t*>(xr + v * 8);
    half8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)(__expf((float)h[e] * scale - mx) * inv);
    *reinterpret_cast<half8_t*>(yr + v * 8) = o;
  }
}

// per-step fused update, see lgd_hip.h
__global__ __launch_bounds__(256) void cfg_ddim_kernel(
    const float* __restrict__ eps, const float* __restrict__ x, float* __restrict__ x_out,
    const float* __restrict__ coef_table, const int32_t* __restrict__ dyn,
    const float* __restrict__ frozen_ref, const float* __restrict__ mask,
    float* __restrict__ hist, int B, int CHW, int HW) {
  const int step = dyn[0];
  const int frozen_steps = dyn[1];
  const float a_t = coef_table[step * 4 + 0], a_p = coef_table[step * 4 + 1];
  const float gs = coef_table[step * 4 + 2];
  const bool vpred = coef_table[step * 4 + 3] != 0.f;
  const float sa = sqrtf(a_t), sb = sqrtf(1.f - a_t), pa = sqrtf(a_p), pb = sqrtf(1.f - a_p);
  const long n = (long)B * CHW;
  const bool blend = frozen_ref && mask && step < frozen_steps;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    float eu = eps[i], ec = eps[n + i];
    float m = eu + gs * (ec - eu);
    float xv = x[i];
    float x0, e;
    if (vpred) {
      x0 = sa * xv - sb * m;
      e = sa * m + sb * xv;
    } else {
      e = m;
      x0 = (xv - sb * e) / sa;
    }
    float xn = pa * x0 + pb * e;
    if (blend) {
      int b = (int)(i / CHW);
      int p = (int)(i % HW);
      float mk = mask[(long)b * HW + p];
      xn = frozen_ref[(long)(step + 1) * n + i] * mk + xn * (1.f - mk);
    }
    x_out[i] = xn;
    if (hist) hist[(long)(step + 1) * n + i] = xn;
  }
}

// Classifier-free guidance + one step of a LINEAR MULTISTEP sampler (DPM-Solver++ 2M and anything else whose update
// is linear in the latents, the current data prediction and the previous one) + frozen-mask blend + history:
//     m  = eu + gs (ec - eu)                  model output under CFG
//     x0 = c0 x + c1 m                        data prediction (epsilon: 1/alpha_t, -sigma_t/alpha_t; v: alpha_t, -sigma_t)
//     x' = A x + B x0 + C x0_prev             first-order steps have C = 0 (x0_prev is not read)
//     x0_prev <- x0
// coef rows: fp32 [T][8] = {c0, c1, A, B, C, guidance_scale, -, -}.
__global__ __launch_bounds__(256) void cfg_multistep_kernel(
    const float* __restrict__ eps, const float* __restrict__ x, float* __restrict__ x_out, float* __restrict__ x0_prev,
    const float* __restrict__ coef_table, const int32_t* __restrict__ dyn, const float* __restrict__ frozen_ref,
    const float* __restrict__ mask, float* __restrict__ hist, int B, int CHW, int HW) {
  const int step = dyn[0];
  const int frozen_steps = dyn[1];
  const float* c = coef_table + step * 8;
  const float c0 = c[0], c1 = c[1], A = c[2], Bc = c[3], Cc = c[4], gs = c[5];
  const long n = (long)B * CHW;
  const bool blend = frozen_ref && mask && step < frozen_steps;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const float eu = eps[i], ec = eps[n + i];
    const float m = eu + gs * (ec - eu);
    const float xv = x[i];
    const float x0 = c0 * xv + c1 * m;
    float xn = A * xv + Bc * x0;
    if (Cc != 0.f) xn += Cc * x0_prev[i];
    x0_prev[i] = x0;
    if (blend) {
      const int b = (int)(i / CHW);
      const int p = (int)(i % HW);
      const float mk = mask[(long)b * HW + p];
      xn = frozen_ref[(long)(step + 1) * n + i] * mk + xn * (1.f - mk);
    }
    x_out[i] = xn;
    if (hist) hist[(long)(step + 1) * n + i] = xn;
  }
}

// Classifier-free guidance + one evaluation of PLMS ([ext] diffusers PNDMScheduler, skip_prk_steps): see lgd_hip.h.
// Four fp32 lanes per thread (16-byte loads), grid-stride over n/4 vectors; everything that varies by evaluation is in
// coefficient row dyn[0]:  {w_m, w_ring0, w_ring1, w_ring2, a, b, gs, push slot (-1: none), src = cur, save cur, ...}.
// A ring slot is read only where its weight is non-zero, and written (push) after it was read.
__global__ __launch_bounds__(256) void cfg_plms_kernel(
    const float* __restrict__ eps, const float* x, float* x_out, float* __restrict__ ets,
    float* __restrict__ cur, const float* __restrict__ coef_table, const int32_t* __restrict__ dyn,
    float* __restrict__ hist, long n) {
  const int step = dyn[0];
  const float* c = coef_table + step * 16;
  const float wm = c[0], w0 = c[1], w1 = c[2], w2 = c[3], A = c[4], Bc = c[5], gs = c[6];
  const int push = (int)c[7];
  const bool from_cur = c[8] != 0.f, save_cur = c[9] != 0.f;
  const long nv = n >> 2;
  const f32x4* eu4 = reinterpret_cast<const f32x4*>(eps);
  const f32x4* ec4 = reinterpret_cast<const f32x4*>(eps + n);
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  f32x4* r0 = reinterpret_cast<f32x4*>(ets);
  f32x4* r1 = reinterpret_cast<f32x4*>(ets + n);
  f32x4* r2 = reinterpret_cast<f32x4*>(ets + 2 * n);
  f32x4* cur4 = reinterpret_cast<f32x4*>(cur);
  for (long v = blockIdx.x * 256L + threadIdx.x; v < nv; v += gridDim.x * 256L) {
    const f32x4 eu = eu4[v], ec = ec4[v];
    const f32x4 m = eu + gs * (ec - eu);
    f32x4 comb = wm * m;
    if (w0 != 0.f) comb += w0 * r0[v];
    if (w1 != 0.f) comb += w1 * r1[v];
    if (w2 != 0.f) comb += w2 * r2[v];
    if (push == 0) r0[v] = m;
    else if (push == 1) r1[v] = m;
    else if (push == 2) r2[v] = m;
    const f32x4 xv = x4[v];
    const f32x4 src = from_cur ? cur4[v] : xv;
    if (save_cur) cur4[v] = xv;
    const f32x4 xn = A * src + Bc * comb;
    reinterpret_cast<f32x4*>(x_out)[v] = xn;
    if (hist) reinterpret_cast<f32x4*>(hist + (long)(step + 1) * n)[v] = xn;
  }
}

// Classifier-free guidance + one step of the order-4 linear multistep sampler in sigma space ([ext] diffusers
// LMSDiscreteScheduler) + frozen-mask blend + history: see lgd_hip.h.  Four fp32 lanes per thread (16-byte accesses),
// grid-stride over n/4 vectors; coefficient row dyn[0] = {c0, c1, 1/sigma, w_0..w_3 by ring slot, gs, slot, ...}.  The
// host has permuted the LMS coefficients onto slots.  This step's own slot is not read (its weight multiplies the
// fresh derivative); another slot is read only where its weight is non-zero, and the own slot is written after them.
__global__ __launch_bounds__(256) void cfg_lms_kernel(
    const float* __restrict__ eps, const float* x, float* x_out, float* __restrict__ ring,
    const float* __restrict__ coef_table, const int32_t* __restrict__ dyn, const float* __restrict__ frozen_ref,
    const float* __restrict__ mask, float* __restrict__ hist, long n, int CHW, int HW) {
  const int step = dyn[0];
  const int frozen_steps = dyn[1];
  const float* c = coef_table + step * 16;
  const float c0 = c[0], c1 = c[1], inv_sigma = c[2], gs = c[7];
  const int slot = (int)c[8] & 3;  // a slot outside the ring cannot address past it
  const float w0 = slot == 0 ? 0.f : c[3], w1 = slot == 1 ? 0.f : c[4], w2 = slot == 2 ? 0.f : c[5],
              w3 = slot == 3 ? 0.f : c[6];
  const float w_self = c[3 + slot];
  const bool blend = frozen_ref && mask && step < frozen_steps;
  const long nv = n >> 2;
  const f32x4* eu4 = reinterpret_cast<const f32x4*>(eps);
  const f32x4* ec4 = reinterpret_cast<const f32x4*>(eps + n);
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  f32x4* r0 = reinterpret_cast<f32x4*>(ring);
  f32x4* r1 = reinterpret_cast<f32x4*>(ring + n);
  f32x4* r2 = reinterpret_cast<f32x4*>(ring + 2 * n);
  f32x4* r3 = reinterpret_cast<f32x4*>(ring + 3 * n);
  f32x4* rs = reinterpret_cast<f32x4*>(ring + (long)slot * n);
  for (long v = blockIdx.x * 256L + threadIdx.x; v < nv; v += gridDim.x * 256L) {
    const f32x4 eu = eu4[v], ec = ec4[v];
    const f32x4 m = eu + gs * (ec - eu);
    const f32x4 xv = x4[v];
    const f32x4 x0 = c0 * xv + c1 * m;
    const f32x4 d = (xv - x0) * inv_sigma;
    f32x4 xn = xv + w_self * d;
    if (w0 != 0.f) xn += w0 * r0[v];
    if (w1 != 0.f) xn += w1 * r1[v];
    if (w2 != 0.f) xn += w2 * r2[v];
    if (w3 != 0.f) xn += w3 * r3[v];
    rs[v] = d;
    if (blend) {
      // CHW % 4 == 0 is not given, HW % 4 == 0 neither: the four lanes may straddle an image or a mask row
      const long e = v << 2;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long i = e + k;
        const float mk = mask[(i / CHW) * HW + (i % HW)];
        xn[k] = frozen_ref[(long)(step + 1) * n + i] * mk + xn[k] * (1.f - mk);
      }
    }
    reinterpret_cast<f32x4*>(x_out)[v] = xn;
    if (hist) reinterpret_cast<f32x4*>(hist + (long)(step + 1) * n)[v] = xn;
  }
}

// One MultiDiffusion step over P region prompts (generation/multidiffusion.py of the reference, one 512x512 view,
// indep_uncond, no normalization): see lgd_hip.h.  Four fp32 lanes of one latent plane per thread (16-byte accesses;
// HW % 4 == 0, so the four lanes share one mask row), one wave per workgroup so that the 16K-element SD latent spreads
// over 64 CUs.  A thread reads x_k (the UNet input rows it wrote one step earlier) and the CFG pair of every prompt in
// prompt order and owns its output elements: no atomics, deterministic.  The DDIM arithmetic is cfg_ddim_kernel's,
// lane by lane, so that one prompt with mask 1 reproduces the plain CFG + DDIM step bit for bit.
__device__ __forceinline__ float md_ddim_of(float m, float xv, bool vpred, float sa, float sb, float pa, float pb) {
  float x0, e;
  if (vpred) {
    x0 = sa * xv - sb * m;
    e = sa * m + sb * xv;
  } else {
    e = m;
    x0 = (xv - sb * e) / sa;
  }
  return pa * x0 + pb * e;
}

__device__ __forceinline__ float md_ddim(float eu, float ec, float xv, float gs, bool vpred, float sa, float sb,
                                         float pa, float pb) {
  return md_ddim_of(eu + gs * (ec - eu), xv, vpred, sa, sb, pa, pb);
}

__global__ __launch_bounds__(64) void multidiffusion_step_kernel(
    const float* __restrict__ eps, float* __restrict__ x_in, float* __restrict__ latent,
    const float* __restrict__ masks, const float* __restrict__ bg, const float* __restrict__ noise,
    const int32_t* __restrict__ picks, const float* __restrict__ coef_table, const int32_t* __restrict__ dyn,
    float* __restrict__ hist, int P, int Pp, int HW, long n, int n_steps, int n_boot, int prep) {
  const int step = dyn[0];
  if (step < 0 || step >= n_steps) return;
  const long v = blockIdx.x * 64L + threadIdx.x;
  if (v >= (n >> 2)) return;
  const long e = v << 2;
  const long p = e % HW;
  f32x4 acc;
  int next = step;
  if (prep) {
    acc = reinterpret_cast<const f32x4*>(latent)[v];
  } else {
    const float* c = coef_table + step * 4;
    const float a_t = c[0], a_p = c[1], gs = c[2];
    const bool vpred = c[3] != 0.f;
    const float sa = sqrtf(a_t), sb = sqrtf(1.f - a_t), pa = sqrtf(a_p), pb = sqrtf(1.f - a_p);
    for (int k = 0; k < P; ++k) {
      const f32x4 eu = reinterpret_cast<const f32x4*>(eps + (long)k * n)[v];
      const f32x4 ec = reinterpret_cast<const f32x4*>(eps + (long)(Pp + k) * n)[v];
      const f32x4 xv = reinterpret_cast<const f32x4*>(x_in + (long)k * n)[v];
      const f32x4 mk = *reinterpret_cast<const f32x4*>(masks + (long)k * HW + p);
      f32x4 d;
      d.x = md_ddim(eu.x, ec.x, xv.x, gs, vpred, sa, sb, pa, pb);
      d.y = md_ddim(eu.y, ec.y, xv.y, gs, vpred, sa, sb, pa, pb);
      d.z = md_ddim(eu.z, ec.z, xv.z, gs, vpred, sa, sb, pa, pb);
      d.w = md_ddim(eu.w, ec.w, xv.w, gs, vpred, sa, sb, pa, pb);
      acc = k == 0 ? mk * d : acc + mk * d;
    }
    reinterpret_cast<f32x4*>(latent)[v] = acc;
    if (hist) reinterpret_cast<f32x4*>(hist + (long)(step + 1) * n)[v] = acc;
    next = step + 1;
  }
  if (next >= n_steps) return;
  // UNet input of step `next`: torch.cat([x_0 .. x_{Pp-1}] * 2), rows 1..P-1 bootstrapped while next < n_boot
  const bool boot = next < n_boot && P > 1;
  float sa = 0.f, sb = 0.f;
  f32x4 nz = {0.f, 0.f, 0.f, 0.f};
  if (boot) {
    const float a_n = coef_table[next * 4];
    sa = sqrtf(a_n);
    sb = sqrtf(1.f - a_n);
    nz = reinterpret_cast<const f32x4*>(noise)[v];
  }
  for (int k = 0; k < Pp; ++k) {
    f32x4 x = acc;
    if (boot && k >= 1 && k < P) {
      int pk = picks[(long)next * (P - 1) + (k - 1)];
      pk = pk < 0 ? 0 : (pk >= n_boot ? n_boot - 1 : pk);
      const f32x4 g = reinterpret_cast<const f32x4*>(bg + (long)pk * n)[v];
      const f32x4 mk = *reinterpret_cast<const f32x4*>(masks + (long)k * HW + p);
      f32x4 b;
      b.x = mk.x >= 0.5f ? 1.f : 0.f;
      b.y = mk.y >= 0.5f ? 1.f : 0.f;
      b.z = mk.z >= 0.5f ? 1.f : 0.f;
      b.w = mk.w >= 0.5f ? 1.f : 0.f;
      const f32x4 noisy = sa * g + sb * nz;                   // DDIMScheduler.add_noise(bg, noise, t_next)
      x = acc * b + noisy * (1.f - b);
    }
    reinterpret_cast<f32x4*>(x_in + (long)k * n)[v] = x;
    reinterpret_cast<f32x4*>(x_in + (long)(Pp + k) * n)[v] = x;
  }
}

// MultiDiffusion over V overlapping 64x64 views of a latent panorama [C][Hp][Wp] (MultiDiffusion.generate of the
// reference, generation/multidiffusion.py:210-280; window 64, stride 8): see lgd_hip.h.  The UNet batch holds a chunk of
// whole views [v0, v0 + nv): view j of the chunk owns rows j*Pp + k (uncond half) and nvc*Pp + j*Pp + k (cond half).
//
// prep: one thread = four consecutive fp32 lanes of one plane of one view of the chunk; it writes the UNet input rows of
// step dyn[0] (the bootstrapping blend is multidiffusion_step_kernel's expression, with panorama-sized noise and masks).
constexpr int MD_WIN = 64, MD_STRIDE = 8, MD_WHW = MD_WIN * MD_WIN;

__global__ __launch_bounds__(64) void multidiffusion_views_prep_kernel(
    float* __restrict__ x_in, const float* __restrict__ latent, const float* __restrict__ masks,
    const float* __restrict__ bg, const float* __restrict__ noise, const int32_t* __restrict__ picks,
    const float* __restrict__ coef_table, const int32_t* __restrict__ dyn, int P, int Pp, int C, int Hp, int Wp,
    int nbw, int V, int v0, int nv, int nvc, int n_steps, int n_boot) {
  const int step = dyn[0];
  if (step < 0 || step >= n_steps) return;
  const long t = blockIdx.x * 64L + threadIdx.x;
  const long per_view = (long)C * (MD_WHW / 4);
  if (t >= nv * per_view) return;
  const int j = (int)(t / per_view);
  const int r = (int)(t - j * per_view);
  const int c = r / (MD_WHW / 4);
  const int p = (r - c * (MD_WHW / 4)) << 2;                 // first of four lanes inside the 64x64 window
  const int v = v0 + j;
  const int y = (v / nbw) * MD_STRIDE + p / MD_WIN, x = (v % nbw) * MD_STRIDE + p % MD_WIN;
  const long plane = (long)Hp * Wp;
  const long q = (long)y * Wp + x;                           // panorama position of the four lanes (one row: x % 4 == 0)
  const f32x4 acc = *reinterpret_cast<const f32x4*>(latent + c * plane + q);
  const bool boot = step < n_boot && P > 1;
  float sa = 0.f, sb = 0.f;
  f32x4 nz = {0.f, 0.f, 0.f, 0.f};
  if (boot) {
    const float a_n = coef_table[step * 4];
    sa = sqrtf(a_n);
    sb = sqrtf(1.f - a_n);
    nz = *reinterpret_cast<const f32x4*>(noise + c * plane + q);
  }
  const long row = (long)C * MD_WHW;
  const long in_row = (long)c * MD_WHW + p;
  for (int k = 0; k < Pp; ++k) {
    f32x4 xk = acc;
    if (boot && k >= 1 && k < P) {
      int pk = picks[((long)step * V + v) * (P - 1) + (k - 1)];
      pk = pk < 0 ? 0 : (pk >= n_boot ? n_boot - 1 : pk);
      const f32x4 g = *reinterpret_cast<const f32x4*>(bg + pk * row + in_row);
      const f32x4 mk = *reinterpret_cast<const f32x4*>(masks + k * plane + q);
      f32x4 b;
      b.x = mk.x >= 0.5f ? 1.f : 0.f;
      b.y = mk.y >= 0.5f ? 1.f : 0.f;
      b.z = mk.z >= 0.5f ? 1.f : 0.f;
      b.w = mk.w >= 0.5f ? 1.f : 0.f;
      const f32x4 noisy = sa * g + sb * nz;                   // DDIMScheduler.add_noise(bg, noise[view], t)
      xk = acc * b + noisy * (1.f - b);
    }
    *reinterpret_cast<f32x4*>(x_in + ((long)j * Pp + k) * row + in_row) = xk;
    *reinterpret_cast<f32x4*>(x_in + ((long)(nvc + j) * Pp + k) * row + in_row) = xk;
  }
}

// accumulate: one thread = four consecutive fp32 lanes of the panorama (view starts are multiples of 8, so the four lanes
// lie inside or outside a view together).  It gathers from the chunk's views that cover it in ascending view order and
// owns its value / count / latent elements: no atomics, and the add order does not depend on how the views are chunked.
__global__ __launch_bounds__(64) void multidiffusion_views_accum_kernel(
    const float* __restrict__ eps, const float* __restrict__ x_in, float* __restrict__ latent, float* __restrict__ value,
    float* __restrict__ count, const float* __restrict__ masks, const float* __restrict__ coef_table,
    const int32_t* __restrict__ dyn, float* __restrict__ hist, int P, int Pp, int C, int Hp, int Wp, int nbw, int V,
    int v0, int nv, int nvc, int n_steps, int indep_uncond, int normalization) {
  const int step = dyn[0];
  if (step < 0 || step >= n_steps) return;
  const long plane = (long)Hp * Wp;
  const long n = C * plane;
  const long e = (blockIdx.x * 64L + threadIdx.x) << 2;
  if (e >= n) return;
  const int c = (int)(e / plane);
  const long q = e - c * plane;
  const int y = (int)(q / Wp), x = (int)(q - (long)y * Wp);
  const float* ct = coef_table + step * 4;
  const float a_t = ct[0], a_p = ct[1], gs = ct[2];
  const bool vpred = ct[3] != 0.f;
  const float sa = sqrtf(a_t), sb = sqrtf(1.f - a_t), pa = sqrtf(a_p), pb = sqrtf(1.f - a_p);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 val = zero, cnt = zero;
  if (v0 > 0) {
    val = *reinterpret_cast<const f32x4*>(value + e);
    if (normalization) cnt = *reinterpret_cast<const f32x4*>(count + e);
  }
  const long row = (long)C * MD_WHW;
  for (int j = 0; j < nv; ++j) {
    const int v = v0 + j;
    const int hs = (v / nbw) * MD_STRIDE, ws = (v % nbw) * MD_STRIDE;
    if (y < hs || y >= hs + MD_WIN || x < ws || x >= ws + MD_WIN) continue;
    const long in_row = (long)c * MD_WHW + (y - hs) * MD_WIN + (x - ws);
    const float* eu_row = eps + (long)j * Pp * row + in_row;
    const float* ec_row = eps + (long)(nvc + j) * Pp * row + in_row;
    const float* x_row = x_in + (long)j * Pp * row + in_row;
    const f32x4 eu0 = *reinterpret_cast<const f32x4*>(eu_row);
    f32x4 vs = zero, cs = zero;
    for (int k = 0; k < P; ++k) {
      const f32x4 eu = *reinterpret_cast<const f32x4*>(eu_row + k * row);
      const f32x4 ec = *reinterpret_cast<const f32x4*>(ec_row + k * row);
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x_row + k * row);
      const f32x4 mk = *reinterpret_cast<const f32x4*>(masks + k * plane + q);
      f32x4 d;
      if (indep_uncond) {
        d.x = md_ddim(eu.x, ec.x, xv.x, gs, vpred, sa, sb, pa, pb);
        d.y = md_ddim(eu.y, ec.y, xv.y, gs, vpred, sa, sb, pa, pb);
        d.z = md_ddim(eu.z, ec.z, xv.z, gs, vpred, sa, sb, pa, pb);
        d.w = md_ddim(eu.w, ec.w, xv.w, gs, vpred, sa, sb, pa, pb);
      } else {                                               // one unconditional row per view, the directions differ
        const f32x4 m = gs * (ec - eu) + eu0;
        d.x = md_ddim_of(m.x, xv.x, vpred, sa, sb, pa, pb);
        d.y = md_ddim_of(m.y, xv.y, vpred, sa, sb, pa, pb);
        d.z = md_ddim_of(m.z, xv.z, vpred, sa, sb, pa, pb);
        d.w = md_ddim_of(m.w, xv.w, vpred, sa, sb, pa, pb);
      }
      vs = k == 0 ? mk * d : vs + mk * d;                     // the sum over prompts first, then into the panorama
      cs = k == 0 ? mk : cs + mk;
    }
    val += vs;
    cnt += cs;
  }
  if (v0 + nv < V) {
    *reinterpret_cast<f32x4*>(value + e) = val;
    if (normalization) *reinterpret_cast<f32x4*>(count + e) = cnt;
    return;
  }
  if (normalization) {                                        // torch.where(count > 0, value / count, value)
    val.x = cnt.x > 0.f ? val.x / cnt.x : val.x;
    val.y = cnt.y > 0.f ? val.y / cnt.y : val.y;
    val.z = cnt.z > 0.f ? val.z / cnt.z : val.z;
    val.w = cnt.w > 0.f ? val.w / cnt.w : val.w;
  }
  *reinterpret_cast<f32x4*>(latent + e) = val;
  if (hist) *reinterpret_cast<f32x4*>(hist + (long)(step + 1) * n + e) = val;
}

// uint8 HWC images [npix][3] -> the 8-channel fp16 operand of the VAE encoder's conv_in (lgd_hip.h): channels 0..2 =
// fp16(x), 3..5 = fp16(x - fp16(x)), 6..7 zero, x = lut[u] (the host's 2 * (u / 255) - 1 in fp32, pipelines.py:101-104).
// One thread = 4 pixels: three 4-byte loads (12 bytes), four 16-byte stores.
__global__ __launch_bounds__(256) void image_u8_to_nhwc8_kernel(const uint32_t* __restrict__ img,
                                                                 const float* __restrict__ table, half_t* __restrict__ y,
                                                                 long nquad) {
  __shared__ float lut[256];
  lut[threadIdx.x] = table[threadIdx.x];
  __syncthreads();
  for (long i = blockIdx.x * 256L + threadIdx.x; i < nquad; i += gridDim.x * 256L) {
    const uint32_t w[3] = {img[3 * i], img[3 * i + 1], img[3 * i + 2]};
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      half8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int k = 3 * p + c;  // byte k of the 12 (little endian)
        const float v = lut[(w[k >> 2] >> (8 * (k & 3))) & 255u];
        const half_t hi = (half_t)v;
        o[c] = hi;
        o[c + 3] = (half_t)(v - (float)hi);
      }
      reinterpret_cast<half8_t*>(y)[4 * i + p] = o;
    }
  }
}

// DiagonalGaussianDistribution.sample of the VAE encoder's moments, scaled (lgd_hip.h).  moments fp16 [B*HW][2z]
// (channels-last: z means, then z log-variances), noise / out NCHW fp32 (B, z, HW).  One thread = 4 pixels x 4 channels:
// eight 8-byte loads of moments, four 16-byte loads of noise, four 16-byte stores.
__global__ __launch_bounds__(256) void vae_sample_kernel(const half_t* __restrict__ moments,
                                                          const float* __restrict__ noise, float* __restrict__ out,
                                                          int z, long HW, float scale, long total) {
  const long hw4 = HW / 4;
  const int z4 = z / 4;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
    const long pq = i % hw4;
    const int cg = (int)((i / hw4) % z4);
    const long b = i / (hw4 * z4);
    const long p0 = pq * 4;
    f32x4 mean[4], sd[4];  // [pixel][channel of the group]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const half_t* row = moments + ((b * HW + p0 + j) * 2 * z + cg * 4);
      const half4_t m = *reinterpret_cast<const half4_t*>(row);
      const half4_t lv = *reinterpret_cast<const half4_t*>(row + z);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        mean[j][c] = (float)m[c];
        sd[j][c] = expf(0.5f * fminf(fmaxf((float)lv[c], -30.f), 20.f));
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long o = (b * z + cg * 4 + c) * HW + p0;
      const f32x4 nz = *reinterpret_cast<const f32x4*>(noise + o);
      f32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = scale * (mean[j][c] + sd[j][c] * nz[j]);
      *reinterpret_cast<f32x4*>(out + o) = r;
    }
  }
}

__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                         const float* __restrict__ table,
                                                         const int32_t* __restrict__ dyn, int row_stride, int col,
                                                         long n, int reps) {
  const float s = table[(long)dyn[0] * row_stride + col];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const float v = x[i] * s;
    for (int r = 0; r < reps; ++r) out[r * n + i] = v;
  }
}

__global__ __launch_bounds__(256) void axpy_kernel(const float* __restrict__ g, float* __restrict__ x,
                                                    const float* __restrict__ coef_table,
                                                    const int32_t* __restrict__ step_idx, int col,
                                                    const float* __restrict__ active, long per_sample,
                                                    long n) {
  const float s = coef_table[(*step_idx) * 4 + col];
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const float a = active ? active[i / per_sample] : 1.f;   // per-image on/off (batched guidance)
    x[i] -= a * s * g[i];
  }
}

__global__ __launch_bounds__(256) void select_row_kernel(const float* __restrict__ table,
                                                          const int32_t* __restrict__ idx,
                                                          float* __restrict__ out, int n) {
  const long r = *idx;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) out[i] = table[r * n + i];
}

// Range probe of an fp16 matrix (lgd_hip.h: lgd_range_f16): the largest finite magnitude and the count of non-finite
// elements, accumulated into out2.  The bit pattern of |x| orders fp16 magnitudes, and >= 0x7c00 is Inf or NaN, so the
// whole reduction is integer max / add: exact and the same for every grid.  VEC: a unit is a 16-byte vector of 8
// elements, else one element; `per_row` units of each row are read, rows are `ld` elements apart.
constexpr int RANGE_WGS = 4 * 256;  // 4 workgroups (16 waves) on each of the 256 CUs, two loads in flight per lane

__device__ __forceinline__ void range_take(uint32_t h, uint32_t& mx, uint32_t& bad) {
  h &= 0x7fffu;
  const bool nf = h >= 0x7c00u;
  mx = max(mx, nf ? 0u : h);
  bad += nf ? 1u : 0u;
}

template <bool VEC>
__device__ __forceinline__ void range_unit(const uint16_t* __restrict__ x, long i, long per_row, long ld, bool narrow,
                                           uint32_t& mx, uint32_t& bad) {
  // (the host hands a contiguous matrix over as one row, so only a padded one pays for the division)
  const long r = per_row == 0 ? 0 : (narrow ? (long)((uint32_t)i / (uint32_t)per_row) : i / per_row);
  const long c = i - r * per_row;
  if (VEC) {
    const uint4 v = *reinterpret_cast<const uint4*>(x + r * ld + c * 8);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      range_take(w[e], mx, bad);
      range_take(w[e] >> 16, mx, bad);
    }
  } else {
    range_take(x[r * ld + c], mx, bad);
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void range_f16_kernel(const uint16_t* __restrict__ x, long rows, long per_row, long ld,
                                                         uint32_t* out2) {
  __shared__ uint32_t red[8];
  const long total = rows * per_row, stride = gridDim.x * 256L;
  const bool narrow = total <= 0x7fffffffL;
  const long div = rows == 1 ? 0 : per_row;  // one row: unit i is column i
  uint32_t mx = 0, bad = 0;
  long i = blockIdx.x * 256L + threadIdx.x;
  for (; i + stride < total; i += 2 * stride) {
    uint32_t m1 = 0, b1 = 0;
    range_unit<VEC>(x, i, div, ld, narrow, mx, bad);
    range_unit<VEC>(x, i + stride, div, ld, narrow, m1, b1);
    mx = max(mx, m1);
    bad += b1;
  }
  if (i < total) range_unit<VEC>(x, i, div, ld, narrow, mx, bad);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    bad += (uint32_t)__shfl_xor((int)bad, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = mx;
    red[4 + (threadIdx.x >> 6)] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mx = max(max(red[0], red[1]), max(red[2], red[3]));
    bad = red[4] + red[5] + red[6] + red[7];  // at most 2^40 elements over RANGE_WGS workgroups: 2^30 in one
    if (mx) atomicMax(out2, __float_as_uint((float)__builtin_bit_cast(_Float16, (uint16_t)mx)));
    if (bad) {
      // saturating: the counter leaves 0xffffffff only through an add, which wraps, and whoever wraps it pins it again
      const uint32_t was = atomicAdd(out2 + 1, bad);
      if (was + bad < was) atomicMax(out2 + 1, 0xffffffffu);
    }
  }
}

using lgd_contract::misaligned;
using lgd_contract::overlaps;
using lgd_contract::partly_overlaps;

// y = f(x) over n fp16 elements in 16-byte vectors; y is x itself or a range apart (lgd_hip.h)
inline bool bad_unary_f16(const void* x, const void* y, int64_t n) {
  return !x || !y || n < 1 || (n % 8) || misaligned(x, 16) || misaligned(y, 16) || partly_overlaps(y, x, n * 2);
}

// what the two fused sampler steps share (lgd_hip.h): fp32 scalars, x_out is x itself or apart, the blend takes both of
// frozen_ref and mask; x_out overlaps none of the inputs whose extent the arguments give
inline bool bad_step_f32(const float* eps, const float* x, const float* x_out, const float* coef_table, const int32_t* dyn,
                         const float* frozen_ref, const float* mask, const float* hist, int B, int C, int HW) {
  if (!eps || !x || !x_out || !coef_table || !dyn || B < 1 || C < 1 || HW < 1) return true;
  if ((frozen_ref != nullptr) != (mask != nullptr)) return true;
  if (misaligned(eps, 4) || misaligned(x, 4) || misaligned(x_out, 4) || misaligned(coef_table, 4) || misaligned(dyn, 4) ||
      misaligned(frozen_ref, 4) || misaligned(mask, 4) || misaligned(hist, 4))
    return true;
  const int64_t nb = (int64_t)B * C * HW * 4;
  return partly_overlaps(x_out, x, nb) || overlaps(x_out, nb, eps, 2 * nb) || overlaps(x_out, nb, mask, (int64_t)B * HW * 4);
}

inline int ew_blocks(long n) {
  long b = (n + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int lgd_conv_in_f16(const float* x_nchw, const void* w, const float* bias, void* y, int B,
                               int Cin, int L, int Cout, void* stream) {
  if (!x_nchw || !w || !y || B < 1 || L < 1 || Cin < 1 || Cin > 8 || Cout < 1) return LGD_ERR_ARG;
  if (misaligned(x_nchw, 4) || misaligned(w, 2) || misaligned(bias, 4) || misaligned(y, 2)) return LGD_ERR_ARG;
  const int K = 9 * Cin;
  {
    const int64_t yb = (int64_t)B * L * L * Cout * 2;
    if (overlaps(y, yb, x_nchw, (int64_t)B * Cin * L * L * 4) || overlaps(y, yb, w, (int64_t)Cout * K * 2) ||
        overlaps(y, yb, bias, (int64_t)Cout * 4))
      return LGD_ERR_ARG;
  }
  size_t smem = (size_t)((K * Cout * 2 + 15) & ~15) + (size_t)CI_PIX * K * 4;
  if (smem > 64 * 1024) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  long npix = (long)B * L * L;
  hipLaunchKernelGGL(conv_in_kernel, dim3((unsigned)((npix + CI_PIX - 1) / CI_PIX)), dim3(256), smem,
                     reinterpret_cast<hipStream_t>(stream), x_nchw, (const half_t*)w, bias,
                     (half_t*)y, B, Cin, L, Cout);
  return lgd_check_launch();
}

extern "C" int lgd_conv_out_f16(const void* x, const void* w, const float* bias, float* y_nchw, int B,
                                int Cin, int L, int Cout, float out_scale, void* stream) {
  if (!x || !w || !y_nchw || B < 1 || L < 1 || (Cin % 8) || Cin < 8) return LGD_ERR_ARG;
  if (misaligned(x, 16) || misaligned(w, 16) || misaligned(bias, 4) || misaligned(y_nchw, 4)) return LGD_ERR_ARG;
  long npix = (long)B * L * L;
  if (Cout == 4 || Cout == 8) {  // the extent of y_nchw is known
    const int64_t yb = (int64_t)npix * Cout * 4;
    if (overlaps(y_nchw, yb, x, (int64_t)npix * Cin * 2) || overlaps(y_nchw, yb, w, (int64_t)Cout * 9 * Cin * 2) ||
        overlaps(y_nchw, yb, bias, (int64_t)Cout * 4))
      return LGD_ERR_ARG;
  }
  if (Cout != 4 && Cout != 8) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  dim3 grid((unsigned)((npix + 3) / 4));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (Cout == 4)
    hipLaunchKernelGGL((conv_out_kernel<4>), grid, dim3(256), 0, st, (const half_t*)x,
                       (const half_t*)w, bias, y_nchw, B, Cin, L, out_scale);
  else
    hipLaunchKernelGGL((conv_out_kernel<8>), grid, dim3(256), 0, st, (const half_t*)x,
                       (const half_t*)w, bias, y_nchw, B, Cin, L, out_scale);
  return lgd_check_launch();
}

extern "C" int lgd_add_f16(const void* a, const void* b, void* y, int64_t n, void* stream) {
  if (!a || !b || !y || n < 1 || (n % 8) || misaligned(a, 16) || misaligned(b, 16) || misaligned(y, 16)) return LGD_ERR_ARG;
  if (partly_overlaps(y, a, n * 2) || partly_overlaps(y, b, n * 2)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(add_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)a, (const half_t*)b,
                     (half_t*)y, (long)(n / 8));
  return lgd_check_launch();
}

extern "C" int lgd_scale_f16(const void* x, void* y, float alpha, int64_t n, void* stream) {
  if (bad_unary_f16(x, y, n)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(scale_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)x, (half_t*)y, alpha,
                     (long)(n / 8));
  return lgd_check_launch();
}

extern "C" int lgd_nchw_to_nhwc8_f16(const float* x, void* y, int B, int C, int HW, void* stream) {
  if (!x || !y || B < 1 || C < 1 || C > 8 || HW < 1 || misaligned(x, 4) || misaligned(y, 16)) return LGD_ERR_ARG;
  const long total = (long)B * HW;
  if (overlaps(y, (int64_t)total * 16, x, (int64_t)total * C * 4)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(nchw_to_nhwc8_kernel, dim3(ew_blocks(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     (half_t*)y, C, (long)HW, total);
  return lgd_check_launch();
}

extern "C" int lgd_image_u8_to_nhwc8_f16(const void* img, const float* table, void* y, int B, int HW, void* stream) {
  if (!img || !table || !y || B < 1 || HW < 1) return LGD_ERR_ARG;
  const long npix = (long)B * HW;
  if ((npix & 3) || misaligned(img, 4) || misaligned(table, 4) || misaligned(y, 16))
    return LGD_ERR_ARG;  // four pixels = three whole 4-byte words in, four 16-byte vectors out
  if (overlaps(y, (int64_t)npix * 16, img, (int64_t)npix * 3) || overlaps(y, (int64_t)npix * 16, table, 256 * 4)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(image_u8_to_nhwc8_kernel, dim3(ew_blocks(npix / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const uint32_t*)img, table, (half_t*)y, npix / 4);
  return lgd_check_launch();
}

extern "C" int lgd_vae_sample_f32(const void* moments, const float* noise, float* out, int B, int z, int HW, float scale,
                                  void* stream) {
  if (!moments || !noise || !out || B < 1 || z < 4 || HW < 4) return LGD_ERR_ARG;
  if ((z & 3) || (HW & 3) || misaligned(moments, 8) || misaligned(noise, 16) || misaligned(out, 16))
    return LGD_ERR_ARG;  // 8-byte vectors of 4 moments, 16-byte vectors of 4 pixels
  {
    const int64_t ob = (int64_t)B * z * HW * 4;
    if (overlaps(out, ob, moments, ob) || overlaps(out, ob, noise, ob)) return LGD_ERR_ARG;  // moments: 2z halfs per pixel
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  const long total = (long)B * (z / 4) * (HW / 4);
  hipLaunchKernelGGL(vae_sample_kernel, dim3(ew_blocks(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const half_t*)moments, noise, out, z, (long)HW, scale, total);
  return lgd_check_launch();
}

extern "C" int lgd_quick_gelu_f16(const void* x, void* y, int64_t n, void* stream) {
  if (bad_unary_f16(x, y, n)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)x, (half_t*)y, (long)(n / 8));
  return lgd_check_launch();
}

extern "C" int lgd_geglu_fwd_f16(const void* h, void* y, int64_t rows, int n, void* stream) {
  if (!h || !y || rows < 1 || n < 16 || (n % 16) || misaligned(h, 16) || misaligned(y, 16)) return LGD_ERR_ARG;
  if (overlaps(y, rows * n * 2, h, rows * n * 4)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(geglu_fwd_kernel, dim3(ew_blocks(rows * (n / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)h, (half_t*)y, (long)rows, n);
  return lgd_check_launch();
}

extern "C" int lgd_geglu_bwd_f16(const void* h, const void* gy, void* gh, int64_t rows, int n,
                                 void* stream) {
  if (!h || !gy || !gh || rows < 1 || n < 16 || (n % 16) || misaligned(h, 16) || misaligned(gy, 16) || misaligned(gh, 16))
    return LGD_ERR_ARG;
  if (overlaps(gh, rows * n * 4, h, rows * n * 4) || overlaps(gh, rows * n * 4, gy, rows * n * 2)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3(ew_blocks(rows * (n / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)h, (const half_t*)gy,
                     (half_t*)gh, (long)rows, n);
  return lgd_check_launch();
}

extern "C" int lgd_upsample2x_bwd_f16(const void* gy, void* gx, int B, int H, int W, int C,
                                      void* stream) {
  if (!gy || !gx || B < 1 || H < 1 || W < 1 || C < 8 || (C % 8) || misaligned(gy, 16) || misaligned(gx, 16)) return LGD_ERR_ARG;
  {
    const int64_t xb = (int64_t)B * H * W * C * 2;
    if (overlaps(gx, xb, gy, 4 * xb)) return LGD_ERR_ARG;
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(ew_blocks((long)B * H * W * (C / 8))), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)gy, (half_t*)gx, B, H, W,
                     C);
  return lgd_check_launch();
}

extern "C" int lgd_softmax_rows_f16(const void* x, void* y, int64_t rows, int n, float scale,
                                    void* stream) {
  if (rows < 1 || n < 8 || (n % 8) || bad_unary_f16(x, y, rows * n)) return LGD_ERR_ARG;  // every row starts on a vector
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), (const half_t*)x, (half_t*)y, (long)rows, n,
                     scale);
  return lgd_check_launch();
}

extern "C" int lgd_cfg_ddim_step_f32(const float* eps, const float* x, float* x_out,
                                     const float* coef_table, const int32_t* dyn,
                                     const float* frozen_ref, const float* mask, float* hist, int B,
                                     int C, int HW, void* stream) {
  if (bad_step_f32(eps, x, x_out, coef_table, dyn, frozen_ref, mask, hist, B, C, HW)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(cfg_ddim_kernel, dim3(ew_blocks((long)B * C * HW)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), eps, x, x_out, coef_table, dyn, frozen_ref,
                     mask, hist, B, C * HW, HW);
  return lgd_check_launch();
}

extern "C" int lgd_cfg_multistep_step_f32(const float* eps, const float* x, float* x_out, float* x0_prev,
                                          const float* coef_table, const int32_t* dyn, const float* frozen_ref,
                                          const float* mask, float* hist, int B, int C, int HW, void* stream) {
  if (!x0_prev || misaligned(x0_prev, 4) || bad_step_f32(eps, x, x_out, coef_table, dyn, frozen_ref, mask, hist, B, C, HW))
    return LGD_ERR_ARG;
  {
    const int64_t nb = (int64_t)B * C * HW * 4;  // the state is read and rewritten: apart from every other operand
    if (overlaps(x0_prev, nb, x, nb) || overlaps(x0_prev, nb, x_out, nb) || overlaps(x0_prev, nb, eps, 2 * nb) ||
        overlaps(x0_prev, nb, mask, (int64_t)B * HW * 4))
      return LGD_ERR_ARG;
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(cfg_multistep_kernel, dim3(ew_blocks((long)B * C * HW)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), eps, x, x_out, x0_prev, coef_table, dyn, frozen_ref,
                     mask, hist, B, C * HW, HW);
  return lgd_check_launch();
}

extern "C" int lgd_cfg_plms_step_f32(const float* eps, const float* x, float* x_out, float* ets, float* cur_sample,
                                     const float* coef_table, const int32_t* dyn, float* hist, int B, int C, int HW,
                                     void* stream) {
  if (!eps || !x || !x_out || !ets || !cur_sample || !coef_table || !dyn || B < 1 || C < 1 || HW < 1)
    return LGD_ERR_ARG;
  const long n = (long)B * C * HW;
  if ((n & 3) || misaligned(eps, 16) || misaligned(x, 16) || misaligned(x_out, 16) || misaligned(ets, 16) ||
      misaligned(cur_sample, 16) || misaligned(hist, 16) || misaligned(coef_table, 4) || misaligned(dyn, 4))
    return LGD_ERR_ARG;  // 16-byte vectors: every plane starts on a vector boundary
  {
    const int64_t nb = (int64_t)n * 4;  // x_out is x itself or apart; the ring and the saved sample are read and rewritten
    if (partly_overlaps(x_out, x, nb) || overlaps(x_out, nb, eps, 2 * nb) || overlaps(x_out, nb, ets, 3 * nb) ||
        overlaps(x_out, nb, cur_sample, nb))
      return LGD_ERR_ARG;
    if (overlaps(ets, 3 * nb, eps, 2 * nb) || overlaps(ets, 3 * nb, x, nb) || overlaps(ets, 3 * nb, cur_sample, nb))
      return LGD_ERR_ARG;
    if (overlaps(cur_sample, nb, eps, 2 * nb) || overlaps(cur_sample, nb, x, nb)) return LGD_ERR_ARG;
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(cfg_plms_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), eps,
                     x, x_out, ets, cur_sample, coef_table, dyn, hist, n);
  return lgd_check_launch();
}

extern "C" int lgd_cfg_lms_step_f32(const float* eps, const float* x, float* x_out, float* ring, const float* coef_table,
                                    const int32_t* dyn, const float* frozen_ref, const float* mask, float* hist, int B,
                                    int C, int HW, void* stream) {
  if (!ring || bad_step_f32(eps, x, x_out, coef_table, dyn, frozen_ref, mask, hist, B, C, HW)) return LGD_ERR_ARG;
  const long n = (long)B * C * HW;
  if ((n & 3) || misaligned(eps, 16) || misaligned(x, 16) || misaligned(x_out, 16) || misaligned(ring, 16) ||
      misaligned(hist, 16))
    return LGD_ERR_ARG;  // 16-byte vectors: every latent starts on a vector boundary
  {
    const int64_t nb = (int64_t)n * 4;  // the ring is read and rewritten: apart from every other operand
    if (overlaps(ring, 4 * nb, eps, 2 * nb) || overlaps(ring, 4 * nb, x, nb) || overlaps(ring, 4 * nb, x_out, nb) ||
        overlaps(ring, 4 * nb, mask, (int64_t)B * HW * 4) || overlaps(ring, 4 * nb, coef_table, 16 * 4) ||
        overlaps(ring, 4 * nb, dyn, 2 * 4))
      return LGD_ERR_ARG;
    // frozen_ref and hist hold step + 2 latents, and the step is read on the device: the two every step addresses
    if (overlaps(ring, 4 * nb, frozen_ref, 2 * nb) || overlaps(ring, 4 * nb, hist, 2 * nb)) return LGD_ERR_ARG;
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(cfg_lms_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), eps, x,
                     x_out, ring, coef_table, dyn, frozen_ref, mask, hist, n, C * HW, HW);
  return lgd_check_launch();
}

extern "C" int lgd_multidiffusion_step_f32(const float* eps, float* x_in, float* latent, const float* masks,
                                           const float* bg, const float* noise, const int32_t* picks,
                                           const float* coef_table, const int32_t* dyn, float* hist, int P, int Pp,
                                           int C, int HW, int n_steps, int n_boot, int prep, void* stream) {
  if (!x_in || !latent || !masks || !coef_table || !dyn || P < 1 || Pp < P || C < 1 || HW < 1 || n_steps < 1 ||
      n_boot < 0 || (prep != 0 && prep != 1) || (!prep && !eps))
    return LGD_ERR_ARG;
  const bool boots = n_boot > 0 && P > 1;
  if (boots && (!bg || !noise || !picks)) return LGD_ERR_ARG;
  const long n = (long)C * HW;
  if ((HW & 3) || misaligned(eps, 16) || misaligned(x_in, 16) || misaligned(latent, 16) || misaligned(masks, 16) ||
      misaligned(bg, 16) || misaligned(noise, 16) || misaligned(hist, 16) || misaligned(picks, 4) ||
      misaligned(coef_table, 4) || misaligned(dyn, 4))
    return LGD_ERR_ARG;  // 16-byte vectors: every plane and mask row starts on a vector boundary
  {
    const int64_t nb = (int64_t)n * 4, rows = 2 * (int64_t)Pp * nb, mb = (int64_t)P * HW * 4;
    if (overlaps(x_in, rows, latent, nb) || overlaps(x_in, rows, eps, rows) || overlaps(latent, nb, eps, rows) ||
        overlaps(x_in, rows, masks, mb) || overlaps(latent, nb, masks, mb))
      return LGD_ERR_ARG;
    if (boots && (overlaps(x_in, rows, bg, n_boot * nb) || overlaps(latent, nb, bg, n_boot * nb) ||
                  overlaps(x_in, rows, noise, nb) || overlaps(latent, nb, noise, nb)))
      return LGD_ERR_ARG;
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  const long nv = n / 4;
  hipLaunchKernelGGL(multidiffusion_step_kernel, dim3((unsigned)((nv + 63) / 64)), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), eps, x_in, latent, masks, bg, noise, picks, coef_table,
                     dyn, hist, P, Pp, HW, n, n_steps, n_boot, prep);
  return lgd_check_launch();
}

extern "C" int lgd_multidiffusion_views_f32(const float* eps, float* x_in, float* latent, float* value, float* count,
                                            const float* masks, const float* bg, const float* noise,
                                            const int32_t* picks, const float* coef_table, const int32_t* dyn,
                                            float* hist, int P, int Pp, int C, int Hp, int Wp, int V, int v0, int nv,
                                            int nvc, int n_steps, int n_boot, int indep_uncond, int normalization,
                                            int prep, void* stream) {
  if (!x_in || !latent || !masks || !coef_table || !dyn || P < 1 || Pp < P || C < 1 || n_steps < 1 || n_boot < 0 ||
      (prep != 0 && prep != 1) || (!prep && !eps))
    return LGD_ERR_ARG;
  if (Hp < MD_WIN || Wp < MD_WIN || (Wp & 3) || Hp > 4096 || Wp > 4096 || C > 64) return LGD_ERR_ARG;
  const int nbh = (Hp - MD_WIN) / MD_STRIDE + 1, nbw = (Wp - MD_WIN) / MD_STRIDE + 1;   // get_views
  if (V != nbh * nbw || v0 < 0 || nv < 1 || v0 + nv > V || nvc < nv || (long)nvc * Pp > (1 << 20)) return LGD_ERR_ARG;
  const bool single = v0 == 0 && nv == V;
  if (!prep && !single && (!value || (normalization && !count))) return LGD_ERR_ARG;
  const bool boots = prep && n_boot > 0 && P > 1;
  if (boots && (!bg || !noise || !picks)) return LGD_ERR_ARG;
  if (misaligned(eps, 16) || misaligned(x_in, 16) || misaligned(latent, 16) || misaligned(value, 16) ||
      misaligned(count, 16) || misaligned(masks, 16) || misaligned(bg, 16) || misaligned(noise, 16) ||
      misaligned(hist, 16) || misaligned(picks, 4) || misaligned(coef_table, 4) || misaligned(dyn, 4))
    return LGD_ERR_ARG;  // 16-byte vectors: every plane, window row and mask row starts on a vector boundary
  {
    const int64_t wb = (int64_t)C * MD_WHW * 4, rows = 2 * (int64_t)nvc * Pp * wb, pb = (int64_t)C * Hp * Wp * 4,
                  mb = (int64_t)P * Hp * Wp * 4;
    if (prep) {
      if (overlaps(x_in, rows, latent, pb) || overlaps(x_in, rows, masks, mb)) return LGD_ERR_ARG;
      if (boots && (overlaps(x_in, rows, bg, n_boot * wb) || overlaps(x_in, rows, noise, pb))) return LGD_ERR_ARG;
    } else {
      const float* outs[3] = {latent, value, count};
      for (int i = 0; i < 3; ++i) {
        if (overlaps(outs[i], pb, eps, rows) || overlaps(outs[i], pb, x_in, rows) || overlaps(outs[i], pb, masks, mb))
          return LGD_ERR_ARG;
        for (int j = i + 1; j < 3; ++j)
          if (overlaps(outs[i], pb, outs[j], pb)) return LGD_ERR_ARG;
      }
    }
  }
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (prep) {
    const long nt = (long)nv * C * (MD_WHW / 4);
    hipLaunchKernelGGL(multidiffusion_views_prep_kernel, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, x_in, latent,
                       masks, bg, noise, picks, coef_table, dyn, P, Pp, C, Hp, Wp, nbw, V, v0, nv, nvc, n_steps, n_boot);
  } else {
    const long nt = (long)C * Hp * Wp / 4;
    hipLaunchKernelGGL(multidiffusion_views_accum_kernel, dim3((unsigned)((nt + 63) / 64)), dim3(64), 0, s, eps, x_in,
                       latent, value, count, masks, coef_table, dyn, hist, P, Pp, C, Hp, Wp, nbw, V, v0, nv, nvc,
                       n_steps, indep_uncond ? 1 : 0, normalization ? 1 : 0);
  }
  return lgd_check_launch();
}

extern "C" int lgd_scale_rows_f32(const float* x, float* out, const float* table, const int32_t* dyn, int row_stride,
                                  int col, int64_t n, int reps, void* stream) {
  if (!x || !out || !table || !dyn || n < 1 || reps < 1 || col < 0 || col >= row_stride) return LGD_ERR_ARG;
  if (misaligned(x, 4) || misaligned(out, 4) || misaligned(table, 4) || misaligned(dyn, 4) || overlaps(out, reps * n * 4, x, n * 4))
    return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(scale_rows_kernel, dim3(ew_blocks(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, out,
                     table, dyn, row_stride, col, (long)n, reps);
  return lgd_check_launch();
}

extern "C" int lgd_axpy_f32(const float* g, float* x, const float* coef_table,
                            const int32_t* step_idx, int col, const float* active, int64_t per_sample,
                            int64_t n, void* stream) {
  if (!g || !x || !coef_table || !step_idx || n < 1 || col < 0 || col > 3 || per_sample < 0) return LGD_ERR_ARG;
  if (misaligned(g, 4) || misaligned(x, 4) || misaligned(coef_table, 4) || misaligned(step_idx, 4) || misaligned(active, 4))
    return LGD_ERR_ARG;
  if (active && per_sample > 0 && (n % per_sample)) return LGD_ERR_ARG;  // whole images: n / per_sample entries of active
  if (overlaps(x, n * 4, g, n * 4)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(axpy_kernel, dim3(ew_blocks(n)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), g, x, coef_table, step_idx, col, active,
                     (long)(per_sample > 0 ? per_sample : n), (long)n);
  return lgd_check_launch();
}

extern "C" int lgd_select_row_f32(const float* table, const int32_t* idx, float* out, int n,
                                  void* stream) {
  if (!table || !idx || !out || n < 1 || misaligned(table, 4) || misaligned(idx, 4) || misaligned(out, 4)) return LGD_ERR_ARG;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL(select_row_kernel, dim3(ew_blocks(n)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), table, idx, out, n);
  return lgd_check_launch();
}

extern "C" int lgd_range_f16(const void* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* out2, void* stream) {
  if (!x || !out2 || rows < 1 || cols < 1 || ld < cols || misaligned(x, 2) || misaligned(out2, 4)) return LGD_ERR_ARG;
  constexpr int64_t MAX_ELEMS = (int64_t)1 << 40;
  if (rows > MAX_ELEMS / cols) return LGD_ERR_UNSUPPORTED;
  if (rows > 1 && ld > ((int64_t)1 << 60) / rows) return LGD_ERR_ARG;  // no such address range
  if (overlaps(out2, 8, x, ((rows - 1) * ld + cols) * 2)) return LGD_ERR_ARG;
  const bool vec = (cols % 8) == 0 && (ld % 8) == 0 && !misaligned(x, 16);
  if (ld == cols || rows == 1) {  // contiguous: one long row
    cols *= rows;
    rows = 1;
    ld = cols;
  }
  const long per_row = vec ? cols / 8 : cols;
  const long wgs = (rows * per_row + 255) / 256;
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  const dim3 grid((unsigned)(wgs < RANGE_WGS ? wgs : RANGE_WGS));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL((range_f16_kernel<true>), grid, dim3(256), 0, st, (const uint16_t*)x, (long)rows, per_row, (long)ld, out2);
  else
    hipLaunchKernelGGL((range_f16_kernel<false>), grid, dim3(256), 0, st, (const uint16_t*)x, (long)rows, per_row, (long)ld, out2);
  return lgd_check_launch();
}
