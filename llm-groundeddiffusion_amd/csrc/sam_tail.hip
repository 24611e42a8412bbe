// What surrounds the SAM network in the mask refinement of LMD / LMD+ (reference models/sam.py), for a whole batch of
// (image, prompt) items and without a host read:
//
//  * sam_tail_resample_kernel + sam_tail_select_kernel — models/sam.py:45-55 (`post_process_masks`, the bilinear resize
//    to the latent grid, `.bool()`), :63-65 (`get_iou_with_resize`), :67-111 (`select_mask`) and the per-box part of
//    :182-213.  The three resamplings (S x S logits -> target x target -> crop -> h x w, > 0 -> H x W, != 0) are chained
//    per OUTPUT pixel: a latent-grid pixel reads 4 pixels of the thresholded h x w image, each of those 4 of the
//    target x target image, each of those 4 logits — 64 reads that the caches serve, no intermediate image is stored.
//    Every step is torch's `upsample_bilinear2d` (align_corners=False) term for term; this file is compiled with
//    floating-point contraction off so that products and sums round where torch's do.  One wave per (row block,
//    candidate, item) writes the candidate bytes and its three counts; one workgroup per item then sums the counts in a
//    fixed order, applies the selection rule and copies the winning candidate.  No atomics; every store has one owner.
//  * sam_attn_prompt_kernel — models/sam.py:113-122 (`preprocess_mask`, no erosion) and :125-147 (the point-prompt
//    branch of `sam_refine_attn`): scipy.ndimage.gaussian_filter (separable, axis 0 then axis 1, mode `reflect`),
//    min-max normalisation, threshold, first arg-max.  One workgroup per item, the map in LDS, fp32.
//  * sam_attn_box_prompt_kernel — the box-prompt branch of the same lines (use_box_input=True): the same smoothing and
//    threshold (one device function serves both kernels), then `preprocess_mask`'s opening (scipy.ndimage.binary_erosion /
//    binary_dilation, 4-neighbourhood, border 0) on two byte masks in LDS and utils.binary_mask_to_box as a min / max
//    reduction.  One workgroup per item.
#include "common.h"

#include <float.h>

namespace {

constexpr int TAIL_MAX_K = 4, TAIL_MAX_SIDE = 4096, TAIL_MAX_SRC = 32768, TAIL_MAX_N = 65535;
constexpr int SEL_THREADS = 256;
constexpr int PROMPT_THREADS = 256, PROMPT_MAX_PIX = 4096, PROMPT_MAX_RADIUS = 64, PROMPT_MAX_OPEN = 64;

// One axis of torch's bilinear sampling (align_corners=False): at::native::area_pixel_compute_source_index and
// guard_index_and_lambda.  `scale` = (float)in / out.
struct Tap {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Tap tap_of(int dst, float scale, int in) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  if (!(src >= 0.f)) src = 0.f;
  int i0 = (int)src;
  i0 = max(min(i0, in - 1), 0);  // in range whatever the geometry row holds
  Tap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  t.l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}

__device__ __forceinline__ float blend(const Tap& ty, const Tap& tx, float a, float b, float c, float d) {
  return ty.l0 * (tx.l0 * a + tx.l1 * b) + ty.l1 * (tx.l0 * c + tx.l1 * d);
}

struct TailArgs {
  const float* logits;     // [N][K][S][S]
  const float* iou;        // [N][K]
  const int32_t* geom;     // [N][4] = {h, w, nh, nw}
  const uint8_t* coarse;   // [N][hc][wc]
  uint8_t* cand;           // [N][K][H][W] (the caller's, or the tail of the workspace)
  int32_t* counts;         // [N][K][RB][3] = {area, inter, union} of a row block
  uint8_t* mask;           // [N][H][W]
  float* conf;             // [N]
  int32_t* stats;          // [N][1 + 3K]
  int N, K, S, target, H, W, hc, wc, rows, RB;
  double below_conf, below_iou;
};

// the target x target image at (Y, X), from the logits of one candidate
__device__ __forceinline__ float m1_at(const float* lg, int S, float s1, int Y, int X) {
  const Tap ty = tap_of(Y, s1, S), tx = tap_of(X, s1, S);
  const float* r0 = lg + (long)ty.i0 * S;
  const float* r1 = lg + (long)ty.i1 * S;
  return blend(ty, tx, r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1]);
}

// the thresholded h x w image at (y, x): the crop [0, nh) x [0, nw) of the target x target image, resampled
__device__ __forceinline__ float b2_at(const float* lg, int S, float s1, float s2h, float s2w, int nh, int nw, int y, int x) {
  const Tap ty = tap_of(y, s2h, nh), tx = tap_of(x, s2w, nw);
  const float v = blend(ty, tx, m1_at(lg, S, s1, ty.i0, tx.i0), m1_at(lg, S, s1, ty.i0, tx.i1),
                        m1_at(lg, S, s1, ty.i1, tx.i0), m1_at(lg, S, s1, ty.i1, tx.i1));
  return v > 0.f ? 1.f : 0.f;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(LGD_WAVE) void sam_tail_resample_kernel(const TailArgs a) {
  const int rb = blockIdx.x, k = blockIdx.y, n = blockIdx.z, lane = threadIdx.x;
  const int32_t* g = a.geom + (long)n * 4;
  const int h = max(g[0], 1), w = max(g[1], 1);
  const int nh = max(min(g[2], a.target), 1), nw = max(min(g[3], a.target), 1);
  const float s1 = (float)a.S / (float)a.target;
  const float s2h = (float)nh / (float)h, s2w = (float)nw / (float)w;
  const float s3h = (float)h / (float)a.H, s3w = (float)w / (float)a.W;
  const float* lg = a.logits + ((long)n * a.K + k) * a.S * a.S;
  const bool same = a.hc == a.H && a.wc == a.W;
  const uint8_t* co = a.coarse + (long)n * a.hc * a.wc;
  uint8_t* out = a.cand + ((long)n * a.K + k) * a.H * a.W;

  const int row0 = rb * a.rows, row1 = min(row0 + a.rows, a.H);
  int area = 0, inter = 0, uni = 0;
  for (int p = row0 * a.W + lane; p < row1 * a.W; p += LGD_WAVE) {
    const int oy = p / a.W, ox = p - oy * a.W;
    const Tap ty = tap_of(oy, s3h, h), tx = tap_of(ox, s3w, w);
    const float v = blend(ty, tx, b2_at(lg, a.S, s1, s2h, s2w, nh, nw, ty.i0, tx.i0),
                          b2_at(lg, a.S, s1, s2h, s2w, nh, nw, ty.i0, tx.i1),
                          b2_at(lg, a.S, s1, s2h, s2w, nh, nw, ty.i1, tx.i0),
                          b2_at(lg, a.S, s1, s2h, s2w, nh, nw, ty.i1, tx.i1));
    const int bit = v != 0.f ? 1 : 0;  // `.bool()`
    out[p] = (uint8_t)bit;
    area += bit;
    if (same) {
      const int c = co[p] != 0 ? 1 : 0;
      inter += bit & c;
      uni += bit | c;
    }
  }
  area = wave_sum_i(area), inter = wave_sum_i(inter), uni = wave_sum_i(uni);
  if (lane == 0) {
    int32_t* dst = a.counts + (((long)n * a.K + k) * a.RB + rb) * 3;
    dst[0] = area, dst[1] = inter, dst[2] = uni;
  }
}

// block-wide integer sum for SEL_THREADS threads; `red`: SEL_THREADS / 64 ints of LDS
__device__ __forceinline__ int block_sum_i(int v, int* red) {
  v = wave_sum_i(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int i = 0; i < SEL_THREADS / LGD_WAVE; ++i) r += red[i];
  return r;
}

__global__ __launch_bounds__(SEL_THREADS) void sam_tail_select_kernel(const TailArgs a) {
  __shared__ int s_red[SEL_THREADS / LGD_WAVE];
  __shared__ int s_pick;
  const int n = blockIdx.x, tid = threadIdx.x;
  const bool same = a.hc == a.H && a.wc == a.W;
  const uint8_t* co = a.coarse + (long)n * a.hc * a.wc;
  __shared__ int s_area[TAIL_MAX_K], s_inter[TAIL_MAX_K], s_uni[TAIL_MAX_K];
#pragma unroll 1
  for (int k = 0; k < a.K; ++k) {
    const int32_t* cnt = a.counts + ((long)n * a.K + k) * a.RB * 3;
    int ar = 0, in = 0, un = 0;
#pragma unroll 1
    for (int b = tid; b < a.RB; b += SEL_THREADS) {
      ar += cnt[b * 3];
      if (same) in += cnt[b * 3 + 1], un += cnt[b * 3 + 2];
    }
    if (!same) {  // get_iou_with_resize: the 0 / 1 candidate resampled to the coarse map's size, > 0
      const uint8_t* cd = a.cand + ((long)n * a.K + k) * a.H * a.W;
      const float sh = (float)a.H / (float)a.hc, sw = (float)a.W / (float)a.wc;
#pragma unroll 1
      for (int p = tid; p < a.hc * a.wc; p += SEL_THREADS) {
        const int cy = p / a.wc, cx = p - cy * a.wc;
        const Tap ty = tap_of(cy, sh, a.H), tx = tap_of(cx, sw, a.W);
        const uint8_t* r0 = cd + (long)ty.i0 * a.W;
        const uint8_t* r1 = cd + (long)ty.i1 * a.W;
        const float v = blend(ty, tx, r0[tx.i0] ? 1.f : 0.f, r0[tx.i1] ? 1.f : 0.f, r1[tx.i0] ? 1.f : 0.f,
                              r1[tx.i1] ? 1.f : 0.f);
        const int bit = v > 0.f ? 1 : 0;
        const int c = co[p] != 0 ? 1 : 0;
        in += bit & c;
        un += bit | c;
      }
    }
    ar = block_sum_i(ar, s_red), in = block_sum_i(in, s_red), un = block_sum_i(un, s_red);
    if (tid == 0) s_area[k] = ar, s_inter[k] = in, s_uni[k] = un;
  }
  if (tid == 0) {
    // select_mask, rule "largest_over_conf": score = area - max(area) [conf < below_conf] - max(area) [iou < below_iou],
    // the first maximum wins (np.argmax); numpy compares the fp32 confidences in fp32 and the fp64 IoUs in fp64
    int penalty = 0;
    for (int k = 0; k < a.K; ++k) penalty = max(penalty, s_area[k]);
    const float th_conf = (float)a.below_conf;
    int best = 0;
    long best_score = 0;
    int32_t* st = a.stats + (long)n * (1 + 3 * a.K);
    for (int k = 0; k < a.K; ++k) {
      const double iou = (double)s_inter[k] / ((double)s_uni[k] + 1e-6);
      long score = s_area[k];
      if (a.iou[(long)n * a.K + k] < th_conf) score -= penalty;
      if (iou < a.below_iou) score -= penalty;
      if (k == 0 || score > best_score) best = k, best_score = score;
      st[1 + k] = s_area[k];
      st[1 + a.K + k] = s_inter[k];
      st[1 + 2 * a.K + k] = s_uni[k];
    }
    st[0] = best;
    a.conf[n] = a.iou[(long)n * a.K + best];
    s_pick = best;
  }
  __syncthreads();
  const uint8_t* win = a.cand + ((long)n * a.K + s_pick) * a.H * a.W;
  uint8_t* m = a.mask + (long)n * a.H * a.W;
#pragma unroll 1
  for (int p = tid; p < a.H * a.W; p += SEL_THREADS) m[p] = win[p];
}

struct PromptArgs {
  const float* attn;  // [N][hm][wm]
  uint8_t* coarse;    // [N][hm][wm]
  float* points;      // [N][2]
  float* smooth;      // [N][hm][wm] or NULL
  int hm, wm, radius, up_w, up_h;
  float sigma, mask_th;
};

// `reflect` of scipy.ndimage (d c b a | a b c d | d c b a), any distance: the index is periodic with period 2n
__device__ __forceinline__ int reflect_index(int i, int n) {
  int m = i % (2 * n);
  if (m < 0) m += 2 * n;
  return m < n ? m : 2 * n - 1 - m;
}

// What both prompt kernels share (models/sam.py:128 and the first two lines of :113-116): item n's map smoothed into s_a
// (and into `smooth` when given), and the block-wide minimum, maximum and first arg-max of the smoothed map.  s_a, s_b:
// PROMPT_MAX_PIX floats of LDS each.  Every thread leaves with the same three values; s_a[p] is final for the thread
// that owns p (p = tid, tid + PROMPT_THREADS, ..), for the others after the next barrier.
struct SmoothStat {
  float lo, hi;
  int at;
};

__device__ __forceinline__ SmoothStat prompt_smooth(const float* attn, float* smooth, int n, int hm, int wm, int r,
                                                    float sigma, float* s_a, float* s_b) {
  __shared__ float s_w[2 * PROMPT_MAX_RADIUS + 1];
  constexpr int NW = PROMPT_THREADS / LGD_WAVE;
  __shared__ float s_red[2 * NW];
  __shared__ int s_idx[NW];
  const int tid = threadIdx.x, P = hm * wm;
  const float* src = attn + (long)n * P;
  for (int p = tid; p < P; p += PROMPT_THREADS) s_a[p] = src[p];
  // scipy's _gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2) over [-r, r], divided by its sum (fp64 there; here fp64 too,
  // rounded once to fp32)
  if (tid == 0) {
    const double c = -0.5 / ((double)sigma * (double)sigma);
    double sum = 0.0;
    for (int j = -r; j <= r; ++j) sum += exp(c * (double)(j * j));
    for (int j = -r; j <= r; ++j) s_w[j + r] = (float)(exp(c * (double)(j * j)) / sum);
  }
  __syncthreads();
  for (int p = tid; p < P; p += PROMPT_THREADS) {  // axis 0
    const int y = p / wm, x = p - y * wm;
    float acc = 0.f;
    for (int j = -r; j <= r; ++j) acc += s_w[j + r] * s_a[reflect_index(y + j, hm) * wm + x];
    s_b[p] = acc;
  }
  __syncthreads();
  float lo = FLT_MAX, hi = -FLT_MAX;
  int at = P;
  for (int p = tid; p < P; p += PROMPT_THREADS) {  // axis 1
    const int y = p / wm, x = p - y * wm;
    float acc = 0.f;
    for (int j = -r; j <= r; ++j) acc += s_w[j + r] * s_b[y * wm + reflect_index(x + j, wm)];
    s_a[p] = acc;
    if (smooth) smooth[(long)n * P + p] = acc;
    lo = fminf(lo, acc);
    if (acc > hi) hi = acc, at = p;  // ascending p: the first of equal maxima
  }
  // minimum, and the maximum with the lowest index that holds it
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    const float h2 = __shfl_xor(hi, o, 64);
    const int a2 = __shfl_xor(at, o, 64);
    if (h2 > hi || (h2 == hi && a2 < at)) hi = h2, at = a2;
  }
  if ((tid & 63) == 0) s_red[tid >> 6] = lo, s_red[NW + (tid >> 6)] = hi, s_idx[tid >> 6] = at;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    lo = fminf(lo, s_red[i]);
    const float h2 = s_red[NW + i];
    const int a2 = s_idx[i];
    if (h2 > hi || (h2 == hi && a2 < at)) hi = h2, at = a2;
  }
  SmoothStat st;
  st.lo = lo, st.hi = hi, st.at = at;
  return st;
}

// preprocess_mask's `(a - min) / max(a - min) > mask_th`; span = max - min = max(a - min): the subtraction is monotonic.
// A constant map has span 0: 0 / 0 = NaN, and NaN > th is false, as in numpy.
__device__ __forceinline__ int prompt_bit(float v, float lo, float span, float mask_th) {
  return ((v - lo) / span > mask_th) ? 1 : 0;
}

__global__ __launch_bounds__(PROMPT_THREADS) void sam_attn_prompt_kernel(const PromptArgs a) {
  __shared__ float s_a[PROMPT_MAX_PIX], s_b[PROMPT_MAX_PIX];
  const int n = blockIdx.x, tid = threadIdx.x, P = a.hm * a.wm;
  const SmoothStat st = prompt_smooth(a.attn, a.smooth, n, a.hm, a.wm, a.radius, a.sigma, s_a, s_b);
  const float span = st.hi - st.lo;
  uint8_t* co = a.coarse + (long)n * P;
  for (int p = tid; p < P; p += PROMPT_THREADS) co[p] = (uint8_t)prompt_bit(s_a[p], st.lo, span, a.mask_th);
  if (tid == 0) {
    const int peak_y = st.at / a.wm, peak_x = st.at - peak_y * a.wm;
    a.points[(long)n * 2] = (float)(peak_x * a.up_h);  // the reference's swapped (w, h) naming (:135,:146)
    a.points[(long)n * 2 + 1] = (float)(peak_y * a.up_w);
  }
}

struct BoxPromptArgs {
  const float* attn;  // [N][hm][wm]
  uint8_t* coarse;    // [N][hm][wm]
  float* boxes;       // [N][4]
  int32_t* empty;     // [N]
  float* smooth;      // [N][hm][wm] or NULL
  int hm, wm, radius, n_open, up_w, up_h;
  float sigma, mask_th;
};

__global__ __launch_bounds__(PROMPT_THREADS) void sam_attn_box_prompt_kernel(const BoxPromptArgs a) {
  __shared__ float s_a[PROMPT_MAX_PIX], s_b[PROMPT_MAX_PIX];
  __shared__ uint8_t s_m0[PROMPT_MAX_PIX], s_m1[PROMPT_MAX_PIX];
  constexpr int NW = PROMPT_THREADS / LGD_WAVE;
  __shared__ int s_box[4 * NW];
  const int n = blockIdx.x, tid = threadIdx.x, hm = a.hm, wm = a.wm, P = hm * wm;
  const SmoothStat st = prompt_smooth(a.attn, a.smooth, n, hm, wm, a.radius, a.sigma, s_a, s_b);
  const float span = st.hi - st.lo;
  for (int p = tid; p < P; p += PROMPT_THREADS) s_m0[p] = (uint8_t)prompt_bit(s_a[p], st.lo, span, a.mask_th);
  __syncthreads();
  // the opening (preprocess_mask :118-120): n_open erosions, then n_open dilations, with the pixel and its 4 neighbours
  // (generate_binary_structure(2, 1)) and border_value = 0: whatever lies outside the map is 0 for both, so a set pixel
  // on the border erodes and the outside never dilates inward.  One step per pass, from one byte mask into the other.
  uint8_t* cur = s_m0;
  uint8_t* nxt = s_m1;
#pragma unroll 1
  for (int s = 0; s < 2 * a.n_open; ++s) {
    const bool erode = s < a.n_open;
    for (int p = tid; p < P; p += PROMPT_THREADS) {
      const int y = p / wm, x = p - y * wm;
      const int up = y > 0 ? cur[p - wm] : 0, down = y < hm - 1 ? cur[p + wm] : 0;
      const int left = x > 0 ? cur[p - 1] : 0, right = x < wm - 1 ? cur[p + 1] : 0;
      const int c = cur[p];
      nxt[p] = (uint8_t)(erode ? (c & up & down & left & right) : (c | up | down | left | right));
    }
    __syncthreads();
    uint8_t* t = cur;
    cur = nxt, nxt = t;
  }
  // the opened mask out, and its bounding box: min / max per thread, per wave, then over the waves through LDS
  uint8_t* co = a.coarse + (long)n * P;
  int y0 = hm, y1 = -1, x0 = wm, x1 = -1;
  for (int p = tid; p < P; p += PROMPT_THREADS) {
    const int bit = cur[p];
    co[p] = (uint8_t)bit;
    if (bit) {
      const int y = p / wm, x = p - y * wm;
      y0 = min(y0, y), y1 = max(y1, y), x0 = min(x0, x), x1 = max(x1, x);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    y0 = min(y0, __shfl_xor(y0, o, 64)), y1 = max(y1, __shfl_xor(y1, o, 64));
    x0 = min(x0, __shfl_xor(x0, o, 64)), x1 = max(x1, __shfl_xor(x1, o, 64));
  }
  if ((tid & 63) == 0) {
    int* d = s_box + 4 * (tid >> 6);
    d[0] = y0, d[1] = y1, d[2] = x0, d[3] = x1;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      y0 = min(y0, s_box[4 * i]), y1 = max(y1, s_box[4 * i + 1]);
      x0 = min(x0, s_box[4 * i + 2]), x1 = max(x1, s_box[4 * i + 3]);
    }
    // utils.binary_mask_to_box(enlarge_box_by_one=True, w_scale=up_w, h_scale=up_h): the reference's swapped (w, h)
    // naming (:135,:141) kept.  An empty mask (the reference raises there) is flagged and gets the zero box.
    const bool none = y1 < 0;
    const int ymin = max(y0 - 1, 0), ymax = min(y1 + 1, hm), xmin = max(x0 - 1, 0), xmax = min(x1 + 1, wm);
    float* b = a.boxes + (long)n * 4;
    b[0] = none ? 0.f : (float)(xmin * a.up_w);
    b[1] = none ? 0.f : (float)(ymin * a.up_h);
    b[2] = none ? 0.f : (float)(xmax * a.up_w);
    b[3] = none ? 0.f : (float)(ymax * a.up_h);
    a.empty[n] = none ? 1 : 0;
  }
}

inline bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) & (n - 1); }

inline int tail_rows(int W) { return W >= LGD_WAVE ? 1 : LGD_WAVE / W; }

}  // namespace

extern "C" int lgd_sam_mask_tail_f32(const float* logits, const float* iou, const int32_t* geom, const uint8_t* coarse,
                                     int N, int K, int S, int target, int H, int W, int hc, int wc,
                                     double below_conf, double below_iou, uint8_t* cand, uint8_t* mask, float* conf,
                                     int32_t* stats, void* workspace, void* stream) {
  if (!logits || !iou || !geom || !coarse || !mask || !conf || !stats || !workspace) return LGD_ERR_ARG;
  if (N <= 0 || K <= 0 || K > TAIL_MAX_K || S <= 0 || target <= 0 || H <= 0 || W <= 0 || hc <= 0 || wc <= 0)
    return LGD_ERR_ARG;
  if (misaligned(logits, 4) || misaligned(iou, 4) || misaligned(geom, 4) || misaligned(conf, 4) || misaligned(stats, 4) ||
      misaligned(workspace, 4))
    return LGD_ERR_ARG;
  if (N > TAIL_MAX_N || H > TAIL_MAX_SIDE || W > TAIL_MAX_SIDE || hc > TAIL_MAX_SIDE || wc > TAIL_MAX_SIDE ||
      S > TAIL_MAX_SRC || target > TAIL_MAX_SRC)
    return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  TailArgs a;
  a.logits = logits, a.iou = iou, a.geom = geom, a.coarse = coarse;
  a.N = N, a.K = K, a.S = S, a.target = target, a.H = H, a.W = W, a.hc = hc, a.wc = wc;
  a.rows = tail_rows(W);
  a.RB = (H + a.rows - 1) / a.rows;
  a.counts = static_cast<int32_t*>(workspace);
  a.cand = cand ? cand : reinterpret_cast<uint8_t*>(a.counts + (long)N * K * a.RB * 3);
  a.mask = mask, a.conf = conf, a.stats = stats;
  a.below_conf = below_conf, a.below_iou = below_iou;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sam_tail_resample_kernel, dim3((unsigned)a.RB, (unsigned)K, (unsigned)N), dim3(LGD_WAVE), 0, st, a);
  hipLaunchKernelGGL(sam_tail_select_kernel, dim3((unsigned)N), dim3(SEL_THREADS), 0, st, a);
  return lgd_check_launch();
}

extern "C" int lgd_sam_attn_prompt_f32(const float* attn, int N, int hm, int wm, float sigma, float mask_th, int up_w,
                                       int up_h, uint8_t* coarse, float* points, float* smooth, void* stream) {
  if (!attn || !coarse || !points) return LGD_ERR_ARG;
  if (N <= 0 || hm <= 0 || wm <= 0 || !(sigma > 0.f) || up_w <= 0 || up_h <= 0) return LGD_ERR_ARG;
  if (misaligned(attn, 4) || misaligned(points, 4) || misaligned(smooth, 4)) return LGD_ERR_ARG;
  const int radius = (int)(4.0 * (double)sigma + 0.5);  // scipy: truncate = 4.0
  if (N > TAIL_MAX_N || (long)hm * wm > PROMPT_MAX_PIX || radius > PROMPT_MAX_RADIUS) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  PromptArgs a;
  a.attn = attn, a.coarse = coarse, a.points = points, a.smooth = smooth;
  a.hm = hm, a.wm = wm, a.radius = radius, a.up_w = up_w, a.up_h = up_h;
  a.sigma = sigma, a.mask_th = mask_th;
  hipLaunchKernelGGL(sam_attn_prompt_kernel, dim3((unsigned)N), dim3(PROMPT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return lgd_check_launch();
}

extern "C" int lgd_sam_attn_box_prompt_f32(const float* attn, int N, int hm, int wm, float sigma, float mask_th,
                                           int n_open, int up_w, int up_h, uint8_t* coarse, float* boxes,
                                           int32_t* empty, float* smooth, void* stream) {
  if (!attn || !coarse || !boxes || !empty) return LGD_ERR_ARG;
  if (N <= 0 || hm <= 0 || wm <= 0 || !(sigma > 0.f) || up_w <= 0 || up_h <= 0 || n_open < 0) return LGD_ERR_ARG;
  if (misaligned(attn, 4) || misaligned(boxes, 4) || misaligned(empty, 4) || misaligned(smooth, 4)) return LGD_ERR_ARG;
  const int radius = (int)(4.0 * (double)sigma + 0.5);  // scipy: truncate = 4.0
  if (N > TAIL_MAX_N || (long)hm * wm > PROMPT_MAX_PIX || radius > PROMPT_MAX_RADIUS || n_open > PROMPT_MAX_OPEN)
    return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  BoxPromptArgs a;
  a.attn = attn, a.coarse = coarse, a.boxes = boxes, a.empty = empty, a.smooth = smooth;
  a.hm = hm, a.wm = wm, a.radius = radius, a.n_open = n_open, a.up_w = up_w, a.up_h = up_h;
  a.sigma = sigma, a.mask_th = mask_th;
  hipLaunchKernelGGL(sam_attn_box_prompt_kernel, dim3((unsigned)N), dim3(PROMPT_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return lgd_check_launch();
}
