// The hand-off between the two stages of LMD / LMD+ for all layouts of a batch, without a host read: what
// utils/latents.py:85-118 (`align_with_bboxes`, `compose_latents_with_alignment`), utils/utils.py:72-123,145-180
// (`binary_mask_to_box`, `binary_mask_to_box_mask`, `binary_mask_to_center`, `shift_tensor`), utils/latents.py:38-83
// (`compose_latents`), utils/attn.py:40-70 (`shift_saved_attns`) and utils/guidance.py:201 (the gather of the saved maps
// into the reference tensor) compute on the host, box by box.
//
//  * handoff_place_kernel — one workgroup per layout.  Per box: the integer sums of the mask, the fp32 centre, the fp64
//    offset and its half-to-even rounding on the 8 x 8 grid, the area and the grown bounding box of the SHIFTED mask.
//    Then the painter's order (descending shifted area, equal areas lower index first) and, per pixel, the last box in
//    that order whose shifted mask / grown box covers it.  Everything a later box would overwrite on the host is never
//    written here: the two owner maps name the one box whose value survives.
//  * handoff_compose_kernel — one thread per output element: `composed`, `fg_idx` and (optionally) the aligned histories
//    are one gather each through the owner maps and the plan rows.
//  * handoff_ref_maps_kernel — one thread per element of the reference-map tensor the energy kernel reads.
//
// Copy and integer work only; compiled with floating-point contraction off so that the offset arithmetic rounds where
// Python's does.  No atomics, no memset in front: every output element is written once, by one owner.
#include "common.h"

namespace {

constexpr int HO_THREADS = 256, HO_MAX_BOXES = 64, HO_MAX_SIDE = 1024, HO_PLAN = 8;
constexpr int HO_MAX_LAYOUTS = 65535;
// plan row (int32 x 8): pixel offset, shifted area, grown box of the shifted mask (inclusive, as binary_mask_to_box
// returns it: the far side is clipped to L, not L - 1), empty flag
enum { P_OX = 0, P_OY, P_AREA, P_X0, P_Y0, P_X1, P_Y1, P_EMPTY };

struct PlaceArgs {
  const uint8_t* masks;    // [NB][L][L], non-zero = inside
  const double* targets;   // [NB][4] xyxy in [0, 1]
  const int32_t* seg;      // [NL + 1]: layout l owns boxes seg[l] .. seg[l + 1] - 1
  int32_t* plan;           // [NB][8]
  int32_t* win;            // [NL][2][L][L]: win_mask, win_box (box index inside the layout, or -1)
  int L, align, horizontal_only;
};

// block-wide reductions for HO_THREADS threads; `red`: HO_THREADS / 64 slots of LDS.  Every thread gets the result.
__device__ __forceinline__ long long block_sum_ll(long long v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  long long r = 0;
#pragma unroll
  for (int i = 0; i < HO_THREADS / LGD_WAVE; ++i) r += red[i];
  return r;
}
__device__ __forceinline__ int block_min_i(int v, long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = (int)red[0];
#pragma unroll
  for (int i = 1; i < HO_THREADS / LGD_WAVE; ++i) r = min(r, (int)red[i]);
  return r;
}

// round(v * 8) of Python (half to even) times the width of an eighth of the frame: shift_tensor with offset_normalized
__device__ __forceinline__ int quantised_offset(double v, int L) { return (int)rint(v * 8.0) * (L / 8); }

__global__ __launch_bounds__(HO_THREADS) void handoff_place_kernel(const PlaceArgs a) {
  __shared__ long long s_red[HO_THREADS / LGD_WAVE];
  __shared__ int s_row[HO_MAX_BOXES][HO_PLAN];
  __shared__ int s_order[HO_MAX_BOXES];
  const int lay = blockIdx.x, tid = threadIdx.x, L = a.L, P = L * L;
  const int b0 = a.seg[lay], nb = min(max(a.seg[lay + 1] - b0, 0), HO_MAX_BOXES);

#pragma unroll 1
  for (int i = 0; i < nb; ++i) {
    const uint8_t* m = a.masks + (long)(b0 + i) * P;
    long long n = 0, sx = 0, sy = 0;
#pragma unroll 1
    for (int p = tid; p < P; p += HO_THREADS) {
      if (m[p]) {
        const int y = p / L, x = p - y * L;
        n += 1, sx += x, sy += y;
      }
    }
    n = block_sum_ll(n, s_red), sx = block_sum_ll(sx, s_red), sy = block_sum_ll(sy, s_red);
    int ox = 0, oy = 0;
    if (a.align && n > 0) {
      // binary_mask_to_center on a torch mask: one fp32 division of the two integer sums; the rest is Python's fp64
      const double* t = a.targets + (long)(b0 + i) * 4;
      const double cx = (double)((float)sx / (float)n) / (double)L;
      const double cy = (double)((float)sy / (float)n) / (double)L;
      ox = quantised_offset((t[0] + t[2]) / 2 - cx, L);
      oy = a.horizontal_only ? 0 : quantised_offset((t[1] + t[3]) / 2 - cy, L);
    }
    // the shifted mask M(y, x) = m(y - oy, x - ox): its area and bounding box, walked over the source pixels
    long long area = 0;
    int x_lo = L, y_lo = L, x_hi = -1, y_hi = -1;
#pragma unroll 1
    for (int p = tid; p < P; p += HO_THREADS) {
      if (m[p]) {
        const int y = p / L + oy, x = p % L + ox;
        if (x >= 0 && x < L && y >= 0 && y < L) {
          area += 1;
          x_lo = min(x_lo, x), y_lo = min(y_lo, y), x_hi = max(x_hi, x), y_hi = max(y_hi, y);
        }
      }
    }
    area = block_sum_ll(area, s_red);
    x_lo = block_min_i(x_lo, s_red), y_lo = block_min_i(y_lo, s_red);
    x_hi = -block_min_i(-x_hi, s_red), y_hi = -block_min_i(-y_hi, s_red);
    if (tid == 0) {
      const bool empty = area == 0;
      s_row[i][P_OX] = ox, s_row[i][P_OY] = oy, s_row[i][P_AREA] = (int)area;
      s_row[i][P_X0] = empty ? 0 : max(x_lo - 1, 0), s_row[i][P_Y0] = empty ? 0 : max(y_lo - 1, 0);
      s_row[i][P_X1] = empty ? -1 : min(x_hi + 1, L), s_row[i][P_Y1] = empty ? -1 : min(y_hi + 1, L);
      s_row[i][P_EMPTY] = empty ? 1 : 0;
    }
  }
  __syncthreads();
  // painter's order: descending shifted area, equal areas lower index first (a stable sort of -area)
  for (int i = tid; i < nb; i += HO_THREADS) {
    int rank = 0;
    for (int j = 0; j < nb; ++j) {
      const int aj = s_row[j][P_AREA], ai = s_row[i][P_AREA];
      rank += (aj > ai || (aj == ai && j < i)) ? 1 : 0;
    }
    s_order[rank] = i;
  }
  for (int e = tid; e < nb * HO_PLAN; e += HO_THREADS) a.plan[(long)b0 * HO_PLAN + e] = s_row[e / HO_PLAN][e % HO_PLAN];
  __syncthreads();

  int32_t* wm_out = a.win + (long)lay * 2 * P;
  int32_t* wb_out = wm_out + P;
#pragma unroll 1
  for (int p = tid; p < P; p += HO_THREADS) {
    const int y = p / L, x = p - y * L;
    int wm = -1, wb = -1;
#pragma unroll 1
    for (int k = 0; k < nb; ++k) {
      const int i = s_order[k];
      if (s_row[i][P_EMPTY]) continue;
      const int sx = x - s_row[i][P_OX], sy = y - s_row[i][P_OY];
      if (sx >= 0 && sx < L && sy >= 0 && sy < L && a.masks[(long)(b0 + i) * P + sy * L + sx]) wm = i;
      if (x >= s_row[i][P_X0] && x <= s_row[i][P_X1] && y >= s_row[i][P_Y0] && y <= s_row[i][P_Y1]) wb = i;
    }
    wm_out[p] = wm, wb_out[p] = wb;
  }
}

struct ComposeArgs {
  const int32_t* plan;     // [NB][8]
  const int32_t* win;      // [NL][2][L][L]
  const int32_t* seg;      // [NL + 1]
  const int64_t* hist;     // [NB][2]: address of the box's history (fp32 [rows][C][L][L] at a step stride), that stride
  const float* bg;         // [NL][C][L][L]
  float* composed;         // [NL][S1][C][L][L]
  int64_t* fg_idx;         // [NL][L][L]
  float* aligned;          // [NB][rows][C][L][L] or NULL
  int NL, NB, S1, C, L, rows;
  long n_comp, n_fg, n_al;
};

// the box's history at step t, channel c, read at the source of (y, x) under the box's offset; 0 outside the frame
__device__ __forceinline__ float hist_at(const ComposeArgs& a, int box, int t, int c, int y, int x) {
  const int32_t* row = a.plan + (long)box * HO_PLAN;
  const int sx = x - row[P_OX], sy = y - row[P_OY];
  if (sx < 0 || sx >= a.L || sy < 0 || sy >= a.L) return 0.f;
  const float* h = reinterpret_cast<const float*>(static_cast<uintptr_t>(a.hist[(long)box * 2]));
  return h[(long)t * a.hist[(long)box * 2 + 1] + ((long)c * a.L + sy) * a.L + sx];
}

__global__ __launch_bounds__(HO_THREADS) void handoff_compose_kernel(const ComposeArgs a) {
  long e = (long)blockIdx.x * HO_THREADS + threadIdx.x;
  const int L = a.L, P = L * L;
  if (e < a.n_comp) {
    const int x = (int)(e % L), y = (int)(e / L % L), c = (int)(e / P % a.C);
    const int t = (int)(e / ((long)P * a.C) % a.S1), lay = (int)(e / ((long)P * a.C * a.S1));
    const int32_t* w = a.win + (long)lay * 2 * P;
    const int b0 = a.seg[lay], wm = w[y * L + x];
    float v = 0.f;
    if (wm >= 0) {
      v = hist_at(a, b0 + wm, t, c, y, x);
    } else if (t == 0) {
      const int wb = w[P + y * L + x];
      v = wb >= 0 ? hist_at(a, b0 + wb, 0, c, y, x) : a.bg[((long)lay * a.C + c) * P + y * L + x];
    }
    a.composed[e] = v;
    return;
  }
  e -= a.n_comp;
  if (e < a.n_fg) {
    const int lay = (int)(e / P), p = (int)(e % P);
    a.fg_idx[e] = (int64_t)(a.win[(long)lay * 2 * P + p] + 1);
    return;
  }
  e -= a.n_fg;
  if (e < a.n_al) {
    const int x = (int)(e % L), y = (int)(e / L % L), c = (int)(e / P % a.C);
    const int t = (int)(e / ((long)P * a.C) % a.rows), box = (int)(e / ((long)P * a.C * a.rows));
    a.aligned[e] = hist_at(a, box, t, c, y, x);
  }
}

struct RefArgs {
  const int32_t* plan;     // [NB][8]
  const int32_t* seg;      // [NL + 1]
  const int32_t* lay_of;   // [NB]: the layout of a box
  const int64_t* maps;     // [NB][NK][3]: address of the saved map (fp32 [rows][1][heads][side^2][1]), rows, side
  float* out;              // per layout [T][n_boxes][NK][heads][max_hw], the layouts back to back
  int NB, T, NK, heads, max_hw, L;
  long n;
};

__global__ __launch_bounds__(HO_THREADS) void handoff_ref_maps_kernel(const RefArgs a) {
  const long e = (long)blockIdx.x * HO_THREADS + threadIdx.x;
  if (e >= a.n) return;
  const int p = (int)(e % a.max_hw), h = (int)(e / a.max_hw % a.heads);
  const int k = (int)(e / ((long)a.max_hw * a.heads) % a.NK);
  const int t = (int)(e / ((long)a.max_hw * a.heads * a.NK) % a.T);
  const int box = (int)(e / ((long)a.max_hw * a.heads * a.NK * a.T));
  const int64_t* m = a.maps + ((long)box * a.NK + k) * 3;
  const int rows = (int)m[1], side = (int)m[2];
  float v = 0.f;
  if (t < rows && p < side * side) {
    // the same quantised eighth of the frame as the latents (shift_saved_attns -> shift_tensor on the map's own grid)
    const int32_t* row = a.plan + (long)box * HO_PLAN;
    const int eighth = a.L / 8;
    const int y = p / side, x = p - y * side;
    const int sx = x - row[P_OX] / eighth * (side / 8), sy = y - row[P_OY] / eighth * (side / 8);
    if (sx >= 0 && sx < side && sy >= 0 && sy < side) {
      const float* src = reinterpret_cast<const float*>(static_cast<uintptr_t>(m[0]));
      v = src[((long)t * a.heads + h) * side * side + sy * side + sx];
    }
  }
  const int lay = a.lay_of[box], b0 = a.seg[lay], nb = a.seg[lay + 1] - b0;
  const long per_box = (long)a.NK * a.heads * a.max_hw;
  a.out[(long)b0 * a.T * per_box + ((long)t * nb + (box - b0)) * per_box + ((long)k * a.heads + h) * a.max_hw + p] = v;
}

inline bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) & (n - 1); }
inline unsigned blocks_for(long n) { return (unsigned)((n + HO_THREADS - 1) / HO_THREADS); }
constexpr long HO_MAX_ELEMS = (long)HO_THREADS * 0x7fffffffL;

}  // namespace

extern "C" int lgd_handoff_place(const uint8_t* masks, const double* targets, const int32_t* seg, int NL, int NB,
                                 int max_boxes, int L, int align, int horizontal_only, int32_t* plan, int32_t* win,
                                 void* stream) {
  if (!seg || !win || (NB > 0 && (!masks || !targets || !plan))) return LGD_ERR_ARG;  // no boxes: no per-box tables
  if (NL <= 0 || NB < 0 || max_boxes < 0 || max_boxes > NB || L <= 0 || L % 8 != 0) return LGD_ERR_ARG;
  if (misaligned(targets, 8) || misaligned(seg, 4) || misaligned(plan, 4) || misaligned(win, 4)) return LGD_ERR_ARG;
  if (max_boxes > HO_MAX_BOXES || L > HO_MAX_SIDE || NL > HO_MAX_LAYOUTS) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  PlaceArgs a;
  a.masks = masks, a.targets = targets, a.seg = seg, a.plan = plan, a.win = win;
  a.L = L, a.align = align ? 1 : 0, a.horizontal_only = horizontal_only ? 1 : 0;
  hipLaunchKernelGGL(handoff_place_kernel, dim3((unsigned)NL), dim3(HO_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     a);
  return lgd_check_launch();
}

extern "C" int lgd_handoff_compose_f32(const int32_t* plan, const int32_t* win, const int32_t* seg, const int64_t* hist,
                                       const float* bg, int NL, int NB, int steps, int C, int L, int rows,
                                       float* composed, int64_t* fg_idx, float* aligned, void* stream) {
  if (!win || !seg || !bg || !composed || !fg_idx || (NB > 0 && (!plan || !hist))) return LGD_ERR_ARG;
  if (NL <= 0 || NB < 0 || steps < 0 || C <= 0 || L <= 0 || L % 8 != 0) return LGD_ERR_ARG;
  if (aligned && rows <= 0) return LGD_ERR_ARG;
  if (misaligned(plan, 4) || misaligned(win, 4) || misaligned(seg, 4) || misaligned(hist, 8) || misaligned(bg, 4) ||
      misaligned(composed, 4) || misaligned(fg_idx, 8) || misaligned(aligned, 4))
    return LGD_ERR_ARG;
  if (L > HO_MAX_SIDE || NL > HO_MAX_LAYOUTS) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  ComposeArgs a;
  a.plan = plan, a.win = win, a.seg = seg, a.hist = hist, a.bg = bg;
  a.composed = composed, a.fg_idx = fg_idx, a.aligned = aligned;
  a.NL = NL, a.NB = NB, a.S1 = steps + 1, a.C = C, a.L = L, a.rows = aligned ? rows : 0;
  a.n_comp = (long)NL * a.S1 * C * L * L;
  a.n_fg = (long)NL * L * L;
  a.n_al = aligned ? (long)NB * rows * C * L * L : 0;
  const long n = a.n_comp + a.n_fg + a.n_al;
  if (n > HO_MAX_ELEMS) return LGD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(handoff_compose_kernel, dim3(blocks_for(n)), dim3(HO_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return lgd_check_launch();
}

extern "C" int lgd_handoff_ref_maps_f32(const int32_t* plan, const int32_t* seg, const int32_t* lay_of,
                                        const int64_t* maps, int NB, int T, int NK, int heads, int max_hw, int L,
                                        float* out, void* stream) {
  if (!plan || !seg || !lay_of || !maps || !out) return LGD_ERR_ARG;
  if (NB <= 0 || T <= 0 || NK <= 0 || heads <= 0 || max_hw <= 0 || L <= 0 || L % 8 != 0) return LGD_ERR_ARG;
  if (misaligned(plan, 4) || misaligned(seg, 4) || misaligned(lay_of, 4) || misaligned(maps, 8) || misaligned(out, 4))
    return LGD_ERR_ARG;
  if (L > HO_MAX_SIDE) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  RefArgs a;
  a.plan = plan, a.seg = seg, a.lay_of = lay_of, a.maps = maps, a.out = out;
  a.NB = NB, a.T = T, a.NK = NK, a.heads = heads, a.max_hw = max_hw, a.L = L;
  a.n = (long)NB * T * NK * heads * max_hw;
  if (a.n > HO_MAX_ELEMS) return LGD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(handoff_ref_maps_kernel, dim3(blocks_for(a.n)), dim3(HO_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return lgd_check_launch();
}
