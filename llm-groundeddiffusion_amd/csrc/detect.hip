// Detection tail of the stage-2 evaluator (reference scripts/owl_vit_eval.py -> utils/eval/eval.py::eval_prompt, which
// calls the Hugging Face `OwlViTForObjectDetection`): what follows the GEMMs of the class and box heads.
//
//  * owl_heads_kernel — the tail of [ext] transformers OwlViTClassPredictionHead.forward (normalise both sides with the
//    +1e-6, similarity, shift, elu(scale) + 1, query mask) and of OwlViTForObjectDetection.box_predictor (bias table,
//    sigmoid).  One wave per image token: the token's class embedding lives in registers (fp16 -> fp32, <= 16 values per
//    lane), every query row is streamed past it once, and norms and dot products are wave64 butterfly sums in fp32.
//  * detect_nms_kernel — `post_process` (sigmoid of the best logit, its first index, cxcywh -> xyxy), the score filter
//    of eval.py:144-148 and the greedy loops of eval.py:11-105 (`nms`, `class_aware_nms`), one workgroup per image.
//    Candidates are ordered by ONE bitonic sort in LDS over the key (label when class-aware | score descending | token
//    index ascending), so the class-aware form is the same walk with suppression confined to equal labels and its output
//    order (labels ascending, each label's picks by descending score) is the sorted order itself.  The walk makes one
//    round per PICKED box: all lanes find the next live candidate in the LDS flags, then the candidates behind it are
//    tested against it in parallel.  No atomics; every store has one owner; the result does not depend on timing.
//    numpy's argsort (eval.py:45) leaves the order of equal scores open; here the lower token index goes first.
#include "common.h"
#include "../../include/lgd_hip.h"

#include <float.h>

namespace {

constexpr int HEADS_MAX_D = 1024, HEADS_MAX_Q = 64, HEADS_WAVES = 4;
constexpr int NMS_MAX_P = 4096, NMS_THREADS = 256;

__device__ __forceinline__ float sigmoid_exact_f(float x) { return 1.f / (1.f + expf(-x)); }

struct HeadsArgs {
  const half_t* e;    // [B*P][ld_e]
  const float* query; // [B][Q][D]
  const int32_t* mask;
  const float *shift, *scale_raw;
  const void* box_raw;
  const float* box_bias;
  float *logits, *boxes;
  long ld_e, ld_ss;
  int B, P, Q, D, box_f32;
};

// KV = values of the class embedding per lane: D <= 64 * KV (a compile-time bound keeps `ev` in registers)
template <int KV>
__global__ __launch_bounds__(HEADS_WAVES* LGD_WAVE) void owl_heads_kernel(const HeadsArgs a) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * HEADS_WAVES + (threadIdx.x >> 6);  // token of this wave (wave-uniform)
  if (t >= (long)a.B * a.P) return;
  const int b = (int)(t / a.P), p = (int)(t - (long)b * a.P);

  float ev[KV];
  float ee = 0.f;
  const half_t* er = a.e + t * a.ld_e;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int c = k * LGD_WAVE + lane;
    ev[k] = c < a.D ? (float)er[c] : 0.f;
    ee = fmaf(ev[k], ev[k], ee);
  }
  const float ne = sqrtf(wave_sum(ee)) + 1e-6f;
  const float shift = a.shift[t * a.ld_ss];
  const float sr = a.scale_raw[t * a.ld_ss];
  const float scale = sr > 0.f ? sr + 1.f : expf(sr);  // elu(x) + 1

  float mine = 0.f;
  for (int q = 0; q < a.Q; ++q) {
    const float* qr = a.query + ((long)b * a.Q + q) * a.D;
    float dot = 0.f, qq = 0.f;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int c = k * LGD_WAVE + lane;
      const float qv = c < a.D ? qr[c] : 0.f;
      dot = fmaf(ev[k], qv, dot);
      qq = fmaf(qv, qv, qq);
    }
    dot = wave_sum(dot);
    const float nq = sqrtf(wave_sum(qq)) + 1e-6f;
    float v = (dot / (ne * nq) + shift) * scale;
    if (a.mask && a.mask[b * a.Q + q] == 0) v = -FLT_MAX;
    if (lane == q) mine = v;
  }
  if (lane < a.Q) a.logits[t * a.Q + lane] = mine;
  if (lane < 4) {
    const float raw = a.box_f32 ? static_cast<const float*>(a.box_raw)[t * 4 + lane]
                                : (float)static_cast<const half_t*>(a.box_raw)[t * 4 + lane];
    a.boxes[t * 4 + lane] = sigmoid_exact_f(raw + a.box_bias[p * 4 + lane]);
  }
}

struct NmsArgs {
  const float* in0;      // mode 0: logits [B][P][Q];     mode 1: scores [B][P]
  const float* in_boxes; // mode 0: cxcywh [B][P][4];     mode 1: xyxy [B][P][4]
  const int32_t* in_labels;
  const int32_t* in_count;
  float *out_boxes, *out_scores;
  int32_t *out_labels, *out_index, *out_count;
  int B, P, Q, mode, class_aware;
  float score_thr, nms_thr;
};

struct Box {
  float x0, y0, x1, y1;
};

__device__ __forceinline__ Box load_box(const NmsArgs& a, int b, int i) {
  const f32x4 v = *reinterpret_cast<const f32x4*>(a.in_boxes + ((long)b * a.P + i) * 4);
  if (a.mode) return {v[0], v[1], v[2], v[3]};
  const float hw = v[2] / 2, hh = v[3] / 2;  // post_process / center_to_corners_format
  return {v[0] - hw, v[1] - hh, v[0] + hw, v[1] + hh};
}

// key bits: [63:44] label (class-aware only) | [43:12] ~score bits (scores are >= 0: the bit pattern is monotonic) |
// [11:0] token index
constexpr uint64_t KEY_NONE = ~0ull;

__global__ __launch_bounds__(NMS_THREADS) void detect_nms_kernel(const NmsArgs a) {
  __shared__ uint64_t s_key[NMS_MAX_P];
  __shared__ unsigned char s_dead[NMS_MAX_P];
  __shared__ int s_red[NMS_THREADS / LGD_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x;
  int N2 = 1;
  while (N2 < a.P) N2 <<= 1;
  const int limit = a.in_count ? min(max(a.in_count[b], 0), a.P) : a.P;

  // ---- score, label, filter
  int mine = 0;
  for (int i = tid; i < N2; i += NMS_THREADS) {
    uint64_t key = KEY_NONE;
    if (i < limit) {
      float score;
      int label;
      if (a.mode) {
        score = a.in0[(long)b * a.P + i] + 0.f;  // -0 -> +0: the key needs the bit pattern of a non-negative float
        label = a.in_labels ? a.in_labels[(long)b * a.P + i] : 0;
      } else {
        const float* lg = a.in0 + ((long)b * a.P + i) * a.Q;
        float best = lg[0];
        label = 0;
        for (int q = 1; q < a.Q; ++q) {
          const float v = lg[q];
          if (v > best) best = v, label = q;  // the first of equal maxima, as torch.max
        }
        score = sigmoid_exact_f(best);
      }
      if (score >= a.score_thr && score >= 0.f) {
        const uint64_t lab = a.class_aware ? ((uint64_t)(uint32_t)label & 0xfffffull) : 0ull;
        key = (lab << 44) | ((uint64_t)(~__float_as_uint(score)) << 12) | (uint64_t)i;
        ++mine;
      }
    }
    s_key[i] = key;
    s_dead[i] = 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((tid & 63) == 0) s_red[tid >> 6] = mine;
  __syncthreads();
  const int n = s_red[0] + s_red[1] + s_red[2] + s_red[3];

  // ---- bitonic sort, ascending keys (unique but for the KEY_NONE padding)
  for (int k = 2; k <= N2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < N2; i += NMS_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint64_t x = s_key[i], y = s_key[ixj];
          if ((x > y) == ((i & k) == 0)) s_key[i] = y, s_key[ixj] = x;
        }
      }
      __syncthreads();
    }
  }

  // ---- greedy walk: one round per picked box
  int cur = 0, cnt = 0;
  const long ob = (long)b * a.P;
  while (true) {
    while (cur < n && s_dead[cur]) ++cur;
    if (cur >= n) break;
    const uint64_t kc = s_key[cur];
    const int ic = (int)(kc & 0xfff);
    const uint64_t lc = kc >> 44;
    const Box bc = load_box(a, b, ic);
    const float area_c = (bc.x1 - bc.x0) * (bc.y1 - bc.y0);
    if (tid == 0) {
      *reinterpret_cast<f32x4*>(a.out_boxes + (ob + cnt) * 4) = (f32x4){bc.x0, bc.y0, bc.x1, bc.y1};
      a.out_scores[ob + cnt] = __uint_as_float(~(uint32_t)(kc >> 12));
      int label;
      if (a.mode) {
        label = a.in_labels ? a.in_labels[ob + ic] : 0;
      } else {
        const float* lg = a.in0 + (ob + ic) * a.Q;
        float best = lg[0];
        label = 0;
        for (int q = 1; q < a.Q; ++q)
          if (lg[q] > best) best = lg[q], label = q;
      }
      a.out_labels[ob + cnt] = label;
      a.out_index[ob + cnt] = ic;
    }
    ++cnt;
    for (int j = cur + 1 + tid; j < n; j += NMS_THREADS) {
      const uint64_t kj = s_key[j];
      if (s_dead[j] || (kj >> 44) != lc) continue;
      const Box bj = load_box(a, b, (int)(kj & 0xfff));
      const float w = fmaxf(0.f, fminf(bc.x1, bj.x1) - fmaxf(bc.x0, bj.x0));
      const float h = fmaxf(0.f, fminf(bc.y1, bj.y1) - fmaxf(bc.y0, bj.y0));
      const float inter = w * h;
      const float area_j = (bj.x1 - bj.x0) * (bj.y1 - bj.y0);
      const float ratio = inter / (area_c + area_j - inter);
      if (!(ratio < a.nms_thr)) s_dead[j] = 1;  // eval.py:75 keeps `ratio < threshold` (a NaN ratio is dropped too)
    }
    ++cur;
    __syncthreads();
  }
  if (tid == 0) a.out_count[b] = cnt;
}

inline bool misaligned(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) & (n - 1); }

}  // namespace

extern "C" int lgd_owl_heads_f32(const void* class_embeds, int64_t ld_embeds, const float* query_embeds,
                                 const int32_t* query_mask, const float* shift, const float* scale_raw, int64_t ld_ss,
                                 const void* box_raw, int box_is_f32, const float* box_bias, float* logits,
                                 float* pred_boxes, int B, int P, int Q, int D, void* stream) {
  if (!class_embeds || !query_embeds || !shift || !scale_raw || !box_raw || !box_bias || !logits || !pred_boxes)
    return LGD_ERR_ARG;
  if (B <= 0 || P <= 0 || Q <= 0 || D <= 0 || ld_embeds < D || ld_ss < 1) return LGD_ERR_ARG;
  if (D > HEADS_MAX_D || Q > HEADS_MAX_Q) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  HeadsArgs a;
  a.e = static_cast<const half_t*>(class_embeds);
  a.query = query_embeds;
  a.mask = query_mask;
  a.shift = shift;
  a.scale_raw = scale_raw;
  a.box_raw = box_raw;
  a.box_bias = box_bias;
  a.logits = logits;
  a.boxes = pred_boxes;
  a.ld_e = ld_embeds;
  a.ld_ss = ld_ss;
  a.B = B, a.P = P, a.Q = Q, a.D = D, a.box_f32 = box_is_f32 ? 1 : 0;
  const long tokens = (long)B * P;
  const unsigned grid = (unsigned)((tokens + HEADS_WAVES - 1) / HEADS_WAVES);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 block(HEADS_WAVES * LGD_WAVE);
  if (D <= 64) hipLaunchKernelGGL(owl_heads_kernel<1>, dim3(grid), block, 0, st, a);
  else if (D <= 128) hipLaunchKernelGGL(owl_heads_kernel<2>, dim3(grid), block, 0, st, a);
  else if (D <= 256) hipLaunchKernelGGL(owl_heads_kernel<4>, dim3(grid), block, 0, st, a);
  else if (D <= 512) hipLaunchKernelGGL(owl_heads_kernel<8>, dim3(grid), block, 0, st, a);
  else if (D <= 768) hipLaunchKernelGGL(owl_heads_kernel<12>, dim3(grid), block, 0, st, a);
  else hipLaunchKernelGGL(owl_heads_kernel<16>, dim3(grid), block, 0, st, a);
  return lgd_check_launch();
}

extern "C" int lgd_detect_nms_f32(int mode, const float* logits_or_scores, const float* boxes, const int32_t* labels,
                                  const int32_t* counts, int B, int P, int Q, float score_threshold,
                                  float nms_threshold, int class_aware, float* out_boxes, float* out_scores,
                                  int32_t* out_labels, int32_t* out_index, int32_t* out_count, void* stream) {
  if ((mode != 0 && mode != 1) || !logits_or_scores || !boxes || !out_boxes || !out_scores || !out_labels ||
      !out_index || !out_count)
    return LGD_ERR_ARG;
  if (B <= 0 || P <= 0 || (mode == 0 && Q <= 0)) return LGD_ERR_ARG;
  if (misaligned(boxes, 16) || misaligned(out_boxes, 16)) return LGD_ERR_ARG;
  if (P > NMS_MAX_P) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  NmsArgs a;
  a.in0 = logits_or_scores;
  a.in_boxes = boxes;
  a.in_labels = mode ? labels : nullptr;
  a.in_count = mode ? counts : nullptr;
  a.out_boxes = out_boxes;
  a.out_scores = out_scores;
  a.out_labels = out_labels;
  a.out_index = out_index;
  a.out_count = out_count;
  a.B = B, a.P = P, a.Q = Q, a.mode = mode, a.class_aware = class_aware ? 1 : 0;
  a.score_thr = score_threshold;
  a.nms_thr = nms_threshold;
  hipLaunchKernelGGL(detect_nms_kernel, dim3((unsigned)B), dim3(NMS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
  return lgd_check_launch();
}
