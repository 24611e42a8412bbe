// Safety checker of the `sd` baseline (reference generation/stable_diffusion_generate.py:14,44-49 builds
// StableDiffusionPipeline with its default checker): what follows the CLIP vision tower and `visual_projection`.
//
//  * safety_head_kernel — the tail of [ext] diffusers StableDiffusionSafetyChecker.forward: cosine scores of the image
//    embedding against the special-care and the concept embeddings, the per-row thresholds, the 0.01 adjustment a special-care
//    hit adds to every row behind it, and the two decisions.  One wave per image: the normalised embedding lives in
//    registers (16-byte loads, <= 4 vectors per lane), every stored row is streamed past it once, norms and dot products are
//    wave64 butterfly sums in fp32.  Row j's cosine ends in lane j & 63 (two registers cover the 96 rows), and the decision
//    rule is evaluated once for the whole wave from ballots of those registers.
//  * blank_flagged_kernel — zeroes the images whose flag is set, in place.  A workgroup reads its image's flag first and
//    returns when it is 0: an unflagged image is neither read nor written.
//
// No atomics; every output element has one owner and is written once.  Built with -ffp-contract=off: the decision
// `(cos - w) + adj`, `* 1000`, `> 0.5` is four separate fp32 operations.
#include "common.h"
#include "contract.h"
#include "../../include/lgd_hip.h"

#include <limits.h>

namespace {

constexpr int SAFETY_MAX_D = 1024, SAFETY_MAX_SPECIAL = 32, SAFETY_MAX_CONCEPTS = 64, SAFETY_MAX_B = 65535;
constexpr int SAFETY_WAVES = 4;
constexpr int BLANK_THREADS = 256, BLANK_MAX_CHUNKS = 64, BLANK_VECS_PER_THREAD = 4;

struct SafetyArgs {
  const float* embeds;    // [B][ld]
  const float *special, *special_w, *concepts, *concept_w;
  float* scores;          // [B][ns + nc]
  int32_t* flags;         // [B][2]
  long ld;
  int B, D, ns, nc;
};

// round(score, 3) > 0 of a numpy.float32: the fp32 product against 0.5 (include/lgd_hip.h)
__device__ __forceinline__ bool safety_hit(float s) { return s * 1000.f > 0.5f; }

// KV = 16-byte vectors of a row per lane: D <= 256 * KV (a compile-time bound keeps the rows in registers)
template <int KV>
__global__ __launch_bounds__(SAFETY_WAVES* LGD_WAVE) void safety_head_kernel(const SafetyArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * SAFETY_WAVES + (threadIdx.x >> 6);  // image of this wave (wave-uniform)
  if (b >= a.B) return;
  const int total = a.ns + a.nc;

  f32x4 ev[KV];
  float ee = 0.f;
  const float* er = a.embeds + (long)b * a.ld;
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int c = (k * LGD_WAVE + lane) * 4;
    ev[k] = c < a.D ? *reinterpret_cast<const f32x4*>(er + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) ee = fmaf(ev[k][i], ev[k][i], ee);
  }
  const float ne = fmaxf(sqrtf(wave_sum(ee)), 1e-12f);
#pragma unroll
  for (int k = 0; k < KV; ++k) ev[k] = ev[k] / ne;

  float cos0 = 0.f, cos1 = 0.f;  // rows lane and lane + 64
  for (int j = 0; j < total; ++j) {
    const float* cr = j < a.ns ? a.special + (long)j * a.D : a.concepts + (long)(j - a.ns) * a.D;
    f32x4 cv[KV];
    float cc = 0.f;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const int c = (k * LGD_WAVE + lane) * 4;
      cv[k] = c < a.D ? *reinterpret_cast<const f32x4*>(cr + c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) cc = fmaf(cv[k][i], cv[k][i], cc);
    }
    const float nc = fmaxf(sqrtf(wave_sum(cc)), 1e-12f);
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < KV; ++k) {
      const f32x4 n = cv[k] / nc;
#pragma unroll
      for (int i = 0; i < 4; ++i) dot = fmaf(ev[k][i], n[i], dot);
    }
    dot = wave_sum(dot);
    if (lane == (j & 63)) {
      if (j < LGD_WAVE) cos0 = dot;
      else cos1 = dot;
    }
  }

  // The rule walks the special rows in ascending order with adj = 0 until the first hit and 0.01 behind it: adj is 0 for
  // every row up to and including the FIRST special row that hits under adj = 0, and 0.01 for every row after that one.
  const int r0 = lane, r1 = lane + LGD_WAVE;
  const bool in0 = r0 < total, in1 = r1 < total;
  const float w0 = !in0 ? 0.f : r0 < a.ns ? a.special_w[r0] : a.concept_w[r0 - a.ns];
  const float w1 = in1 ? a.concept_w[r1 - a.ns] : 0.f;  // ns <= 32: rows >= 64 are concepts
  const float raw0 = cos0 - w0, raw1 = cos1 - w1;
  const unsigned long long first_mask = __ballot(r0 < a.ns && safety_hit(raw0 + 0.f));
  const int first = first_mask ? __ffsll(first_mask) - 1 : INT_MAX;
  const float s0 = raw0 + (r0 > first ? 0.01f : 0.f);
  const float s1 = raw1 + (r1 > first ? 0.01f : 0.f);
  const bool concept0 = in0 && r0 >= a.ns && safety_hit(s0);
  const bool concept1 = in1 && safety_hit(s1);
  const unsigned long long nsfw = __ballot(concept0 || concept1);
  float* sr = a.scores + (long)b * total;
  if (in0) sr[r0] = s0;
  if (in1) sr[r1] = s1;
  if (lane == 0) a.flags[2 * (long)b] = nsfw ? 1 : 0;
  if (lane == 1) a.flags[2 * (long)b + 1] = first_mask ? 1 : 0;
}

struct BlankArgs {
  uint8_t* images;
  const int32_t* flags;
  long image_bytes, flag_stride;
  int chunks;
};

__global__ __launch_bounds__(BLANK_THREADS) void blank_flagged_kernel(const BlankArgs a) {
  const long n = blockIdx.x / a.chunks;
  const int chunk = blockIdx.x - (int)n * a.chunks;
  if (a.flags[n * a.flag_stride] == 0) return;
  uint8_t* p = a.images + n * a.image_bytes;
  long head = (long)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15);
  if (head > a.image_bytes) head = a.image_bytes;
  const long vecs = (a.image_bytes - head) >> 4;
  const long tail = head + (vecs << 4);  // first byte behind the vector body
  if (chunk == 0) {                      // at most 15 bytes on each side
    if ((long)threadIdx.x < head) p[threadIdx.x] = 0;
    if (tail + (long)threadIdx.x < a.image_bytes) p[tail + threadIdx.x] = 0;
  }
  uint4* body = reinterpret_cast<uint4*>(p + head);
  for (long v = (long)chunk * BLANK_THREADS + threadIdx.x; v < vecs; v += (long)a.chunks * BLANK_THREADS)
    body[v] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

extern "C" int lgd_safety_head_f32(const float* embeds, int64_t ld_embeds, const float* special, const float* special_w,
                                   int n_special, const float* concepts, const float* concept_w, int n_concepts,
                                   float* scores, int32_t* flags, int B, int D, void* stream) {
  using namespace lgd_contract;
  if (!embeds || !concepts || !concept_w || !scores || !flags) return LGD_ERR_ARG;
  if (n_special < 0 || (n_special > 0 && (!special || !special_w))) return LGD_ERR_ARG;
  if (B <= 0 || D <= 0 || n_concepts <= 0 || D % 4 || ld_embeds < D || ld_embeds % 4) return LGD_ERR_ARG;
  if (misaligned(embeds, 16) || misaligned(special, 16) || misaligned(concepts, 16) || misaligned(special_w, 4) ||
      misaligned(concept_w, 4) || misaligned(scores, 4) || misaligned(flags, 4))
    return LGD_ERR_ARG;
  if (D > SAFETY_MAX_D || n_special > SAFETY_MAX_SPECIAL || n_concepts > SAFETY_MAX_CONCEPTS || B > SAFETY_MAX_B)
    return LGD_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)n_special + n_concepts;
  const int64_t scores_b = (int64_t)B * total * 4, flags_b = (int64_t)B * 2 * 4;
  const struct { const void* p; int64_t bytes; } in[] = {{embeds, ((int64_t)(B - 1) * ld_embeds + D) * 4},
                                                         {special, (int64_t)n_special * D * 4},
                                                         {special_w, (int64_t)n_special * 4},
                                                         {concepts, (int64_t)n_concepts * D * 4},
                                                         {concept_w, (int64_t)n_concepts * 4}};
  for (const auto& i : in)
    if (i.bytes > 0 && (overlaps(scores, scores_b, i.p, i.bytes) || overlaps(flags, flags_b, i.p, i.bytes)))
      return LGD_ERR_ARG;
  if (overlaps(scores, scores_b, flags, flags_b)) return LGD_ERR_ARG;
  (void)hipGetLastError();
  SafetyArgs a;
  a.embeds = embeds;
  a.special = special, a.special_w = special_w, a.concepts = concepts, a.concept_w = concept_w;
  a.scores = scores, a.flags = flags;
  a.ld = ld_embeds;
  a.B = B, a.D = D, a.ns = n_special, a.nc = n_concepts;
  const dim3 grid((unsigned)((B + SAFETY_WAVES - 1) / SAFETY_WAVES)), block(SAFETY_WAVES * LGD_WAVE);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (D <= 256) hipLaunchKernelGGL(safety_head_kernel<1>, grid, block, 0, st, a);
  else if (D <= 512) hipLaunchKernelGGL(safety_head_kernel<2>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(safety_head_kernel<4>, grid, block, 0, st, a);
  return lgd_check_launch();
}

extern "C" int lgd_blank_flagged_u8(uint8_t* images, int64_t image_bytes, const int32_t* flags, int64_t flag_stride, int N,
                                    void* stream) {
  using namespace lgd_contract;
  if (!images || !flags || image_bytes <= 0 || flag_stride <= 0 || N <= 0) return LGD_ERR_ARG;
  if (misaligned(flags, 4)) return LGD_ERR_ARG;
  if (image_bytes > INT64_MAX / N || flag_stride > INT64_MAX / 4 / N) return LGD_ERR_UNSUPPORTED;
  if (overlaps(images, image_bytes * N, flags, ((int64_t)(N - 1) * flag_stride + 1) * 4)) return LGD_ERR_ARG;
  const int64_t per_block = (int64_t)BLANK_THREADS * 16 * BLANK_VECS_PER_THREAD;
  int64_t chunks = (image_bytes + per_block - 1) / per_block;
  if (chunks > BLANK_MAX_CHUNKS) chunks = BLANK_MAX_CHUNKS;
  if ((int64_t)N * chunks > INT_MAX) return LGD_ERR_UNSUPPORTED;
  (void)hipGetLastError();
  BlankArgs a;
  a.images = images;
  a.flags = flags;
  a.image_bytes = image_bytes, a.flag_stride = flag_stride;
  a.chunks = (int)chunks;
  hipLaunchKernelGGL(blank_flagged_kernel, dim3((unsigned)(N * chunks)), dim3(BLANK_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), a);
  return lgd_check_launch();
}
