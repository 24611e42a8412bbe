/*
 * lgd_hip.h — C ABI of liblgd_hip.so: the hand-written gfx950 (MI355X) kernels of the
 * LMD / LMD+ stage-2 denoising hot path.
 *
 * The reference (TonyLianLong/LLM-groundedDiffusion) is pure Python on PyTorch; it has no FFI of
 * its own.  Each entry point below therefore replaces a *PyTorch op sequence* of the reference and
 * cites it (file:line under the reference root).  The ctypes binding a maintainer would add is
 * llm-groundeddiffusion_amd/_lib.py.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless the parameter is documented "host";
 *  - activations / weights are IEEE fp16 (`_Float16`), statistics / biases / losses fp32;
 *  - feature maps are channels-last: [B][H*W][C] row-major ("NHWC"); the UNet boundary tensors
 *    (latents in, noise prediction out) are NCHW fp32 exactly as the reference passes them;
 *  - no allocation, no synchronisation, no host<->device copy inside any call: every output and
 *    workspace is caller-allocated; kernels are enqueued on `stream` (a hipStream_t passed as
 *    void*) and the call returns immediately — all calls are hipGraph-capturable;
 *  - return value: 0 on success, negative LGD_ERR_* otherwise (the Python side raises RuntimeError,
 *    the error convention of the reference's plugin boundary: generate.py:391-396).
 */
#ifndef LGD_HIP_H
#define LGD_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Return codes of every call. */
#define LGD_OK 0
#define LGD_ERR_ARG (-1)
#define LGD_ERR_LAUNCH (-2)
#define LGD_ERR_UNSUPPORTED (-3)

#define LGD_ABI_VERSION 12
int lgd_abi_version(void);
/* Kernel-variant switches of the library (A/B timing and tests; the defaults are what the benchmark runs).  No
 * counterpart in the reference.  "attn32": self-attention forward without map capture — 0 = the 16x16x32 kernel,
 * 1 = (default) the 32x32x16 software-pipelined kernel where it applies (d + 2 <= 96, enough work to fill the chip),
 * 2 = that kernel for every problem size.  "attn_w4": the d = 40 kernel of round 4 (csrc/attn_w4.hip: 4-wave
 * workgroups, LDS-DMA K / V, transposing V reads) — 0 = never, 1 = (default) once a launch has >= 256 workgroups of
 * 256 queries and >= 256 keys, 2 = for every problem size; "attn_w4_pipe": 1 = (default) one wave per SIMD with the
 * in-wave software pipeline, 0 = two waves per SIMD.  "gn_fused": the largest map (pixels per image) lgd_groupnorm_f16
 * normalises in ONE launch (a workgroup holds its image x groups slab in registers); default 256 (16x16), 0 = always
 * the two-launch form.  "gn_slab": 1 = (default) lgd_groupnorm_bwd_f16 runs in one launch where a workgroup can hold its
 * (image, groups) slab of x and gy in registers (<= 96 KB: the 8x8 and 16x16 maps), 0 = two launches.  "ln_stream": 1 =
 * (default) the statistics-only form of lgd_layernorm_f16 (y = NULL) runs the streaming kernel (lane groups share a row),
 * 0 = the one-wave-per-row kernels.  "gn_apply_wgs" (tools): the number of workgroups per launch the GroupNorm apply passes
 * aim at, 64 .. 8192, default 1024.  "cfg_pair": 1 = (default) launch plans of a classifier-free-guidance batch
 * compute the ops in front of the first text / grounding-token read once per pair (LgdGemmDesc.pair, lgd_*_pair_f16),
 * 0 = twice, as before; read by the plan builder when a plan is built (lgd_get_option), the kernels themselves always do
 * what a call asks.  "attn32_nw": waves per workgroup of the 32x32x16 kernel, 8 (default) or 4; "attn32_var" (tools): its
 * fragment prefetch, 0 = (default) 2 slots ahead in pinned order, 1 = 4 ahead, 2 = the compiler's order.
 * Every option has a range and a value outside it is refused, "attn32" (0 .. 2) included.  The initial values of
 * "attn32", "attn32_nw", "attn_w4" and "attn_w4_pipe" come from LGD_ATTN32, LGD_ATTN32_NW, LGD_ATTN_W4 and LGD_W4_PIPE in
 * the environment, read once; a value outside the option's range there leaves the default.  The options are atomics: any
 * thread may set one while others launch.  Returns 0, or LGD_ERR_ARG for an unknown name or a value out of range. */
int lgd_set_option(const char* name, int value);
/* Current value (>= 0) of any option lgd_set_option knows, or LGD_ERR_ARG (negative) for any other name. */
int lgd_get_option(const char* name);

/* ---------------------------------------------------------------------------------------------
 * GEMM / implicit-GEMM convolution on MFMA (v_mfma_f32_16x16x32_f16).
 *   C[m][n] = epilogue( sum_k A(m,k) * W[n][k] )
 * Replaces: nn.Linear / nn.Conv2d calls of the UNet — attention_processor.py:338-363,426-453
 * (to_q/to_k/to_v/to_out), attention.py:286-289,333-335 (FeedForward/GEGLU), transformer_2d.py:
 * 283-291,319-325 (proj_in/proj_out), [ext diffusers 0.18.0] ResnetBlock2D conv1/conv2/
 * conv_shortcut, Downsample2D, Upsample2D (call sites unet_2d_blocks.py:186-197,315-326,360-362,
 * 577-588,621), and their input-gradient (dgrad) forms used by pipelines.py:56.
 *
 * A operand ("taps" = 1: plain rows; "taps" = 9: 3x3 gather, zero padding 1):
 *   A(m,k): k -> (tap, c) with c in [0, c0+c1); c < c0 reads source a0 else a1 (channel concat of
 *   two feature maps without materialising torch.cat, unet_2d_blocks.py:646-649);
 *   taps=9: m -> (b, oy, ox) over hout*wout; input pixel (oy*stride+ky-1, ox*stride+kx-1); with
 *   ups=1 the logical input is the nearest-2x upsampling of the stored hin*win map; with ups=2
 *   it is the zero-inserted map (data at even coordinates only: dgrad of a stride-2 conv).
 * Epilogue (in this order): +bias[n] +bias2[n]; GEGLU pairs (value, gate) column blocks of 16 and
 * emits value*gelu(gate) (N/2 output columns); *alpha; +res[m][n]; store fp16 (or fp32).
 * ------------------------------------------------------------------------------------------- */
#define LGD_EPI_GEGLU 1   /* weights/bias rows packed [16 value | 16 gate] blocks               */
#define LGD_EPI_OUT_F32 2 /* C is fp32                                                           */
#define LGD_EPI_RES_F32 4 /* res is fp32                                                         */
#define LGD_EPI_ROWNORM 8 /* LayerNorm of the A rows folded into the GEMM (ABI v8): the contraction runs on the RAW rows
                             x with W' = W * gamma (per input channel), and the epilogue computes, per row m and column n,
                             rstd[m] * (acc - mean[m] * colsum[n]) before bias / GEGLU / alpha / residual, where
                             colsum[n] = sum_k W'[n][k] and the bias holds b[n] + sum_k beta[k] W[n][k]:
                             LN(x) W^T + b  =  rstd (x W'^T - mean colsum) + b'   (attention.py:185,206,223 followed by
                             attention_processor.py to_q/k/v, attention.py:286-289 GEGLU).  Needs rowstat + colsum. */

typedef struct LgdGemmDesc {
  const void* a0;
  const void* a1;
  int64_t lda0, lda1; /* row (pixel) stride of each source, elements                       */
  int32_t c0, c1;     /* channels taken from a0 / a1; K = taps*(c0+c1)                      */
  int32_t taps;       /* 1 or 9                                                             */
  int32_t hin, win, hout, wout, stride, ups;
  const void* w;      /* [N][K] fp16                                                        */
  int64_t ldw;
  int32_t M, N, K;
  int32_t nb_o, nb_i; /* batch = nb_o*nb_i problems (e.g. image x head)                     */
  int64_t a_bs_o, a_bs_i, w_bs_o, w_bs_i, c_bs_o, c_bs_i, r_bs_o, r_bs_i;
  const float* bias;  /* [N] or NULL                                                        */
  const float* bias2; /* [N] or NULL (time-embedding projection of the current step)        */
  const void* res;    /* [M][ldr] or NULL                                                   */
  int64_t ldr;
  float alpha;
  int32_t epi;
  void* c;
  int64_t ldc;
  int32_t splits;     /* split-K factor (>=1); >1 needs ws                                  */
  float* ws;          /* fp32 [batch][splits][M][N]                                         */
  int32_t tile;       /* 0 auto; else a code of the tile table GEMM_TILES in csrc/gemm.hip (main loop, block shape,
                         the descriptors it serves); lgd_gemm_check tells whether a code serves a descriptor      */
  int32_t* cnt;       /* split-K arrival counters (ABI v5), device int32[batches * tiles], ALL ZERO on entry, or NULL.
                         With counters the split-K combine happens inside the GEMM launch: every workgroup stores its
                         fp32 partial, publishes it (agent-scope release) and takes a ticket; the last arriver of an
                         output tile sums the `splits` partials in split order 0,1,2.. (bit-identical to the separate
                         reduce kernel), applies the epilogue and leaves the counter at zero again.  NULL = second
                         launch (splitk_reduce_kernel).  One counter buffer may serve every GEMM of a stream. */
  const float* rowstat; /* LGD_EPI_ROWNORM: fp32 [M][2] = (mean, rstd) of every A row (lgd_layernorm_f16 with y = NULL) */
  const float* colsum;  /* LGD_EPI_ROWNORM: fp32 [N] = row sums of the (gamma-scaled) weight matrix as stored          */
  int32_t pair;         /* CFG pair mode, 0 = off (field appended behind the v12 layout: LGD_ABI_VERSION stays 12, callers
                           are rebuilt against this header): rows m and m + M/2 of A (and of res / rowstat) are IDENTICAL — the
                           classifier-free-guidance batch [uncond; cond] in front of the first op that reads text or
                           grounding tokens (pipelines.py:436-441 duplicates the latents).  Only rows m < M/2 are computed
                           (tile walk and grid cover M/2 rows; res, rowstat are read for row m only), with the tile the
                           full launch would take: results are bit-identical to it.  LGD_PAIR_HALF: rows >= M/2 of C are
                           left untouched; LGD_PAIR_DUP: every stored piece is also stored at row m + M/2.  Needs
                           splits == 1, nb_o * nb_i == 1 and an even M (for a convolution M/2 is then a whole number
                           of images), else LGD_ERR_ARG. */
} LgdGemmDesc;
#define LGD_PAIR_HALF 1
#define LGD_PAIR_DUP 2

int lgd_gemm_f16(const LgdGemmDesc* desc /* host */, void* stream);
/* lgd_gemm_check (ABI v11): LGD_OK exactly when lgd_gemm_f16 would launch `desc`, else LGD_ERR_ARG — the same check
 * lgd_gemm_f16 runs first.  Host only: no HIP runtime call, pointers count for NULL-ness and alignment and are never
 * dereferenced, so it answers on a host without a GPU (e.g. whether a tuning-table tile serves a descriptor). */
int lgd_gemm_check(const LgdGemmDesc* desc /* host */);
/* lgd_gemm_tile (additive export: LGD_ABI_VERSION stays 12): row `index` (0, 1, ..) of the tile table: the code
 * LgdGemmDesc.tile takes, the block shape and the name of the kernel instantiation the code launches (NUL-terminated, cut
 * to name_cap - 1 characters; every output pointer may be NULL).  LGD_ERR_ARG past the end.  Host only.  The Python
 * binding fills ops.TILE_NAMES (the profiler's kernel names) from it. */
int lgd_gemm_tile(int index, int* code, int* bm, int* bn, char* name, int name_cap);

/* ---------------------------------------------------------------------------------------------
 * conv_in: latents NCHW fp32 (B,4,L,L) -> [B][L*L][Cout] fp16, 3x3 pad 1 (unet_2d_condition.py:860)
 * w: [Cout][3][3][Cin] fp16, bias fp32 [Cout] or NULL.
 * Preconditions (else LGD_ERR_ARG, before any launch): x_nchw, w, y non-NULL; B, L >= 1; 1 <= Cin <= 8; Cout >= 1;
 * x_nchw / bias 4-byte and w / y 2-byte aligned (scalar accesses); y overlaps none of x_nchw, w, bias (no aliasing).
 * LGD_ERR_UNSUPPORTED when the transposed filter and the pixel patches do not fit 64 KB of LDS.
 * ------------------------------------------------------------------------------------------- */
int lgd_conv_in_f16(const float* x_nchw, const void* w, const float* bias, void* y, int B, int Cin,
                    int L, int Cout, void* stream);
/* conv_out: [B][L*L][Cin] fp16 (already GroupNorm+SiLU'd) -> NCHW fp32 (B,Cout,L,L), times
 * out_scale (unet_2d_condition.py:972-975).  w: [Cout][3][3][Cin] fp16.  Called with the
 * flipped/transposed conv_in weights it is also conv_in's input gradient (the latent gradient of
 * pipelines.py:56; out_scale then undoes the fp16 gradient scaling).
 *   y[b][co][oy][ox] = out_scale * (bias[co] + sum_{ky,kx,ci} x[b][oy+ky-1][ox+kx-1][ci] * w[co][ky][kx][ci])
 * (taps outside the map are zero; bias fp32 [Cout] or NULL = 0).
 * Preconditions (else LGD_ERR_ARG, before any launch): x, w, y_nchw non-NULL; B, L >= 1; Cin >= 8 and Cin % 8 == 0;
 * x and w 16-byte aligned (read as 8-half vectors), bias and y_nchw 4-byte; y_nchw overlaps none of x, w, bias (no
 * aliasing).  Cout outside {4, 8}: LGD_ERR_UNSUPPORTED. */
int lgd_conv_out_f16(const void* x, const void* w, const float* bias, float* y_nchw, int B, int Cin,
                     int L, int Cout, float out_scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * GroupNorm (+SiLU) over channels-last maps, two launches: statistics then apply.
 * Replaces [ext] ResnetBlock2D norm1/norm2 + nonlinearity, transformer_2d.py:283 (eps 1e-6, no
 * SiLU) and unet_2d_condition.py:972-974.  x may be the channel concat of two maps (x0: c0
 * channels, x1: c1 channels).  part: fp32 workspace [B][nchunk][G][2]; stats: fp32 [B][G][2]
 * (mean, rstd) written by apply for the backward pass.
 * ------------------------------------------------------------------------------------------- */
int lgd_groupnorm_f16(const void* x0, const void* x1, int c0, int c1, int B, int HW, int G,
                      float eps, const float* gamma, const float* beta, int silu, void* y,
                      float* part, int nchunk, float* stats, void* stream);
/* CFG pair form (additive export: LGD_ABI_VERSION stays 12; see LgdGemmDesc.pair): images b and b + B/2 of x are identical, images b < B/2 are normalised,
 * with the launch geometry of the full call (bit-identical).  LGD_PAIR_HALF: images >= B/2 of y are left untouched;
 * LGD_PAIR_DUP: every stored piece is also stored for image b + B/2.  No statistics output (no-grad forward only). */
int lgd_groupnorm_pair_f16(const void* x0, const void* x1, int c0, int c1, int B, int HW, int G,
                           float eps, const float* gamma, const float* beta, int silu, void* y,
                           float* part, int nchunk, int pair, void* stream);
/* backward of the above w.r.t. x: gy [B][HW][C] -> gx0 (c0 channels, row stride c0) and gx1.
 * accumulate!=0 adds into gx (gradient fan-in). */
int lgd_groupnorm_bwd_f16(const void* gy, const void* x0, const void* x1, int c0, int c1, int B,
                          int HW, int G, const float* gamma, const float* beta, int silu,
                          const float* stats, void* gx0, void* gx1, float* part, int nchunk,
                          int accumulate, void* stream);
/* lgd_groupnorm_plan (additive export: LGD_ABI_VERSION stays 12): the code of the kernel instantiation a GroupNorm call
 * with these arguments runs under the current option state ("gn_fused", "gn_slab") — answered by the function the launches
 * themselves choose their kernel with; host only, nothing is launched.
 *   op = LGD_GN_OP_FWD: lgd_groupnorm_f16 (pair = 0) / lgd_groupnorm_pair_f16 (pair = LGD_PAIR_HALF / LGD_PAIR_DUP; the
 *                       choice follows the full B).  `silu` is not read: every forward kernel serves both.
 *   op = LGD_GN_OP_BWD: lgd_groupnorm_bwd_f16 (pair must be 0).
 * Negative: LGD_ERR_ARG, as the launch would answer.
 * Preconditions of the three GroupNorm entry points (else LGD_ERR_ARG, before anything touches the device):
 *   1 <= G <= 64; B >= 1; HW >= 1; c0 >= 8, c1 >= 0, both multiples of 8; c0 + c1 <= 4096 and a multiple of G;
 *   nchunk >= 1; x0, gamma, beta, y and part not NULL (part also where one launch does not read it); x1 not NULL when
 *   c1 > 0; pair form: pair LGD_PAIR_HALF or LGD_PAIR_DUP and B even (it has no statistics output);
 *   backward: gy, stats, gx0 and part not NULL, x1 and gx1 not NULL when c1 > 0.
 * The plan query checks those of them that its arguments show. */
#define LGD_GN_OP_FWD 0
#define LGD_GN_OP_BWD 1
/* (lgd_norm_variant below names the kernel instantiation behind each code) */
#define LGD_GN_FUSED_4 104            /* forward in one launch, at most 4 pixels per thread */
#define LGD_GN_FUSED_8 108            /* at most 8 */
#define LGD_GN_FUSED_16 116           /* at most 16 */
#define LGD_GN_FUSED_32 132           /* at most 32 */
#define LGD_GN_TWO_LAUNCH 201         /* forward in two launches (statistics, apply), one channel pass (C <= 2048) */
#define LGD_GN_TWO_LAUNCH_2PASS 202   /* the same, two channel passes */
#define LGD_GN_BWD_SLAB_256 300       /* backward in one launch, 256 threads hold the slab in registers */
#define LGD_GN_BWD_SLAB_256_SILU 301  /* the same through SiLU */
#define LGD_GN_BWD_SLAB_512 310       /* 512 threads */
#define LGD_GN_BWD_SLAB_512_SILU 311  /* the same through SiLU */
#define LGD_GN_BWD_TWO_LAUNCH 400     /* backward in two launches */
int lgd_groupnorm_plan(int op, int c0, int c1, int B, int HW, int G, int silu, int pair);

/* LayerNorm over the last dim (attention.py:185,206,223; GatedSelfAttentionDense norm1/norm2
 * attention.py:35-36,50-51). rows x C, C % 8 == 0. y row stride ldy (lets the fuser write visual
 * tokens into the [S+30] concat buffer). stats [rows][2] (mean, rstd) optional. */
int lgd_layernorm_f16(const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int C, float eps,
                      const float* gamma, const float* beta, float* stats, int rows_per_batch,
                      int64_t x_bs, int64_t y_bs, void* stream);
/* CFG pair form (additive export: LGD_ABI_VERSION stays 12): rows r and r + rows/2 are identical; the first rows/2 rows are processed by the kernel the
 * full call would run.  pair = LGD_PAIR_HALF only (y / stats of the second half are left untouched). */
int lgd_layernorm_pair_f16(const void* x, int64_t ldx, void* y, int64_t ldy, int rows, int C, float eps,
                           const float* gamma, const float* beta, float* stats, int rows_per_batch,
                           int64_t x_bs, int64_t y_bs, int pair, void* stream);
int lgd_layernorm_bwd_f16(const void* gy, int64_t ldgy, const void* x, int64_t ldx, void* gx,
                          int64_t ldgx, int rows, int C, const float* gamma, const float* stats,
                          int rows_per_batch, int64_t gy_bs, int64_t x_bs, int64_t gx_bs,
                          int accumulate, void* stream);
/* lgd_layernorm_plan (additive export: LGD_ABI_VERSION stays 12): the code of the kernel instantiation a LayerNorm call
 * runs — answered by the function the launches themselves choose their kernel with; host only, nothing is launched.
 *   op = LGD_LN_OP_FWD: lgd_layernorm_f16 / lgd_layernorm_pair_f16 with y; LGD_LN_OP_STATS: the same with y = NULL
 *        (statistics only); LGD_LN_OP_BWD: lgd_layernorm_bwd_f16.
 *   rows: the row count of the FULL call (the pair form launches the kernel chosen for it over the first rows / 2).
 *   ln_stream: the "ln_stream" option the answer holds under, 0 or 1; negative = the current option state.
 * Negative: LGD_ERR_ARG, as the launch would answer.
 * Preconditions of the three LayerNorm entry points (else LGD_ERR_ARG, before anything touches the device):
 *   C a multiple of 8, C <= 2560; rows >= 1; statistics only: stats not NULL and C <= 1536 unless "ln_stream" is on;
 *   pair form: pair LGD_PAIR_HALF, rows even and rows / 2 a multiple of rows_per_batch (where that is >= 1);
 *   x not NULL; with y: y, gamma and beta not NULL; backward: gy, gx, gamma and stats not NULL;
 *   every fp16 operand moves as 16-byte vectors: base pointer 16-byte aligned, leading dimension a multiple of 8, and the
 *   batch stride too once rows > rows_per_batch >= 1 makes it count.
 * The plan query checks those of them that its arguments show. */
#define LGD_LN_OP_FWD 0
#define LGD_LN_OP_STATS 1
#define LGD_LN_OP_BWD 2
/* (GroupNorm codes lie below 500, LayerNorm codes from 500 up; lgd_norm_variant names the instantiation behind each) */
#define LGD_LN_ROWS_1 514    /* a wave per row set, one 16-byte vector per lane: C <= 512 */
#define LGD_LN_ROWS_2 524    /* two vectors per lane: C <= 1024 */
#define LGD_LN_ROWS_3 532    /* three: C <= 1536 */
#define LGD_LN_WAVE 550      /* a wave per row, up to five vectors per lane: C <= 2560 */
#define LGD_LN_STATS_8 608   /* statistics only, streaming: 8 lanes share a row, C <= 320 */
#define LGD_LN_STATS_16 616  /* 16 lanes: C <= 640 */
#define LGD_LN_STATS_32 632  /* 32 lanes: C <= 1280 */
#define LGD_LN_STATS_64 664  /* 64 lanes: C <= 2560 */
#define LGD_LN_BWD 700       /* the backward: a wave per row */
int lgd_layernorm_plan(int op, int rows, int C, int ln_stream);
/* lgd_norm_variant (additive export: LGD_ABI_VERSION stays 12): row `index` (0, 1, ..) of the library's table of norm
 * kernel instantiations, GroupNorm rows then LayerNorm rows: its LGD_GN_* / LGD_LN_* code and the name of what it
 * launches (NUL-terminated, cut to name_cap - 1 characters; every output pointer may be NULL).  LGD_ERR_ARG past the
 * end.  Host only.  The Python binding fills ops.GN_VARIANTS / ops.LN_VARIANTS from it. */
int lgd_norm_variant(int index, int* code, char* name, int name_cap);

/* ---------------------------------------------------------------------------------------------
 * Scaled-dot-product attention, flash style (online softmax, K/V tiles staged in LDS, MFMA for
 * QK^T and PV).  Replaces F.scaled_dot_product_attention at attention_processor.py:355-357 and
 * the baddbmm/softmax/bmm path at :201-233,447 when no map is requested.
 *   q: [B][Sq][H*d] view with row stride ldq (so a fused QKV buffer can be passed), k/v likewise.
 *   o: [B][Sq][H*d] fp16.  lse (optional): fp32 [B][H][Sq] = log2-domain log-sum-exp, for backward.
 * ------------------------------------------------------------------------------------------- */
int lgd_attn_fwd_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                     int64_t k_bs, const void* v, int64_t ldv, int64_t v_bs, void* o, int64_t ldo,
                     int64_t o_bs, float* lse, int B, int H, int Sq, int Sk, int d, float scale,
                     void* stream);
/* CFG pair form (additive export: LGD_ABI_VERSION stays 12): images b and b + B/2 hold identical q / k / v (see LgdGemmDesc.pair), images b < B/2 are
 * computed with the kernel the full launch would run (bit-identical).  pair = LGD_PAIR_HALF: o / lse of images >= B/2
 * are left untouched; LGD_PAIR_DUP: every store is repeated for image b + B/2.  B even. */
int lgd_attn_fwd_pair_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                          int64_t k_bs, const void* v, int64_t ldv, int64_t v_bs, void* o, int64_t ldo,
                          int64_t o_bs, float* lse, int B, int H, int Sq, int Sk, int d, float scale,
                          int pair, void* stream);
/* backward: given q,k,v,o,do,lse -> dq,dk,dv (fp16, same views). delta: fp32 ws [B][H][Sq]. */
int lgd_attn_bwd_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                     int64_t k_bs, const void* v, int64_t ldv, int64_t v_bs, const void* o,
                     int64_t ldo, int64_t o_bs, const void* go, int64_t ldgo, int64_t go_bs,
                     const float* lse, float* delta, void* gq, int64_t ldgq, int64_t gq_bs, void* gk,
                     int64_t ldgk, int64_t gk_bs, void* gv, int64_t ldgv, int64_t gv_bs, int B, int H,
                     int Sq, int Sk, int d, float scale, void* stream);
/* The same with dK / dV computed for the first Sk_grad <= Sk keys only (ABI v10); dQ still sums over all Sk keys.
 * GLIGEN's gated self-attention (attention.py:43-53) attends over [visual tokens ; 30 grounding tokens] and keeps the
 * visual rows; the grounding rows of the concatenated input are constants of a run, so nothing reads the gradient of
 * their keys / values, and the key block that holds them would cost the dK/dV pass a whole extra round of workgroups
 * (4096 + 30 keys = 17 blocks of 256 per (image, head) on a grid that 16 fill exactly).  Rows >= Sk_grad of gk / gv are
 * not written. */
int lgd_attn_bwd_keys_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                          int64_t k_bs, const void* v, int64_t ldv, int64_t v_bs, const void* o,
                          int64_t ldo, int64_t o_bs, const void* go, int64_t ldgo, int64_t go_bs,
                          const float* lse, float* delta, void* gq, int64_t ldgq, int64_t gq_bs, void* gk,
                          int64_t ldgk, int64_t gk_bs, void* gv, int64_t ldgv, int64_t gv_bs, int B, int H,
                          int Sq, int Sk, int Sk_grad, int d, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-attention over the 77 text tokens with probability-map capture — the hook of
 * attention_processor.py:426-480 (slow path).  Whole K/V of a head lives in LDS.
 *   probs (optional): fp32 [Bp][H][Sq][Tp] where, following :466-476,
 *     tok < 0  : all Sk columns are stored (Tp = Sk)
 *     tok >= 0 : only column `tok` (Tp = 1)                      (return_token_ca_only=int)
 *     cond_only: only batch items b >= B/2 are stored (Bp = B/2) (return_cond_ca_only)
 * ------------------------------------------------------------------------------------------- */
int lgd_cross_attn_fwd_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                           int64_t k_bs, const void* v, int64_t ldv, int64_t v_bs, void* o,
                           int64_t ldo, int64_t o_bs, float* probs, int tok, int cond_only, int B,
                           int H, int Sq, int Sk, int d, float scale, void* stream);
/* backward w.r.t. q only (text K/V are constants of the run): recomputes P; takes the upstream
 * gradient on the output (go, may be NULL) and on the probability map (gp fp32 [B][H][Sq][Sk], may
 * be NULL) — the map is an output with its own gradient (guidance.py:244-286 via pipelines.py:56). */
int lgd_cross_attn_bwd_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk,
                           int64_t k_bs, const void* v, int64_t ldv, int64_t v_bs, const void* go,
                           int64_t ldgo, int64_t go_bs, const float* gp, void* gq, int64_t ldgq,
                           int64_t gq_bs, int B, int H, int Sq, int Sk, int d, float scale,
                           void* stream);

/* Causal self-attention (key j visible to query i iff j <= i), exact softmax: the CLIP text encoder's attention
 * ([ext] transformers 4.29.2 CLIPAttention with the causal mask of CLIPTextTransformer; called from
 * models/models.py:67-80 and pipelines.py:303-304 through `text_encoder(...)`).  Views as lgd_attn_fwd_f16. */
int lgd_attn_causal_fwd_f16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs,
                            const void* v, int64_t ldv, int64_t v_bs, void* o, int64_t ldo, int64_t o_bs, int B,
                            int H, int S, int d, float scale, void* stream);

/* Single-head attention forward for wide heads (additive export: LGD_ABI_VERSION stays 12; csrc/attn_wide.hip):
 * O = softmax(scale Q K^T) V for 8 <= d <= 512, one launch, no score matrix.  Replaces, for the mid-block Attention of
 * AutoencoderKL ([ext] diffusers models/attention_processor.py, AttnProcessor.__call__ with heads = 1: attn.to_q / to_k /
 * to_v, get_attention_scores = baddbmm(q, k^T) * scale -> softmax(dim = -1), torch.bmm(probs, v)), the op sequence
 * baddbmm -> softmax -> bmm; the projections and the GroupNorm stay with the caller.
 *   q [B][Sq][d], k / v [B][Sk][d], o [B][Sq][d] fp16 views: row stride ld*, per-image stride bs* (elements; 0 on an input
 *   repeats it for every image), so q and k may be the halves of one [B*S][2 d] projection.
 * Arithmetic: inputs exact, Q K^T in fp32, scale * log2(e) applied to the fp32 logit, running max and row sum in fp32
 * (the sum from the fp32 probabilities), v_exp_f32, P rounded to fp16 for P V, P V in fp32 (rescaled when the running max
 * moves), one fp16 rounding of O.  No logit or probability is stored anywhere; no atomics, no workspace, no host
 * synchronisation: bit-identical from run to run and under graph capture.
 * Its own contract, not a row of lgd_attn_variant.  Refused before any runtime call — LGD_ERR_ARG: a NULL operand; B, Sq or
 * Sk < 1; d < 8 or d % 8 != 0; ld / bs / base of an input not multiples of 8 / 16-byte aligned, of o not multiples of 4 /
 * 8-byte aligned; an ld below d, a negative bs, images of o overlapping each other; o overlapping q, k or v.
 * LGD_ERR_UNSUPPORTED: d > 512, B > 65535. */
int lgd_attn_wide_f16(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int d, int64_t ldq,
                      int64_t ldk, int64_t ldv, int64_t ldo, int64_t bsq, int64_t bsk, int64_t bsv, int64_t bso,
                      float scale, void* stream);

/* lgd_attn_plan (additive export: LGD_ABI_VERSION stays 12): the variant code of the kernel instantiation a call with these arguments runs under the
 * current option state ("attn32", "attn32_nw", "attn32_var", "attn_w4", "attn_w4_pipe") — answered by the function the
 * launches themselves choose their kernel with; host only, nothing is launched.  code = family * 100000 + DP * 100 + sub (DP: the padded
 * head dim of the instantiation); lgd_attn_variant below names every code (the Python binding: ops.ATTN_VARIANTS).
 *   op = LGD_ATTN_OP_FWD:       lgd_attn_fwd_f16 / lgd_attn_fwd_pair_f16 (pair != 0) / lgd_cross_attn_fwd_f16 (probs != 0:
 *                               a map is captured) / lgd_attn_causal_fwd_f16 (causal != 0).  `aligned` is ignored: every
 *                               view the entry points accept suits every forward kernel.
 *   op = LGD_ATTN_OP_BWD:       lgd_attn_bwd_f16 / lgd_attn_bwd_keys_f16 (Sk_grad <= Sk).
 *   op = LGD_ATTN_OP_CROSS_BWD: lgd_cross_attn_bwd_f16.  aligned: q / go as 16-byte and gq as 8-byte vectors (ld, per-image
 *                               stride, base pointer); 0 selects the one-wave-per-row kernel.
 * Sk_grad is only read by LGD_ATTN_OP_BWD.  Negative: LGD_ERR_ARG / LGD_ERR_UNSUPPORTED as the launch would answer.
 * Preconditions of every attention entry point (else LGD_ERR_ARG, before anything touches the device): d % 8 == 0; ld and
 * per-image stride of every fp16 input view multiples of 8 and its base 16-byte aligned; of every fp16 output view
 * multiples of 4 and 8-byte aligned (lgd_cross_attn_bwd_f16 also serves q / go / gq views that are not, element by
 * element). */
#define LGD_ATTN_OP_FWD 0
#define LGD_ATTN_OP_BWD 1
#define LGD_ATTN_OP_CROSS_BWD 2
int lgd_attn_plan(int op, int B, int H, int Sq, int Sk, int Sk_grad, int d, int probs, int causal, int pair,
                  int aligned);
/* lgd_attn_variant (additive export: LGD_ABI_VERSION stays 12): row `index` (0, 1, ..) of the library's table of
 * attention kernel variants — the table the launches themselves look a code up in, so it holds exactly the codes
 * lgd_attn_plan can answer.  *code: the variant code; *env_only: 1 when only the A/B switches of the environment
 * (LGD_ATTN_NW, LGD_ATTN_BWD) select it, which no option state reaches; name (host buffer of name_cap bytes): the
 * instantiation's name, NUL-terminated and cut to name_cap - 1 characters (the longest has fewer than 100).  Any of the
 * three may be NULL.  Host only.  Returns 0, or LGD_ERR_ARG for an index past the end. */
int lgd_attn_variant(int index, int* code, int* env_only, char* name, int name_cap);

/* ---------------------------------------------------------------------------------------------
 * Elementwise pieces.
 * ------------------------------------------------------------------------------------------- */
/* The preconditions an entry point of this section — and lgd_act_f16, lgd_sam_relpos_qkv_f16 and
 * lgd_sam_window_merge_f16 of the SAM section behind it — can see from its arguments — NULL-ness, alignment, counts,
 * divisibility, and the overlap of ranges whose extent the arguments give — are checked on the host, before any runtime
 * call; a call that misses one answers LGD_ERR_ARG and launches nothing.  The rest is the caller's duty and is NOT
 * checked: inputs are finite unless an entry point says otherwise; operands whose extent is not an argument (a
 * coefficient table, frozen_ref, hist, picks, the table of lgd_select_row_f32) are large enough for the row or step the
 * device index selects and share no byte with an output (x_out, x0_prev and hist against frozen_ref and hist; out against
 * the table).
 * "16-byte aligned": the operand moves as vectors of 8 halfs or 4 floats.  "No aliasing": the output range, whose extent
 * the arguments give, shares no byte with an input range.  "y may be x": the output is the input itself or a range apart
 * from it; a partial overlap is refused. */
/* GEGLU backward (attention.py:333-335): h = proj(x) packed [16 value|16 gate] blocks, width 2*n: value j of a row sits
 * at h[(j / 16) * 32 + j % 16], its gate 16 elements behind;  gy [rows][n] -> gh [rows][2n] in the same packed layout:
 *   gh_value[j] = gy[j] * gelu(gate[j]);  gh_gate[j] = gy[j] * value[j] * gelu'(gate[j])      (gelu: the erf form)
 * rows >= 1; n >= 16 and n % 16 == 0; h, gy, gh non-NULL and 16-byte aligned; no aliasing (gh against h and gy). */
int lgd_geglu_bwd_f16(const void* h, const void* gy, void* gh, int64_t rows, int n, void* stream);
/* GEGLU forward on a stored packed pre-activation h [rows][2n] -> y [rows][n] (grad-enabled pass):
 *   y[j] = value[j] * gelu(gate[j]).
 * rows >= 1; n >= 16 and n % 16 == 0; h, y non-NULL and 16-byte aligned; no aliasing. */
int lgd_geglu_fwd_f16(const void* h, void* y, int64_t rows, int n, void* stream);
/* y = x * sigmoid(1.702 x) (fp16): CLIP text encoder MLP activation ([ext] transformers CLIPMLP, "quick_gelu").
 * n >= 1 and n % 8 == 0; x, y non-NULL and 16-byte aligned; y may be x. */
int lgd_quick_gelu_f16(const void* x, void* y, int64_t n, void* stream);
/* NCHW fp32 (B, C <= 8, HW) -> channels-last fp16 [B*HW][8]: channels 0..C-1 = fp16(x), channels C..2C-1 (when 2C <= 8)
 * = fp16(x - fp16(x)), the rest zero.  Input of the UNet's conv_in (unet_2d_condition.py:860, 4 -> 320 channels) when
 * it runs as an implicit GEMM with K = 9*8 and the filter duplicated over the remainder channels.
 * B, HW >= 1; 1 <= C <= 8; x, y non-NULL, x 4-byte and y 16-byte aligned; no aliasing. */
int lgd_nchw_to_nhwc8_f16(const float* x, void* y, int B, int C, int HW, void* stream);
/* y = a + b (fp16, one rounding of the sum; an overflowing sum is +-inf), n elements (gradient fan-in / residual).
 * n >= 1 and n % 8 == 0; a, b, y non-NULL and 16-byte aligned; y may be a, b or both (a and b may overlap freely). */
int lgd_add_f16(const void* a, const void* b, void* y, int64_t n, void* stream);
/* y = alpha * x (fp16).  n >= 1 and n % 8 == 0; x, y non-NULL and 16-byte aligned; y may be x. */
int lgd_scale_f16(const void* x, void* y, float alpha, int64_t n, void* stream);
/* uint8 HWC images -> the 8-channel fp16 operand of the VAE encoder's conv_in (additive export: LGD_ABI_VERSION stays
 * 12) — models/pipelines.py:99-105 of the reference (`encode`: astype(float32) / 255, transpose to NCHW, 2 x - 1)
 * followed by lgd_nchw_to_nhwc8_f16's layout, in one pass over the bytes:
 *   x = table[u];  y[pixel] = {fp16(x_r), fp16(x_g), fp16(x_b), fp16(x_r - fp16(x_r)), ..g, ..b, 0, 0}
 * img: uint8 [B][HW][3]; table: device fp32 [256], written by the host as 2 * (u / 255) - 1 in fp32 with true division
 * (what numpy computes at :101-104, exactly); y: fp16 [B*HW][8].  Bit-exact.
 * B, HW >= 1 and B*HW % 4 == 0 (four pixels are three whole words); img, table, y non-NULL, img and table 4-byte and y
 * 16-byte aligned; no aliasing (y against the 3*B*HW bytes of img and the 1024 bytes of table). */
int lgd_image_u8_to_nhwc8_f16(const void* img, const float* table, void* y, int B, int HW, void* stream);
/* Sample of the VAE posterior, scaled (additive export, ABI v12) — models/pipelines.py:110-112 of the reference:
 * vae.encode(image).latent_dist.sample(generator) ([ext] diffusers DiagonalGaussianDistribution: chunk the moments,
 * clamp logvar to [-30, 20], std = exp(0.5 logvar), mean + std * noise) times vae.config.scaling_factor:
 *   out = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise)
 * moments: fp16 [B*HW][2z] as the encoder's last convolution writes them (z means, then z log-variances per pixel);
 * noise, out: NCHW fp32 (B, z, HW).  The log-variance may be any finite fp16 value (the clamp is part of the definition).
 * B >= 1; z, HW >= 4 with z % 4 == 0 and HW % 4 == 0; moments, noise, out non-NULL, moments 8-byte and noise / out 16-byte
 * aligned; no aliasing (out against moments and against noise). */
int lgd_vae_sample_f32(const void* moments, const float* noise, float* out, int B, int z, int HW, float scale,
                       void* stream);
/* y = softmax(scale * x) over the last dim, rows x n fp16 (VAE decoder mid-block attention, [ext]
 * AutoencoderKL; pipelines.py:117-127 decode).  Elements may be -inf (masked: probability 0) as long as one element of
 * every row is finite; +inf and NaN are not inputs.
 * rows >= 1; n >= 8 and n % 8 == 0; x, y non-NULL and 16-byte aligned; y may be x. */
int lgd_softmax_rows_f16(const void* x, void* y, int64_t rows, int n, float scale, void* stream);
/* Range probe of an fp16 matrix (additive export: LGD_ABI_VERSION stays 12) — what vae.calibrate_ranges measures of
 * every tensor the VAE blocks store, to choose the power-of-two scales of an overflow-prone (SDXL) VAE:
 *   out2[0] = max(out2[0], bits of the fp32 value of the largest |x| among the FINITE elements)
 *   out2[1] += number of non-finite elements (+-Inf, NaN), saturating at 2^32 - 1
 * Non-negative floats order like their bit patterns, so out2[0] read as a float is the running maximum.  The caller
 * zeroes the 8 bytes to start a measurement; several calls accumulate into one pair.  Both combiners are
 * order-independent: the result is exact and the same for every grid.  x: fp16 [rows][ld], of which only the columns
 * < cols of each row are read (the padding up to ld may hold anything, NaN included).  One launch (capturable): 16-byte
 * loads when cols % 8 == 0, ld % 8 == 0 and x is 16-byte aligned, element loads otherwise; one atomic max and, where
 * there is something to count, one atomic add per workgroup.  This entry point takes non-finite inputs: counting them
 * is its purpose.
 * rows, cols >= 1; ld >= cols; x, out2 non-NULL, x 2-byte and out2 4-byte aligned; out2 outside the range of x
 * (LGD_ERR_ARG otherwise); more than 2^40 elements: LGD_ERR_UNSUPPORTED. */
int lgd_range_f16(const void* x, int64_t rows, int64_t cols, int64_t ld, uint32_t* out2, void* stream);
/* sum over the 2x2 children of a nearest-2x upsampling: gy [B][2H*2W][C] -> gx [B][H*W][C],
 *   gx[b][y][x][c] = sum_{dy,dx < 2} gy[b][2y+dy][2x+dx][c]      (fp32 sum, one fp16 rounding).
 * B, H, W >= 1; C >= 8 and C % 8 == 0; gy, gx non-NULL and 16-byte aligned; no aliasing. */
int lgd_upsample2x_bwd_f16(const void* gy, void* gx, int B, int H, int W, int C, void* stream);

/* Classifier-free guidance + DDIM (eta=0) step + frozen-mask blend + latent history in one pass
 * (pipelines.py:436-453; [ext] DDIMScheduler.step).  eps: NCHW fp32 (2B,C,L,L) = [uncond; cond].
 *   e = eu + gs*(ec-eu); epsilon or v prediction; x0 = (x - sqrt(1-a_t) e)/sqrt(a_t);
 *   x' = sqrt(a_p) x0 + sqrt(1-a_p) e;
 *   if step < frozen_steps: x' = frozen_ref[step+1]*mask + x'*(1-mask)   (mask [B][HW] fp32)
 *   hist[step+1] = x'  (save_all_latents) when hist != NULL.   x_out may alias x.
 * coef_table: device fp32 [T][4] = {a_t, a_prev, guidance_scale, v_prediction flag}.
 * dyn: device int32[2] = {step, frozen_steps} — read on the device so that one captured hipGraph
 * replays for every step and for both stages.
 * Preconditions: eps, x, x_out, coef_table, dyn non-NULL; B, C, HW >= 1; frozen_ref and mask both given or both NULL
 * (one without the other is refused, not skipped); hist optional; every pointer 4-byte aligned.  x_out may be x; x_out
 * overlaps neither eps nor mask.  Not checked (the step count is not an argument): frozen_ref and hist hold step + 2
 * latents and share no byte with x_out or with each other. */
int lgd_cfg_ddim_step_f32(const float* eps, const float* x, float* x_out, const float* coef_table,
                          const int32_t* dyn, const float* frozen_ref, const float* mask, float* hist,
                          int B, int C, int HW, void* stream);
/* The same fused step for LINEAR MULTISTEP samplers — [ext] diffusers DPMSolverMultistepScheduler (dpmsolver++,
 * order 2, midpoint; models/models.py:46-47 `use_dpm_multistep_scheduler`), whose update is linear in the latents, the
 * current data prediction x0 and the previous one:
 *   m = eu + gs*(ec-eu);  x0 = c0 x + c1 m;  x' = A x + B x0 + C x0_prev;  x0_prev <- x0;  blend / hist as above.
 * coef_table: device fp32 [T][8] = {c0, c1, A, B, C, guidance_scale, 0, 0} (host: scheduler.DPMSolverMultistepScheduler).
 * x0_prev: fp32 state buffer (B,C,L,L), read only when C != 0, always rewritten.
 * Preconditions: those of lgd_cfg_ddim_step_f32, and x0_prev non-NULL, 4-byte aligned and apart from eps, x, x_out and
 * mask. */
int lgd_cfg_multistep_step_f32(const float* eps, const float* x, float* x_out, float* x0_prev,
                               const float* coef_table, const int32_t* dyn, const float* frozen_ref,
                               const float* mask, float* hist, int B, int C, int HW, void* stream);
/* The same fused step for PLMS (ABI v12) — [ext] diffusers 0.18.0 PNDMScheduler with skip_prk_steps=True, the sampler of
 * StableDiffusionPipeline for SD 1.5 / SD 2.1-base (generation/stable_diffusion_generate.py:13) driving the plain CFG loop
 * of models/pipelines.py:257-273.  One launch per UNet evaluation k (n steps make n+1 evaluations: the second one is
 * re-evaluated and averaged):
 *   m = eu + gs*(ec-eu);
 *   comb = w_m m + w_0 ets[0] + w_1 ets[1] + w_2 ets[2]          (PLMS weights 1; 1/2,1/2; 3/2,-1/2; 23/12,-16/12,5/12;
 *                                                                 55/24,-59/24,37/24,-9/24 over the newest outputs)
 *   if push >= 0: ets[push] = m                                   (ring of the last 3 pushed outputs; k = 1 does not push)
 *   src = from_cur ? cur_sample : x;  if save_cur: cur_sample = x  (k = 0 saves, k = 1 restarts from it)
 *   x' = a src + b comb;  hist[step+1] = x' when hist != NULL.  x_out may alias x.
 * a, b fold PNDMScheduler._get_prev_sample (and, for v_prediction, m <- sqrt(a_t) m + sqrt(1-a_t) src) into one affine map.
 * coef_table: device fp32 [E][16] = {w_m, w_0, w_1, w_2, a, b, guidance_scale, push slot (-1 = none), from_cur, save_cur,
 * 0...} (host: scheduler.PNDMScheduler.plms_table); dyn: device int32 {evaluation index, ...}.
 * ets: fp32 [3][B,C,L,L]; cur_sample: fp32 (B,C,L,L).  A ring slot is read only where its weight is not 0 and before the
 * push, cur_sample only with from_cur; nothing else of ets and cur_sample is written.
 * Preconditions: eps, x, x_out, ets, cur_sample, coef_table, dyn non-NULL, hist optional; B, C, HW >= 1 and
 * B*C*HW % 4 == 0; eps, x, x_out, ets, cur_sample, hist 16-byte aligned, coef_table and dyn 4-byte aligned.  x_out may be
 * x; no aliasing otherwise: x_out is apart from eps, ets and cur_sample, ets (three latents) from eps, x, x_out and
 * cur_sample, cur_sample from eps, x and x_out.  Not checked (the evaluation count is not an argument): coef_table holds
 * row dyn[0], hist holds dyn[0] + 2 latents and shares no byte with another operand. */
int lgd_cfg_plms_step_f32(const float* eps, const float* x, float* x_out, float* ets, float* cur_sample,
                          const float* coef_table, const int32_t* dyn, float* hist, int B, int C, int HW, void* stream);
/* The same fused step for the order-4 LINEAR MULTISTEP sampler in sigma space (additive export: LGD_ABI_VERSION stays
 * 12) — [ext] diffusers 0.18.0 LMSDiscreteScheduler, one of the k-diffusion samplers `generate.py --scheduler NAME` hands
 * to models.load_sd(scheduler_cls=...) (models/models.py:50-53).  For that family the loops of models/pipelines.py call
 * scheduler.scale_model_input before the UNet (:42, :196, :261, :422, :573: lgd_scale_rows_f32 here) and
 * latent_backward_guidance takes its `sigmas` branch, latents - grad * sigmas[index]**2 (:60-61: lgd_axpy_f32 here).  One
 * launch per step i = dyn[0], after the UNet:
 *   m = eu + gs*(ec-eu);  x0 = c0 x + c1 m          (epsilon: 1, -sigma;  v: 1/(sigma^2+1), -sigma/sqrt(sigma^2+1))
 *   d = (x - x0) * inv_sigma                         (the derivative of step i)
 *   x' = x + w[slot] d + sum_{s != slot} w[s] ring[s]
 *   ring[slot] = d;  blend / hist as lgd_cfg_ddim_step_f32.   x_out may alias x.
 * w holds the LMS coefficients (integrals of the Lagrange basis polynomials over [sigma_i, sigma_{i+1}]) permuted onto
 * ring slots by the host, the derivative of step j living in slot j % 4; a weight is 0 where the order min(i+1, 4) does
 * not reach.  coef_table: device fp32 [T][16] = {c0, c1, inv_sigma, w[0], w[1], w[2], w[3], guidance_scale, slot, 0...}
 * (host: scheduler.LMSDiscreteScheduler.lms_table); the slot is taken modulo 4.  ring: fp32 [4][B,C,L,L].  Slot `slot` is
 * never read and always written; another slot is read only where its weight is not 0; nothing else of ring is written.
 * Preconditions: those of lgd_cfg_ddim_step_f32, and ring non-NULL; B*C*HW % 4 == 0; eps, x, x_out, ring and hist
 * 16-byte aligned.  The ring (four latents) is apart from eps, x, x_out, mask, row 0 of coef_table, dyn and the first two
 * latents of frozen_ref and hist.  Not checked (the step count is not an argument): coef_table holds row dyn[0], frozen_ref
 * and hist hold dyn[0] + 2 latents and share no byte with x_out, the ring or each other. */
int lgd_cfg_lms_step_f32(const float* eps, const float* x, float* x_out, float* ring, const float* coef_table,
                         const int32_t* dyn, const float* frozen_ref, const float* mask, float* hist, int B, int C, int HW,
                         void* stream);
/* One MultiDiffusion step (additive export: LGD_ABI_VERSION stays 12) — generation/multidiffusion.py:226-289 of the
 * reference with its single 512x512 view, indep_uncond=True and normalization=False (count == 1), DDIM eta 0.  P region
 * prompts (row 0 the background), padded to Pp UNet rows; one launch after the UNet of step i = dyn[0]:
 *   d_k = DDIM(x_k, eu_k + gs*(ec_k - eu_k))    for k < P     (x_k = x_in row k: what the UNet consumed)
 *   latent = sum_k masks[k] * d_k                (prompt order);  hist[i+1] = latent when hist != NULL
 * and, when i+1 < n_steps, writes step i+1's UNet input, both CFG halves (x_in rows k and Pp+k, k < Pp):
 *   x_k = latent, and for 1 <= k < P while i+1 < n_boot:  b = (masks[k] >= 0.5),
 *   x_k = latent*b + (sqrt(a)*bg[picks[i+1][k-1]] + sqrt(1-a)*noise)*(1-b),  a = coef_table[i+1][0]
 *   (DDIMScheduler.add_noise at timestep t_{i+1}).
 * prep = 1 writes step dyn[0]'s input rows from `latent` only (once per run, before the first UNet call).
 * eps: fp32 [2Pp][C][HW] = [uncond rows; cond rows]; x_in: fp32 [2Pp][C][HW]; latent, noise: fp32 [C][HW];
 * masks: fp32 [>= P][HW] (broadcast over channels); bg: fp32 [n_boot][C][HW]; picks: device int32 [n_steps][P-1]
 * (rows >= n_boot unused; indices clamped to [0, n_boot)); coef_table: lgd_cfg_ddim_step_f32's fp32 [n_steps][4]
 * {alpha_bar_t, alpha_bar_prev, guidance_scale, v_pred}; dyn: device int32 {step, ...}.  A step outside [0, n_steps)
 * writes nothing; the last step writes latent and hist and leaves x_in as it is.
 * Preconditions: x_in, latent, masks, coef_table, dyn non-NULL; eps non-NULL unless prep = 1 (not read then); bg, noise
 * and picks non-NULL when n_boot > 0 and P > 1 (not read otherwise); hist optional; 1 <= P <= Pp; C, HW, n_steps >= 1;
 * HW % 4 == 0; n_boot >= 0; prep 0 or 1; eps, x_in, latent, masks, bg, noise, hist 16-byte aligned, picks, coef_table and
 * dyn 4-byte aligned.  No aliasing: the outputs x_in (2*Pp rows) and latent are apart from each other and from eps
 * (2*Pp rows), masks (P planes), and, when bootstrapping, bg (n_boot latents) and noise.  Not checked: the extents of
 * picks, coef_table and hist ([n_steps+1] latents), and hist against the other operands. */
int lgd_multidiffusion_step_f32(const float* eps, float* x_in, float* latent, const float* masks, const float* bg,
                                const float* noise, const int32_t* picks, const float* coef_table, const int32_t* dyn,
                                float* hist, int P, int Pp, int C, int HW, int n_steps, int n_boot, int prep,
                                void* stream);
/* MultiDiffusion over overlapping views (additive export: LGD_ABI_VERSION stays 12) — MultiDiffusion.generate of the
 * reference (generation/multidiffusion.py:210-280): a latent panorama [C][Hp][Wp] seen through V = nbh*nbw windows of
 * 64x64 at stride 8, view v starting at ((v / nbw)*8, (v % nbw)*8) with nbh = (Hp-64)/8+1, nbw = (Wp-64)/8+1
 * (get_views).  The UNet batch holds a chunk of whole views [v0, v0+nv) in a buffer with room for nvc views: view j of
 * the chunk owns rows j*Pp + k of the uncond half and (nvc + j)*Pp + k of the cond half, k < Pp (P prompts padded to Pp).
 * Two launches bracket the UNet call of every chunk of step i = dyn[0]:
 *   prep = 1: x_in rows of the chunk's views, both halves:  x_k = latent[view], and for 1 <= k < P while i < n_boot
 *     b = (masks[k][view] >= 0.5),  x_k = x_k*b + (sqrt(a)*bg[picks[i][v][k-1]] + sqrt(1-a)*noise[view])*(1-b),
 *     a = coef_table[i][0]  (DDIMScheduler.add_noise at t_i).  eps, value, count and hist are not read.
 *   prep = 0: for every panorama element, over the chunk's views that cover it in ascending view order
 *     value += sum_k masks[k] * DDIM(x_k, cfg_k)   (the sum over k first, in prompt order),
 *     count += sum_k masks[k]                       (normalization only),
 *     cfg_k = eu_k + gs*(ec_k - eu_k) with indep_uncond, else gs*(ec_k - eu_k) + eu_0 (the view's prompt-0 uncond row).
 *     The chunk with v0 == 0 starts from zero instead of reading value / count (no memset launch); the chunk with
 *     v0 + nv == V finishes: latent = normalization ? (count > 0 ? value / count : value) : value, hist[i+1] = latent
 *     when hist != NULL (it does not store value / count).  Without normalization overlapping views sum, as in the
 *     reference; elements no view covers come out 0.  One thread owns four consecutive elements and gathers: no atomics,
 *     and the result does not depend on how the V views are split into chunks.
 * eps, x_in: fp32 [2*nvc*Pp][C][64*64]; latent, value, count, noise: fp32 [C][Hp][Wp]; masks: fp32 [>= P][Hp][Wp];
 * bg: fp32 [n_boot][C][64*64]; picks: device int32 [n_steps][V][P-1] (indices clamped to [0, n_boot)); hist: fp32
 * [n_steps+1][C][Hp][Wp] or NULL; coef_table, dyn: as lgd_multidiffusion_step_f32.  A step outside [0, n_steps) writes
 * nothing; x_in rows of views outside [v0, v0+nv) are not written.
 * Preconditions: x_in, latent, masks, coef_table, dyn non-NULL; eps non-NULL unless prep = 1; value non-NULL, and count
 * with normalization, unless prep = 1 or one chunk holds all views (v0 == 0 and nv == V); bg, noise and picks non-NULL
 * when prep = 1, n_boot > 0 and P > 1; hist optional; 1 <= P <= Pp; 1 <= C <= 64; 64 <= Hp, Wp <= 4096; Wp % 4 == 0;
 * V == nbh*nbw; v0 >= 0, nv >= 1, v0 + nv <= V, nv <= nvc, nvc*Pp <= 2^20; n_steps >= 1; n_boot >= 0; prep 0 or 1; eps, x_in,
 * latent, value, count, masks, bg, noise, hist 16-byte aligned, picks, coef_table and dyn 4-byte aligned.  No aliasing:
 * with prep = 1 the output x_in (2*nvc*Pp rows) is apart from latent, masks (P planes) and, when bootstrapping, bg (n_boot
 * rows) and noise; with prep = 0 the outputs latent, value and count are apart from each other and from eps, x_in and
 * masks.  Not checked: the extents of picks, coef_table and hist, and hist against the other operands. */
int lgd_multidiffusion_views_f32(const float* eps, float* x_in, float* latent, float* value, float* count,
                                 const float* masks, const float* bg, const float* noise, const int32_t* picks,
                                 const float* coef_table, const int32_t* dyn, float* hist, int P, int Pp, int C, int Hp,
                                 int Wp, int V, int v0, int nv, int nvc, int n_steps, int n_boot, int indep_uncond,
                                 int normalization, int prep, void* stream);
/* Model-input scaling of sigma-space samplers — [ext] diffusers EulerDiscreteScheduler.scale_model_input, which the
 * SDXL-refiner pass applies before every UNet call (generation/sdxl_refinement.py:29 -> StableDiffusionXLImg2ImgPipeline):
 *   out[r][i] = x[i] * table[dyn[0] * row_stride + col]   for r < reps   (reps = 2: the CFG pair reads one latent).
 * The factor is read on the device, so the call sits inside a captured hipGraph that replays for every step.
 * x, out, table, dyn non-NULL and 4-byte aligned; n, reps >= 1; 0 <= col < row_stride; no aliasing (out [reps][n]
 * against x). */
int lgd_scale_rows_f32(const float* x, float* out, const float* table, const int32_t* dyn, int row_stride, int col,
                       int64_t n, int reps, void* stream);
/* guidance latent update (pipelines.py:60-69): x -= active[i/per_sample] * coef_table[*step_idx][col] * g.
 * active (device fp32 per image, or NULL = all on) emulates the per-image `while` exit of
 * pipelines.py:30 when several layouts are guided in one batch.
 * g, x, coef_table, step_idx non-NULL; active optional; every pointer 4-byte aligned; n >= 1; col in 0..3 (the table
 * has four columns); per_sample >= 0, 0 standing for n (one image); with active, n % per_sample == 0.  x is updated in
 * place and overlaps no byte of g. */
int lgd_axpy_f32(const float* g, float* x, const float* coef_table, const int32_t* step_idx, int col,
                 const float* active, int64_t per_sample, int64_t n, void* stream);
/* copy row `*idx` (device int32) of a [T][n] fp32 table into out[n] — per-step time-embedding
 * bias of every resnet without changing any kernel argument (graph-replay friendly).  Bit-exact.
 * table, idx, out non-NULL and 4-byte aligned; n >= 1.  Not checked (the table's extent is not an argument): out lies
 * outside the table. */
int lgd_select_row_f32(const float* table, const int32_t* idx, float* out, int n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SAM mask refinement (models/sam.py:25-55 -> [ext] transformers SamModel): pieces of the ViT image encoder and the
 * mask decoder that are not GEMM / LayerNorm / attention calls above.
 * ------------------------------------------------------------------------------------------- */
#define LGD_ACT_GELU 1 /* exact (erf) GELU: SamMLPBlock of the image encoder, mask-decoder upscaling */
#define LGD_ACT_RELU 2 /* SamMLPBlock / SamFeedForward of the mask decoder */
/* y = act(x), fp16.  n >= 1 and n % 8 == 0; x, y non-NULL and 16-byte aligned; mode one of the two above; y may be x;
 * inputs finite; all else LGD_ERR_ARG before any launch. */
int lgd_act_f16(const void* x, void* y, int64_t n, int mode, void* stream);
/* Window partition + decomposed relative-position bias of SamVisionAttention, folded into the attention operands.
 * qkv [B*Hs*Ws][3*NH*d] fp16 (fused projection, raster token order), qkv_bias fp32 [3*NH*d] (value of the zero-padded
 * window positions), rel_h / rel_w fp32 [2*S-1][d] with S = window (window > 0: ceil(Hs/S) x ceil(Ws/S) windows,
 * padded) or S = Hs = Ws (window == 0: global attention).  Writes qa / ka / va [B*nwin*S*S][NH*DA] fp16,
 *   qa = [q | q.Rh[qy-j+S-1]/scale, j<S | q.Rw[qx-j+S-1]/scale, j<S | 0],  ka = [k | onehot(ky) | onehot(kx) | 0],
 *   va = [v | 0],   DA >= d + 2*S, DA % 8 == 0,
 * so that lgd_attn_fwd_f16(qa, ka, va, d = DA, scale) computes softmax(scale*q.k + rel_h + rel_w) v in columns 0..d-1
 * of every head.  Rows of padded window positions are written too: q, k, v = fp16(qkv_bias), the rel columns from the
 * fp32 bias.  The rel columns are fp32 dot products of d terms times 1/scale, rounded once to fp16; the rest is copied.
 * Preconditions: all seven pointers non-NULL; qkv, qa, ka, va 2-byte and qkv_bias, rel_h, rel_w 4-byte aligned (scalar
 * accesses); B, Hs, Ws, NH >= 1; d >= 8 and d % 8 == 0; DA % 8 == 0 and DA >= d + 2*S; window >= 0, window == 0 only
 * with Hs == Ws; scale > 0 (NaN is refused).  No aliasing: qa, ka and va are apart from each other and from qkv, qkv_bias,
 * rel_h and rel_w.  LGD_ERR_UNSUPPORTED: more than 2^31 - 1 window rows, or NH*(d + 2*S) floats past 64 KB of LDS. */
int lgd_sam_relpos_qkv_f16(const void* qkv, const float* qkv_bias, const float* rel_h, const float* rel_w, int B,
                           int Hs, int Ws, int window, int NH, int d, int DA, float scale, void* qa, void* ka,
                           void* va, void* stream);
/* Inverse gather (SamVisionLayer.window_unpartition): oa [B*nwin*S*S][NH*DA] in window order -> out [B*Hs*Ws][NH*d]
 * in raster order, padding positions and the DA-d extra columns dropped (they are not read).  Bit-exact.
 * oa, out non-NULL and 16-byte aligned; B, Hs, Ws, NH >= 1; d >= 8 and d % 8 == 0; DA % 8 == 0 and DA >= d; window >= 0,
 * window == 0 only with Hs == Ws; no aliasing.  LGD_ERR_UNSUPPORTED: more than 2^31 - 1 tokens. */
int lgd_sam_window_merge_f16(const void* oa, void* out, int B, int Hs, int Ws, int window, int NH, int d, int DA,
                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-attention energy of LMD / LMD+ and its gradient on the probability maps, one launch for
 * all (key, object, token, head) items: utils/guidance.py:91-148 (box loss, both branches: max-based fg/bg
 * top-k :131-145 and the ratio-based default :118-130 that generation/backward_guidance.py runs),
 * :150-242 (reference-attention L1 transfer), :244-286 (compute_ca_lossv3), times loss_scale
 * (pipelines.py:48).
 *   items: int32 [n_items][8] = {map_id, kind(0 topk, 1 ref, 2 ratio), token, mask_id, k_fg, k_bg, ref_id, image},
 *          sorted so that the items of one (map, image, token) column are adjacent;
 *   groups: int32 [n_groups][2] = {first item, item count} of each column — one workgroup per (group, head)
 *          sums the column's map gradients in a fixed order and stores them once (no atomics)
 *   coefs: fp32  [n_items][4] = {fg_coef, bg_coef, ref_coef, ratio_coef} (all normalisations folded in;
 *          kind 2: term = ratio_coef * (1 - sum(A*M)/sum(A))^2 per head, ABI v7)
 *   maps:  device array of n_maps pointers to fp32 [n_samples][H][HW][T]; gmaps likewise (pre-zeroed)
 *          or NULL; loss: fp32 [n_samples] (one value per image of the batch)
 *   map_hw: int32[n_maps]; masks: fp32 [n_masks][max_hw] (1 inside the box); refs: fp32
 *   [T][n_refs][H][max_hw] reference maps R_b (guidance.py:201); the slice of step dyn[0] (device
 *   int32) is used: refs + dyn[0]*refs_step_stride
 *   partial: fp32 [n_items*H] workspace; loss: fp32[1] = sum of all terms.
 *   grad_scale multiplies the map gradients only (static loss scaling for the fp16 backward pass;
 *   undone by the out_scale of the final conv_in dgrad).
 *   max_hw <= 4096 (ABI v9; 1024 before): guidance keys at the 64x64 level of a 512^2 SD 1.x network are legal, as
 *   utils/guidance.py accepts any `guidance_attn_keys`; larger maps return LGD_ERR_ARG.
 * Masks may be any fp32 in [0, 1] (M weighs the inside, 1 - M the outside); map_hw[m] <= max_hw is the row stride of
 * masks and refs, and elements of a row past map_hw[m] are not read.
 * Top-k (kind 0) takes the k largest of A*M (and of A*(1-M)) by exact ranking; among equal values THE LOWEST INDEX WINS.
 * Stored: loss[0 .. n_samples) (0 for an image without items), partial[item*H + h], and, with gmaps, the map_hw
 * positions of every group's (map, image, head, token) column — element ((image*H + h)*HW + i)*T + token, the sum over
 * the column's items in table order.  No other element of a gmaps buffer is touched; with n_items = 0 none is.
 * Refused with LGD_ERR_ARG before any launch: NULL loss; with n_items > 0 a NULL maps, map_hw, items, coefs, masks,
 * partial or groups, or n_groups < 1; refs without dyn; n_items < 0, n_groups < 0, n_samples < 1, H < 1, T < 1,
 * max_hw < 1 or > 4096, refs_step_stride < 0; a pointer table (maps, gmaps) off 8 bytes or any other table off 4 bytes.
 * gmaps is optional; refs and dyn are optional together when no item is of kind 1.
 * ------------------------------------------------------------------------------------------- */
int lgd_ca_energy_f32(const float* const* maps, float* const* gmaps, const int32_t* map_hw,
                      const int32_t* items, const float* coefs, const float* masks, const float* refs,
                      int64_t refs_step_stride, const int32_t* dyn, const int32_t* groups, int n_groups,
                      int n_items, int n_samples, int H, int T, int max_hw, float grad_scale, float* partial,
                      float* loss, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BoxDiff energy (ABI v9) and its gradient on the probability maps, one launch, one workgroup per image:
 * utils/boxdiff.py:20-101 (_compute_max_attention_per_index: x100 token soft-max of the layer- and head-averaged map
 * without its first and last token, reflect-padded 3x3 smoothing, inner- / outer-box top-k means, corner terms),
 * :104-118 (_compute_loss), :121-196 (compute_ca_loss_boxdiff), times amp_loss_scale (:224).  Replaces that Python loop
 * over objects x phrase tokens and the autograd graph through it (torch.cat / mean over the maps included).
 *   maps / gmaps: device arrays of n_maps pointers to fp32 [n_samples][H][side*side][T] (all maps of ONE resolution:
 *          generation/boxdiff.py:33-39 lists five 16x16 keys); gmaps pre-zeroed or NULL (value only)
 *   items: int32 [n_items][8] = {token (index in the 77-token prompt), mask_id, k_fg, k_bg, 0, 0, 0, 0}, the items of an
 *          image adjacent; k = (mask.sum() * P).long() as :80,:85 compute it; k = 0 drops that term (Python's
 *          max(0, nan) = 0, :107-109)
 *   groups: int32 [n_samples][2] = {first item, item count} per image; max_items = the largest count (sizes the LDS)
 *   masks: fp32 [n_masks][3][side*side]: row 0 the union of the object's boxes; row 1 corner_mask_x[side] |
 *          corner_mask_y[side] (:64-67); row 2 gt_proj_x[side] | gt_proj_y[side] (:90-91)
 *   smooth: 9 fp32 weights of GaussianSmoothing(kernel_size 3, sigma) (utils/attn.py:92-110) or NULL (no smoothing)
 *   loss: fp32 [n_samples] = loss_scale * energy; the map gradients carry loss_scale * grad_scale.
 * Item tokens satisfy 1 <= token <= T-2 (the soft-max runs over those tokens only).  Box masks may be any fp32 in [0, 1].
 * Top-k takes the k largest of the smoothed image times M (times 1 - M) by exact ranking, and the corner terms the maximum
 * of every row and column of the smoothed image; among equal values THE LOWEST INDEX WINS in both.
 * Stored: loss[0 .. n_samples) (0 for an image without items) and, with gmaps, tokens 1 .. T-2 of every (map, image,
 * head, position) row (zero for an image without items); tokens 0 and T-1 and everything else of a gmaps buffer are
 * not touched.
 * Returns LGD_ERR_ARG for a NULL maps, items, masks, groups or loss, n_maps < 1, n_samples < 1, H < 1, max_items < 0, a
 * pointer table (maps, gmaps) off 8 bytes or another table off 4 bytes; LGD_ERR_UNSUPPORTED for side < 2 or > 32,
 * T < 3 or > 128, or more items per image than fit the LDS: (7 + 2 max_items) * side*side * 4 bytes <= 150 KB
 * (71 items at 16x16).  gmaps and smooth are optional.
 * ------------------------------------------------------------------------------------------- */
int lgd_boxdiff_energy_f32(const float* const* maps, float* const* gmaps, int n_maps, int side, const int32_t* items,
                           const float* masks, const float* smooth, const int32_t* groups, int n_samples,
                           int max_items, int H, int T, float loss_scale, float grad_scale, float* loss, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stage-2 evaluator (additive exports: LGD_ABI_VERSION stays 12) — scripts/owl_vit_eval.py -> utils/eval/eval.py:120-174
 * (`eval_prompt`): OWL-ViT open-vocabulary detection, `post_process`, score filter, NMS.  The towers and the linears of
 * the heads are the GEMM / LayerNorm / attention calls above; these two are the detection tail.
 * ------------------------------------------------------------------------------------------- */
/* Tail of the class head and of the box head — [ext] transformers modeling_owlvit.py, OwlViTClassPredictionHead.forward
 * (image_class_embeds / (norm + 1e-6), query_embeds / (norm + 1e-6), einsum "...pd,...qd->...pq", + logit_shift,
 * * (elu(logit_scale) + 1), torch.where(query_mask == 0, finfo.min, .)) and OwlViTForObjectDetection.box_predictor
 * (pred_boxes += box_bias; sigmoid):
 *   logits[b][p][q]  = (e.q / ((|e| + 1e-6) (|q| + 1e-6)) + shift) * (elu(scale_raw) + 1),  -FLT_MAX where query_mask == 0
 *   pred_boxes[b][p] = sigmoid(box_raw + box_bias[p])                                        (cx, cy, w, h)
 * class_embeds: fp16 [B*P][ld_embeds], the `dense0` output (D columns read); query_embeds: fp32 [B][Q][D]; query_mask:
 * int32 [B][Q] or NULL (none masked); shift / scale_raw: fp32, element t at [t * ld_ss] (the two 1-wide linears, e.g.
 * columns 0 and 1 of one fp32 GEMM output); box_raw: [B*P][4], fp32 when box_is_f32 else fp16 (the last box-MLP layer);
 * box_bias: fp32 [P][4] (compute_box_bias, host table).  logits: fp32 [B][P][Q]; pred_boxes: fp32 [B][P][4].  Norms and
 * dot products are fp32, one wave per token.  D <= 1024 and Q <= 64, else LGD_ERR_UNSUPPORTED. */
int lgd_owl_heads_f32(const void* class_embeds, int64_t ld_embeds, const float* query_embeds,
                      const int32_t* query_mask, const float* shift, const float* scale_raw, int64_t ld_ss,
                      const void* box_raw, int box_is_f32, const float* box_bias, float* logits, float* pred_boxes,
                      int B, int P, int Q, int D, void* stream);
/* `post_process` + score filter + greedy NMS in one launch, one workgroup per image — [ext] OwlViTImageProcessor
 * .post_process (max / argmax over the queries, sigmoid, center_to_corners_format), utils/eval/eval.py:144-148 (keep
 * score >= score_threshold), :11-81 (`nms`) and :83-105 (`class_aware_nms`), boxes normalised to [0, 1] as eval_prompt
 * passes them (input_in_pixels=False: areas without the +1).
 *   mode 0 (from the model): logits_or_scores = logits fp32 [B][P][Q], boxes = pred_boxes fp32 [B][P][4] cxcywh; per
 *          token score = sigmoid(max_q logit), label = the first argmax_q, box = (cx - w/2, cy - h/2, cx + w/2, cy + h/2);
 *          labels / counts are not read.
 *   mode 1 (candidates): logits_or_scores = scores fp32 [B][P] (>= 0), labels int32 [B][P] in [0, 2^20) or NULL (all 0),
 *          boxes fp32 [B][P][4] xyxy, counts int32 [B] = candidates of each image (NULL: P); Q is not read.
 * Candidates with score >= score_threshold are ordered by descending score, EQUAL scores by ascending token index (a
 * choice: numpy's argsort at eval.py:45 leaves it open), and walked greedily in fp32: a picked box drops every later box
 * whose inter / (area_i + area_j - inter) is not < nms_threshold.  class_aware != 0 runs that walk per label and emits
 * the labels in ascending order, each label's picks by descending score (the output order of class_aware_nms).
 * out_boxes fp32 [B][P][4] xyxy, out_scores fp32 [B][P], out_labels / out_index int32 [B][P] (out_index = the token a
 * pick came from) in picking order, out_count int32 [B]; rows past the count are left untouched.  Deterministic, no
 * atomics.  boxes / out_boxes 16-byte aligned, else LGD_ERR_ARG; P <= 4096 (large-patch14 has 3600 tokens), else
 * LGD_ERR_UNSUPPORTED. */
int lgd_detect_nms_f32(int mode, const float* logits_or_scores, const float* boxes, const int32_t* labels,
                       const int32_t* counts, int B, int P, int Q, float score_threshold, float nms_threshold,
                       int class_aware, float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_index,
                       int32_t* out_count, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Safety checker of the `sd` baseline (additive exports: LGD_ABI_VERSION stays 12; csrc/safety.hip) —
 * generation/stable_diffusion_generate.py:14,44-49 builds StableDiffusionPipeline with its default checker, which blanks
 * the images it flags.  The CLIP vision tower and `visual_projection` are the GEMM / LayerNorm / attention calls above;
 * these two are what follows them.
 * ------------------------------------------------------------------------------------------- */
/* Tail of [ext, unpinned] diffusers 0.18.0 pipelines/stable_diffusion/safety_checker.py, StableDiffusionSafetyChecker
 * .forward, restated here (diffusers itself was not available to this project; this text is the contract).  Per image,
 * all in fp32 and in exactly this order:
 *   n(x)  = x / max(|x|_2, 1e-12)                          (torch.nn.functional.normalize)
 *   cos_j = n(e) . n(c_j)                                  for the n_special special-care rows, then the n_concepts rows
 *   adj   = 0
 *   special rows, ascending j:  s_j = (cos_j - w_j) + adj;  the row HITS iff fl32(s_j * 1000) > 0.5;  a hit sets
 *                               adj = 0.01 for every LATER special row and for all concept rows (a sequential prefix:
 *                               the hitting row itself and the rows before it keep adj = 0)
 *   concept rows:               s_j = (cos_j - w_j) + adj,  the same hit test;  has_nsfw iff any concept row hits
 * The hit test is the reference's `round(score, 3) > 0` of a numpy.float32 score (checked equal over 400 005 values,
 * 200 000 of them within 2e-6 of the boundary 0.0005, under NumPy 2.2).  Under NumPy 1.x the reference's `cos - w + adj`
 * is promoted to fp64: the two can differ only for a score within ~1e-6 of 0.0005.
 * embeds: fp32 [B][ld_embeds], the `visual_projection` output (D columns read); special: fp32 [n_special][D] and
 * special_w: fp32 [n_special] (`special_care_embeds`, `special_care_embeds_weights`; both may be NULL when n_special is
 * 0); concepts: fp32 [n_concepts][D] and concept_w: fp32 [n_concepts] (`concept_embeds`, `concept_embeds_weights`) — the
 * raw checkpoint tensors, normalised inside the kernel.  scores: fp32 [B][n_special + n_concepts], the unrounded s_j,
 * special rows first; flags: int32 [B][2] = {has_nsfw, a special-care row hit}.  One wave per image, 16-byte loads along
 * D, wave64 sums; no atomics, every output element is written once.
 * LGD_ERR_ARG, before any runtime call: a NULL operand; B, D or n_concepts <= 0, n_special < 0; D % 4 or ld_embeds % 4
 * != 0, ld_embeds < D; embeds, special or concepts not 16-byte aligned, any other operand not 4-byte aligned; scores or
 * flags overlapping an input or each other.  LGD_ERR_UNSUPPORTED: D > 1024, n_special > 32, n_concepts > 64, B > 65535. */
int lgd_safety_head_f32(const float* embeds, int64_t ld_embeds, const float* special, const float* special_w,
                        int n_special, const float* concepts, const float* concept_w, int n_concepts, float* scores,
                        int32_t* flags, int B, int D, void* stream);
/* Zeroes the flagged images of a batch in place (what the checker does to `images[idx]`).  Image n is the image_bytes
 * bytes at images + n * image_bytes and is zeroed iff flags[n * flag_stride] != 0 (int32; flag_stride in elements, e.g. 2
 * for column 0 of lgd_safety_head_f32's flags).  A workgroup reads its image's flag first and returns when it is 0: an
 * unflagged image is neither read nor written.  16-byte stores with byte stores for an unaligned head and tail: images
 * and image_bytes need no alignment.  Nothing outside [images, images + N * image_bytes) is written.
 * LGD_ERR_ARG, before any runtime call: images or flags NULL, image_bytes, flag_stride or N <= 0, flags not 4-byte
 * aligned, flags inside the images.  LGD_ERR_UNSUPPORTED: N * image_bytes beyond int64, or more than 2^31 - 1
 * workgroups (N * min(64, ceil(image_bytes / 16384))). */
int lgd_blank_flagged_u8(uint8_t* images, int64_t image_bytes, const int32_t* flags, int64_t flag_stride, int N,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Mask refinement around the SAM network for a batch of (image, prompt) items (additive exports: LGD_ABI_VERSION stays
 * 12) — models/sam.py as generation/lmd_plus.py:122-130 and generation/lmd.py:124-149 call it, everything that follows
 * the model's logits and, for LMD, everything that precedes its point prompt, without a host read.
 * ------------------------------------------------------------------------------------------- */
/* Low-resolution mask logits -> the selected mask on the latent grid: models/sam.py:45-55 (`post_process_masks` of the
 * [ext] SamImageProcessor: bilinear to target x target, crop to the resized size, bilinear to the original size, > 0; then
 * F.interpolate(.float(), (H, W), mode="bilinear").bool()), :63-65 (get_iou_with_resize), :67-111 (select_mask, rule
 * "largest_over_conf") and the per-box part of :182-213 (sam_refine_boxes).
 *   logits: fp32 [N][K][S][S] (pred_masks of the model, S = 256 for sam-vit-base); iou: fp32 [N][K], the model's predicted
 *   IoUs — item n is scored with ITS row (the reference's sam() hands out row 0 of image 0; its plugins call with one
 *   image and one prompt); geom: int32 [N][4] = {h, w, nh, nw}, original and resized (unpadded) image size per item —
 *   items of different sizes may share a launch, a row outside 1 <= nh, nw <= target is clamped into it; target: the
 *   model's input side; coarse: uint8 [N][hc][wc], non-zero = inside.
 *   Every resampling is torch's upsample_bilinear2d with align_corners=False in fp32: src = (in / out) (dst + 0.5) - 0.5,
 *   clamped at 0; i1 = i0 + (i0 < in - 1); value = l0h (l0w a + l1w b) + l1h (l0w c + l1w d), evaluated without
 *   contraction.  Step 3 (0 / 1 image at h x w -> H x W) keeps `!= 0`; when (hc, wc) != (H, W) the candidates are
 *   resampled once more to hc x wc and kept where > 0 before they meet the coarse mask.  Counts are integers;
 *   IoU_k = inter_k / (union_k + 1e-6) in fp64; score_k = area_k - max(area) [iou[n][k] < (float)below_conf]
 *   - max(area) [IoU_k < below_iou]; the first maximum wins.
 *   cand: uint8 [N][K][H][W] (0 / 1) or NULL; mask: uint8 [N][H][W], the winning candidate; conf: fp32 [N] =
 *   iou[n][pick]; stats: int32 [N][1 + 3K] = {pick, area_k.., inter_k.., union_k..} (area on H x W, the other two on
 *   hc x wc); workspace: 12 N K H bytes, plus N K H W when cand is NULL, 4-byte aligned.
 * Two launches, no atomics, deterministic: one wave per (row block, candidate, item), then one workgroup per item.
 * LGD_ERR_ARG: a NULL operand other than cand, K > 4, a size <= 0, fp32 / int32 operands not 4-byte aligned.
 * LGD_ERR_UNSUPPORTED: H, W, hc or wc > 4096, S or target > 32768, N > 65535. */
int lgd_sam_mask_tail_f32(const float* logits, const float* iou, const int32_t* geom, const uint8_t* coarse, int N,
                          int K, int S, int target, int H, int W, int hc, int wc, double below_conf,
                          double below_iou, uint8_t* cand, uint8_t* mask, float* conf, int32_t* stats, void* workspace,
                          void* stream);
/* LMD's prompt from the object token's attention map: models/sam.py:125-147 with use_box_input=False (scipy.ndimage
 * .gaussian_filter, the arg-max as the point prompt) and :113-122 (preprocess_mask without erosion: min-max normalise,
 * > mask_th).  The smoothing is scipy's with its defaults: separable, axis 0 then axis 1, radius int(4 sigma + 0.5),
 * weights exp(-x^2 / 2 sigma^2) normalised to sum 1, mode `reflect` (d c b a | a b c d | d c b a) at any distance.
 *   attn: fp32 [N][hm][wm]; coarse: uint8 [N][hm][wm] (0 / 1); points: fp32 [N][2] = {peak_x * up_h, peak_y * up_w} of
 *   the first maximum in raster order — up_w = height / wm and up_h = width / hm, the reference's swapped naming
 *   (:135,:146) kept; smooth: fp32 [N][hm][wm], the filtered map, or NULL.  One workgroup per item, fp32 in LDS.
 * LGD_ERR_ARG: NULL attn / coarse / points, a size or scale <= 0, sigma <= 0.  LGD_ERR_UNSUPPORTED: hm * wm > 4096 (a
 * 64 x 64 map), radius > 64, N > 65535.  The box branch (use_box_input=True) is lgd_sam_attn_box_prompt_f32 below. */
int lgd_sam_attn_prompt_f32(const float* attn, int N, int hm, int wm, float sigma, float mask_th, int up_w, int up_h,
                            uint8_t* coarse, float* points, float* smooth, void* stream);
/* LMD's BOX prompt from the object token's attention map: models/sam.py:125-147 with use_box_input=True and :113-122
 * (preprocess_mask WITH its opening), then utils/utils.py:72-88 (binary_mask_to_box).  One workgroup per item; the map
 * and two byte masks live in LDS; no atomics; every output element is written once.
 *   Smoothing and threshold: exactly those of lgd_sam_attn_prompt_f32 (one device function serves both kernels): scipy's
 *   gaussian_filter defaults — mode `reflect`, radius int(4 sigma + 0.5), fp32 — and the mask
 *   (a - min) / max(a - min) > mask_th.
 *   Opening: n_open erosions, then n_open dilations (scipy.ndimage.binary_erosion / binary_dilation, iterations =
 *   n_open).  The structuring element is scipy's default generate_binary_structure(2, 1): a pixel and its 4 neighbours.
 *   border_value = 0 for both: a set pixel on the border, which has an outside neighbour, erodes, and the outside never
 *   dilates inward.  iterations = n equals n single steps, here with one barrier per step.  n_open = 0 skips it.
 *   coarse: uint8 [N][hm][wm], 0 / 1: the OPENED mask.
 *   boxes: fp32 [N][4] = {xmin * up_w, ymin * up_h, xmax * up_w, ymax * up_h} with ymin = max(min_y - 1, 0), ymax =
 *   min(max_y + 1, hm), xmin = max(min_x - 1, 0), xmax = min(max_x + 1, wm) over the set pixels — binary_mask_to_box(
 *   enlarge_box_by_one=True, w_scale=up_w, h_scale=up_h) as sam_refine_attn calls it, with up_w = height / wm and up_h =
 *   width / hm: the reference's swapped (w, h) naming (:135,:141) kept, as the point kernel keeps it.  The values are
 *   small integers, exact in fp32.  Minimum and maximum come from wave reductions and one pass over LDS.
 *   empty: int32 [N], 1 where the opened mask has no pixel (the reference fails there: min() of an empty sequence).  A
 *   constant map counts: max(a - min) = 0, and the reference's NaN > mask_th is False everywhere.  boxes is {0, 0, 0, 0}
 *   there.
 *   smooth: fp32 [N][hm][wm], the filtered map, or NULL.
 * LGD_ERR_ARG: NULL attn / coarse / boxes / empty, a size or scale <= 0, sigma <= 0, n_open < 0, an fp32 / int32 operand
 * not 4-byte aligned.  LGD_ERR_UNSUPPORTED: hm * wm > 4096, radius > 64, N > 65535, n_open > 64.  Both are refused on
 * the host before any launch: nothing is written. */
int lgd_sam_attn_box_prompt_f32(const float* attn, int N, int hm, int wm, float sigma, float mask_th, int n_open,
                                int up_w, int up_h, uint8_t* coarse, float* boxes, int32_t* empty, float* smooth,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * The hand-off between the two stages of LMD / LMD+ for all layouts of a batch (additive exports: LGD_ABI_VERSION stays
 * 12; csrc/handoff.hip) — centre-of-mass alignment, painter's-order composition and the reference-map gather as three
 * launches without a host read.  Boxes are numbered through the batch; `seg`: int32 [NL + 1], layout l owns boxes
 * seg[l] .. seg[l + 1] - 1.  L (the latent side) must be a multiple of 8, as shift_tensor asserts: else LGD_ERR_ARG.
 * ------------------------------------------------------------------------------------------- */
/* Place: utils/latents.py:85-106 (align_with_bboxes), utils/utils.py:102-123 (binary_mask_to_center), :145-180
 * (shift_tensor's offset rule), :72-100 (binary_mask_to_box / _box_mask) and the ordering of utils/latents.py:52-57
 * (compose_latents: np.argsort of the negated mask areas).  One workgroup per layout.
 *   masks: uint8 [NB][L][L], non-zero = inside; targets: fp64 [NB][4], the xyxy box (fractions of the frame) each
 *   generation will occupy in the overall one.
 *   plan: int32 [NB][8] = {ox, oy, area, x0, y0, x1, y1, empty}.  Sum m, sum x m and sum y m are exact integers; the centre
 *   is float(sum x m) / float(sum m), ONE fp32 division (the reference divides torch / numpy fp32 scalars); then in fp64
 *   c = centre / L, off = (t[0] + t[2]) / 2 - c (y likewise, or 0 with horizontal_only) and ox = rint(off * 8) * (L / 8),
 *   rint half to even as Python's round.  align == 0: the offsets are 0.  The shifted mask is M(y, x) = m(y - oy, x - ox),
 *   0 where the source lies outside the frame; `area` counts M; the box is M's bounding box grown by one and clipped as
 *   binary_mask_to_box does (near side to 0, far side to L; covered pixels are x0 <= x <= x1).  A box whose M is empty
 *   has empty = 1, area 0, an empty box, and takes no part below (the reference raises ValueError('The mask is empty')
 *   there; a launch cannot raise without a read).
 *   win: int32 [NL][2][L][L].  Painter's order = descending area, EQUAL areas lower index first (a choice: np.argsort
 *   leaves it open).  win[l][0] = the last box in that order whose M covers the pixel, win[l][1] = the last whose grown
 *   box covers it, as indices inside the layout, -1 where none does.
 *   max_boxes: the largest box count of a layout (host; what seg holds).  NB == 0 (no layout has a box): the per-box
 *   tables may be NULL, here and in the composition, and both owner maps are -1 throughout.
 * LGD_ERR_ARG: NULL operand, NL <= 0, L % 8 != 0, misaligned tables.  LGD_ERR_UNSUPPORTED: max_boxes > 64, L > 1024,
 * NL > 65535. */
int lgd_handoff_place(const uint8_t* masks, const double* targets, const int32_t* seg, int NL, int NB, int max_boxes,
                      int L, int align, int horizontal_only, int32_t* plan, int32_t* win, void* stream);
/* Compose: utils/latents.py:38-83 (compose_latents with compose_box_to_bg) on the histories shifted as
 * utils/latents.py:96-100 shifts them (shift_tensor, utils/utils.py:145-180), as ONE gather per output element.
 *   hist: int64 [NB][2] = {device address of the box's history, fp32 [rows >= steps + 1][C][L][L] with the steps
 *   `stride` elements apart; that stride} — the histories are views of the denoising batches; bg: fp32 [NL][C][L][L].
 *   composed: fp32 [NL][steps + 1][C][L][L]; fg_idx: int64 [NL][L][L].  With w = win[l][0] at the pixel: w >= 0 -> every
 *   step t takes box w's history of step t at (y - oy_w, x - ox_w), fg_idx = w + 1.  Else fg_idx = 0, steps >= 1 are 0 and
 *   step 0 takes box win[l][1]'s step-0 latent at its shifted source — 0 where that lies outside the frame — or bg where
 *   no grown box covers the pixel.
 *   aligned: fp32 [NB][rows][C][L][L] or NULL — the shifted histories themselves, zero filled (what align_with_bboxes
 *   returns); `rows` is read only with it.
 * One thread per output element; every element is written.  LGD_ERR_ARG / LGD_ERR_UNSUPPORTED as above. */
int lgd_handoff_compose_f32(const int32_t* plan, const int32_t* win, const int32_t* seg, const int64_t* hist,
                            const float* bg, int NL, int NB, int steps, int C, int L, int rows, float* composed,
                            int64_t* fg_idx, float* aligned, void* stream);
/* Reference maps: utils/attn.py:40-70 (shift_saved_attns) and the gather of utils/guidance.py:201.
 *   maps: int64 [NB][NK][3] = {device address of the saved map, fp32 [rows][1][heads][side * side][1]; rows; side};
 *   lay_of: int32 [NB], the layout of each box.  out: fp32, per layout [T][n_boxes][NK][heads][max_hw], the layouts back
 *   to back (layout l starts at seg[l] * T * NK * heads * max_hw).  Element (t, b, k, h, p) = the map at the source of
 *   p = y * side + x under the offset (ox / (L / 8)) * (side / 8) — the same eighth of the frame as the latents; 0
 *   outside the frame, for t >= rows and for p >= side * side.  Every element is written.  side % 8 == 0 is the
 *   caller's to check (shift_tensor asserts it). */
int lgd_handoff_ref_maps_f32(const int32_t* plan, const int32_t* seg, const int32_t* lay_of, const int64_t* maps, int NB,
                             int T, int NK, int heads, int max_hw, int L, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pillow's Image.resize for 8-bit RGB images (additive exports: LGD_ABI_VERSION stays 12; csrc/resample.hip) — what
 * generation/sdxl_refinement.py:26 (`image.resize((1024, 1024), Image.LANCZOS)`) and the [ext] OwlViTImageProcessor in
 * front of utils/eval/eval.py:127 compute on the host: [ext] Pillow src/libImaging/Resample.c (ImagingResample for
 * 8-bit images), bit for bit.
 *
 * The contract, for one axis with `in` input and `out` output samples and a filter (f, support0):
 *   bilinear: f(x) = 1 - |x| on |x| < 1, support0 = 1;
 *   bicubic:  a = -0.5; f(x) = ((a + 2)|x| - (a + 3)) x^2 + 1 on |x| < 1, (((|x| - 5)|x| + 8)|x| - 4) a on |x| < 2,
 *             support0 = 2;
 *   lanczos:  f(x) = sinc(x) sinc(x / 3) on -3 <= x < 3, sinc(x) = sin(pi x) / (pi x), sinc(0) = 1, support0 = 3;
 *   0 elsewhere.  In fp64: scale = in / out, filterscale = max(scale, 1), support = support0 * filterscale,
 *   ss = 1 / filterscale, row width = 2 * (int)ceil(support) + 1.  For every output index xx:
 *     center = (xx + 0.5) * scale;  xmin = max((int)(center - support + 0.5), 0);
 *     count = min((int)(center + support + 0.5), in) - xmin;
 *     w[x] = f((x + xmin - center + 0.5) * ss) for x < count, each divided by their sum (summed in ascending x) when that
 *     sum is not 0;  k[x] = (int)(w[x] * 2^22 - 0.5) when w[x] < 0, else (int)(w[x] * 2^22 + 0.5); k[x] = 0 for x >= count.
 *   A pass computes, per channel in int32,  clip8(((1 << 21) + sum_x k[x] * pix[xmin + x]) >> 22),  clip8 clamping to
 *   0 .. 255 after the arithmetic shift.  The horizontal pass runs first and writes uint8; the vertical pass runs on that
 *   uint8 image.  A pass whose in == out is left out, not run with identity weights.
 * ------------------------------------------------------------------------------------------- */
#define LGD_FILTER_LANCZOS 1  /* Pillow's own codes (Image.Resampling) */
#define LGD_FILTER_BILINEAR 2
#define LGD_FILTER_BICUBIC 3
/* The tables of one axis.  HOST ONLY: no runtime call, every pointer is a host pointer, so it answers on a host without a
 * GPU.  *width (may be NULL when the tables are asked for) = the row width; coef: int32 [out][width], bounds: int32
 * [out][2] = {xmin, count}.  coef and bounds both NULL: only *width is written — the query a caller sizes its tables
 * with.  LGD_ERR_ARG: in or out <= 0, an unknown filter, one table without the other, nothing to write, a pointer not
 * 4-byte aligned, tables that overlap each other.  LGD_ERR_UNSUPPORTED: in or out > 16384.  The Python binding reads its
 * tables from here (ops.resample_tables) and keeps the device copy per (in, out, filter). */
int lgd_resample_plan(int in, int out, int filter, int32_t* coef /* host */, int32_t* bounds /* host */,
                      int* width /* host */);
/* Output forms, folded into the last pass (no separate cast, normalise or transpose launch); v = the Pillow byte. */
#define LGD_RESAMPLE_U8 0     /* uint8 [N][H][W][3]: Image.resize itself */
#define LGD_RESAMPLE_AFFINE 1 /* [N][3][H][W]: (v * r - m_c) / s_c in fp32, in this order, without contraction — the
                                 rescale and normalise steps of an [ext] transformers image processor */
#define LGD_RESAMPLE_UNIT 2   /* [N][3][H][W]: v / 255 * 2 - 1 in fp32, in this order (models/pipelines.py:99-105) */
/* src: uint8 [N][h][w][3] -> out [N] x (H, W) in `form`; out_f16 = 0: fp32, 1: fp16 (the fp32 value rounded once; not
 * read for LGD_RESAMPLE_U8 beyond its range check).  r, m0..m2, s0..s2: the fp32 parameters of LGD_RESAMPLE_AFFINE, by
 * value (not read by the other forms).
 * (coef_x, bounds_x, width_x, rows_x): device copies of the tables lgd_resample_plan(w, W, filter) made, their row
 * width and row count; (.._y): of lgd_resample_plan(h, H, filter).  The tables of an axis whose size does not change
 * are not read and may be NULL.  scratch: uint8, N * h * W * 3 bytes, read and written when both axes change size, else
 * not touched and may be NULL.
 * Two launches (horizontal into scratch, vertical from it), one when a single axis changes, one (the form applied to the
 * bytes) when none does.  One thread per output pixel; no atomics, every output element is written once.
 * LGD_ERR_ARG, before any runtime call: src or out NULL; N, h, w, H or W <= 0; an unknown filter or form; out_f16 not 0 or 1;
 * for an axis that changes size: a NULL or not 4-byte aligned table, width_* that is not the plan's row width for these
 * sizes, rows_* that is not the output size; scratch NULL when both axes change; out not aligned to its element (1, 2 or
 * 4 bytes — src and scratch need none: they move byte by byte); out overlapping src, scratch or a table; scratch
 * overlapping src.  LGD_ERR_UNSUPPORTED: N > 65535 or a size > 16384.
 * The caller's duty, not checked: the tables hold what the plan function wrote for exactly these sizes and filter (a
 * window that leaves the input is clamped into it: wrong pixels, no fault), and share no byte with scratch. */
int lgd_resample_u8(const uint8_t* src, int N, int h, int w, int H, int W, int filter, const int32_t* coef_x,
                    const int32_t* bounds_x, int width_x, int rows_x, const int32_t* coef_y, const int32_t* bounds_y,
                    int width_y, int rows_y, uint8_t* scratch, int form, int out_f16, float r, float m0, float m1,
                    float m2, float s0, float s1, float s2, void* out, void* stream);
/* The same resize written into a larger canvas (additive export: LGD_ABI_VERSION stays 12) — the resize, rescale,
 * normalise and pad steps of the [ext] transformers SamImageProcessor in front of models/sam.py:39 in one call.  Every
 * argument up to `out` means what it means for lgd_resample_u8, except that out is
 *   fp32 / fp16 [N][3][CH][CW] for LGD_RESAMPLE_AFFINE and LGD_RESAMPLE_UNIT,  uint8 [N][CH][CW][3] for LGD_RESAMPLE_U8,
 * with the resized H x W image at the top-left corner (element (y, x) of the image is element (y, x) of the canvas; no
 * offset, no cropping) and every element with y >= H or x >= W set to `pad`, in output units (after the form: a
 * processor that pads with zeros after normalising passes 0).  fp16: pad rounded once; uint8: pad itself.
 * The same passes as lgd_resample_u8; the LAST one to run has one thread per CANVAS pixel and stores either its pixel or
 * the pad — no memset, no copy, no pad launch, and with both axes unchanged the call is one launch.  The pass into
 * scratch is the dense one.  Every canvas element is written exactly once and nothing outside the canvas is written;
 * pad pixels read neither src nor the tables.  No atomics.  CH == H and CW == W gives lgd_resample_u8's bits.
 * LGD_ERR_ARG, before any runtime call: everything lgd_resample_u8 refuses (out's extent for the overlap checks is the
 * canvas); CH < H or CW < W; pad not finite; for LGD_RESAMPLE_U8 a pad that is not an integer in 0 .. 255.
 * LGD_ERR_UNSUPPORTED: what lgd_resample_u8 answers so, or CH or CW > 16384. */
int lgd_resample_canvas_u8(const uint8_t* src, int N, int h, int w, int H, int W, int filter, const int32_t* coef_x,
                           const int32_t* bounds_x, int width_x, int rows_x, const int32_t* coef_y,
                           const int32_t* bounds_y, int width_y, int rows_y, uint8_t* scratch, int form, int out_f16,
                           float r, float m0, float m1, float m2, float s0, float s1, float s2, void* out, int CH, int CW,
                           float pad, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LGD_HIP_H */
