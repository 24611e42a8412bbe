// Single-head attention forward for WIDE heads (8 <= d <= 512): O = softmax(scale Q K^T) V, fp16 operands, everything in
// between in fp32 and in registers.  Replaces the mid-block Attention of AutoencoderKL ([ext] diffusers
// models/attention_processor.py, AttnProcessor: to_q / to_k / to_v -> baddbmm -> softmax -> bmm at heads = 1, width 512),
// which the VAE otherwise runs as GEMM -> row softmax -> GEMM over a materialised fp16 score matrix (vae.py, _Blocks._attn).
//
// Its own entry point with its own contract (lgd_attn_wide_f16), NOT a row of the attention variant table: the flash
// kernels of attn.hip stop at d = 192 because they hold a whole K / V^T tile of 64 keys and two query tiles per wave.
//
// Shape of the kernel (attn_fwd_kernel's transposed products, one pass, online softmax):
//   * 4 waves per workgroup, each wave owns 16 query rows; DP = d padded to 64 / 128 / 256 / 512 (zero fill: a zero
//     column adds nothing to a logit; padded V columns are multiplied but never stored).  The column loops have no
//     condition on d: a branch per MFMA would put every LDS read, its wait and its MFMA into a block of their own;
//   * S^T = K Q^T (A := K rows, B := Q rows), MFMA 16x16x32: a lane holds query (lane & 15) and keys 4 g + r of each
//     16-key block (g = lane >> 4); the Q fragments (DP / 32 x 8 halfs) stay in registers for the whole kernel;
//   * O^T = V^T P^T (A := V^T, B := P^T): the S^T accumulators become the P^T operand in registers; the O^T accumulator
//     is DP / 16 x 4 fp32 per lane (128 registers at DP = 512: one wave per SIMD, unified 512-entry register file);
//   * key tiles of 32 keys, K and V both ROW-major in LDS ([key][DP + 16] halfs), two stages (132 KB at DP = 512): tile
//     t + 1 travels global -> registers while tile t is multiplied, registers -> the other stage behind it, one barrier per
//     tile.  V^T fragments come from the transposing LDS read (ds_read_b64_tr_b16, as attn_w4.hip): per 16-lane group a
//     4-key x 16-column block, lane n receives column n — keys 4 g .. 4 g + 3 and 16 + 4 g .. in the order P^T has them.
//     EXEC is all ones at every such read (no lane-dependent branch in the loop).
// Rounding points (the conformance bound of tests/attn_wide_cases.py is derived from exactly these): inputs exact; Q K^T
// accumulates in fp32; scale log2(e) multiplies the fp32 logit; running max (exact, per tile) and row sum in fp32, the sum
// taken from the fp32 p; v_exp_f32; P rounded to fp16 for P V; P V accumulates in fp32 and is multiplied by exp2(m_old -
// m_new) whenever a tile raises a row's max; one fp16 rounding of O.  No logit or probability reaches memory at all.
// No atomics, no workspace, one launch: results do not depend on scheduling.
#include "common.h"
#include "attn_plan.h"
#include "contract.h"

namespace {

typedef short short4_t __attribute__((ext_vector_type(4)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) short4_t* lds_s4_ptr;

constexpr int KT = 32;            // keys per tile: one k-step of the P V product
constexpr int QROWS = 64;         // query rows per workgroup: 4 waves x 16
constexpr float NEG_BIG = -1.0e30f;

struct WideArgs {
  const half_t* q; const half_t* k; const half_t* v; half_t* o;
  long ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;
  int Sq, Sk, d;
  float scale_log2;               // scale * log2(e)
};

template <int DP>
__global__ __launch_bounds__(256, 1) void attn_wide_kernel(const WideArgs a) {
  constexpr int LD = DP + 16;             // halfs per LDS row: ds_read_b128 fragment reads conflict-free (attn.hip, K_LD)
  constexpr int NDC = DP / 32;            // 32-wide chunks of the head dim (Q K^T contraction)
  constexpr int NDT = DP / 16;            // 16-row tiles of dv (O^T rows)
  constexpr int SEG = DP / 8;             // 16-byte segments per row
  constexpr int IT = KT * SEG / 256;      // segments per thread and operand
  constexpr int TILE = KT * LD;           // halfs per operand and stage
  static_assert(KT * SEG % 256 == 0, "a tile is a whole number of 16-byte segments per thread");

  __shared__ __attribute__((aligned(16))) half_t smem[4 * TILE];      // stage s: K at 2 s TILE, V at (2 s + 1) TILE

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int b = blockIdx.z;
  const int q0 = blockIdx.x * QROWS + wid * 16;
  const int d = a.d;
  const half_t* Qb = a.q + (long)b * a.bsq;
  const half_t* Kb = a.k + (long)b * a.bsk;
  const half_t* Vb = a.v + (long)b * a.bsv;

  // ---- Q fragments (B operand of S^T): lane -> query c16, head-dim elements 32 dc + 8 g ..+7
  half8_t qf[NDC];
  {
    const int qrow = q0 + c16;
#pragma unroll
    for (int dc = 0; dc < NDC; ++dc) {
      const int dd = dc * 32 + g * 8;
      if (qrow < a.Sq && dd < d) qf[dc] = *reinterpret_cast<const half8_t*>(Qb + (long)qrow * a.ldq + dd);
      else qf[dc] = (half8_t){0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  // ---- tile staging: rows past Sk and columns past d arrive as zeros (nothing outside the logical operands is read)
  // Every lane loads from an address inside the operands (row and segment clamped) and the value is dropped afterwards:
  // no branch around a load, so the loads of a tile go out back to back.
  uint4 k_reg[IT], v_reg[IT];
  const int last_seg = (d >> 3) - 1;
  auto load_tile = [&](int kv0) {
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / SEG, seg = idx % SEG;
      const bool ok = kv0 + row < a.Sk && seg <= last_seg;
      const long r = min(kv0 + row, a.Sk - 1);
      const int c = min(seg, last_seg) * 8;
      const uint4 kk = *reinterpret_cast<const uint4*>(Kb + r * a.ldk + c);
      const uint4 vv = *reinterpret_cast<const uint4*>(Vb + r * a.ldv + c);
      k_reg[i] = ok ? kk : make_uint4(0, 0, 0, 0);
      v_reg[i] = ok ? vv : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&](int stage) {
    half_t* Ks = smem + 2 * stage * TILE;
    half_t* Vs = Ks + TILE;
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / SEG, seg = idx % SEG;
      *reinterpret_cast<uint4*>(Ks + row * LD + seg * 8) = k_reg[i];
      *reinterpret_cast<uint4*>(Vs + row * LD + seg * 8) = v_reg[i];
    }
  };

  f32x4 oacc[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) oacc[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run = NEG_BIG, l_run = 0.f;      // l_run: this lane's keys only; the four lanes of a query are summed at the end

  const int n_tiles = (a.Sk + KT - 1) / KT;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const bool more = t + 1 < n_tiles;                                // workgroup-uniform
    if (more) load_tile((t + 1) * KT);
    const half_t* Ks = smem + 2 * (t & 1) * TILE;
    const half_t* Vs = Ks + TILE;

    // ---- S^T of the tile, log2 domain, padded keys masked
    // The two 16-key blocks are two independent accumulation chains, and the K fragments are requested one group of
    // KG chunks ahead of the MFMAs that read them (written out: left to itself the compiler waits for every fragment
    // right behind its request).
    f32x4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    {
      constexpr int KG = 2;                   // 4 at DP = 512 spills (the register budget is the O^T accumulator's)
      const half_t* klane = Ks + c16 * LD + g * 8;
      half8_t kf[2][KG][2];
#pragma unroll
      for (int j = 0; j < KG; ++j)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) kf[0][j][kt] = *reinterpret_cast<const half8_t*>(klane + kt * 16 * LD + j * 32);
#pragma unroll
      for (int dg = 0; dg < NDC / KG; ++dg) {
        if (dg + 1 < NDC / KG) {
#pragma unroll
          for (int j = 0; j < KG; ++j)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
              kf[(dg + 1) & 1][j][kt] = *reinterpret_cast<const half8_t*>(klane + kt * 16 * LD + ((dg + 1) * KG + j) * 32);
        }
        __builtin_amdgcn_sched_barrier(0);          // the requests of group dg + 1 stay in front of the MFMAs of group dg
#pragma unroll
        for (int j = 0; j < KG; ++j)
#pragma unroll
          for (int kt = 0; kt < 2; ++kt)
            s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[dg & 1][j][kt], qf[dg * KG + j], s[kt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] = t * KT + kt * 16 + g * 4 + r < a.Sk ? s[kt][r] * a.scale_log2 : NEG_BIG;

    // ---- online softmax: the max is exact per tile; the accumulators are rescaled only when some row's max moved
    float mx = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])), fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    if (__builtin_amdgcn_ballot_w64(m_new > m_run) != 0) {            // wave-uniform
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      l_run *= alpha;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) oacc[dt] *= alpha;
      m_run = m_new;
    }
    half8_t pf;                   // P^T fragment: element e <-> key (e < 4 ? 4 g + e : 16 + 4 g + e - 4) of the tile
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[kt][r] - m_run);
        l_run += p;
        pf[4 * kt + r] = (half_t)p;
      }

    // ---- O^T += V^T P^T: two transposing reads per 16 columns (keys 4 g ..+3 and 16 + 4 g ..+3 of the row-major tile)
    const half_t* vlane = Vs + (g * 4 + (c16 >> 2)) * LD + 4 * (c16 & 3);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(uintptr_t)(unsigned)(uintptr_t)(vlane + dt * 16));
      const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)(uintptr_t)(unsigned)(uintptr_t)(vlane + 16 * LD + dt * 16));
      const short8_t both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, both), pf, oacc[dt], 0, 0, 0);
    }

    // stage (t + 1) & 1 was last read in iteration t - 1, which every wave left through the barrier below
    if (more) store_tile((t + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: lane owns query q0 + c16, dv = 16 dt + 4 g + r
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  const int qrow = q0 + c16;
  if (qrow < a.Sq) {
    const float inv = 1.f / l_run;
    half_t* orow = a.o + (long)b * a.bso + (long)qrow * a.ldo;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) {
      const int dv = dt * 16 + g * 4;
      if (dv < d) {                 // d % 8 == 0: four columns are inside together or not at all
        const half4_t o4 = {(half_t)(oacc[dt][0] * inv), (half_t)(oacc[dt][1] * inv), (half_t)(oacc[dt][2] * inv), (half_t)(oacc[dt][3] * inv)};
        *reinterpret_cast<half4_t*>(orow + dv) = o4;
      }
    }
  }
}

template <int DP>
int launch_wide(const WideArgs& a, int B, hipStream_t st) {
  (void)hipGetLastError();  // drop stale errors of unrelated earlier runtime calls
  hipLaunchKernelGGL((attn_wide_kernel<DP>), dim3((a.Sq + QROWS - 1) / QROWS, 1, B), dim3(256), 0, st, a);
  return lgd_check_launch();
}

// bytes from the first to behind the last element of a view of `rows` rows of d halfs in B images
int64_t extent_bytes(const AttnView& v, int B, int rows, int d) {
  return 2 * ((int64_t)(B - 1) * v.bs + (int64_t)(rows - 1) * v.ld + d);
}

}  // namespace

// Refused before any runtime call, in this order — LGD_ERR_ARG: a NULL operand; B, Sq or Sk < 1, d < 8; d % 8 != 0 or a
// view that does not move as whole vectors (AttnView: inputs 16-byte, o 8-byte); a leading dimension below d or a
// negative per-image stride; images of o that overlap each other; o overlapping q, k or v.  LGD_ERR_UNSUPPORTED: d > 512,
// B > 65535.
extern "C" int lgd_attn_wide_f16(const void* q, const void* k, const void* v, void* o, int B, int Sq, int Sk, int d,
                                 int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t bsq, int64_t bsk,
                                 int64_t bsv, int64_t bso, float scale, void* stream) {
  if (!q || !k || !v || !o) return LGD_ERR_ARG;
  if (int e = check_problem(B, 1, Sq, Sk, d)) return e;
  const AttnView Q{q, ldq, bsq}, K{k, ldk, bsk}, V{v, ldv, bsv}, O{o, ldo, bso};
  if (!attn_vectors_ok(d, {Q, K, V}, {O})) return LGD_ERR_ARG;
  if (ldq < d || ldk < d || ldv < d || ldo < d || bsq < 0 || bsk < 0 || bsv < 0 || bso < 0) return LGD_ERR_ARG;
  if (B > 1 && bso < (int64_t)(Sq - 1) * ldo + d) return LGD_ERR_ARG;
  const int64_t ob = extent_bytes(O, B, Sq, d);
  if (lgd_contract::overlaps(o, ob, q, extent_bytes(Q, B, Sq, d)) || lgd_contract::overlaps(o, ob, k, extent_bytes(K, B, Sk, d)) ||
      lgd_contract::overlaps(o, ob, v, extent_bytes(V, B, Sk, d)))
    return LGD_ERR_ARG;
  if (d > 512 || B > 65535) return LGD_ERR_UNSUPPORTED;
  WideArgs a;
  a.q = (const half_t*)q; a.k = (const half_t*)k; a.v = (const half_t*)v; a.o = (half_t*)o;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.bsq = bsq; a.bsk = bsk; a.bsv = bsv; a.bso = bso;
  a.Sq = Sq; a.Sk = Sk; a.d = d;
  a.scale_log2 = scale * 1.4426950408889634f;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (d <= 64) return launch_wide<64>(a, B, st);
  if (d <= 128) return launch_wide<128>(a, B, st);
  if (d <= 256) return launch_wide<256>(a, B, st);
  return launch_wide<512>(a, B, st);
}
