// The attention launch contract, host side: variant codes, the variant table's row type, the view predicate and the
// problem check every entry point uses.  Internal to attn.hip / attn_bwd.hip / attn_w4.hip; the codes themselves are public
// through lgd_attn_plan and lgd_attn_variant (include/lgd_hip.h).
//
//   code = family * 100000 + DP * 100 + sub        DP: padded head dim of the instantiation (DK for the 32x32x16 kernel)
//
// Every launch path first CHOOSES a code (plan_* functions: arguments + option state -> code), looks its row up and calls
// the row's launcher, so the query and the launch cannot disagree; a code without a row is LGD_ERR_UNSUPPORTED.
//
// The variant table is the library's: families 1-4 in attn.hip, 5-7 in attn_bwd.hip.  A row is written as ONE set of
// arguments, e.g. (DP, mode, shape), from which both its code and the template arguments of its launcher follow, and it
// says whether only LGD_ATTN_NW / LGD_ATTN_BWD select it (env_only: the conformance suite is not required to reach it).
// lgd_attn_variant enumerates the rows; the Python side (ops.ATTN_VARIANTS, ops.ATTN_VARIANTS_ENV_ONLY) is filled from
// it.  A new kernel is a new row; a threshold change that makes an env-only code reachable by default clears the row's
// flag; tests/test_attn_conformance_cpu.py sweeps the plan against the table.
#pragma once
#include <stdint.h>
#include <initializer_list>
#include "common.h"

enum {
  ATTN_FAM_SELF = 1,        // attn_self_kernel<DP, ONES, QT, NDT, NW>: sub = 10 * mode + shape
  ATTN_FAM_SELF32 = 2,      // attn_self32_kernel<DK, ..>: sub = ATTN32_*
  ATTN_FAM_W4 = 3,          // attn_w4_kernel (d = 40): sub = 1 one wave per SIMD (pipelined), 0 two waves per SIMD
  ATTN_FAM_TWOPASS = 4,     // attn_fwd_kernel<DP>: exact two-pass softmax (map capture, causal)
  ATTN_FAM_BWD = 5,         // attn_bwd_dq_kernel + attn_bwd_dkv_kernel: sub = 10 * (three 16-row tiles for d <= 48) + shape
  ATTN_FAM_XBWD_MFMA = 6,   // cross_attn_bwd_mfma_kernel<DP>
  ATTN_FAM_XBWD_ROWS = 7,   // cross_attn_bwd_kernel (one wave per query row), DP = 0
};
enum { SELF_PLAIN = 0, SELF_ONES = 1, SELF_ONES3 = 2 };            // mode: d == DP / d < DP (row of ones) / d < 48 at DP = 64
enum { SELF_QT1 = 0, SELF_QT2 = 1, SELF_QT2_NW8 = 2 };             // shape: query tiles per wave, waves per workgroup
enum { ATTN32_NW4 = 0, ATTN32_NW8 = 1, ATTN32_NW8_PF4 = 2, ATTN32_NW8_FREE = 3 };
enum { BWD_T1 = 0, BWD_T2 = 1, BWD_T2_DB = 2, BWD_T2_DB_NW8 = 3 };  // tiles per wave, double buffering, 8 waves

constexpr int attn_code(int fam, int dp, int sub) { return fam * 100000 + dp * 100 + sub; }
constexpr int attn_code_fam(int code) { return code / 100000; }
constexpr int attn_code_dp(int code) { return (code / 100) % 1000; }
constexpr int attn_code_sub(int code) { return code % 100; }

// One row of a variant table.  Args: the kernel argument struct of the family (AttnArgs, AttnBwdArgs, CrossBwdArgs).
struct AttnVariantInfo {
  int code;
  int env_only;             // only the A/B switches of the environment select it
  const char* name;         // the profiler's and the gate messages' name of the instantiation
};
template <class Args>
struct AttnVariant {
  AttnVariantInfo info;
  int (*launch)(const Args&, hipStream_t);
};

template <class Args, int N>
int attn_launch_code(const AttnVariant<Args> (&rows)[N], int code, const Args& a, hipStream_t st) {
  for (const AttnVariant<Args>& r : rows)
    if (r.info.code == code) return r.launch(a, st);
  return LGD_ERR_UNSUPPORTED;
}

// A strided fp16 operand: base pointer, leading dimension and per-image stride (elements).  Every kernel but the
// one-wave-per-row cross backward reads its input rows as 16-byte vectors and writes its output rows as 8-byte vectors.
struct AttnView {
  const void* p;
  int64_t ld, bs;
  bool reads16() const { return ld % 8 == 0 && bs % 8 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
  bool writes8() const { return ld % 4 == 0 && bs % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
};

inline int check_problem(int B, int H, int Sq, int Sk, int d) {
  return (B < 1 || H < 1 || Sq < 1 || Sk < 1 || d < 8) ? LGD_ERR_ARG : LGD_OK;
}
// rows of d halfs move as whole vectors: d % 8, every view in `reads` as 16-byte and every view in `writes` as 8-byte vectors
inline bool attn_vectors_ok(int d, std::initializer_list<AttnView> reads, std::initializer_list<AttnView> writes) {
  bool ok = d % 8 == 0;
  for (const AttnView& v : reads) ok = ok && v.reads16();
  for (const AttnView& v : writes) ok = ok && v.writes8();
  return ok;
}

int lgd_attn_bwd_plan(int B, int H, int Sq, int Sk, int d);          // attn_bwd.hip
int lgd_cross_attn_bwd_plan(int Sk, int d, int aligned);              // attn_bwd.hip
const AttnVariantInfo* lgd_attn_bwd_variant_info(int index);          // attn_bwd.hip: rows of families 5-7, nullptr past the end
