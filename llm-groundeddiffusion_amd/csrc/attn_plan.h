// Variant codes of the attention dispatch: which kernel instantiation a call runs.  Internal to attn.hip / attn_bwd.hip /
// attn_w4.hip; the codes themselves are public through lgd_attn_plan (include/lgd_hip.h) and named in ops.ATTN_VARIANTS.
//
//   code = family * 100000 + DP * 100 + sub        DP: padded head dim of the instantiation (DK for the 32x32x16 kernel)
//
// Every launch path first CHOOSES a code (plan_* functions: arguments + option state -> code) and then switches on it, so
// the query and the launch cannot disagree.
//
// Two tables on the Python side mirror this file by hand and move with it: ops.ATTN_VARIANTS (a name for every code the
// plan_* functions can return) and ops.ATTN_VARIANTS_ENV_ONLY (the codes only LGD_ATTN_NW / LGD_ATTN_BWD select, which the
// conformance suite is therefore not required to reach).  A new code, or a threshold change that makes an env-only code
// reachable by default, needs both edited; tests/test_attn_conformance_cpu.py sweeps the plan against them.
#pragma once

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

int lgd_attn_bwd_plan(int B, int H, int Sq, int Sk, int d);          // attn_bwd.hip
int lgd_cross_attn_bwd_plan(int Sk, int d, int aligned);              // attn_bwd.hip
