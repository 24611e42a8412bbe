// The option state of the library (lgd_set_option / lgd_get_option, include/lgd_hip.h): one table in options.hip, one
// reader for the launch paths.  Internal; host only.
#pragma once

enum LgdOption {   // row index of the table in options.hip (same order)
  OPT_CFG_PAIR, OPT_GN_FUSED, OPT_GN_SLAB, OPT_LN_STREAM, OPT_GN_APPLY_WGS,
  OPT_ATTN32, OPT_ATTN32_NW, OPT_ATTN32_VAR, OPT_ATTN_W4, OPT_ATTN_W4_PIPE, OPT_COUNT
};

// Current value: a relaxed atomic load.  Lane threads launch concurrently while another thread may set an option, so a
// launch path that uses a value twice reads it once into a local.
int lgd_option(LgdOption o);
