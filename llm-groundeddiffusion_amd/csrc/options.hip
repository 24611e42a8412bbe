// The option table: every switch lgd_set_option / lgd_get_option know, with its allowed values, its default and the
// environment variable that gives its initial value.  Pure host code (no HIP header): the launch paths of attn.hip,
// attn_w4.hip and norm.hip read it through lgd_option (options.h), from every lane thread at launch time, while another
// thread may set a value — hence the atomics.  include/lgd_hip.h documents what each value selects.
#include "options.h"
#include "../../include/lgd_hip.h"
#include <atomic>
#include <stdlib.h>
#include <string.h>

namespace {

struct Option {
  const char* name;
  int lo, hi, step;         // allowed: lo, lo + step, .. hi
  int def;
  const char* env;          // initial value (read once, for the whole table, before the first answer), or nullptr
  std::atomic<int> value;
  constexpr Option(const char* name, int lo, int hi, int step, int def, const char* env)
      : name(name), lo(lo), hi(hi), step(step), def(def), env(env), value(def) {}
  bool allows(int v) const { return v >= lo && v <= hi && (v - lo) % step == 0; }
};

Option g_options[OPT_COUNT] = {      // in the order of LgdOption
    {"cfg_pair", 0, 1, 1, 1, nullptr},           // the library only keeps it: the plan builder reads it back
    {"gn_fused", 0, 4096, 1, 256, nullptr},      // largest map (pixels) the one-launch GroupNorm takes; 0 = always two launches
    {"gn_slab", 0, 1, 1, 1, nullptr},            // the one-launch GroupNorm backward takes every slab of <= 96 KB it can hold
    {"ln_stream", 0, 1, 1, 1, nullptr},          // statistics-only LayerNorm runs ln_stats_kernel / the row kernels
    {"gn_apply_wgs", 64, 8192, 1, 1024, nullptr},   // (tools) workgroups per launch the GroupNorm apply passes aim at
    {"attn32", 0, 2, 1, 1, "LGD_ATTN32"},        // 32x32x16 kernel: 0 = never (A/B timing), 1 = default, 2 = every size (tests)
    {"attn32_nw", 4, 8, 4, 8, "LGD_ATTN32_NW"},  // its waves per workgroup: 8 (256 queries per workgroup) or 4
    {"attn32_var", 0, 2, 1, 0, nullptr},         // (tools) 0 = prefetch 2 slots ahead, pinned order; 1 = 4 ahead; 2 = compiler's order
    {"attn_w4", 0, 2, 1, 1, "LGD_ATTN_W4"},      // d = 40 kernel (attn_w4.hip): 0 = never (A/B timing), 1 = default, 2 = every size (tests)
    {"attn_w4_pipe", 0, 1, 1, 1, "LGD_W4_PIPE"}, // 1 = one wave per SIMD, in-wave software pipeline; 0 = two waves per SIMD
};

// a value of the environment outside the option's allowed set leaves the default
void read_env_once() {
  static const bool done = [] {
    for (Option& o : g_options) {
      const char* e = o.env ? getenv(o.env) : nullptr;
      if (e && o.allows(atoi(e))) o.value.store(atoi(e), std::memory_order_relaxed);
    }
    return true;
  }();
  (void)done;
}

Option* find(const char* name) {
  if (!name) return nullptr;
  read_env_once();
  for (Option& o : g_options)
    if (!strcmp(o.name, name)) return &o;
  return nullptr;
}

}  // namespace

int lgd_option(LgdOption o) {
  read_env_once();
  return g_options[o].value.load(std::memory_order_relaxed);
}

extern "C" int lgd_get_option(const char* name) {
  const Option* o = find(name);
  return o ? o->value.load(std::memory_order_relaxed) : LGD_ERR_ARG;
}

extern "C" int lgd_set_option(const char* name, int value) {
  Option* o = find(name);
  if (!o || !o->allows(value)) return LGD_ERR_ARG;
  o->value.store(value, std::memory_order_relaxed);
  return LGD_OK;
}
