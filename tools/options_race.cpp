// Race check of the option table (csrc/options.hip) under ThreadSanitizer: reader threads read every option in a loop, the
// way lane threads do at launch time, while one thread sets allowed values.  Host only: options.hip includes no HIP
// header, so the host compiler builds both files; run from the repository root, it must report nothing and print "ok".
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -x c++ tools/options_race.cpp llm-groundeddiffusion_amd/csrc/options.hip \
//       -o /tmp/options_race && /tmp/options_race
#include <atomic>
#include <stdio.h>
#include <thread>
#include <vector>
#include "../include/lgd_hip.h"
#include "../llm-groundeddiffusion_amd/csrc/options.h"

struct Row { const char* name; int lo, hi, step; };
static const Row ROWS[OPT_COUNT] = {   // in the order of LgdOption; the allowed values include/lgd_hip.h documents
    {"cfg_pair", 0, 1, 1}, {"gn_fused", 0, 4096, 1}, {"gn_slab", 0, 1, 1}, {"ln_stream", 0, 1, 1}, {"gn_apply_wgs", 64, 8192, 1},
    {"attn32", 0, 2, 1}, {"attn32_nw", 4, 8, 4}, {"attn32_var", 0, 2, 1}, {"attn_w4", 0, 2, 1}, {"attn_w4_pipe", 0, 1, 1},
};

int main() {
  std::atomic<bool> stop{false};
  std::atomic<long> bad{0};
  std::vector<std::thread> readers;
  for (int t = 0; t < 6; ++t)      // the first reads race with the first set for the one-time read of the environment
    readers.emplace_back([&] {
      while (!stop.load(std::memory_order_relaxed))
        for (int o = 0; o < OPT_COUNT; ++o) {
          const int v = lgd_option((LgdOption)o), g = lgd_get_option(ROWS[o].name);
          for (int x : {v, g})
            if (x < ROWS[o].lo || x > ROWS[o].hi || (x - ROWS[o].lo) % ROWS[o].step) bad.fetch_add(1);
        }
    });
  std::thread writer([&] {
    for (int it = 0; it < 20000; ++it)
      for (int o = 0; o < OPT_COUNT; ++o) {
        const Row& r = ROWS[o];
        const int n = (r.hi - r.lo) / r.step + 1;
        if (lgd_set_option(r.name, r.lo + (it % n) * r.step) != LGD_OK) bad.fetch_add(1);
        if (lgd_set_option(r.name, r.hi + 1) != LGD_ERR_ARG) bad.fetch_add(1);
      }
  });
  writer.join();
  stop.store(true);
  for (std::thread& t : readers) t.join();
  printf(bad.load() ? "FAILED: %ld values outside their range\n" : "ok\n", bad.load());
  return bad.load() ? 1 : 0;
}
