// A program of its own around the host monitor of monitorhost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_monitor_cpu.py builds it twice, plain and
// with -fsanitize=address,undefined, and compares what the two print).
//
//   monitorhost_main STREAM...   each STREAM a file written by the test: int32 n, int32 steps, then per step reward f32[n],
//                                terminated u8[n], truncated u8[n]
// For every stream: unlimited mode and the quotas of n_eval_episodes in {1, n - 1, n, 3 n + 7}; one line per case with the
// number of counted episodes and an FNV-1a digest of the stats, the histogram and the log.
#include <inttypes.h>
#include <stdio.h>

#include <set>

#include "monitorhost.hpp"

namespace {

uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

}  // namespace

int main(int argc, char** argv) {
  const int max_len = 12;  // some of the 40-step episodes are longer: bin 0
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[2];
    if (!f || fread(head, sizeof(int32_t), 2, f) != 2 || head[0] <= 0 || head[1] < 0) { fprintf(stderr, "%s: bad stream\n", argv[a]); return 2; }
    const int n = head[0], steps = head[1];
    std::vector<float> reward((size_t)n * steps);
    std::vector<uint8_t> te((size_t)n * steps), tr((size_t)n * steps);
    for (int t = 0; t < steps; t++) {
      const size_t o = (size_t)n * t, N = (size_t)n;
      if (fread(&reward[o], 4, N, f) != N || fread(&te[o], 1, N, f) != N || fread(&tr[o], 1, N, f) != N) { fprintf(stderr, "%s: short stream\n", argv[a]); return 2; }
    }
    fclose(f);
    std::set<int> quotas = {-1, 1, n - 1, n, 3 * n + 7};  // -1: unlimited
    for (const int E : quotas) {
      monitorhost::HostMonitor m(n, max_len, E < 0 ? 0 : E);
      std::vector<int32_t> targets((size_t)n);
      for (int i = 0; i < n; i++) targets[(size_t)i] = (E + i) / n;
      if (m.reset(E < 0 ? nullptr : targets.data()) != 0) { fprintf(stderr, "reset refused the targets\n"); return 2; }
      for (int t = 0; t < steps; t++) {
        if (t == steps / 2) {  // stats in the middle of a stream change nothing
          brs_episode_stats mid;
          m.stats(&mid);
        }
        m.update(&reward[(size_t)n * t], &te[(size_t)n * t], &tr[(size_t)n * t]);
      }
      brs_episode_stats s;
      m.stats(&s);
      uint64_t h = fnv(14695981039346656037ull, &s, sizeof(s));
      h = fnv(h, m.hist.data(), m.hist.size() * sizeof(int64_t));
      const size_t R = (size_t)m.rows;
      if (R) {
        h = fnv(h, m.log_env.data(), R * 4); h = fnv(h, m.log_ret.data(), R * 8); h = fnv(h, m.log_len.data(), R * 4);
        h = fnv(h, m.log_time_limit.data(), R);
      }
      printf("n=%d quota=%d episodes=%" PRId64 " digest=%016" PRIx64 "\n", n, E, s.episodes, h);
    }
  }
  return 0;
}
