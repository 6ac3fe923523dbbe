// A program of its own around the host build of td3host.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_td3_cpu.py builds it twice, plain and with
// -fsanitize=address,undefined, and compares what the two print).
//
//   td3host_main CASE...   each CASE a file written by the test: int32 m, steps, policy_delay; uint32 draw0; uint64 seed; float tau,
//                          gamma, policy_noise, noise_clip; double lr, beta1, beta2, eps; actor f32[NACTOR]; critics f32[2 NCRITIC];
//                          then per step obs f32[m][6], act f32[m][2], next_obs f32[m][6], reward f32[m], done u8[m]
// For every case: the targets start as copies, the moments at zero; per step the TD3 target (draw0 + step) from the targets as they
// are, then one update with the delay.  One line with FNV-1a digests of the four networks, of the last y, a', z and of the two
// gradient buffers.  Every array has exactly its size, so an index past an end is seen.
#include <inttypes.h>
#include <stdio.h>

#include <vector>

#include "td3host.hpp"

namespace {

template <class T> uint64_t fnv(const std::vector<T>& v) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t i = 0; i < v.size() * sizeof(T); i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

template <class T> bool read(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace td3host;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[3];
    uint32_t draw0;
    uint64_t seed;
    float fl[4];
    brs_adam_config cfg;
    if (!f || fread(head, sizeof(int32_t), 3, f) != 3 || fread(&draw0, sizeof draw0, 1, f) != 1 || fread(&seed, sizeof seed, 1, f) != 1 ||
        fread(fl, sizeof(float), 4, f) != 4 || fread(&cfg, sizeof cfg, 1, f) != 1 || head[0] < 1 || head[1] < 1 || head[2] < 1) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    const int m = head[0], steps = head[1], delay = head[2];
    const size_t M = (size_t)m;
    std::vector<float> actor, critics;
    if (!read(f, actor, (size_t)BRS_DDPG_NACTOR) || !read(f, critics, 2 * (size_t)NC)) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    State s(actor.data(), critics.data());
    std::vector<float> y(M), na(M * 2), z(M * 2);
    int actor_updates = 0;
    for (int t = 0; t < steps; t++) {
      std::vector<float> obs, act, next_obs, reward;
      std::vector<uint8_t> done;
      if (!read(f, obs, M * 6) || !read(f, act, M * 2) || !read(f, next_obs, M * 6) || !read(f, reward, M) || !read(f, done, M)) {
        fprintf(stderr, "%s: short case\n", argv[a]);
        return 2;
      }
      if (td3_target(s.actor_t.data(), s.critics_t.data(), m, next_obs.data(), reward.data(), done.data(), fl[1], fl[2], fl[3], seed,
                     draw0 + (uint32_t)t, y.data(), na.data(), z.data()) != 0) {
        fprintf(stderr, "%s: target %d refused\n", argv[a], t);
        return 2;
      }
      const int rc = step(s, m, obs.data(), act.data(), y.data(), &cfg, fl[0], delay);
      if (rc < 0) {
        fprintf(stderr, "%s: step %d refused\n", argv[a], t);
        return 2;
      }
      actor_updates += rc;
    }
    fclose(f);
    printf("m=%d steps=%d actor_updates=%d actor=%016" PRIx64 " critics=%016" PRIx64 " actor_target=%016" PRIx64 " critics_target=%016" PRIx64
           " y=%016" PRIx64 " a=%016" PRIx64 " z=%016" PRIx64 " ga=%016" PRIx64 " gc=%016" PRIx64 "\n",
           m, steps, actor_updates, fnv(s.actor), fnv(s.critics), fnv(s.actor_t), fnv(s.critics_t), fnv(y), fnv(na), fnv(z), fnv(s.ga), fnv(s.gc));
  }
  return 0;
}
