// A program of its own around the host build of sachost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_sac_cpu.py builds it twice, plain and with
// -fsanitize=address,undefined, and compares what the two print).
//
//   sachost_main CASE...   each CASE a file written by the test: int32 m, steps, learn_alpha; uint32 draw0; uint64 seed; float tau,
//                          gamma, target_entropy; double lr, beta1, beta2, eps; actor f32[NACTOR + 1]; critics f32[2 NCRITIC]; then
//                          per step obs f32[m][6], act f32[m][2], next_obs f32[m][6], reward f32[m], done u8[m]
// For every case: the critics' targets start as copies, the moments at zero; per step an act on obs (step counter t), the SAC target
// (draw0 + t) from the critics' targets and the current actor, then one update (actor noise draw0 + t).  One line with FNV-1a digests
// of the three networks, of the last action, y, a', logp', z and of the two gradient buffers.  Every array has exactly its size, so
// an index past an end is seen.
#include <inttypes.h>
#include <stdio.h>

#include <vector>

#include "sachost.hpp"

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
  using namespace sachost;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[3];
    uint32_t draw0;
    uint64_t seed;
    float fl[3];
    brs_adam_config cfg;
    if (!f || fread(head, sizeof(int32_t), 3, f) != 3 || fread(&draw0, sizeof draw0, 1, f) != 1 || fread(&seed, sizeof seed, 1, f) != 1 ||
        fread(fl, sizeof(float), 3, f) != 3 || fread(&cfg, sizeof cfg, 1, f) != 1 || head[0] < 1 || head[1] < 1) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    const int m = head[0], steps = head[1], learn_alpha = head[2];
    const size_t M = (size_t)m;
    std::vector<float> actor, critics;
    if (!read(f, actor, (size_t)NA1) || !read(f, critics, 2 * (size_t)NC)) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    State s(actor.data(), critics.data());
    std::vector<float> y(M), na(M * 2), lp(M), z(M * 2), action(M * 2), mu(M * 2), ls(M * 2), za(M * 2);
    for (int t = 0; t < steps; t++) {
      std::vector<float> obs, act, next_obs, reward;
      std::vector<uint8_t> done;
      if (!read(f, obs, M * 6) || !read(f, act, M * 2) || !read(f, next_obs, M * 6) || !read(f, reward, M) || !read(f, done, M)) {
        fprintf(stderr, "%s: short case\n", argv[a]);
        return 2;
      }
      if (sac_act_host(s.actor.data(), m, obs.data(), seed, 0, (uint32_t)t, 0, 0, action.data(), mu.data(), ls.data(), za.data()) != 0 ||
          sac_target_host(s.actor.data(), s.critics_t.data(), m, next_obs.data(), reward.data(), done.data(), fl[1], seed, draw0 + (uint32_t)t,
                          y.data(), na.data(), lp.data(), z.data()) != 0) {
        fprintf(stderr, "%s: act or target %d refused\n", argv[a], t);
        return 2;
      }
      if (step(s, m, obs.data(), act.data(), y.data(), seed, draw0 + (uint32_t)t, learn_alpha, fl[2], &cfg, fl[0]) != 0) {
        fprintf(stderr, "%s: step %d refused\n", argv[a], t);
        return 2;
      }
    }
    fclose(f);
    printf("m=%d steps=%d actor=%016" PRIx64 " critics=%016" PRIx64 " critics_target=%016" PRIx64 " action=%016" PRIx64 " y=%016" PRIx64
           " a=%016" PRIx64 " logp=%016" PRIx64 " z=%016" PRIx64 " ga=%016" PRIx64 " gc=%016" PRIx64 "\n",
           m, steps, fnv(s.actor), fnv(s.critics), fnv(s.critics_t), fnv(action), fnv(y), fnv(na), fnv(lp), fnv(z), fnv(s.ga), fnv(s.gc));
  }
  return 0;
}
