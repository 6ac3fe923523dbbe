// A program of its own around the host build of sacarchhost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_sac_arch_cpu.py builds it twice, plain and with
// -fsanitize=address,undefined, and compares what the two print).
//
//   sacarchhost_main M STEPS   weights in torch's default init (uniform in +-1 / sqrt(fan_in)) and inputs from a 64-bit LCG, so that
//                              the program needs no file; per step an act on obs, the SAC target from the critics' targets and the
//                              current actor, the twin critic gradient, Adam with Polyak, the actor's gradient, Adam
// One line with FNV-1a digests of the three networks, of the last action, y, a', logp', z and of the two gradient buffers.  Every
// array has exactly its size, so an index past an end is seen.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sacarchhost.hpp"

namespace {

template <class T> uint64_t fnv(const std::vector<T>& v) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t i = 0; i < v.size() * sizeof(T); i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

struct Lcg {
  uint64_t s;
  float unit() {  // in [-1, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(s >> 11) * (1.0 / 4503599627370496.0) - 1.0);
  }
};

// W1 b1 W2 b2 W3 b3 of network N into w
template <class N> void init(Lcg& r, float* w) {
  const int fan[3] = {N::IN, N::H1, N::H2}, rows[3] = {N::H1, N::H2, N::OUT};
  for (int l = 0; l < 3; l++) {
    const float bound = 1.0f / sqrtf((float)fan[l]);
    for (int i = 0; i < rows[l] * fan[l] + rows[l]; i++) *w++ = bound * r.unit();
  }
}

}  // namespace

int main(int argc, char** argv) {
  using H = sacarchhost::H;
  if (argc != 3 || atoi(argv[1]) < 1 || atoi(argv[2]) < 1) {
    fprintf(stderr, "usage: sacarchhost_main M STEPS\n");
    return 2;
  }
  const int m = atoi(argv[1]), steps = atoi(argv[2]);
  const size_t M = (size_t)m;
  Lcg r{12345};
  std::vector<float> actor((size_t)H::NA1), critics(2 * (size_t)H::NC);
  init<H::Pi>(r, actor.data());
  actor[H::NA - 2] -= 2.0f;  // the two log_std biases: sigma around 0.13
  actor[H::NA - 1] -= 2.0f;
  actor[H::NA] = -0.5f;      // log_ent_coef
  init<H::Qf>(r, critics.data());
  init<H::Qf>(r, critics.data() + H::NC);
  H::State s(actor.data(), critics.data());
  const brs_adam_config cfg = {3e-4, 0.9, 0.999, 1e-8};
  const uint64_t seed = 11;
  std::vector<float> y(M), na(M * 2), lp(M), z(M * 2), action(M * 2), mu(M * 2), ls(M * 2), za(M * 2);
  for (int t = 0; t < steps; t++) {
    std::vector<float> obs(M * 6), act(M * 2), next_obs(M * 6), reward(M);
    std::vector<uint8_t> done(M);
    for (auto& v : obs) v = 1.5f * r.unit();
    for (auto& v : act) v = r.unit();
    for (auto& v : next_obs) v = 1.5f * r.unit();
    for (auto& v : reward) v = r.unit();
    for (size_t i = 0; i < M; i++) done[i] = i % 3 == 1;
    if (H::act(s.actor.data(), m, obs.data(), seed, 0, (uint32_t)t, 0, 0, action.data(), mu.data(), ls.data(), za.data()) != 0 ||
        H::target(s.actor.data(), s.critics_t.data(), m, next_obs.data(), reward.data(), done.data(), 0.99f, seed, (uint32_t)t, y.data(), na.data(),
                  lp.data(), z.data()) != 0 ||
        H::step(s, m, obs.data(), act.data(), y.data(), seed, (uint32_t)t, 1, -2.0f, &cfg, 0.005f) != 0) {
      fprintf(stderr, "step %d refused\n", t);
      return 2;
    }
  }
  printf("arch=%d m=%d steps=%d actor=%016" PRIx64 " critics=%016" PRIx64 " critics_target=%016" PRIx64 " action=%016" PRIx64 " y=%016" PRIx64
         " a=%016" PRIx64 " logp=%016" PRIx64 " z=%016" PRIx64 " ga=%016" PRIx64 " gc=%016" PRIx64 "\n",
         H::Arch::ID, m, steps, fnv(s.actor), fnv(s.critics), fnv(s.critics_t), fnv(action), fnv(y), fnv(na), fnv(lp), fnv(z), fnv(s.ga), fnv(s.gc));
  return 0;
}
