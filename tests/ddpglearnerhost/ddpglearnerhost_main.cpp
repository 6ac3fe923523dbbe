// A program of its own around the host build of ddpglearnerhost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_ddpg_learner_cpu.py builds it twice, plain
// and with -fsanitize=address,undefined, and compares what the two print).
//
//   ddpglearnerhost_main CASE...   each CASE a file written by the test: int32 m, steps; float tau; double lr, beta1, beta2, eps;
//                                  actor f32[NACTOR]; critic f32[NCRITIC]; then per step obs f32[m][6], act f32[m][2], y f32[m]
//   ddpglearnerhost_main --split-sweep LO HI M...   sample_split checked over every m of [LO, HI] (one line: how many m break a
//                                  rule, the first of them and its bits), then one line "m mp span nsplit" per M
// For every case: the targets start as copies, the moments at zero; per step critic_grad, apply (critic), actor_grad with the
// updated critic, apply (actor).  One line with FNV-1a digests of the four networks and of the two last gradient buffers.  Every
// array has exactly its size, so an index past an end is seen.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ddpglearnerhost.hpp"

namespace {

uint64_t fnv(const std::vector<float>& v) {
  uint64_t h = 14695981039346656037ull;
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t i = 0; i < v.size() * sizeof(float); i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

bool read(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(float), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace ddpglearnerhost;
  constexpr size_t NA = BRS_DDPG_NACTOR, NC = BRS_DDPG_NCRITIC;
  if (argc >= 4 && !strcmp(argv[1], "--split-sweep")) {
    int first_bad;
    unsigned first_mask;
    const long long bad = split_sweep(atoi(argv[2]), atoi(argv[3]), &first_bad, &first_mask);
    printf("sweep %d..%d bad=%lld first=%d mask=%u\n", atoi(argv[2]), atoi(argv[3]), bad, first_bad, first_mask);
    for (int a = 4; a < argc; a++) {
      int out[3];
      split_of(atoi(argv[a]), out);
      printf("%d %d %d %d\n", atoi(argv[a]), out[0], out[1], out[2]);
    }
    return bad ? 1 : 0;
  }
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[2];
    float tau;
    brs_adam_config cfg;
    if (!f || fread(head, sizeof(int32_t), 2, f) != 2 || fread(&tau, sizeof tau, 1, f) != 1 || fread(&cfg, sizeof cfg, 1, f) != 1 || head[0] < 1 ||
        head[1] < 1) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    const int m = head[0], steps = head[1];
    const size_t M = (size_t)m;
    std::vector<float> actor, critic;
    if (!read(f, actor, NA) || !read(f, critic, NC)) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    std::vector<float> actor_t(actor), critic_t(critic), ma(NA, 0.0f), va(NA, 0.0f), mc(NC, 0.0f), vc(NC, 0.0f), ga(NA + 2), gc(NC + 2);
    for (int t = 0; t < steps; t++) {
      std::vector<float> obs, act, y;
      if (!read(f, obs, M * 6) || !read(f, act, M * 2) || !read(f, y, M)) {
        fprintf(stderr, "%s: short case\n", argv[a]);
        return 2;
      }
      if (critic_grad(critic.data(), m, obs.data(), act.data(), y.data(), gc.data()) != 0 ||
          apply((int)NC, critic.data(), gc.data(), mc.data(), vc.data(), critic_t.data(), &cfg, t + 1, tau) != 0 ||
          actor_grad(actor.data(), critic.data(), m, obs.data(), ga.data()) != 0 ||
          apply((int)NA, actor.data(), ga.data(), ma.data(), va.data(), actor_t.data(), &cfg, t + 1, tau) != 0) {
        fprintf(stderr, "%s: step %d refused\n", argv[a], t);
        return 2;
      }
    }
    fclose(f);
    printf("m=%d steps=%d actor=%016" PRIx64 " critic=%016" PRIx64 " actor_target=%016" PRIx64 " critic_target=%016" PRIx64 " ga=%016" PRIx64
           " gc=%016" PRIx64 "\n",
           m, steps, fnv(actor), fnv(critic), fnv(actor_t), fnv(critic_t), fnv(ga), fnv(gc));
  }
  return 0;
}
