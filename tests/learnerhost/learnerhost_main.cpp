// A program of its own around the host learner of learnerhost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_learner_cpu.py builds it twice, plain and
// with -fsanitize=address,undefined, and compares what the two print).
//
//   learnerhost_main CASE...   each CASE a file written by the test: int32 n_rows, m, max_workgroups, steps; the brs_ppo_config;
//                              params f32[NPARAM]; obs f32[n_rows][6]; act f32[n_rows][2]; logp_old, adv, ret f32[n_rows]; idx i32[m]
// For every case: `steps` times grad + apply from zeroed Adam moments; one line with the Adam steps taken and FNV-1a digests of
// the last gradient buffer and of the parameters.
#include <inttypes.h>
#include <stdio.h>

#include "learnerhost.hpp"

namespace {

uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

template <class T> bool read(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  using namespace learnerhost;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[4];
    brs_ppo_config cfg;
    if (!f || fread(head, sizeof(int32_t), 4, f) != 4 || head[0] <= 0 || head[1] < 2 || fread(&cfg, sizeof(cfg), 1, f) != 1) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    const size_t N = (size_t)head[0], M = (size_t)head[1];
    std::vector<float> params, obs, act, logp, adv, ret;
    std::vector<int32_t> idx;
    if (!read(f, params, (size_t)NPARAM) || !read(f, obs, N * OBS) || !read(f, act, N * ACT) || !read(f, logp, N) || !read(f, adv, N) ||
        !read(f, ret, N) || !read(f, idx, M)) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    fclose(f);
    HostLearner l(head[2]);
    std::vector<float> grad((size_t)(NPARAM + NSTAT)), m1((size_t)NPARAM, 0.0f), m2((size_t)NPARAM, 0.0f);
    for (int s = 0; s < head[3]; s++) {
      if (l.grad(params.data(), head[0], obs.data(), act.data(), logp.data(), adv.data(), ret.data(), idx.data(), head[1], &cfg, grad.data()) != 0 ||
          l.apply(params.data(), grad.data(), m1.data(), m2.data(), &cfg) != 0) {
        fprintf(stderr, "%s: the learner refused the case\n", argv[a]);
        return 2;
      }
    }
    printf("m=%d steps=%" PRId64 " bad=%d grad=%016" PRIx64 " params=%016" PRIx64 "\n", head[1], l.info.steps, l.info.bad_index,
           fnv(14695981039346656037ull, grad.data(), grad.size() * sizeof(float)),
           fnv(14695981039346656037ull, params.data(), params.size() * sizeof(float)));
  }
  return 0;
}
