// A program of its own around the host A2C learner of a2chost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_a2c_cpu.py builds it twice, plain and with
// -fsanitize=address,undefined, and compares what the two print).
//
//   a2chost_main CASE...   each CASE a file written by the test: int32 n_rows, m, max_workgroups, steps, with_idx; the brs_a2c_config;
//                          params f32[NPARAM]; obs f32[n_rows][6]; act f32[n_rows][2]; adv, ret f32[n_rows]; idx i32[m] if with_idx
// For every case: `steps` times grad + apply from square averages of one; one line with the steps taken and FNV-1a digests of the
// last gradient buffer, the parameters and the square averages.
#include <inttypes.h>
#include <stdio.h>

#include "a2chost.hpp"

namespace {

uint64_t fnv(const void* data, size_t bytes) {
  uint64_t h = 14695981039346656037ull;
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
  using namespace a2chost;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[5];
    brs_a2c_config cfg;
    if (!f || fread(head, sizeof(int32_t), 5, f) != 5 || head[0] <= 0 || head[1] < 1 || fread(&cfg, sizeof(cfg), 1, f) != 1) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    const size_t N = (size_t)head[0], M = (size_t)head[1];
    std::vector<float> params, obs, act, adv, ret;
    std::vector<int32_t> idx;
    if (!read(f, params, (size_t)NPARAM) || !read(f, obs, N * OBS) || !read(f, act, N * ACT) || !read(f, adv, N) || !read(f, ret, N) ||
        (head[4] && !read(f, idx, M))) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    fclose(f);
    HostA2C l(head[2]);
    std::vector<float> grad((size_t)(NPARAM + NSTAT)), sq((size_t)NPARAM, 1.0f);
    for (int s = 0; s < head[3]; s++) {
      if (l.grad(params.data(), head[0], obs.data(), act.data(), adv.data(), ret.data(), head[4] ? idx.data() : nullptr, head[1], &cfg,
                 grad.data()) != 0 ||
          l.apply(params.data(), grad.data(), sq.data(), &cfg) != 0) {
        fprintf(stderr, "%s: the learner refused the case\n", argv[a]);
        return 2;
      }
    }
    printf("m=%d steps=%" PRId64 " bad=%d grad=%016" PRIx64 " params=%016" PRIx64 " sq=%016" PRIx64 "\n", head[1], l.info.steps, l.info.bad_index,
           fnv(grad.data(), grad.size() * sizeof(float)), fnv(params.data(), params.size() * sizeof(float)), fnv(sq.data(), sq.size() * sizeof(float)));
  }
  return 0;
}
