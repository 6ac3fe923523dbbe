// A program of its own around the host build of the normalising replay sample (vecnormreplayhost.hpp), so that it can run under
// AddressSanitizer and UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_vecnorm_replay_cpu.py
// builds it twice, plain and with -fsanitize=address,undefined, and compares what the two print).
//
//   vecnormreplayhost_main BUFFER...   each BUFFER a file written by the test: int32 n, int32 cap, uint32 draw, int32 zero,
//                                      float64 clip_obs, float64 clip_reward, float64 stats[21], then the storage: obs f32[cap][n][6],
//                                      next_obs f32[cap][n][6], action f32[cap][n][2], reward f32[cap][n], done u8[cap][n]
// For every buffer: all four settings of norm_obs / norm_reward, the full buffer and a partly filled one (size 3), every m of the
// GPU test; the outputs are allocated at their exact sizes.  One line per setting with the number of clipped elements and an
// FNV-1a digest of every output and of idx.
#include <inttypes.h>
#include <stdio.h>

#include "vecnormreplayhost.hpp"

namespace {

uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

template <class T> bool read_into(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

}  // namespace

int main(int argc, char** argv) {
  const int ms[] = {1, 31, 32, 33, 257, 2049};
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[4];
    double clips[2], stats[brs::vecnorm::NSTAT];
    if (!f || fread(head, sizeof(int32_t), 4, f) != 4 || fread(clips, sizeof(double), 2, f) != 2 ||
        fread(stats, sizeof(double), brs::vecnorm::NSTAT, f) != (size_t)brs::vecnorm::NSTAT || head[0] <= 0 || head[1] < 3) {
      fprintf(stderr, "%s: bad buffer\n", argv[a]);
      return 2;
    }
    const int n = head[0], cap = head[1];
    const uint32_t draw = (uint32_t)head[2];
    const size_t cells = (size_t)n * cap;
    std::vector<float> obs(6 * cells), next_obs(6 * cells), action(2 * cells), reward(cells);
    std::vector<uint8_t> done(cells);
    const bool ok = read_into(f, obs) && read_into(f, next_obs) && read_into(f, action) && read_into(f, reward) && read_into(f, done);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short buffer\n", argv[a]); return 2; }
    const brs_replay_storage store = {obs.data(), next_obs.data(), action.data(), reward.data(), done.data()};
    for (int mode = 0; mode < 4; mode++) {
      const brs_vecnorm_config cfg = {0.99, 1e-8, clips[0], clips[1], mode & 1, (mode >> 1) & 1};
      vecnormhost::HostVecNorm v(n, cfg);
      memcpy(v.stats, stats, sizeof(stats));
      uint64_t h = 14695981039346656037ull;
      long clipped = 0;
      for (int size : {cap, 3}) {
        for (int m : ms) {
          const size_t M = (size_t)m;
          std::vector<float> o(6 * M), no(6 * M), ac(2 * M), r(M);
          std::vector<uint8_t> d(M);
          std::vector<int32_t> idx(2 * M);
          const brs_replay_storage out = {o.data(), no.data(), ac.data(), r.data(), d.data()};
          const char* why = nullptr;
          if (vecnormreplayhost::replay_sample(v, store, n, cap, size, m, 1234u, draw, out, idx.data(), &why)) {
            fprintf(stderr, "%s: %s\n", argv[a], why);
            return 2;
          }
          for (size_t k = 0; k < 2 * M; k += 2)
            if (idx[k] < 0 || idx[k] >= size || idx[k + 1] < 0 || idx[k + 1] >= n) { fprintf(stderr, "%s: idx out of range\n", argv[a]); return 2; }
          if (cfg.norm_obs)
            for (float x : o) clipped += x == (float)clips[0] || x == (float)-clips[0];
          h = fnv(h, o.data(), 4 * o.size()); h = fnv(h, no.data(), 4 * no.size()); h = fnv(h, ac.data(), 4 * ac.size());
          h = fnv(h, r.data(), 4 * r.size()); h = fnv(h, d.data(), d.size()); h = fnv(h, idx.data(), 4 * idx.size());
        }
      }
      printf("n=%d cap=%d norm_obs=%d norm_reward=%d clipped_obs=%ld digest=%016" PRIx64 "\n", n, cap, cfg.norm_obs, cfg.norm_reward, clipped, h);
    }
  }
  return 0;
}
