// A program of its own around the host VecNormalize of vecnormhost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_vecnorm_cpu.py builds it twice, plain and
// with -fsanitize=address,undefined, and compares what the two print).
//
//   vecnormhost_main STREAM...   each STREAM a file written by the test: int32 n, int32 steps, float64 clip_obs, float64
//                                clip_reward, obs f32[n][6] of the reset, then per step obs f32[n][6], reward f32[n],
//                                terminated u8[n], truncated u8[n], terminal_obs f32[n][6]
// For every stream: all four settings of norm_obs / norm_reward, training, with the last step frozen and a stateless call at
// m = n + 3; one line per case with the return statistics' count and an FNV-1a digest of every output, the statistics and the
// returns.
#include <inttypes.h>
#include <stdio.h>

#include "vecnormhost.hpp"

namespace {

uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

template <class T> bool read_into(FILE* f, std::vector<T>& v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

}  // namespace

int main(int argc, char** argv) {
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[2];
    double clips[2];
    if (!f || fread(head, sizeof(int32_t), 2, f) != 2 || fread(clips, sizeof(double), 2, f) != 2 || head[0] <= 0 || head[1] < 0) {
      fprintf(stderr, "%s: bad stream\n", argv[a]);
      return 2;
    }
    const int n = head[0], steps = head[1];
    const size_t N = (size_t)n;
    std::vector<float> obs0(6 * N), obs(6 * N * steps), tobs(6 * N * steps), reward(N * steps);
    std::vector<uint8_t> te(N * steps), tr(N * steps);
    bool ok = read_into(f, obs0);
    for (int t = 0; ok && t < steps; t++) {
      ok = fread(&obs[6 * N * t], 4, 6 * N, f) == 6 * N && fread(&reward[N * t], 4, N, f) == N && fread(&te[N * t], 1, N, f) == N &&
           fread(&tr[N * t], 1, N, f) == N && fread(&tobs[6 * N * t], 4, 6 * N, f) == 6 * N;
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short stream\n", argv[a]); return 2; }
    for (int mode = 0; mode < 4; mode++) {
      const brs_vecnorm_config cfg = {0.99, 1e-8, clips[0], clips[1], mode & 1, (mode >> 1) & 1};
      vecnormhost::HostVecNorm v(n, cfg);
      std::vector<float> obs_out(6 * N), tobs_out(6 * N), reward_out(N), more_in(6 * (N + 3)), more_out(6 * (N + 3));
      uint64_t h = 14695981039346656037ull;
      v.reset(obs0.data(), true, obs_out.data());
      h = fnv(h, obs_out.data(), 4 * obs_out.size());
      for (int t = 0; t < steps; t++) {
        v.step(&obs[6 * N * t], &reward[N * t], &te[N * t], &tr[N * t], &tobs[6 * N * t], t + 1 < steps, obs_out.data(), reward_out.data(),
               tobs_out.data());
        h = fnv(h, obs_out.data(), 4 * obs_out.size()); h = fnv(h, reward_out.data(), 4 * reward_out.size());
        h = fnv(h, tobs_out.data(), 4 * tobs_out.size()); h = fnv(h, v.stats, sizeof(v.stats));
        h = fnv(h, v.returns.data(), 8 * v.returns.size());
      }
      for (size_t k = 0; k < more_in.size(); k++) more_in[k] = obs0[k % obs0.size()] * 1.5f;
      v.normalize_obs(n + 3, more_in.data(), more_out.data());
      h = fnv(h, more_out.data(), 4 * more_out.size());
      v.normalize_reward(n + 3, more_in.data(), more_out.data());
      h = fnv(h, more_out.data(), 4 * (N + 3));
      printf("n=%d norm_obs=%d norm_reward=%d ret_count=%.4f digest=%016" PRIx64 "\n", n, cfg.norm_obs, cfg.norm_reward, v.stats[20], h);
    }
  }
  return 0;
}
