// A program of its own around the host build of offpolicyhost.hpp, so that it can run under AddressSanitizer and
// UndefinedBehaviorSanitizer without anything being loaded into Python (tests/test_offpolicy_cpu.py builds it twice, plain and
// with -fsanitize=address,undefined, and compares what the two print).
//
//   offpolicyhost_main CASE...   each CASE a file written by the test: int32 n, cap, steps, m; uint64 seed; float sigma, gamma;
//                                actor f32[NACTOR]; critic f32[NCRITIC]; then per step obs, new_obs, terminal_obs f32[n][6],
//                                reward f32[n], terminated, truncated u8[n]
// For every case: per step t act (uniform on odd t) from obs and add at row t % cap; then one sample of m from the filled rows,
// the TD target of the sample (the two networks as their own targets) and Q of the sampled pairs.  One line with FNV-1a digests
// of the storage, the sample and its indices, y and q.  Every array has exactly its size, so an index past an end is seen.
#include <inttypes.h>
#include <stdio.h>

#include <vector>

#include "offpolicyhost.hpp"

namespace {

uint64_t fnv(uint64_t h, const void* data, size_t bytes) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; i++) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
template <class T> uint64_t fnv(uint64_t h, const std::vector<T>& v) { return fnv(h, v.data(), v.size() * sizeof(T)); }

template <class T> bool read(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

struct Storage {
  std::vector<float> obs, next_obs, action, reward;
  std::vector<uint8_t> done;
  explicit Storage(size_t cells) : obs(cells * 6, -7.0f), next_obs(cells * 6, -7.0f), action(cells * 2, -7.0f), reward(cells, -7.0f), done(cells, 9) {}
  brs_replay_storage view() { return brs_replay_storage{obs.data(), next_obs.data(), action.data(), reward.data(), done.data()}; }
  uint64_t digest() const { return fnv(fnv(fnv(fnv(fnv(14695981039346656037ull, obs), next_obs), action), reward), done); }
};

}  // namespace

int main(int argc, char** argv) {
  using namespace offpolicyhost;
  for (int a = 1; a < argc; a++) {
    FILE* f = fopen(argv[a], "rb");
    int32_t head[4];
    uint64_t seed;
    float fl[2];
    if (!f || fread(head, sizeof(int32_t), 4, f) != 4 || fread(&seed, sizeof seed, 1, f) != 1 || fread(fl, sizeof(float), 2, f) != 2 || head[0] < 1 ||
        head[1] < 1 || head[2] < 1 || head[3] < 1) {
      fprintf(stderr, "%s: bad case\n", argv[a]);
      return 2;
    }
    const int n = head[0], cap = head[1], steps = head[2], m = head[3];
    const size_t N = (size_t)n;
    std::vector<float> actor, critic;
    if (!read(f, actor, (size_t)BRS_DDPG_NACTOR) || !read(f, critic, (size_t)BRS_DDPG_NCRITIC)) {
      fprintf(stderr, "%s: short case\n", argv[a]);
      return 2;
    }
    Storage st((size_t)cap * N);
    const brs_replay_storage sv = st.view();
    for (int t = 0; t < steps; t++) {
      std::vector<float> obs, new_obs, tobs, reward, action(N * 2);
      std::vector<uint8_t> term, trunc;
      if (!read(f, obs, N * 6) || !read(f, new_obs, N * 6) || !read(f, tobs, N * 6) || !read(f, reward, N) || !read(f, term, N) || !read(f, trunc, N)) {
        fprintf(stderr, "%s: short case\n", argv[a]);
        return 2;
      }
      if (act(actor.data(), n, obs.data(), seed, 0, (uint32_t)t, fl[0], t & 1, action.data(), nullptr, nullptr) != 0 ||
          replay_add(&sv, n, cap, t % cap, obs.data(), action.data(), new_obs.data(), reward.data(), term.data(), trunc.data(), tobs.data()) != 0) {
        fprintf(stderr, "%s: step %d refused\n", argv[a], t);
        return 2;
      }
    }
    fclose(f);
    Storage out((size_t)m);
    const brs_replay_storage ov = out.view();
    std::vector<int32_t> idx((size_t)m * 2);
    std::vector<float> y((size_t)m), qv((size_t)m);
    if (replay_sample(&sv, n, cap, steps < cap ? steps : cap, m, seed, 0, &ov, idx.data()) != 0 ||
        td_target(actor.data(), critic.data(), m, out.next_obs.data(), out.reward.data(), out.done.data(), fl[1], y.data()) != 0 ||
        q(critic.data(), m, out.obs.data(), out.action.data(), qv.data()) != 0) {
      fprintf(stderr, "%s: sample refused\n", argv[a]);
      return 2;
    }
    printf("n=%d cap=%d steps=%d m=%d storage=%016" PRIx64 " sample=%016" PRIx64 " idx=%016" PRIx64 " y=%016" PRIx64 " q=%016" PRIx64 "\n", n, cap,
           steps, m, st.digest(), out.digest(), fnv(14695981039346656037ull, idx), fnv(14695981039346656037ull, y), fnv(14695981039346656037ull, qv));
  }
  return 0;
}
