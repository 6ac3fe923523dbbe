// How conservative is the cost class (balance_robot_mujoco_rl_amd/csrc/brs_state.hpp: cost_class)?  Host build of the kernel
// source, fp32, -DBRS_STATS (tests/test_lane_map_ref_cpu.py compiles and runs it).  Reads populations from stdin:
//     variant n steps max_episode_steps substeps timestep seed auto_reset planted
//     planted ? n rows of 16 qpos and 14 qvel : nothing
//     steps * n * 2 actions
// until the input ends, and steps them.  For every lane-step it takes the key of the state the step starts from and whether
// the step walked, in any substep, the path a clear wheel bit / floor bit or a set far bit rules out: a block<->floor contact
// row, the wheel narrow phase, the torso narrow phase.  Output, one line per key and one per bit:
//     key K lane_steps
//     bit NAME ruled_out walked allowed walked_where_allowed
// (the last two show that the path's counter is live: lane-steps whose key allowed the path, and those of them that walked it)
#include <cstdio>
#include <vector>

#include "brs_state.hpp"

using namespace brs;
using R = float;
using L = Layout<true>;

int main() {
  long per_key[8] = {0}, ruled[3] = {0}, walked[3] = {0}, allowed[3] = {0}, walked_allowed[3] = {0};
  int variant, n, steps, max_steps, nsub, auto_reset, planted;
  double h;
  unsigned long long seed;
  while (scanf("%d %d %d %d %d %lf %llu %d %d", &variant, &n, &steps, &max_steps, &nsub, &h, &seed, &auto_reset, &planted) == 9) {
    const size_t N = (size_t)n;
    const Params<R> P = make_params<R>(variant, auto_reset, -1, max_steps, nsub, h, seed, 0);
    std::vector<double> d(L::ND * N);
    std::vector<R> f(L::NF * N);
    std::vector<int> ii(L::NI * N);
    hostconv::init_state<true>(d.data(), f.data(), ii.data(), N, seed, 0);
    float obs[6];
    for (size_t i = 0; i < N; i++) {
      EnvState<R, true> S;
      load_state<R, true>(S, d.data(), f.data(), ii.data(), N, i);
      Stream<R> rng;
      rng.open(P.seed, P.gid_base + (int64_t)i, S.rng_ctr);
      Sim<R, true>::env_reset(P, S, rng, obs);
      S.rng_ctr = rng.ctr;
      store_state<R, true>(S, d.data(), f.data(), ii.data(), N, i);
    }
    if (planted) {
      std::vector<double> qpos(L::NQ * N), qvel(L::NV * N);
      for (double& x : qpos) if (scanf("%lf", &x) != 1) return 2;
      for (double& x : qvel) if (scanf("%lf", &x) != 1) return 2;
      hostconv::set_state<true>(d.data(), f.data(), N, qpos.data(), qvel.data(), nullptr, nullptr);
      hostconv::mark_bad_start<true>(d.data(), f.data(), ii.data(), N);
    }
    std::vector<float> act(2 * N);
    std::vector<int> key(N), walk(N);
    for (int t = 0; t < steps; t++) {
      for (float& a : act) if (scanf("%f", &a) != 1) return 2;
#pragma omp parallel for schedule(dynamic, 4)
      for (size_t i = 0; i < N; i++) {
        EnvState<R, true> S0;
        load_state<R, true>(S0, d.data(), f.data(), ii.data(), N, i);
        key[i] = cost_class<R, true>(P, S0);
        R buf[LDS_WORDS_ENV03];
        Store<R> st{buf, 1};
        Stream<R> rng;
        rng.open(P.seed, P.gid_base + (int64_t)i, 0u);
        int te, tr;
        float o[6], to[6], rw;
        stats() = Stats{};  // (thread-local)
        env_step_mem<R, true, R>(P, st, rng, d.data(), f.data(), ii.data(), N, i, act[2 * i], act[2 * i + 1], o, to, rw, te, tr);
        const Stats& s = stats();
        walk[i] = (s.nfb_hist[1] + s.nfb_hist[2] + s.nfb_hist[3] + s.nfb_hist[4] > 0 ? 1 : 0) | (s.cp_wheel > 0 ? 2 : 0) | (s.cp_torso > 0 ? 4 : 0);
      }
      for (size_t i = 0; i < N; i++) {
        const int out = (key[i] ^ 3) & 7;  // the paths the key rules out: floor and wheel bits clear, far bit set
        per_key[key[i]]++;
        for (int b = 0; b < 3; b++) {
          ruled[b] += (out >> b) & 1; walked[b] += (out & walk[i]) >> b & 1;
          allowed[b] += (~out >> b) & 1; walked_allowed[b] += (~out & walk[i]) >> b & 1;
        }
      }
    }
  }
  const char* name[3] = {"floor", "wheel", "far"};
  for (int k = 0; k < 8; k++) printf("key %d %ld\n", k, per_key[k]);
  for (int b = 0; b < 3; b++) printf("bit %s %ld %ld %ld %ld\n", name[b], ruled[b], walked[b], allowed[b], walked_allowed[b]);
  return 0;
}
