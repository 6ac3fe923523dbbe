// Host build of TD3's kernel source: the target through forward_row plus the per-row tail of brs_offpolicy.hpp
// (td3_action_tail, td3_combine), and the twin critic gradient as the host's row loop over both critics (brs_ddpg_learner.hpp), behind
// the argument rules of the C ABI (include/brs_policy.h: brs_td3_td_target, brs_ddpg_learner_twin_critic_grad).  Shared by
// td3host.cpp (a library for tests/test_td3_cpu.py) and td3host_main.cpp (a program of its own, for the sanitizers).
#pragma once
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../ddpglearnerhost/ddpglearnerhost.hpp"
#include "../offpolicyhost/offpolicyhost.hpp"

namespace td3host {

using namespace brs::ddpg_learner;
constexpr int NC = BRS_DDPG_NCRITIC, TWIN_LEN = 2 * NC + BRS_TD3_NSTAT;

inline int td3_target(const float* actor_t, const float* critics_t, int m, const float* next_obs, const float* reward, const uint8_t* done,
                      float gamma, float policy_noise, float noise_clip, uint64_t seed, uint32_t draw, float* y, float* next_action, float* noise) {
  if (td3_target_argument_error(actor_t, critics_t, m, next_obs, reward, done, policy_noise, noise_clip, y)) return BRS_ERR_ARG;
  for (int i = 0; i < m; i++) {
    float x[OBS + ACT], mu[ACT], z[ACT], q1, q2;
    memcpy(x, next_obs + (size_t)OBS * i, OBS * sizeof(float));
    forward_row<Actor>(actor_t, x, mu);
    td3_action_tail(seed, draw, (uint32_t)i, policy_noise, noise_clip, mu, x + OBS, z);
    forward_row<Critic>(critics_t, x, &q1);
    forward_row<Critic>(critics_t + NC, x, &q2);
    y[i] = td3_combine(reward[i], done[i], gamma, q1, q2);
    for (int k = 0; k < ACT; k++) {
      if (next_action) next_action[(size_t)ACT * i + k] = x[OBS + k];
      if (noise) noise[(size_t)ACT * i + k] = z[k];
    }
  }
  return BRS_OK;
}

// grad[2 NC + 4]: block 0, block 1, then (Lc, mean Q) of critic 0 and of critic 1
inline int twin_critic_grad(const float* critics, int m, const float* obs, const float* act, const float* y, float* grad) {
  if (!critics || !obs || !act || !y || !grad || m < 1) return BRS_ERR_ARG;
  twin_critic_grad_host<Critic>(critics, m, obs, act, y, 1.0f, grad);
  return BRS_OK;
}

// one update of TD3.train on host arrays; the caller counts n_updates from 1 and the two Adam steps.  -> 1 if the actor was
// updated, 0 if not, < 0 on a refused argument
struct State {
  std::vector<float> actor, critics, actor_t, critics_t, ma, va, mc, vc, ga, gc;
  int64_t steps_actor = 0, steps_critics = 0, n_updates = 0;
  State(const float* a, const float* c)
      : actor(a, a + BRS_DDPG_NACTOR), critics(c, c + 2 * NC), actor_t(actor), critics_t(critics), ma(actor.size(), 0.0f), va(actor.size(), 0.0f),
        mc(critics.size(), 0.0f), vc(critics.size(), 0.0f), ga(actor.size() + NSTAT, 0.0f), gc((size_t)TWIN_LEN, 0.0f) {}
};
inline int step(State& s, int m, const float* obs, const float* act, const float* y, const brs_adam_config* cfg, float tau, int policy_delay) {
  if (policy_delay < 1) return BRS_ERR_ARG;
  const bool delayed = ++s.n_updates % policy_delay == 0;
  if (twin_critic_grad(s.critics.data(), m, obs, act, y, s.gc.data()) != BRS_OK) return BRS_ERR_ARG;
  if (ddpglearnerhost::apply(2 * NC, s.critics.data(), s.gc.data(), s.mc.data(), s.vc.data(), delayed ? s.critics_t.data() : nullptr, cfg,
                             ++s.steps_critics, tau) != BRS_OK)
    return BRS_ERR_ARG;
  if (!delayed) return 0;
  if (ddpglearnerhost::actor_grad(s.actor.data(), s.critics.data(), m, obs, s.ga.data()) != BRS_OK) return BRS_ERR_ARG;
  if (ddpglearnerhost::apply(BRS_DDPG_NACTOR, s.actor.data(), s.ga.data(), s.ma.data(), s.va.data(), s.actor_t.data(), cfg, ++s.steps_actor, tau) !=
      BRS_OK)
    return BRS_ERR_ARG;
  return 1;
}

}  // namespace td3host
