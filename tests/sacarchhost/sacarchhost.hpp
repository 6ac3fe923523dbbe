// Host build of SAC's kernel source for an ARCHITECTURE (balance_robot_mujoco_rl_amd/csrc/brs_sac.hpp: ArchReference,
// ArchSacDefault): the act, the target and the actor's chain as plain row loops (forward_row_keep / backward_row of brs_ddpg_learner.hpp),
// templates over the actor and the critic of the architecture, around the per-row functions the kernels call -- clamp and gate, sample,
// logp, the two dz3 formulas, min-select, combine, shares -- and the critic gradient with the 0.5 at the loss head, behind the argument
// rules of the C ABI (include/brs_policy.h: brs_sac_*).  tests/sachost is Host<ArchReference> of this file.  Shared by sacarchhost.cpp (a library for tests/test_sac_arch_cpu.py) and sacarchhost_main.cpp (a
// program of its own, for the sanitizers).  SACARCH names the architecture of a build: -DSACARCH=ArchSacDefault (the default) or
// ArchReference.
#pragma once
#include <stddef.h>
#include <string.h>

#include <vector>

#include "../ddpglearnerhost/ddpglearnerhost.hpp"
#include "brs_sac.hpp"

#ifndef SACARCH
#define SACARCH ArchSacDefault
#endif

namespace sacarchhost {

using namespace brs::sac;

template <class A> struct Host {
  using Arch = A;
  using Pi = typename A::Pi;
  using Qf = typename A::Qf;
  static constexpr int NA = nparam<Pi>(), NC = nparam<Qf>(), NA1 = NA + 1, ROW_LEN = NA + SAC_TAIL, TWIN_LEN = 2 * NC + BRS_TD3_NSTAT;

  static int act(const float* actor, int n, const float* obs, uint64_t seed, int64_t base, uint32_t step, int deterministic, int random,
                 float* action, float* mu, float* log_std, float* z) {
    if (sac_act_argument_error(actor, n, obs, random, action)) return BRS_ERR_ARG;
    for (int i = 0; i < n; i++) {
      float out[Pi::OUT] = {0.0f, 0.0f, 0.0f, 0.0f}, a[ACT], m[ACT], ls[ACT], zz[ACT];
      if (!random) forward_row<Pi>(actor, obs + (size_t)OBS * i, out);
      sac_act_tail(seed, base + i, step, deterministic, random, out, a, m, ls, zz);
      for (int k = 0; k < ACT; k++) {
        action[(size_t)ACT * i + k] = a[k];
        if (mu) mu[(size_t)ACT * i + k] = m[k];
        if (log_std) log_std[(size_t)ACT * i + k] = ls[k];
        if (z) z[(size_t)ACT * i + k] = zz[k];
      }
    }
    return BRS_OK;
  }

  static int q(const float* critic, int n, const float* obs, const float* act_, float* out) {
    if (!critic || !obs || !act_ || !out || n < 1) return BRS_ERR_ARG;
    for (int i = 0; i < n; i++) {
      float x[Qf::IN];
      memcpy(x, obs + (size_t)OBS * i, OBS * sizeof(float));
      memcpy(x + OBS, act_ + (size_t)ACT * i, ACT * sizeof(float));
      forward_row<Qf>(critic, x, out + i);
    }
    return BRS_OK;
  }

  static int target(const float* actor, const float* critics_t, int m, const float* next_obs, const float* reward, const uint8_t* done, float gamma,
                    uint64_t seed, uint32_t draw, float* y, float* next_action, float* logp, float* z) {
    if (sac_target_argument_error(actor, critics_t, m, next_obs, reward, done, gamma, y)) return BRS_ERR_ARG;
    const float alpha = ent_coef_of<Pi>(actor);
    for (int i = 0; i < m; i++) {
      float x[OBS + ACT], out[Pi::OUT], zz[ACT], q0, q1;
      uint32_t o[4];
      memcpy(x, next_obs + (size_t)OBS * i, OBS * sizeof(float));
      forward_row<Pi>(actor, x, out);
      sac_row_block(BRS_SAC_TAG_TARGET, seed, draw, (uint32_t)i, o);
      normal_pair(o[0], o[1], zz);
      Sample s;
      sample(out, zz, s);
      for (int k = 0; k < ACT; k++) x[OBS + k] = s.a[k];
      forward_row<Qf>(critics_t, x, &q0);
      forward_row<Qf>(critics_t + NC, x, &q1);
      y[i] = sac_combine(reward[i], done[i], gamma, q0, q1, alpha, s.logp);
      if (logp) logp[i] = s.logp;
      for (int k = 0; k < ACT; k++) {
        if (next_action) next_action[(size_t)ACT * i + k] = s.a[k];
        if (z) z[(size_t)ACT * i + k] = zz[k];
      }
    }
    return BRS_OK;
  }

  // grad[2 NC + 4]: the twin gradient with loss_scale at the head (1: TD3's; 0.5: SAC's)
  static int twin_critic_grad(const float* critics, int m, const float* obs, const float* act_, const float* y, float loss_scale, float* grad) {
    if (sac_critic_grad_argument_error(critics, m, obs, act_, y, grad)) return BRS_ERR_ARG;
    twin_critic_grad_host<Qf>(critics, m, obs, act_, y, loss_scale, grad);
    return BRS_OK;
  }

  // grad[NA + 1 + SAC_NSTAT]; dz3 (may be null) receives the rows' dz3 [m][4], what the kernels pass between their two launches
  static int actor_grad(const float* actor, const float* critics, int m, const float* obs, uint64_t seed, uint32_t draw, int learn_alpha,
                        float target_entropy, float* grad, float* dz3_out) {
    if (sac_actor_grad_argument_error(actor, critics, m, obs, target_entropy, grad)) return BRS_ERR_ARG;
    std::vector<double> g((size_t)ROW_LEN, 0.0);
    const float inv_m = 1.0f / (float)m, alpha = ent_coef_of<Pi>(actor), alpha_m = alpha * inv_m;
    RowTape<Pi> ta;
    RowTape<Qf> tc0, tc1;
    for (int i = 0; i < m; i++) {
      float x[Qf::IN], z[ACT], dx0[Qf::IN], dx1[Qf::IN], dz3[Pi::OUT], share[SAC_TAIL];
      uint32_t o[4];
      for (int k = 0; k < OBS; k++) x[k] = obs[(size_t)OBS * i + k];
      forward_row_keep<Pi>(actor, x, ta);
      sac_row_block(BRS_SAC_TAG_PI, seed, draw, (uint32_t)i, o);
      normal_pair(o[0], o[1], z);
      Sample s;
      sample(ta.pre, z, s);
      for (int k = 0; k < ACT; k++) x[OBS + k] = s.a[k];
      forward_row_keep<Qf>(critics, x, tc0);
      forward_row_keep<Qf>(critics + NC, x, tc1);
      const int sel = min_select(tc0.pre[0], tc1.pre[0]);
      const float dq0 = sel == 0 ? actor_dq(inv_m) : 0.0f, dq1 = sel == 1 ? actor_dq(inv_m) : 0.0f;
      backward_row<Qf>(critics + NC, tc1, &dq1, nullptr, dx1);
      backward_row<Qf>(critics, tc0, &dq0, nullptr, dx0);
      for (int k = 0; k < ACT; k++) {
        const float du = sac_du(dx1[OBS + k] + dx0[OBS + k], s.a[k], s.g[k], alpha_m);
        dz3[k] = du;
        dz3[ACT + k] = sac_dlog_std(du, s.sigma[k], z[k], alpha_m, ta.pre[ACT + k]);
      }
      if (dz3_out) memcpy(dz3_out + (size_t)Pi::OUT * i, dz3, sizeof dz3);
      backward_row<Pi>(actor, ta, dz3, g.data(), nullptr);
      sac_shares(learn_alpha, target_entropy, alpha, s.logp, sel ? tc1.pre[0] : tc0.pre[0], inv_m, share);
      for (int k = 0; k < SAC_TAIL; k++) g[NA + k] += (double)share[k];
    }
    for (int j = 0; j < ROW_LEN; j++) grad[j] = (float)g[j];
    return BRS_OK;
  }

  // one update of SAC.train on host arrays: the critic gradient with its 0.5 (for a y from the critics' targets and the CURRENT actor),
  // one Adam with Polyak over both critics, the actor's gradient through the UPDATED critics, one Adam over the actor and the temperature
  struct State {
    std::vector<float> actor, critics, critics_t, ma, va, mc, vc, ga, gc;
    int64_t steps = 0;
    State(const float* a, const float* c)
        : actor(a, a + NA1), critics(c, c + 2 * NC), critics_t(critics), ma(actor.size(), 0.0f), va(actor.size(), 0.0f), mc(critics.size(), 0.0f),
          vc(critics.size(), 0.0f), ga((size_t)ROW_LEN, 0.0f), gc((size_t)TWIN_LEN, 0.0f) {}
  };
  static int step(State& s, int m, const float* obs, const float* act_, const float* y, uint64_t seed, uint32_t draw, int learn_alpha,
                  float target_entropy, const brs_adam_config* cfg, float tau) {
    ++s.steps;
    if (twin_critic_grad(s.critics.data(), m, obs, act_, y, 0.5f, s.gc.data()) != BRS_OK) return BRS_ERR_ARG;
    if (ddpglearnerhost::apply(2 * NC, s.critics.data(), s.gc.data(), s.mc.data(), s.vc.data(), s.critics_t.data(), cfg, s.steps, tau) != BRS_OK)
      return BRS_ERR_ARG;
    if (actor_grad(s.actor.data(), s.critics.data(), m, obs, seed, draw, learn_alpha, target_entropy, s.ga.data(), nullptr) != BRS_OK)
      return BRS_ERR_ARG;
    if (ddpglearnerhost::apply(NA1, s.actor.data(), s.ga.data(), s.ma.data(), s.va.data(), nullptr, cfg, s.steps, tau) != BRS_OK) return BRS_ERR_ARG;
    return BRS_OK;
  }
};

using H = Host<SACARCH>;

}  // namespace sacarchhost
