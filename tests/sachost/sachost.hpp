// Host build of SAC's kernel source at the reference widths: tests/sacarchhost/sacarchhost.hpp's Host<ArchReference> --
// the act, the target, the two gradients and one update as plain row loops around the per-row functions of brs_sac.hpp -- under the
// names sachost.cpp (a library for tests/test_sac_cpu.py) and sachost_main.cpp (a program of its own, for the sanitizers) call.
#pragma once
#include "../sacarchhost/sacarchhost.hpp"
#include "../td3host/td3host.hpp"  // offpolicyhost::q and ddpglearnerhost::apply, for sachost.cpp

namespace sachost {

using H = sacarchhost::Host<brs::sac::ArchReference>;
using State = H::State;
constexpr int NC = H::NC, NA1 = H::NA1;
inline constexpr auto sac_act_host = H::act;
inline constexpr auto sac_target_host = H::target;
inline constexpr auto twin_critic_grad = H::twin_critic_grad;
inline constexpr auto sac_actor_grad_host = H::actor_grad;
inline constexpr auto step = H::step;

}  // namespace sachost
