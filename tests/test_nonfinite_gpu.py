"""The NaN rule of the float actors, critics and learners on the device: the cases of tests/nonfinite_cases.py
through the Python classes over the C ABI (brs_ddpg_act, brs_ddpg_q, brs_ddpg_td_target, brs_td3_td_target, brs_sac_act,
brs_sac_td_target; the five off-policy gradient calls, brs_learner_grad, brs_a2c_grad), every output between guard zones that must
stay untouched, the off-policy learner handles filled with NaN before their first call; and the collector end to end with an actor
whose b3[0] is NaN: the simulator's bad-state guard of DESIGN.md 3.2 must see every action."""
import numpy as np
import pytest

import ddpg_learner_cases as DC
import nonfinite_cases as NF
import offpolicy_cases as OC
import ref_learner as PL
import sac_cases as SC
from test_ddpg_learner_gpu import _poison
from test_offpolicy_gpu import Guarded, _cuda

pytestmark = pytest.mark.gpu
SEED = NF.SEED
MAX_BATCH = 1024   # the handles' rows are longer than the padded batch at both sizes (ld != mp)


def _back(*guards):
    import torch
    torch.cuda.synchronize()
    assert all(g.intact() for g in guards), "a kernel wrote outside its output"
    out = tuple(g.np() for g in guards)
    return out if len(out) > 1 else out[0]


class DeviceRun:
    """the HIP kernels behind the surface the cases call"""

    def __init__(self):
        from balance_robot_mujoco_rl_amd import DeviceDDPGLearner, DeviceDDPGNets, DeviceSACLearner, DeviceSACNets, DeviceTD3Learner
        self.nets, self.sacnets = DeviceDDPGNets(device=0, seed=SEED), DeviceSACNets(device=0, seed=SEED)
        self.ddpg, self.td3 = DeviceDDPGLearner(device=0, max_batch=MAX_BATCH, **DC.ADAM), DeviceTD3Learner(device=0, max_batch=MAX_BATCH, **DC.ADAM)
        self.sac = DeviceSACLearner(device=0, max_batch=MAX_BATCH, seed=SEED, **{**SC.SAC_ADAM, "target_entropy": SC.TARGET_ENTROPY})
        for lrn in (self.ddpg, self.td3, self.sac):
            _poison(lrn)

    def close(self):
        for x in (self.nets, self.sacnets, self.ddpg, self.td3, self.sac):
            x.close()

    def act(self, actor, obs, step, sigma):
        n = len(obs)
        a, m, z = Guarded((n, 2)), Guarded((n, 2)), Guarded((n, 2))
        self.nets.act(_cuda(actor), _cuda(obs), step, sigma, out=a.t, mean=m.t, noise=z.t)
        return _back(a, m, z)

    def q(self, critic, obs, act):
        q = Guarded((len(obs),))
        self.nets.q(_cuda(critic), _cuda(obs), _cuda(act), out=q.t)
        return _back(q)

    def td_target(self, actor_t, critic_t, next_obs, reward, done, gamma):
        y = Guarded((len(next_obs),))
        self.nets.td_target(_cuda(actor_t), _cuda(critic_t), _cuda(next_obs), _cuda(reward), _cuda(done), gamma, out=y.t)
        return _back(y)

    def td3_target(self, actor_t, critics_t, next_obs, reward, done, gamma, policy_noise, noise_clip, draw):
        m = len(next_obs)
        y, a, z = Guarded((m,)), Guarded((m, 2)), Guarded((m, 2))
        self.nets.td3_target(_cuda(actor_t), _cuda(critics_t), _cuda(next_obs), _cuda(reward), _cuda(done), gamma, policy_noise, noise_clip, draw,
                             out=y.t, next_action=a.t, noise=z.t)
        return _back(y, a, z)

    def sac_act(self, actor, obs, step, deterministic):
        n = len(obs)
        a, mu, ls, z = (Guarded((n, 2)) for _ in range(4))
        self.sacnets.act(_cuda(actor), _cuda(obs), step, deterministic=deterministic, out=a.t, mean=mu.t, log_std=ls.t, noise=z.t)
        return _back(a, mu, ls, z)

    def sac_target(self, actor, critics_t, next_obs, reward, done, gamma, draw):
        m = len(next_obs)
        y, a, lp, z = Guarded((m,)), Guarded((m, 2)), Guarded((m,)), Guarded((m, 2))
        self.sacnets.sac_target(_cuda(actor), _cuda(critics_t), _cuda(next_obs), _cuda(reward), _cuda(done), gamma, draw, out=y.t, next_action=a.t,
                                logp=lp.t, noise=z.t)
        return _back(y, a, lp, z)

    def critic_grad(self, critic, obs, act, y):
        g = Guarded((NF.NC + 2,))
        self.ddpg.critic_grad(_cuda(critic), _cuda(obs), _cuda(act), _cuda(y), out=g.t)
        return _back(g)

    def actor_grad(self, actor, critic, obs):
        g = Guarded((NF.NA + 2,))
        self.ddpg.actor_grad(_cuda(actor), _cuda(critic), _cuda(obs), out=g.t)
        return _back(g)

    def twin_critic_grad(self, critics, obs, act, y):
        g = Guarded((2 * NF.NC + 4,))
        self.td3.twin_critic_grad(_cuda(critics), _cuda(obs), _cuda(act), _cuda(y), out=g.t)
        return _back(g)

    def sac_twin_critic_grad(self, critics, obs, act, y):
        g = Guarded((2 * NF.NC + 4,))
        self.sac.twin_critic_grad(_cuda(critics), _cuda(obs), _cuda(act), _cuda(y), out=g.t)
        return _back(g)

    def sac_actor_grad(self, actor, critics, obs, draw):
        g = Guarded((NF.SNA + 1 + 4,))
        self.sac.actor_grad(_cuda(actor), _cuda(critics), _cuda(obs), draw, out=g.t)
        return _back(g)

    def ppo_grad(self, case, idx, cfg, max_workgroups):
        from test_learner_gpu import KEYS, _learner
        lrn, g = _learner(cfg, case["params"], max_workgroups), Guarded((PL.NPARAM + PL.NSTAT,))
        lrn.grad(*[_cuda(case[k]) for k in KEYS], _cuda(np.asarray(idx, np.int32)), out=g.t)
        out = _back(g)
        lrn.close()
        return out

    def a2c_grad(self, case, idx, cfg, max_workgroups):
        import ref_a2c as A
        from test_a2c_gpu import _learner
        lrn, g = _learner(cfg, case["params"], max_workgroups), Guarded((PL.NPARAM + PL.NSTAT,))
        lrn.grad(*[_cuda(case[k]) for k in A.KEYS], _cuda(np.asarray(idx, np.int32)), out=g.t)
        out = _back(g)
        lrn.close()
        return out


@pytest.fixture(scope="module")
def run():
    r = DeviceRun()
    yield r
    r.close()


# --------------------------------------------------------------------------------------- 1. the forwards
@pytest.mark.parametrize("rotation", NF.ROTATIONS)
def test_kernel_ddpg_rows(run, rotation):
    NF.ddpg_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.ddpg_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)


def test_kernel_ddpg_target_reward_and_done(run):
    NF.ddpg_target_table(run, NF.FORWARD_N, NF.FORWARD_ROWS)


@pytest.mark.parametrize("rotation", NF.ROTATIONS)
def test_kernel_td3_rows(run, rotation):
    NF.td3_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.td3_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)


@pytest.mark.parametrize("rotation", NF.ROTATIONS)
def test_kernel_sac_rows(run, rotation):
    NF.sac_act_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.sac_act_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)
    NF.sac_target_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.sac_target_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)


@pytest.mark.parametrize("sigma", NF.SIGMAS, ids=("sigma0", "sigma0.1"))
@pytest.mark.parametrize("value", NF.WEIGHT_VALUES, ids=("nan", "inf", "-inf"))
def test_kernel_ddpg_actor_bias(run, value, sigma):
    NF.ddpg_actor_bias(run, value, sigma)


@pytest.mark.parametrize("det", (False, True), ids=("sampled", "deterministic"))
@pytest.mark.parametrize("value", NF.WEIGHT_VALUES, ids=("nan", "inf", "-inf"))
@pytest.mark.parametrize("which", (0, 2), ids=("mu_bias", "log_std_bias"))
def test_kernel_sac_actor_bias(run, which, value, det):
    NF.sac_actor_bias(run, which, value, det)


def test_kernel_target_critic_bias_and_temperature(run):
    NF.target_critic_bias(run)


# --------------------------------------------------------------------------------------- 2. the gradients
@pytest.mark.parametrize("m", NF.OFFPOLICY_GRAD_M)
def test_kernel_offpolicy_gradients(run, m):
    NF.offpolicy_gradients(run, m)


@pytest.mark.parametrize("algo", ("ppo", "a2c"))
def test_kernel_onpolicy_gradients(run, algo):
    NF.onpolicy_gradients(run, algo)


# --------------------------------------------------------------------------------------- 3. end to end
@pytest.mark.parametrize("family", ("ddpg", "sac"))
def test_collector_with_a_nan_actor_trips_the_bad_state_guard(family):
    """64 Env01-v1 envs, an actor whose b3[0] is NaN, three collected steps: every env is reset by the guard in every step
    (aux[:, 7] == 3), the stored action's first component is the NaN the actor produced, and every observation and reward in the
    buffer is finite"""
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGNets, DeviceOffPolicyCollector, DeviceReplayBuffer, DeviceSACNets
    n, steps = 64, 3
    if family == "ddpg":
        nets, actor = DeviceDDPGNets(device=0, seed=SEED), OC.weights("init")[0].copy()
        actor[NF.NA - 2] = NF.NAN
    else:
        nets, actor = DeviceSACNets(device=0, seed=SEED), SC.weights("init")[0].copy()
        actor[NF.SNA - 4] = NF.NAN
    sim = BatchedSim("Env01-v1", n, seed=3, auto_reset=True)
    replay = DeviceReplayBuffer(n, 4, device=0, seed=SEED)
    DeviceOffPolicyCollector(sim, nets, _cuda(actor), replay, sigma=0.1).collect(steps)
    torch.cuda.synchronize()
    aux = np.asarray(sim.get_aux())
    assert aux.shape[0] == n and np.all(aux[:, 7] == steps), aux[:, 7]
    action = replay.action[:steps].cpu().numpy()
    assert np.isnan(action[:, :, 0]).all() and np.isfinite(action[:, :, 1]).all()
    for t in (replay.obs, replay.next_obs, replay.reward):
        assert torch.isfinite(t[:steps]).all()
    assert replay.pos == steps and not replay.full
    sim.close(); nets.close()
