"""The NaN rule of the float actors, critics and learners without a GPU: the cases of tests/nonfinite_cases.py on the
host builds of the kernel source (offpolicyhost, td3host, sachost, ddpglearnerhost, learnerhost, a2chost), which share the per-row
tails, the selects, the gates and the loss heads with the HIP kernels; and the two checks on planted arrays of their own -- a
swallowed NaN, a changed neighbour row and a missing gradient NaN must each fail them."""
import numpy as np
import pytest

import a2c_cases as AC
import ddpg_learner_cases as DC
import learner_cases as LC
import nonfinite_cases as NF
import offpolicy_cases as OC
import sac_cases as SC
import td3_cases as TC

SEED = NF.SEED


class HostRun:
    """the host builds behind the surface the cases call"""

    def __init__(self, directory):
        self.off, self.td3, self.sac = OC.build_host(directory), TC.build_host(directory), SC.build_host(directory)
        self.ddpg, self.ppo, self.a2c = DC.build_host(directory), LC.build_host(directory), AC.build_host(directory)

    def act(self, actor, obs, step, sigma):
        return OC.host_act(self.off, actor, obs, SEED, 0, step, sigma)

    def q(self, critic, obs, act):
        return OC.host_q(self.off, critic, obs, act)

    def td_target(self, actor_t, critic_t, next_obs, reward, done, gamma):
        return OC.host_td_target(self.off, actor_t, critic_t, next_obs, reward, done, gamma)

    def td3_target(self, actor_t, critics_t, next_obs, reward, done, gamma, policy_noise, noise_clip, draw):
        return TC.host_td3_target(self.td3, actor_t, critics_t, next_obs, reward, done, gamma, policy_noise, noise_clip, SEED, draw)

    def sac_act(self, actor, obs, step, deterministic):
        return SC.host_act(self.sac, actor, obs, SEED, 0, step, deterministic=deterministic)

    def sac_target(self, actor, critics_t, next_obs, reward, done, gamma, draw):
        return SC.host_target(self.sac, actor, critics_t, next_obs, reward, done, gamma, SEED, draw)

    def critic_grad(self, critic, obs, act, y):
        return DC.host_critic_grad(self.ddpg, critic, obs, act, y)

    def actor_grad(self, actor, critic, obs):
        return DC.host_actor_grad(self.ddpg, actor, critic, obs)

    def twin_critic_grad(self, critics, obs, act, y):
        return SC.host_twin_critic_grad(self.sac, critics, obs, act, y, loss_scale=1.0)   # TD3's: the same loops with the head's scale at 1

    def sac_twin_critic_grad(self, critics, obs, act, y):
        return SC.host_twin_critic_grad(self.sac, critics, obs, act, y)

    def sac_actor_grad(self, actor, critics, obs, draw):
        return SC.host_actor_grad(self.sac, actor, critics, obs, SEED, draw)

    def ppo_grad(self, case, idx, cfg, max_workgroups):
        h = LC.HostLearner(self.ppo, cfg, case["params"], max_workgroups)
        g = h.grad(case, idx)
        h.close()
        return g

    def a2c_grad(self, case, idx, cfg, max_workgroups):
        h = AC.HostA2C(self.a2c, cfg, case["params"], max_workgroups)
        g = h.grad(case, idx)
        h.close()
        return g


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return HostRun(tmp_path_factory.mktemp("nonfinitehost"))


# --------------------------------------------------------------------------------------- 1. the checks on planted arrays
def test_classes():
    x = np.array([0.0, -1.5, np.nan, np.inf, -np.inf, 3e38], np.float32)
    assert NF.classes(x).tolist() == [NF.FINITE, NF.FINITE, NF.ISNAN, NF.POSINF, NF.NEGINF, NF.FINITE]
    assert NF.classes(x.astype(np.float64).reshape(3, 2)).shape == (3, 2)


def test_forward_check_fails_on_a_swallowed_nan_and_on_a_changed_neighbour():
    clean = np.linspace(-1, 1, 12, dtype=np.float32).reshape(6, 2)
    ref = clean.astype(np.float64)
    ref[2, 0], ref[4, 1] = np.nan, np.inf
    keep = NF.rows_mask(6, (2, 4))
    good = clean.copy()
    good[2, 0], good[4, 1] = np.nan, np.inf
    assert NF.check_forward("planted", good, ref, clean, keep) == 2
    swallowed = good.copy()
    swallowed[2, 0] = -1.0                      # what fminf(1, fmaxf(-1, NaN)) returns
    with pytest.raises(AssertionError, match="another class"):
        NF.check_forward("planted", swallowed, ref, clean, keep)
    wrong_inf = good.copy()
    wrong_inf[4, 1] = -np.inf
    with pytest.raises(AssertionError, match="another class"):
        NF.check_forward("planted", wrong_inf, ref, clean, keep)
    spread = good.copy()
    spread[3, 0] = np.nan                       # a NaN the reference does not report
    with pytest.raises(AssertionError, match="another class"):
        NF.check_forward("planted", spread, ref, clean, keep)
    neighbour = good.copy()
    neighbour[3, 1] = np.nextafter(neighbour[3, 1], np.float32(2))   # one ulp: within the gate, not the clean run's bytes
    with pytest.raises(AssertionError, match="differ from the clean run"):
        NF.check_forward("planted", neighbour, ref, clean, keep)
    off = good.copy()
    off[2, 1] += np.float32(1e-3)               # a finite element of a poisoned row is still held to the gate
    with pytest.raises(AssertionError):
        NF.check_forward("planted", off, ref, clean, keep)
    clean0, ref0, minus_zero = clean.copy(), ref.copy(), good.copy()
    clean0[0, 0], ref0[0, 0], minus_zero[0, 0] = 0.0, 0.0, -0.0
    with pytest.raises(AssertionError, match="differ from the clean run"):   # bytes, not values
        NF.check_forward("planted", minus_zero, ref0, clean0, keep)


def test_gradient_check_fails_on_a_missing_nan_and_counts_the_extra_ones(capsys):
    g64 = np.arange(10, dtype=np.float64)
    g64[[1, 7]] = np.nan
    g = g64.astype(np.float32)
    assert NF.check_gradient_nans("planted", g, g64) == 0
    more = g.copy()
    more[3] = np.nan
    assert NF.check_gradient_nans("planted", more, g64) == 1 and "1 of them where fp64 is finite" in capsys.readouterr().out
    missing = g.copy()
    missing[7] = 0.0                            # a closed gate's exact zero
    with pytest.raises(AssertionError, match="element 7"):
        NF.check_gradient_nans("planted", missing, g64)
    NF.reference_reaches("planted", g64, {"a": slice(0, 3), "b": 7}, ("a", "b"))
    with pytest.raises(AssertionError, match="does not reach c"):
        NF.reference_reaches("planted", g64, {"c": slice(2, 7)}, ("c",))


def test_poison_tables():
    obs = np.zeros((NF.FORWARD_N, 6), np.float32)
    seen = set()
    for rot in NF.ROTATIONS:
        p = NF.poison_obs(obs, NF.FORWARD_ROWS, rot)
        assert (NF.classes(p) != NF.FINITE).sum() == len(NF.FORWARD_ROWS) and not (NF.classes(obs) != NF.FINITE).any()   # a copy, one per row
        for row in NF.FORWARD_ROWS:
            col = int(np.flatnonzero(NF.classes(p[row]))[0])
            seen.add((row, col, int(NF.classes(p[row, col]))))
    assert len(seen) == len(NF.FORWARD_ROWS) * len(NF.OBS_POISONS)   # every row meets every poison
    no, rw, dn, r = NF.reward_and_done_poisons(obs, np.ones(NF.FORWARD_N, np.float32), np.zeros(NF.FORWARD_N, np.uint8), NF.FORWARD_ROWS)
    assert [bool(np.isnan(rw[k])) for k in r] == [True, True, False, False] and dn[r].tolist() == [0, 1, 0, 1]
    assert [bool(np.isnan(no[k, 0])) for k in r] == [False, False, True, True]


# --------------------------------------------------------------------------------------- 2. the forwards on the host builds
@pytest.mark.parametrize("rotation", NF.ROTATIONS)
def test_host_ddpg_rows(run, rotation):
    NF.ddpg_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.ddpg_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)


def test_host_ddpg_target_reward_and_done(run):
    NF.ddpg_target_table(run, NF.FORWARD_N, NF.FORWARD_ROWS)


@pytest.mark.parametrize("rotation", NF.ROTATIONS)
def test_host_td3_rows(run, rotation):
    NF.td3_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.td3_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)


@pytest.mark.parametrize("rotation", NF.ROTATIONS)
def test_host_sac_rows(run, rotation):
    NF.sac_act_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.sac_act_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)
    NF.sac_target_rows(run, NF.FORWARD_N, NF.FORWARD_ROWS, rotation)
    NF.sac_target_rows(run, NF.SMALL_N, NF.SMALL_ROWS, rotation)


@pytest.mark.parametrize("sigma", NF.SIGMAS, ids=("sigma0", "sigma0.1"))
@pytest.mark.parametrize("value", NF.WEIGHT_VALUES, ids=("nan", "inf", "-inf"))
def test_host_ddpg_actor_bias(run, value, sigma):
    NF.ddpg_actor_bias(run, value, sigma)


@pytest.mark.parametrize("det", (False, True), ids=("sampled", "deterministic"))
@pytest.mark.parametrize("value", NF.WEIGHT_VALUES, ids=("nan", "inf", "-inf"))
@pytest.mark.parametrize("which", (0, 2), ids=("mu_bias", "log_std_bias"))
def test_host_sac_actor_bias(run, which, value, det):
    NF.sac_actor_bias(run, which, value, det)


def test_host_target_critic_bias_and_temperature(run):
    NF.target_critic_bias(run)


# --------------------------------------------------------------------------------------- 3. the gradients on the host builds
@pytest.mark.parametrize("m", NF.OFFPOLICY_GRAD_M)
def test_host_offpolicy_gradients(run, m):
    NF.offpolicy_gradients(run, m)


@pytest.mark.parametrize("algo", ("ppo", "a2c"))
def test_host_onpolicy_gradients(run, algo):
    NF.onpolicy_gradients(run, algo)
