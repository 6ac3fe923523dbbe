"""The PPO rollout kernels' yardstick and cases without a GPU (tests/ref_policy.py, tests/policy_cases.py): the fp64 restatement against
torch.nn modules and torch.distributions in fp64, its noise against the Philox known answer of tests/test_policy_kernels.py, every
admission condition of every case tests/test_policy_kernels_gpu.py uses, and every check of that file run on the fp32 numpy restatement
of the kernels' arithmetic (policy_cases.act32 / bootstrap32 / gae32): a check that plain fp32 cannot pass would not tell a kernel bug
from rounding.

Largest distances the fp32 numpy restatement reaches here, next to each bound:
  forward cases (bound: a third of the gate, 3.3e-6): init 1.9e-7, x3 8.4e-7; no row had to be redrawn
  GAE cases (bound: half the gate, 5e-6): 1.5e-6 (T = 37 and the two T = 32 cases); every case was admitted at the first draw
  act outputs, gate 1e-5: noise 1.4e-6, mean 8.4e-7, action and clipped action 7.1e-7, value 6.9e-7, logp 1.2e-7 (all but noise and logp
    on x3; on init they stay below 2.0e-7)
  bootstrap 4.4e-7; the logp contract 1.9e-7, of which the reference alone (the action stored in fp32) 6.2e-8 (bound 3.3e-6)"""
import math

import numpy as np
import pytest
import torch

import policy_cases as PC
import ref_learner as RL
import ref_policy as P
from offpolicy_cases import GATE, gate
from test_policy_kernels import _ref_gae


def _modules(seed=0):
    torch.manual_seed(seed)
    lin, seq, tanh = torch.nn.Linear, torch.nn.Sequential, torch.nn.Tanh
    pi, vf = seq(lin(6, 64), tanh(), lin(64, 64), tanh()), seq(lin(6, 64), tanh(), lin(64, 64), tanh())
    an, vn = lin(64, 2), lin(64, 1)
    log_std = torch.tensor(PC.LOG_STD)
    sd = {"mlp_extractor.policy_net.0.weight": pi[0].weight, "mlp_extractor.policy_net.0.bias": pi[0].bias,
          "mlp_extractor.policy_net.2.weight": pi[2].weight, "mlp_extractor.policy_net.2.bias": pi[2].bias,
          "action_net.weight": an.weight, "action_net.bias": an.bias,
          "mlp_extractor.value_net.0.weight": vf[0].weight, "mlp_extractor.value_net.0.bias": vf[0].bias,
          "mlp_extractor.value_net.2.weight": vf[2].weight, "mlp_extractor.value_net.2.bias": vf[2].bias,
          "value_net.weight": vn.weight, "value_net.bias": vn.bias, "log_std": log_std}
    return sd, (lambda o: an.double()(pi.double()(o))), (lambda o: vn.double()(vf.double()(o)).squeeze(1))


# --------------------------------------------------------------------------------------- 1. the reference itself
def test_reference_forward_and_logp_equal_torch_modules_in_fp64():
    """a layout slip in the reference would show here: the flat vector goes through flatten_sb3_state_dict, the modules keep torch's
    own layout"""
    from balance_robot_mujoco_rl_amd.policy import flatten_sb3_state_dict
    sd, mean_of, value_of = _modules()
    flat = flatten_sb3_state_dict(sd)          # float32, before the modules are widened (the values are the same)
    case = PC.forward_case(257, "init")["obs"]
    obs = np.concatenate([case[7:40], case[:1]])   # 33 ordinary rows and a saturated one (row 0)
    with torch.no_grad():
        mean, value = mean_of(torch.from_numpy(obs).double()).numpy(), value_of(torch.from_numpy(obs).double()).numpy()
    m, v = P.forward(flat, obs)
    assert np.abs(m - mean).max() <= 1e-12 and np.abs(v - value).max() <= 1e-12
    z = np.random.default_rng(0).standard_normal((len(obs), 2))
    ls = P.log_std_of(flat)
    action, clipped, logp = P.act_from(m, ls, z)
    dist = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(np.exp(ls)).expand(len(obs), 2))
    want = dist.log_prob(torch.from_numpy(action)).sum(-1).numpy()
    assert np.abs(logp - want).max() <= 1e-12 and np.abs(P.logp_of_action(m, ls, action) - want).max() <= 1e-12
    assert np.array_equal(clipped, np.clip(action, -1, 1)) and (np.abs(action) > 1).any()
    a_det, _, lp_det, v_det, z_det = P.act(flat, obs, 1, 0, 0, deterministic=True)
    assert np.array_equal(a_det, m) and not z_det.any() and np.allclose(lp_det, -ls.sum() - math.log(2 * math.pi), rtol=0, atol=1e-14)


def test_reference_noise_known_answer_split_and_the_high_word():
    from oracle import oracle as O
    o = O.philox([3, 0x504f4c49, 1000, 0], [5, 0])   # the known answer of tests/test_policy_kernels.py: seed 5, step 3, gid 1000
    u1, u2 = ((o[0] >> 8) + 0.5) / 16777216.0, ((o[1] >> 8) + 0.5) / 16777216.0
    r = math.sqrt(-2 * math.log(u1))
    assert np.array_equal(P.noise(5, 1000, 3, 1)[0], [r * math.cos(2 * math.pi * u2), r * math.sin(2 * math.pi * u2)])
    assert np.array_equal(P.words(5, [1000], 3)[0], np.array(o, np.uint32))
    base, n = 2 ** 32 - 33, 65                       # gid_hi goes from 0 to 1 between rows 32 and 33
    z = P.noise(5, base, 3, n)
    for k in range(n + 1):                           # unchanged when the batch is split at any base
        assert np.array_equal(np.concatenate([P.noise(5, base, 3, k).reshape(k, 2), P.noise(5, base + k, 3, n - k).reshape(n - k, 2)]), z)
    assert len({tuple(row) for row in z}) == n       # the rows on either side of 2^32 differ from each other ...
    low = P.noise(5, 0, 3, 32)                       # ... and gid = 2^32 + i is not gid = i
    assert not (z[33:] == low).any()
    assert not (P.noise(5, 2 ** 40 + 7, 3, 8) == P.noise(5, 7, 3, 8)).any()
    assert not (P.noise(2 ** 63 + 12345, 0, 3, 8) == P.noise(12345, 0, 3, 8)).any()        # the key's high word
    assert not (P.noise(5, 0, 2 ** 32 - 1, 8) == P.noise(5, 0, 2 ** 31 - 1, 8)).any()      # the step's high bit
    assert np.array_equal(P.noise(5, 0, 2 ** 32 + 3, 4), P.noise(5, 0, 3, 4))              # the step is a 32-bit word
    big = P.noise(5, 0, 0, 4096)
    assert abs(big.mean()) < 0.05 and abs(big.std() - 1) < 0.05 and abs(np.corrcoef(big[:, 0], big[:, 1])[0, 1]) < 0.05


def test_reference_bootstrap_and_gae_on_hand_cases():
    """the hand case of tests/test_policy_kernels.py (gamma = 0.5, lambda = 1) through ref_policy.gae with flags of 1, 2 and 255, and
    one row of every flag combination through ref_policy.bootstrap"""
    rew, val = np.ones((3, 2), np.float32), np.zeros((3, 2), np.float32)
    start = np.array([[1, 1], [0, 0], [0, 255]], np.uint8)
    adv, ret = P.gae(rew, val, start, np.array([4, 4], np.float32), np.array([0, 2], np.uint8), 0.5, 1.0)
    assert adv.dtype == np.float64
    np.testing.assert_allclose(adv[:, 0], [1 + 0.5 * (1 + 0.5 * (1 + 0.5 * 4)), 1 + 0.5 * (1 + 0.5 * 4), 1 + 0.5 * 4], rtol=0, atol=1e-15)
    np.testing.assert_allclose(adv[:, 1], [1 + 0.5 * 1, 1, 1], rtol=0, atol=1e-15)
    assert np.array_equal(ret, adv + val)
    assert np.array_equal(adv, _ref_gae(rew, val, (start != 0).astype(np.uint8), np.array([4, 4], np.float32), np.array([0, 1], np.uint8), 0.5, 1.0,
                                        dtype=np.float64)[0])
    c = PC.forward_case(33, "init")
    tobs = np.full((4, 6), np.nan, np.float32)
    tobs[1] = c["obs"][3]
    term, trunc = np.array([0, 0, 1, 2], np.uint8), np.array([0, 255, 0, 1], np.uint8)   # only row 1 is a time limit
    reward = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    out = P.bootstrap(c["params"], tobs, term, trunc, 0.9, reward)
    assert np.array_equal(out[[0, 2, 3]], [1.0, 3.0, 4.0]) and out[1] == 2.0 + 0.9 * c["value"][3] and c["value"][3] != 0.0
    assert np.array_equal(P.bootstrapped(term, trunc), [False, True, False, False])


# --------------------------------------------------------------------------------------- 2. the admission conditions
def test_every_forward_case_is_admitted_and_carries_its_saturated_rows():
    worst = {}
    for kind in PC.WEIGHT_SETS:
        for n in PC.ROWS:
            c = PC.forward_case(n, kind)
            print(f"forward case n={n} {kind}: restatement {c['restatement']:.3g} (bound {GATE / 3:.3g}), {len(c['saturated'])} saturated rows, "
                  f"{c['redrawn']} rows redrawn")
            assert c["restatement"] <= GATE / 3
            assert len(c["saturated"]) == (6 if n >= 33 else 0) and len(set(c["saturated"])) == len(c["saturated"])
            for j, row in enumerate(c["saturated"]):
                want = np.float32(1e30 if j % 2 == 0 else -1e30)
                assert c["obs"][row, j] == want and (np.abs(np.delete(c["obs"][row], j)) < 50).all()
                # layer 1 of both towers is exactly +-1 in fp64, with the sign of the weight (times the feature's)
                flat = torch.from_numpy(c["params"].astype(np.float64))
                Pm = RL.unflatten(flat)
                for t in ("pi", "vf"):
                    h = torch.tanh(torch.from_numpy(c["obs"][row].astype(np.float64)) @ Pm[t + ".W1"].T + Pm[t + ".b1"]).numpy()
                    assert np.array_equal(h, np.sign(Pm[t + ".W1"][:, j].numpy()) * np.sign(float(want)))
            assert np.isfinite(c["mean"]).all() and np.isfinite(c["value"]).all()
            worst[kind] = max(worst.get(kind, 0.0), c["restatement"])
    print(f"largest restatement distance over the forward cases: {worst}")
    assert PC.saturated_rows(513) == [0, 102, 204, 307, 409, 512]


def test_every_gae_case_is_admitted():
    for case in PC.GAE_CASES:
        c = PC.gae_case(*case)
        print(f"GAE case {case}: restatement {c['restatement']:.3g} (bound {GATE / 2:.3g}), admitted at draw {c['attempt']}")
        assert c["restatement"] <= GATE / 2
        flags = set(np.unique(c["episode_start"])) | set(np.unique(c["last_done"]))
        assert flags <= {0, 1, 2, 255} and (case[1] == 1 or case[4] == 0 or {2, 255} <= set(np.unique(c["episode_start"])))
    assert not PC.gae_case(32, 257, 1., 1., 0.)["episode_start"].any()


def test_bootstrap_pattern_table():
    for pattern, n, kind in PC.BOOTSTRAP_CASES:
        c = PC.bootstrap_case(pattern, n, kind)
        rows = c["rows"]
        groups = sorted(set((np.flatnonzero(rows) // 256).tolist()))
        print(f"bootstrap pattern {pattern} n={n} {kind}: {int(rows.sum())} rows bootstrapped, in workgroups {groups}")
        assert np.isnan(c["terminal_obs"][~rows]).all() and np.isfinite(c["terminal_obs"][rows]).all()
        assert np.isfinite(c["want"]).all() and np.array_equal(c["want"][~rows], c["reward"][~rows].astype(np.float64))
        if pattern.startswith("lone"):
            assert np.flatnonzero(rows).tolist() == [int(pattern[4:])]
        elif pattern in ("none", "both"):
            assert not rows.any() and bool(c["truncated"].all()) == (pattern == "both")
        elif pattern == "mixed":
            pairs = set(zip(c["terminated"].tolist(), c["truncated"].tolist()))
            assert len(pairs) == 16 and rows.sum() == (np.asarray(c["truncated"]) != 0)[c["terminated"] == 0].sum() > 64
        else:
            assert rows[0] and (n == 1 or 0 < rows.sum() < n)


def test_the_reference_alone_pays_little_for_the_fp32_action():
    d = PC.reference_alone(PC.contract_case())
    print(f"logp from the fp32-rounded exact action against logp from z, fp64: {d:.3g} (bound {GATE / 3:.3g})")
    assert d <= GATE / 3


# --------------------------------------------------------------------------------------- 3. the GPU file's checks on the restatement
@pytest.mark.parametrize("kind", PC.WEIGHT_SETS)
@pytest.mark.parametrize("n", PC.ROWS)
def test_fp32_restatement_passes_the_act_checks(n, kind):
    c = PC.forward_case(n, kind)
    out = PC.act32(c["params"], c["obs"])
    PC.check_act(c, out, f"restatement n={n} {kind}")
    det0, det7 = (PC.act32(c["params"], c["obs"], step=s, deterministic=True) for s in (0, 7))
    PC.check_deterministic(c, det0, det7, out, f"restatement n={n} {kind}")
    assert PC.act32(c["params"], c["obs"], step=PC.STEP + 1)["noise"].tobytes() != out["noise"].tobytes()


@pytest.mark.parametrize("how", ("nan", "inf"))
@pytest.mark.parametrize("n", PC.ISOLATION_ROWS)
def test_fp32_restatement_passes_the_isolation_checks(n, how):
    c = PC.forward_case(n, "init")
    base = PC.act32(c["params"], c["obs"])
    for row in (0, 31, 32, 63, 64, n - 1):
        PC.check_isolation(c, row, how, base, PC.act32(c["params"], PC.poisoned(c, row, how)), f"restatement n={n} row {row} {how}")


@pytest.mark.parametrize("name", list(PC.COUNTERS))
def test_fp32_restatement_passes_the_counter_checks(name):
    c, k = PC.forward_case(PC.COUNTER_ROWS, "init"), PC.counter_case(name)
    out = PC.act32(c["params"], c["obs"], **k["kw"])
    PC.check_act(c, out, f"restatement {name}", z=k["z"])
    assert not (k["z"] == c["z"]).any()


@pytest.mark.parametrize("pattern,n,kind", PC.BOOTSTRAP_CASES)
def test_fp32_restatement_passes_the_bootstrap_checks(pattern, n, kind):
    c = PC.bootstrap_case(pattern, n, kind)
    out = PC.bootstrap32(c["params"], c["terminal_obs"], c["terminated"], c["truncated"], PC.GAMMA, c["reward"])
    PC.check_bootstrap(c, out, (c["terminal_obs"], c["terminated"], c["truncated"]), f"restatement {pattern} n={n} {kind}")


@pytest.mark.parametrize("case", PC.GAE_CASES)
def test_fp32_restatement_passes_the_gae_checks(case):
    c = PC.gae_case(*case)
    adv, ret = PC.gae32(c)
    PC.check_gae(c, adv, ret, f"restatement {case}")
    flipped = dict(c, episode_start=c["episode_start"].copy())
    flipped["episode_start"][0] = (flipped["episode_start"][0] == 0).astype(np.uint8)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(PC.gae32(flipped), (adv, ret)))   # episode_start[0] is never read, as in SB3


def test_fp32_restatement_passes_the_contract_checks():
    c = PC.contract_case()
    out = PC.act32(c["params"], c["obs"])
    PC.check_contract(c, out, "restatement")
    kl, clipfrac = PC.contract_statistics(c, out["action"], out["logp"])
    print(f"fp64 approx_kl with the restatement's action and logp: {kl:.3g}, clip fraction {clipfrac:.3g}")
    assert clipfrac == 0.0 and abs(kl) <= 1e-8
