"""SAC (include/brs_policy.h: brs_sac_*) without a GPU: the host build of the kernel source (tests/sachost) against the
fp64 restatement (tests/ref_sac.py) on the cases of tests/sac_cases.py; the 0.5 rule of the critic gradient; the fixed temperature; the
exact reductions; a six-step chain; the same host code as a program under the sanitizers; the C ABI's argument checks; the Python
layer; the tool's usage errors and its torch update.

Largest distances reached here by the host build, next to each gate (fp32 torch on the same case in brackets):
  act / target outputs, gate 1e-5: log_std 8.8e-6 (spread, n = 257: the output layer's rows are x 60 and cancel), mu 6.0e-6 (x3), a'
    4.2e-6, action 3.7e-6, y 2.9e-6, z 2.8e-6, logp' 2.8e-6
  actor gradient blocks, gate 1e-5: init 2.2e-7 [fp32 torch 2.4e-7], x3 1.1e-6 [5.0e-3], spread 3.1e-6 [7.4e-2]; statistics 9.2e-7.
    fp32 torch misses the gate on x3 and spread by the way SB3 writes the loss: 1 - tanh(u)^2 cancels where the tanh saturates (the
    kernels take it from the exponential), and Normal.log_prob's (u - mu)^2 / (2 std^2) does not return z^2 / 2 in fp32.  The cases'
    conditions hold on the fp64 reference, and the kernel source meets the gate there: no case was changed for fp32 torch's sake.
  six chained steps: every block at 1.0x fp32 torch's floored distance (gate 4x)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_offpolicy as R
import ref_sac as S
import sac_cases as SC
import td3_cases as TC
from balance_robot_mujoco_rl_amd import _lib, offpolicy
from offpolicy_cases import GAMMA, GXX, ROOT, SEED, gate

ERR_ARG, ERR_HIP = -1, -2
NA, NC = SC.NA, SC.NC


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return SC.build_host(tmp_path_factory.mktemp("sachost"))


# --------------------------------------------------------------------------------------- 1. cases, act, target
def test_the_cases_cover_every_branch():
    tables = SC.assert_branch_coverage()
    assert tables[("gradient", 33)]["log_std_low"] >= 1 and tables[("target", 257)]["saturated"] >= 8
    for kind in SC.WEIGHT_SETS:   # the conditions of a gradient case, read back from what is stored
        c = SC.grad_case(257, kind)
        assert np.abs(c["q"][:, 0] - c["q"][:, 1]).min() >= SC.MARGIN[kind]
        assert min(np.abs(c["raw"] - S.LOG_STD_MIN).min(), np.abs(c["raw"] - S.LOG_STD_MAX).min()) >= SC.MARGIN[kind]
    raw = SC.grad_case(257, "spread")["raw"]
    assert raw.min() < -25 and raw.max() > 7   # well past both clamps


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("n", SC.ACT_ROWS_CPU)
def test_host_act_against_fp64(host, n, kind):
    c = SC.act_case(n, kind)
    a, mu, ls, z = SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0)
    for x, ref, name in zip((a, mu, ls, z), c["act"], ("action", "mu", "log_std", "z")):
        gate(x, ref, f"n={n} {kind} {name}")
    assert np.abs(a).max() <= 1.0 and ls.min() >= S.LOG_STD_MIN and ls.max() <= S.LOG_STD_MAX
    assert SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0, extras=False)[0].tobytes() == a.tobytes()
    # deterministic: tanh(mu), whatever the step
    d0, mu0 = SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0, deterministic=True)[:2]
    d1 = SC.host_act(host, c["actor"], c["obs"], SEED, 0, 5, deterministic=True)[0]
    assert d0.tobytes() == d1.tobytes() and mu0.tobytes() == mu.tobytes()
    gate(d0, c["act_det"][0], f"n={n} {kind} deterministic action"); gate(d0, np.tanh(mu0.astype(np.float64)), "tanh(mu)")
    # warm-up: the uniform of words 2 and 3, no network
    r, rmu, rls, rz = SC.host_act(host, None, None, SEED, 0, 0, random=True, n=n)
    ref = S.act(None, None, SEED, 0, 0, random=True, n=n)
    assert np.array_equal(r.astype(np.float64), ref[0]) and r.tobytes() == rmu.tobytes() and not rls.any() and rz.tobytes() == z.tobytes()
    assert SC.host_act(host, c["actor"], c["obs"], SEED, 0, 1)[3].tobytes() != z.tobytes()   # another step, another z


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("m", SC.ACT_ROWS_CPU)
def test_host_target_against_fp64(host, m, kind):
    c = SC.target_case(m, kind)
    y, a, lp, z = SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 0)
    for x, name in ((z, "z"), (a, "a"), (lp, "logp"), (y, "y")):
        gate(x, c[name], f"m={m} {kind} {name}")
    ended = c["done"] != 0
    assert y[ended].tobytes() == c["reward"][ended].tobytes() and np.abs(a).max() <= 1.0
    assert SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 0, extras=False)[0].tobytes() == y.tobytes()
    assert SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 1)[3].tobytes() != z.tobytes()


def test_target_without_entropy_is_the_td3_formula_on_the_same_action(host):
    """log_ent_coef = -inf (alpha = 0) and a log-std head that sits below the lower clamp: y is td3_combine of the two target Q on the
    a' the call returns, byte for byte, and a' is tanh(mu) to rounding"""
    for m, kind in ((33, "init"), (257, "x3")):
        c = SC.target_case(m, kind)
        actor = c["actor"].copy()
        sl = S.RL.block_slices(S.ACTOR_SIZES)
        actor[sl["W3"]].reshape(4, 200)[2:] = 0.0
        actor[sl["b3"]][2:] = -30.0
        actor[NA] = -np.inf
        y, a, lp, z = SC.host_target(host, actor, c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 0)
        q = [np.zeros(m, np.float32) for _ in (0, 1)]
        for k in (0, 1):
            assert host.sh_q(c["critics"][k * NC:].ctypes.data, m, c["next_obs"].ctypes.data, a.ctypes.data, q[k].ctypes.data) == 0
        ref = np.zeros(m, np.float32)
        assert host.sh_td3_combine(m, c["reward"].ctypes.data, c["done"].ctypes.data, GAMMA, q[0].ctypes.data, q[1].ctypes.data, ref.ctypes.data) == 0
        assert y.tobytes() == ref.tobytes() and np.isfinite(lp).all()
        gate(a, np.tanh(S.heads(actor, c["next_obs"])[0]), "a' with sigma = exp(-20) is tanh(mu)")


# --------------------------------------------------------------------------------------- 2. gradients
@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("n", SC.GRAD_ROWS_CPU)
def test_host_actor_gradient_against_fp64(host, n, kind):
    c = SC.grad_case(n, kind)
    g64, g32 = SC.references(n, kind)
    g = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, c["draw"])
    SC.check_actor_gradient(f"n={n} {kind}", g, g64, g32, gate)
    assert abs(g[NA + 4] - np.exp(np.float64(c["actor"][NA]))) <= 1e-6


@pytest.mark.parametrize("kind", ("init", "x3"))
@pytest.mark.parametrize("n", (1, 33, 257))
def test_half_rule_of_the_critic_gradient_on_the_host_build(host, n, kind):
    """loss_scale = 0.5 is exact: every parameter block and both loss statistics are 0.5 x TD3's bytes wherever TD3's value is at least
    2^-125 in magnitude, the two mean Q are TD3's; and it is SB3's critic loss against fp64"""
    c = TC.twin_case(n, kind)   # conditioned for both critics on (obs, act)
    td3, sac = (SC.host_twin_critic_grad(host, c["critics"], c["obs"], c["act"], c["y"], s) for s in (1.0, 0.5))
    halved = np.concatenate([np.arange(2 * NC), [2 * NC, 2 * NC + 2]])
    big = halved[np.abs(td3[halved]) >= 2.0 ** -125]
    assert (np.float32(0.5) * td3[big]).tobytes() == sac[big].tobytes() and len(big) > 1000   # (n = 1: the closed gates' zeros)
    assert td3[[2 * NC + 1, 2 * NC + 3]].tobytes() == sac[[2 * NC + 1, 2 * NC + 3]].tobytes()
    g64 = S.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"])
    for k in (0, 1):
        d = SC.block_distances(sac[k * NC:(k + 1) * NC], g64[k * NC:(k + 1) * NC], R.CRITIC_SIZES)
        print(f"n={n} {kind} critic {k}: largest block distance from fp64 {max(d.values()):.3g}")
        assert max(d.values()) <= SC.GRAD_GATE
    gate(sac[2 * NC:], g64[2 * NC:], "statistics")


def test_fixed_temperature_gets_a_zero_gradient_and_adam_leaves_it(host):
    c = SC.grad_case(33, "init")
    g = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, 0, learn_alpha=False)
    learned = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, 0, learn_alpha=True)
    assert g[NA] == 0.0 and learned[NA] != 0.0
    assert np.delete(g, NA).tobytes() == np.delete(learned, NA).tobytes()
    g64 = SC.references(33, "init", learn_alpha=False)[0]
    assert g64[NA] == 0.0
    h = SC.HostSAC(host, c["actor"], c["critics"], learn_alpha=False, **SC.SAC_ADAM)
    for s in range(3):
        h.step(c["obs"], c["act"], c["y"], SEED, s)
    assert h.flat["actor"][NA:].tobytes() == c["actor"][NA:].tobytes() and h.mom["actor"][0][NA] == 0.0 and h.mom["actor"][1][NA] == 0.0
    assert not np.array_equal(h.flat["actor"][:NA], c["actor"][:NA])


# --------------------------------------------------------------------------------------- 3. the chain
def test_six_chained_steps_against_the_fp64_chain(host):
    case = SC.chain_case("init")
    h = SC.HostSAC(host, case["actor"], case["critics"], **SC.SAC_ADAM)
    for s in range(SC.CHAIN_STEPS):
        sl = slice(s * SC.CHAIN_ROWS, (s + 1) * SC.CHAIN_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        before = h.flat["actor"][NA]
        h.step(obs, act, h.target(no, rew, done, GAMMA, SEED, s), SEED, s)
        assert h.flat["actor"][NA] != before   # the temperature moves in every step
    worst = SC.check_chain("host chain", h.flat, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| after six chained steps = {worst:.3g}")
    assert case["ref64"]["actor"][NA] != case["actor"][NA]


# --------------------------------------------------------------------------------------- 4. the same code under the sanitizers
def _fnv(a):
    h = 14695981039346656037
    for b in a.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_stand_alone_program_is_clean_under_asan_and_ubsan(host, tmp_path):
    """sachost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests, and they are
    the digests of what the library build returns"""
    m, steps, draw0 = 33, 3, 5
    c, t = SC.grad_case(257, "spread"), SC.target_case(257, "spread")
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([m, steps, 1], np.int32).tobytes()); f.write(np.array([draw0], np.uint32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes()); f.write(np.array([SC.SAC_ADAM["tau"], GAMMA, SC.TARGET_ENTROPY], np.float32).tobytes())
        f.write(np.array([SC.SAC_ADAM["lr"], *SC.SAC_ADAM["betas"], SC.SAC_ADAM["eps"]], np.float64).tobytes())
        f.write(c["actor"].tobytes()); f.write(c["critics"].tobytes())
        for s in range(steps):
            sl = slice(s * m, (s + 1) * m)
            for a in (c["obs"][sl], c["act"][sl], t["next_obs"][sl], t["reward"][sl], t["done"][sl]):
                f.write(np.ascontiguousarray(a).tobytes())
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"sachost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(SC.HOST_DIR, "sachost_main.cpp")])
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    h = SC.HostSAC(host, c["actor"], c["critics"], **SC.SAC_ADAM)
    for s in range(steps):
        sl = slice(s * m, (s + 1) * m)
        obs, act, no, rew, done = (np.ascontiguousarray(a) for a in (c["obs"][sl], c["act"][sl], t["next_obs"][sl], t["reward"][sl], t["done"][sl]))
        action = SC.host_act(host, h.flat["actor"], obs, SEED, 0, s)[0]
        y, a, lp, z = SC.host_target(host, h.flat["actor"], h.flat["critics_target"], no, rew, done, GAMMA, SEED, draw0 + s)
        h.step(obs, act, y, SEED, draw0 + s)
    assert out["plain"] == (f"m={m} steps={steps} actor={_fnv(h.flat['actor']):016x} critics={_fnv(h.flat['critics']):016x} "
                            f"critics_target={_fnv(h.flat['critics_target']):016x} action={_fnv(action):016x} y={_fnv(y):016x} a={_fnv(a):016x} "
                            f"logp={_fnv(lp):016x} z={_fnv(z):016x} ga={_fnv(h.grad['actor']):016x} gc={_fnv(h.grad['critics']):016x}\n")


# --------------------------------------------------------------------------------------- 5. C ABI without a device
SYMBOLS = ("brs_sac_act", "brs_sac_td_target", "brs_ddpg_learner_create_sac", "brs_sac_twin_critic_grad", "brs_sac_actor_grad")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "brs_policy.h")).read()
    tags = {"ACT": S.TAG_ACT, "TARGET": S.TAG_TARGET, "PI": S.TAG_PI}
    for name, value in tags.items():
        assert f"#define BRS_SAC_TAG_{name} 0x{value:08x}u" in hdr
    assert (_lib.SAC_TAG_ACT, _lib.SAC_TAG_TARGET, _lib.SAC_TAG_PI) == tuple(tags.values())
    assert len({*tags.values(), _lib.DDPG_TAG_ACT, _lib.DDPG_TAG_SAMPLE, _lib.TD3_TAG_NOISE}) == 6   # one word per noise stream
    assert "#define BRS_SAC_NSTAT 4" in hdr and _lib.SAC_NSTAT == S.NSTAT == 4 and _lib.SAC_NACTOR == S.NACTOR == offpolicy.SAC_NACTOR


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    buf, nan, inf = C.c_void_p(64), float("nan"), float("inf")
    err, lerr = (lambda: L.brs_ddpg_last_error(None)), (lambda: L.brs_ddpg_learner_last_error(None))

    def act(actor=buf, n=4, obs=buf, random=0, action=buf):
        return L.brs_sac_act(None, actor, n, obs, 11, 0, 0, 0, random, action, None, None, None, None)
    for kw, why in ((dict(n=0), b"n must be at least 1"), (dict(action=None), b"null argument"), (dict(actor=None), b"null argument"),
                    (dict(obs=None), b"null argument"), (dict(), b"null handle"), (dict(actor=None, obs=None, random=1), b"null handle")):
        assert act(**kw) == ERR_ARG and err() == b"brs_sac_act: " + why, (kw, err())

    def target(actor=buf, critics=buf, m=4, next_obs=buf, reward=buf, done=buf, gamma=0.99, y=buf):
        return L.brs_sac_td_target(None, actor, critics, m, next_obs, reward, done, gamma, 11, 0, y, None, None, None, None)
    for kw, why in ((dict(actor=None), b"null argument"), (dict(critics=None), b"null argument"), (dict(next_obs=None), b"null argument"),
                    (dict(reward=None), b"null argument"), (dict(done=None), b"null argument"), (dict(y=None), b"null argument"),
                    (dict(m=0), b"m must be at least 1"), (dict(gamma=nan), b"gamma must be finite"), (dict(gamma=inf), b"gamma must be finite"),
                    (dict(), b"null handle")):
        assert target(**kw) == ERR_ARG and err() == b"brs_sac_td_target: " + why, (kw, err())
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create_sac(0, 256, None) == ERR_ARG and lerr() == b"brs_ddpg_learner_create_sac: null argument"
    for bad in (0, -5, (1 << 22) + 1):
        assert L.brs_ddpg_learner_create_sac(0, bad, C.byref(h)) == ERR_ARG and h.value is None
        assert lerr() == b"brs_ddpg_learner_create_sac: max_batch must be in [1, 2^22]"
    cg = lambda m, critics=buf, obs=buf, act=buf, y=buf, out=buf: L.brs_sac_twin_critic_grad(None, critics, m, obs, act, y, out, None)
    for args, why in (((4, None), b"null argument"), ((4, buf, None), b"null argument"), ((4, buf, buf, None), b"null argument"),
                      ((4, buf, buf, buf, None), b"null argument"), ((4, buf, buf, buf, buf, None), b"null argument"),
                      ((0,), b"m must be at least 1"), ((4,), b"null handle")):
        assert cg(*args) == ERR_ARG and lerr() == b"brs_sac_twin_critic_grad: " + why, why

    def ag(actor=buf, critics=buf, m=4, obs=buf, te=-2.0, out=buf):
        return L.brs_sac_actor_grad(None, actor, critics, m, obs, 11, 0, 1, te, out, None)
    for kw, why in ((dict(actor=None), b"null argument"), (dict(critics=None), b"null argument"), (dict(obs=None), b"null argument"),
                    (dict(out=None), b"null argument"), (dict(m=0), b"m must be at least 1"), (dict(m=-1), b"m must be at least 1"),
                    (dict(te=nan), b"target_entropy must be finite"), (dict(te=-inf), b"target_entropy must be finite"), (dict(), b"null handle")):
        assert ag(**kw) == ERR_ARG and lerr() == b"brs_sac_actor_grad: " + why, (kw, lerr())
    assert err() != lerr()   # a slot per family


def test_host_build_shares_the_argument_rules(host):
    buf = C.c_void_p(64)
    assert host.sh_argument_error(0, buf, None, 0, buf, None, None, 0.0, buf, 0) == b"n must be at least 1"
    assert host.sh_argument_error(1, buf, buf, 4, buf, buf, buf, float("nan"), buf, 0) == b"gamma must be finite"
    assert host.sh_argument_error(2, buf, None, 4, buf, buf, None, 0.0, buf, 0) == b"null argument"
    assert host.sh_argument_error(3, buf, buf, 4, buf, None, None, float("inf"), buf, 0) == b"target_entropy must be finite"
    assert host.sh_argument_error(3, buf, buf, 4, buf, None, None, -2.0, buf, 0) is None


def test_everything_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create_sac(0, 256, C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_ddpg_learner_last_error(None)
    assert msg.startswith(b"brs_ddpg_learner_create_sac: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    from balance_robot_mujoco_rl_amd import BrsError, DeviceSACLearner, DeviceSACNets
    with pytest.raises(BrsError, match="SAC learner has no CPU fallback"):
        DeviceSACLearner()
    with pytest.raises(BrsError):
        DeviceSACNets()


# --------------------------------------------------------------------------------------- 6. the Python layer and the tool
def test_flatten_sac_actor_round_trip_in_both_namings():
    actor = SC.weights("spread")[0]
    for naming, first in (("sb3", "actor.latent_pi.0.weight"), ("tool", "actor.body.0.weight")):
        sd = offpolicy.unflatten_sac_actor(actor, naming)
        assert first in sd and len(sd) == 9 and sd[first].shape == (300, 6) and sd["actor.log_std.weight"].shape == (2, 200)
        assert float(sd["log_ent_coef"][0]) == actor[NA]
        back = offpolicy.flatten_sac_actor(sd)
        assert back.dtype == np.float32 and back.tobytes() == actor.tobytes()
        # rows 2-3 of the stacked output layer are the log_std head
        w3 = actor[S.RL.block_slices(S.ACTOR_SIZES)["W3"]].reshape(4, 200)
        assert np.array_equal(sd["actor.mu.weight"].numpy(), w3[:2]) and np.array_equal(sd["actor.log_std.weight"].numpy(), w3[2:])
        mu, raw = S.heads(actor, np.ones((1, 6)))
        h = torch.relu(torch.relu(torch.ones(1, 6) @ sd[first].T + sd[first.replace("weight", "bias")]) @ sd[first.replace("0.weight", "2.weight")].T
                       + sd[first.replace("0.weight", "2.bias")])
        assert np.allclose((h @ sd["actor.log_std.weight"].T + sd["actor.log_std.bias"]).numpy(), raw, rtol=1e-4, atol=1e-4)
    sd = offpolicy.unflatten_sac_actor(actor, "sb3")
    with pytest.raises(ValueError, match="actor.mu.bias: missing"):
        offpolicy.flatten_sac_actor({k: v for k, v in sd.items() if k != "actor.mu.bias"})
    with pytest.raises(ValueError, match="log_ent_coef: missing"):
        offpolicy.flatten_sac_actor({k: v for k, v in sd.items() if k != "log_ent_coef"})
    with pytest.raises(ValueError, match="expected shape"):
        offpolicy.flatten_sac_actor({**sd, "actor.log_std.weight": torch.zeros(4, 200)})
    with pytest.raises(ValueError, match="neither"):
        offpolicy.flatten_sac_actor({"actor.mu.0.weight": torch.zeros(300, 6)})
    with pytest.raises(ValueError):
        offpolicy.unflatten_sac_actor(actor[:NA])
    with pytest.raises(ValueError):
        offpolicy.unflatten_sac_actor(actor, "td3")


def test_tool_usage_errors():
    tool = os.path.join(ROOT, "tools", "train_sac_torch.py")
    for args, text in ((["--device-learner"], "--device-learner requires --device-data"), (["--ent-coef", "0"], "--ent-coef must be 'auto' or a positive number"),
                       (["--ent-coef", "high"], "--ent-coef must be 'auto' or a positive number"), (["--target-entropy", "nan"], "--target-entropy must be finite")):
        r = subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr[-500:])
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--ent-coef" in r.stdout and "--target-entropy" in r.stdout


def test_tool_gradient_step_against_the_restatement():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_sac_torch as T
    model = T.SAC("cpu", seed=0)
    assert model.flat["actor"].shape == (NA + 1,) and model.flat["critics"].shape == (2 * NC,) and float(model.flat["actor"][-1]) == 0.0
    assert model.actor.log_std.bias.data_ptr() == model.flat["actor"][NA - 2:].data_ptr() and model.log_ent_coef.data_ptr() == model.flat["actor"][NA:].data_ptr()
    assert offpolicy.flatten_sac_actor(model.state_dict()).tobytes() == model.flat["actor"].numpy().tobytes()
    assert offpolicy.flatten_td3_critics(model.state_dict(), "critic").tobytes() == model.flat["critics"].numpy().tobytes()
    fixed = T.SAC("cpu", seed=0, ent_coef="0.2")
    assert abs(float(fixed.flat["actor"][-1]) - np.log(0.2)) < 1e-6 and not fixed.learn_alpha
    c = SC.grad_case(33, "init")
    start = {k: model.flat[k].numpy().copy() for k in ("actor", "critics")}
    ref = S.TorchSAC(start["actor"], start["critics"], torch.float32, target_entropy=-2.0, **SC.SAC_ADAM)
    obs, act, y = (torch.from_numpy(c[k]) for k in ("obs", "act", "y"))
    for s in range(3):
        z = torch.from_numpy(S.row_noise(S.TAG_PI, SEED, s, 33)).float()
        _, _, ent = model.gradient_step(obs, act, y, z=z)
        ref.step(c["obs"], c["act"], c["y"], SEED, s)
        fixed.gradient_step(obs, act, y, z=z)
    assert abs(float(ent) - float(np.exp(ref.flats()["actor"][NA] + 0.0))) < 1e-2
    # two fp32 evaluations of one rule: Adam's first steps are +-lr wherever |g| >> eps, so they can differ only on elements whose
    # gradient is at rounding level; another rule (the first critic alone, the new temperature in the actor's loss) moves it by O(1)
    begin = {"actor": start["actor"], "critics": start["critics"], "critics_target": start["critics"]}
    for k, v in ref.flats().items():
        d, dref = model.flat[k].detach().numpy() - begin[k], v - begin[k]
        assert np.linalg.norm(d - dref) <= 1e-2 * np.linalg.norm(dref) and np.linalg.norm(dref) > 0, k
    assert float(model.flat["actor"][-1]) != 0.0 and abs(float(fixed.flat["actor"][-1]) - np.log(0.2)) < 1e-6
    y_t = model.td_target_torch(obs, torch.from_numpy(c["y"]), torch.zeros(33, dtype=torch.uint8), 0.99, z=torch.zeros(33, 2))
    assert y_t.shape == (33,) and torch.isfinite(y_t).all()
