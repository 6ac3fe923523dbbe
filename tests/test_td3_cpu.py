"""TD3 (include/brs_policy.h: brs_td3_td_target, brs_ddpg_learner_create_twin, brs_ddpg_learner_twin_critic_grad)
without a GPU: the host build of the kernel source (tests/td3host) against the fp64 restatement (tests/ref_td3.py); the reduction to
DDPG; the delay; the same host code as a program under the sanitizers; the C ABI's argument checks; the Python layer; the tool's
usage errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ddpg_learner_cases as DC
import ref_offpolicy as R
import ref_td3 as T3
import td3_cases as TC
from balance_robot_mujoco_rl_amd import _lib, offpolicy
from ddpg_learner_cases import ADAM, CPU_ROWS, WEIGHT_SETS, check_gradient
from offpolicy_cases import GAMMA, GXX, ROOT, SEED, gate

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3
NC, NA = TC.NC, TC.NA


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TC.build_host(tmp_path_factory.mktemp("td3host"))


# --------------------------------------------------------------------------------------- 1. the target
def test_the_cases_cover_every_branch_of_the_target():
    total = TC.assert_branch_coverage(TC.coverage_cases())
    first = TC.branch_counts(TC.coverage_cases()[0])
    assert (first["noise_low"], first["noise_high"], first["noise_in"]) == (15, 22, 29)   # what the issue counted on this case
    assert total["done_1"] > 0 and total["done_0"] > 0


@pytest.mark.parametrize("pair", (TC.SB3_NOISE, TC.TIGHT_NOISE))
@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("m", TC.TARGET_ROWS_CPU)
def test_host_target_against_fp64(host, m, kind, pair):
    c = TC.target_case(m, kind, pair)
    y, a, z = TC.host_td3_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, pair[0], pair[1], SEED, 0)
    gate(z, c["z"], f"m={m} {kind} {pair} z"); gate(a, c["a"], f"m={m} {kind} {pair} a'"); gate(y, c["y"], f"m={m} {kind} {pair} y")
    ended = c["done"] != 0
    assert y[ended].tobytes() == c["reward"][ended].tobytes()       # y == r exactly
    assert np.abs(a).max() <= 1.0
    y_only = TC.host_td3_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, pair[0], pair[1], SEED, 0, extras=False)[0]
    assert y_only.tobytes() == y.tobytes()


def test_target_without_noise_and_with_equal_critics_is_the_ddpg_target(host):
    """the reduction to DDPG: policy_noise = 0, both halves one critic -> the bytes of the host's td_target; and the draw matters
    only through z"""
    for m, kind in ((33, "init"), (257, "x3")):
        c = TC.target_case(m, kind, TC.SB3_NOISE)
        one = c["critics"][:NC]
        y, a, z = TC.host_td3_target(host, c["actor"], np.concatenate([one, one]), c["next_obs"], c["reward"], c["done"], GAMMA, 0.0, 0.5, SEED, 0)
        ref = np.zeros(m, np.float32)
        assert host.th_td_target(c["actor"].ctypes.data, one.ctypes.data, m, c["next_obs"].ctypes.data, c["reward"].ctypes.data, c["done"].ctypes.data,
                                 GAMMA, ref.ctypes.data) == 0
        assert y.tobytes() == ref.tobytes()
        gate(a, R.actor(c["actor"], c["next_obs"]), "a' without noise is the target actor's output")
        z1 = TC.host_td3_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, 0.2, 0.5, SEED, 1)[2]
        assert z1.tobytes() != z.tobytes()


# --------------------------------------------------------------------------------------- 2. the twin gradient
@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("n", CPU_ROWS)
def test_host_twin_gradient_against_fp64(host, n, kind):
    c = TC.twin_case(n, kind)
    g64, g32 = TC.twin_references(n, kind)
    g = TC.host_twin_critic_grad(host, c["critics"], c["obs"], c["act"], c["y"])
    for k, (mine, r64, r32) in enumerate(zip(TC.split_twin(g), TC.split_twin(g64), TC.split_twin(g32))):
        check_gradient(f"n={n} {kind} critic {k}", mine, r64, r32, R.CRITIC_SIZES, gate)
        single = np.zeros(NC + 2, np.float32)
        assert host.th_critic_grad(c["critics"][k * NC:].ctypes.data, n, c["obs"].ctypes.data, c["act"].ctypes.data, c["y"].ctypes.data,
                                   single.ctypes.data) == 0
        assert mine.tobytes() == single.tobytes()   # block k is the single-critic gradient of critic k


def test_twin_conditions_hold_for_the_second_critic():
    c = TC.twin_case(1000, "x3")
    pre = TC._critic_pre(c["critics"][NC:], c["obs"], c["act"])
    assert np.abs(pre).min() >= 1e-4
    t = 2.0 * (R.critic(c["critics"][NC:], c["obs"], c["act"]) - c["y"]) / 1000
    assert abs(t.sum()) >= 0.25 * np.abs(t).sum()
    frac = (pre[:, :200] > 0).mean(axis=1)
    assert frac.min() >= 0.25 and frac.max() <= 0.75


# --------------------------------------------------------------------------------------- 3. the delay
def test_delay_freezes_the_actor_and_all_targets_on_odd_steps(host):
    """six steps with policy_delay = 2 on the host build: after steps 1, 3 and 5 the actor and all three targets are byte-identical to
    before the step, after 2, 4 and 6 they have moved; the chain ends within the trajectory rule of the fp64 chain"""
    case = TC.chain_case("init")
    h = TC.HostTD3(host, case["actor"], case["critics"], policy_delay=TC.POLICY_DELAY, **ADAM)
    for s in range(TC.CHAIN_STEPS):
        sl = slice(s * TC.CHAIN_ROWS, (s + 1) * TC.CHAIN_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        before = {k: h.flat[k].copy() for k in h.flat}
        delayed = h.step(obs, act, h.td3_target(no, rew, done, GAMMA, *TC.SB3_NOISE, SEED, s))
        assert delayed == (s % 2 == 1)
        assert h.flat["critics"].tobytes() != before["critics"].tobytes()
        for k in ("actor", "actor_target", "critics_target"):
            assert (h.flat[k].tobytes() == before[k].tobytes()) == (not delayed), (s, k)
        if delayed:   # both halves of the critics' target moved
            assert not np.array_equal(h.flat["critics_target"][:NC], before["critics_target"][:NC])
            assert not np.array_equal(h.flat["critics_target"][NC:], before["critics_target"][NC:])
    assert h.steps == {"actor": 3, "critics": 6}
    worst = TC.check_chain("host chain", h.flat, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| after six chained steps = {worst:.3g}")


def test_delay_one_without_noise_and_with_equal_critics_is_ddpg(host, tmp_path):
    """policy_delay = 1, policy_noise = 0, both halves one critic: the first half follows HostDDPG byte for byte, and so does the second"""
    case = TC.chain_case("init")
    one = case["critics"][:NC]
    h = TC.HostTD3(host, case["actor"], np.concatenate([one, one]), policy_delay=1, **ADAM)
    d = DC.HostDDPG(DC.build_host(tmp_path), case["actor"], one, **ADAM)
    for s in range(3):
        sl = slice(s * TC.CHAIN_ROWS, (s + 1) * TC.CHAIN_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        assert h.step(obs, act, h.td3_target(no, rew, done, GAMMA, 0.0, 0.5, SEED, s))
        y = np.zeros(TC.CHAIN_ROWS, np.float32)
        assert host.th_td_target(d.flat["actor_target"].ctypes.data, d.flat["critic_target"].ctypes.data, TC.CHAIN_ROWS, no.ctypes.data, rew.ctypes.data,
                                 done.ctypes.data, GAMMA, y.ctypes.data) == 0
        d.step(obs, act, y)
        for mine, theirs in (("actor", "actor"), ("actor_target", "actor_target"), ("critics", "critic"), ("critics_target", "critic_target")):
            n = d.flat[theirs].size
            assert h.flat[mine][:n].tobytes() == d.flat[theirs].tobytes(), (s, mine)
            assert h.flat[mine][-n:].tobytes() == d.flat[theirs].tobytes(), (s, mine)
    assert not np.array_equal(d.flat["actor"], case["actor"])


# --------------------------------------------------------------------------------------- 4. the same code under the sanitizers
def _fnv(a):
    h = 14695981039346656037
    for b in a.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_stand_alone_program_is_clean_under_asan_and_ubsan(host, tmp_path):
    """td3host_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests, and they are
    the digests of what the library build returns"""
    m, steps, delay, draw0 = 33, 4, 2, 5
    c = TC.twin_case(257, "x3")
    t = TC.target_case(257, "x3", TC.TIGHT_NOISE)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([m, steps, delay], np.int32).tobytes()); f.write(np.array([draw0], np.uint32).tobytes())
        f.write(np.array([SEED], np.uint64).tobytes()); f.write(np.array([ADAM["tau"], GAMMA, *TC.TIGHT_NOISE], np.float32).tobytes())
        f.write(np.array([ADAM["lr"], *ADAM["betas"], ADAM["eps"]], np.float64).tobytes())
        f.write(c["actor"].tobytes()); f.write(c["critics"].tobytes())
        for s in range(steps):
            sl = slice(s * m, (s + 1) * m)
            for a in (c["obs"][sl], c["act"][sl], t["next_obs"][sl], t["reward"][sl], t["done"][sl]):
                f.write(np.ascontiguousarray(a).tobytes())
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"td3host_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(TC.HOST_DIR, "td3host_main.cpp")])
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    h = TC.HostTD3(host, c["actor"], c["critics"], policy_delay=delay, **ADAM)
    for s in range(steps):
        sl = slice(s * m, (s + 1) * m)
        obs, act, no, rew, done = (np.ascontiguousarray(a) for a in (c["obs"][sl], c["act"][sl], t["next_obs"][sl], t["reward"][sl], t["done"][sl]))
        y, a, z = TC.host_td3_target(host, h.flat["actor_target"], h.flat["critics_target"], no, rew, done, GAMMA, *TC.TIGHT_NOISE, SEED, draw0 + s)
        h.step(obs, act, y)
    assert out["plain"] == (f"m={m} steps={steps} actor_updates=2 actor={_fnv(h.flat['actor']):016x} critics={_fnv(h.flat['critics']):016x} "
                            f"actor_target={_fnv(h.flat['actor_target']):016x} critics_target={_fnv(h.flat['critics_target']):016x} "
                            f"y={_fnv(y):016x} a={_fnv(a):016x} z={_fnv(z):016x} ga={_fnv(h.grad['actor']):016x} gc={_fnv(h.grad['critics']):016x}\n")


# --------------------------------------------------------------------------------------- 5. C ABI without a device
SYMBOLS = ("brs_td3_td_target", "brs_ddpg_learner_create_twin", "brs_ddpg_learner_twin_critic_grad")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "brs_policy.h")).read()
    assert "#define BRS_TD3_TAG_NOISE 0x5444334eu" in hdr and "#define BRS_TD3_NSTAT 4" in hdr
    assert _lib.TD3_TAG_NOISE == T3.TAG_NOISE == int.from_bytes(b"TD3N", "big") and _lib.TD3_NSTAT == T3.NSTAT == 2 * _lib.DDPG_NSTAT


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    buf = C.c_void_p(64)
    nan, inf = float("nan"), float("inf")
    err = lambda: L.brs_ddpg_last_error(None)
    good = dict(actor=buf, critics=buf, m=4, next_obs=buf, reward=buf, done=buf, policy_noise=0.2, noise_clip=0.5, y=buf)

    def tt(**kw):
        a = {**good, **kw}
        return L.brs_td3_td_target(None, a["actor"], a["critics"], a["m"], a["next_obs"], a["reward"], a["done"], 0.99, a["policy_noise"],
                                   a["noise_clip"], 11, 0, a["y"], None, None, None)
    for kw, why in ((dict(actor=None), b"null argument"), (dict(critics=None), b"null argument"), (dict(next_obs=None), b"null argument"),
                    (dict(reward=None), b"null argument"), (dict(done=None), b"null argument"), (dict(y=None), b"null argument"),
                    (dict(m=0), b"m must be at least 1"), (dict(m=-3), b"m must be at least 1"),
                    (dict(policy_noise=-0.1), b"policy_noise must be finite and >= 0"), (dict(policy_noise=nan), b"policy_noise must be finite and >= 0"),
                    (dict(policy_noise=inf), b"policy_noise must be finite and >= 0"),
                    (dict(noise_clip=-0.5), b"noise_clip must be finite and >= 0"), (dict(noise_clip=nan), b"noise_clip must be finite and >= 0"),
                    (dict(noise_clip=inf), b"noise_clip must be finite and >= 0"),
                    (dict(), b"null handle"), (dict(policy_noise=0.0, noise_clip=0.0), b"null handle")):
        assert tt(**kw) == ERR_ARG and err() == b"brs_td3_td_target: " + why, (kw, err())
    lerr = lambda: L.brs_ddpg_learner_last_error(None)
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create_twin(0, 256, None) == ERR_ARG and lerr() == b"brs_ddpg_learner_create_twin: null argument"
    for bad in (0, -5, (1 << 22) + 1):
        assert L.brs_ddpg_learner_create_twin(0, bad, C.byref(h)) == ERR_ARG and h.value is None
        assert lerr() == b"brs_ddpg_learner_create_twin: max_batch must be in [1, 2^22]"
    tg = lambda m, critics=buf, obs=buf, act=buf, y=buf, out=buf: L.brs_ddpg_learner_twin_critic_grad(None, critics, m, obs, act, y, out, None)
    for args, why in (((4, None), b"null argument"), ((4, buf, None), b"null argument"), ((4, buf, buf, None), b"null argument"),
                      ((4, buf, buf, buf, None), b"null argument"), ((4, buf, buf, buf, buf, None), b"null argument"),
                      ((0,), b"m must be at least 1"), ((-2,), b"m must be at least 1"), ((4,), b"null handle")):
        assert tg(*args) == ERR_ARG and lerr() == b"brs_ddpg_learner_twin_critic_grad: " + why, why
    assert err() != lerr()   # a slot per family


def test_everything_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create_twin(0, 256, C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_ddpg_learner_last_error(None)
    assert msg.startswith(b"brs_ddpg_learner_create_twin: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    from balance_robot_mujoco_rl_amd import BrsError, DeviceDDPGNets, DeviceTD3Learner
    with pytest.raises(BrsError, match="TD3 learner has no CPU fallback"):
        DeviceTD3Learner()
    assert callable(DeviceDDPGNets.td3_target)
    with pytest.raises(BrsError):
        DeviceDDPGNets()   # td3_target lives on an object that cannot exist without a device


# --------------------------------------------------------------------------------------- 6. the Python layer and the tool
def test_flatten_td3_critics_round_trip_in_both_namings():
    _, critics = TC.weights("init")
    for naming, first in (("sb3", "critic.qf0.0.weight"), ("tool", "critic.0.0.weight")):
        for net in ("critic", "critic_target"):
            sd = offpolicy.unflatten_td3_critics(critics, net, naming)
            assert first.replace("critic", net, 1) in sd and len(sd) == 12
            assert sd[first.replace("critic", net, 1)].shape == (200, 8)
            back = offpolicy.flatten_td3_critics(sd, net)
            assert back.dtype == np.float32 and back.tobytes() == critics.tobytes()
            # critic k of the pair is the DDPG critic's flat order
            one = offpolicy.unflatten_ddpg_state_dict(critics[NC:], "critic", "sb3")
            key = (f"{net}.qf1.4.bias" if naming == "sb3" else f"{net}.1.4.bias")
            assert torch.equal(sd[key], one["critic.qf0.4.bias"])
    sd = offpolicy.unflatten_td3_critics(critics, "critic", "sb3")
    with pytest.raises(ValueError, match="critic.qf1.2.weight: missing"):
        offpolicy.flatten_td3_critics({k: v for k, v in sd.items() if k != "critic.qf1.2.weight"})
    with pytest.raises(ValueError, match="expected shape"):
        offpolicy.flatten_td3_critics({**sd, "critic.qf0.0.weight": torch.zeros(200, 6)})
    with pytest.raises(ValueError, match="neither"):
        offpolicy.flatten_td3_critics({"actor.mu.0.weight": torch.zeros(300, 6)})
    with pytest.raises(ValueError, match="neither"):
        offpolicy.flatten_td3_critics(sd, "critic_target")   # the dict holds the online critics only
    with pytest.raises(ValueError):
        offpolicy.unflatten_td3_critics(critics[:NC])
    with pytest.raises(ValueError):
        offpolicy.flatten_td3_critics(sd, "actor")
    # the DDPG helpers stay as they are: a TD3 state_dict in SB3's naming still gives the first critic
    assert offpolicy.flatten_ddpg_state_dict(sd, "critic").tobytes() == critics[:NC].tobytes()


def test_learner_state_dict_round_trip_includes_n_updates():
    from balance_robot_mujoco_rl_amd import DeviceTD3Learner

    def bare(fill):
        o = object.__new__(DeviceTD3Learner)
        o.device, o.h = torch.device("cpu"), None
        o.m_critics, o.v_critics = torch.full((2 * NC,), fill), torch.full((2 * NC,), 2 * fill)
        o.m_actor, o.v_actor = torch.full((NA,), 3 * fill), torch.full((NA,), 4 * fill)
        o.steps_critics, o.steps_actor, o.n_updates = int(10 * fill), int(5 * fill), int(11 * fill)
        return o
    a, b = bare(1.0), bare(0.0)
    sd = a.state_dict()
    assert sorted(sd) == ["m_actor", "m_critics", "n_updates", "steps_actor", "steps_critics", "v_actor", "v_critics"]
    a.m_critics.zero_()   # the state_dict is a copy
    assert float(sd["m_critics"][0]) == 1.0
    b.load_state_dict(sd)
    assert (b.steps_critics, b.steps_actor, b.n_updates) == (10, 5, 11)
    assert torch.equal(b.v_actor, torch.full((NA,), 4.0)) and b.m_critics.dtype == torch.float32
    with pytest.raises(ValueError):
        b.load_state_dict({**sd, "m_critics": torch.zeros(NC)})


def test_tool_usage_errors():
    tool = os.path.join(ROOT, "tools", "train_td3_torch.py")
    for args, text in ((["--device-learner"], "--device-learner requires --device-data"), (["--policy-delay", "0"], "--policy-delay must be at least 1"),
                       (["--target-noise-clip", "-1"], "--target-policy-noise and --target-noise-clip must be >= 0")):
        r = subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and text in r.stderr, (args, r.stderr[-500:])
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "NormalActionNoise(0.1) is kept" in " ".join(r.stdout.split())


def test_tool_holds_the_critics_as_views_of_one_vector():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_td3_torch as T
    model = T.TD3("cpu", seed=0)
    assert model.flat["critics"].shape == (2 * NC,) and model.flat["critics_target"].shape == (2 * NC,) and model.flat["actor"].shape == (NA,)
    assert model.critic[1][0].weight.data_ptr() == model.flat["critics"][NC:].data_ptr()
    assert torch.equal(model.flat["critics"], model.flat["critics_target"]) and not torch.equal(model.flat["critics"][:NC], model.flat["critics"][NC:])
    assert offpolicy.flatten_td3_critics(model.state_dict(), "critic").tobytes() == model.flat["critics"].numpy().tobytes()
    # gradient_step against the fp64 restatement, three steps on given targets: the delay, the first critic in the actor's loss
    c = TC.twin_case(33, "init")
    model0 = {k: model.flat[k].numpy().copy() for k in ("actor", "critics")}
    ref = T3.TorchTD3(model0["actor"], model0["critics"], torch.float32, **ADAM)
    obs, act, y = (torch.from_numpy(c[k]) for k in ("obs", "act", "y"))
    for s in range(3):
        before = model.flat["actor_target"].clone()
        _, la = model.gradient_step(obs, act, y)
        ref.step(c["obs"], c["act"], c["y"])
        assert (la is None) == (s % 2 == 0) and torch.equal(before, model.flat["actor_target"]) == (s % 2 == 0)
    # two fp32 evaluations of one rule: Adam's first steps are +-lr wherever |g| >> eps, so they can differ only on elements whose
    # gradient is at rounding level, a vanishing share of the update's norm; another rule (the second critic in the actor's loss, no
    # delay) moves it by O(1)
    start = {"actor": model0["actor"], "critics": model0["critics"], "actor_target": model0["actor"], "critics_target": model0["critics"]}
    for k, v in ref.flats().items():
        d, dref = model.flat[k].numpy() - start[k], v - start[k]
        assert np.linalg.norm(d - dref) <= 1e-2 * np.linalg.norm(dref) and np.linalg.norm(dref) > 0, k
