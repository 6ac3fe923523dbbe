"""The DDPG data path (include/brs_policy.h: brs_ddpg_*, brs_replay_*) without a GPU: the host build of the
kernel source (tests/offpolicyhost: the shared header brs_offpolicy.hpp with a plain-loop forward) against the fp64 numpy
restatement (tests/ref_offpolicy.py); the same host code as a program under the sanitizers; the C ABI's argument checks; the
state_dict conversions of the Python layer; the torch path of tools/train_ddpg_torch.py on a toy env."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_offpolicy as R
from balance_robot_mujoco_rl_amd import _lib, offpolicy
from offpolicy_cases import (BUFFER_CASES, FORWARD_ROWS, GAMMA, GXX, HOST_DIR, ROOT, SAMPLE_M, SEED, SENTINEL, SENTINEL_DONE, WEIGHT_SETS,
                             HostBuffer, build_host, conditioned, env_steps, gate, host_act, host_q, host_td_target, reference_buffer, weights)

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("offpolicyhost"))


# --------------------------------------------------------------------------------------- 1. the forwards
def _torch32(case):
    """fp32 torch on the same inputs -> (mean, q, y): how far plain fp32 is from the yardstick"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))

    def net(flat, sizes, squash, x):
        at = 0
        for k, (i, o) in enumerate(zip(sizes[:-1], sizes[1:])):
            W = t(flat[at:at + o * i]).view(o, i); at += o * i
            b = t(flat[at:at + o]); at += o
            x = torch.nn.functional.linear(x, W, b)
            x = torch.relu(x) if k < 2 else (torch.tanh(x) if squash else x)
        return x
    obs, act = t(case["obs"]), t(case["act"])
    mu = net(case["actor"], R.ACTOR_SIZES, True, obs)
    q = net(case["critic"], R.CRITIC_SIZES, False, torch.cat([obs, act], 1))[:, 0]
    qn = net(case["critic"], R.CRITIC_SIZES, False, torch.cat([obs, mu], 1))[:, 0]
    y = t(case["reward"]) + (1 - t(case["done"]).float()) * np.float32(GAMMA) * qn
    return mu.numpy(), q.numpy(), y.numpy()


def _rel(x, ref):
    return float((np.abs(np.asarray(x, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("n", FORWARD_ROWS)
def test_host_forwards_against_fp64(host, n, kind):
    c = conditioned(n, kind)
    mu64 = R.actor(c["actor"], c["obs"])
    q64 = R.critic(c["critic"], c["obs"], c["act"])
    y64 = R.td_target(c["actor"], c["critic"], c["obs"], c["reward"], c["done"], GAMMA)
    _, mu, _ = host_act(host, c["actor"], c["obs"], SEED, 0, 0, 0.0)
    q = host_q(host, c["critic"], c["obs"], c["act"])
    y = host_td_target(host, c["actor"], c["critic"], c["obs"], c["reward"], c["done"], GAMMA)
    mine = max(gate(mu, mu64, f"n={n} {kind} mean"), gate(q, q64, f"n={n} {kind} q"), gate(y, y64, f"n={n} {kind} y"))
    t32 = max(_rel(a, b) for a, b in zip(_torch32(c), (mu64, q64, y64)))
    print(f"n={n} {kind}: host build {mine:.3g}, fp32 torch {t32:.3g} from fp64")
    if kind == "x3" and n >= 255:
        assert np.abs(q64).max() > 3.0 and np.abs(mu64).max() > 0.9   # the second set does what it is for
    assert y[c["done"] == 1].tobytes() == c["reward"][c["done"] == 1].tobytes()   # a done row is the reward itself


def test_conditioned_inputs_exercise_relu_and_padding():
    c = conditioned(257, "init")
    _, a1, a2 = R.actor(c["actor"], c["obs"], hidden=True)
    _, c1, c2 = R.critic(c["critic"], c["obs"], c["act"], hidden=True)
    for p, width in ((a1, 300), (a2, 200), (c1, 200), (c2, 150)):
        frac = (p > 0).mean(axis=1)
        assert p.shape[1] == width and frac.min() >= 0.25 and frac.max() <= 0.75


# --------------------------------------------------------------------------------------- 2. noise
def test_noise_clip_and_modes(host):
    c = conditioned(65, "init")
    n, sigma, step, base = 65, 0.1, 5, 1000
    a, m, z = host_act(host, c["actor"], c["obs"], SEED, base, step, sigma)
    a64, m64, z64 = R.act(c["actor"], c["obs"], SEED, base, step, sigma)
    # r <= 5.9 for 24-bit uniforms and the fp32 rounding of 2 pi u2 moves cos by <= 4e-7: ~3e-6 in all
    assert np.abs(z - z64).max() <= 1e-5
    gate(m, m64, "mean")
    formed = np.clip(m + np.float32(sigma) * z, np.float32(-1), np.float32(1))
    assert formed.dtype == np.float32 and np.abs(a - formed).max() <= 1e-7
    assert np.abs(a - a64).max() <= 1e-5
    # sigma = 0 returns the mean: predict(deterministic=True)
    a0, m0, _ = host_act(host, c["actor"], c["obs"], SEED, base, step, 0.0)
    assert a0.tobytes() == m0.tobytes() == m.tobytes()
    # the learning_starts phase: the documented map of words 2 and 3, exactly; the noise is added there too
    ar, mr, zr = host_act(host, None, None, SEED, base, step, sigma, random=True, n=n)
    _, mr64, _ = R.act(None, [None] * n, SEED, base, step, sigma, random=True)
    assert mr.min() >= -1.0 and mr.max() <= 1.0 and np.array_equal(mr.astype(np.float64), mr64)
    assert zr.tobytes() == z.tobytes() and ar.min() >= -1.0 and ar.max() <= 1.0
    assert np.abs(ar - np.clip(mr + np.float32(sigma) * zr, np.float32(-1), np.float32(1))).max() <= 1e-7
    assert np.unique(mr).size > n   # not one value repeated
    # a large sigma clips
    ab, _, _ = host_act(host, c["actor"], c["obs"], SEED, base, step, 5.0)
    assert ab.min() == -1.0 and ab.max() == 1.0
    # another step or another env: other draws
    _, _, z_step = host_act(host, c["actor"], c["obs"], SEED, base, step + 1, sigma)
    _, _, z_env = host_act(host, c["actor"], c["obs"], SEED, base + 1, step, sigma)
    assert not np.array_equal(z_step, z) and np.array_equal(z_env[:-1], z[1:]) and not np.array_equal(z_env[0], z[0])
    assert len({tuple(r) for r in z}) == n


def test_sharded_calls_return_the_bytes_of_the_single_call(host):
    c = conditioned(65, "init")
    obs = np.concatenate([c["obs"], c["obs"][::-1]])   # n = 130
    whole = host_act(host, c["actor"], obs, SEED, 0, 9, 0.1)
    lo, hi = host_act(host, c["actor"], obs[:65].copy(), SEED, 0, 9, 0.1), host_act(host, c["actor"], obs[65:].copy(), SEED, 65, 9, 0.1)
    for w, a, b in zip(whole, lo, hi):
        assert w.tobytes() == np.concatenate([a, b]).tobytes()


# --------------------------------------------------------------------------------------- 3. the buffer
@pytest.mark.parametrize("n,cap", BUFFER_CASES)
def test_host_buffer_follows_the_rules_byte_for_byte(host, n, cap):
    steps = env_steps(n, 2 * cap + 1)
    assert {(int(a != 0), int(b)) for s in steps for a, b in zip(s["terminated"], s["truncated"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    hb = HostBuffer(host, n, cap)
    for t, s in enumerate(steps):
        before = [a.copy() for a in hb.arrays]
        pos = hb.pos
        hb.add(s)
        ref = reference_buffer(n, cap, steps[:t + 1])
        for a, b, r in zip(hb.arrays, before, ref.arrays()):
            others = np.arange(cap) != pos
            assert a[others].tobytes() == b[others].tobytes()   # an add changes row pos only
            if t < cap:
                assert np.all(a[t + 1:] == (SENTINEL_DONE if a.dtype == np.uint8 else SENTINEL))
            filled = np.arange(cap) < ref.rows
            assert a[filled].tobytes() == r[filled].tobytes()
        assert (hb.pos, hb.full) == (ref.pos, ref.full)
        # the rule itself, on the row just written
        ended = (s["terminated"] != 0) | (s["truncated"] != 0)
        assert np.array_equal(hb.arrays[1][pos][ended], s["terminal_obs"][ended]) and np.array_equal(hb.arrays[1][pos][~ended], s["obs"][~ended])
        assert np.array_equal(hb.arrays[4][pos], (s["terminated"] != 0).astype(np.uint8))   # a time-limit end keeps done = 0


# --------------------------------------------------------------------------------------- 4. sampling
@pytest.fixture(scope="module")
def filled(host):
    n, cap = 65, 4
    hb = HostBuffer(host, n, cap)
    for s in env_steps(n, cap):
        hb.add(s)
    return hb


@pytest.mark.parametrize("m", SAMPLE_M)
def test_host_sample_indices_and_rows(filled, m):
    (o, no, a, r, d), idx = filled.sample(m, draw=3)
    rows, envs = R.sample_indices(SEED, 3, m, filled.cap, filled.n)
    assert np.array_equal(idx[:, 0], rows) and np.array_equal(idx[:, 1], envs)
    for got, arr in zip((o, no, a, r, d), filled.arrays):
        assert got.tobytes() == arr[rows, envs].tobytes()
    again, idx2 = filled.sample(m, draw=3)
    nxt, idx3 = filled.sample(m, draw=4)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (o, no, a, r, d))) and idx2.tobytes() == idx.tobytes()
    assert m < 64 or idx3.tobytes() != idx.tobytes()


def test_host_sample_from_a_buffer_that_is_not_full(host):
    n, cap = 65, 4
    hb = HostBuffer(host, n, cap)
    for s in env_steps(n, 2):
        hb.add(s)
    assert hb.rows == 2
    (o, _, _, r, d), idx = hb.sample(1000)
    assert idx[:, 0].max() == 1 and idx[:, 0].min() == 0 and idx[:, 1].max() < n and not np.any(r == SENTINEL) and not np.any(d == SENTINEL_DONE)
    _, idx1 = hb.sample(256, size=1)
    assert np.all(idx1[:, 0] == 0) and np.unique(idx1[:, 1]).size > 32
    assert hb.draw == 2   # every sample() without a given draw takes the counter's next value


def test_index_map_is_uniform():
    """the yardstick's map alone: 120,000 draws over the 12 cells of (size 4, n 3); every count within 6 binomial sigma of 10,000
    (sigma = sqrt(120000 x 1/12 x 11/12) = 95.7, six of them ~ 575)"""
    w = np.random.default_rng(0).integers(0, 2 ** 32, size=(120000, 2), dtype=np.uint64)
    rows, envs = R.index_map(w[:, 0], w[:, 1], 4, 3)
    assert rows.min() == 0 and rows.max() == 3 and envs.min() == 0 and envs.max() == 2
    counts = np.bincount(rows * 3 + envs, minlength=12)
    assert counts.size == 12 and np.abs(counts - 10000).max() <= 6 * np.sqrt(120000 * (1 / 12) * (11 / 12)), counts
    r, e = R.index_map([0, 2 ** 32 - 1], [0, 2 ** 32 - 1], 4, 3)
    assert list(r) == [0, 3] and list(e) == [0, 2]


# --------------------------------------------------------------------------------------- 5. the same code under the sanitizers
def _fnv(*arrays):
    h = 14695981039346656037
    for a in arrays:
        for b in a.tobytes():
            h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_stand_alone_program_is_clean_under_asan_and_ubsan(host, tmp_path):
    """offpolicyhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests, and
    they are the digests of what the library build returns"""
    n, cap, nsteps, m, sigma = 33, 3, 7, 65, 0.1
    actor_w, critic_w = weights("init")
    steps = env_steps(n, nsteps, seed=5)
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([n, cap, nsteps, m], np.int32).tobytes()); f.write(np.array([SEED], np.uint64).tobytes())
        f.write(np.array([sigma, GAMMA], np.float32).tobytes()); f.write(actor_w.tobytes()); f.write(critic_w.tobytes())
        for s in steps:
            for k in ("last_obs", "obs", "terminal_obs", "reward", "terminated", "truncated"):
                f.write(s[k].tobytes())
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"offpolicyhost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(HOST_DIR, "offpolicyhost_main.cpp")])
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    hb = HostBuffer(host, n, cap)
    hb.arrays = tuple(np.full_like(a, 9 if a.dtype == np.uint8 else -7.0) for a in hb.arrays)   # the program's fill
    for t, s in enumerate(steps):
        action, _, _ = host_act(host, actor_w, s["last_obs"], SEED, 0, t, sigma, random=bool(t & 1))
        hb.add({**s, "action": action})
    (o, no, a, r, d), idx = hb.sample(m, draw=0)
    y, q = host_td_target(host, actor_w, critic_w, no, r, d, GAMMA), host_q(host, critic_w, o, a)
    assert out["plain"] == (f"n={n} cap={cap} steps={nsteps} m={m} storage={_fnv(*hb.arrays):016x} sample={_fnv(o, no, a, r, d):016x} "
                            f"idx={_fnv(idx):016x} y={_fnv(y):016x} q={_fnv(q):016x}\n")


# --------------------------------------------------------------------------------------- 6. C ABI without a device
OFFPOLICY_SYMBOLS = ("brs_ddpg_create", "brs_ddpg_destroy", "brs_ddpg_last_error", "brs_ddpg_act", "brs_ddpg_q", "brs_ddpg_td_target",
                     "brs_replay_add", "brs_replay_sample", "brs_replay_last_error")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in OFFPOLICY_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    assert ("brs_offpolicy.hip", [], False) in _lib.UNITS
    assert (_lib.DDPG_NACTOR, _lib.DDPG_NCRITIC) == (62702, 32101) == (R.NACTOR, R.NCRITIC)
    assert (_lib.DDPG_TAG_ACT, _lib.DDPG_TAG_SAMPLE) == (R.TAG_ACT, R.TAG_SAMPLE)
    assert len({_lib.DDPG_TAG_ACT, _lib.DDPG_TAG_SAMPLE, 0x504f4c49, 0}) == 4
    hdr = open(os.path.join(ROOT, "include", "brs_policy.h")).read()
    assert "0x44445047u" in hdr and "0x5245504cu" in hdr
    assert C.sizeof(_lib.BrsReplayStorage) == 5 * C.sizeof(C.c_void_p)


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    buf = C.c_void_p(64)
    err = lambda: L.brs_ddpg_last_error(None)
    assert L.brs_ddpg_create(0, None) == ERR_ARG and err() == b"brs_ddpg_create: null argument"
    act = lambda n, sigma, random, actor=buf, out=buf: L.brs_ddpg_act(None, actor, n, buf, 1, 0, 0, sigma, random, out, None, None, None)
    for args, why in (((0, 0.1, 0), b"brs_ddpg_act: n must be at least 1"), ((-3, 0.1, 1), b"brs_ddpg_act: n must be at least 1"),
                      ((4, -0.1, 0), b"brs_ddpg_act: sigma must be >= 0"), ((4, float("nan"), 0), b"brs_ddpg_act: sigma must be >= 0"),
                      ((4, 0.1, 0, None), b"brs_ddpg_act: null argument"), ((4, 0.1, 1, None, None), b"brs_ddpg_act: null argument"),
                      ((4, 0.1, 0), b"brs_ddpg_act: null handle"), ((4, 0.1, 1, None), b"brs_ddpg_act: null handle")):
        assert act(*args) == ERR_ARG and err() == why, why
    assert L.brs_ddpg_q(None, buf, 0, buf, buf, buf, None) == ERR_ARG and err() == b"brs_ddpg_q: n must be at least 1"
    assert L.brs_ddpg_q(None, buf, 4, buf, None, buf, None) == ERR_ARG and err() == b"brs_ddpg_q: null argument"
    assert L.brs_ddpg_q(None, buf, 4, buf, buf, buf, None) == ERR_ARG and err() == b"brs_ddpg_q: null handle"
    td = lambda m, done=buf: L.brs_ddpg_td_target(None, buf, buf, m, buf, buf, done, 0.99, buf, None)
    assert td(0) == ERR_ARG and err() == b"brs_ddpg_td_target: m must be at least 1"
    assert td(4, None) == ERR_ARG and err() == b"brs_ddpg_td_target: null argument"
    assert td(4) == ERR_ARG and err() == b"brs_ddpg_td_target: null handle"
    assert L.brs_ddpg_destroy(None) == ERR_STATE
    # the replay calls have no handle and a slot of their own
    st = _lib.BrsReplayStorage(64, 64, 64, 64, 64)
    hole = _lib.BrsReplayStorage(64, 64, None, 64, 64)
    rerr = L.brs_replay_last_error
    add = lambda s, n, cap, pos, last=buf: L.brs_replay_add(0, s, n, cap, pos, last, buf, buf, buf, buf, buf, buf, None)
    for args, why in (((None, 4, 4, 0), b"brs_replay_add: null storage pointer"), ((C.byref(hole), 4, 4, 0), b"brs_replay_add: null storage pointer"),
                      ((C.byref(st), 0, 4, 0), b"brs_replay_add: n and cap must be at least 1"),
                      ((C.byref(st), 4, 0, 0), b"brs_replay_add: n and cap must be at least 1"),
                      ((C.byref(st), 65536, 32768, 0), b"brs_replay_add: cap * n exceeds 2^31 - 1"),
                      ((C.byref(st), 4, 4, 4), b"brs_replay_add: pos must be in [0, cap)"), ((C.byref(st), 4, 4, -1), b"brs_replay_add: pos must be in [0, cap)"),
                      ((C.byref(st), 4, 4, 0, None), b"brs_replay_add: null argument")):
        assert add(*args) == ERR_ARG and rerr() == why, why
    sample = lambda s, size, m, out=C.byref(st): L.brs_replay_sample(0, s, 4, 4, size, m, 1, 0, out, None, None)
    for args, why in (((None, 1, 1), b"brs_replay_sample: null storage pointer"), ((C.byref(st), 0, 8), b"brs_replay_sample: size must be in [1, cap]"),
                      ((C.byref(st), 5, 8), b"brs_replay_sample: size must be in [1, cap]"), ((C.byref(st), 4, 0), b"brs_replay_sample: m must be in [1, 2^27]"),
                      ((C.byref(st), 4, 8, None), b"brs_replay_sample: null output pointer"),
                      ((C.byref(st), 4, 8, C.byref(hole)), b"brs_replay_sample: null output pointer")):
        assert sample(*args) == ERR_ARG and rerr() == why, why
    assert err() == b"brs_ddpg_td_target: null handle"   # one slot per family
    assert L.brs_replay_add(-1, C.byref(st), 4, 4, 0, buf, buf, buf, buf, buf, buf, buf, None) in (ERR_ARG, ERR_HIP)


def test_everything_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.brs_ddpg_create(0, C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_ddpg_last_error(None)
    assert msg.startswith(b"brs_ddpg_create: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    st, buf = _lib.BrsReplayStorage(64, 64, 64, 64, 64), C.c_void_p(64)
    assert L.brs_replay_add(0, C.byref(st), 4, 4, 0, buf, buf, buf, buf, buf, buf, buf, None) == ERR_HIP
    assert L.brs_replay_last_error().startswith(b"brs_replay_add: no HIP device (")
    assert L.brs_replay_sample(0, C.byref(st), 4, 4, 4, 8, 1, 0, C.byref(st), None, None) == ERR_HIP
    from balance_robot_mujoco_rl_amd import BrsError, DeviceDDPGNets, DeviceReplayBuffer
    with pytest.raises(BrsError):
        DeviceDDPGNets()
    with pytest.raises(BrsError):
        DeviceReplayBuffer(4, 4)


# --------------------------------------------------------------------------------------- 7. the Python layer's conversions
def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ddpg_torch as T
    return T


def test_state_dict_round_trips_in_both_namings():
    T = _tool()
    model = T.DDPG("cpu", seed=3)
    sd = model.state_dict()
    assert offpolicy.naming_of(sd) == "tool" and len(sd) == 24
    for net, size in (("actor", R.NACTOR), ("critic", R.NCRITIC), ("actor_target", R.NACTOR), ("critic_target", R.NCRITIC)):
        flat = offpolicy.flatten_ddpg_state_dict(sd, net)
        assert flat.dtype == np.float32 and flat.shape == (size,)
        np.testing.assert_array_equal(flat, model.flat[net].numpy())   # the tool's flat vector IS the header's order
        back = offpolicy.unflatten_ddpg_state_dict(flat, net, "tool")
        assert sorted(back) == sorted(k for k in sd if k.startswith(net + "."))
        for k in back:
            assert torch.equal(back[k], sd[k]), k
        sb3 = offpolicy.unflatten_ddpg_state_dict(flat, net, "sb3")
        assert offpolicy.naming_of(sb3) == "sb3"
        np.testing.assert_array_equal(offpolicy.flatten_ddpg_state_dict(sb3, net), flat)
    sb3 = offpolicy.unflatten_ddpg_state_dict(model.flat["actor"], "actor", "sb3")
    assert sorted(sb3) == sorted(f"actor.mu.{i}.{k}" for i in (0, 2, 4) for k in ("weight", "bias")) and offpolicy.naming_of(sb3) == "sb3"
    assert tuple(sb3["actor.mu.2.weight"].shape) == (200, 300)
    csb3 = offpolicy.unflatten_ddpg_state_dict(model.flat["critic"], "critic", "sb3")
    assert tuple(csb3["critic.qf0.0.weight"].shape) == (200, 8) and tuple(csb3["critic.qf0.4.bias"].shape) == (1,)
    # the yardstick reads the same order
    (W1, _), _, (W3, b3) = R.layers(model.flat["actor"].numpy(), R.ACTOR_SIZES)
    np.testing.assert_array_equal(W1, sd["actor.0.weight"].numpy().astype(np.float64)); np.testing.assert_array_equal(b3, sd["actor.4.bias"].numpy())
    with pytest.raises(ValueError):
        offpolicy.flatten_ddpg_state_dict({"weight": 1})
    with pytest.raises(ValueError):
        offpolicy.flatten_ddpg_state_dict({**sd, "actor.2.weight": torch.zeros(300, 200)})
    with pytest.raises(ValueError):
        offpolicy.unflatten_ddpg_state_dict(np.zeros(5, np.float32))


# --------------------------------------------------------------------------------------- 8. the tool's torch path on a toy env
class _ToySim:
    """BatchedSim's surface in torch on the CPU: a point that is pushed by the action; falls and time limits both happen"""

    def __init__(self, n, limit=7):
        self.n, self.device, self.limit = n, torch.device("cpu"), limit
        self.gen = torch.Generator().manual_seed(0)

    def reset(self):
        self.x, self.t = torch.randn((self.n, 6), generator=self.gen) * 0.1, torch.zeros(self.n, dtype=torch.int32)
        return self.x

    def step(self, a):
        self.x = self.x + 0.3 * torch.cat([a, a, a], dim=1) + 0.05 * torch.randn((self.n, 6), generator=self.gen)
        self.t += 1
        term = (self.x[:, 0].abs() > 0.8).to(torch.uint8)
        trunc = (self.t >= self.limit).to(torch.uint8)
        tobs, ended = self.x.clone(), (term | trunc).bool()
        self.x = torch.where(ended[:, None], torch.zeros_like(self.x), self.x); self.t[ended] = 0
        return self.x, 1.0 - self.x[:, 0].abs(), term, trunc, tobs


def test_tool_torch_path_on_a_toy_env():
    T = _tool()
    sim = _ToySim(16)
    model = T.DDPG("cpu", seed=1)
    start = {k: v.clone() for k, v in model.flat.items()}
    data = T.TorchData(sim, model, cap=8, sigma=0.1, seed=1)
    log = {}
    updates = T.train(sim, model, data, steps=20, batch=32, learning_starts=48, gradient_steps=1, train_freq=2, log=log)
    assert updates == 9 and data.full and data.rows == 8   # 10 rounds, the first one (32 transitions) below learning_starts
    for k in start:
        assert torch.isfinite(model.flat[k]).all() and not torch.equal(model.flat[k], start[k]), k
    assert np.isfinite(log["critic_loss_last"]) and np.isfinite(log["actor_loss_last"])
    assert int(data.done.sum()) > 0 and int(data.done.sum()) < data.done.numel()
    # the parameters are views of the flat vectors: what Adam wrote is what a kernel would read
    assert model.actor[0].weight.data_ptr() == model.flat["actor"].data_ptr()
    np.testing.assert_array_equal(offpolicy.flatten_ddpg_state_dict(model.state_dict(), "critic_target"), model.flat["critic_target"].numpy())
