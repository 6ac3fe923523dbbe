"""VecNormalize for the off-policy family (include/brs_policy.h: brs_replay_sample_vecnorm) without a GPU: the
host build of the sampling kernel's source against the numpy reference, the conditions of the cases, the same host code as a program
under the sanitizers, fold_vecnormalize in float64, the collector's call sequence, the tools' refusals and the argument checks that
need no device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ref_offpolicy as RO
import vecnorm_cases as K
import vecnorm_replay_cases as V
from balance_robot_mujoco_rl_amd import _lib, nets, vecnorm

ERR_ARG, ERR_STATE = -1, -3


# --------------------------------------------------------------------------------------- 1. the cases
def test_cases_meet_their_conditions():
    """decided on the reference alone: no stored value near a clip, and the chosen draw's largest sample holds every kind of
    clipped element its storage holds"""
    for n in V.SIZES:
        b = V.buffer(n)
        margin, kinds, draw = V.stored_margin(b), V.stored_kinds(b), V.draw_of(n)
        print(f"n = {n}: nearest stored value {margin:.3g} of a clip away; kinds {sorted(k for k, v in kinds.items() if v)}; draw {draw}")
        assert margin > V.NEAR
        if n >= 256:
            assert kinds == dict(obs_hi=True, obs_lo=True, next_hi=False, next_lo=True, rew_hi=True, rew_lo=True)
        else:
            assert kinds == dict(obs_hi=True, obs_lo=True, next_hi=True, next_lo=True, rew_hi=False, rew_lo=True)
        s = V.reference(n, V.MS[-1])
        assert all(V.coverage(b, s).values())
        # the smallest such draw: the vectorised search saw every earlier one fail; its cells are sample_indices' cells
        assert np.array_equal(V.cells_of([draw], V.MS[-1], V.CAP, n)[0], s.idx[:, 0].astype(np.int64) * n + s.idx[:, 1])
        if 0 < draw <= 32:   # where the search is short, every earlier draw once more through the reference itself
            assert not any(all(V.coverage(b, V.reference_sample(b, V.MS[-1], d)).values()) for d in range(draw))
        # the buffer's rows follow the collector's rule: the terminal observation where the env ended, done = terminated
        c = b.case
        for t, (obs, reward, te, tr, tobs) in enumerate(c.steps):
            ended = (te | tr) != 0
            assert np.array_equal(b.next_obs[t], np.where(ended[:, None], tobs, obs)) and np.array_equal(b.done[t], te)
            assert np.array_equal(b.obs[t], c.reset_obs if t == 0 else c.steps[t - 1][0]) and np.array_equal(b.reward[t], reward)


# --------------------------------------------------------------------------------------- 2. host build against the reference
@pytest.mark.parametrize("n", V.SIZES)
def test_host_build_against_the_reference(n):
    b = V.buffer(n)
    for m in V.MS:
        s, (out, idx) = V.reference(n, m), V.host_reference(n, m)
        assert np.array_equal(idx, s.idx), (n, m)
        V.assert_sample_close(out, s, b, (n, m))
    # a partly filled buffer, and each half switched off
    m, draw = 257, V.draw_of(n)
    out, idx = V.host_sample(b, m, draw, size=3)
    s = V.reference_sample(b, m, draw, size=3)
    assert idx[:, 0].max() < 3 and np.array_equal(idx, s.idx)
    V.assert_sample_close(out, s, b, (n, "size 3"))
    full = V.host_reference(n, 257)[0]
    for norm_obs, norm_reward in ((False, True), (True, False), (False, False)):
        out, idx = V.host_sample(b, m, draw, norm_obs=norm_obs, norm_reward=norm_reward)
        s = V.reference_sample(b, m, draw, norm_obs=norm_obs, norm_reward=norm_reward)
        V.assert_sample_close(out, s, b, (n, norm_obs, norm_reward), norm_obs=norm_obs, norm_reward=norm_reward)
        if norm_obs:
            assert out[0].tobytes() == full[0].tobytes() and out[1].tobytes() == full[1].tobytes()
        if norm_reward:
            assert out[3].tobytes() == full[3].tobytes()


def test_host_build_equals_the_composed_host_calls():
    """the contract on the host: the fused sample's bytes are the plain gather's through vecnormhost's stateless calls"""
    n, m = 257, 2049
    b = V.buffer(n)
    out, idx = V.host_reference(n, m)
    h = K.HostVecNormalize(n, clip_obs=b.clip_obs, clip_reward=b.clip_reward)
    h.set_stats(b.stats)
    rows, envs = idx[:, 0], idx[:, 1]
    assert out[0].tobytes() == h.normalize_obs(np.ascontiguousarray(b.obs[rows, envs])).tobytes()
    assert out[1].tobytes() == h.normalize_obs(np.ascontiguousarray(b.next_obs[rows, envs])).tobytes()
    assert out[3].tobytes() == h.normalize_reward(np.ascontiguousarray(b.reward[rows, envs])).tobytes()
    assert out[2].tobytes() == b.action[rows, envs].tobytes() and out[4].tobytes() == b.done[rows, envs].tobytes()
    h.close()


# --------------------------------------------------------------------------------------- 3. the same code under the sanitizers
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """vecnormreplayhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests"""
    files = []
    for n in V.SIZES:
        path = str(tmp_path / f"buffer_{n}.bin")
        V.write_buffer(V.buffer(n), path, V.draw_of(n))
        files.append(path)
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"vecnormreplayhost_{name}")
        subprocess.check_call(K.GXX + flags + ["-o", exe, os.path.join(V.HOST_DIR, "vecnormreplayhost_main.cpp")])
        r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    lines = out["plain"].splitlines()
    assert len(lines) == 4 * len(V.SIZES) and len(set(lines)) == len(lines)
    want = [f"n={n} cap={V.CAP} norm_obs={m & 1} norm_reward={m >> 1} " for n in V.SIZES for m in range(4)]
    assert all(line.startswith(w) for line, w in zip(lines, want)), (lines[:3], want[:3])
    # nothing sits at a clip where obs is copied through; at n = 63 (clips of 1) every normalising sample holds clipped elements
    assert all("clipped_obs=0 " in line for line in lines if "norm_obs=0" in line)
    assert not any("clipped_obs=0 " in line for line in lines if line.startswith("n=63 ") and "norm_obs=1" in line)


# --------------------------------------------------------------------------------------- 4. fold_vecnormalize
@pytest.mark.parametrize("net_arch", ["reference", "sb3"])
def test_fold_vecnormalize_in_float64(net_arch):
    arch, b = nets.arch(net_arch), V.buffer(257)
    sd = dict(obs_mean=b.stats[0:6], obs_var=b.stats[6:12])
    raw = b.obs.reshape(-1, 6).astype(np.float64)
    z = (raw - sd["obs_mean"]) / np.sqrt(sd["obs_var"] + K.EPSILON)
    keep = (np.abs(z) < b.clip_obs).all(axis=1)
    assert 0 < keep.sum() < len(raw)   # rows without a clipped column, and the buffer holds clipped ones too
    raw, z = raw[keep], z[keep]
    rng = np.random.default_rng(11)
    for mlp, extra in ((arch.actor, 0), (arch.sac_actor, 0), (arch.sac_actor, 1)):   # DDPG / TD3 actor, SAC actor without and with log_ent_coef
        flat = (rng.standard_normal(mlp.count + extra) * 0.2).astype(np.float32)
        folded = vecnorm.fold_vecnormalize(flat, sd, net_arch=net_arch, epsilon=K.EPSILON)
        h0 = arch.pi[0]
        assert folded.dtype == np.float32 and folded.shape == flat.shape and folded is not flat
        assert folded[7 * h0:].tobytes() == flat[7 * h0:].tobytes()   # the untouched tail
        # the fold in float64 ...
        w, bias = vecnorm.fold_first_layer(flat[:6 * h0].reshape(h0, 6), flat[6 * h0:7 * h0], sd["obs_mean"], sd["obs_var"], K.EPSILON)
        exact = np.concatenate([w.ravel(), bias, flat[7 * h0:mlp.count].astype(np.float64)])
        sizes = (6,) + tuple(n_out for _, n_out in mlp.sizes)   # ReLU, ReLU, linear (the output's tanh is one-to-one), in float64
        want, got = RO.forward(flat[:mlp.count], z, sizes, False), RO.forward(exact, raw, sizes, False)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print(f"{net_arch}, {mlp.count + extra} parameters: folded on raw rows against the original on normalised rows {err:.3g}")
        assert err <= 1e-9
        # ... and what the function returns is that, rounded once
        assert folded[:7 * h0].tobytes() == np.concatenate([w.ravel(), bias]).astype(np.float32).tobytes()
    with pytest.raises(ValueError):
        vecnorm.fold_vecnormalize(np.zeros(5, np.float32), sd, net_arch=net_arch)
    with pytest.raises(ValueError):
        vecnorm.fold_vecnormalize(np.zeros(arch.actor.count, np.float32), {"obs_mean": np.zeros(6)}, net_arch=net_arch)
    with pytest.raises(ValueError):
        vecnorm.fold_vecnormalize(np.zeros(arch.actor.count, np.float32), dict(obs_mean=np.zeros(5), obs_var=np.ones(5)), net_arch=net_arch)
    with pytest.raises(ValueError):
        vecnorm.fold_vecnormalize(np.zeros(arch.actor.count, np.float32), sd, net_arch="td3")


# --------------------------------------------------------------------------------------- 5. the library's and the package's surface
def test_symbol_signature_and_null_handle():
    import balance_robot_mujoco_rl_amd as P
    L = _lib.lib()
    assert hasattr(L, "brs_replay_sample_vecnorm") and "brs_replay_sample_vecnorm" in _lib.SYMBOLS
    restype, argtypes = _lib.SIGNATURES["brs_policy.h"]["brs_replay_sample_vecnorm"]
    assert restype is C.c_int and len(argtypes) == 11
    assert argtypes[1:] == _lib.SIGNATURES["brs_policy.h"]["brs_replay_sample"][1][1:]   # brs_replay_sample's, behind the handle
    store = _lib.BrsReplayStorage(8, 8, 8, 8, 8)
    assert L.brs_replay_sample_vecnorm(None, C.byref(store), 4, 4, 4, 4, 0, 0, C.byref(store), None, None) == ERR_STATE
    assert P.fold_vecnormalize is vecnorm.fold_vecnormalize and "fold_vecnormalize" in P.__all__


def test_python_signatures():
    import inspect
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceOffPolicyCollector, DeviceReplayBuffer
    assert list(inspect.signature(DeviceReplayBuffer.sample).parameters) == ["self", "m", "out", "idx", "normalize"]
    sig = inspect.signature(DeviceOffPolicyCollector.__init__)
    assert list(sig.parameters) == ["self", "sim", "nets", "actor_params", "replay", "sigma", "monitor", "normalize"]
    assert sig.parameters["normalize"].default is None and sig.parameters["sigma"].default == 0.1
    sig = inspect.signature(vecnorm.fold_vecnormalize)
    assert list(sig.parameters) == ["actor_flat", "state_dict", "net_arch", "epsilon"]
    assert (sig.parameters["net_arch"].default, sig.parameters["epsilon"].default) == ("reference", 1e-8)


# --------------------------------------------------------------------------------------- 6. the collector's call sequence
def _fake_collect(normalize, steps=3, n=4, random=False, norm_n=None):
    """DeviceOffPolicyCollector on stand-ins that only record: the calls collect() makes, with the tensors' identities"""
    import torch
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceOffPolicyCollector
    log, names = [], {}
    name = lambda t: names.get(t.data_ptr(), "private")

    class Sim:
        device = torch.device("cpu")

        def __init__(self):
            self.n = n
            self.out = (torch.ones(n, 6), torch.ones(n), torch.zeros(n, dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8), torch.ones(n, 6))
            for k, t in zip(("sim.obs", "sim.reward", "sim.terminated", "sim.truncated", "sim.terminal_obs"), self.out):
                names[t.data_ptr()] = k

        def reset(self):
            log.append(("sim.reset",))
            return self.out[0]

        def step(self, a):
            log.append(("sim.step",))
            return self.out

    class Nets:
        def act(self, params, obs, step, sigma, random=False, out=None):
            log.append(("nets.act", name(obs), float(obs.flatten()[0]), step, random))

    class Replay:
        def __init__(self):
            self.n = n

        def add(self, last_obs, action, obs, tobs, rew, term, trunc):
            log.append(("replay.add", name(last_obs), float(last_obs.flatten()[0])) + tuple(name(x) for x in (obs, tobs, rew, term, trunc)))

    class Mon:
        def update(self, rew, term, trunc):
            log.append(("monitor.update", name(rew), name(term), name(trunc)))

    class Norm:
        def __init__(self):
            self.n = n if norm_n is None else norm_n
            self.out = (torch.full((n, 6), 2.0), torch.full((n,), 3.0), torch.full((n, 6), 4.0))
            for k, t in zip(("norm.obs", "norm.reward", "norm.terminal_obs"), self.out):
                names[t.data_ptr()] = k

        def reset(self, obs):
            log.append(("normalize.reset", float(obs.flatten()[0])))
            return self.out[0]

        def step(self, obs, rew, term, trunc, tobs):
            log.append(("normalize.step",) + tuple(name(x) for x in (obs, rew, term, trunc, tobs)))
            return self.out
    kw = {} if normalize == "absent" else {"normalize": Norm() if normalize else None}
    col = DeviceOffPolicyCollector(Sim(), Nets(), None, Replay(), monitor=Mon(), **kw)
    col.collect(steps, random=random)
    first = len(log)
    col.collect(steps, random=random)
    return col, log[:first], log[first:]


def test_collector_without_a_normaliser_makes_the_calls_it_made_before():
    step = lambda t: [("nets.act", "private", 1.0, t, False), ("sim.step",), ("monitor.update", "sim.reward", "sim.terminated", "sim.truncated"),
                      ("replay.add", "private", 1.0, "sim.obs", "sim.terminal_obs", "sim.reward", "sim.terminated", "sim.truncated")]
    for normalize in ("absent", None):
        col, first, second = _fake_collect(normalize)
        assert col.normalize is None
        assert first == [("sim.reset",)] + sum((step(t) for t in range(3)), [])
        assert second == sum((step(t) for t in range(3, 6)), [])


@pytest.mark.parametrize("random", [False, True])
def test_collector_with_a_normaliser_follows_sb3s_off_policy_rule(random):
    """the actor sees the normaliser's observation, the buffer the raw last observation and the simulator's raw outputs, the
    monitor the env's own reward; the statistics train in the warm-up too"""
    col, first, second = _fake_collect(True, random=random)
    step = lambda t: [("nets.act", "norm.obs", 2.0, t, random), ("sim.step",), ("monitor.update", "sim.reward", "sim.terminated", "sim.truncated"),
                      ("normalize.step", "sim.obs", "sim.reward", "sim.terminated", "sim.truncated", "sim.terminal_obs"),
                      ("replay.add", "private", 1.0, "sim.obs", "sim.terminal_obs", "sim.reward", "sim.terminated", "sim.truncated")]
    assert first == [("sim.reset",), ("normalize.reset", 1.0)] + sum((step(t) for t in range(3)), [])
    assert second == sum((step(t) for t in range(3, 6)), [])   # no second reset
    with pytest.raises(ValueError, match="the normaliser holds 5 envs, the simulator 4"):
        _fake_collect(True, norm_n=5)


# --------------------------------------------------------------------------------------- 7. the tools' flag
TOOLS = ("train_ddpg_torch.py", "train_td3_torch.py", "train_sac_torch.py")


@pytest.mark.parametrize("tool", TOOLS)
def test_tools_refuse_vec_normalize_without_device_data_and_under_more_than_one_rank(tool):
    path = os.path.join(K.ROOT, "tools", tool)
    r = subprocess.run([sys.executable, path, "--vec-normalize"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--vec-normalize requires --device-data" in r.stderr, (tool, r.stderr[-500:])
    r = subprocess.run([sys.executable, path, "--vec-normalize", "--device-data"], capture_output=True, text=True,
                       env=dict(os.environ, WORLD_SIZE="2"), timeout=120)
    assert r.returncode == 2 and "--vec-normalize runs on one rank only" in r.stderr, (tool, r.stderr[-500:])


def test_eval_quant_policy_takes_vec_normalize_with_an_actor_only():
    r = subprocess.run([sys.executable, os.path.join(K.ROOT, "tools", "eval_quant_policy.py"), "--vec-normalize", "x.npz"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--vec-normalize goes with --actor" in r.stderr, r.stderr[-500:]


def test_sample_indices_are_the_plain_samples():
    """the normalising sample draws brs_replay_sample's cells: the reference's idx is sample_indices' at the buffer's seed and draw"""
    n, m = 63, 33
    s = V.reference(n, m)
    rows, envs = RO.sample_indices(V.SEED, V.draw_of(n), m, V.CAP, n)
    assert np.array_equal(s.idx[:, 0], rows) and np.array_equal(s.idx[:, 1], envs)
