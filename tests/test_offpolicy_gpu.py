"""The DDPG data path on the device (include/brs_policy.h: brs_ddpg_*, brs_replay_*): the HIP kernels against
the fp64 numpy restatement (tests/ref_offpolicy.py) and against the host build of the same source (tests/offpolicyhost), on the
cases of tests/offpolicy_cases.py plus the kernel's own tile edges.  Every output and every storage array sits between guard
rows that must stay untouched; every result is computed twice and must come back with identical bytes."""
import os
import sys

import numpy as np
import pytest

import ref_offpolicy as R
from offpolicy_cases import (ADD_ORDER, BUFFER_CASES, FORWARD_ROWS, GAMMA, KERNEL_ROWS, ROOT, SAMPLE_M, SEED, SENTINEL, SENTINEL_DONE, WEIGHT_SETS,
                             HostBuffer, build_host, conditioned, env_steps, gate, host_act, host_q, host_td_target, reference_buffer)

pytestmark = pytest.mark.gpu

GUARD_FILL = {np.dtype(np.float32): -3.25, np.dtype(np.uint8): 173, np.dtype(np.int32): -99}


class Guarded:
    """a device tensor of `shape` between two guard zones filled with a sentinel; `guard` elements each (65 puts a float32 array
    on a 4-byte boundary only: the kernels' scalar paths)"""

    def __init__(self, shape, dtype=np.float32, guard=64, fill=None):
        import torch
        self.guard, self.size = guard, int(np.prod(shape))
        tdtype = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32}[np.dtype(dtype)]
        self.sentinel = GUARD_FILL[np.dtype(dtype)]
        self.base = torch.full((self.size + 2 * guard,), self.sentinel, dtype=tdtype, device="cuda")
        self.t = self.base[guard:guard + self.size].view(*shape)
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        b = self.base.cpu().numpy()
        return bool(np.all(b[:self.guard] == self.sentinel) and np.all(b[self.guard + self.size:] == self.sentinel))

    def np(self):
        return self.t.cpu().numpy()


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("offpolicyhost"))


@pytest.fixture(scope="module")
def nets():
    from balance_robot_mujoco_rl_amd import DeviceDDPGNets
    d = DeviceDDPGNets(device=0, seed=SEED)
    yield d
    d.close()


# --------------------------------------------------------------------------------------- 1. the forwards
@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("n", sorted(set(FORWARD_ROWS + KERNEL_ROWS + (1000,))))
def test_kernel_forwards_against_fp64_and_the_host_build(nets, host, n, kind):
    import torch
    c = conditioned(n, kind)
    actor, critic, obs, act, rew, done = (_cuda(c[k]) for k in ("actor", "critic", "obs", "act", "reward", "done"))
    runs = []
    for _ in range(2):
        a, mu, q, y = Guarded((n, 2)), Guarded((n, 2)), Guarded((n,)), Guarded((n,))
        nets.act(actor, obs, 0, 0.0, out=a.t, mean=mu.t)
        nets.q(critic, obs, act, out=q.t)
        nets.td_target(actor, critic, obs, rew, done, GAMMA, out=y.t)
        torch.cuda.synchronize()
        assert all(g.intact() for g in (a, mu, q, y)), "a kernel wrote outside its output"
        runs.append([g.np() for g in (a, mu, q, y)])
    for x, z in zip(*runs):
        assert x.tobytes() == z.tobytes(), "two runs on the same inputs differ"
    a, mu, q, y = runs[0]
    assert a.tobytes() == mu.tobytes()   # sigma = 0
    gate(mu, R.actor(c["actor"], c["obs"]), f"n={n} {kind} mean")
    gate(q, R.critic(c["critic"], c["obs"], c["act"]), f"n={n} {kind} q")
    gate(y, R.td_target(c["actor"], c["critic"], c["obs"], c["reward"], c["done"], GAMMA), f"n={n} {kind} y")
    # the host build of the same source, on the same inputs
    gate(mu, host_act(host, c["actor"], c["obs"], SEED, 0, 0, 0.0)[1], "mean against the host build")
    gate(q, host_q(host, c["critic"], c["obs"], c["act"]), "q against the host build")
    gate(y, host_td_target(host, c["actor"], c["critic"], c["obs"], c["reward"], c["done"], GAMMA), "y against the host build")
    # the one-launch chain is the composition of the other two entry points
    qn = nets.q(critic, obs, nets.act(actor, obs, 0, 0.0)).cpu().numpy()
    comp = c["reward"].astype(np.float64) + (1.0 - c["done"]) * GAMMA * qn.astype(np.float64)
    assert np.all(np.abs(y - comp) <= 1e-6 * np.maximum(1.0, np.abs(comp)))
    if n > 1:
        assert c["done"].sum() > 0
    assert y[c["done"] == 1].tobytes() == c["reward"][c["done"] == 1].tobytes()   # y == r exactly


# --------------------------------------------------------------------------------------- 2. noise
def test_kernel_noise_clip_modes_and_sharding(nets, host):
    import torch
    from balance_robot_mujoco_rl_amd import DeviceDDPGNets
    c = conditioned(65, "init")
    actor = _cuda(c["actor"])
    obs_np = np.concatenate([c["obs"], c["obs"][::-1]])   # n = 130: two workgroups, the second one a partial wave
    obs, n, sigma, step = _cuda(obs_np), 130, 0.1, 5
    base = DeviceDDPGNets(device=0, seed=SEED, env_index_base=1000)

    def run(d, o, st, sg, random=False):
        k = o.shape[0]
        a, m, z = Guarded((k, 2)), Guarded((k, 2)), Guarded((k, 2))
        d.act(None if random else actor, o, st, sg, random=random, out=a.t, mean=m.t, noise=z.t)
        torch.cuda.synchronize()
        assert a.intact() and m.intact() and z.intact()
        return a.np(), m.np(), z.np()
    a, m, z = run(base, obs, step, sigma)
    a64, m64, z64 = R.act(c["actor"], obs_np, SEED, 1000, step, sigma)
    assert np.abs(z - z64).max() <= 1e-5   # derivation: tests/test_offpolicy_cpu.py
    gate(m, m64, "mean")
    formed = np.clip(m + np.float32(sigma) * z, np.float32(-1), np.float32(1))
    assert np.abs(a - formed).max() <= 1e-7 and np.abs(a - a64).max() <= 1e-5
    a0, m0, _ = run(base, obs, step, 0.0)
    assert a0.tobytes() == m0.tobytes() == m.tobytes()
    ar, mr, zr = run(base, obs, step, sigma, random=True)
    _, mr64, _ = R.act(None, [None] * n, SEED, 1000, step, sigma, random=True)
    assert np.array_equal(mr.astype(np.float64), mr64) and mr.min() >= -1 and mr.max() <= 1 and zr.tobytes() == z.tobytes()
    assert np.abs(ar - np.clip(mr + np.float32(sigma) * zr, np.float32(-1), np.float32(1))).max() <= 1e-7 and np.abs(ar).max() <= 1.0
    hr = host_act(host, None, None, SEED, 1000, step, sigma, random=True, n=n)
    assert hr[1].tobytes() == mr.tobytes() and np.abs(hr[2] - zr).max() <= 1e-5
    assert run(base, obs, step, 5.0)[0].min() == -1.0
    _, _, z_step = run(base, obs, step + 1, sigma)
    assert not np.array_equal(z_step, z) and len({tuple(r) for r in z}) == n
    # 65 + 65 with env_index_base 0 and 65: the bytes of the single call
    lo, hi = DeviceDDPGNets(device=0, seed=SEED, env_index_base=0), DeviceDDPGNets(device=0, seed=SEED, env_index_base=65)
    whole = run(lo, obs, step, sigma)
    parts = run(lo, obs[:65].contiguous(), step, sigma), run(hi, obs[65:].contiguous(), step, sigma)
    for w, p, q in zip(whole, *parts):
        assert w.tobytes() == np.concatenate([p, q]).tobytes()
    assert not np.array_equal(whole[2], z)   # another base: other envs, other draws
    for d in (base, lo, hi):
        d.close()


# --------------------------------------------------------------------------------------- 3. the buffer
class GuardedBuffer:
    """DeviceReplayBuffer whose five storage tensors are replaced by guarded ones, pre-filled with the sentinel"""

    def __init__(self, n, cap, guard=64):
        from balance_robot_mujoco_rl_amd import DeviceReplayBuffer
        from balance_robot_mujoco_rl_amd.offpolicy import _storage
        self.b = DeviceReplayBuffer(n, cap, device=0, seed=SEED)
        self.g = [Guarded((cap, n, 6), guard=guard, fill=SENTINEL), Guarded((cap, n, 6), guard=guard, fill=SENTINEL),
                  Guarded((cap, n, 2), guard=guard, fill=SENTINEL), Guarded((cap, n), guard=guard, fill=SENTINEL),
                  Guarded((cap, n), np.uint8, guard=guard, fill=SENTINEL_DONE)]
        self.b.obs, self.b.next_obs, self.b.action, self.b.reward, self.b.done = (g.t for g in self.g)
        self.b._store = _storage(*(g.t for g in self.g))

    def add(self, s):
        self.b.add(*[_cuda(s[k]) for k in ADD_ORDER])

    def arrays(self):
        return [g.np() for g in self.g]

    def intact(self):
        return all(g.intact() for g in self.g)


# the issue's three (odd n: the scalar kernel) + n % 4 == 0 for the 16-byte kernel, one of them with more than one workgroup,
# and the same n on a 4-byte boundary (falls back to the scalar kernel)
@pytest.mark.parametrize("n,cap,guard", [(n, cap, 64) for n, cap in BUFFER_CASES] + [(64, 3, 64), (260, 2, 64), (64, 2, 65)])
def test_kernel_buffer_byte_for_byte(host, n, cap, guard):
    import torch
    steps = env_steps(n, 2 * cap + 1)
    gb, hb = GuardedBuffer(n, cap, guard), HostBuffer(host, n, cap)
    for t, s in enumerate(steps):
        before, pos = gb.arrays(), gb.b.pos
        gb.add(s); hb.add(s)
        torch.cuda.synchronize()
        assert gb.intact()
        ref = reference_buffer(n, cap, steps[:t + 1])
        for a, b, h, r in zip(gb.arrays(), before, hb.arrays, ref.arrays()):
            others = np.arange(cap) != pos
            assert a[others].tobytes() == b[others].tobytes()     # an add changes row pos only (sentinel rows included)
            assert a.tobytes() == h.tobytes()                     # the host build: identical bytes
            filled = np.arange(cap) < ref.rows
            assert a[filled].tobytes() == r[filled].tobytes()     # the yardstick
        assert (gb.b.pos, gb.b.full, gb.b.rows) == (ref.pos, ref.full, ref.rows) and len(gb.b) == ref.rows * n


# --------------------------------------------------------------------------------------- 4. sampling
def _filled(host, n, cap, rows, guard=64):
    import torch
    gb, hb = GuardedBuffer(n, cap, guard), HostBuffer(host, n, cap)
    for s in env_steps(n, rows):
        gb.add(s); hb.add(s)
    torch.cuda.synchronize()
    return gb, hb


def _sample(gb, m, draw, guard=64):
    import torch
    out = [Guarded((m, 6), guard=guard), Guarded((m, 6), guard=guard), Guarded((m, 2), guard=guard), Guarded((m,), guard=guard),
           Guarded((m,), np.uint8, guard=guard)]
    idx = Guarded((m, 2), np.int32, guard=guard)
    gb.b.draw = draw
    gb.b.sample(m, out=tuple(g.t for g in out), idx=idx.t)
    torch.cuda.synchronize()
    assert all(g.intact() for g in out) and idx.intact() and gb.intact()
    return [g.np() for g in out], idx.np()


@pytest.mark.parametrize("guard", [64, 65])
def test_kernel_sample_indices_rows_and_draws(host, guard):
    n, cap = 65, 4
    gb, hb = _filled(host, n, cap, cap, guard)
    arrays = gb.arrays()
    for m in SAMPLE_M:
        got, idx = _sample(gb, m, 3, guard)
        rows, envs = R.sample_indices(SEED, 3, m, cap, n)
        assert np.array_equal(idx[:, 0], rows) and np.array_equal(idx[:, 1], envs)
        for g, arr in zip(got, arrays):
            assert g.tobytes() == arr[rows, envs].tobytes()
        hgot, hidx = hb.sample(m, draw=3)
        assert hidx.tobytes() == idx.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(got, hgot))
        again, idx2 = _sample(gb, m, 3, guard)
        assert idx2.tobytes() == idx.tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
        assert gb.b.draw == 4   # the counter moved on
        _, idx3 = _sample(gb, m, 4, guard)
        assert m < 64 or idx3.tobytes() != idx.tobytes()


def test_kernel_sample_from_a_buffer_that_is_not_full(host):
    n, cap = 65, 4
    gb, hb = _filled(host, n, cap, 2)
    assert gb.b.rows == 2 and len(gb.b) == 2 * n
    (o, no, a, r, d), idx = _sample(gb, 1000, 0)
    assert idx[:, 0].max() == 1 and idx[:, 0].min() == 0 and 0 <= idx[:, 1].min() and idx[:, 1].max() < n
    assert not np.any(r == SENTINEL) and not np.any(d == SENTINEL_DONE)
    # size = 1
    gb1, _ = _filled(host, n, cap, 1)
    _, idx1 = _sample(gb1, 256, 0)
    assert np.all(idx1[:, 0] == 0) and np.unique(idx1[:, 1]).size > 32
    from balance_robot_mujoco_rl_amd import DeviceReplayBuffer
    with pytest.raises(ValueError):
        DeviceReplayBuffer(4, 4).sample(8)   # empty


# --------------------------------------------------------------------------------------- 5. the collector
def test_collector_fills_the_buffer_like_a_stepwise_loop():
    """256 Env03-v2 envs, cap 16, 40 steps with uniform actions: the buffer wraps and episodes end.  The fused loop against a loop
    of separate calls that feeds the numpy yardstick"""
    import torch
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGNets, DeviceOffPolicyCollector, DeviceReplayBuffer, EpisodeMonitor
    n, cap, steps = 256, 16, 40
    actor = _cuda(conditioned(1, "init")["actor"])

    def make():
        return BatchedSim("Env03-v2", n, seed=3, auto_reset=True), DeviceDDPGNets(device=0, seed=SEED)
    sim, nets = make()
    replay = DeviceReplayBuffer(n, cap, device=0, seed=SEED)
    mon = EpisodeMonitor(n, device=0, max_len=int(sim.max_episode_steps))
    col = DeviceOffPolicyCollector(sim, nets, actor, replay, sigma=0.1, monitor=mon)
    col.collect(25, random=True).collect(15, random=True)
    torch.cuda.synchronize()
    assert mon.stats().steps == steps and col.step == steps and replay.full and replay.pos == steps % cap
    fused = [t.cpu().numpy() for t in (replay.obs, replay.next_obs, replay.action, replay.reward, replay.done)]
    sim.close(); nets.close(); mon.close()
    sim, nets = make()
    ref = R.Buffer(n, cap)
    last = sim.reset().clone()
    terminated_rows = time_limit_rows = 0
    for t in range(steps):
        a = nets.act(None, last, t, 0.1, random=True)
        obs, rew, term, trunc, tobs = sim.step(a)
        host_side = [x.cpu().numpy().copy() for x in (last, a, obs, tobs, rew, term, trunc)]
        ref.add(*host_side)
        terminated_rows += int((host_side[5] != 0).sum()); time_limit_rows += int(((host_side[6] != 0) & (host_side[5] == 0)).sum())
        last = obs.clone()
    sim.close(); nets.close()
    assert terminated_rows >= 1, "no episode terminated in 40 steps: the terminal-observation substitution was not exercised"
    print(f"collector: {terminated_rows} terminated rows, {time_limit_rows} time-limit rows in {steps} steps of {n} envs")
    for got, want, name in zip(fused, ref.arrays(), ("obs", "next_obs", "action", "reward", "done")):
        assert got.tobytes() == want.tobytes(), name
    assert int(fused[4].sum()) >= 1


# --------------------------------------------------------------------------------------- 6. end to end
def test_tool_with_device_data_end_to_end():
    """tools/train_ddpg_torch.py --device-data: 256 Env01-v1 envs, 40 collected steps, 10 gradient steps at batch 256.  It finishes,
    parameters and targets change, everything is finite, the monitor counted every step.  No learning-quality gate."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ddpg_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor
    sim = BatchedSim("Env01-v1", 256, seed=0, auto_reset=True)
    model = T.DDPG(sim.device, seed=0)
    start = {k: v.clone() for k, v in model.flat.items()}
    mon = EpisodeMonitor(256, device=0, max_len=int(sim.max_episode_steps))
    data = T.DeviceData(sim, model, 16, 0.1, 0)
    log = {}
    updates = T.train(sim, model, data, steps=40, batch=256, learning_starts=100, gradient_steps=1, train_freq=4, monitor=mon, log=log)
    torch.cuda.synchronize()
    assert updates == 10 and mon.stats().steps == 40 and data.replay.full
    for k, v in model.flat.items():
        assert torch.isfinite(v).all() and not torch.equal(v, start[k]), k
    assert np.isfinite(log["critic_loss_last"]) and np.isfinite(log["actor_loss_last"])
    for t in (data.replay.obs, data.replay.next_obs, data.replay.action, data.replay.reward):
        assert torch.isfinite(t).all()
    # the kernels read what Adam and lerp_ wrote: the actor the collector uses IS the module's parameter storage
    assert model.actor[0].weight.data_ptr() == model.flat["actor"].data_ptr()
    obs = data.replay.obs[0]
    with torch.no_grad():
        want = model.actor(obs)
    got = data.nets.act(model.flat["actor"], obs, 0, 0.0)
    assert torch.allclose(got, want, atol=1e-5, rtol=0)
    mon.close(); sim.close(); data.nets.close()
