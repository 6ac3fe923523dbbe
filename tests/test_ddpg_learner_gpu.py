"""The DDPG learner on the device (include/brs_policy.h: brs_ddpg_learner_*): the HIP kernels against fp64 torch
autograd (tests/ref_ddpg_learner.py) and against the host build of the same source (tests/ddpglearnerhost), on the cases of
tests/ddpg_learner_cases.py at the kernels' own tile edges.  Every output sits between guard zones that must stay untouched, the
handle's scratch is filled with NaN before the call (every word of it, read back to make sure), and every result must come back with identical bytes from a second
handle."""
import os
import sys

import numpy as np
import pytest

import ref_ddpg_learner as RL
import ref_offpolicy as R
from ddpg_learner_cases import (ADAM, GAMMA, GPU_ROWS, GRAD_GATE, HOST_ROWS_MAX, SPLIT_BIG, SPLIT_CASES, SPLIT_SEQUENCE, STEP_ROWS, STEPS, WEIGHT_SETS,
                                HostDDPG, block_distances, build_host, check_gradient, check_trajectory, host_actor_grad, host_critic_grad, learner_case,
                                references, trajectory_case)
from offpolicy_cases import ROOT, gate
from test_offpolicy_gpu import Guarded, _cuda

pytestmark = pytest.mark.gpu
NC, NA = RL.NCRITIC, RL.NACTOR


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("ddpglearnerhost"))


def _learner(max_batch):
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner
    return DeviceDDPGLearner(device=0, max_batch=max_batch, **ADAM)


@pytest.fixture(scope="module")
def big():
    lrn = _learner(1024)
    yield lrn
    lrn.close()


@pytest.fixture(scope="module")
def huge():
    """max_batch = 8,448: its rows are longer than the padded batch (ld != mp) at every row of ddpg_learner_cases.SPLIT_ROWS"""
    lrn = _learner(SPLIT_BIG)
    yield lrn
    lrn.close()


def _poison(lrn):
    """fill the handle's whole allocation (activation images and partial rows) with NaN through the HIP runtime the library is
    linked to, and read three places back: a call that returns finite numbers afterwards has read nothing it did not write"""
    import ctypes as C
    import torch
    from balance_robot_mujoco_rl_amd import _lib
    # the HIP runtime libbrs_hip.so is linked to -- the one that made the allocation -- looked up through the library's handle
    # (dlsym searches its dependencies); another copy of the runtime loaded by name would not know the pointer
    L = _lib.lib()
    memset = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_size_t)(("hipMemsetD32", L))
    memcpy = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)(("hipMemcpy", L))
    sync = C.CFUNCTYPE(C.c_int)(("hipDeviceSynchronize", L))
    ptr, size = lrn.scratch()
    assert ptr and size >= 4 * 1092 * 128
    torch.cuda.synchronize()
    assert memset(ptr, 0x7fc00000, size // 4) == 0 and sync() == 0
    for offset in (0, (size // 8) * 4, size - 256):
        back = np.zeros(64, np.float32)
        assert memcpy(back.ctypes.data, ptr + offset, 256, 2) == 0 and np.isnan(back).all()   # 2: device to host


def _grads(lrn, c, dev):
    gc, ga = Guarded((NC + 2,)), Guarded((NA + 2,))
    lrn.critic_grad(dev["critic"], dev["obs"], dev["act"], dev["y"], out=gc.t)
    crit = gc.np()   # the scratch is shared: the critic's buffer is complete before the actor's call is enqueued on the same stream
    lrn.actor_grad(dev["actor"], dev["critic"], dev["obs"], out=ga.t)
    assert gc.intact() and ga.intact()
    return crit, ga.np()


# --------------------------------------------------------------------------------------- 1. the two gradients
def _check_gradients(host, big, n, kind, with_host=True):
    c = learner_case(n, kind)
    c64, a64, c32, a32 = references(n, kind)
    dev = {k: _cuda(c[k]) for k in ("obs", "act", "y", "actor", "critic")}
    own = _learner(n)                       # max_batch == m, fresh
    gc, ga = _grads(own, c, dev)
    own.close()
    _poison(big)                            # a larger max_batch, every word of its allocation NaN
    gc_big, ga_big = _grads(big, c, dev)
    assert np.isfinite(gc).all() and np.isfinite(ga).all()
    assert gc.tobytes() == gc_big.tobytes() and ga.tobytes() == ga_big.tobytes()   # nothing stale read, the handle's size does not matter
    check_gradient(f"n={n} {kind} critic", gc, c64, c32, R.CRITIC_SIZES, gate)
    check_gradient(f"n={n} {kind} actor", ga, a64, a32, R.ACTOR_SIZES, gate)
    if not with_host:
        return
    hc, ha = host_critic_grad(host, c["critic"], c["obs"], c["act"], c["y"]), host_actor_grad(host, c["actor"], c["critic"], c["obs"])
    dc, da = block_distances(gc[:NC], hc[:NC], R.CRITIC_SIZES), block_distances(ga[:NA], ha[:NA], R.ACTOR_SIZES)
    print(f"n={n} {kind}: largest block distance from the host build {max(dc.values()):.3g} (critic), {max(da.values()):.3g} (actor)")
    assert max(dc.values()) <= GRAD_GATE and max(da.values()) <= GRAD_GATE
    gate(gc[NC:], hc[NC:], "critic statistics against the host build"); gate(ga[NA:], ha[NA:], "actor statistics against the host build")


@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("n", GPU_ROWS)
def test_gradients_against_fp64_and_the_host_build(host, big, n, kind):
    _check_gradients(host, big, n, kind)    # big: max_batch = 1,024


@pytest.mark.parametrize("n,kind", SPLIT_CASES)
def test_gradients_at_every_split_geometry(host, huge, n, kind):
    """the assertions of test_gradients_against_fp64_and_the_host_build at the rows of ddpg_learner_cases.SPLIT_ROWS: two to eight
    partial rows, even and uneven splits, a last split with one real row, on a handle of max_batch = 8,448 (ld != mp everywhere).
    The host build's plain loops take 2 s (critic) and 5 s (actor) per gradient at 8,192 rows on a CPU, so the comparison with the
    host build is made up to 2,049 rows; the fp64 gate and every other assertion hold at all rows."""
    _check_gradients(host, huge, n, kind, with_host=n <= HOST_ROWS_MAX)


def test_identical_bytes_and_no_leftover_scratch(big):
    """two runs return identical bytes; 1,000 rows and then 33 on the same handle return what a fresh handle returns for the 33"""
    c1000, c33 = learner_case(1000, "init"), learner_case(33, "init")
    d1000, d33 = ({k: _cuda(c[k]) for k in ("obs", "act", "y", "actor", "critic")} for c in (c1000, c33))
    _poison(big)
    first, second = _grads(big, c1000, d1000), _grads(big, c1000, d1000)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    after = _grads(big, c33, d33)
    fresh_handle = _learner(33)
    fresh = _grads(fresh_handle, c33, d33)
    fresh_handle.close()
    assert after[0].tobytes() == fresh[0].tobytes() and after[1].tobytes() == fresh[1].tobytes()


def test_no_leftover_between_split_geometries_on_one_handle(huge):
    """8,193 -> 513 -> 33 -> 2,049 -> 769 rows on the NaN-filled large handle (8 partial rows, then 2, none, 6 and 3): every result
    is what a fresh handle of exactly that size returns, byte for byte, and the sequence a second time returns the same bytes"""
    cases = {n: learner_case(n, "init") for n in SPLIT_SEQUENCE}
    devs = {n: {k: _cuda(c[k]) for k in ("obs", "act", "y", "actor", "critic")} for n, c in cases.items()}
    fresh = {}
    for n in SPLIT_SEQUENCE:
        own = _learner(n)
        fresh[n] = _grads(own, cases[n], devs[n])
        own.close()
        assert np.isfinite(fresh[n][0]).all() and np.isfinite(fresh[n][1]).all()
    _poison(huge)
    for run in range(2):
        for n in SPLIT_SEQUENCE:
            gc, ga = _grads(huge, cases[n], devs[n])
            assert gc.tobytes() == fresh[n][0].tobytes() and ga.tobytes() == fresh[n][1].tobytes(), (run, n)


def test_calls_are_refused_past_max_batch():
    import torch
    from balance_robot_mujoco_rl_amd import BrsError
    lrn = _learner(32)
    z = lambda *s: torch.zeros(s, device="cuda")
    with pytest.raises(BrsError, match="brs_ddpg_learner_critic_grad: m exceeds the handle's max_batch"):
        lrn.critic_grad(z(NC), z(33, 6), z(33, 2), z(33))
    with pytest.raises(BrsError, match="brs_ddpg_learner_actor_grad: m exceeds the handle's max_batch"):
        lrn.actor_grad(z(NA), z(NC), z(33, 6))
    with pytest.raises(ValueError):
        lrn.critic_grad(z(NC).double(), z(8, 6), z(8, 2), z(8))
    lrn.close()


# --------------------------------------------------------------------------------------- 2. apply
def test_apply_against_the_host_build_and_torch_adam(host, big):
    """five steps from given gradients, parameters from zero: params, m, v and the target equal the host build's byte for byte;
    the update agrees with torch.optim.Adam to 1e-6 per block; guard zones around all five arrays; no target, no target written"""
    rng = np.random.default_rng(5)
    h = HostDDPG(host, np.zeros(NA, np.float32), np.zeros(NC, np.float32), **ADAM)
    t = RL.TorchAdam(np.zeros(NC, np.float32), **ADAM)
    p, tg, g = Guarded((NC,), fill=0.0), Guarded((NC,), fill=0.0), Guarded((NC + 2,), fill=0.0)
    big.load_state_dict({"m_critic": np.zeros(NC, np.float32), "v_critic": np.zeros(NC, np.float32), "m_actor": np.zeros(NA, np.float32),
                         "v_actor": np.zeros(NA, np.float32), "steps_critic": 0, "steps_actor": 0})
    m, v = Guarded((NC,), fill=0.0), Guarded((NC,), fill=0.0)
    big.m_critic, big.v_critic = m.t, v.t
    worst = 0.0
    for step in range(5):
        grad = (rng.standard_normal(NC + 2) * (0.02 if step % 2 else 0.002)).astype(np.float32)
        g.t.copy_(_cuda(grad))
        before, before_t = p.np(), t.p.detach().numpy().copy()
        big.apply_critic(p.t, tg.t, grad=g.t); h.apply("critic", grad); t.apply(grad[:NC])
        for mine, theirs, name in ((p.np(), h.flat["critic"], "params"), (m.np(), h.mom["critic"][0], "m"), (v.np(), h.mom["critic"][1], "v"),
                                   (tg.np(), h.flat["critic_target"], "target")):
            assert mine.tobytes() == theirs.tobytes(), (step, name, float(np.abs(mine - theirs).max()))
        err = block_distances(p.np().astype(np.float64) - before, t.p.detach().numpy().astype(np.float64) - before_t, R.CRITIC_SIZES)
        worst = max(worst, max(err.values()))
        assert max(err.values()) <= 1e-6, (step, err)
    print(f"largest per-block relative error of an Adam update against torch = {worst:.3g}")
    assert all(x.intact() for x in (p, tg, g, m, v)) and big.steps_critic == 5
    frozen = tg.np()
    big.apply_critic(p.t, None, grad=g.t)
    assert tg.np().tobytes() == frozen.tobytes() and p.np().tobytes() != h.flat["critic"].tobytes()
    sd = big.state_dict()
    assert sd["steps_critic"] == 6 and sd["m_critic"].cpu().numpy().tobytes() == m.np().tobytes()
    big.load_state_dict({**sd, "steps_critic": 0})


# --------------------------------------------------------------------------------------- 3. whole steps
def test_five_full_steps_chained_with_the_td_target(host):
    """brs_ddpg_td_target -> critic_grad -> apply -> actor_grad -> apply, five times on the kernels and on the host builds, each
    against the same chain in fp64 within the CPU test's gate (4 x fp32 torch's distance, floored)"""
    import tempfile
    from balance_robot_mujoco_rl_amd import DeviceDDPGNets
    import offpolicy_cases as OC
    case = trajectory_case("init", chain=True)
    oh = OC.build_host(tempfile.mkdtemp())
    h = HostDDPG(host, case["actor"], case["critic"], **ADAM)
    nets, lrn = DeviceDDPGNets(device=0), _learner(STEP_ROWS)
    flat = {k: _cuda(case[k.split("_")[0]]) for k in ("actor", "critic", "actor_target", "critic_target")}
    for s in range(STEPS):
        sl = slice(s * STEP_ROWS, (s + 1) * STEP_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        y = nets.td_target(flat["actor_target"], flat["critic_target"], _cuda(no), _cuda(rew), _cuda(done), GAMMA)
        lrn.step(flat, _cuda(obs), _cuda(act), y)
        h.step(obs, act, OC.host_td_target(oh, h.flat["actor_target"], h.flat["critic_target"], no, rew, done, GAMMA))
    mine = {k: v.cpu().numpy() for k, v in flat.items()}
    worst_h = check_trajectory("host chain", h.flat, case)
    worst = check_trajectory("kernels", mine, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| after five chained steps: kernels {worst:.3g}, host build {worst_h:.3g}")
    s = lrn.stats()
    assert all(np.isfinite(v) for v in s.values()) and s["critic_loss"] > 0 and (lrn.steps_critic, lrn.steps_actor) == (5, 5)
    nets.close(); lrn.close()


def test_actor_gradient_uses_the_critic_it_is_given():
    """step 0 of the trajectory case: the actor gradient through the UPDATED critic differs from the one through the old critic,
    and each matches the fp64 gradient through its own critic"""
    case = trajectory_case("init")
    sl = slice(0, STEP_ROWS)
    obs, act, y = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "y"))
    lrn = _learner(STEP_ROWS)
    actor, critic, target = _cuda(case["actor"]), _cuda(case["critic"]), _cuda(case["critic"])
    g_old = lrn.actor_grad(actor, critic, _cuda(obs)).cpu().numpy()
    lrn.critic_grad(critic, _cuda(obs), _cuda(act), _cuda(y)); lrn.apply_critic(critic, target)
    new_critic = critic.cpu().numpy()
    g_new = lrn.actor_grad(actor, critic, _cuda(obs)).cpu().numpy()
    lrn.close()
    assert not np.array_equal(new_critic, case["critic"])
    moved = block_distances(g_new[:NA], g_old[:NA], R.ACTOR_SIZES)
    print(f"the actor gradient moved by {min(moved.values()):.3g} .. {max(moved.values()):.3g} of its block norms with the critic's step")
    assert min(moved.values()) > 100 * GRAD_GATE
    for what, g, cr in (("old critic", g_old, case["critic"]), ("updated critic", g_new, new_critic)):
        check_gradient(what, g, RL.actor_grad(case["actor"], cr, obs), RL.actor_grad(case["actor"], cr, obs, dtype=__import__("torch").float32),
                       R.ACTOR_SIZES, gate)


def test_tool_with_device_learner_end_to_end():
    """tools/train_ddpg_torch.py --device-data --device-learner on 256 Env01-v1 envs for 40 env steps: it runs, takes as many
    updates as the torch learner, everything is finite, the targets moved by tau-sized amounts.  No learning-quality gate."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ddpg_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGLearner
    runs = {}
    for mode in ("device", "torch"):
        sim = BatchedSim("Env01-v1", 256, seed=0, auto_reset=True)
        model = T.DDPG(sim.device, seed=0)
        start = {k: v.clone() for k, v in model.flat.items()}
        data = T.DeviceData(sim, model, 16, 0.1, 0)
        learner = DeviceDDPGLearner(device=sim.device, max_batch=256, lr=1e-3, tau=0.005) if mode == "device" else None
        log = {}
        updates = T.train(sim, model, data, steps=40, batch=256, learning_starts=100, gradient_steps=1, train_freq=4, log=log, learner=learner)
        torch.cuda.synchronize()
        runs[mode] = (updates, log, {k: float((model.flat[k] - start[k]).abs().max()) for k in start}, model)
        if learner is not None:
            assert (learner.steps_critic, learner.steps_actor) == (updates, updates)
            learner.close()
        sim.close()
    updates, log, moved, model = runs["device"]
    assert updates == runs["torch"][0] == 10
    assert all(torch.isfinite(v).all() for v in model.flat.values())
    assert np.isfinite(log["critic_loss_last"]) and np.isfinite(log["actor_loss_last"]) and log["critic_loss_last"] > 0
    lr, tau = 1e-3, 0.005
    for net in ("actor", "critic"):
        # Adam moves an element by at most lr (1 - beta1) / sqrt(1 - beta2) = 3.2 lr per step, so the online network is within
        # 3.2 lr k of its start after k steps and the target has gone at most tau times the sum of that
        assert 0 < moved[net] <= 3.2 * lr * updates, (net, moved)
        assert 0 < moved[net + "_target"] <= tau * 3.2 * lr * updates * (updates + 1) / 2, (net, moved)
        assert moved[net + "_target"] < 0.1 * moved[net]
        assert 0.2 < moved[net] / runs["torch"][2][net] < 5   # the same recipe: the torch learner moved the network about as far
    # the modules' parameters are views of the vectors the kernels wrote
    assert model.actor[0].weight.data_ptr() == model.flat["actor"].data_ptr()
