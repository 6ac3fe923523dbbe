"""TD3 on the device (include/brs_policy.h: brs_td3_td_target, brs_ddpg_learner_create_twin,
brs_ddpg_learner_twin_critic_grad): the HIP kernels against the fp64 restatement (tests/ref_td3.py) and against the host build of the
same source (tests/td3host), on the cases of tests/td3_cases.py at the kernels' own tile edges.  Every output sits between guard
zones that must stay untouched, the twin handle's scratch is filled with NaN before the call, and block k of the twin gradient must
be the single-critic call's result byte for byte."""
import os
import sys

import numpy as np
import pytest

import ref_offpolicy as R
import td3_cases as TC
from ddpg_learner_cases import (ADAM, GPU_ROWS, GRAD_GATE, HOST_ROWS_MAX, SPLIT_BIG, SPLIT_CASES, SPLIT_SEQUENCE, WEIGHT_SETS, block_distances,
                                check_gradient)
from offpolicy_cases import GAMMA, ROOT, SEED, gate
from test_ddpg_learner_gpu import _poison
from test_offpolicy_gpu import Guarded, _cuda

pytestmark = pytest.mark.gpu
NC, NA = TC.NC, TC.NA


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TC.build_host(tmp_path_factory.mktemp("td3host"))


@pytest.fixture(scope="module")
def nets():
    from balance_robot_mujoco_rl_amd import DeviceDDPGNets
    d = DeviceDDPGNets(device=0, seed=SEED)
    yield d
    d.close()


def _twin(max_batch, **kw):
    from balance_robot_mujoco_rl_amd import DeviceTD3Learner
    return DeviceTD3Learner(device=0, max_batch=max_batch, **{**ADAM, **kw})


def _single(max_batch):
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner
    return DeviceDDPGLearner(device=0, max_batch=max_batch, **ADAM)


@pytest.fixture(scope="module")
def big():
    lrn = _twin(1024)
    yield lrn
    lrn.close()


@pytest.fixture(scope="module")
def huge():
    """a twin handle of max_batch = 8,448: ld != mp at every row of ddpg_learner_cases.SPLIT_ROWS"""
    lrn = _twin(SPLIT_BIG)
    yield lrn
    lrn.close()


def _target(nets, c, dev, policy_noise, noise_clip, draw, extras=True):
    import torch
    m = len(c["next_obs"])
    y, a, z = Guarded((m,)), Guarded((m, 2)), Guarded((m, 2))
    nets.td3_target(dev["actor"], dev["critics"], dev["next_obs"], dev["reward"], dev["done"], GAMMA, policy_noise, noise_clip, draw, out=y.t,
                    next_action=a.t if extras else None, noise=z.t if extras else None)
    torch.cuda.synchronize()
    assert y.intact() and a.intact() and z.intact(), "the kernel wrote outside its outputs"
    return y.np(), a.np(), z.np()


# --------------------------------------------------------------------------------------- 1. the target
@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("m", GPU_ROWS)
def test_target_against_fp64_and_the_host_build(nets, host, m, kind):
    TC.assert_branch_coverage(TC.coverage_cases())   # a condition on the inputs, on the fp64 reference, before anything is compared
    for pair in (TC.SB3_NOISE,) + ((TC.TIGHT_NOISE,) if m in (33, 257) else ()):
        c = TC.target_case(m, kind, pair)
        dev = {k: _cuda(c[k]) for k in ("actor", "critics", "next_obs", "reward", "done")}
        y, a, z = _target(nets, c, dev, pair[0], pair[1], 0)
        what = f"m={m} {kind} {pair}"
        gate(z, c["z"], what + " z"); gate(a, c["a"], what + " a'"); gate(y, c["y"], what + " y")
        hy, ha, hz = TC.host_td3_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, pair[0], pair[1], SEED, 0)
        gate(z, hz, what + " z against the host build"); gate(a, ha, what + " a' against the host build"); gate(y, hy, what + " y against the host build")
        ended = c["done"] != 0
        assert y[ended].tobytes() == c["reward"][ended].tobytes() and np.abs(a).max() <= 1.0
        y_only, a_none, z_none = _target(nets, c, dev, pair[0], pair[1], 0, extras=False)
        assert y_only.tobytes() == y.tobytes()
        assert (a_none == np.float32(-3.25)).all() and (z_none == np.float32(-3.25)).all()   # NULL outputs: nothing written


@pytest.mark.parametrize("m", (33, 129, 1000))
def test_target_reduces_to_the_ddpg_target(nets, m):
    """policy_noise = 0 with both halves one critic returns brs_ddpg_td_target's bytes; the same seed and draw twice give identical
    bytes; another draw gives another z"""
    c = TC.target_case(m, "x3", TC.SB3_NOISE)
    one = np.ascontiguousarray(c["critics"][:NC])
    dev = {k: _cuda(c[k]) for k in ("actor", "next_obs", "reward", "done")}
    dev["critics"] = _cuda(np.concatenate([one, one]))
    y = _target(nets, c, dev, 0.0, 0.5, 0)[0]
    ref = nets.td_target(dev["actor"], _cuda(one), dev["next_obs"], dev["reward"], dev["done"], GAMMA).cpu().numpy()
    assert y.tobytes() == ref.tobytes()
    dev["critics"] = _cuda(c["critics"])
    first, second, other = (_target(nets, c, dev, 0.2, 0.5, d) for d in (3, 3, 4))
    for x, w in zip(first, second):
        assert x.tobytes() == w.tobytes()
    assert other[2].tobytes() != first[2].tobytes() and other[0].tobytes() != first[0].tobytes()


# --------------------------------------------------------------------------------------- 2. the twin gradient
def _twin_grad(lrn, dev):
    g = Guarded((2 * NC + 4,))
    lrn.twin_critic_grad(dev["critics"], dev["obs"], dev["act"], dev["y"], out=g.t)
    out = g.np()
    assert g.intact(), "a kernel wrote outside the twin gradient buffer"
    return out


def _dev(c):
    return {k: _cuda(c[k]) for k in ("obs", "act", "y", "actor", "critics")}


def _check_twin_gradient(host, big, n, kind, with_host=True):
    c = TC.twin_case(n, kind)
    g64, g32 = TC.twin_references(n, kind)
    dev = _dev(c)
    own = _twin(n)                          # max_batch == m, fresh
    g = _twin_grad(own, dev)
    own.close()
    _poison(big)                            # a larger max_batch, every word of its allocation NaN
    g_big = _twin_grad(big, dev)
    assert np.isfinite(g).all() and g.tobytes() == g_big.tobytes()   # nothing stale read, the handle's size does not matter
    hg = TC.host_twin_critic_grad(host, c["critics"], c["obs"], c["act"], c["y"]) if with_host else g
    single = _single(n)
    for k, (mine, r64, r32, h) in enumerate(zip(TC.split_twin(g), TC.split_twin(g64), TC.split_twin(g32), TC.split_twin(hg))):
        alone = Guarded((NC + 2,))
        single.critic_grad(_cuda(np.ascontiguousarray(c["critics"][k * NC:(k + 1) * NC])), dev["obs"], dev["act"], dev["y"], out=alone.t)
        assert mine.tobytes() == alone.np().tobytes(), f"block {k} is not the single-critic call's result"
        check_gradient(f"n={n} {kind} critic {k}", mine, r64, r32, R.CRITIC_SIZES, gate)
        if not with_host:
            continue
        d = block_distances(mine[:NC], h[:NC], R.CRITIC_SIZES)
        print(f"n={n} {kind} critic {k}: largest block distance from the host build {max(d.values()):.3g}")
        assert max(d.values()) <= GRAD_GATE
        gate(mine[NC:], h[NC:], f"critic {k} statistics against the host build")
    single.close()


@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("n", GPU_ROWS)
def test_twin_gradient_against_fp64_the_host_build_and_the_single_call(host, big, n, kind):
    _check_twin_gradient(host, big, n, kind)   # big: max_batch = 1,024


@pytest.mark.parametrize("n,kind", SPLIT_CASES)
def test_twin_gradient_at_every_split_geometry(host, huge, n, kind):
    """the assertions of test_twin_gradient_against_fp64_the_host_build_and_the_single_call at the rows of
    ddpg_learner_cases.SPLIT_ROWS: two to eight partial rows of the twin length, even and uneven splits, a last split with one real row,
    on a twin handle of max_batch = 8,448 (ld != mp everywhere).  One host gradient of one critic takes 2 s at 8,192 rows on a CPU
    (the actor's, in the DDPG file, 5 s), so the comparison with the host build is made up to 2,049 rows in both files; the fp64 gate,
    the identity with the single-critic call and every other assertion hold at all rows."""
    _check_twin_gradient(host, huge, n, kind, with_host=n <= HOST_ROWS_MAX)


def test_no_leftover_scratch_between_sizes(big):
    """1,000 rows and then 33 on the same handle return what a fresh handle returns for the 33; two runs return identical bytes"""
    d1000, d33 = _dev(TC.twin_case(1000, "init")), _dev(TC.twin_case(33, "init"))
    _poison(big)
    first, second = _twin_grad(big, d1000), _twin_grad(big, d1000)
    assert first.tobytes() == second.tobytes()
    after = _twin_grad(big, d33)
    fresh_handle = _twin(33)
    fresh = _twin_grad(fresh_handle, d33)
    fresh_handle.close()
    assert after.tobytes() == fresh.tobytes()


def test_no_leftover_between_split_geometries_on_one_twin_handle(huge):
    """8,193 -> 513 -> 33 -> 2,049 -> 769 rows on the NaN-filled large twin handle (8 partial rows, then 2, none, 6 and 3): every
    result is what a fresh twin handle of exactly that size returns, byte for byte, and the sequence a second time returns the same"""
    devs = {n: _dev(TC.twin_case(n, "init")) for n in SPLIT_SEQUENCE}
    fresh = {}
    for n in SPLIT_SEQUENCE:
        own = _twin(n)
        fresh[n] = _twin_grad(own, devs[n])
        own.close()
        assert np.isfinite(fresh[n]).all()
    _poison(huge)
    for run in range(2):
        for n in SPLIT_SEQUENCE:
            assert _twin_grad(huge, devs[n]).tobytes() == fresh[n].tobytes(), (run, n)


# --------------------------------------------------------------------------------------- 3. handles
def test_twin_call_needs_a_twin_handle_and_respects_max_batch():
    import ctypes as C
    import torch
    from balance_robot_mujoco_rl_amd import BrsError, _lib
    from balance_robot_mujoco_rl_amd.policy import _p
    z = lambda *s: torch.zeros(s, device="cuda")
    plain = _single(64)
    rc = _lib.lib().brs_ddpg_learner_twin_critic_grad(plain.h, _p(z(2 * NC)), 8, _p(z(8, 6)), _p(z(8, 2)), _p(z(8)), _p(z(2 * NC + 4)), None)
    assert rc == -1
    assert _lib.lib().brs_ddpg_learner_last_error(plain.h) == (b"brs_ddpg_learner_twin_critic_grad: the handle was not created with "
                                                               b"brs_ddpg_learner_create_twin")
    plain.close()
    twin = _twin(32)
    with pytest.raises(BrsError, match="brs_ddpg_learner_twin_critic_grad: m exceeds the handle's max_batch"):
        twin.twin_critic_grad(z(2 * NC), z(33, 6), z(33, 2), z(33))
    with pytest.raises(ValueError):
        twin.twin_critic_grad(z(NC), z(8, 6), z(8, 2), z(8))
    twin.close()
    assert C.sizeof(C.c_void_p) == 8


def test_existing_calls_return_the_same_bytes_on_a_twin_handle():
    """critic_grad, actor_grad (through critics[:NCRITIC]) and apply on a twin handle against an ordinary one; the ordinary handle's
    allocation keeps its size"""
    import ctypes as C
    import torch
    from balance_robot_mujoco_rl_amd import _lib
    from balance_robot_mujoco_rl_amd.policy import _p
    c = TC.twin_case(257, "x3")
    dev = _dev(c)
    plain, twin = _single(257), _twin(257)
    assert plain.scratch()[1] == 4 * (1092 * 384 + 8 * (NA + 2)) and twin.scratch()[1] == 4 * (2 * 772 * 384 + 8 * (2 * NC + 4))
    L, cfg = _lib.lib(), _lib.BrsAdamConfig(1e-3, 0.9, 0.999, 1e-8)
    results = []
    for lrn in (plain, twin):
        gc, ga = Guarded((NC + 2,)), Guarded((NA + 2,))
        assert L.brs_ddpg_learner_critic_grad(lrn.h, _p(dev["critics"]), 257, _p(dev["obs"]), _p(dev["act"]), _p(dev["y"]), _p(gc.t), None) == 0
        crit = gc.np()
        assert L.brs_ddpg_learner_actor_grad(lrn.h, _p(dev["actor"]), _p(dev["critics"]), 257, _p(dev["obs"]), _p(ga.t), None) == 0
        act = ga.np()
        p, m, v, tg = (Guarded((NC,), fill=f) for f in (0.25, 0.0, 0.0, 0.25))
        assert L.brs_ddpg_learner_apply(lrn.h, NC, _p(p.t), _p(gc.t), _p(m.t), _p(v.t), _p(tg.t), C.byref(cfg), 1, 0.005, None) == 0
        torch.cuda.synchronize()
        assert all(x.intact() for x in (gc, ga, p, m, v, tg))
        results.append([crit, act, p.np(), m.np(), v.np(), tg.np()])
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes() and np.isfinite(a).all()
    assert not np.array_equal(results[0][2], np.full(NC, 0.25, np.float32))
    plain.close(); twin.close()


# --------------------------------------------------------------------------------------- 4. whole steps
def test_six_chained_steps_with_the_delay(nets, host):
    """brs_td3_td_target from the three targets as they are -> DeviceTD3Learner.step, six times with policy_delay = 2, on the kernels
    and on the host build, each against the same chain in fp64 by the trajectory rule; targets and actor byte-frozen on odd steps"""
    case = TC.chain_case("init")
    h = TC.HostTD3(host, case["actor"], case["critics"], policy_delay=TC.POLICY_DELAY, **ADAM)
    lrn = _twin(TC.CHAIN_ROWS, policy_delay=TC.POLICY_DELAY)
    flat = {k: _cuda(case[k.split("_")[0]]) for k in ("actor", "critics", "actor_target", "critics_target")}
    for s in range(TC.CHAIN_STEPS):
        sl = slice(s * TC.CHAIN_ROWS, (s + 1) * TC.CHAIN_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        before = {k: v.cpu().numpy() for k, v in flat.items()}
        y = nets.td3_target(flat["actor_target"], flat["critics_target"], _cuda(no), _cuda(rew), _cuda(done), GAMMA, *TC.SB3_NOISE, s)
        delayed = lrn.step(flat, _cuda(obs), _cuda(act), y)
        assert delayed == (s % 2 == 1) == h.step(obs, act, h.td3_target(no, rew, done, GAMMA, *TC.SB3_NOISE, SEED, s))
        after = {k: v.cpu().numpy() for k, v in flat.items()}
        assert after["critics"].tobytes() != before["critics"].tobytes()
        for k in ("actor", "actor_target", "critics_target"):
            assert (after[k].tobytes() == before[k].tobytes()) == (not delayed), (s, k)
    mine = {k: v.cpu().numpy() for k, v in flat.items()}
    worst_h = TC.check_chain("host chain", h.flat, case)
    worst = TC.check_chain("kernels", mine, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| after six chained steps: kernels {worst:.3g}, host build {worst_h:.3g}")
    s = lrn.stats()
    assert all(np.isfinite(v) for v in s.values()) and s["critic_loss"] > 0
    assert (lrn.steps_critics, lrn.steps_actor, lrn.n_updates) == (6, 3, 6)
    sd = lrn.state_dict()
    assert sd["n_updates"] == 6 and sd["m_critics"].shape == (2 * NC,)
    lrn.close()


def test_tool_with_device_learner_end_to_end():
    """tools/train_td3_torch.py --envs 64 --steps 40 --batch 64 --device-data --device-learner: it trains, the actor is updated on
    every second update, everything is finite, all four vectors moved.  No learning-quality gate."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_td3_torch as T
    log = T.main(["--envs", "64", "--steps", "40", "--batch", "64", "--device-data", "--device-learner"])
    assert log["updates"] == 39 and log["actor_updates"] == log["updates"] // 2   # 100 transitions are in after two steps of 64 envs
    assert log["finite"] and log["learner"] == "device" and log["data_path"] == "device"
    assert all(log["moved"][k] > 0 for k in ("actor", "critics", "actor_target", "critics_target")), log["moved"]
    assert log["moved"]["critics_target"] < log["moved"]["critics"] and log["moved"]["actor_target"] < log["moved"]["actor"]
    assert np.isfinite(log["critic_loss_last"]) and log["critic_loss_last"] > 0 and np.isfinite(log["actor_loss_last"])
