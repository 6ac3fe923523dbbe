"""The bad-state guard on poisoned inputs, on the GPU: the table, the predicate and the assertions of tests/test_bad_state_cpu.py
(tests/poison_cases.py) through BatchedSim, with the oracle alongside.  The step kernels are separate compilations
(tests/test_launch_geometry_gpu.py) built with -ffast-math, where a NaN may be treated differently from the host build: Env01-v2
on the capped two-waves-per-SIMD kernel (64 threads) and the uncapped one (128), Env02-v1 with the friction rows, Env03-v2 at 64
and 256 threads, with and without lane grouping.  Several full waves and a partial one, poisoned and healthy lanes in every wave.

Run this file only after tests/test_bad_state_cpu.py is green, its sanitizer run included: that is the evidence that no index in
the kernel source follows a NaN out of range."""
import functools
import os

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import poison_cases as pc

pytestmark = pytest.mark.gpu

# (env id, block_threads, lane grouping) -> the step kernel it has to launch
CONFIGS = {
    ("Env01-v2", 64, True): "brs_step_kernel_occ2<1>",
    ("Env01-v2", 128, True): "brs_step_kernel<false, 1>",
    ("Env02-v1", 64, True): "brs_step_kernel_occ2<5>",
    ("Env03-v2", 64, True): "brs_step_kernel<true, 3>",
    ("Env03-v2", 64, False): "brs_step_kernel<true, 3>",
    ("Env03-v2", 256, True): "brs_step_kernel<true, 3>",
}


def geometry(env_id):
    """-> (stride, n): case k in lane stride * k + 1, n = 64 * w + 37 with the last poisoned lane inside the partial wave"""
    k = len(pc.cases(env_id))
    for stride in range(2, 8):
        last = stride * (k - 1) + 1
        if last % 64 <= 35:
            return stride, 64 * (last // 64) + 37
    raise AssertionError(env_id)


@functools.lru_cache(maxsize=None)
def gpu_run(env_id, block_threads, grouping, poisoned=True):
    from balance_robot_mujoco_rl_amd import BatchedSim
    stride, n = geometry(env_id)
    sim = BatchedSim(env_id, n, seed=pc.SEED, auto_reset=True, obs_noise=False, block_threads=block_threads, lane_grouping=grouping)
    try:
        assert sim.step_kernel_name() == CONFIGS[env_id, block_threads, grouping]
        return pc.Run(sim, env_id, stride=stride, n=n, poisoned=poisoned)
    finally:
        sim.close()


@functools.lru_cache(maxsize=None)
def oracle_run(env_id):
    stride, n = geometry(env_id)
    return pc.Run(Oracle(env_id, n, seed=pc.SEED, auto_reset=True, noise=False, threads=min(16, os.cpu_count() or 1)), env_id, stride=stride, n=n)


def test_every_wave_holds_poisoned_and_healthy_lanes():
    for env_id in {c[0] for c in CONFIGS}:
        stride, n = geometry(env_id)
        lanes = {stride * k + 1 for k in range(len(pc.cases(env_id)))}
        assert n % 64 == 37 and n // 64 >= 4
        for w in range(n // 64 + 1):
            wave = set(range(64 * w, min(64 * w + 64, n)))
            assert wave & lanes and wave - lanes, (env_id, w)


@pytest.mark.parametrize("env_id,block_threads,grouping", list(CONFIGS))
def test_guard_follows_the_predicate(env_id, block_threads, grouping):
    """items 1-4 on the HIP path, and the guard's reset against the oracle's"""
    who = f"hip bt={block_threads} grouping={grouping}"
    r = gpu_run(env_id, block_threads, grouping)
    assert {c[1] for lane, c in r.case_rows() if r.expected[lane]} == {"qpos", "qvel", "action"}
    pc.check_contract(r, who)
    pc.check_action_reward_kept(r, gpu_run(env_id, block_threads, grouping, False))
    o = oracle_run(env_id)
    pc.check_contract(o, "oracle")
    pc.check_reset_matches_oracle(r, o, who)


@pytest.mark.parametrize("env_id,block_threads,grouping", list(CONFIGS))
def test_healthy_lanes_do_not_notice(env_id, block_threads, grouping):
    """item 5 against a control handle on the GPU"""
    pc.check_healthy_identical(gpu_run(env_id, block_threads, grouping), gpu_run(env_id, block_threads, grouping, False),
                               f"hip bt={block_threads} grouping={grouping}")


@pytest.mark.parametrize("other", [("Env03-v2", 64, False), ("Env03-v2", 256, True)])
def test_env03_bitwise_across_lane_maps_and_workgroup_sizes(other):
    """A lane whose guard fired gets its cost class from the reset state, so the lane map stays a permutation: with and without
    lane grouping (and at another workgroup size) everything is bit-identical, poisoned lanes included, on all 21 steps"""
    a, b = gpu_run("Env03-v2", 64, True), gpu_run(*other)
    for x, y in zip(a.start, b.start):
        assert np.array_equal(x, y, equal_nan=True)
    for k, (sa, sb) in enumerate(zip(a.steps, b.steps)):
        for key in sa:
            same = (sa[key] == sb[key]) | ((sa[key] != sa[key]) & (sb[key] != sb[key])) if sa[key].dtype.kind == "f" else sa[key] == sb[key]
            assert same.all(), f"step {k}: {key} differs on lanes {np.flatnonzero(~same.reshape(a.n, -1).all(axis=1))[:8]} between {('Env03-v2', 64, True)} and {other}"
