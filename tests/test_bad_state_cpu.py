"""The bad-state guard on poisoned inputs, on the CPU: the fp64 oracle and the kernel's own source compiled for the host (fp32 and
fp64), each against the numpy predicate of tests/poison_cases.py (the contract is written out there and in DESIGN.md 3.2).
Every case of the table runs for every registered id; nothing is filtered."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import poison_cases as pc
from tests.hostsim import hostsim

THREADS = min(16, os.cpu_count() or 1)
SIMS = ("oracle", "host64", "host32")


def make_sim(who, env_id, n):
    kw = dict(seed=pc.SEED, auto_reset=True, noise=False, threads=THREADS)
    if who == "oracle":
        return Oracle(env_id, n, **kw)
    return hostsim.HostSim(env_id, n, double=(who == "host64"), **kw)


@functools.lru_cache(maxsize=None)
def run(who, env_id, poisoned=True):
    n = 2 * len(pc.cases(env_id)) + 2
    return pc.Run(make_sim(who, env_id, n), env_id, stride=2, n=n, poisoned=poisoned)


def test_case_table_is_complete():
    for env_id in pc.ENV_IDS:
        blk = env_id.startswith("Env03")
        nq, nv = (16, 14) if blk else (9, 8)
        cs = pc.cases(env_id)
        assert len(cs) == 5 * (nq + 2 * nv) + 12 + (2 if env_id == "Env02-v1" else 0)
        assert len({c[0] for c in cs}) == len(cs)
        for field, ncol in (("qpos", nq), ("qvel", nv), ("warm", nv), ("action", 2)):
            assert {c[2] for c in cs if c[1] == field} == set(range(ncol))
    assert pc.is_bad([np.nan, np.inf, -np.inf, 1.0000001e10, -1.0000001e10]).all() and not pc.is_bad([0.0, 1e10, -1e10, 9.9e9]).any()


@pytest.mark.parametrize("env_id", pc.ENV_IDS)
@pytest.mark.parametrize("who", SIMS)
def test_guard_follows_the_predicate(who, env_id):
    """items 1-4: verdict, elapsed / time / return of the new episode, everything finite over the poisoned step and twenty more"""
    r = run(who, env_id)
    fields = {c[1] for lane, c in r.case_rows() if r.expected[lane]}
    assert fields == {"qpos", "qvel", "action"}  # the table does make the guard fire, and never through a warm start or a friction
    pc.check_contract(r, who)
    pc.check_action_reward_kept(r, run(who, env_id, False))


@pytest.mark.parametrize("env_id", pc.ENV_IDS)
@pytest.mark.parametrize("who", SIMS)
def test_healthy_lanes_do_not_notice(who, env_id):
    """item 5: bit-identical to a control run of the same configuration and seed in which no lane was poisoned"""
    pc.check_healthy_identical(run(who, env_id), run(who, env_id, False), who)


@pytest.mark.parametrize("env_id", pc.ENV_IDS)
@pytest.mark.parametrize("who", ("host64", "host32"))
def test_guard_reset_draws_what_the_oracle_draws(who, env_id):
    pc.check_reset_matches_oracle(run(who, env_id), run("oracle", env_id), who)


@pytest.mark.parametrize("who", ("host64", "host32"))
def test_range_edge(who):
    """1e10 itself is not bad, the next number above it is (fp32: as the stored fp64 velocity rounds)"""
    n = 4
    sim = make_sim(who, "Env01-v2", n)
    sim.reset()
    qpos, qvel, _, _ = sim.get_state()
    qvel[0, 1], qvel[1, 1], qvel[2, 1], qpos[3, 1] = 1e10, np.nextafter(1e10, np.inf), -1e10, -np.nextafter(1e10, np.inf)
    sim.set_state(qpos=qpos, qvel=qvel)
    sim.step(np.zeros((n, 2), np.float32))
    assert sim.get_aux()[:, pc.AUX_BAD].tolist() == [0, 1, 0, 1]


_UBSAN_CHILD = """
import sys
from tests import poison_cases as pc
from tests.hostsim import hostsim
hostsim.use_library("libbrs_hostsim_ubsan.so")
for env_id in ("Env01-v2", "Env03-v2"):
    n = 2 * len(pc.cases(env_id)) + 2
    sim = hostsim.HostSim(env_id, n, seed=pc.SEED, auto_reset=True, noise=False, threads=int(sys.argv[1]))
    pc.check_contract(pc.Run(sim, env_id, stride=2, n=n), "host32+ubsan")
print("ubsan child: done")
"""


def test_no_undefined_behaviour_on_poisoned_inputs():
    """the whole table through the kernel source built with -fsanitize=undefined,float-cast-overflow (no recovery: a report aborts
    the child): no array index and no float -> int conversion is driven out of range by a NaN"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), os.environ.get("PYTHONPATH", "")]),
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([sys.executable, "-c", _UBSAN_CHILD, str(THREADS)], cwd=os.path.dirname(here), env=env, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0 and "ubsan child: done" in p.stdout, f"exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-6000:]}"
    assert "runtime error" not in p.stderr, p.stderr[-6000:]
