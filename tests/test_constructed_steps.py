"""Full env steps from the constructed contact states (tests/constructed_states.py: run_scenario_steps), kernel source on the
host against the oracle: reward and control law on the pre-step state, 250 substeps, block state machine, termination,
observation -- the path brs_step runs, on states a rollout from reset reaches only by chance.  The same procedure on the HIP
step kernels: tests/test_constructed_steps_gpu.py."""
import numpy as np
import pytest

from tests import constructed_states as cs, parity as P

BLOCK = ("block_robot", "edge_edge", "pinned")


@pytest.mark.parametrize("name", sorted(cs.SCENARIOS))
def test_double_build_env_steps_from_constructed_states(name):
    """cap: that of test_hostsim_parity.py::test_double_instantiation_matches_oracle"""
    cs.run_scenario_steps_on("host64", name, cap=1e-7)


@pytest.mark.parametrize("name", sorted(cs.SCENARIOS))
def test_float_build_env_steps_from_constructed_states(name):
    cs.run_scenario_steps_on("host32", name)


@pytest.mark.parametrize("name,env_id", [("floor", "Env01-v1"), ("floor", "Env01-v3"), ("floor", "Env02-v1")]
                         + [(name, "Env03-v1") for name in BLOCK])
def test_float_build_env_steps_on_the_other_ids(name, env_id):
    """the floor states under the other reward / observation / friction rules of the Env01 family (Env02's per-episode
    friction is forced with the aux row), the block states under Env03-v1's block rules"""
    g, _, recs, _ = cs.run_scenario_steps_on("host32", name, env_id)
    if name == "floor":
        assert g.n["fallen"] > 0.25 * len(recs) * len(recs[0].skip), "robots that lie on the ground"


class _OffByOneBlockCoordinate:
    """a student whose get_state reports one block coordinate of env 0 as 2e-4 further than it is"""
    def __init__(self, sim):
        self.sim = sim

    def __getattr__(self, name):
        return getattr(self.sim, name)

    def get_state(self):
        qpos, *rest = self.sim.get_state()
        qpos[0, 10] += 2e-4
        return (qpos, *rest)


def test_the_procedure_fails_on_a_planted_error():
    """(without the plant: test_double_build_env_steps_from_constructed_states[pinned])"""
    assert P.upright(cs.scenario_inputs("pinned")[0][:1])[0], "env 0 starts upright: its block coordinates are under G2"
    with pytest.raises(AssertionError, match=r"pinned.*G2: block coordinates 0\.0002"):
        cs.run_scenario_steps_on("host64", "pinned", student=_OffByOneBlockCoordinate)


def test_all_scenarios_are_covered():
    assert sorted(cs.SCENARIOS) == sorted(BLOCK + ("floor",))
    for name in cs.SCENARIOS:
        qpos, qvel, ctrl = cs.scenario_inputs(name)
        assert len(qpos) == len(qvel) == len(ctrl) and np.isfinite(qpos).all() and np.isfinite(qvel).all()
