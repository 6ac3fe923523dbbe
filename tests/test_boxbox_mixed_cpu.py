"""The mixed wave of tests/boxbox_mixed.py -- every case of the block<->torso generator side by side -- on the host builds of
the kernel source against the oracle, through full env steps at the tolerances of tests/test_constructed_steps.py, and the
check that the oracle alone puts every chosen state into the case it was chosen for.  The HIP path: tests/test_boxbox_mixed_wave_gpu.py."""
import collections

import numpy as np
import pytest

from tests import boxbox_mixed as bm, constructed_states as cs


def test_the_oracle_classifies_every_chosen_state_as_intended():
    qpos, qvel, ctrl, kinds, source = bm.population()
    assert qpos.shape == (64, 16) and qvel.shape == (64, 14) and ctrl.shape == (64, 2)
    assert [bm.kind(q) for q in qpos] == list(kinds)
    count = collections.Counter(kinds)
    assert sorted(count) == sorted(bm.KINDS) and min(count.values()) >= 8, count
    # interleaved: no two neighbouring lanes of one kind, so that no arm is walked by a run of lanes only
    assert (kinds[1:] != kinds[:-1]).all()
    # the far lanes are out of reach of the wheel generator as well (it runs behind the same reach test)
    assert all(np.linalg.norm(bm.geometry(q)[0]) > 0.3 for q in qpos[kinds == "far"])


def test_the_oracle_emits_what_the_kinds_say():
    """block<->robot contacts of the teacher at the start: none for the separated and far lanes, 1 for an edge pair inside
    the margin (plus at most the wheel point), >= 1 for the face lanes"""
    from tests import parity as P
    qpos, qvel, _, kinds, _ = bm.population()
    orc = P.make("oracle", "Env03-v2", 64, noise=False)
    orc.set_state(qpos, qvel)
    ncoupled = cs.coupled_contact_count(orc, 64)
    orc.close()
    assert (ncoupled[kinds == "far"] == 0).all()
    assert (ncoupled[np.isin(kinds, ("edge_in", "faceT", "faceB"))] >= 1).all()
    assert (ncoupled[np.isin(kinds, ("edge_out", "sep"))] <= 1).all()   # (the wheel point alone, where a wheel is near)
    assert ncoupled[np.isin(kinds, ("faceT", "faceB"))].max() >= 4


@pytest.mark.parametrize("env_id", ["Env03-v2", "Env03-v1"])
@pytest.mark.parametrize("backend,cap", [("host64", 1e-7), ("host32", None)])
def test_host_builds_env_steps_on_the_mixed_wave(backend, cap, env_id, monkeypatch):
    monkeypatch.setitem(cs.SCENARIOS, "boxbox_mixed", bm.scenario(env_id))
    cs.run_scenario_steps_on(backend, "boxbox_mixed", env_id, **({} if cap is None else dict(cap=cap)))


@pytest.mark.parametrize("backend,q_cap,max_cap", [("host64", 1e-9, 1e-8), ("host32", None, None)])
def test_host_builds_five_substeps_on_the_mixed_wave(backend, q_cap, max_cap, monkeypatch):
    """the physics call alone; float build: per source scenario the caps the HIP path holds on that scenario (cs.HIP_CAPS)"""
    monkeypatch.setitem(cs.SCENARIOS, "boxbox_mixed", bm.scenario())
    err, vt = cs.run_scenario_on(backend, "boxbox_mixed")
    source = bm.population()[4]
    for name in ("block_robot", "edge_edge", "pinned"):
        m = source == name
        print(f"{backend}, lanes from {name}: rel. velocity error max {err[m].max():.3g}")
        if backend == "host32":
            cs.check_hip_caps(name, err[m], vt[m])
        else:
            assert err[m].max() < max_cap
