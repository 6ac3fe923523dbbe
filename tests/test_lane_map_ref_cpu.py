"""The references the device lane map is held to (tests/test_lane_map_device_gpu.py), checked without a GPU:

  * the fp64 numpy restatement of the cost class (tests/ref_lane_map.py) against the source itself, through the double host
    build of brs_state.hpp: cost_class (tests/hostsim: hs_cost_class) -- keys and both sides of every comparison;
  * its tolerance: the fp32 host build of the same source agrees on every decided bit of every population;
  * the populations (tests/lane_map_cases.py): auto-resets, steps with too few far lanes, all eight keys, few undecided bits;
  * how conservative the cost class is on them: printed, not gated (tests/lanemap/costclass_host.cpp)."""
import os
import subprocess

import numpy as np
import pytest

from tests import lane_map_cases as lc, ref_lane_map as ref

RUNS = lc.RUNS
_id = lambda r: "-".join(map(str, r))


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_restatement_equals_the_source_in_double(run):
    """the double host build: the stored velocities ARE get_state's qvel (world linear, body angular, no conversion), both
    sides of every comparison agree to 1e-12 relative and the keys on every decided bit (in fact on every bit)"""
    kind, n, env_id = run
    for k, s in enumerate(lc.host_run(kind, n, env_id, double=True)):
        r = s["ref"]
        np.testing.assert_allclose(r["lhs"], s["cmp"][:, :, 0], rtol=1e-12, atol=0, err_msg=f"{run} step {k}: lhs")
        np.testing.assert_allclose(r["rhs"], s["cmp"][:, :, 1], rtol=1e-12, atol=0, err_msg=f"{run} step {k}: rhs")
        decided, undecided, _ = ref.compare_keys(r, s["key"])
        assert decided == 0, f"{run} step {k}: {decided} decided bits differ from cost_class in double"
        assert (r["scale"] >= np.maximum(np.abs(r["lhs"]), np.abs(r["rhs"]))).all()  # a sum of |terms| bounds both sides


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_float_host_build_agrees_on_every_decided_bit(run):
    """the tolerance of the restatement: the fp32 host build of cost_class, on its own fp32 rollout, never differs from the
    fp64 restatement of the same stored state where that calls the bit decided; at most 1 in 1,000 bits are undecided"""
    kind, n, env_id = run
    steps = lc.host_run(kind, n, env_id)
    bad = und_differ = und = 0
    for s in steps:
        assert np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all()
        a, b, c = ref.compare_keys(s["ref"], s["key"])
        bad, und_differ, und = bad + a, und_differ + b, und + c
    print(f"{_id(run)}: undecided {und} of {3 * n * len(steps)} (env, bit) pairs, fp32 host differs on {und_differ} of them")
    assert bad == 0, f"{run}: the fp32 host build differs on {bad} decided bits: TOL is too tight"
    assert und <= ref.UNDECIDED_CAP * 3 * n * len(steps)


@pytest.mark.parametrize("n", lc.ROLLOUT_SIZES)
@pytest.mark.parametrize("env_id", ["Env03-v2", "Env03-v1"])
def test_rollouts_reset_and_run_out_of_far_lanes(env_id, n):
    """population (a) on the reference: every env is auto-reset (twice), the key after such a step is the reset state's (far:
    the block starts 30 cm away), and on Env03-v2 some step has too few far lanes to fill every bucket's last wave.  (Env03-v1
    throws its block too late for episodes of 5 steps: every key of that rollout is far, and the map it is held to is the
    identity layout of one bucket.  Its expensive buckets are those of the constructed population.)"""
    steps = lc.host_run("rollout", n, env_id)
    assert len(steps) == lc.ROLLOUT_STEPS
    assert sum(int(s["done"].sum()) for s in steps) == 2 * n
    for s in steps:
        assert (s["ref"]["key"][s["done"]] == lc.FAR).all()
    cnts = [np.bincount(s["ref"]["key"], minlength=lc.NBUCKET) for s in steps]
    if env_id == "Env03-v2":
        assert len({tuple(c) for c in cnts}) >= 2   # the map has something to regroup
        assert any(lc.gaps(c) > c[lc.FAR] for c in cnts)


@pytest.mark.parametrize("run", [r for r in RUNS if r[0] != "rollout"], ids=_id)
def test_constructed_population_has_all_eight_keys_after_one_step(run):
    """populations (b) and (c) on the reference: all eight keys after ONE step (and after every later one), and more gaps than
    far lanes: buckets share waves.  (d) has far lanes to spare instead: its wheel buckets are diluted, and the layout at the
    cap BRS_RARE_CAP is another than at 64"""
    kind = run[0]
    steps = lc.host_run(*run)
    assert len(steps) == lc.CONSTRUCTED_STEPS
    for k, s in enumerate(steps):
        cnt = np.bincount(s["ref"]["key"], minlength=lc.NBUCKET)
        assert len(cnt) == lc.NBUCKET and (cnt > 0).all(), f"{kind} step {k}: keys {cnt.tolist()}"
        if kind == "constructed_diluted":
            diluted, packed = lc.owner_of(cnt, lc.RARE_CAP), lc.owner_of(cnt, lc.WAVE)
            assert lc.gaps(cnt) <= cnt[lc.FAR] and (diluted != packed).sum() >= lc.WAVE
            for b in (2, 3, 6, 7):  # every wheel bucket at the cap, in every wave that holds it
                assert max((diluted[w:w + lc.WAVE] == b).sum() for w in range(0, len(diluted), lc.WAVE)) <= lc.RARE_CAP
        else:
            assert lc.gaps(cnt) > cnt[lc.FAR]


def test_owner_of_matches_lane_plan_properties():
    """owner_of on the counts of a constructed step: every bucket gets its count of slots, and the most expensive one the first"""
    cnt = np.bincount(lc.host_run("constructed", lc.CONSTRUCTED_N)[0]["ref"]["key"], minlength=lc.NBUCKET)
    for cap in (lc.RARE_CAP, lc.WAVE):
        owner = lc.owner_of(cnt, cap)
        assert np.array_equal(np.bincount(owner, minlength=lc.NBUCKET), cnt)
        assert (owner[:cnt[3]] == 3).all()


REPORT_REPEATS = 10   # population (b) is stepped this many times, each with other actions: key 6 is held by 5 of its 357 envs


def _population_text(kind, n, action_seed=None):
    """one population in the input format of tests/lanemap/costclass_host.cpp"""
    from tests.hostsim.hostsim import VARIANTS
    if kind == "rollout":
        cfg, acts, rows = lc.ROLLOUT, lc.rollout_actions(n), []
    else:
        cfg, rows = lc.CONSTRUCTED, list(lc.constructed_state())
        acts = np.random.default_rng(action_seed).uniform(-1.5, 1.5, size=(lc.CONSTRUCTED_STEPS, n, 2)).astype(np.float32)
    head = [VARIANTS["Env03-v2"], n, len(acts), cfg.get("max_episode_steps", 0), 0, 0.0, cfg["seed"], int(cfg["auto_reset"]), int(bool(rows))]
    return "\n".join([" ".join(map(str, head))] + [" ".join(repr(float(x)) for x in a.ravel()) for a in rows + [acts]]) + "\n"


def test_cost_class_conservativeness_report(tmp_path):
    """Printed, not gated (the robot accelerates inside a step: nothing in the project bounds these shares): of the lane-steps
    whose key ruled a path out -- floor bit clear: block<->floor contact rows, wheel bit clear: the wheel narrow phase, far bit
    set: the torso narrow phase -- the share that walked it in some substep, on the -DBRS_STATS fp32 host build.  Gated: every
    key value contributes at least 100 lane-steps, or the shares say nothing about it, and every path is walked by some
    lane-step whose key allowed it, or a dead counter would print the same zeros.  Population (b) alone gives key 6 some 16
    lane-steps in its 3 steps: it is stepped REPORT_REPEATS times from the same start, each time with other actions."""
    exe = str(tmp_path / "costclass_host")
    subprocess.check_call(["g++", "-O2", "-fopenmp", "-std=c++17", "-DBRS_STATS", "-ffp-contract=off", "-w",
                           "-I" + os.path.join(lc.ROOT, "balance_robot_mujoco_rl_amd", "csrc"), "-o", exe,
                           os.path.join(lc.ROOT, "tests", "lanemap", "costclass_host.cpp")])
    text = _population_text("rollout", 1061) + "".join(_population_text("constructed", lc.CONSTRUCTED_N, 100 + r) for r in range(REPORT_REPEATS))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True,
                         env=dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))).stdout
    rows = [ln.split() for ln in out.splitlines()]
    per_key = {int(r[1]): int(r[2]) for r in rows if r[0] == "key"}
    bits = {r[1]: tuple(map(int, r[2:6])) for r in rows if r[0] == "bit"}
    assert sorted(per_key) == list(range(8)) and sorted(bits) == sorted(ref.BITS)
    assert sum(per_key.values()) == 1061 * lc.ROLLOUT_STEPS + REPORT_REPEATS * lc.CONSTRUCTED_N * lc.CONSTRUCTED_STEPS
    print("lane-steps per key:", per_key)
    for name in ref.BITS:
        ruled, walked, allowed, walked_allowed = bits[name]
        print(f"bit {name}: {walked} of {ruled} lane-steps walked the path their key had ruled out ({walked / max(ruled, 1):.4%}); "
              f"{walked_allowed} of the {allowed} whose key allowed it walked it")
        assert 0 <= walked <= ruled and ruled + allowed == sum(per_key.values())
        assert 0 < walked_allowed <= allowed, f"bit {name}: no lane-step walked the path at all: is its counter live (-DBRS_STATS)?"
    assert min(per_key.values()) >= 100, per_key
