"""The Env03 lane map ON THE DEVICE against its contract, read through brs_get_lane_map after every step:

  1  perm is a permutation of the envs;
  2  the 17 counter words (bucket counts, cursors, ticket) are 0 again;
  3  keys[e] is the cost class of the state env e's NEXT step starts from (after an auto-reset: the reset state), on every bit
     the fp64 restatement (tests/ref_lane_map.py) calls decided;
  4  the bucket at every lane slot, keys[perm], is the one brs_state.hpp: lane_slot puts there (tests/lane_map_cases.py:
     owner_of) for the device's own key counts and the reported wheel cap -- slot by slot; the order inside a bucket is the
     order the atomics arrived in and is not compared;
  5  the wheel cap is BRS_RARE_CAP while the launch fits one wave per SIMD, 64 above that.

tests/test_lane_map_gpu.py shows that the map is a permutation that changes no result; any permutation passes there.  The
populations and what makes them worth running are checked on the host in tests/test_lane_map_ref_cpu.py."""
import numpy as np
import pytest

from tests import lane_map_cases as lc, ref_lane_map as ref

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

OUTPUTS = ("obs", "reward", "terminated", "truncated", "terminal_obs")


def _sim(env_id, n, **kw):
    from balance_robot_mujoco_rl_amd import BatchedSim
    return BatchedSim(env_id, n, **kw)


def _expected_cap(n):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return lc.RARE_CAP if -(-n // lc.WAVE) <= 4 * cus else lc.WAVE   # CDNA: 4 SIMDs per CU


class Tally:
    """undecided bits over a run: their share is capped, the differences on them are printed"""
    def __init__(self, what):
        self.what, self.pairs, self.undecided, self.differ = what, 0, 0, 0

    def close(self):
        print(f"{self.what}: undecided {self.undecided} of {self.pairs} (env, bit) pairs, the device differs on {self.differ} of them")
        assert self.undecided <= ref.UNDECIDED_CAP * self.pairs, self.what


def check_keys(sim, lm, how, tally, where):
    """assertion 3"""
    qpos, qvel, _, _ = sim.get_state()
    assert np.isfinite(qpos).all() and np.isfinite(qvel).all(), where
    r = ref.cost_class(qpos, qvel, **how)
    decided, undecided_differ, undecided = ref.compare_keys(r, lm["keys"])
    tally.pairs += 3 * sim.n; tally.undecided += undecided; tally.differ += undecided_differ
    if decided:
        bad = np.flatnonzero((((lm["keys"][:, None].astype(np.int64) >> np.arange(3)) & 1) != r["bit"]).any(axis=1) & ~r["undecided"].any(axis=1))[:5]
        raise AssertionError(f"{where}: {decided} decided key bits differ from the cost class of the post-step state; envs {bad.tolist()}: "
                             f"device keys {lm['keys'][bad].tolist()}, reference {r['key'][bad].tolist()}")
    return r


def check_layout(sim, lm, where, cap=None):
    """assertions 1, 2, 4, 5"""
    n, perm, keys = sim.n, lm["perm"], lm["keys"]
    assert np.array_equal(np.sort(perm), np.arange(n)), f"{where}: perm is not a permutation of the envs"
    assert lm["counters"].shape == (17,) and not lm["counters"].any(), f"{where}: counters {lm['counters'].tolist()}"
    assert lm["wheel_cap"] == (_expected_cap(n) if cap is None else cap), f"{where}: wheel cap {lm['wheel_cap']}"
    assert keys.max() < lc.NBUCKET
    cnt = np.bincount(keys, minlength=lc.NBUCKET)
    owner = lc.owner_of(cnt, lm["wheel_cap"])
    got = keys[perm].astype(np.int64)
    if not np.array_equal(got, owner):
        s = np.flatnonzero(got != owner)
        raise AssertionError(f"{where}: key counts {cnt.tolist()}, cap {lm['wheel_cap']}: {len(s)} lane slots hold another bucket than "
                             f"lane_slot's; first {s[:8].tolist()}: device {got[s[:8]].tolist()}, lane_slot {owner[s[:8]].tolist()}")
    return cnt


def _act(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("run", lc.RUNS, ids=lambda r: "-".join(map(str, r)))
def test_device_map_after_every_step(run):
    """populations (a), (b), (c) and the diluted (d): assertions 1-5 after every step.  All of them fit one wave per SIMD: the
    cap is BRS_RARE_CAP, and on (d), which has far lanes to spare, the layout at that cap is another than at 64"""
    kind, n, env_id = run
    sim, acts, how = lc.start(_sim, kind, n, env_id)
    tally, seen, done = Tally("-".join(map(str, run))), np.zeros(lc.NBUCKET, np.int64), 0
    for k, a in enumerate(acts):
        _, _, te, tr, _ = sim.step(_act(a))
        done += int((te | tr).sum())
        lm, where = sim.get_lane_map(), f"{run} step {k}"
        r = check_keys(sim, lm, how, tally, where)
        seen += check_layout(sim, lm, where)   # the cap by the CU-count rule ...
        assert lm["wheel_cap"] == lc.RARE_CAP    # ... which for these sizes is BRS_RARE_CAP on any CDNA part of 5 CUs or more
        if kind == "rollout":  # the key of an env that was just reset is the reset state's: far, the block is 30 cm away
            fresh = (te | tr).cpu().numpy().astype(bool)
            assert (lm["keys"][fresh & ~r["undecided"].any(axis=1)] == lc.FAR).all(), where
    tally.close()
    if kind == "rollout":
        assert done >= 2 * n, "episodes of at most 5 steps: every env is auto-reset at least twice in 12"
    else:
        assert (seen > 0).all(), f"{run}: device keys seen {seen.tolist()}"
    sim.close()


def test_cap_64_above_one_wave_per_simd():
    """the smallest launch that selects the undiluted layout: one env more than one wave per SIMD holds"""
    n = lc.WAVE * 4 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    sim = _sim("Env03-v2", n, **lc.ROLLOUT)
    sim.reset()
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    for k in range(3):
        sim.step(torch.rand((n, 2), generator=g, device="cuda") * 3 - 1.5)
        lm = sim.get_lane_map()
        assert lm["wheel_cap"] == lc.WAVE
        check_layout(sim, lm, f"cap 64, n {n}, step {k}", cap=lc.WAVE)
    sim.close()
    small = _sim("Env03-v2", n - 1)   # ... and one env less is diluted
    assert small.get_lane_map()["wheel_cap"] == lc.RARE_CAP
    small.close()


def test_grouping_off_keeps_the_identity_and_still_writes_keys():
    n = lc.CONSTRUCTED_N
    sim, acts, how = lc.start(_sim, "constructed", n, lane_grouping=False)
    tally = Tally("grouping off")
    for k, a in enumerate(acts):
        sim.step(_act(a))
        lm = sim.get_lane_map()
        assert np.array_equal(lm["perm"], np.arange(n)), f"step {k}: perm moved without lane grouping"
        assert not lm["counters"].any(), f"step {k}: counters {lm['counters'].tolist()}"
        check_keys(sim, lm, how, tally, f"grouping off, step {k}")
    tally.close()
    sim.close()


def test_masked_reset_and_set_state_leave_the_map_alone():
    """brs_reset and brs_set_state between two steps do not touch perm (it stays a permutation built from the keys of the
    step before); the step after them regroups from the new states"""
    n = lc.CONSTRUCTED_N
    sim, acts, how = lc.start(_sim, "constructed", n)
    sim.step(_act(acts[0]))
    before = sim.get_lane_map()
    check_layout(sim, before, "before the reset")
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda"); mask[::3] = 1
    sim.reset(mask)
    qpos, qvel = lc.constructed_state()
    sim.set_state(np.roll(qpos, 5, axis=0), np.roll(qvel, 5, axis=0))
    after = sim.get_lane_map()
    for what in ("perm", "keys", "counters"):
        assert np.array_equal(before[what], after[what]), what
    sim.step(_act(acts[1]))
    lm, tally = sim.get_lane_map(), Tally("after masked reset")
    check_keys(sim, lm, how, tally, "step after the masked reset")
    check_layout(sim, lm, "step after the masked reset")
    tally.close()
    assert not np.array_equal(lm["perm"], before["perm"])
    sim.close()


def test_env01_has_no_lane_map():
    from balance_robot_mujoco_rl_amd import BrsError
    sim = _sim("Env01-v2", 65)
    with pytest.raises(BrsError, match="brs_get_lane_map: the Env01 family has no lane map"):
        sim.get_lane_map()
    sim.reset()
    sim.step(torch.zeros((65, 2), device="cuda"))   # the handle is still good
    sim.close()


def test_reading_the_map_has_no_side_effect():
    """two identical handles, one read after every step: outputs, states and aux stay bit-identical"""
    n = 357
    (read, acts, _), (plain, _, _) = (lc.start(_sim, "rollout", n) for _ in range(2))
    for k, a in enumerate(acts[:10]):
        out_r = [x.clone() for x in read.step(_act(a))]
        first = read.get_lane_map()
        second = read.get_lane_map()
        for what in ("perm", "keys", "counters"):
            assert np.array_equal(first[what], second[what])
        for nm, x, y in zip(OUTPUTS, out_r, plain.step(_act(a))):
            assert torch.equal(x, y), f"step {k}: {nm} differs after reading the lane map"
    for x, y in zip(read.get_state(), plain.get_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(read.get_aux(), plain.get_aux(), equal_nan=True)
    assert np.array_equal(read.get_lane_map()["keys"], plain.get_lane_map()["keys"])
    read.close(); plain.close()
