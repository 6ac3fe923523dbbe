"""The PPO learner (include/brs_policy.h: brs_learner_*) without a GPU: the host build of the kernel source
(tests/learnerhost, the shared header brs_learner.hpp with plain loops for the towers) against fp64 torch autograd of the tool's
minibatch body (tests/ref_learner.py), the clip + Adam step against torch.optim.Adam, the early stop, the same host code as a
program under the sanitizers, the C ABI's argument checks and the state_dict conversions of the Python layer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_learner as R
from balance_robot_mujoco_rl_amd import _lib, learner
from learner_cases import GXX, HOST_DIR, N_ROWS, NPARAM, NSTAT, ROOT, HostLearner, build_host, conditioned, gate as _gate

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("learnerhost"))


# --------------------------------------------------------------------------------------- 1. the gradient
@pytest.mark.parametrize("m", [2, 65, 1000])
def test_host_gradient_against_fp64_autograd(host, m):
    cfg = R.Cfg()
    case, idx = conditioned(m, cfg)
    h = HostLearner(host, cfg, case["params"])
    g = h.grad(case, idx)
    assert h.stats().bad_index == 0
    _gate(g, R.grad_buffer(case, idx, cfg), f"m={m}")
    h.close()


@pytest.mark.parametrize("name,change", [("normalize_adv=0", dict(normalize_adv=0)), ("ent_coef=0.01", dict(ent_coef=0.01)),
                                         ("ret_scale=3", dict(ret_scale=3.0)), ("clip_range=0.1", dict(clip_range=0.1)),
                                         ("several chunks per workgroup", dict())])
def test_host_gradient_switches(host, name, change):
    cfg = R.Cfg(**change)
    case, idx = conditioned(1000, cfg)
    h = HostLearner(host, cfg, case["params"], max_workgroups=0 if change else 2)
    g = h.grad(case, idx)
    g64 = R.grad_buffer(case, idx, cfg)
    _gate(g, g64, name)
    if "ent_coef" in change:   # the bonus is there: d(-ent_coef entropy) / d log_std = -ent_coef
        g0 = R.grad_buffer(case, idx, R.Cfg())
        np.testing.assert_allclose(g64[NPARAM - 2:NPARAM] - g0[NPARAM - 2:NPARAM], -0.01, rtol=1e-9)
    h.close()


def test_actor_off_gives_a_zero_actor_gradient_bit_for_bit(host):
    cfg = R.Cfg(actor_on=0, ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    h = HostLearner(host, cfg, case["params"])
    g = h.grad(case, idx)
    sl = R.block_slices()
    for name in R.ACTOR_BLOCKS:
        assert g[sl[name]].tobytes() == bytes(4 * (sl[name].stop - sl[name].start)), name
    _gate(g, R.grad_buffer(case, idx, cfg), "actor_on=0")   # the critic's gradient is vf_coef x the value loss's
    h.close()


def test_bad_indices_are_left_out_and_counted(host):
    cfg = R.Cfg(normalize_adv=0)
    case, idx = conditioned(65, cfg)
    h = HostLearner(host, cfg, case["params"])
    g = h.grad(case, idx)
    bad = np.concatenate([idx, np.array([-1, N_ROWS, 2 ** 31 - 1], np.int32)])
    g_bad = h.grad(case, bad)
    assert h.stats().bad_index == 3
    err = R.block_errors(g_bad * (68 / 65), g)   # the same sums under 1 / 68
    assert max(err.values()) <= R.GATE, err
    R.stats_close(g_bad * (68 / 65), g)
    h.close()


def test_linearity_the_data_parallel_contract(host):
    """normalize_adv=0: the average of the gradient buffers of two disjoint halves is the buffer of the whole minibatch"""
    cfg = R.Cfg(normalize_adv=0, ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    h = HostLearner(host, cfg, case["params"])
    whole, a, b = h.grad(case, idx), h.grad(case, idx[:500]), h.grad(case, idx[500:])
    g64 = R.grad_buffer(case, idx, cfg)
    _gate(0.5 * (a.astype(np.float64) + b), g64, "mean of two halves")
    _gate(whole, g64, "whole")
    h.close()


# --------------------------------------------------------------------------------------- 2. clip + Adam
def _update_errors(theta_before, theta_after, ref_before, ref_after):
    """per block |dtheta - dtheta_ref| / |dtheta_ref| of one step's update"""
    d, dr = theta_after.astype(np.float64) - theta_before, ref_after.astype(np.float64) - ref_before
    return {name: float(np.linalg.norm(d[sl] - dr[sl]) / np.linalg.norm(dr[sl])) for name, sl in R.block_slices().items()}


@pytest.mark.parametrize("joint", [0, 1])
def test_apply_against_torch_adam_from_given_gradients(host, joint):
    """five steps from given gradient vectors: both sides do the same few fp32 operations per element in a different order, so
    the update of a step agrees to rtol 1e-6 -- taken per parameter block in the 2-norm, as every gate here is: element by
    element a moment that nearly cancels (0.9 m + 0.1 g close to 0) has no relative accuracy on either side.  Adam's update
    does not depend on theta, so theta starts at ZERO: theta stays of the size of the updates and the difference of two fp32
    thetas IS the update (from an initialised network one update is 1e-4 of theta, and a rounding of theta that falls the other
    way is 1e-4 of the update, whatever the learner did)"""
    cfg = R.Cfg(joint_norm=joint)
    rng = np.random.default_rng(5)
    theta0 = np.zeros(NPARAM, np.float32)
    h, t = HostLearner(host, cfg, theta0), R.TorchLearner(theta0, cfg)
    worst = 0.0
    for step in range(5):
        g = np.zeros(NPARAM + NSTAT, np.float32)
        g[:NPARAM] = rng.standard_normal(NPARAM) * (0.02 if step % 2 else 0.002)   # norms on both sides of max_grad_norm = 0.5
        before_h, before_t = h.params.copy(), t.flat()
        h.apply(g); t.apply(g)
        s = h.stats()
        npi = np.linalg.norm(np.concatenate([g[:R.block_slices()["vf.W1"].start], g[NPARAM - 2:NPARAM]]).astype(np.float64))
        nall = np.linalg.norm(g[:NPARAM].astype(np.float64))
        np.testing.assert_allclose(s.grad_norm_pi, nall if joint else npi, rtol=1e-6)
        err = _update_errors(before_h, h.params, before_t, t.flat())
        worst = max(worst, max(err.values()))
        assert max(err.values()) <= 1e-6, (step, err)
    print(f"joint_norm={joint}: largest per-block relative error of an Adam update = {worst:.3g}")
    assert h.stats().steps == 5
    h.close()


@pytest.mark.parametrize("separate", [True, False])
def test_five_full_steps_against_the_fp64_restatement(host, separate):
    """grad + apply five times: |theta - theta64| <= 4 |theta32torch - theta64| per block, the right-hand side measured here"""
    cfg = R.Cfg(joint_norm=int(not separate), ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    h = HostLearner(host, cfg, case["params"])
    t64, t32 = R.TorchLearner(case["params"], cfg, torch.float64), R.TorchLearner(case["params"], cfg, torch.float32)
    for _ in range(5):
        h.grad(case, idx); h.apply()
        t64.step(case, idx); t32.step(case, idx)
    worst = 0.0
    for name, sl in R.block_slices().items():
        mine, torch32 = np.linalg.norm(h.params[sl] - t64.flat()[sl]), np.linalg.norm(t32.flat()[sl] - t64.flat()[sl])
        worst = max(worst, mine / torch32)
        assert mine <= 4 * torch32, (name, mine, torch32)
    print(f"separate_clip={separate}: largest |theta - theta64| / |theta32torch - theta64| over the blocks after five steps = {worst:.3g}")
    assert np.linalg.norm(h.params - case["params"]) > 1e-3   # the parameters moved
    h.close()


def test_early_stop_is_sticky_until_begin_iteration(host):
    case, idx = conditioned(1000)
    kl = float(R.grad_buffer(case, idx, R.Cfg())[NPARAM + 3])
    assert kl > 1e-4
    cfg = R.Cfg(target_kl=kl / 3)   # 1.5 x target_kl = kl / 2 < kl
    h = HostLearner(host, cfg, case["params"])
    h.cfg = R.Cfg(target_kl=10 * kl)
    h.grad(case, idx); h.apply()    # below the target: a step is taken
    assert h.stats().steps == 1 and not h.stats().stopped
    h.cfg = cfg
    frozen = [h.params.copy(), h.m.copy(), h.v.copy()]
    for later_cfg in (cfg, R.Cfg(), R.Cfg(target_kl=10 * kl)):   # sticky: later calls change nothing, whatever their KL
        h.cfg = later_cfg
        h.grad(case, idx); h.apply()
        s = h.stats()
        assert s.stopped == 1 and s.steps == 1
        for a, b in zip(frozen, (h.params, h.m, h.v)):
            assert a.tobytes() == b.tobytes()
        np.testing.assert_allclose(s.stat[3], h.grad_buf[NPARAM + 3])   # the stats slot still reports what apply saw
    h.begin_iteration()
    h.grad(case, idx); h.apply()
    assert h.stats().steps == 2 and not h.stats().stopped and h.params.tobytes() != frozen[0].tobytes()
    h.close()


# --------------------------------------------------------------------------------------- 3. the same code under the sanitizers
def _fnv(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_stand_alone_program_is_clean_under_asan_and_ubsan(host, tmp_path):
    """learnerhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests, and
    they are the digests of what the library build returns"""
    cfg = R.Cfg(ent_coef=0.01)
    case, idx = conditioned(65, cfg)
    steps, max_wg = 2, 0
    path = tmp_path / "case_65.bin"
    with open(path, "wb") as f:
        f.write(np.array([N_ROWS, idx.size, max_wg, steps], np.int32).tobytes())
        f.write(bytes(cfg.c()))
        for k in ("params", "obs", "act", "logp_old", "adv", "ret"):
            f.write(case[k].tobytes())
        f.write(idx.tobytes())
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"learnerhost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(HOST_DIR, "learnerhost_main.cpp")])
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    h = HostLearner(host, cfg, case["params"], max_wg)
    for _ in range(steps):
        h.grad(case, idx); h.apply()
    assert out["plain"] == f"m=65 steps={steps} bad=0 grad={_fnv(h.grad_buf.tobytes()):016x} params={_fnv(h.params.tobytes()):016x}\n"
    h.close()


# --------------------------------------------------------------------------------------- 4. C ABI without a device
LEARNER_SYMBOLS = ("brs_learner_create", "brs_learner_destroy", "brs_learner_last_error", "brs_learner_begin_iteration", "brs_learner_grad",
                   "brs_learner_apply", "brs_learner_stats")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in LEARNER_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    assert len([s for s in _lib.SIGNATURES["brs_policy.h"] if s.startswith("brs_learner_")]) == 7
    assert C.sizeof(_lib.BrsPpoConfig) == 4 * 8 + 7 * 4 + 3 * 4 and C.sizeof(_lib.BrsLearnerInfo) == 8 + 4 + 4 + 5 * 4 + 4 + 4 + 4
    assert ("brs_learner.hip", [], False) in _lib.UNITS
    assert _lib.POLICY_NPARAM + _lib.LEARNER_NSTAT == 9413 + 5


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    h, buf, cfg = C.c_void_p(1), C.c_void_p(8), R.Cfg().c()
    assert L.brs_learner_create(0, 0, None) == ERR_ARG and L.brs_learner_last_error(None) == b"brs_learner_create: null argument"
    grad = lambda handle, idx, m, c: L.brs_learner_grad(handle, buf, 8, buf, buf, buf, buf, buf, idx, m, c, buf, None)
    for args, why in (((None, buf, 8, None), b"brs_learner_grad: null config"),
                      ((None, None, 8, C.byref(cfg)), b"brs_learner_grad: null idx"),
                      ((None, buf, 1, C.byref(cfg)), b"brs_learner_grad: a minibatch needs at least two samples (unbiased std)"),
                      ((None, None, 0, C.byref(cfg)), b"brs_learner_grad: a minibatch needs at least two samples (unbiased std)"),
                      ((None, buf, -5, C.byref(cfg)), b"brs_learner_grad: a minibatch needs at least two samples (unbiased std)"),
                      ((None, buf, 8, C.byref(cfg)), b"brs_learner_grad: null handle")):
        assert grad(*args) == ERR_ARG and L.brs_learner_last_error(None) == why, why
    assert L.brs_learner_apply(None, buf, buf, buf, buf, None, None) == ERR_ARG
    assert L.brs_learner_last_error(None) == b"brs_learner_apply: null config"
    assert L.brs_learner_apply(None, buf, buf, buf, buf, C.byref(cfg), None) == ERR_ARG
    assert L.brs_learner_last_error(None) == b"brs_learner_apply: null handle"
    assert L.brs_learner_begin_iteration(None, None) == ERR_ARG and L.brs_learner_stats(None, C.byref(_lib.BrsLearnerInfo()), None) == ERR_ARG
    assert L.brs_learner_destroy(None) == ERR_STATE
    del h


def test_create_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.brs_policy_create(0, None) == ERR_ARG   # another family's last error ...
    assert L.brs_learner_create(0, 0, C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_learner_last_error(None)
    assert msg.startswith(b"brs_learner_create: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    assert b"brs_policy_create" in L.brs_policy_last_error(None)   # ... stays its own: one slot per family
    from balance_robot_mujoco_rl_amd import BrsError, DevicePPOLearner
    with pytest.raises(BrsError):
        DevicePPOLearner()


# --------------------------------------------------------------------------------------- 5. the Python layer's conversions
def _tool_state_dict(seed=0):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_ppo_torch as T
    torch.manual_seed(seed)
    model = T.ActorCritic(-0.5)
    model.ret_scale.fill_(2.5)
    return model, model.state_dict()


def test_state_dict_round_trips_in_both_namings():
    from balance_robot_mujoco_rl_amd.policy import SB3_LAYOUT, flatten_sb3_state_dict
    model, sd = _tool_state_dict()
    flat, rs = learner.flatten_state_dict(sd)
    assert rs == 2.5 and flat.dtype == np.float32 and flat.size == NPARAM
    back = learner.unflatten_state_dict(flat, "tool", rs)
    assert sorted(back) == sorted(sd)
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    model.load_state_dict(back)   # the tool's module takes it
    # the flat order is brs_policy.h's: the tool's flat_params, with the critic's unit folded in as rollout_params() does
    import train_ppo_torch as T
    want = T.flat_params(model).numpy()
    mine = flat.copy(); mine[learner.CRITIC_HEAD] *= rs
    np.testing.assert_array_equal(mine, want)
    # SB3's naming: same vector, no ret_scale entry; a unit other than 1 is folded into value_net
    sb3 = learner.unflatten_state_dict(flat, "sb3")
    assert sorted(sb3) == sorted(n for n, _ in SB3_LAYOUT) and learner.naming_of(sb3) == "sb3"
    np.testing.assert_array_equal(flatten_sb3_state_dict(sb3), flat)
    flat2, rs2 = learner.flatten_state_dict(sb3)
    assert rs2 == 1.0
    np.testing.assert_array_equal(flat2, flat)
    again = learner.unflatten_state_dict(flat2, "sb3", rs2)
    for k in sb3:
        assert torch.equal(again[k], sb3[k]), k
    folded = learner.unflatten_state_dict(flat, "sb3", 2.5)
    assert torch.equal(folded["value_net.weight"], sb3["value_net.weight"] * 2.5) and torch.equal(folded["value_net.bias"], sb3["value_net.bias"] * 2.5)
    with pytest.raises(ValueError):
        learner.flatten_state_dict({"weight": 1})
    with pytest.raises(ValueError):
        learner.flatten_state_dict({**sd, "pi.0.weight": torch.zeros(6, 64)})
