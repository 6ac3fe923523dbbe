"""The DDPG learner (include/brs_policy.h: brs_ddpg_learner_*) without a GPU: the host build of the kernel source
(tests/ddpglearnerhost: the shared header brs_ddpg_learner.hpp with a plain-loop forward/backward) against fp64 torch autograd
(tests/ref_ddpg_learner.py); the same host code as a program under the sanitizers; the C ABI's argument checks; the Python layer's
state_dict; the tool's usage error."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ref_ddpg_learner as RL
import ref_offpolicy as R
from balance_robot_mujoco_rl_amd import _lib, offpolicy
from ddpg_learner_cases import (ADAM, CPU_ROWS, HOST_DIR, SPLIT_LAST_REAL, SPLIT_ROWS, SPLIT_TABLE, STEP_ROWS, STEPS, WEIGHT_SETS, HostDDPG, adam_config, block_distances, build_host,
                                check_gradient, check_trajectory, host_actor_grad, host_critic_grad, learner_case, references, trajectory_case)
from offpolicy_cases import GXX, ROOT, gate

ERR_ARG, ERR_HIP, ERR_STATE = -1, -2, -3


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("ddpglearnerhost"))


# --------------------------------------------------------------------------------------- 1. the two gradients
@pytest.mark.parametrize("kind", WEIGHT_SETS)
@pytest.mark.parametrize("n", CPU_ROWS)
def test_host_gradients_against_fp64(host, n, kind):
    c = learner_case(n, kind)
    c64, a64, c32, a32 = references(n, kind)
    check_gradient(f"n={n} {kind} critic", host_critic_grad(host, c["critic"], c["obs"], c["act"], c["y"]), c64, c32, R.CRITIC_SIZES, gate)
    check_gradient(f"n={n} {kind} actor", host_actor_grad(host, c["actor"], c["critic"], c["obs"]), a64, a32, R.ACTOR_SIZES, gate)


def test_conditions_hold_and_do_what_they_are_for():
    c = learner_case(1000, "x3")
    pre = RL.preactivations(c["actor"], c["critic"], c["obs"], c["act"])
    assert np.abs(pre).min() >= 1e-4
    tq, tz = RL.row_terms(c["actor"], c["critic"], c["obs"], c["act"], c["y"])
    for t in (tq, tz[:, 0], tz[:, 1]):
        assert abs(t.sum()) >= 0.25 * np.abs(t).sum()
    a64 = references(1000, "x3")[1]
    assert a64[-1] > 0.5   # the x3 set saturates the tanh: the mean of pi(s)^2 says so


@pytest.mark.parametrize("kind", WEIGHT_SETS)
def test_linearity_the_data_parallel_contract(host, kind):
    """the buffer of the whole batch is the row-weighted mean of the buffers of two unequal halves, to 1e-6 per block"""
    c = learner_case(257, kind)
    k, n = 100, 257
    lo, hi = slice(0, k), slice(k, n)
    part = lambda s: {x: np.ascontiguousarray(c[x][s]) for x in ("obs", "act", "y")}
    for sizes, run in ((R.CRITIC_SIZES, lambda p: host_critic_grad(host, c["critic"], p["obs"], p["act"], p["y"])),
                       (R.ACTOR_SIZES, lambda p: host_actor_grad(host, c["actor"], c["critic"], p["obs"]))):
        whole, a, b = run(part(slice(0, n))), run(part(lo)), run(part(hi))
        mix = (k * a.astype(np.float64) + (n - k) * b.astype(np.float64)) / n
        d = block_distances(whole[:-2], mix[:-2], sizes)
        print(f"{kind}: largest block distance of whole from the weighted halves = {max(d.values()):.3g}")
        assert max(d.values()) <= 1e-6, d
        np.testing.assert_allclose(whole[-2:], mix[-2:], rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------------------------------- 2. apply
def _update_errors(before, after, before_t, after_t, sizes):
    return block_distances(after.astype(np.float64) - before, after_t.astype(np.float64) - before_t, sizes)


def test_apply_against_torch_adam_from_given_gradients(host):
    """five steps from given gradient vectors with the parameters starting at ZERO (so that the difference of two fp32 thetas is
    the update): the update agrees with torch.optim.Adam to rtol 1e-6 per block; the target follows the fp64 formula
    target + tau (param_new - target) to 1e-6 of its update; target NULL leaves no target written"""
    rng = np.random.default_rng(5)
    h = HostDDPG(host, np.zeros(RL.NACTOR, np.float32), np.zeros(RL.NCRITIC, np.float32), **ADAM)
    t = RL.TorchAdam(np.zeros(RL.NCRITIC, np.float32), torch.float32, **ADAM)
    worst = worst_t = 0.0
    for step in range(5):
        g = (rng.standard_normal(RL.NCRITIC + 2) * (0.02 if step % 2 else 0.002)).astype(np.float32)
        before, before_t, target0 = h.flat["critic"].copy(), t.p.detach().numpy().copy(), h.flat["critic_target"].copy()
        h.apply("critic", g); t.apply(g[:RL.NCRITIC])
        err = _update_errors(before, h.flat["critic"], before_t, t.p.detach().numpy(), R.CRITIC_SIZES)
        worst = max(worst, max(err.values()))
        assert max(err.values()) <= 1e-6, (step, err)
        want = ADAM["tau"] * (h.flat["critic"].astype(np.float64) - target0)
        err_t = block_distances(h.flat["critic_target"].astype(np.float64) - target0, want, R.CRITIC_SIZES)
        worst_t = max(worst_t, max(err_t.values()))
        assert max(err_t.values()) <= 1e-6, (step, err_t)
        np.testing.assert_allclose(h.flat["critic_target"], t.target.numpy(), rtol=0, atol=1e-6 * np.abs(t.target.numpy()).max())
    print(f"largest per-block relative error of an Adam update = {worst:.3g}, of a Polyak update = {worst_t:.3g}")
    assert h.steps["critic"] == 5
    # without a target nothing but params, m and v is written
    frozen = h.flat["actor_target"].copy()
    h.apply("actor", (rng.standard_normal(RL.NACTOR + 2) * 0.01).astype(np.float32), target=False)
    assert h.flat["actor_target"].tobytes() == frozen.tobytes() and np.abs(h.flat["actor"]).max() > 0
    # any n_param >= 1: one element
    p, g, m, v, tg = (np.array([x], np.float32) for x in (0.5, 0.25, 0.0, 0.0, 0.5))
    cfg = adam_config(**ADAM)
    assert host.dh_apply(1, p.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, tg.ctypes.data, C.byref(cfg), 1, 0.5) == 0
    assert abs(p[0] - (0.5 - 1e-3)) < 1e-7 and abs(tg[0] - (0.5 + 0.5 * (p[0] - 0.5))) < 1e-7


def test_apply_element_is_adam_update_operation_by_operation(host):
    """brs_learner.hpp's adam_update and this learner's apply_element (the same arithmetic with contraction off, for byte
    identity between kernel and host build) return the same bytes under g++, over five steps: the two cannot drift apart"""
    rng = np.random.default_rng(9)
    n, cfg = 4096, adam_config(**ADAM)
    a, b = ([np.zeros(n, np.float32) for _ in range(3)] for _ in range(2))
    for step in range(1, 6):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)).astype(np.float32)
        host.dh_adam_pair(n, g.ctypes.data, C.byref(cfg), step, *[x.ctypes.data for x in a + b])
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes() and np.isfinite(x).all()
    assert np.abs(a[0]).max() > 1e-3


def test_five_full_steps_against_the_fp64_restatement(host):
    """critic_grad, apply, actor_grad with the updated critic, apply, five times on five minibatches: per block,
    |d - d64| <= 4 |d32torch - d64| for d = theta_5 - theta_0, the right-hand side measured here and floored at its largest value
    over the blocks of the network"""
    case = trajectory_case("init")
    h = HostDDPG(host, case["actor"], case["critic"], **ADAM)
    for s in range(STEPS):
        sl = slice(s * STEP_ROWS, (s + 1) * STEP_ROWS)
        h.step(np.ascontiguousarray(case["obs"][sl]), np.ascontiguousarray(case["act"][sl]), np.ascontiguousarray(case["y"][sl]))
    worst = check_trajectory("host build", h.flat, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| over the blocks after five steps = {worst:.3g}")
    assert h.flat["actor"].tobytes() != case["actor"].tobytes()   # (the arrays of the case are never written)
    assert np.linalg.norm(h.flat["actor"] - case["actor"]) > 1e-3 and np.linalg.norm(h.flat["critic"] - case["critic"]) > 1e-3
    assert not np.array_equal(h.flat["actor_target"], case["actor"])


# --------------------------------------------------------------------------------------- 3. the same code under the sanitizers
def _fnv(a):
    h = 14695981039346656037
    for b in a.tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_stand_alone_program_is_clean_under_asan_and_ubsan(host, tmp_path):
    """ddpglearnerhost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds print the same digests, and
    they are the digests of what the library build returns"""
    m, steps = 33, 2
    c = learner_case(257, "init")
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([m, steps], np.int32).tobytes()); f.write(np.array([ADAM["tau"]], np.float32).tobytes())
        f.write(np.array([ADAM["lr"], *ADAM["betas"], ADAM["eps"]], np.float64).tobytes())
        f.write(c["actor"].tobytes()); f.write(c["critic"].tobytes())
        for s in range(steps):
            for k in ("obs", "act", "y"):
                f.write(np.ascontiguousarray(c[k][s * m:(s + 1) * m]).tobytes())
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"ddpglearnerhost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(HOST_DIR, "ddpglearnerhost_main.cpp")])
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"]
    h = HostDDPG(host, c["actor"], c["critic"], **ADAM)
    for s in range(steps):
        sl = slice(s * m, (s + 1) * m)
        obs, act, y = (np.ascontiguousarray(c[k][sl]) for k in ("obs", "act", "y"))
        gc = host_critic_grad(host, h.flat["critic"], obs, act, y); h.apply("critic", gc)
        ga = host_actor_grad(host, h.flat["actor"], h.flat["critic"], obs); h.apply("actor", ga)
    assert out["plain"] == (f"m={m} steps={steps} actor={_fnv(h.flat['actor']):016x} critic={_fnv(h.flat['critic']):016x} "
                            f"actor_target={_fnv(h.flat['actor_target']):016x} critic_target={_fnv(h.flat['critic_target']):016x} "
                            f"ga={_fnv(ga):016x} gc={_fnv(gc):016x}\n")


# --------------------------------------------------------------------------------------- 3b. the split of the sample axis
MAX_BATCH = 1 << 22   # the ABI's range of max_batch (brs_ddpg_learner_create)
SPLIT_RULES = ("span is no multiple of 128", "nsplit is outside [1, 8]", "nsplit * span < mp", "(nsplit - 1) * span >= m: a split without a real row",
               "nsplit == 1 is not the same as mp < 512", "the partial rows do not fit the allocation", "mp is not m padded to 128")


def _split(host, m):
    out = (C.c_int * 3)()
    host.dh_sample_split(m, C.byref(out))
    return tuple(out)


def test_sample_split_over_every_batch_size_of_the_abi(host):
    """brs_ddpg_learner.hpp's sample_split, the function launch_weight_kernels calls, for every m in [1, 2^22], the loop run inside
    the host library: span a multiple of 128, 1 <= nsplit <= 8, the splits cover mp, every launched split holds a real row,
    one split exactly below 512 padded rows, and nsplit partial rows fit what the handle allocates (single and twin).  Then the
    nine geometries of ddpg_learner_cases' table as known answers."""
    first, mask = C.c_int(), C.c_uint()
    bad = host.dh_split_sweep(1, MAX_BATCH, C.byref(first), C.byref(mask))
    assert bad == 0, (bad, first.value, [r for k, r in enumerate(SPLIT_RULES) if mask.value >> k & 1], _split(host, first.value))
    for m, want in SPLIT_TABLE.items():
        assert _split(host, m) == want, (m, _split(host, m), want)
    for m in (1, 128, 383, 384):
        assert _split(host, m)[2] == 1
    assert set(SPLIT_ROWS) | {384, 1000} == set(SPLIT_TABLE)
    for m, real in SPLIT_LAST_REAL.items():
        mp, span, nsplit = _split(host, m)
        assert m - (nsplit - 1) * span == real and min(span, mp - (nsplit - 1) * span) >= real


def test_split_sweep_in_the_stand_alone_program_under_asan_and_ubsan(tmp_path):
    """the same sweep in ddpglearnerhost_main.cpp built with -fsanitize=address,undefined: no overflow in the split's integer
    arithmetic anywhere in the ABI's range, and the table's rows as the program prints them"""
    exe = str(tmp_path / "ddpglearnerhost_san")
    subprocess.check_call(GXX + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                                 os.path.join(HOST_DIR, "ddpglearnerhost_main.cpp")])
    r = subprocess.run([exe, "--split-sweep", "1", str(MAX_BATCH)] + [str(m) for m in SPLIT_TABLE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[0] == f"sweep 1..{MAX_BATCH} bad=0 first=0 mask=0"
    assert lines[1:] == [f"{m} {mp} {span} {nsplit}" for m, (mp, span, nsplit) in SPLIT_TABLE.items()]


# --------------------------------------------------------------------------------------- 4. C ABI without a device
SYMBOLS = ("brs_ddpg_learner_create", "brs_ddpg_learner_destroy", "brs_ddpg_learner_last_error", "brs_ddpg_learner_scratch", "brs_ddpg_learner_critic_grad",
           "brs_ddpg_learner_actor_grad", "brs_ddpg_learner_apply")


def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    assert ("brs_ddpg_learner.hip", [], False) in _lib.UNITS
    assert _lib.DDPG_NSTAT == RL.NSTAT == 2
    hdr = open(os.path.join(ROOT, "include", "brs_policy.h")).read()
    assert "#define BRS_DDPG_NSTAT 2" in hdr
    assert C.sizeof(_lib.BrsAdamConfig) == 4 * C.sizeof(C.c_double)


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    buf = C.c_void_p(64)
    err = lambda: L.brs_ddpg_learner_last_error(None)
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create(0, 256, None) == ERR_ARG and err() == b"brs_ddpg_learner_create: null argument"
    for bad in (0, -5):
        assert L.brs_ddpg_learner_create(0, bad, C.byref(h)) == ERR_ARG and h.value is None
        assert err() == b"brs_ddpg_learner_create: max_batch must be in [1, 2^22]"
    cg = lambda m, critic=buf, y=buf, out=buf: L.brs_ddpg_learner_critic_grad(None, critic, m, buf, buf, y, out, None)
    for args, why in (((4, None), b"null argument"), ((4, buf, None), b"null argument"), ((4, buf, buf, None), b"null argument"),
                      ((0,), b"m must be at least 1"), ((-2,), b"m must be at least 1"), ((4,), b"null handle")):
        assert cg(*args) == ERR_ARG and err() == b"brs_ddpg_learner_critic_grad: " + why, why
    ag = lambda m, actor=buf, critic=buf, obs=buf: L.brs_ddpg_learner_actor_grad(None, actor, critic, m, obs, buf, None)
    for args, why in (((4, None), b"null argument"), ((4, buf, None), b"null argument"), ((4, buf, buf, None), b"null argument"),
                      ((0,), b"m must be at least 1"), ((4,), b"null handle")):
        assert ag(*args) == ERR_ARG and err() == b"brs_ddpg_learner_actor_grad: " + why, why
    good = dict(n=8, params=buf, grad=buf, m=buf, v=buf, cfg=(1e-3, 0.9, 0.999, 1e-8), step=1, tau=0.005)

    def ap(**kw):
        a = {**good, **kw}
        cfg = None if a["cfg"] is None else C.byref(_lib.BrsAdamConfig(*a["cfg"]))
        return L.brs_ddpg_learner_apply(None, a["n"], a["params"], a["grad"], a["m"], a["v"], None, cfg, a["step"], a["tau"], None)
    nan = float("nan")
    for kw, why in ((dict(cfg=None), b"null config"), (dict(params=None), b"null argument"), (dict(grad=None), b"null argument"),
                    (dict(m=None), b"null argument"), (dict(v=None), b"null argument"), (dict(n=0), b"n_param must be at least 1"),
                    (dict(step=0), b"step must be at least 1"), (dict(step=-1), b"step must be at least 1"),
                    (dict(tau=-0.1), b"tau must be in [0, 1]"), (dict(tau=1.5), b"tau must be in [0, 1]"), (dict(tau=nan), b"tau must be in [0, 1]"),
                    (dict(cfg=(-1e-3, 0.9, 0.999, 1e-8)), b"lr and eps must be >= 0"), (dict(cfg=(1e-3, 0.9, 0.999, -1.0)), b"lr and eps must be >= 0"),
                    (dict(cfg=(nan, 0.9, 0.999, 1e-8)), b"lr and eps must be >= 0"),
                    (dict(cfg=(1e-3, 1.0, 0.999, 1e-8)), b"betas must be in [0, 1)"), (dict(cfg=(1e-3, 0.9, -0.1, 1e-8)), b"betas must be in [0, 1)"),
                    (dict(), b"null handle"), (dict(tau=0.0), b"null handle"), (dict(tau=1.0, cfg=(0.0, 0.0, 0.0, 0.0)), b"null handle")):
        assert ap(**kw) == ERR_ARG and err() == b"brs_ddpg_learner_apply: " + why, (kw, err())
    ptr, size = C.c_void_p(), C.c_int64()
    assert L.brs_ddpg_learner_scratch(None, None, C.byref(size)) == ERR_ARG and err() == b"brs_ddpg_learner_scratch: null argument"
    assert L.brs_ddpg_learner_scratch(None, C.byref(ptr), C.byref(size)) == ERR_ARG and err() == b"brs_ddpg_learner_scratch: null handle"
    assert L.brs_ddpg_learner_destroy(None) == ERR_STATE
    assert L.brs_ddpg_last_error(None) != err()   # a slot of its own family


def test_everything_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create(0, 256, C.byref(h)) == ERR_HIP and h.value is None
    msg = L.brs_ddpg_learner_last_error(None)
    assert msg.startswith(b"brs_ddpg_learner_create: no HIP device (") and msg.endswith(b"); there is no CPU fallback"), msg
    from balance_robot_mujoco_rl_amd import BrsError, DeviceDDPGLearner
    with pytest.raises(BrsError):
        DeviceDDPGLearner()


# --------------------------------------------------------------------------------------- 5. the Python layer and the tool
def test_state_dict_round_trip():
    """the moments and the counters; the object is put together without a handle (its state_dict methods touch only tensors)"""
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner

    def bare(fill):
        o = object.__new__(DeviceDDPGLearner)
        o.device, o.h = torch.device("cpu"), None
        o.m_critic, o.v_critic = torch.full((RL.NCRITIC,), fill), torch.full((RL.NCRITIC,), 2 * fill)
        o.m_actor, o.v_actor = torch.full((RL.NACTOR,), 3 * fill), torch.full((RL.NACTOR,), 4 * fill)
        o.steps_critic, o.steps_actor = int(10 * fill), int(20 * fill)
        return o
    a, b = bare(1.0), bare(0.0)
    sd = a.state_dict()
    assert sorted(sd) == ["m_actor", "m_critic", "steps_actor", "steps_critic", "v_actor", "v_critic"]
    sd_copy = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in sd.items()}
    a.m_critic.zero_()   # the state_dict is a copy
    assert torch.equal(sd["m_critic"], sd_copy["m_critic"])
    b.load_state_dict(sd)
    for k in ("m_critic", "v_critic", "m_actor", "v_actor"):
        assert torch.equal(getattr(b, k), sd_copy[k]) and getattr(b, k).dtype == torch.float32
    assert (b.steps_critic, b.steps_actor) == (10, 20)
    with pytest.raises(ValueError):
        b.load_state_dict({**sd, "m_actor": torch.zeros(5)})
    assert "DeviceDDPGLearner" in offpolicy.__dict__ and offpolicy.NACTOR == RL.NACTOR


def test_tool_device_learner_needs_device_data():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_ddpg_torch.py"), "--device-learner"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--device-learner requires --device-data" in r.stderr
