"""The A2C learner (include/brs_policy.h: brs_a2c_*) without a GPU: the host build of the kernel source
(tests/a2chost: the shared header brs_learner.hpp with learnerhost's plain loops for the towers) against fp64 torch autograd of
SB3's A2C.train() restated in tests/ref_a2c.py, the clip + RMSpropTFLike step against its restatement and against
torch.optim.RMSprop where the two coincide, the same host code as a program under the sanitizers, the C ABI's argument checks and
the Python layer's conversions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_a2c as A
import ref_learner as R
from a2c_cases import HOST_DIR, NPARAM, NSTAT, HostA2C, _ptr, build_host, conditioned, gate, head
from balance_robot_mujoco_rl_amd import _lib, learner
from learner_cases import GXX, N_ROWS, ROOT

ERR_ARG, ERR_STATE = -1, -3


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("a2chost"))


# --------------------------------------------------------------------------------------- 1. the gradient
@pytest.mark.parametrize("m", [2, 65, 1000])
def test_host_gradient_against_fp64_autograd(host, m):
    cfg = A.Cfg()
    case, idx = conditioned(m, cfg)
    h = HostA2C(host, cfg, case["params"])
    g = h.grad(case, idx)
    assert h.stats().bad_index == 0
    gate(g, A.grad_buffer(case, idx, cfg), f"m={m}")
    h.close()


@pytest.mark.parametrize("name,change", [("normalize_adv=1", dict(normalize_adv=1)), ("ent_coef=0.01", dict(ent_coef=0.01)),
                                         ("joint_norm=0", dict(joint_norm=0)), ("ret_scale=7", dict(ret_scale=7.0)),
                                         ("several chunks per workgroup", dict())])
def test_host_gradient_switches(host, name, change):
    cfg = A.Cfg(**change)
    case, idx = conditioned(1000, cfg)
    h = HostA2C(host, cfg, case["params"], max_workgroups=0 if change else 2)
    g = h.grad(case, idx)
    g64 = A.grad_buffer(case, idx, cfg)
    gate(g, g64, name)
    if "ent_coef" in change:   # the bonus is there: d(-ent_coef entropy) / d log_std = -ent_coef
        g0 = A.grad_buffer(case, idx, A.Cfg())
        np.testing.assert_allclose(g64[NPARAM - 2:NPARAM] - g0[NPARAM - 2:NPARAM], -0.01, rtol=1e-9)
    h.close()


def test_actor_off_gives_a_zero_actor_gradient_bit_for_bit(host):
    cfg = A.Cfg(actor_on=0, ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    h = HostA2C(host, cfg, case["params"])
    g = h.grad(case, idx)
    sl = R.block_slices()
    for name in R.ACTOR_BLOCKS:
        assert g[sl[name]].tobytes() == bytes(4 * (sl[name].stop - sl[name].start)), name
    g64 = A.grad_buffer(case, idx, cfg)
    gate(g, g64, "actor_on=0")   # the critic's gradient is vf_coef x the value loss's
    assert g64[NPARAM] != 0.0    # the policy loss is still reported
    h.close()


@pytest.mark.parametrize("normalize", [0, 1])
def test_null_idx_is_the_buffer_in_its_own_order_byte_for_byte(host, normalize):
    cfg = A.Cfg(normalize_adv=normalize, ent_coef=0.01)
    case, idx = conditioned(1000, cfg, whole=True)
    assert idx is None and case["obs"].shape[0] == 1000
    h = HostA2C(host, cfg, case["params"])
    g = h.grad(case, None)
    gate(g, A.grad_buffer(case, None, cfg), f"idx=NULL normalize_adv={normalize}")
    assert g.tobytes() == h.grad(case, np.arange(1000, dtype=np.int32)).tobytes()
    # m < n_rows: the first m rows
    full = conditioned(1000, cfg)[0]
    assert h.grad_rc(full, None, m=300) == 0
    assert h.grad_buf.tobytes() == h.grad(full, np.arange(300, dtype=np.int32)).tobytes()
    h.close()


def test_linearity_the_data_parallel_contract(host):
    """normalize_adv=0: the average of the gradient buffers of two disjoint halves is the buffer of the whole batch"""
    cfg = A.Cfg(ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    h = HostA2C(host, cfg, case["params"])
    whole, a, b = h.grad(case, idx), h.grad(case, idx[:500]), h.grad(case, idx[500:])
    g64 = A.grad_buffer(case, idx, cfg)
    gate((0.5 * (a.astype(np.float64) + b)).astype(np.float32), g64, "mean of two halves")
    gate(whole, g64, "whole")
    h.close()


def test_bad_indices_are_left_out_and_counted(host):
    cfg = A.Cfg()
    case, idx = conditioned(65, cfg)
    h = HostA2C(host, cfg, case["params"])
    g = h.grad(case, idx)
    g_bad = h.grad(case, np.concatenate([idx, np.array([-1, N_ROWS, 2 ** 31 - 1], np.int32)]))
    assert h.stats().bad_index == 3
    err = R.block_errors(g_bad * (68 / 65), g)   # the same sums under 1 / 68
    assert max(err.values()) <= R.GATE, err
    R.stats_close(g_bad * (68 / 65), g)
    h.close()


# --------------------------------------------------------------------------------------- 2. clip + RMSpropTFLike
def _update_errors(theta_before, theta_after, ref_before, ref_after):
    """per block |dtheta - dtheta_ref| / |dtheta_ref| of one step's update"""
    d, dr = theta_after.astype(np.float64) - theta_before, ref_after.astype(np.float64) - ref_before
    return {name: float(np.linalg.norm(d[sl] - dr[sl]) / np.linalg.norm(dr[sl])) for name, sl in R.block_slices().items()}


def _given_gradient(rng, step):
    g = np.zeros(NPARAM + NSTAT, np.float32)
    g[:NPARAM] = rng.standard_normal(NPARAM) * (0.02 if step % 2 else 0.002)   # norms on both sides of max_grad_norm = 0.5
    return g


@pytest.mark.parametrize("joint", [0, 1])
def test_apply_against_rmsprop_tf_like_from_given_gradients(host, joint):
    """tests/test_learner_cpu.py::test_apply_against_torch_adam_from_given_gradients with the optimiser exchanged -- its comparison
    and its tolerance: five steps from given gradient vectors, theta starts at ZERO so that the difference of two fp32 thetas IS the
    update, and the update of a step agrees with the fp32 restatement to 1e-6 per parameter block in the 2-norm"""
    cfg = A.Cfg(joint_norm=joint)
    rng = np.random.default_rng(5)
    theta0 = np.zeros(NPARAM, np.float32)
    h, t = HostA2C(host, cfg, theta0), A.TorchA2C(theta0, cfg, torch.float32)
    worst = 0.0
    for step in range(5):
        g = _given_gradient(rng, step)
        before_h, before_t = h.params.copy(), t.flat().copy()
        h.apply(g); t.apply(g)
        s = h.stats()
        nall = np.linalg.norm(g[:NPARAM].astype(np.float64))
        nvf = np.linalg.norm(g[R.block_slices()["vf.W1"].start:NPARAM - 2].astype(np.float64))
        np.testing.assert_allclose([s.grad_norm_pi, s.grad_norm_vf], [nall, nall] if joint else [np.sqrt(nall ** 2 - nvf ** 2), nvf], rtol=1e-6)
        err = _update_errors(before_h, h.params, before_t, t.flat())
        worst = max(worst, max(err.values()))
        assert max(err.values()) <= 1e-6, (step, err)
    print(f"joint_norm={joint}: largest per-block relative error of an RMSpropTFLike update = {worst:.3g}")
    np.testing.assert_allclose(h.sq, t.opt.sq.numpy(), rtol=1e-6)
    assert h.stats().steps == 5 and h.stats().stopped == 0
    h.close()


def _rmsprop(host, p, sq, g, cfg):
    p, sq, g = (np.array(a, np.float32) for a in (p, sq, g))
    c = cfg.c()
    host.ah_rmsprop(_ptr(p), _ptr(sq), _ptr(g), p.size, C.byref(c))
    return p, sq


def test_first_step_from_ones_in_closed_form(host):
    """square_avg starts at ONE and epsilon sits inside the root: p - lr g / sqrt(alpha + (1 - alpha) g^2 + eps)"""
    cfg = A.Cfg()
    rng = np.random.default_rng(7)
    p0, g = rng.standard_normal(4096).astype(np.float32), (rng.standard_normal(4096) * np.logspace(-4, 1, 4096)).astype(np.float32)
    p, sq = _rmsprop(host, p0, np.ones(4096, np.float32), g, cfg)
    g64, p64 = g.astype(np.float64), p0.astype(np.float64)
    want_sq = cfg.alpha + (1 - cfg.alpha) * g64 * g64
    np.testing.assert_allclose(sq, want_sq, rtol=3e-7)
    want_step = -cfg.lr * g64 / np.sqrt(want_sq + cfg.eps)
    np.testing.assert_allclose(p.astype(np.float64) - p64, want_step, rtol=1e-6, atol=2.0 ** -24 * np.abs(p64).max())   # one rounding of p
    # zeros would give another step: the start at one is observable
    assert not np.allclose(_rmsprop(host, p0, np.zeros(4096, np.float32), g, cfg)[0], p)


def test_with_eps_zero_it_is_torch_optim_rmsprop(host):
    """the pin that needs no SB3: eps = 0 removes the one difference in the formula, and a pre-loaded square_avg the one in the
    initial state -- then one step equals torch.optim.RMSprop(alpha, eps=0) with the same state"""
    cfg = A.Cfg(eps=0.0, lr=1e-2)
    rng = np.random.default_rng(9)
    n = 4096
    p0, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    sq0 = rng.uniform(0.1, 3.0, n).astype(np.float32)
    param = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.RMSprop([param], lr=cfg.lr, alpha=cfg.alpha, eps=0.0)
    param.grad = torch.from_numpy(g.copy())
    opt.step()   # creates the state (from zeros) ...
    with torch.no_grad():   # ... which is then set, the parameter put back, and the step under test taken
        param.copy_(torch.from_numpy(p0))
        opt.state[param]["square_avg"].copy_(torch.from_numpy(sq0))
    opt.step()
    p, sq = _rmsprop(host, p0, sq0, g, cfg)
    np.testing.assert_allclose(sq, opt.state[param]["square_avg"].numpy(), rtol=3e-7)
    # the two updates differ by a few roundings of a 1e-2-sized step, and each side rounds its new parameter once: one ulp of the
    # largest parameter covers both
    np.testing.assert_allclose(p, param.detach().numpy(), rtol=0, atol=float(np.spacing(np.abs(p0).max())))
    assert np.abs(p - p0).mean() > 1e-3   # the steps are four orders of magnitude above that


@pytest.mark.parametrize("separate", [True, False])
def test_five_full_steps_against_the_fp64_restatement(host, separate):
    """grad + clip + RMSpropTFLike five times: |theta - theta64| <= 4 |theta32torch - theta64| per block, the right-hand side
    measured here (the factor is the PPO learner's test's)"""
    cfg = A.Cfg(joint_norm=int(not separate), ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    h = HostA2C(host, cfg, case["params"])
    t64, t32 = A.TorchA2C(case["params"], cfg, torch.float64), A.TorchA2C(case["params"], cfg, torch.float32)
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
    assert h.stats().steps == 5
    h.close()


# --------------------------------------------------------------------------------------- 3. the same code under the sanitizers
def _fnv(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_stand_alone_program_is_clean_under_asan_and_ubsan(host, tmp_path):
    """a2chost_main.cpp has its own main: nothing sanitized is loaded into Python.  Both builds exit 0 and print the same digests,
    and they are the digests of what the library build returns; one case with an index list, one with idx = NULL"""
    cfg = A.Cfg(ent_coef=0.01, normalize_adv=1)
    steps, max_wg, paths, want = 2, 2, [], ""
    for whole, m in ((False, 65), (True, 300)):
        case, idx = conditioned(m, cfg, whole=whole)
        path = tmp_path / f"case_{m}.bin"
        with open(path, "wb") as f:
            f.write(np.array([case["obs"].shape[0], m, max_wg, steps, 0 if whole else 1], np.int32).tobytes())
            f.write(bytes(cfg.c()))
            for k in ("params",) + A.KEYS:
                f.write(case[k].tobytes())
            if not whole:
                f.write(idx.tobytes())
        paths.append(str(path))
        h = HostA2C(host, cfg, case["params"], max_wg)
        for _ in range(steps):
            h.grad(case, idx); h.apply()
        want += (f"m={m} steps={steps} bad=0 grad={_fnv(h.grad_buf.tobytes()):016x} params={_fnv(h.params.tobytes()):016x} "
                 f"sq={_fnv(h.sq.tobytes()):016x}\n")
        h.close()
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"a2chost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(HOST_DIR, "a2chost_main.cpp")])
        r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"] == want


# --------------------------------------------------------------------------------------- 4. C ABI without a device
def test_symbols_are_exported_and_in_the_table():
    L = _lib.lib()
    for name in ("brs_a2c_grad", "brs_a2c_apply"):
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    assert C.sizeof(_lib.BrsA2cConfig) == 3 * 8 + 5 * 4 + 3 * 4
    assert [f[0] for f in _lib.BrsA2cConfig._fields_] == ["lr", "alpha", "eps", "vf_coef", "ent_coef", "max_grad_norm_pi", "max_grad_norm_vf",
                                                          "ret_scale", "normalize_adv", "actor_on", "joint_norm"]


def test_argument_checks_that_need_no_device(host):
    L = _lib.lib()
    buf, cfg = C.c_void_p(8), A.Cfg().c()
    grad = lambda idx, m, c, n_rows=8: L.brs_a2c_grad(None, buf, n_rows, buf, buf, buf, buf, idx, m, c, buf, None)
    for args, why in (((buf, 8, None), b"brs_a2c_grad: null config"),
                      ((None, 9, C.byref(cfg)), b"brs_a2c_grad: null idx takes rows 0..m-1, m must not exceed n_rows"),
                      ((buf, 0, C.byref(cfg)), b"brs_a2c_grad: an update needs at least one sample"),
                      ((buf, 1, C.byref(A.Cfg(normalize_adv=1).c())), b"brs_a2c_grad: normalize_adv needs at least two samples (unbiased std)"),
                      ((buf, 8, C.byref(A.Cfg(ret_scale=0.0).c())), b"brs_a2c_grad: ret_scale must be positive"),
                      ((buf, 8, C.byref(A.Cfg(ret_scale=-1.0).c())), b"brs_a2c_grad: ret_scale must be positive"),
                      ((buf, 1, C.byref(cfg)), b"brs_a2c_grad: null handle"),    # m = 1 is a batch without normalize_adv
                      ((None, 8, C.byref(cfg)), b"brs_a2c_grad: null handle")):  # and a null idx with m <= n_rows is one too
        assert grad(*args) == ERR_ARG and L.brs_learner_last_error(None) == why, why
    assert L.brs_a2c_apply(None, buf, buf, buf, None, None) == ERR_ARG and L.brs_learner_last_error(None) == b"brs_a2c_apply: null config"
    assert L.brs_a2c_apply(None, buf, buf, buf, C.byref(cfg), None) == ERR_ARG and L.brs_learner_last_error(None) == b"brs_a2c_apply: null handle"
    # the host build refuses the same calls
    case = conditioned(65)[0]
    h = HostA2C(host, A.Cfg(), case["params"])
    assert h.grad_rc(case, None, m=N_ROWS + 1) == ERR_ARG and h.grad_rc(case, None, m=N_ROWS) == 0
    h.cfg = A.Cfg(ret_scale=0.0)
    assert h.grad_rc(case, None) == ERR_ARG
    h.cfg = None
    assert h.grad_rc(case, None) == ERR_ARG
    h.close()


def test_create_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    from balance_robot_mujoco_rl_amd import BrsError, DeviceA2CLearner
    with pytest.raises(BrsError):
        DeviceA2CLearner()


# --------------------------------------------------------------------------------------- 5. the Python layer
def test_defaults_are_sb3s_in_this_projects_value_loss_convention():
    import inspect
    from balance_robot_mujoco_rl_amd import DeviceA2CLearner
    d = {k: p.default for k, p in inspect.signature(DeviceA2CLearner.__init__).parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(device=0, lr=7e-4, alpha=0.99, eps=1e-5, vf_coef=1.0, ent_coef=0.0, max_grad_norm=0.5, normalize_advantage=False,
                     separate_clip=False, ret_scale=1.0, actor_on=True, max_workgroups=0)
    assert "vf_coef = 1.0" in DeviceA2CLearner.__doc__
    for method in ("load", "state_dict", "rollout_params", "grad", "apply", "step", "stats", "close"):
        assert callable(getattr(DeviceA2CLearner, method))


def test_state_dict_round_trips_in_both_namings():
    """the conversions DeviceA2CLearner.load / state_dict go through, with the tool's own module"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_a2c_torch as T
    torch.manual_seed(0)
    model = T.ActorCritic(-0.5)
    model.ret_scale.fill_(2.5)
    sd = model.state_dict()
    flat, rs = learner.flatten_state_dict(sd)
    assert rs == 2.5 and flat.size == NPARAM
    for naming in ("tool", "sb3"):
        back = learner.unflatten_state_dict(flat, naming, 1.0 if naming == "sb3" else rs)
        flat2, rs2 = learner.flatten_state_dict(back)
        np.testing.assert_array_equal(flat2, flat)
        assert rs2 == (1.0 if naming == "sb3" else 2.5)
    model.load_state_dict(learner.unflatten_state_dict(flat, "tool", rs))
    # the tool's RMSpropTFLike is the restatement's
    p = [torch.nn.Parameter(torch.from_numpy(flat.copy()))]
    opt, ref = T.RMSpropTFLike(p, lr=7e-4, alpha=0.99, eps=1e-5), A.RmspropTFLike64(flat, dtype=torch.float32)
    rng = np.random.default_rng(2)
    for _ in range(3):
        g = rng.standard_normal(NPARAM).astype(np.float32)
        p[0].grad = torch.from_numpy(g.copy())
        opt.step(); ref.step(g)
    assert torch.equal(p[0].detach(), ref.p)
