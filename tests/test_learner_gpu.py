"""The PPO learner's HIP kernels (include/brs_policy.h: brs_learner_*) on the GPU: the gradient against fp64 torch
autograd of the tool's minibatch body at the tile, wave and workgroup edges, determinism, guard rows around every output, clip +
Adam against torch.optim.Adam, the early stop, the kernels against the host build of the same source, the rollout parameters, and
stage 1 of the curriculum trained with the learner in place of torch's gradient step."""
import os
import sys
import time

import numpy as np
import pytest
import torch

import ref_learner as R
from learner_cases import N_ROWS, NPARAM, NSTAT, ROOT, HostLearner, build_host, conditioned, gate

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "tools"))
KEYS = ("obs", "act", "logp_old", "adv", "ret")


def _learner(cfg, params, max_workgroups=0):
    from balance_robot_mujoco_rl_amd import DevicePPOLearner
    lrn = DevicePPOLearner(device=0, lr=cfg.lr, clip_range=cfg.clip_range, vf_coef=cfg.vf_coef, ent_coef=cfg.ent_coef,
                           max_grad_norm=cfg.max_grad_norm_pi, separate_clip=not cfg.joint_norm, target_kl=cfg.target_kl or None,
                           normalize_advantage=bool(cfg.normalize_adv), max_workgroups=max_workgroups, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    lrn.params.copy_(torch.from_numpy(np.asarray(params, np.float32)))
    lrn.ret_scale, lrn.actor_on = cfg.ret_scale, bool(cfg.actor_on)
    return lrn


_DEV = {}


def _dev(case):
    """the rollout on the device, uploaded once per case"""
    if id(case) not in _DEV:
        _DEV[id(case)] = [torch.from_numpy(case[k]).cuda() for k in KEYS]
    return _DEV[id(case)]


def _grad(lrn, case, idx):
    g = lrn.grad(*_dev(case), torch.from_numpy(np.ascontiguousarray(idx, np.int32)).cuda())
    return g.cpu().numpy()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("learnerhost"))


# --------------------------------------------------------------------------------------- 1. the gradient
@pytest.mark.parametrize("m,max_wg", [(2, 0), (63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (257, 0), (1000, 0), (1000, 2), (8192, 0)])
def test_gradient_against_fp64_autograd(m, max_wg):
    """the 32-sample N-tile, the 64-sample wave and the 256-sample workgroup edges; 1,000 on two workgroups (two chunks each, the
    last one partial); 8,192 on the default grid"""
    cfg = R.Cfg()
    case, idx = conditioned(m, cfg)
    lrn = _learner(cfg, case["params"], max_wg)
    g = _grad(lrn, case, idx)
    lrn.apply()
    assert lrn.stats().bad_index == 0
    gate(g, R.grad_buffer(case, idx, cfg), f"m={m} max_workgroups={max_wg}")
    lrn.close()


@pytest.mark.parametrize("name,change", [("normalize_adv=0", dict(normalize_adv=0)), ("ent_coef=0.01", dict(ent_coef=0.01)),
                                         ("ret_scale=3", dict(ret_scale=3.0)), ("actor_on=0", dict(actor_on=0, ent_coef=0.01))])
def test_gradient_switches(name, change):
    cfg = R.Cfg(**change)
    case, idx = conditioned(1000, cfg)
    lrn = _learner(cfg, case["params"])
    g = _grad(lrn, case, idx)
    gate(g, R.grad_buffer(case, idx, cfg), name)
    if not cfg.actor_on:
        sl = R.block_slices()
        for block in R.ACTOR_BLOCKS:
            assert g[sl[block]].tobytes() == bytes(4 * (sl[block].stop - sl[block].start)), block
    lrn.close()


def test_gradient_with_all_indices_equal_and_with_the_list_reversed():
    """one row 300 times (the advantage is not normalised there: its std is zero), and the 1,000-row list backwards: another
    assignment of samples to lanes, the same sums"""
    cfg = R.Cfg(normalize_adv=0)
    case, idx = conditioned(1000, cfg)
    lrn = _learner(cfg, case["params"])
    same = next(s for s in (np.full(300, r, np.int32) for r in idx) if R.well_defined(case, s, cfg).size == 0)
    gate(_grad(lrn, case, same), R.grad_buffer(case, same, cfg), "all indices equal")
    lrn.normalize_advantage = True
    cfg = R.Cfg()
    case, idx = conditioned(1000, cfg)
    lrn.params.copy_(torch.from_numpy(case["params"]))
    g64 = R.grad_buffer(case, idx, cfg)
    gate(_grad(lrn, case, idx[::-1]), g64, "reversed")
    lrn.close()


def test_linearity_the_data_parallel_contract():
    cfg = R.Cfg(normalize_adv=0, ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    lrn = _learner(cfg, case["params"])
    a, b = _grad(lrn, case, idx[:500]).astype(np.float64), _grad(lrn, case, idx[500:])
    gate(0.5 * (a + b), R.grad_buffer(case, idx, cfg), "mean of two halves")
    lrn.close()


def test_bad_indices_are_left_out_and_counted():
    cfg = R.Cfg(normalize_adv=0)
    case, idx = conditioned(65, cfg)
    lrn = _learner(cfg, case["params"])
    g = _grad(lrn, case, idx)
    g_bad = _grad(lrn, case, np.concatenate([idx, np.array([-1, N_ROWS, 2 ** 31 - 1], np.int32)]))
    lrn.apply()
    assert lrn.stats().bad_index == 3
    err = R.block_errors(g_bad * (68 / 65), g)
    assert max(err.values()) <= R.GATE, err
    lrn.close()


# --------------------------------------------------------------------------------------- 2. determinism, guard rows
def test_two_runs_return_identical_bytes():
    cfg = R.Cfg(ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    out = []
    for _ in range(2):
        lrn = _learner(cfg, case["params"])
        g = _grad(lrn, case, idx)
        lrn.apply()
        g2 = _grad(lrn, case, idx)   # from the updated parameters
        lrn.apply()
        out.append((g.tobytes(), g2.tobytes(), lrn.params.cpu().numpy().tobytes(), lrn.m.cpu().numpy().tobytes(), lrn.v.cpu().numpy().tobytes()))
        lrn.close()
    assert out[0] == out[1] and out[0][0] != out[0][1]


def test_nothing_is_written_outside_the_outputs():
    cfg = R.Cfg()
    case, idx = conditioned(1000, cfg)
    lrn = _learner(cfg, case["params"])
    pattern = 12345.678
    guarded = {}
    for name, n in (("params", NPARAM), ("m", NPARAM), ("v", NPARAM), ("grad_buf", NPARAM + NSTAT)):
        block = torch.full((3, n), pattern, dtype=torch.float32, device="cuda")
        block[1].copy_(getattr(lrn, name))
        guarded[name] = block
        setattr(lrn, name, block[1])
    rollout = [t.clone() for t in _dev(case)]
    di = torch.from_numpy(idx).cuda()
    for _ in range(2):
        lrn.grad(*rollout, di)
        lrn.apply()
    torch.cuda.synchronize()
    for name, block in guarded.items():
        assert bool((block[0] == pattern).all()) and bool((block[2] == pattern).all()), name
        assert not bool((block[1] == pattern).any()), name
    for t, want in zip(rollout, _dev(case)):
        assert torch.equal(t, want)
    assert torch.equal(di, torch.from_numpy(idx).cuda()) and lrn.stats().steps == 2
    lrn.close()


# --------------------------------------------------------------------------------------- 3. clip + Adam, early stop
@pytest.mark.parametrize("joint", [0, 1])
def test_apply_against_torch_adam_from_given_gradients(joint):
    """tests/test_learner_cpu.py's test of the same name, on the apply kernel: theta starts at zero so that the difference of two
    fp32 thetas is the update; per block, |dtheta - dtheta_torch| <= 1e-6 |dtheta_torch|"""
    cfg = R.Cfg(joint_norm=joint)
    rng = np.random.default_rng(5)
    lrn, t = _learner(cfg, np.zeros(NPARAM, np.float32)), R.TorchLearner(np.zeros(NPARAM, np.float32), cfg)
    worst = 0.0
    for step in range(5):
        g = np.zeros(NPARAM + NSTAT, np.float32)
        g[:NPARAM] = rng.standard_normal(NPARAM) * (0.02 if step % 2 else 0.002)   # norms on both sides of max_grad_norm = 0.5
        before, before_t = lrn.params.cpu().numpy(), t.flat()
        lrn.apply(torch.from_numpy(g).cuda()); t.apply(g)
        d = lrn.params.cpu().numpy().astype(np.float64) - before
        dt = t.flat().astype(np.float64) - before_t
        for name, sl in R.block_slices().items():
            err = np.linalg.norm(d[sl] - dt[sl]) / np.linalg.norm(dt[sl])
            worst = max(worst, err)
            assert err <= 1e-6, (step, name, err)
        s = lrn.stats()
        nall = np.linalg.norm(g[:NPARAM].astype(np.float64))
        nvf = np.linalg.norm(g[R.block_slices()["vf.W1"].start:NPARAM - 2].astype(np.float64))
        np.testing.assert_allclose([s.grad_norm_pi, s.grad_norm_vf], [nall, nall] if joint else [np.sqrt(nall ** 2 - nvf ** 2), nvf], rtol=1e-6)
    print(f"joint_norm={joint}: largest per-block relative error of an Adam update = {worst:.3g}")
    assert lrn.stats().steps == 5
    lrn.close()


@pytest.mark.parametrize("separate", [True, False])
def test_five_full_steps_against_the_fp64_restatement(separate):
    cfg = R.Cfg(joint_norm=int(not separate), ent_coef=0.01)
    case, idx = conditioned(1000, cfg)
    lrn = _learner(cfg, case["params"])
    t64, t32 = R.TorchLearner(case["params"], cfg, torch.float64), R.TorchLearner(case["params"], cfg, torch.float32)
    di = torch.from_numpy(idx).cuda()
    for _ in range(5):
        lrn.step(*_dev(case), di)
        t64.step(case, idx); t32.step(case, idx)
    theta, worst = lrn.params.cpu().numpy(), 0.0
    for name, sl in R.block_slices().items():
        mine, torch32 = np.linalg.norm(theta[sl] - t64.flat()[sl]), np.linalg.norm(t32.flat()[sl] - t64.flat()[sl])
        worst = max(worst, mine / torch32)
        assert mine <= 4 * torch32, (name, mine, torch32)
    print(f"separate_clip={separate}: largest |theta - theta64| / |theta32torch - theta64| over the blocks after five steps = {worst:.3g}")
    lrn.close()


def test_early_stop_is_sticky_until_begin_iteration():
    case, idx = conditioned(1000)
    kl = float(R.grad_buffer(case, idx, R.Cfg())[NPARAM + 3])
    lrn = _learner(R.Cfg(target_kl=10 * kl), case["params"])
    di = torch.from_numpy(idx).cuda()
    lrn.step(*_dev(case), di)
    s = lrn.stats()
    assert s.steps == 1 and not s.stopped
    frozen = [t.clone() for t in (lrn.params, lrn.m, lrn.v)]
    for target in (kl / 3, None, 10 * kl):   # 1.5 x kl / 3 < kl: stops; and stays stopped whatever the later calls ask for
        lrn.target_kl = target
        lrn.step(*_dev(case), di)
        s = lrn.stats()
        assert s.stopped and s.steps == 1
        assert all(torch.equal(a, b) for a, b in zip(frozen, (lrn.params, lrn.m, lrn.v)))
        np.testing.assert_allclose(s.approx_kl, float(lrn.grad_buf[NPARAM + 3]))
    lrn.begin_iteration()
    lrn.step(*_dev(case), di)
    s = lrn.stats()
    assert s.steps == 2 and not s.stopped and not torch.equal(frozen[0], lrn.params)
    lrn.close()


# --------------------------------------------------------------------------------------- 4. kernels against the host build
@pytest.mark.parametrize("m,max_wg", [(257, 0), (1000, 2)])
def test_kernels_against_the_host_build(host, m, max_wg):
    """same source for everything but the towers: 1e-5 per block both for the gradient and, after two steps, for the parameters'
    movement.  Bit equality is not asked of the MFMA part (another tanh, another order of the sums)"""
    cfg = R.Cfg(ent_coef=0.01)
    case, idx = conditioned(m, cfg)
    lrn, h = _learner(cfg, case["params"], max_wg), HostLearner(host, cfg, case["params"], max_wg)
    err = R.block_errors(_grad(lrn, case, idx), h.grad(case, idx))
    print(f"m={m}: largest |g - g_host| / |g_host| per block = {max(err.values()):.3g}")
    assert max(err.values()) <= R.GATE, err
    lrn.apply(); h.apply()
    _grad(lrn, case, idx); h.grad(case, idx)
    lrn.apply(); h.apply()
    err = R.block_errors(lrn.params.cpu().numpy() - case["params"], h.params - case["params"])
    assert max(err.values()) <= R.GATE, err
    a, b = lrn.stats(), h.stats()
    assert (a.steps, a.stopped, a.bad_index) == (b.steps, bool(b.stopped), b.bad_index) == (2, False, 0)
    np.testing.assert_allclose([a.grad_norm_pi, a.grad_norm_vf], [b.grad_norm_pi, b.grad_norm_vf], rtol=1e-5)
    lrn.close(); h.close()


# --------------------------------------------------------------------------------------- 5. the Python layer
def test_rollout_params_carry_the_critics_unit():
    import train_ppo_torch as T
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    torch.manual_seed(3)
    model = T.ActorCritic(-0.5).cuda()
    model.ret_scale.fill_(2.5)
    lrn = _learner(R.Cfg(), np.zeros(NPARAM, np.float32)).load(model.state_dict())
    assert lrn.ret_scale == 2.5
    for naming in ("tool", "sb3"):   # state_dict -> load -> state_dict
        sd = lrn.state_dict(naming)
        again = _learner(R.Cfg(), np.zeros(NPARAM, np.float32)).load(sd)
        sd2 = again.state_dict(naming)
        assert sorted(sd) == sorted(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
        again.close()
    model2 = T.ActorCritic(-0.5).cuda()
    model2.load_state_dict(lrn.state_dict())
    obs = (torch.randn(300, 6, device="cuda") * torch.tensor(R.OBS_SCALE, device="cuda")).contiguous()
    pol = DevicePolicy(device=0)
    pol.use_device_weights(lrn.rollout_params())
    with torch.no_grad():
        want = 2.5 * model2.v(obs).squeeze(-1)
    torch.testing.assert_close(pol.value(obs), want, rtol=1e-5, atol=1e-6)
    assert lrn.rollout_params().data_ptr() == lrn.rollout_params().data_ptr()   # refreshed in place: the policy's pointer stays good
    pol.close(); lrn.close()


# --------------------------------------------------------------------------------------- 6. end to end
def test_stage1_of_the_curriculum_trains_to_balance_with_the_device_learner():
    """tests/test_ppo_device_rollout.py's recipe and assertions; device_learner=True is the only difference"""
    import train_ppo_torch as T
    from balance_robot_mujoco_rl_amd import BatchedSim
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    model = T.ActorCritic(-0.5).to(dev)
    with torch.no_grad():
        sc = torch.tensor([1, 0.02, 1, 1, 1, 1], device=dev)
        model.pi[0].weight.mul_(sc); model.v[0].weight.mul_(sc)
    torch.manual_seed(1000)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    n = 16384
    sim = BatchedSim("Env01-v2", n, device=0, seed=0, auto_reset=True)
    log = []
    t0 = time.time()
    T.train(sim, model, opt, iters=80, n_steps=64, epochs=4, minibatch=8192, gamma=0.999, lam=0.95, clip=0.2, log=log, tag="Env01-v2",
            reward_clip=1.0, device_rollout=True, seed=1000, device_learner=True)
    sim.close()
    wall = time.time() - t0
    before = T.evaluate("Env01-v2", T.ActorCritic(-0.5).to(dev), 2048, 300)
    after = T.evaluate("Env01-v2", model, 2048, 600)
    print(f"stage 1 with the device learner: {wall:.1f} s, {log[-1]['env_steps']} env-steps, {log[-1]['env_steps'] / wall / 1e6:.2f} M env-steps/s; "
          f"untrained: {before['first_episode_still_running']} of 2048 still up after 300 steps; trained: "
          f"{after['first_episode_still_running']} of 2048 still up after 600 steps, {after['fell']} falls")
    assert before["first_episode_still_running"] < 0.05 * 2048
    assert after["first_episode_still_running"] > 0.2 * 2048, after
    assert wall < 150, wall
