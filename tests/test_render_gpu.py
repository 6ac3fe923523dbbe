"""HIP render kernel on the MI355X: against the numpy reference, determinism and batch invariance,
no effect on the simulation, the VecEnv path, and argument checks at the C ABI."""
import ctypes as C

import numpy as np
import pytest
import torch

from balance_robot_mujoco_rl_amd import BalanceVecEnv, BatchedSim, _lib
from tests import ref_render as R
from tests.test_render_cpu import assert_matches_reference

pytestmark = pytest.mark.gpu

POSES = R.constructed_poses()
NAMES = sorted(POSES)


def _posed(env_id):
    sim = BatchedSim(env_id, len(NAMES), device=0, seed=0, auto_reset=False)
    q = np.stack([POSES[k] for k in NAMES])
    sim.set_state(qpos=q if sim.nq == 16 else q[:, :9])
    return sim, sim.get_state()[0]


def _np(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("env_id", ["Env01-v2", "Env03-v2"])
@pytest.mark.parametrize("size", [(84, 84), (97, 61)])
def test_kernel_matches_reference_constructed(env_id, size):
    sim, qpos = _posed(env_id)
    cam = dict(width=size[0], height=size[1])
    rgb, dep, seg = _np(*sim.render(camera=cam, depth=True, segmentation=True))
    assert rgb.shape == (len(NAMES), size[1], size[0], 3) and dep.dtype == np.float32 and seg.dtype == np.uint8
    block = sim.nq == 16
    for i, name in enumerate(NAMES):
        assert_matches_reference(rgb[i], dep[i], seg[i], R.render(qpos[i], block, cam), f"{env_id} {name} {size}")
    if not block:
        assert seg.max() <= R.SEG_WHEEL_R
    sim.close()


@pytest.mark.parametrize("name", ["block_wheel", "far60m"])
def test_kernel_matches_reference_800(name):
    sim, qpos = _posed("Env03-v2")
    i = NAMES.index(name)
    rgb, dep, seg = _np(*sim.render(env_ids=[i], depth=True, segmentation=True))
    assert rgb.shape == (1, 800, 800, 3)
    assert_matches_reference(rgb[0], dep[0], seg[0], R.render(qpos[i], True), f"{name} 800x800")
    sim.close()


def test_kernel_matches_reference_after_random_steps():
    n = 256
    sim = BatchedSim("Env03-v2", n, device=0, seed=5)
    sim.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(100):
        sim.step(torch.rand((n, 2), device="cuda", generator=g) * 2 - 1)
    torch.cuda.synchronize()
    qpos = sim.get_state()[0]
    cam = dict(width=84, height=84)
    rgb, dep, seg = _np(*sim.render(camera=cam, depth=True, segmentation=True))
    for i in range(n):
        assert_matches_reference(rgb[i], dep[i], seg[i], R.render(qpos[i], True, cam), f"env {i}")
    assert (seg == R.SEG_BLOCK).any(axis=(1, 2)).sum() > 0
    sim.close()


def test_deterministic_and_batch_invariant():
    n = 4096
    sim = BatchedSim("Env03-v2", n, device=0, seed=9)
    sim.reset()
    g = torch.Generator(device="cuda").manual_seed(1)
    for _ in range(20):
        sim.step(torch.rand((n, 2), device="cuda", generator=g) * 2 - 1)
    cam = dict(width=84, height=84)
    full = _np(*sim.render(camera=cam, depth=True, segmentation=True))
    again = _np(*sim.render(camera=cam, depth=True, segmentation=True))
    rev = _np(*sim.render(env_ids=np.arange(n)[::-1].copy(), camera=cam, depth=True, segmentation=True))
    for a, b, c in zip(full, again, rev):
        assert np.array_equal(a, b) and np.array_equal(a, c[::-1])
    for i in (0, 1234, n - 1):
        alone = _np(*sim.render(env_ids=[i], camera=cam, depth=True, segmentation=True))
        for a, b in zip(alone, full):
            assert np.array_equal(a[0], b[i])
    sim.close()


def test_rendering_does_not_change_the_simulation():
    n = 512
    a = BatchedSim("Env03-v2", n, device=0, seed=13)
    b = BatchedSim("Env03-v2", n, device=0, seed=13)
    a.reset(); b.reset()
    g = torch.Generator(device="cuda").manual_seed(2)
    for _ in range(50):
        act = torch.rand((n, 2), device="cuda", generator=g) * 2 - 1
        oa, ra = (t.clone() for t in a.step(act)[:2])
        ob, rb = (t.clone() for t in b.step(act)[:2])
        b.render(env_ids=[0, 7, n - 1], camera=dict(width=64, height=48), depth=True, segmentation=True)
        assert torch.equal(oa, ob) and torch.equal(ra, rb)
    torch.cuda.synchronize()
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    a.close(); b.close()


def test_vecenv_render_matches_batched_sim():
    n = 8
    env = BalanceVecEnv("Env03-v2", n, devices=[0, 0], seed=4, render_mode="rgb_array", render_envs=(0,))
    assert env.get_attr("render_mode") == ["rgb_array"] * n
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(10):
        env.step_async(rng.uniform(-1, 1, size=(n, 2)))
        with pytest.raises(RuntimeError):
            env.render()
        env.step_wait()
    frame = env.render()
    qpos = np.concatenate([s.get_state()[0] for s in env._sims])
    ref = BatchedSim("Env03-v2", n, device=0, auto_reset=False)
    ref.set_state(qpos=qpos)
    expect = _np(ref.render(env_ids=[0, 6]))[0]
    assert frame.shape == (800, 800, 3) and np.array_equal(frame, expect[0])
    env.render_envs = [6]  # owned by the second shard (its own handle and stream)
    assert np.array_equal(env.render(), expect[1])
    imgs = env.get_images()
    assert [i for i, f in enumerate(imgs) if f is not None] == [6]
    env.close(); ref.close()


def test_bad_arguments_return_arg_error():
    L = _lib.lib()
    q = torch.zeros((4, 16), dtype=torch.float64, device="cuda")
    q[:, 3] = q[:, 12] = 1  # upright robots at the origin, block at the origin
    rgb = torch.zeros((4, 8, 8, 3), dtype=torch.uint8, device="cuda")
    cam = _lib.BrsCamera(8, 8, 45.0, 1.25, 45.0, -25.0)
    qp, rp = C.c_void_p(q.data_ptr()), C.c_void_p(rgb.data_ptr())
    assert L.brs_render(0, 3, 4, qp, C.byref(cam), rp, None, None, None) == 0
    torch.cuda.synchronize()
    assert L.brs_render(0, 3, 0, qp, C.byref(cam), rp, None, None, None) == -1
    for w in (0, 5000):
        bad = _lib.BrsCamera(w, 8, 45.0, 1.25, 45.0, -25.0)
        assert L.brs_render(0, 3, 1, qp, C.byref(bad), rp, None, None, None) == -1
    assert L.brs_render(0, 3, 1, qp, C.byref(cam), None, None, None, None) == -1
    assert L.brs_render(0, 9, 1, qp, C.byref(cam), rp, None, None, None) == -1
    assert L.brs_render(0, 3, 1, None, C.byref(cam), rp, None, None, None) == -1
    assert L.brs_render_last_error()
    sim = BatchedSim("Env01-v2", 4, device=0)
    with pytest.raises(IndexError):
        sim.render(env_ids=[4])
    with pytest.raises(ValueError):
        sim.render(camera=dict(width=5000))
    sim.close()
    torch.cuda.synchronize()
