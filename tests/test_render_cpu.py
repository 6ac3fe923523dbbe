"""Renderer without a GPU: the camera conventions pinned analytically, geometry facts, the kernel's own
source (brs_render.hpp, compiled for the host by g++) against the independent numpy reference, and BalanceVecEnv's
rendering logic on stand-in simulators."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from balance_robot_mujoco_rl_amd.vec_env import BalanceVecEnv, BalanceVectorEnv, shard_ranges, tile_images
from tests import ref_render as R
from tests.fake_render_backend import OracleRenderSim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEG = np.pi / 180


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """tests/renderhost/renderhost.cpp (brs_render.hpp on the host) built into a temporary directory"""
    so = str(tmp_path_factory.mktemp("renderhost") / "librenderhost.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-ffp-contract=off",
                           "-I", os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc"), "-o", so,
                           os.path.join(ROOT, "tests", "renderhost", "renderhost.cpp")])
    L = C.CDLL(so)
    vp, f = C.c_void_p, C.c_float
    L.rh_render.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, f, f, f, f, vp, vp, vp, vp, vp]
    L.rh_pixel_ray.argtypes = [C.c_int, C.c_int, f, f, f, f, f, f, vp, vp]
    return L


def host_render(L, qpos, block, camera=None):
    """-> rgb [k,H,W,3] u8, depth [k,H,W] f32, seg [k,H,W] u8 of the kernel source for k qpos rows"""
    c = R.cam_of(camera)
    W, H = c["width"], c["height"]
    q = np.ascontiguousarray(np.atleast_2d(qpos), dtype=np.float64)
    k = q.shape[0]
    rgb, dep, seg = np.zeros((k, H, W, 3), np.uint8), np.zeros((k, H, W), np.float32), np.zeros((k, H, W), np.uint8)
    sh, ch = np.zeros((k, H, W), np.uint8), np.zeros((k, H, W), np.int8)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    L.rh_render(int(block), k, P(q), q.shape[1], W, H, c["fovy"], c["distance"], c["azimuth"], c["elevation"],
                P(rgb), P(dep), P(seg), P(sh), P(ch))
    return rgb, dep, seg


def ambiguous_cap(height):
    """largest admitted share of ambiguous pixels: 0.5 % at 800 rows.  Far from the robot the floor's 0.1-m cells are
    smaller than a pixel, and the share of pixels within 0.01 px of a cell edge grows as 1 / resolution"""
    return 0.005 * max(1.0, 800.0 / height)


def assert_matches_reference(rgb, dep, seg, ref, what):
    """the pass criteria of kernel vs numpy reference"""
    r_rgb, r_dep, r_seg, amb = ref
    ok = ~amb
    assert amb.mean() <= ambiguous_cap(seg.shape[0]), f"{what}: {amb.mean():.2%} of the pixels are ambiguous"
    bad = (seg != r_seg) & ok
    assert not bad.any(), f"{what}: seg differs on {bad.sum()} non-ambiguous pixels, first at {np.argwhere(bad)[0]}"
    agree = (seg == r_seg) & np.isfinite(r_dep)
    assert np.array_equal(np.isinf(dep), np.isinf(r_dep)) or (np.isinf(dep) != np.isinf(r_dep))[ok].sum() == 0
    rel = np.abs(dep[agree].astype(np.float64) - r_dep[agree]) / r_dep[agree]
    assert rel.max(initial=0) <= 1e-4, f"{what}: depth rel. difference {rel.max():.3g}"
    drgb = np.abs(rgb.astype(int) - r_rgb.astype(int)).max(-1)[ok]
    assert drgb.max(initial=0) <= 2, f"{what}: rgb differs by {drgb.max()} levels"


# ---------------------------------------------------------------------------------------------------- camera conventions
def _ray_through(L, cam, px, py):
    o, d = np.zeros(3, np.float32), np.zeros(3, np.float32)
    L.rh_pixel_ray(cam["width"], cam["height"], cam["fovy"], cam["distance"], cam["azimuth"], cam["elevation"], px, py,
                   o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
    return o.astype(np.float64), d.astype(np.float64)


def _miss_distance(o, d, p):
    v = p - o
    return np.linalg.norm(v - (v @ d) / (d @ d) * d)


def test_camera_conventions_pinned(host):
    cam = R.cam_of(dict(width=161, height=121))
    W, H, dist = cam["width"], cam["height"], cam["distance"]
    a, e = cam["azimuth"] * DEG, cam["elevation"] * DEG
    th = np.tan(cam["fovy"] * DEG / 2)
    # the robot body origin (= lookat) projects to the image centre, in the reference and through the kernel's ray
    assert np.allclose(R.project(np.zeros(3), cam), (W / 2, H / 2))
    o, d = _ray_through(host, cam, W / 2, H / 2)
    assert _miss_distance(o, d, np.zeros(3)) < 1e-6
    # lookat + 0.1 * right: centre row, right of centre, at the pinhole column (0.1 m at depth `dist`)
    p = 0.1 * np.array([np.sin(a), -np.cos(a), 0])
    col_pinhole = W / 2 + 0.1 / (dist * th * W / H) * W / 2
    col, row = R.project(p, cam)
    assert abs(row - H / 2) < 1e-9 and col > W / 2 and abs(col - col_pinhole) <= 0.5
    o, d = _ray_through(host, cam, col_pinhole, H / 2)
    assert _miss_distance(o, d, p) < 0.5 * 2 * dist * th / H  # within half a pixel at that depth
    # lookat + 0.1 z: above the centre (row 0 is the top of the image)
    col, row = R.project(np.array([0, 0, 0.1]), cam)
    assert row < H / 2 and abs(col - W / 2) < 1e-9
    o, d = _ray_through(host, cam, W / 2, H / 2 - 0.1 * np.cos(e) / (dist * th) * H / 2)
    assert d[2] > np.sin(e)


def test_floor_depth_at_centre_closed_form(host):
    """a robot at rest: the centre ray passes between the wheels, under the torso, and hits the floor at
    depth = distance + (floor_z - lookat_z) / sin(elevation)"""
    cam = dict(width=81, height=81)
    q = R.constructed_poses()["upright"].copy()
    q[2] += 0.003  # body origin 3 mm above the floor
    e = R.DEFAULT_CAMERA["elevation"] * DEG
    expect = R.DEFAULT_CAMERA["distance"] + (R.FLOOR_Z - q[2]) / np.sin(e)
    for rgb, dep, seg in ((r[0], r[1], r[2]) for r in (R.render(q[:9], False, cam), [a[0] for a in host_render(host, q[:9], False, cam)])):
        assert seg[40, 40] == R.SEG_FLOOR
        assert abs(dep[40, 40] - expect) < 1e-5 * expect


# ---------------------------------------------------------------------------------------------------- geometry facts
def test_wheels_below_torso(host):
    cam = dict(width=200, height=200)
    for seg in (R.render(R.constructed_poses()["upright"][:9], False, cam)[2],
                host_render(host, R.constructed_poses()["upright"][:9], False, cam)[2][0]):
        rows = lambda s: np.argwhere(seg == s)[:, 0]
        assert rows(R.SEG_TORSO).size and rows(R.SEG_WHEEL_L).size and rows(R.SEG_WHEEL_R).size
        for w in (R.SEG_WHEEL_L, R.SEG_WHEEL_R):
            assert rows(w).mean() > rows(R.SEG_TORSO).mean() + 5


def test_yaw_180_mirror_consistent(host):
    """the robot is symmetric under a half turn about z, with the wheels exchanged"""
    cam = dict(width=160, height=160)
    q0 = R.constructed_poses()["upright"][:9].copy()
    q1 = q0.copy()
    q1[3:7] = [0, 0, 0, 1]
    s0, s1 = host_render(host, q0, False, cam)[2][0], host_render(host, q1, False, cam)[2][0]
    swap = s0.copy()
    swap[s0 == R.SEG_WHEEL_L], swap[s0 == R.SEG_WHEEL_R] = R.SEG_WHEEL_R, R.SEG_WHEEL_L
    amb = R.render(q0, False, cam)[3] | R.render(q1, False, cam)[3]
    assert ((swap != s1) & ~amb).sum() == 0 and (s1 == R.SEG_WHEEL_L).sum() > 20


def test_block_in_front_of_wheel_occludes(host):
    """a block 1 cm in front of the left wheel (toward the camera) hides it exactly where the ray test says so"""
    cam = dict(width=240, height=240)
    q = R.constructed_poses()["upright"].copy()
    wl = R.WHEEL_POS[0] + q[0:3]
    fwd = R.camera_frame(cam)[0]
    towards = -np.array([fwd[0], fwd[1], 0]) / np.hypot(fwd[0], fwd[1])
    q[9:12] = wl + towards * (R.WHEEL_R + 0.01 + R.BLOCK_HALF)
    q[12:16] = [1, 0, 0, 0]
    W, H = cam["width"], cam["height"]
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    t = R.cast(q, True, jj.ravel(), ii.ravel(), R.cam_of(cam))["t"]
    both = np.isfinite(t[R.SEG_BLOCK]) & np.isfinite(t[R.SEG_WHEEL_L])
    hides = (both & (t[R.SEG_BLOCK] < t[R.SEG_WHEEL_L])).reshape(H, W)
    assert hides.sum() > 50, "the block must cover part of the wheel"
    ref = R.render(q, True, cam)
    seg = host_render(host, q, True, cam)[2][0]
    m = hides & ~ref[3]
    assert (seg[m] == R.SEG_BLOCK).all() and (ref[2][m] == R.SEG_BLOCK).all()
    assert ((seg == R.SEG_WHEEL_L) & hides).sum() == 0


def test_env01_never_renders_a_block(host):
    cam = dict(width=96, height=96)
    for name, q in R.constructed_poses().items():
        assert host_render(host, q[:9], False, cam)[2].max() <= R.SEG_WHEEL_R, name


# ---------------------------------------------------------------------------------------------------- kernel source vs reference
@pytest.mark.parametrize("name", sorted(R.constructed_poses()))
def test_kernel_source_matches_reference_constructed(host, name):
    q = R.constructed_poses()[name]
    for block, cam in ((True, dict(width=240, height=240)), (False, dict(width=97, height=61))):
        qq = q if block else q[:9]
        rgb, dep, seg = (a[0] for a in host_render(host, qq, block, cam))
        assert_matches_reference(rgb, dep, seg, R.render(qq, block, cam), f"{name} block={block}")


def test_kernel_source_matches_reference_full_size(host):
    q = R.constructed_poses()["block_wheel"]
    rgb, dep, seg = (a[0] for a in host_render(host, q, True))
    assert_matches_reference(rgb, dep, seg, R.render(q, True), "block_wheel 800x800")


@pytest.mark.parametrize("env_id", ["Env01-v2", "Env03-v2"])
def test_kernel_source_matches_reference_oracle_poses(host, env_id):
    from oracle import oracle as O
    n = 6
    o = O.Oracle(env_id, n, seed=11, auto_reset=True)
    o.reset()
    rng = np.random.default_rng(2)
    for _ in range(50):
        o.step(rng.uniform(-1, 1, size=(n, 2)).astype(np.float32))
    qpos = o.get_state()[0]
    o.close()
    block = env_id.startswith("Env03")
    cam = dict(width=120, height=120)
    rgb, dep, seg = host_render(host, qpos, block, cam)
    for i in range(n):
        assert_matches_reference(rgb[i], dep[i], seg[i], R.render(qpos[i], block, cam), f"{env_id} env {i}")


# ---------------------------------------------------------------------------------------------------- BalanceVecEnv logic
CAM = dict(width=24, height=16)


def _env(n, shards, render_mode="rgb_array", render_envs=(0,)):
    sims = [OracleRenderSim("Env03-v2", cnt, camera=CAM, seed=3, env_index_base=start, max_episode_steps=20)
            for start, cnt in shard_ranges(n, shards)]
    return BalanceVecEnv("Env03-v2", n, render_mode=render_mode, render_envs=render_envs, _sims=sims), sims


def test_tile_images_layout():
    imgs = np.arange(5 * 2 * 3 * 1).reshape(5, 2, 3, 1)
    t = tile_images(imgs)
    assert t.shape == (3 * 2, 2 * 3, 1)  # 3 rows x 2 columns, filled row by row, the last cell black
    assert (t[0:2, 0:3] == imgs[0]).all() and (t[0:2, 3:6] == imgs[1]).all() and (t[2:4, 0:3] == imgs[2]).all()
    assert (t[4:6, 0:3] == imgs[4]).all() and (t[4:6, 3:6] == 0).all()
    assert tile_images(imgs[:1]).shape == (2, 3, 1)


def test_vecenv_render_routes_over_shards():
    n = 7
    env, sims = _env(n, 2, render_envs=(5, 1, 4))  # shards [0, 4) and [4, 7)
    assert BalanceVecEnv.metadata["render_modes"] == ["rgb_array"]
    assert env.get_attr("render_mode") == ["rgb_array"] * n
    env.reset()
    rng = np.random.default_rng(0)
    for _ in range(3):
        env.step(rng.uniform(-1, 1, size=(n, 2)))
    frame = env.render()
    qpos = np.concatenate([s.o.get_state()[0] for s in sims])
    expect = [R.render(qpos[i], True, CAM)[0] for i in (5, 1, 4)]
    assert frame.shape == (2 * 16, 2 * 24, 3) and frame.dtype == np.uint8
    assert np.array_equal(frame, tile_images(np.stack(expect)))
    assert sims[0].rendered[-1] == [1] and sims[1].rendered[-1] == [1, 0]  # local indices on the owning shard
    imgs = env.get_images()
    assert len(imgs) == n and [i for i, f in enumerate(imgs) if f is not None] == [1, 4, 5]
    for i in (1, 4, 5):
        assert np.array_equal(imgs[i], expect[(5, 1, 4).index(i)])
    env.close()


def test_vecenv_default_renders_env0():
    env, _ = _env(3, 1)
    env.reset()
    frame = env.render()
    assert frame.shape == (16, 24, 3)
    assert np.array_equal(frame, env.get_images()[0])
    env.close()


def test_vecenv_render_mode_none_unchanged():
    env, sims = _env(4, 2, render_mode=None)
    env.reset()
    assert env.render() is None and env.get_images() == [None] * 4 and env.get_attr("render_mode") == [None] * 4
    assert all(s.rendered == [] for s in sims)
    env.close()


def test_vecenv_render_while_step_in_flight_raises():
    env, _ = _env(3, 1)
    env.reset()
    env.step_async(np.zeros((3, 2)))
    with pytest.raises(RuntimeError):
        env.render()
    with pytest.raises(RuntimeError):
        env.get_images()
    env.step_wait()
    assert env.render().shape == (16, 24, 3)
    env.close()


def test_vecenv_bad_render_arguments():
    for kw in (dict(render_mode="human"), dict(render_envs=(3,)), dict(render_envs=()), dict(render_envs=(0.5,))):
        with pytest.raises(ValueError):
            _env(3, 1, **{"render_mode": "rgb_array", **kw})


def test_vector_env_render_tuple():
    n = 4
    sims = [OracleRenderSim("Env03-v2", cnt, camera=CAM, seed=1, env_index_base=start) for start, cnt in shard_ranges(n, 2)]
    env = BalanceVectorEnv("Env03-v2", n, render_mode="rgb_array", render_envs=(3, 0), _sims=sims)
    env.reset()
    env.step(np.zeros((n, 2)))
    frames = env.render()
    qpos = np.concatenate([s.o.get_state()[0] for s in sims])
    assert isinstance(frames, tuple) and len(frames) == 2
    assert np.array_equal(frames[0], R.render(qpos[3], True, CAM)[0]) and np.array_equal(frames[1], R.render(qpos[0], True, CAM)[0])
    env.close()


def test_render_header_symbols_exported():
    import re
    from balance_robot_mujoco_rl_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "brs_render.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(brs_[a-z_0-9]+)\s*\(", txt))) == sorted(_lib.RENDER_SYMBOLS)
    _lib.build()
    L = _lib.lib()
    assert all(hasattr(L, s) for s in _lib.RENDER_SYMBOLS)
    cam = _lib.BrsCamera()
    L.brs_render_default_camera(C.byref(cam))
    assert (cam.width, cam.height, cam.fovy_deg, cam.distance, cam.azimuth_deg, cam.elevation_deg) == (800, 800, 45, 1.25, 45, -25)


def test_render_argument_checks_without_device():
    """the checks that need no device, through the C ABI and the Python front end's validators"""
    from balance_robot_mujoco_rl_amd import _lib
    from balance_robot_mujoco_rl_amd.sim import _env_ids, make_camera
    L = _lib.lib()
    cam = _lib.BrsCamera(); L.brs_render_default_camera(C.byref(cam))
    buf = C.c_void_p(1)
    assert L.brs_render(0, 9, 1, buf, C.byref(cam), buf, None, None, None) == -1 and b"variant" in L.brs_render_last_error()
    assert L.brs_render(0, 3, 0, buf, C.byref(cam), buf, None, None, None) == -1
    assert L.brs_render(0, 3, 1, buf, C.byref(cam), None, None, None, None) == -1 and b"rgb" in L.brs_render_last_error()
    for w in (0, 5000):
        bad = _lib.BrsCamera(w, 64, 45.0, 1.25, 45.0, -25.0)
        assert L.brs_render(0, 3, 1, buf, C.byref(bad), buf, None, None, None) == -1
    for key, val in (("width", 0), ("height", 4097), ("fovy", 180), ("distance", 0), ("azimuth", float("nan")), ("zoom", 1),
                     ("width", 12.5)):
        with pytest.raises(ValueError):
            make_camera({key: val})
    assert make_camera(dict(width=97, height=61)).width == 97
    for ids in ([], [0.5], [[0, 1]], [True]):
        with pytest.raises(ValueError):
            _env_ids(ids, 4)
    with pytest.raises(IndexError):
        _env_ids([0, 4], 4)
    with pytest.raises(IndexError):
        _env_ids([-1], 4)
    assert _env_ids(np.array([3, 1], np.int32), 4).tolist() == [3, 1]
