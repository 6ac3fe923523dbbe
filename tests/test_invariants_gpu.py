"""The HIP kernels against the conservation laws and symmetries of tests/invariant_cases.py: what
tests/test_invariants_cpu.py asks of the oracle and the host builds, asked of the device code -- its code generation, the LDS
contact store, fast-math contraction of the fp64 decision code, the lane map.

  physics kernels   Env03-v2 and Env03-v1 (constants folded) and a runtime-constant handle (100 substeps of 5e-5 s), each at 64
                    threads and at the default workgroup size; the 56 cases tiled cyclically to 200 envs (three waves and a
                    partial one): momentum through the collision; mirror, half turn and translation teacher-forced per chunk
  step kernel       one brs_step launch holds the flight cases and their mirror images, 10 env steps teacher-forced, with
                    lane grouping and without: mirror and momentum

Every gate prints the largest value next to it (profiles/invariants_gpu_tests.log)."""
import numpy as np
import pytest

from tests import invariant_cases as ic, parity as P

pytestmark = pytest.mark.gpu

N = 200
RUNTIME = dict(substeps=100, timestep=5e-5)   # the kernels whose model constants are arguments; 100 x 5e-5 s = the same 5 ms chunk
HANDLES = {"Env03-v2": ("Env03-v2", {}), "Env03-v1": ("Env03-v1", {}), "runtime": ("Env03-v2", RUNTIME)}
_cache = {}


def _teacher(handle, scene):
    """the oracle's free run over the cases, once per (handle, scene), tiled to N and left unchanged"""
    if (handle, scene) not in _cache:
        env, kw = HANDLES[handle]
        _cache[handle, scene] = ic.teacher_states(scene, N, nsub=kw.get("substeps", ic.NSUB), env=env, **kw)
    return _cache[handle, scene]


def _meter(n, env):
    if ("meter", n, env) not in _cache:
        _cache["meter", n, env] = ic.Meter(n, env)
    return _cache["meter", n, env]


def _hip(handle, bt, n=N, **more):
    env, kw = HANDLES[handle]
    sim = P.make("hip", env, n, noise=False, auto_reset=False, block_threads=bt, **kw, **more)
    assert ("-1>" in sim.raw.step_kernel_name()) == bool(kw), sim.raw.step_kernel_name()
    return sim


@pytest.mark.parametrize("bt", [64, 0])
@pytest.mark.parametrize("handle", list(HANDLES))
def test_momentum_through_the_collision(handle, bt):
    """flight, free-running 10 chunks through brs_physics: P changes by gravity only, L about the centre of mass not at all"""
    env, kw = HANDLES[handle]
    nsub = kw.get("substeps", ic.NSUB)
    q, v, ctrl = ic.tile(ic.cases("flight"), N)
    sim = _hip(handle, bt)
    states = ic.run_free(sim, q, v, ctrl, nsub=nsub)
    sim.close()
    assert all(np.isfinite(s).all() for st in states for s in st)
    ic.check_conservation(f"momentum, flight, HIP {handle} at {bt or 'default'} threads", *ic.conservation(_meter(N, env), states))


@pytest.mark.parametrize("bt", [64, 0])
@pytest.mark.parametrize("handle", list(HANDLES))
@pytest.mark.parametrize("name", list(ic.MAPS))
def test_symmetry_teacher_forced(name, handle, bt):
    """per chunk: copy A from the oracle's state, copy B from its image; A against the image of B brought back, within the
    strict bound and 8x the larger distance to the oracle -- both scenes"""
    kw = HANDLES[handle][1]
    for scene in ("flight", "floor"):
        ctrl, states = _teacher(handle, scene)
        a, b = _hip(handle, bt), _hip(handle, bt)
        d = ic.forced_symmetry(a, b, ic.MAPS[name], ctrl, states, nsub=kw.get("substeps", ic.NSUB))
        a.close(); b.close()
        ic.check_forced(f"{name}, {scene}, HIP {handle} at {bt or 'default'} threads, teacher-forced", d)


@pytest.mark.parametrize("lane_grouping", [True, False])
def test_step_kernel_mirror_and_momentum(lane_grouping):
    """brs_step (another kernel, indexed through the lane map): the flight cases in the first half of one launch, their
    mirror images in the second, actions U(-1, 1)^2 and (-a1, -a0); 10 env steps, each from the oracle's state.  No block
    timer may start: a removed block goes to (10, 10, 0), which is not mirror-symmetric"""
    half, steps, T = 2 * ic.DRAWS * len(ic.AIMS), ic.CHUNKS, ic.MIRROR
    q, v, _ = ic.tile(ic.cases("flight"), half)
    orc = P.make("oracle", ic.ENV, half, noise=False, auto_reset=False)
    sim = P.make("hip", ic.ENV, 2 * half, noise=False, auto_reset=False, lane_grouping=lane_grouping)
    kernel = sim.raw.step_kernel_name()
    orc.reset(); sim.reset()
    orc.set_state(q, v, np.zeros_like(v), np.zeros(half))
    meter, rng = _meter(half, ic.ENV), np.random.default_rng(11)
    two = lambda x, y: np.concatenate([x, y])
    d = dict(pair=0.0, a=0.0, b=0.0, pair_v=0.0, a_v=0.0, b_v=0.0)
    z, dt = np.array([0.0, 0.0, 1.0]), ic.NSUB * ic.DT
    lin_sum = {k: np.zeros((half, 3)) for k in "ab"}; ang_sum = {k: np.zeros((half, 3)) for k in "ab"}
    lin = {k: np.zeros(half) for k in "ab"}; ang = {k: np.zeros(half) for k in "ab"}
    teacher = [orc.get_state()[:2]]
    for k in range(steps):
        q0, v0, w0, t0 = orc.get_state()
        aux, (xq, xp) = orc.get_aux(), orc.get_xpose()
        sim.set_state(two(q0, T.pos(q0)), two(v0, T.vel(v0)), two(w0, T.vel(w0)), two(t0, t0))
        sim.set_aux(two(aux, aux))
        sim.set_xpose(two(xq, xq * (1, 1, -1, -1)), two(xp, xp * (-1, 1, 1)))
        act = rng.uniform(-1, 1, size=(half, 2)).astype(np.float32)
        orc.step(act)
        sim.step(two(act, np.stack([-act[:, 1], -act[:, 0]], axis=1)))
        q1, v1, _, _ = orc.get_state()
        qs, vs, _, _ = sim.get_state()
        assert np.isfinite(qs).all() and np.isfinite(vs).all()
        assert np.isnan(sim.get_aux()[:, 1]).all() and np.isnan(orc.get_aux()[:, 1]).all(), f"step {k}: a block timer started"
        qa, va, qb, vb = qs[:half], vs[:half], T.inv.pos(qs[half:]), T.inv.vel(vs[half:])
        for key, (x, y) in dict(pair=ic.state_distance(qa, va, qb, vb), a=ic.state_distance(q1, v1, qa, va),
                                b=ic.state_distance(q1, v1, qb, vb)).items():
            d[key] = max(d[key], float(x.max())); d[key + "_v"] = max(d[key + "_v"], float(y.max()))
        # momentum over the same steps: the per-step changes from the forced state, accumulated as a free run accumulates them
        P0, L0, _, (m_r, m_k) = meter.momenta(q0, v0)
        for key, (qq, vv) in dict(a=(qa, va), b=(qb, vb)).items():
            P1, L1, _, _ = meter.momenta(qq, vv)
            lin_sum[key] += P1 - P0 + (m_r + m_k) * ic.G * dt * z; ang_sum[key] += L1 - L0
            lin[key] = np.maximum(lin[key], np.linalg.norm(lin_sum[key], axis=1))
            ang[key] = np.maximum(ang[key], np.linalg.norm(ang_sum[key], axis=1))
        teacher.append((q1, v1))
    sim.close(); orc.close()
    label = f"brs_step ({kernel}, lane grouping {'on' if lane_grouping else 'off'})"
    ic.check_forced(f"mirror, flight, {label}, teacher-forced", d)
    _, _, J = ic.conservation(meter, teacher)
    for key, what in (("a", "cases"), ("b", "mirror images")):
        ic.check_conservation(f"momentum, flight, {label}, {what}", lin[key], ang[key], J)
