"""Constructed contact states shared by tests/test_hostsim_parity.py (kernel source on the host), tests/test_gpu_parity.py (the HIP
path) and tests/test_launch_geometry_gpu.py: states a random rollout reaches only by chance -- the block against every torso face
and both wheels (5- and 6-point patches, edge-edge poses, the wheel barrel) and the robot pressed into the floor in every
orientation.  Geometry re-typed from the reference's XML (envs/robot-02.xml:4-20, envs/env03_v1.xml:31-37).  SCENARIOS holds what
a run of them needs; run_scenario runs one on any back end of tests/parity.py.  Test infrastructure."""
import numpy as np

from tests import parity as P

TC, TS, BS = np.array([0.0, 0.0, 0.0995]), np.array([0.05, 0.0185, 0.0855]), 0.02
WP = {1: np.array([-0.074, 0.0, 0.034]), 2: np.array([0.074, 0.0, 0.034])}


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def block_robot_states(n=96, seed=17):
    """Env03: airborne robot (no floor contacts), block placed with a random pose and approach velocity against the torso
    faces (every third env) or around a wheel's barrel -> (qpos [n,16], qvel [n,14])"""
    rng = np.random.default_rng(seed)
    qpos = np.zeros((n, 16)); qvel = np.zeros((n, 14))
    qpos[:, 3] = 1.0; qpos[:, 2] = 1.0
    for i in range(n):
        if i % 3 == 0:
            face = rng.integers(3); sign = rng.choice([-1.0, 1.0])
            c = TC + rng.uniform(-1, 1, 3) * TS
            c[face] = TC[face] + sign * (TS[face] + BS * rng.uniform(0.7, 1.3))
        else:
            th = rng.uniform(0, 2 * np.pi); rad = 0.034 + BS * rng.uniform(0.7, 1.3)
            c = WP[1 + i % 2] + np.array([rng.uniform(-1, 1) * 0.013, rad * np.cos(th), rad * np.sin(th)])
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        qpos[i, 9:12] = c + np.array([0, 0, 1.0]); qpos[i, 12:16] = q
        qvel[i, 8:11] = rng.normal(size=3) * 2.0
        qvel[i, 11:14] = rng.normal(size=3) * 5.0
        qvel[i, 6:8] = rng.normal(size=2) * 10.0
    return qpos, qvel


def edge_edge_states(n=64, seed=29):
    """Env03: block rotated 45 degrees about two of its axes and pushed edge-first against a vertical edge of the torso box,
    0.5 mm outside ... 1.5 mm inside the 2 mm margin: the edge-pair axis of the SAT wins and the patch is ONE point whose
    existence is the `separation < margin` decision -> (qpos, qvel)"""
    rng = np.random.default_rng(seed)
    qpos = np.zeros((n, 16)); qvel = np.zeros((n, 14))
    qpos[:, 3] = 1.0; qpos[:, 2] = 1.0
    for i in range(n):
        sx, sy = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
        # torso edge along z at (sx TS[0], sy TS[1]); approach direction = outward diagonal in the x-y plane
        out = np.array([sx, sy, 0.0]) / np.sqrt(2.0)
        # block: one edge horizontal and perpendicular to the approach (rotate 45 deg about the horizontal axis normal to `out`)
        t = np.array([-out[1], out[0], 0.0])                       # horizontal, perpendicular to out
        a = np.pi / 4 + rng.normal() * 0.05
        qa = np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * t])  # rotation about t: a block edge parallel to t leads
        yaw = np.arctan2(t[1], t[0]) + rng.normal() * 0.05          # align a block axis with t first
        qy = np.array([np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)])
        w1, x1, y1, z1 = qa; w2, x2, y2, z2 = qy
        q = np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                      w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])
        gap = 0.002 + rng.uniform(-0.0015, 0.0005)                  # edge-to-edge distance along `out`
        edge = TC + np.array([sx * TS[0], sy * TS[1], rng.uniform(0.1, 0.7) * TS[2]])   # upper half: clear of the wheels
        c = edge + out * (gap + BS * np.sqrt(2.0))
        qpos[i, 9:12] = c + np.array([0, 0, 1.0]); qpos[i, 12:16] = q / np.linalg.norm(q)
        qvel[i, 8:11] = -out * rng.uniform(0.0, 1.0) + rng.normal(size=3) * 0.05
        qvel[i, 11:14] = rng.normal(size=3) * 0.5
    return qpos, qvel


def floor_states(n=128, seed=23):
    """Env01: robot in random orientations (upright, lying on the torso's broad face, on a wheel's flat side, anything) pressed
    0..3 mm (flat poses up to 15 mm) into the floor with random velocities -> (qpos [n,9], qvel [n,8])"""
    rng = np.random.default_rng(seed)
    wp = [WP[1], WP[2]]
    pts = [TC + np.array([sx, sy, sz]) * TS for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    for w in wp:
        for th in np.linspace(0, 2 * np.pi, 48, endpoint=False):
            for ax in (-0.013, 0.013):
                pts.append(w + np.array([ax, 0.034 * np.cos(th), 0.034 * np.sin(th)]))
    pts = np.array(pts)
    qpos = np.zeros((n, 9)); qvel = np.zeros((n, 8))
    for i in range(n):
        q = rng.normal(size=4)
        if i % 4 == 0:
            q = np.array([1.0, 0, 0, 0]) + 0.05 * rng.normal(size=4)
        elif i % 4 == 1:
            a = rng.choice([-1.0, 1.0]) * (np.pi / 2 + 0.02 * rng.normal())
            q = np.array([np.cos(a / 2), np.sin(a / 2), 0, 0]) + 0.004 * rng.normal(size=4)
        elif i % 4 == 2:
            a = rng.choice([-1.0, 1.0]) * (np.pi / 2 + 0.02 * rng.normal())
            q = np.array([np.cos(a / 2), 0, np.sin(a / 2), 0]) + 0.004 * rng.normal(size=4)
        q /= np.linalg.norm(q)
        low = (pts @ quat_to_mat(q).T)[:, 2].min()
        qpos[i, 3:7] = q; qpos[i, 2] = -0.02 - low - rng.uniform(0.0, 0.003 if i % 4 in (0, 3) else 0.015)
        qvel[i, :3] = rng.normal(size=3) * 0.3; qvel[i, 3:6] = rng.normal(size=3) * 2.0; qvel[i, 6:8] = rng.normal(size=2) * 15.0
    return qpos, qvel


def coupled_contact_count(orc, n):
    """block<->robot contacts per env as the oracle generates them"""
    return np.array([sum(1 for c in orc.forward(env=i)["contacts"] if c["body2"] == 4 and c["body1"] != 0) for i in range(n)])


def rel_vel_error(v_ref, v):
    return np.abs(v_ref - v).max(axis=1) / (1.0 + np.abs(v_ref).max(axis=1))


# ---- the scenarios: env id, states, wheel-speed targets, substeps, and what the states must cover for the comparison to mean
# something: probe(teacher, qpos) is read on the teacher (the oracle) before every physics call and asserts what the states alone
# decide; covered(probes, teacher qvel) asserts the rest after the run
def _block_robot_covered(most, vt):
    # the kernel holds 7 block<->robot slots (6 patch points + the wheel point): whatever the generator emits fits
    assert 5 <= max(most) <= 7, most   # the states must exercise more than the 4 slots of round 1
    touched = np.abs(vt[:, :6]).max(axis=1) > 1e-6          # the robot was pushed: a coupled contact acted
    assert touched.sum() > len(vt) // 3, "a coupled contact acted on the robot"


def _edge_edge_probe(teacher, qpos):
    from oracle import oracle as O
    codes = [O.box_box_points(TS, BS, q[9:12] - np.array([0, 0, 1.0]) - TC, quat_to_mat(q[12:16]), 0.002)[3] for q in qpos]
    assert sum(c >= 6 for c in codes) > len(qpos) // 2 and sum(c < 0 for c in codes) > 4, "edge-pair contacts and near misses"


def _floor_probe(teacher, qpos):
    ncon = np.array([teacher.forward(env=i)["ncon"] for i in range(len(qpos))])
    assert ncon.min() >= 1 and ncon.max() >= 6, (ncon.min(), ncon.max())


SCENARIOS = {
    "block_robot": dict(env="Env03-v2", states=block_robot_states, ctrl=lambda n: np.zeros((n, 2)), nsub=5, covered=_block_robot_covered,
                        probe=lambda teacher, qpos: int(coupled_contact_count(teacher, len(qpos)).max())),
    "edge_edge": dict(env="Env03-v2", states=edge_edge_states, ctrl=lambda n: np.zeros((n, 2)), nsub=5, covered=lambda probes, vt: None,
                      probe=_edge_edge_probe),
    "floor": dict(env="Env01-v2", states=floor_states, ctrl=lambda n: np.random.default_rng(5).uniform(-30, 30, size=(n, 2)), nsub=5,
                  covered=lambda probes, vt: None, probe=_floor_probe),
}


def scenario_inputs(name, index=None):
    """-> (qpos, qvel, ctrl) of a scenario; index: rows to take (tests/test_launch_geometry_gpu.py tiles them over several waves)"""
    qpos, qvel = SCENARIOS[name]["states"]()
    ctrl = SCENARIOS[name]["ctrl"](len(qpos))
    return (qpos, qvel, ctrl) if index is None else (qpos[index], qvel[index], ctrl[index])


def run_scenario(name, student, teacher, index=None, per_call=None):
    """both sides from the scenario's states, nsub substeps -- in one physics call, or per_call at a time where a test watches
    the contacts in between (on the host builds and on the HIP path the two differ in rounding: hints and the warm start are
    carried inside a call) -- with the targets rounded to the student's precision.  -> (relative velocity error per env, teacher qvel)"""
    sc, (qpos, qvel, ctrl) = SCENARIOS[name], scenario_inputs(name, index)
    ctrl, per_call, probes = P.round_ctrl(ctrl, student), per_call or sc["nsub"], []
    teacher.set_state(qpos, qvel); student.set_state(qpos, qvel)
    for _ in range(0, sc["nsub"], per_call):
        probes.append(sc["probe"](teacher, qpos))
        teacher.physics(ctrl, per_call); student.physics(ctrl, per_call)
    vt, vs = teacher.get_state()[1], student.get_state()[1]
    sc["covered"](probes, vt)
    assert np.isfinite(vs).all()
    return rel_vel_error(vt, vs), vt


def run_scenario_on(backend, name, index=None, per_call=None, **kw):
    """run_scenario on a fresh `backend` student against a fresh oracle.  kw: more arguments of P.make (block_threads)"""
    n = len(scenario_inputs(name, index)[0])
    student = P.make(backend, SCENARIOS[name]["env"], n, noise=False, **kw)
    teacher = P.make("oracle", SCENARIOS[name]["env"], n, noise=False)
    out = run_scenario(name, student, teacher, index, per_call)
    student.close(); teacher.close()
    return out


# ---- caps of the HIP path on the scenarios (tests/test_gpu_parity.py at 64 threads, tests/test_launch_geometry_gpu.py at 256):
# label, quantile, cap on that quantile, cap on the maximum
HIP_CAPS = {
    # measured 2.8e-7 / 3.1e-7 (deterministic arithmetic).  The cap on the maximum sits BELOW the 7.0e-7 the first version of the
    # patch-frame algebra reached (relative twist taken at the torso origin: the block's point acceleration as a difference of two
    # large terms) -- the form that put one campaign env-step at 2.4e-4
    "block_robot": ("block<->robot", 0.98, 5e-7, 5e-7),
    "edge_edge": ("edge-edge", 0.95, 2e-6, 5e-6),   # measured 1.1e-7 / 1.5e-7: a point existing on one side only would show as ~1e-2
    "floor": ("floor", 0.98, 5e-7, 1e-6),           # measured 2.8e-8 / 3.8e-8
}


def check_hip_caps(name, err, vt):
    label, q, q_cap, max_cap = HIP_CAPS[name]
    print(f"{label} constructed states on HIP: rel. velocity error q{round(100 * q)} {np.quantile(err, q):.3g}, max {err.max():.3g}")
    assert np.quantile(err, q) < q_cap and err.max() < max_cap, (np.quantile(err, q), err.max())
