"""Constructed contact states shared by tests/test_hostsim_parity.py and tests/test_constructed_steps.py (kernel source on the
host), tests/test_gpu_parity.py, tests/test_launch_geometry_gpu.py and tests/test_constructed_steps_gpu.py (the HIP path): states a
random rollout reaches only by chance -- the block against every torso face and both wheels (5- and 6-point patches, edge-edge
poses, the wheel barrel), the robot pressed into the floor in every orientation, and a block lying on the floor and pushed
against the standing robot (robot<->floor, block<->floor and block<->robot contacts at once).  Geometry re-typed from the
reference's XML (envs/robot-02.xml:4-20, envs/env03_v1.xml:31-37).  SCENARIOS holds what a run of them needs; on any back end of
tests/parity.py, run_scenario runs one through the physics call (a few substeps, velocities compared) and run_scenario_steps
through full env steps (teacher-forced, gates G1-G3, flags, reward, observations).  Test infrastructure."""
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


def pinned_states(n=96, seed=31):
    """Env03: robot standing on the floor (0..2 mm into it, small pitch), block lying flat on the floor (0..1.5 mm into it)
    and pushed against the robot from the front or the back, gap -1.5 .. +1.5 mm: against a wheel's barrel, against the
    torso's broad face between the wheels, or against that face with the block's side within -1 .. +2 mm of a wheel's inner
    flat side.  Robot<->floor, block<->floor and block<->robot contacts at once -> (qpos [n,16], qvel [n,14])"""
    rng = np.random.default_rng(seed)
    qpos = np.zeros((n, 16)); qvel = np.zeros((n, 14))
    for i in range(n):
        s, side = rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0])
        gap = rng.uniform(-0.0015, 0.0015)
        if i % 3 == 0:     # wheel barrel (radius 0.034)
            x, y = side * 0.074 + rng.uniform(-0.010, 0.010), s * (0.034 + BS + gap)
        elif i % 3 == 1:   # torso broad face, between the wheels
            x, y = rng.uniform(-0.035, 0.035), s * (TS[1] + BS + gap)
        else:              # the same face, the block's side at a wheel's inner flat side (|x| = 0.074 - 0.013)
            x, y = side * (0.074 - 0.013 - BS - rng.uniform(-0.001, 0.002)), s * (TS[1] + BS + gap)
        pitch, yaw = rng.normal() * 0.03, rng.normal() * 0.03
        qpos[i, 2] = -0.02 - rng.uniform(0.0, 0.002)
        qpos[i, 3:7] = [np.cos(pitch / 2), np.sin(pitch / 2), 0, 0]
        qpos[i, 9:12] = [x, y, -0.02 + BS - rng.uniform(0.0, 0.0015)]
        qpos[i, 12:16] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        qvel[i, :3] = rng.normal(size=3) * 0.1; qvel[i, 3:6] = rng.normal(size=3) * 1.0; qvel[i, 6:8] = rng.normal(size=2) * 10.0
        while True:        # a block slower than 0.1 m/s is taken away by the env logic: keep clear of that decision
            v = rng.normal(size=3) * 0.3 + np.array([0.0, -s * rng.uniform(0.0, 1.0), 0.0])
            if np.linalg.norm(v) >= 0.15:
                break
        qvel[i, 8:11] = v; qvel[i, 11:14] = rng.normal(size=3) * 2.0
    return qpos, qvel


def contact_families(orc, n):
    """[n, 3] contacts per env as the oracle generates them: robot<->floor, block<->floor, block<->robot"""
    out = np.zeros((n, 3), int)
    for i in range(n):
        for c in orc.forward(env=i)["contacts"]:
            out[i, 2 if c["body1"] != 0 else 1 if c["body2"] == 4 else 0] += 1
    return out


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


def _pinned_probe(teacher, qpos):
    fam = contact_families(teacher, len(qpos))
    assert (fam[:, 0] == 4).all() and (fam[:, 1] == 4).all(), "4 robot<->floor and 4 block<->floor contacts (the block-slot capacity)"
    assert (fam > 0).all(axis=1).mean() >= 0.8, "all three contact families at once in most envs"
    assert ((fam.sum(axis=1) >= 12) & (fam[:, 2] >= 4)).any(), fam.sum(axis=1).max()


SCENARIOS = {
    "block_robot": dict(env="Env03-v2", states=block_robot_states, ctrl=lambda n: np.zeros((n, 2)), nsub=5, covered=_block_robot_covered,
                        probe=lambda teacher, qpos: int(coupled_contact_count(teacher, len(qpos)).max())),
    "edge_edge": dict(env="Env03-v2", states=edge_edge_states, ctrl=lambda n: np.zeros((n, 2)), nsub=5, covered=lambda probes, vt: None,
                      probe=_edge_edge_probe),
    "floor": dict(env="Env01-v2", states=floor_states, ctrl=lambda n: np.random.default_rng(5).uniform(-30, 30, size=(n, 2)), nsub=5,
                  covered=lambda probes, vt: None, probe=_floor_probe),
    "pinned": dict(env="Env03-v2", states=pinned_states, ctrl=lambda n: np.random.default_rng(5).uniform(-30, 30, size=(n, 2)), nsub=5,
                   covered=lambda probes, vt: None, probe=_pinned_probe),
}


def scenario_inputs(name, index=None):
    """-> (qpos, qvel, ctrl) of a scenario; index: rows to take (tests/test_launch_geometry_gpu.py tiles them over several waves)"""
    qpos, qvel = SCENARIOS[name]["states"]()
    ctrl = SCENARIOS[name]["ctrl"](len(qpos))
    return (qpos, qvel, ctrl) if index is None else (qpos[index], qvel[index], ctrl[index])


def tile(m, n, seed):
    """indices of n states drawn from m: whole random permutations of the m, one after another, cut at n (no two waves hold
    the same states at the same lanes)"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.permutation(m) for _ in range(-(-n // m))])[:n]


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


# ---- full env steps from the scenarios' states: what the product's step kernels (brs_step) run, where run_scenario goes through
# the physics call alone
def _scenario_actions(t, n, rng, obs):
    return rng.uniform(-1.5, 1.5, size=(n, 2)).astype(np.float32)


def run_scenario_steps(name, student, teacher, steps=2, index=None):
    """both sides reset, the teacher put on the scenario's states, then `steps` teacher-forced FULL env steps (P.env_steps) with
    seeded actions U(-1.5, 1.5)^2.  The simulators come with auto-reset and noise off, of any env id whose state has the
    scenario's width.  An env-step is left out only where the block timer went on for one side alone (P.timer_mask): nothing
    is re-drawn without auto-reset, and the robots of `floor` that lie on the ground and terminate at every step are the point.
    -> (P.Gates of the kept env-steps, kept share, [record per step])"""
    qpos, qvel, _ = scenario_inputs(name, index)
    teacher.reset(); student.reset()
    teacher.set_state(qpos, qvel)
    g, recs = P.Gates(), []
    for r in P.env_steps(teacher, student, steps, _scenario_actions, np.random.default_rng(41), skip=P.timer_mask):
        g.add(r.pre["qpos"], r.post_s[0], r.post_t[0], r.skip)
        recs.append(r)
    kept = 1.0 - sum(int(r.skip.sum()) for r in recs) / float(len(qpos) * steps)
    return g, kept, recs


def check_scenario_steps(name, label, g, kept, recs, cap=P.TOL_QPOS):
    """what a run_scenario_steps result must satisfy on every back end; cap: on G1-G3 (<= P.TOL_QPOS).  Reward and observations
    are compared on the env-steps that start upright: a fallen robot's pitch sits near the Euler singularity (the float build
    on the CPU differs from the oracle by 3.7e-3 in obs there), so those are compared in state and flags"""
    label = f"{name} from constructed states, full env steps, {label}"
    try:
        g.check(label, robot_cap=cap, block_cap=cap, fallen_cap=cap)
    except AssertionError as e:
        raise AssertionError(f"{label}: {e}") from None
    n_term = sum(int((r.out_s[2] != r.out_t[2]).sum()) for r in recs)
    print(f"{label}: kept {100 * kept:.2f} % of {len(recs) * len(recs[0].skip)} env-steps, termination disagreements {n_term}")
    assert kept >= 0.98, f"{label}: kept share {kept:.3f}"
    if name == "edge_edge":   # the scenario is about the block: the env logic must not have taken most of them away
        have = int(np.isnan(recs[0].aux_t[:, 1]).sum())
        assert have >= 0.75 * len(recs[0].skip), f"{label}: {have} blocks left after step 0"
    assert n_term <= 2, f"{label}: {n_term} termination disagreements"
    worst = dict(reward=0.0, obs=0.0, obs1=0.0)
    for r in recs:
        (o_s, r_s, te_s, tr_s, to_s), (o_t, r_t, te_t, tr_t, to_t) = r.out_s, r.out_t
        assert np.isfinite(r.post_s[0]).all() and np.isfinite(r.post_s[1]).all(), f"{label}: step {r.t}: state not finite"
        assert np.array_equal(tr_s, tr_t), f"{label}: step {r.t}: truncated differs"
        assert not r.aux_t[:, 7].any(), f"{label}: step {r.t}: the oracle's bad-state guard re-drew an env"
        ok = (te_s == te_t) & ~r.skip
        assert np.array_equal(r.aux_s[ok][:, 2:5], r.aux_t[ok][:, 2:5]), f"{label}: step {r.t}: elapsed steps, rng counter, attack side"
        tim_s, tim_t = r.aux_s[ok][:, 1], r.aux_t[ok][:, 1]
        assert np.array_equal(tim_s[~np.isnan(tim_s)], tim_t[~np.isnan(tim_t)]), f"{label}: step {r.t}: block timers"
        up = ok & P.upright(r.pre["qpos"])
        rest = [0, 2, 3, 4, 5]
        worst["reward"] = max(worst["reward"], float(np.abs(r_s[up] - r_t[up]).max(initial=0.0)))
        for a, b in ((o_s, o_t), (to_s, to_t)):
            worst["obs"] = max(worst["obs"], float(np.abs(a[up][:, rest] - b[up][:, rest]).max(initial=0.0)))
            worst["obs1"] = max(worst["obs1"], float(np.abs(a[up][:, 1] - b[up][:, 1]).max(initial=0.0)))
        np.testing.assert_allclose(r_s[up], r_t[up], atol=1e-4, rtol=1e-5, err_msg=f"{label}: step {r.t}: reward")
        for a, b, what in ((o_s, o_t, "obs"), (to_s, to_t, "terminal_obs")):
            np.testing.assert_allclose(a[up][:, rest], b[up][:, rest], atol=5e-4, rtol=1e-4, err_msg=f"{label}: step {r.t}: {what}")
            np.testing.assert_allclose(a[up][:, 1], b[up][:, 1], atol=5e-3, rtol=1e-3, err_msg=f"{label}: step {r.t}: {what}[1]")
    print(f"{label}: upright env-steps: max |d reward| {worst['reward']:.3g}, |d obs| {worst['obs']:.3g}, |d obs[1]| {worst['obs1']:.3g}")


def run_scenario_steps_on(backend, name, env_id=None, steps=2, index=None, cap=P.TOL_QPOS, student=lambda sim: sim, **kw):
    """run_scenario_steps and check_scenario_steps with a fresh `backend` student (wrapped by `student`) against a fresh oracle.
    env_id: another id than the scenario's own; kw: more arguments of P.make for both sides (block_threads, lane_grouping reach
    the HIP path alone).  -> (Gates, kept share, records, step kernel name or None)"""
    env_id, n = env_id or SCENARIOS[name]["env"], len(scenario_inputs(name, index)[0])
    sim = P.make(backend, env_id, n, noise=False, **kw)
    teacher = P.make("oracle", env_id, n, noise=False, **kw)
    kernel = sim.raw.step_kernel_name() if backend == "hip" else None
    g, kept, recs = run_scenario_steps(name, student(sim), teacher, steps, index)
    sim.close(); teacher.close()
    check_scenario_steps(name, f"{env_id} on {backend}" + (f" ({kernel}, {kw.get('block_threads', 64)} threads)" if kernel else ""),
                         g, kept, recs, cap)
    return g, kept, recs, kernel


# ---- caps of the HIP path on the scenarios (tests/test_gpu_parity.py at 64 threads, tests/test_launch_geometry_gpu.py at 256):
# label, quantile, cap on that quantile, cap on the maximum
HIP_CAPS = {
    # measured 2.8e-7 / 3.1e-7 (deterministic arithmetic).  The cap on the maximum sits BELOW the 7.0e-7 the first version of the
    # patch-frame algebra reached (relative twist taken at the torso origin: the block's point acceleration as a difference of two
    # large terms) -- the form that put one campaign env-step at 2.4e-4
    "block_robot": ("block<->robot", 0.98, 5e-7, 5e-7),
    "edge_edge": ("edge-edge", 0.95, 2e-6, 5e-6),   # measured 1.1e-7 / 1.5e-7: a point existing on one side only would show as ~1e-2
    "floor": ("floor", 0.98, 5e-7, 1e-6),           # measured 2.8e-8 / 3.8e-8
    # measured 3.6e-7 / 7.0e-7 (tiled at 256 threads: 3.5e-7 / 7.0e-7).  The caps are those of the float build on the host
    # (tests/test_hostsim_parity.py, which measures 2.7e-7 / 3.7e-7), not yet tightened to the measurement
    "pinned": ("pinned block", 0.98, 1e-5, 5e-5),
}


def check_hip_caps(name, err, vt):
    label, q, q_cap, max_cap = HIP_CAPS[name]
    print(f"{label} constructed states on HIP: rel. velocity error q{round(100 * q)} {np.quantile(err, q):.3g}, max {err.max():.3g}")
    assert np.quantile(err, q) < q_cap and err.max() < max_cap, (np.quantile(err, q), err.max())
