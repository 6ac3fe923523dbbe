"""Block-robot collisions held to laws the model must obey whatever generates the contacts: shared by
tests/test_invariants_cpu.py (oracle, kernel source on the host) and tests/test_invariants_gpu.py (the HIP path).

  cases       56 seeded Env03 collisions = 8 draws x 7 aim points on the robot (torso faces, a vertical torso edge, both wheel
              rims, both wheels' outer faces), in flight (nothing but the block touches the robot) and standing on the floor
  meter       total linear and angular momentum of robot + block from states alone: contact forces between the two are
              internal (Newton's third law), so in flight both change by gravity only
  maps        the model's exact symmetries with their inverses: mirror x -> -x, half turn about the vertical, horizontal
              translation.  A general yaw is NOT one (the friction pyramid's tangent axes are tied to the world axes)
  runners     free-running chunks, and symmetry pairs teacher-forced per chunk the way tests/parity.py forces them

State layout (Env03): qpos [0:3] torso position, [3:7] quaternion wxyz, [7:9] wheel angles, [9:12] block position, [12:16] block
quaternion; qvel [0:3] world linear, [3:6] body-frame angular, [6:8] wheel rates, [8:11] block linear (world), [11:14] block
angular (block frame).  Test infrastructure, not a test module."""
import numpy as np

from tests import parity as P
from tests.constructed_states import BS, TC, TS, WP, quat_to_mat

ENV = "Env03-v2"
AIMS = np.array([(0.0, 0.0, 0.12), (0.03, 0.0, 0.16),            # torso faces
                 (0.05, 0.0185, 0.1),                            # a vertical torso edge
                 (0.074, 0.0, 0.034), (-0.074, 0.0, 0.034),      # the wheel rims
                 (0.087, 0.0, 0.05), (-0.087, 0.0, 0.03)])       # the wheels' outer faces
WHEEL_AIMS = (3, 4, 5, 6)
DRAWS, START, CLOSING = 8, 0.12, 2.0
CHUNKS, NSUB, DT = 10, 250, 2e-5      # a run: 10 x physics(ctrl, 250) = 50 ms
G = 9.81
ROBOT_COM = np.array([0.0, 0.0, 0.08444365])   # torso frame: model_info() masses / ipos and the wheel positions (robot_com)
TORSO, WHEEL_L, WHEEL_R, BLOCK, FLOOR = 1, 2, 3, 4, 0
COUPLED_PAIRS = {(TORSO, BLOCK), (WHEEL_L, BLOCK), (WHEEL_R, BLOCK)}
FLOOR_PAIRS = {(FLOOR, WHEEL_L), (FLOOR, WHEEL_R), (FLOOR, BLOCK)}


def _unit(v):
    return v / np.linalg.norm(v)


def _clear(c, reach=BS * np.sqrt(3.0) + 0.002 + 0.003):
    """the block's bounding sphere plus the contact margin, centred at c (torso frame), stays 3 mm clear of the torso box and
    of both wheels"""
    d_torso = np.linalg.norm(np.maximum(np.abs(c - TC) - TS, 0.0))
    d_wheel = min(np.hypot(max(abs(c[0] - w[0]) - 0.013, 0.0), max(np.hypot(c[1] - w[1], c[2] - w[2]) - 0.034, 0.0)) for w in WP.values())
    return min(d_torso, d_wheel) > reach


def cases(scene, seed=9, start=START):
    """the 56 cases of `scene` ("flight" | "floor") -> (qpos [56,16], qvel [56,14], ctrl [56,2]); ctrl is representable in
    fp32, so every back end takes the same targets.  start: distance of the block centre from the aim point"""
    assert scene in ("flight", "floor")
    rng = np.random.default_rng([seed, scene == "floor"])
    n = DRAWS * len(AIMS)
    qpos = np.zeros((n, 16)); qvel = np.zeros((n, 14))
    ctrl = (rng.normal(size=(n, 2)) * 5.0).astype(np.float32).astype(np.float64)
    for i in range(n):
        a = i % len(AIMS)
        if scene == "flight":
            qpos[i, 2] = 5.0
            qpos[i, 3:7] = _unit(rng.normal(size=4))
            qvel[i, 0:3] = rng.normal(size=3) * 0.3; qvel[i, 3:6] = rng.normal(size=3) * 2.0
        else:
            qpos[i, 3:7] = _unit(np.concatenate([[1.0], rng.normal(size=3) * 0.08 / 2]))
            qvel[i, 0:3] = rng.normal(size=3) * 0.02; qvel[i, 3:6] = rng.normal(size=3) * 0.2
        qvel[i, 6:8] = rng.normal(size=2) * 5.0
        R = quat_to_mat(qpos[i, 3:7])
        while True:                            # from the aim point to where the block starts; redrawn while the block would
            u = _unit(rng.normal(size=3))      # start within reach of the robot (a random direction can lead THROUGH it)
            if a in WHEEL_AIMS:
                u[0] = np.sign(AIMS[a][0]) * abs(u[0])     # torso frame: a wheel is approached from its own side
            u = R @ u
            if scene == "floor":
                u[2] = abs(u[2])
            if _clear(AIMS[a] + start * (R.T @ u)):
                break
        aim = qpos[i, 0:3] + R @ AIMS[a]
        v_aim = qvel[i, 0:3] + R @ np.cross(qvel[i, 3:6], AIMS[a])
        qpos[i, 9:12] = aim + start * u
        qpos[i, 12:16] = _unit(rng.normal(size=4))
        qvel[i, 8:11] = v_aim - CLOSING * u
        qvel[i, 11:14] = rng.normal(size=3) * 5.0
    return qpos, qvel, ctrl


def tile(arrays, n):
    """the cases repeated cyclically to n rows"""
    idx = np.arange(n) % len(arrays[0])
    return tuple(a[idx] for a in arrays)


# ---- the momentum meter: states in, momenta out.  One Oracle serves every build
def robot_com(orc):
    """the robot's centre of mass in the torso frame, from the oracle's body masses, inertial offsets and the wheel positions"""
    mi = orc.model_info()
    pos = np.array([[0.0, 0.0, 0.0], [-0.074, 0.0, 0.034], [0.074, 0.0, 0.034]]) + mi["body_ipos"][1:4]
    return (mi["body_mass"][1:4, None] * pos).sum(axis=0) / mi["body_mass"][1:4].sum()


class Meter:
    def __init__(self, n, env=ENV):
        self.orc = P.make("oracle", env, n, noise=False)
        self.n = n
        np.testing.assert_allclose(robot_com(self.orc), ROBOT_COM, atol=1e-8)

    def close(self):
        self.orc.close()

    def momenta(self, qpos, qvel):
        """-> (P [n,3] total linear momentum, L_C [n,3] angular momentum about the system's centre of mass,
        p_block [n,3], masses (robot, block))"""
        self.orc.set_state(qpos, qvel)
        Pt, Lc, pb = np.zeros((self.n, 3)), np.zeros((self.n, 3)), np.zeros((self.n, 3))
        for i in range(self.n):
            M = self.orc.forward(env=i)["M"]
            p = M @ qvel[i]
            Rb, Rk = quat_to_mat(_unit(qpos[i, 3:7])), quat_to_mat(_unit(qpos[i, 12:16]))
            xt, xk = qpos[i, 0:3], qpos[i, 9:12]
            m_r, m_k = M[0, 0], M[8, 8]
            Pt[i] = p[0:3] + p[8:11]
            L_O = Rb @ p[3:6] + np.cross(xt, p[0:3]) + Rk @ p[11:14] + np.cross(xk, p[8:11])
            X = (m_r * (xt + Rb @ ROBOT_COM) + m_k * xk) / (m_r + m_k)
            Lc[i] = L_O - np.cross(X, Pt[i])
            pb[i] = p[8:11]
        return Pt, Lc, pb, (m_r, m_k)

    def pairs(self, qpos, qvel, ctrl):
        """body pairs in the oracle's contact lists at these states -> [set per env]"""
        self.orc.set_state(qpos, qvel)
        return [{(int(c["body1"]), int(c["body2"])) for c in self.orc.forward(env=i, ctrl=tuple(ctrl[i]))["contacts"]}
                for i in range(self.n)]


def conservation(meter, states, dt_chunk=NSUB * DT):
    """states: [(qpos, qvel)] at chunk boundaries 0..K -> per case: linear defect max_t |P(t) - P(0) + M g t z|, angular defect
    max_t |L_C(t) - L_C(0)|, exchanged impulse J = max_t |dP_block + m_block g t z|"""
    z = np.array([0.0, 0.0, 1.0])
    P0, L0, b0, (m_r, m_k) = meter.momenta(*states[0])
    lin = np.zeros(meter.n); ang = np.zeros(meter.n); J = np.zeros(meter.n)
    for k, (q, v) in enumerate(states[1:], 1):
        t = k * dt_chunk
        Pk, Lk, bk, _ = meter.momenta(q, v)
        lin = np.maximum(lin, np.linalg.norm(Pk - P0 + (m_r + m_k) * G * t * z, axis=1))
        ang = np.maximum(ang, np.linalg.norm(Lk - L0, axis=1))
        J = np.maximum(J, np.linalg.norm(bk - b0 + m_k * G * t * z, axis=1))
    return lin, ang, J


LIN_GATE, ANG_GATE, ARM, J_MIN = 2e-3, 5e-4, 0.1, 0.01   # defects relative to J and J x 0.1 m; the oracle shows 5.9e-4 / 5.7e-5


def check_conservation(label, lin, ang, J):
    rl, ra = float((lin / J).max()), float((ang / (J * ARM)).max())
    print(f"{label}: J min {J.min():.3g} median {np.median(J):.3g} N s; linear defect / J max {rl:.3g} (gate {LIN_GATE:g}), "
          f"angular defect / (J x 0.1 m) max {ra:.3g} (gate {ANG_GATE:g})")
    assert (J > J_MIN).all(), f"{label}: {int((J <= J_MIN).sum())} cases without a collision (J min {J.min():.3g})"
    assert rl < LIN_GATE, f"{label}: linear momentum defect {rl:.3g} of the impulse exchanged"
    assert ra < ANG_GATE, f"{label}: angular momentum defect {ra:.3g} of the impulse exchanged x 0.1 m"


# ---- the maps: T(qpos, qvel, ctrl) -> image; each with its inverse.  Warm starts (accelerations) map like velocities
def qmul(a, b):
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0); w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


class Map:
    """pos(qpos), vel(qvel), ctrl(ctrl) -> images (new arrays); .inv is the inverse map"""

    def __init__(self, name, pos, vel, ctrl, inv=None):
        self.name, self.pos, self.vel, self.ctrl, self.inv = name, pos, vel, ctrl, inv or self


_SAME = lambda a: np.array(a, dtype=np.float64, copy=True)


def _mirror_pos(q):
    q = _SAME(q)
    q[:, 0] *= -1; q[:, 9] *= -1
    q[:, 3:7] *= (1, 1, -1, -1); q[:, 12:16] *= (1, 1, -1, -1)
    q[:, 7], q[:, 8] = -q[:, 8].copy(), -q[:, 7].copy()     # the hinge axes are (-1,0,0) and (+1,0,0): swap AND negate
    return q


def _mirror_vel(v):
    v = _SAME(v)
    v[:, 0] *= -1; v[:, 8] *= -1
    v[:, 3:6] *= (1, -1, -1); v[:, 11:14] *= (1, -1, -1)    # angular velocity is a pseudo-vector
    v[:, 6], v[:, 7] = -v[:, 7].copy(), -v[:, 6].copy()
    return v


def _mirror_ctrl(c):
    c = np.asarray(c)
    return np.stack([-c[:, 1], -c[:, 0]], axis=1)


def _turn_pos(sign):
    def f(q):
        q = _SAME(q)
        q[:, [0, 1, 9, 10]] *= -1
        h = np.array([0.0, 0.0, 0.0, sign])
        q[:, 3:7] = qmul(h, q[:, 3:7]); q[:, 12:16] = qmul(h, q[:, 12:16])
        return q
    return f


def _turn_vel(v):
    v = _SAME(v)
    v[:, [0, 1, 8, 9]] *= -1
    return v


def _shift_pos(dx, dy):
    def f(q):
        q = _SAME(q)
        q[:, [0, 9]] += dx; q[:, [1, 10]] += dy
        return q
    return f


def yaw_map(angle):
    """rotation of the world about the vertical by `angle`: a symmetry only while nothing touches"""
    c, s = np.cos(angle), np.sin(angle)
    Rz = np.array([[c, -s], [s, c]])

    def mk(a):
        h = np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)])
        Ra = Rz if a == angle else Rz.T

        def pos(q):
            q = _SAME(q)
            q[:, 0:2] = q[:, 0:2] @ Ra.T; q[:, 9:11] = q[:, 9:11] @ Ra.T
            q[:, 3:7] = qmul(h, q[:, 3:7]); q[:, 12:16] = qmul(h, q[:, 12:16])
            return q

        def vel(v):
            v = _SAME(v)
            v[:, 0:2] = v[:, 0:2] @ Ra.T; v[:, 8:10] = v[:, 8:10] @ Ra.T
            return v
        return pos, vel
    m = Map(f"yaw {angle:g}", *mk(angle), _SAME)
    m.inv = Map(f"yaw {-angle:g}", *mk(-angle), _SAME, inv=m)
    return m


MIRROR = Map("mirror", _mirror_pos, _mirror_vel, _mirror_ctrl)
HALF_TURN = Map("half turn", _turn_pos(1.0), _turn_vel, _SAME)
HALF_TURN.inv = Map("half turn back", _turn_pos(-1.0), _turn_vel, _SAME, inv=HALF_TURN)
SHIFT = (37.5, -21.25)
TRANSLATION = Map("translation", _shift_pos(*SHIFT), _SAME, _SAME)
TRANSLATION.inv = Map("translation back", _shift_pos(-SHIFT[0], -SHIFT[1]), _SAME, _SAME, inv=TRANSLATION)
MAPS = {"mirror": MIRROR, "half_turn": HALF_TURN, "translation": TRANSLATION}


def state_distance(qa, va, qb, vb):
    """(max |dqpos|, max |dqvel|) per env, quaternion signs aligned first"""
    qb = _SAME(qb)
    for s in (slice(3, 7), slice(12, 16)):
        flip = (qa[:, s] * qb[:, s]).sum(axis=1) < 0
        qb[flip, s] *= -1
    return np.abs(qa - qb).max(axis=1), np.abs(va - vb).max(axis=1)


# ---- runners
def run_free(sim, qpos, qvel, ctrl, chunks=CHUNKS, nsub=NSUB):
    """set_state, then `chunks` x physics(ctrl, nsub) -> [(qpos, qvel)] at the chunk boundaries 0..chunks"""
    sim.set_state(qpos, qvel, np.zeros_like(qvel), np.zeros(len(qpos)))
    out = [(qpos.copy(), qvel.copy())]
    for _ in range(chunks):
        sim.physics(ctrl, nsub)
        q, v, _, _ = sim.get_state()
        out.append((q, v))
    return out


def free_symmetry(sim_a, sim_b, T, qpos, qvel, ctrl, chunks=CHUNKS, nsub=NSUB):
    """copy A from the state, copy B from its image under T, both free-running -> (max dq, max dv) of A against T^-1(B) over
    all chunk boundaries and cases"""
    sa = run_free(sim_a, qpos, qvel, ctrl, chunks, nsub)
    sb = run_free(sim_b, T.pos(qpos), T.vel(qvel), T.ctrl(ctrl), chunks, nsub)
    dq = dv = 0.0
    for (qa, va), (qb, vb) in zip(sa[1:], sb[1:]):
        a, b = state_distance(qa, va, T.inv.pos(qb), T.inv.vel(vb))
        dq, dv = max(dq, float(a.max())), max(dv, float(b.max()))
    return dq, dv


def teacher_states(scene, n=None, chunks=CHUNKS, nsub=NSUB, env=ENV, **kw):
    """the oracle free-running over the cases of `scene` (tiled to n) -> (ctrl, [(qpos, qvel, warm, time)] at the chunk
    boundaries 0..chunks).  kw: the oracle's substeps / timestep"""
    qpos, qvel, ctrl = cases(scene)
    orc = P.make("oracle", env, len(qpos), noise=False, **kw)     # the unique cases run once; the tiled rows are copies
    orc.set_state(qpos, qvel, np.zeros_like(qvel), np.zeros(len(qpos)))
    out = [orc.get_state()]
    for _ in range(chunks):
        orc.physics(ctrl, nsub)
        out.append(orc.get_state())
    orc.close()
    return (ctrl, out) if not n else (tile((ctrl,), n)[0], [tile(s, n) for s in out])


def forced_symmetry(sim_a, sim_b, T, ctrl, teacher, nsub=NSUB):
    """the convention of tests/parity.py, per chunk: A is forced to the teacher's state S_k and B to T(S_k); both run one
    chunk; A is compared with T^-1(B), and each with the teacher's S_k+1.
    -> dict of max |dqpos| / |dqvel| over chunks and cases: pair, a (A to the teacher), b (T^-1(B) to the teacher)"""
    out = dict(pair=0.0, a=0.0, b=0.0, pair_v=0.0, a_v=0.0, b_v=0.0)
    ctrl_b = T.ctrl(ctrl)
    for (q0, v0, w0, t0), (q1, v1, _, _) in zip(teacher[:-1], teacher[1:]):
        sim_a.set_state(q0, v0, w0, t0); sim_b.set_state(T.pos(q0), T.vel(v0), T.vel(w0), t0)
        sim_a.physics(ctrl, nsub); sim_b.physics(ctrl_b, nsub)
        qa, va, _, _ = sim_a.get_state()
        qb, vb, _, _ = sim_b.get_state()
        qb, vb = T.inv.pos(qb), T.inv.vel(vb)
        for key, (x, y) in dict(pair=state_distance(qa, va, qb, vb), a=state_distance(q1, v1, qa, va),
                                b=state_distance(q1, v1, qb, vb)).items():
            out[key] = max(out[key], float(x.max())); out[key + "_v"] = max(out[key + "_v"], float(y.max()))
    return out


def check_forced(label, d):
    """the project's strict bound, and a cap at 8x the larger of the two distances to the oracle this test measured"""
    cap = 8 * max(d["a"], d["b"])
    print(f"{label}: A against T^-1(B) dq {d['pair']:.3g} dv {d['pair_v']:.3g}; against the oracle: A dq {d['a']:.3g} dv {d['a_v']:.3g}, "
          f"T^-1(B) dq {d['b']:.3g} dv {d['b_v']:.3g}; cap {cap:.3g} (bound {P.TOL_QPOS:g})")
    assert cap <= P.TOL_QPOS, f"{label}: the distance to the oracle puts the cap at {cap:.3g}"
    assert d["pair"] < P.TOL_QPOS and d["pair"] < cap, f"{label}: symmetry defect {d['pair']:.3g} (cap {cap:.3g})"
