"""Teacher-forced parity: the one definition behind the parity tests and the campaign tools.

Before every step the STUDENT is given the TEACHER's qpos / qvel / warm start / time, its aux row and its accessor pose
(force).  Both sides then step.  Env-steps that ended an episode on either side, or whose block timer is on for one side
only, are left out (skip_mask); the rest is split into upright robot, upright block and fallen (group_errors) and compared
(Gates).  Simulators come from make(): the fp64 oracle, the kernel source on the host in double or float, or the HIP path,
all with the oracle's numpy surface.  Test infrastructure: tools/ import it the way they import tests.hostsim."""
import os
import types

import numpy as np

TOL_QPOS = 1e-4
BACKENDS = {"oracle": None, "host64": True, "host32": False, "hip": None}   # the host builds: double?
_CPU_KW = ("max_episode_steps", "substeps", "timestep")
_HIP_KW = _CPU_KW + ("block_threads", "lane_grouping")


class _Hip:
    """BatchedSim behind the oracle's surface: numpy in, arrays the caller owns out (BatchedSim overwrites its output
    tensors on the next call), bool flags.  The state accessors are BatchedSim's own; .raw is the handle"""
    ctrl_dtype = np.float32

    def __init__(self, raw):
        self.raw = raw

    def __getattr__(self, name):   # physics, get_/set_state, get_/set_aux, get_/set_xpose, close, n, nq, nv
        return getattr(self.raw, name)

    def reset(self, mask=None):
        import torch
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8))
        return self.raw.reset(m).cpu().numpy().copy()

    def step(self, act):
        import torch
        obs, rew, te, tr, tob = [x.cpu().numpy().copy() for x in self.raw.step(torch.from_numpy(act).cuda())]
        return obs, rew, te.astype(bool), tr.astype(bool), tob


def make(backend, env_id, n, *, seed=0, env_index_base=0, auto_reset=False, noise=None, threads=None, **kw):
    """one simulator of `backend` (BACKENDS) with reset / step / physics / get_ and set_ state, aux, xpose / close / n, nq, nv
    and ctrl_dtype, the precision in which it takes wheel-speed targets.  kw: max_episode_steps, substeps, timestep, and for
    "hip" block_threads, lane_grouping.  threads: the CPU back ends' pool (results do not depend on it: the loops are per env)"""
    threads = threads or min(16, os.cpu_count() or 1)
    if backend not in BACKENDS or set(kw) - set(_HIP_KW):
        raise TypeError(f"backend {backend!r} is not one of {list(BACKENDS)}, or unknown arguments {sorted(set(kw) - set(_HIP_KW))}")
    known = _HIP_KW if backend == "hip" else _CPU_KW   # the launch geometry means nothing to the CPU back ends
    common = dict(seed=seed, env_index_base=env_index_base, auto_reset=auto_reset, **{k: v for k, v in kw.items() if k in known})
    if backend == "hip":
        from balance_robot_mujoco_rl_amd import BatchedSim
        return _Hip(BatchedSim(env_id, n, device=0, obs_noise=noise, **common))
    if backend == "oracle":
        from oracle import oracle as O
        sim = O.Oracle(env_id, n, noise=noise, threads=threads, **common)
    else:
        from tests.hostsim.hostsim import HostSim
        sim = HostSim(env_id, n, noise=noise, double=BACKENDS[backend], threads=threads, **common)
    sim.ctrl_dtype = np.float64
    return sim


def force(student, teacher):
    """the student starts where the teacher is.  teacher: a simulator, or a state as this function / outlier_arrays return it
    (a dump without aux and accessor pose sets the state alone).  -> that state"""
    st = teacher
    if not isinstance(teacher, dict):
        st = dict(zip(("qpos", "qvel", "warm", "time", "aux", "xquat", "xpos"), (*teacher.get_state(), teacher.get_aux(), *teacher.get_xpose())))
    student.set_state(st["qpos"], st["qvel"], st["warm"], st["time"])
    if "aux" in st:   # per-episode scalars (Env02's friction) live in aux
        student.set_aux(st["aux"]); student.set_xpose(st["xquat"], st["xpos"])
    return st


def outlier_arrays(pre):
    """the `pre` dictionary of one env-step in a tools/parity_locate.py dump or in tests/golden/round3_outlier_states.json
    -> one-env arrays: a state for force(), plus ctrl [2] and action [1, 2] where the dump has them"""
    st = {k: np.array(pre[k], dtype=np.float64)[None] for k in ("qpos", "qvel", "warm", "aux", "xquat", "xpos") if k in pre}
    st.update(time=np.array([pre["time"]]), ctrl=np.array(pre["ctrl"], dtype=np.float64))
    if "action" in pre:
        st["action"] = np.array(pre["action"], dtype=np.float32)[None]
    return st


def skip_mask(out_s, out_t, aux_s, aux_t):
    """env-steps that are not compared: a finished episode was re-drawn; a block removed / re-thrown on one side only (its
    timer, aux column 1, is NaN while off) is a discrete difference"""
    done = np.logical_or.reduce([np.asarray(out[k]).astype(bool) for out in (out_s, out_t) for k in (2, 3)])
    return done | (np.isnan(aux_s[:, 1]) != np.isnan(aux_t[:, 1]))


def timer_mask(out_s, out_t, aux_s, aux_t):
    """skip_mask without the finished episodes, for runs with auto-reset off: nothing is re-drawn there, and robots that
    have fallen (and so terminate at every step) are what such a run is about"""
    return np.isnan(aux_s[:, 1]) != np.isnan(aux_t[:, 1])


def contact_pairs(orc, ctrl):
    """body pairs of the oracle's contact list for its one env, as the campaign tools print them"""
    return sorted((int(c["body1"]), int(c["body2"])) for c in orc.forward(env=0, ctrl=(float(ctrl[0]), float(ctrl[1])))["contacts"])


def reference_policy():
    """the reference's own MuJoCo-trained balance policy (tests/quant_policy.py, envs/RobotMovePolicy.tflite): obs -> actions"""
    import torch
    from tests.quant_policy import QuantMovePolicy
    qp = QuantMovePolicy()
    return lambda o: qp.act(torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32)), "mean").numpy()


def env_steps(teacher, student, steps, actions, rng, obs=None, skip=skip_mask):
    """teacher-forced FULL env steps, one record per step: t, pre (the forced state), act, out_s / out_t (step outputs),
    post_s / post_t (get_state after the step), aux_s / aux_t (after the step), skip (skip_mask, or timer_mask where a run
    with auto-reset off asks for it).  actions: "zero", "random"
    (U(-1,1)^2 from rng, one draw per step), "policy" (reference_policy on the teacher's observations) or a callable
    (t, n, rng, teacher_obs) -> float32 [n, 2].  obs: the teacher's observations before the first step.  Nothing is reset here"""
    n = teacher.n
    if actions == "policy":
        pol = reference_policy()
    actions = {"policy": lambda t, n, rng, obs: pol(obs), "zero": lambda t, n, rng, obs: np.zeros((n, 2), np.float32),
               "random": lambda t, n, rng, obs: rng.uniform(-1, 1, size=(n, 2)).astype(np.float32)}.get(actions, actions)
    for t in range(steps):
        pre = force(student, teacher)
        act = actions(t, n, rng, obs)
        out_s, out_t = student.step(act), teacher.step(act)
        obs, aux_s, aux_t = out_t[0], student.get_aux(), teacher.get_aux()
        yield types.SimpleNamespace(t=t, pre=pre, act=act, out_s=out_s, out_t=out_t, aux_s=aux_s, aux_t=aux_t,
                                    post_s=student.get_state(), post_t=teacher.get_state(),
                                    skip=skip(out_s, out_t, aux_s, aux_t))


def round_ctrl(ctrl, student):
    """wheel-speed targets as BOTH sides take them: rounded to the precision the student's physics() accepts"""
    return np.asarray(ctrl, dtype=np.float64).astype(student.ctrl_dtype).astype(np.float64)


def physics_steps(teacher, student, steps, make_ctrl, nsub=250):
    """teacher-forced physics(nsub) without the env logic, one record per step: t, pre, ctrl, post_s, post_t.
    make_ctrl(t, pre) -> [n, 2] targets"""
    for t in range(steps):
        pre = force(student, teacher)
        ctrl = round_ctrl(make_ctrl(t, pre), student)
        student.physics(ctrl, nsub); teacher.physics(ctrl, nsub)
        yield types.SimpleNamespace(t=t, pre=pre, ctrl=ctrl, post_s=student.get_state(), post_t=teacher.get_state())


def replay_substeps(teacher, student, pre, ctrl, nsub=250, *, jump_abs, jump_ratio, floor, on_substep=lambda k: None):
    """one env-step again, one substep per physics() call, both sides from the state `pre` (outlier_arrays).
    -> (first substep at which max |dqvel| exceeds jump_abs and jump_ratio x its previous value (taken as at least `floor`),
    or None; [(max |dqpos|, max |dqvel|)] per substep).  on_substep(k) is called before substep k and once more, with
    k = nsub, after the last: where a tool reads the oracle's contact list"""
    force(teacher, pre); force(student, pre)
    c = round_ctrl(ctrl, student).reshape(-1, 2)
    first, prev, trace = None, 0.0, []
    for k in range(nsub):
        on_substep(k)
        teacher.physics(c, 1); student.physics(c, 1)
        (qt, vt, _, _), (qs, vs, _, _) = teacher.get_state(), student.get_state()
        ev = float(np.abs(vs - vt).max())
        trace.append((float(np.abs(qs - qt).max()), ev))
        if first is None and ev > jump_abs and ev > jump_ratio * max(prev, floor):
            first = k
        prev = ev
    on_substep(nsub)
    return first, trace


# ---- parity gates (facts behind them: profiles/r03_parity_*.json, tools/parity_report.py)
# An env-step is UPRIGHT if the torso axis is within 60 degrees of vertical when the step starts (the env terminates at
# 50 degrees of pitch, so with auto-reset every step it keeps is upright).  FALLEN robots exist only with auto-reset off.
# Since round 3 (contact-existence and servo-clamp decisions from exact fp64 constants, fp64 velocity accumulators) the
# north-star bound holds as a STRICT maximum in every group: 0 of 8.7 M campaign env-steps above 1e-4 (worst 8.6e-5, a block
# quaternion under the balancing policy; robot coordinates 5.2e-5; fallen robots 7.2e-5).  The gates are that bound, with
# zero exceptions, plus per-test caps at ~5-10x what the test's own sample measured (r03 GPU log), so that a regression of
# one order of magnitude in the bulk fails even when no env-step crosses 1e-4:
#  G1  robot coordinates (torso position, quaternion, wheel angles), upright: max |dqpos| < 1e-4
#  G2  block coordinates, upright:                                            max |dqpos| < 1e-4
#  G3  all coordinates of fallen robots (lying flat, wheels rubbing):         max |dqpos| < 1e-4
# (round 2's gates allowed 5e-5 / 2e-4 of the env-steps above 1e-4 with caps at 1e-3, and one free outlier per test.)
COLUMNS = {"robot": slice(0, 9), "block": slice(9, 16)}


def cos_tilt(qpos):
    """cosine of the angle between the torso axis and the vertical"""
    return 1 - 2 * (qpos[:, 4] ** 2 + qpos[:, 5] ** 2)


def upright(qpos):
    return cos_tilt(qpos) > 0.5


def group_errors(qpos_pre, d, skip=None):
    """|dqpos| rows d split the way the gates split them -> (upright flag of the kept rows, {"robot/upright", "block/upright",
    "robot/fallen", "block/fallen": per-env-step max over the group's columns}).  Rows under skip are left out; a group
    without rows or without columns (no block in the Env01 family) is absent"""
    if skip is not None:
        d = d[~skip]; qpos_pre = qpos_pre[~skip]
    up = upright(qpos_pre)
    return up, {f"{g}/{pose}": d[m][:, cols].max(axis=1) for pose, m in (("upright", up), ("fallen", ~up)) if m.any()
                for g, cols in COLUMNS.items() if d.shape[1] > cols.start}


class Gates:
    def __init__(self):
        self.n = {"up": 0, "fallen": 0}
        self.robot_up_max = self.block_up_max = self.fallen_max = 0.0
        self.skipped = 0.0

    def add(self, qpos_pre, q_student, q_teacher, skip=None):
        up, e = group_errors(qpos_pre, np.abs(q_student - q_teacher), skip)
        self.n["up"] += int(up.sum()); self.n["fallen"] += int((~up).sum())
        worst = lambda k: float(e[k].max()) if k in e else 0.0
        self.robot_up_max = max(self.robot_up_max, worst("robot/upright"))
        self.block_up_max = max(self.block_up_max, worst("block/upright"))
        self.fallen_max = max(self.fallen_max, worst("robot/fallen"), worst("block/fallen"))

    def check(self, label, robot_cap=TOL_QPOS, block_cap=TOL_QPOS, fallen_cap=TOL_QPOS):
        """caps: what THIS test's sample may reach (<= the 1e-4 bound); printed values go to the GPU test log"""
        print(f"{label}: upright {self.n['up']} env-steps: robot max {self.robot_up_max:.3g}, block max {self.block_up_max:.3g}; "
              f"fallen {self.n['fallen']}: max {self.fallen_max:.3g}")
        assert max(robot_cap, block_cap, fallen_cap) <= TOL_QPOS
        assert self.robot_up_max < robot_cap, f"G1: robot coordinates {self.robot_up_max:.3g} on an upright env-step (cap {robot_cap:g})"
        assert self.block_up_max < block_cap, f"G2: block coordinates {self.block_up_max:.3g} on an upright env-step (cap {block_cap:g})"
        assert self.fallen_max < fallen_cap, f"G3: fallen robot {self.fallen_max:.3g} (cap {fallen_cap:g})"
