"""Poisoned inputs for the bad-state guard, shared by tests/test_bad_state_cpu.py (the oracle and the kernel source on the host)
and tests/test_bad_state_gpu.py (the HIP path): one NaN / Inf / out-of-range value in one field of one lane, between healthy
neighbours.  The contract, for one env step:

 1. any stored coordinate of qpos or qvel bad (NaN or |x| > 1e10, MuJoCo's mju_isBad) at the start of the step, or a NaN action
    component -> the lane is reset during the step: bad count +1, elapsed 1, time 0;
 2. +-Inf and huge finite actions are not bad (the servo force is clamped);
 3. a bad qacc_warmstart alone, or a bad friction coefficient alone (Env02), is not bad;
 4. obs, terminal_obs, reward and every column of the state, the accessor pose and aux (but the "no block timer" NaN and, in
    case 3, the poisoned field itself) are finite on the poisoned step and ever after, and the bad count does not move again;
    the reward of a guard reset whose pre-step reward was not finite is 0;
 5. healthy lanes are bit-identical to a control run without poison.

The expected verdict comes from `expect_reset` below -- a numpy predicate over what the simulator stores, independent of the
oracle and of the kernel.  Test infrastructure."""
import numpy as np

NAN, INF = float("nan"), float("inf")
STATE_VALUES = (NAN, INF, -INF, 1e12, -1e12)
ACTION_VALUES = (NAN, INF, -INF, 3e38, -3e38, 1e30)
FRICTION_VALUES = (NAN, INF)         # Env02-v1: aux column 10
ENV_IDS = ("Env01-v1", "Env01-v2", "Env01-v3", "Env02-v1", "Env03-v1", "Env03-v2")
SEED, CLEAN_STEPS, MORE_STEPS = 3, 2, 20
AUX_TIMER, AUX_ELAPSED, AUX_RNG, AUX_SIDE, AUX_RETURN, AUX_BAD, AUX_CTRL, AUX_FRICTION = 1, 2, 3, 4, 6, 7, slice(8, 10), 10


def _vname(v):
    return "nan" if np.isnan(v) else ("%+g" % v).replace("+inf", "+Inf").replace("-inf", "-Inf")


def cases(env_id):
    """-> [(name, field, column, value)], field in qpos / qvel / warm / action / friction"""
    blk = env_id.startswith("Env03")
    nq, nv = (16, 14) if blk else (9, 8)
    out = [(f"{field}[{c}]={_vname(v)}", field, c, v)
           for field, ncol in (("qpos", nq), ("qvel", nv), ("warm", nv)) for c in range(ncol) for v in STATE_VALUES]
    out += [(f"action[{c}]={_vname(v)}", "action", c, v) for c in range(2) for v in ACTION_VALUES]
    if env_id == "Env02-v1":
        out += [(f"friction={_vname(v)}", "friction", AUX_FRICTION, v) for v in FRICTION_VALUES]
    return out


def is_bad(x):
    """MuJoCo's mju_isBad"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.isnan(x) | (np.abs(x) > 1e10)


def expect_reset(qpos, qvel, actions):
    """the contract's verdict per lane, from the STORED qpos / qvel (get_state() after the poison went in: set_state may have
    normalised a quaternion) and the actions of the step"""
    return is_bad(qpos).any(axis=1) | is_bad(qvel).any(axis=1) | np.isnan(np.asarray(actions, dtype=np.float64)).any(axis=1)


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.array(x, copy=True)


class Run:
    """a batch taken through reset, the clean steps, ONE poisoned step and MORE_STEPS zero-action steps; everything recorded"""

    def __init__(self, sim, env_id, stride=2, n=None, poisoned=True):
        self.env_id, self.cases = env_id, cases(env_id)
        self.lanes = np.array([stride * k + 1 for k in range(len(self.cases))])
        self.n = n if n is not None else stride * len(self.cases) + 2
        assert self.n > self.lanes[-1] + 1 and stride >= 2
        self.healthy = np.ones(self.n, bool)
        self.healthy[self.lanes] = False
        zero = np.zeros((self.n, 2), np.float32)
        sim.reset()
        for _ in range(CLEAN_STEPS):
            sim.step(zero)
        qpos, qvel, warm, _ = sim.get_state()
        aux = sim.get_aux()
        actions = zero.copy()
        if poisoned:
            for lane, (_, field, col, val) in zip(self.lanes, self.cases):
                dict(qpos=qpos, qvel=qvel, warm=warm, action=actions, friction=aux)[field][lane, col] = val
        sim.set_state(qpos=qpos, qvel=qvel, warm=warm)  # (the control run takes the same round trip)
        if env_id == "Env02-v1":
            sim.set_aux(aux)
        self.start = [_np(a) for a in sim.get_state()]
        self.aux0 = sim.get_aux()
        self.expected = expect_reset(self.start[0], self.start[1], actions)
        self.steps = []
        for k in range(1 + MORE_STEPS):
            obs, rew, term, trunc, tobs = (_np(a) for a in sim.step(actions if k == 0 else zero))
            qpos, qvel, warm, time = sim.get_state()
            xq, xp = sim.get_xpose()
            self.steps.append(dict(obs=obs, reward=rew, terminated=term.astype(bool), truncated=trunc.astype(bool), terminal_obs=tobs,
                                   qpos=qpos, qvel=qvel, warm=warm, time=time, xquat=xq, xpos=xp, aux=sim.get_aux()))

    def case_rows(self):
        return zip(self.lanes, self.cases)


def check_contract(run, who):
    """items 1-4 on every lane of a poisoned run; `who` names the simulator in the messages"""
    first = run.steps[0]
    dbad = first["aux"][:, AUX_BAD] - run.aux0[:, AUX_BAD]
    names = {int(lane): name for lane, (name, *_) in run.case_rows()}
    label = lambda i: f"{who} {run.env_id} lane {i} ({names.get(int(i), 'healthy')})"
    wrong = np.flatnonzero(dbad != run.expected)
    assert wrong.size == 0, "guard verdict differs from the predicate:\n" + "\n".join(
        f"  {label(i)}: expected {int(run.expected[i])}, bad count moved by {dbad[i]:g}" for i in wrong)
    assert not run.expected[run.healthy].any()
    rs = np.flatnonzero(run.expected)
    # a reset pose is drawn over the whole circle of pitch: where it lies beyond the 50 degree limit the same step also terminates and
    # auto-resets (elapsed 0, return 0); everywhere else the new episode is one step old and its return is this step's reward (0
    # where the pre-step reward was not finite)
    done = first["terminated"][rs] | first["truncated"][rs]
    assert not done.all()
    for key, got, want in (("elapsed", first["aux"][rs, AUX_ELAPSED], np.where(done, 0, 1)), ("time", first["time"][rs], 0 * rs),
                           ("return", first["aux"][rs, AUX_RETURN].astype(np.float32), np.where(done, np.float32(0), first["reward"][rs]))):
        assert np.array_equal(got, want), f"{key} after a guard reset: " + ", ".join(
            f"{label(i)}: {g:g}, expected {w:g}" for i, g, w in zip(rs, got, want) if g != w)
    # item 4.  Not required finite: the block timer's "None"; in case 3 the poisoned field itself (the warm start of that lane, its
    # friction coefficient); on the poisoned step aux 8:10 of a poisoned lane, the oracle's echo of the data.ctrl = qvel + 4 action
    # it was handed (the kernel leaves these two columns unused)
    for k, st in enumerate(run.steps):
        mask = {key: np.isfinite(st[key]) for key in st if st[key].dtype.kind == "f"}
        mask["aux"][:, AUX_TIMER] = True
        for lane, (_, field, col, _v) in run.case_rows():
            if field == "warm":
                mask["warm"][lane] = True
            elif field == "friction":
                mask["aux"][lane, col] = True
            if k == 0:
                mask["aux"][lane, AUX_CTRL] = True
        for key, m in mask.items():
            rows = np.flatnonzero(~m.reshape(run.n, -1).all(axis=1))
            assert rows.size == 0, f"step {k}: non-finite {key}: " + ", ".join(f"{label(i)}: {st[key][i]}" for i in rows[:8])
        assert np.array_equal(st["aux"][:, AUX_BAD], first["aux"][:, AUX_BAD]), \
            f"step {k}: the bad count moved again: " + ", ".join(label(i) for i in np.flatnonzero(st["aux"][:, AUX_BAD] != first["aux"][:, AUX_BAD]))


def check_action_reward_kept(run, control):
    """item 4, last sentence: the reward of a NaN-action step was computed on a healthy state and is kept"""
    for lane, (name, field, _c, _v) in run.case_rows():
        if field == "action":
            assert run.steps[0]["reward"][lane] == control.steps[0]["reward"][lane], name


def check_healthy_identical(run, control, who):
    """item 5: healthy lanes bit-identical to the control run, outputs, state and aux, on every recorded step"""
    h = run.healthy
    for a, b in zip(run.start, control.start):
        assert np.array_equal(a[h], b[h]), f"{who} {run.env_id}: the runs do not start from the same state"
    for k, (st, ct) in enumerate(zip(run.steps, control.steps)):
        for key in st:
            assert np.array_equal(st[key][h], ct[key][h], equal_nan=(key == "aux")), \
                f"{who} {run.env_id} step {k}: {key} of healthy lanes {np.flatnonzero(h)[np.flatnonzero((st[key][h] != ct[key][h]).reshape(h.sum(), -1).any(axis=1))][:8]} differs from the control run"


def check_reset_matches_oracle(run, oracle_run, who):
    """a guard reset draws what any reset draws: obs of the poisoned step within the suite's tolerance for reset observations
    (tests/test_gpu_parity.py: shared_rng_parity), elapsed / RNG counter / attack side exactly the oracle's"""
    rs = np.flatnonzero(run.expected & oracle_run.expected)
    assert rs.size > 0
    a, b = run.steps[0], oracle_run.steps[0]
    np.testing.assert_allclose(a["obs"][rs], b["obs"][rs], atol=2e-5, rtol=1e-5, err_msg=f"{who} {run.env_id} lanes {rs}")
    cols = slice(AUX_ELAPSED, AUX_SIDE + 1)
    assert np.array_equal(a["aux"][rs, cols], b["aux"][rs, cols]), \
        f"{who} {run.env_id}: lanes {rs[(a['aux'][rs, cols] != b['aux'][rs, cols]).any(axis=1)]} drew differently from the oracle"
