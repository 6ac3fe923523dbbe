"""tests/parity.py itself: the skip rule, the upright rule, the gates, and that forcing, control rounding and the substep
replay do what the parity tests and the campaign tools rely on."""
import numpy as np
import pytest

from tests import parity as P


def test_skip_mask_on_hand_made_outputs():
    """six envs: finished on the student only, on the teacher only, truncated (both), timer NaN on one side, on both, nothing"""
    f, t = False, True
    out = lambda te, tr: (None, None, np.array(te), np.array(tr), None)
    out_s = out([t, f, f, f, f, f], [f, f, t, f, f, f])
    out_t = out([f, t, f, f, f, f], [f, f, t, f, f, f])
    aux_s, aux_t = np.zeros((6, 14)), np.zeros((6, 14))
    aux_s[3, 1] = np.nan
    aux_s[4, 1] = aux_t[4, 1] = np.nan
    assert P.skip_mask(out_s, out_t, aux_s, aux_t).tolist() == [t, t, t, t, f, f]
    # BatchedSim's flags are uint8
    as_u8 = lambda o: (None, None, o[2].astype(np.uint8), o[3].astype(np.uint8), None)
    assert P.skip_mask(as_u8(out_s), out_t, aux_s, aux_t).tolist() == [t, t, t, t, f, f]


def _tilted(deg, axis):
    """qpos [1, 16] with the torso tilted `deg` degrees about x (axis 0) or y (axis 1)"""
    q = np.zeros((1, 16))
    q[0, 3] = np.cos(np.radians(deg) / 2); q[0, 4 + axis] = np.sin(np.radians(deg) / 2)
    q[0, 12] = 1.0
    return q


def test_upright_is_within_60_degrees_of_vertical():
    for axis in (0, 1):
        assert P.upright(_tilted(59, axis))[0] and P.upright(_tilted(-59, axis))[0]
        assert not P.upright(_tilted(61, axis))[0] and not P.upright(_tilted(-61, axis))[0]
    assert P.upright(_tilted(0, 0))[0] and not P.upright(_tilted(180, 1))[0]


def _gates_with_plant(row, col):
    """rows 0, 1 upright, row 2 fallen, row 3 upright with an error of 1.0 but skipped; 5e-5 planted at (row, col)"""
    pre = np.concatenate([_tilted(0, 0), _tilted(30, 1), _tilted(90, 0), _tilted(0, 0)])
    q_t = np.random.default_rng(0).normal(size=(4, 16))
    q_s = q_t.copy()
    q_s[row, col] += 5e-5
    q_s[3, 2] += 1.0
    g = P.Gates()
    g.add(pre, q_s, q_t, skip=np.array([False, False, False, True]))
    return g


@pytest.mark.parametrize("row,col,trips", [(1, 5, "G1"), (1, 13, "G2"), (2, 5, "G3"), (2, 13, "G3")])
def test_gates_attribute_a_planted_error_to_its_group(row, col, trips, capsys):
    g = _gates_with_plant(row, col)
    assert g.n == {"up": 2, "fallen": 1}, "the skipped row does not count"
    got = dict(G1=g.robot_up_max, G2=g.block_up_max, G3=g.fallen_max)
    for k, v in got.items():
        assert v == pytest.approx(5e-5, rel=1e-9) if k == trips else v == 0.0, got
    g.check("loose")   # 5e-5 is inside the 1e-4 bound
    with pytest.raises(AssertionError, match=trips):
        g.check("tight", robot_cap=1e-5, block_cap=1e-5, fallen_cap=1e-5)
    assert "upright 2 env-steps" in capsys.readouterr().out


def test_gates_refuse_a_cap_above_the_bound():
    g = P.Gates()
    g.add(_tilted(0, 0), np.zeros((1, 16)), np.zeros((1, 16)))
    for kw in (dict(robot_cap=2e-4), dict(block_cap=1.1e-4), dict(fallen_cap=1e-3)):
        with pytest.raises(AssertionError):
            g.check("cap above 1e-4", **kw)


def test_gates_without_block_columns():
    g = P.Gates()
    q = np.zeros((2, 9)); d = q.copy(); d[0, 8] = 3e-5; d[1, 0] = 2e-5
    g.add(np.concatenate([_tilted(0, 0), _tilted(90, 1)])[:, :9], d, q)
    assert (g.robot_up_max, g.block_up_max, g.fallen_max) == (3e-5, 0.0, 2e-5)


# ---- env_steps: Env03-v2, 8 envs, 6 steps, episodes of at most 4 steps so that the skip rule fires
def _pair(student_backend):
    kw = dict(seed=5, auto_reset=True, noise=False, max_episode_steps=4)
    t = P.make("oracle", "Env03-v2", 8, **kw)
    s = P.make(student_backend, "Env03-v2", 8, **kw)
    t.reset(); s.reset()
    return t, s


def _kept_errors(teacher, student, steps=6):
    recs = list(P.env_steps(teacher, student, steps, "random", np.random.default_rng(1)))
    assert len(recs) == steps
    assert any(r.skip.any() for r in recs), "the time limit must end episodes within the run"
    return recs, np.concatenate([np.abs(r.post_s[0] - r.post_t[0]).max(axis=1)[~r.skip] for r in recs])


def test_env_steps_oracle_against_itself_is_exact():
    t, s = _pair("oracle")
    recs, e = _kept_errors(t, s)
    assert e.size > 24 and (e == 0.0).all()
    for r in recs:
        for a, b in zip(r.out_s, r.out_t):
            assert np.array_equal(a, b)
        assert r.act.dtype == np.float32 and r.act.shape == (8, 2)
        assert np.array_equal(r.skip, P.skip_mask(r.out_s, r.out_t, r.aux_s, r.aux_t))
    # "random" draws U(-1, 1) once per step and nothing else
    rng = np.random.default_rng(1)
    for r in recs:
        assert np.array_equal(r.act, rng.uniform(-1, 1, size=(8, 2)).astype(np.float32))


def test_env_steps_float_student_stays_within_the_float_tolerance():
    t, s = _pair("host32")
    _, e = _kept_errors(t, s)
    # 2e-3: the maximum tests/test_hostsim_parity.py::test_float_instantiation_within_tolerance allows per env step
    assert e.size > 24 and 0.0 < e.max() < 2e-3, e.max()


class _NoSetState:
    """a student that ignores set_state: teacher-forcing without the forcing"""
    def __init__(self, sim):
        self.sim = sim

    def __getattr__(self, name):
        return getattr(self.sim, name)

    def set_state(self, *a, **kw):
        pass


def test_forcing_is_what_keeps_the_two_together():
    """two oracles on the same seed, the student moved 1 mm along x before the run.  Forced, the first step already starts from
    the teacher's state and every kept error is exactly 0; with set_state dropped the millimetre stays, above 1e-4 from the
    first step on, until the time limit re-draws both sides' episodes from the shared streams (those env-steps are skipped)"""
    def moved():
        t, s = _pair("oracle")
        qpos = s.get_state()[0]
        qpos[:, 0] += 1e-3
        s.set_state(qpos)
        return t, s

    _, e = _kept_errors(*moved())
    assert (e == 0.0).all()
    t, s = moved()
    recs, e = _kept_errors(t, _NoSetState(s))
    for r in recs[:3]:   # episodes of 4 steps: nothing ends before the fourth
        assert not r.skip.any()
        assert (np.abs(r.post_s[0] - r.post_t[0]).max(axis=1) > 1e-4).all()
    assert e.max() > 1e-4


# ---- physics_steps: both sides see the controls in the student's precision
class _Recorder:
    def __init__(self, ctrl_dtype, n=3):
        self.n, self.ctrl_dtype, self.seen = n, ctrl_dtype, []

    def get_state(self):
        return np.zeros((self.n, 9)), np.zeros((self.n, 8)), np.zeros((self.n, 8)), np.zeros(self.n)

    def get_aux(self):
        return np.zeros((self.n, 14))

    def get_xpose(self):
        return np.zeros((self.n, 4)), np.zeros((self.n, 3))

    def set_state(self, *a):
        pass

    set_aux = set_xpose = set_state

    def physics(self, ctrl, nsub):
        self.seen.append((np.array(ctrl), nsub))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_physics_steps_round_controls_to_the_students_precision(dtype):
    teacher, student = _Recorder(np.float64), _Recorder(dtype)
    want = np.random.default_rng(2).uniform(-30, 30, size=(4, 3, 2))
    assert not np.array_equal(want, want.astype(np.float32).astype(np.float64))
    recs = list(P.physics_steps(teacher, student, 4, lambda t, pre: want[t]))
    assert [r.t for r in recs] == [0, 1, 2, 3] and len(student.seen) == 4
    for k, ((cs_, ns), (ct, nt)) in enumerate(zip(student.seen, teacher.seen)):
        assert ns == nt == 250 and np.array_equal(cs_, ct) and np.array_equal(recs[k].ctrl, ct)
        assert np.array_equal(ct, want[k].astype(dtype).astype(np.float64))
        assert np.array_equal(ct, want[k]) == (dtype is np.float64)


# ---- replay_substeps: first-jump detection on scripted velocity differences
class _Scripted(_Recorder):
    """one env whose qvel after substep k is dv(k) in every dof"""
    def __init__(self, dv):
        super().__init__(np.float64, n=1)
        self.dv, self.k = dv, -1

    def set_state(self, *a):
        self.k = -1

    def physics(self, ctrl, nsub):
        assert nsub == 1
        self.k += 1

    def get_state(self):
        return np.zeros((1, 9)), np.full((1, 8), self.dv(self.k)), np.zeros((1, 8)), np.zeros(1)


_PRE = dict(qpos=np.zeros((1, 9)), qvel=np.zeros((1, 8)), warm=np.zeros((1, 8)), time=np.zeros(1))
_LOCATE = dict(jump_abs=1e-3, jump_ratio=20, floor=1e-7)   # tools/parity_locate.py, tools/parity_replay_gpu.py


def test_replay_substeps_finds_the_first_jump():
    calls = []
    first, trace = P.replay_substeps(_Scripted(lambda k: 0.0), _Scripted(lambda k: 1e-9 if k < 17 else 1e-2), _PRE, np.zeros(2),
                                     on_substep=calls.append, **_LOCATE)
    assert first == 17 and len(trace) == 250
    assert trace[16] == (0.0, 1e-9) and trace[17] == (0.0, 1e-2)
    assert calls == list(range(251)), "before every substep, and once after the last"


def test_replay_substeps_steady_growth_is_no_jump():
    first, trace = P.replay_substeps(_Scripted(lambda k: 0.0), _Scripted(lambda k: 1e-9 * 2.0 ** k), _PRE, np.zeros(2), **_LOCATE)
    assert first is None and trace[-1][1] > 1e-3
    # the same growth is a jump for a rule that asks for less than a doubling
    first, _ = P.replay_substeps(_Scripted(lambda k: 0.0), _Scripted(lambda k: 1e-9 * 2.0 ** k), _PRE, np.zeros(2),
                                 jump_abs=1e-3, jump_ratio=1.5, floor=1e-7)
    assert first == 20   # 1e-9 * 2^20 = 1.05e-3


def test_outlier_arrays_and_force_on_a_dump_without_aux():
    pre = dict(qpos=list(range(9)), qvel=[0.5] * 8, warm=[0.0] * 8, time=0.25, ctrl=[1.0, -2.0])
    st = P.outlier_arrays(pre)
    assert st["qpos"].shape == (1, 9) and st["time"].tolist() == [0.25] and st["ctrl"].tolist() == [1.0, -2.0]
    assert "aux" not in st and "action" not in st

    class Student(_Recorder):
        def set_aux(self, *a):
            raise AssertionError("the dump holds no aux")

    assert P.force(Student(np.float64, n=1), st) is st


def test_make_refuses_unknown_names():
    with pytest.raises(TypeError):
        P.make("cuda", "Env01-v2", 1)
    with pytest.raises(TypeError):
        P.make("oracle", "Env01-v2", 1, obs_noise=False)
    o = P.make("oracle", "Env01-v2", 2, block_threads=128)   # launch geometry: for the HIP path alone
    assert (o.n, o.nq, o.nv, o.ctrl_dtype) == (2, 9, 8, np.float64)
    o.close()
    h = P.make("host32", "Env03-v2", 2)
    assert (h.n, h.nq, h.nv, h.ctrl_dtype) == (2, 16, 14, np.float64)
    h.close()


@pytest.mark.gpu
def test_hip_adapter_returns_arrays_the_caller_owns():
    """Env03-v2, N = 65 (one full wave and a partial one), two steps"""
    n = 65
    a, b = P.make("hip", "Env03-v2", n, seed=3, auto_reset=True), P.make("hip", "Env03-v2", n, seed=3, auto_reset=True)
    assert a.ctrl_dtype is np.float32 and (a.n, a.nq, a.nv) == (n, 16, 14)
    obs = a.reset()
    assert isinstance(obs, np.ndarray) and np.array_equal(obs, b.raw.reset().cpu().numpy())
    rng = np.random.default_rng(0)
    first = a.step(rng.uniform(-1, 1, size=(n, 2)).astype(np.float32))
    kept = [x.copy() for x in first]
    second = a.step(rng.uniform(-1, 1, size=(n, 2)).astype(np.float32))
    for x, y in zip(first, kept):
        assert np.array_equal(x, y), "the first step's arrays are the caller's"
    assert not np.array_equal(first[0], second[0])
    assert first[2].dtype == bool and first[3].dtype == bool
    assert [x.shape for x in first] == [(n, 6), (n,), (n,), (n,), (n, 6)]
    a.close(); b.close()
