"""What the CPU and the GPU tests of the NaN rule share (tests/test_nonfinite_cpu.py, tests/test_nonfinite_gpu.py):
the poison tables, classes(), the two checks on plain arrays, and the cases themselves, written once against a `run` object that is
the host builds in one file and the HIP kernels in the other.

The rule: a NaN that the fp64 reference reports must not come back as a finite number, and an unpoisoned row must not notice its
neighbour.  Every case is conditioned CLEAN by the helper its family already has (the conditioning loops never see a NaN), then one
value per poisoned row is planted on a copy.

Forward calls -- check_forward, per output: every element is NaN, +inf, -inf or finite as the fp64 reference of the same inputs is
(ref_offpolicy, ref_td3, ref_sac); finite elements meet offpolicy_cases.gate; every unpoisoned element has the bytes of the same call
on the clean case.  One departure, kept on purpose (brs_offpolicy.hpp: td_combine): a row with done != 0 returns its reward bit for
bit, where the references compute 0 * NaN for a poisoned next_obs or target network; the expected y is where(done, reward,
reference), built here.

Gradient calls -- check_gradient_nans: every element of the buffer, statistics included, that is NaN in the fp64 torch-autograd
reference of the poisoned case is NaN in the buffer; NaN where the reference is finite are counted and printed, not gated.  Before
that, reference_reaches asserts on the reference alone that the poison reaches what it can reach, so that no case passes vacuously:
NaN in obs -> every parameter block and every loss; NaN in y or in act -> every block of the critic(s) and their loss(es) (the mean-Q
statistic does not depend on y); NaN in adv or logp_old -> every block of the actor, log_std and the policy loss (the value tower does
not see them).  The entropy, the clip fraction and alpha do not depend on a row's data and stay finite in the reference."""
import numpy as np
import torch

import a2c_cases as AC
import ddpg_learner_cases as DC
import learner_cases as LC
import offpolicy_cases as OC
import ref_a2c as A
import ref_ddpg_learner as RL
import ref_learner as PL
import ref_offpolicy as R
import ref_sac as S
import ref_td3 as T3
import sac_cases as SC
import td3_cases as TC

NAN, INF = np.float32("nan"), np.float32("inf")
SEED, GAMMA = OC.SEED, OC.GAMMA
NA, NC, SNA = R.NACTOR, R.NCRITIC, S.NACTOR

# ---- the poison tables
FORWARD_N = 129                          # workgroup 0 full, workgroup 1 with a lone row in a partial wave
FORWARD_ROWS = (0, 31, 32, 127, 128)     # first and last row of a 32-row wave tile, last row of a workgroup, the lone row
OBS_POISONS = ((0, NAN), (5, NAN), (2, INF), (3, -INF))   # (column, value); column 5 comes from the upper half of the wave
ROTATIONS = (0, 1, 2, 3)                 # poisoned row j takes OBS_POISONS[(j + rotation) % 4]: every row meets every poison
SMALL_N, SMALL_ROWS = 33, (32,)          # a second wave tile of one row
WEIGHT_VALUES = (NAN, INF, -INF)
SIGMAS = (0.0, 0.1)
POLICY_NOISE = TC.SB3_NOISE              # (0.2, 0.5)
OFFPOLICY_GRAD_M = (129, 513)            # below the split threshold; two partial rows, the poisoned sample alone in the second
ONPOLICY_M, ONPOLICY_WG = 257, 2         # a second chunk of one row, on its own workgroup

FINITE, ISNAN, POSINF, NEGINF = 0, 1, 2, 3


def classes(x):
    """per element: 0 finite, 1 NaN, 2 +inf, 3 -inf"""
    x = np.asarray(x)
    return np.where(np.isnan(x), ISNAN, np.where(x == np.inf, POSINF, np.where(x == -np.inf, NEGINF, FINITE))).astype(np.int8)


def check_forward(what, out, ref, clean, untouched):
    """out: the call on the poisoned case; ref: fp64 on the same inputs; clean: the same call on the clean case; untouched: a boolean
    mask (broadcast to out's shape) of the elements the poison cannot reach"""
    out, ref, clean = np.asarray(out), np.asarray(ref, np.float64), np.asarray(clean)
    assert out.shape == ref.shape == clean.shape, (what, out.shape, ref.shape, clean.shape)
    got, want = classes(out), classes(ref)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} of {out.size} elements are of another class than fp64; first at {tuple(bad[0])}: "
                           f"{out[tuple(bad[0])]!r} where fp64 has {ref[tuple(bad[0])]!r}")
    finite = want == FINITE
    if finite.any():
        OC.gate(out[finite], ref[finite], what)
    keep = np.broadcast_to(untouched, out.shape)
    same = out.view(np.uint32) == clean.view(np.uint32) if out.dtype == np.float32 else out == clean
    changed = np.argwhere(keep & ~same)
    assert changed.size == 0, f"{what}: {len(changed)} unpoisoned elements differ from the clean run; first at {tuple(changed[0])}"
    return int((want != FINITE).sum())


def check_gradient_nans(what, g, g64):
    """-> the number of NaN in g where the reference is finite (printed, not gated)"""
    g, g64 = np.asarray(g), np.asarray(g64)
    assert g.shape == g64.shape, (what, g.shape, g64.shape)
    want, have = np.isnan(g64), np.isnan(g)
    missing = np.flatnonzero(want & ~have)
    extra = int((have & ~want).sum())
    print(f"{what}: fp64 reports {int(want.sum())} NaN among {g.size} elements; the buffer holds {int(have.sum())}, {extra} of them where fp64 is finite")
    assert missing.size == 0, (f"{what}: {missing.size} elements are NaN in fp64 and a number in the buffer; first: element {missing[0]} = "
                               f"{g[missing[0]]!r}")
    return extra


def reference_reaches(what, g64, places, need):
    """places: {name: slice or index into the buffer}; every name in `need` holds at least one NaN in the fp64 reference"""
    g64 = np.asarray(g64)
    for name in need:
        assert np.isnan(g64[places[name]]).any(), f"{what}: the poison does not reach {name} in the fp64 reference: the case proves nothing"


def rows_mask(n, rows):
    """[n][1]: True where the row is not poisoned"""
    m = np.ones((n, 1), bool)
    m[list(rows)] = False
    return m


def poison_obs(obs, rows, rotation):
    out = obs.copy()
    for j, row in enumerate(rows):
        col, val = OBS_POISONS[(j + rotation) % len(OBS_POISONS)]
        out[row, col] = val
    return out


def _ref(f, *args, **kw):
    """a reference on poisoned inputs: numpy's warnings off, and torch.distributions' argument validation off (Normal refuses a NaN
    mean before it computes anything; without the check it is the same arithmetic, and the NaN goes through it)"""
    validate = torch.distributions.Distribution._validate_args
    torch.distributions.Distribution.set_default_validate_args(False)
    try:
        with np.errstate(all="ignore"):
            return f(*args, **kw)
    finally:
        torch.distributions.Distribution.set_default_validate_args(validate)


def _where_done(done, reward, y64):
    return np.where(np.asarray(done) != 0, np.asarray(reward, np.float64), y64)


def _compare(what, names, got, ref, clean, masks):
    total = 0
    for name, g, r, c, m in zip(names, got, ref, clean, masks):
        total += check_forward(f"{what} {name}", g, r, c, m)
    return total


# ------------------------------------------------------------------------------------------------ forwards: poisoned rows
def ddpg_rows(run, n, rows, rotation):
    """brs_ddpg_act at both sigmas, brs_ddpg_q (obs poisons, then NaN in act[1]) and brs_ddpg_td_target on `rows` of n"""
    c = OC.conditioned(n, "init")
    obs_p, keep, all_rows = poison_obs(c["obs"], rows, rotation), rows_mask(n, rows), np.ones((n, 1), bool)
    step, nonfinite = 3, 0
    for sigma in SIGMAS:
        clean, got = run.act(c["actor"], c["obs"], step, sigma), run.act(c["actor"], obs_p, step, sigma)
        ref = _ref(R.act, c["actor"], obs_p, SEED, 0, step, sigma)
        nonfinite += _compare(f"act n={n} rotation={rotation} sigma={sigma}", ("action", "mean", "noise"), got, ref, clean, (keep, keep, all_rows))
    clean_q = run.q(c["critic"], c["obs"], c["act"])
    nonfinite += check_forward(f"q n={n} rotation={rotation}", run.q(c["critic"], obs_p, c["act"]), _ref(R.critic, c["critic"], obs_p, c["act"]), clean_q, keep[:, 0])
    act_p = c["act"].copy()
    act_p[list(rows), 1] = NAN
    nonfinite += check_forward(f"q n={n} NaN in act[1]", run.q(c["critic"], c["obs"], act_p), _ref(R.critic, c["critic"], c["obs"], act_p), clean_q, keep[:, 0])
    clean_y = run.td_target(c["actor"], c["critic"], c["obs"], c["reward"], c["done"], GAMMA)
    y64 = _ref(R.td_target, c["actor"], c["critic"], obs_p, c["reward"], c["done"], GAMMA)
    nonfinite += check_forward(f"td_target n={n} rotation={rotation}", run.td_target(c["actor"], c["critic"], obs_p, c["reward"], c["done"], GAMMA),
                               _where_done(c["done"], c["reward"], y64), clean_y, keep[:, 0])
    assert nonfinite > 0
    return nonfinite


def reward_and_done_poisons(next_obs, reward, done, rows):
    """NaN in reward and NaN in next_obs, each once with done = 0 and once with done = 1, on the first four of `rows`"""
    no, rw, dn = next_obs.copy(), reward.copy(), done.copy()
    r = list(rows[:4])
    rw[r[0]], dn[r[0]] = NAN, 0
    rw[r[1]], dn[r[1]] = NAN, 1
    no[r[2], 0], dn[r[2]] = NAN, 0
    no[r[3], 0], dn[r[3]] = NAN, 1
    return no, rw, dn, r


def _target_rows(what, call, ref_call, c, rows, rotation, names):
    """call(next_obs, reward, done) -> outputs, y first; ref_call likewise in fp64.  The obs rotation, then the reward / done table"""
    n = len(c["next_obs"])
    keep, all_rows = rows_mask(n, rows), np.ones((n, 1), bool)
    clean = call(c["next_obs"], c["reward"], c["done"])

    def masks(outs):   # the noise is the row's Philox block: it reads no input, so every row of it is untouched
        per_row = [all_rows if name == "noise" else keep for name in names]
        return [m[:, 0] if o.ndim == 1 else m for m, o in zip(per_row, outs)]
    nonfinite = 0
    obs_p = poison_obs(c["next_obs"], rows, rotation)
    got, ref = call(obs_p, c["reward"], c["done"]), list(_ref(ref_call, obs_p, c["reward"], c["done"]))
    ref[0] = _where_done(c["done"], c["reward"], ref[0])
    nonfinite += _compare(f"{what} rotation={rotation}", names, got, ref, clean, masks(got))
    if rotation == 0 and len(rows) >= 4:
        no, rw, dn, r = reward_and_done_poisons(c["next_obs"], c["reward"], c["done"], rows)
        got, ref = call(no, rw, dn), list(_ref(ref_call, no, rw, dn))
        ref[0] = _where_done(dn, rw, ref[0])
        # what the table asks for, on the expected values themselves: a NaN reward comes back as NaN with either done; a NaN
        # next_obs is a NaN y with done = 0 and the reward, bit for bit, with done = 1
        assert np.isnan(ref[0][r[0]]) and np.isnan(ref[0][r[1]]) and np.isnan(ref[0][r[2]]) and ref[0][r[3]] == np.float64(rw[r[3]])
        nonfinite += _compare(f"{what} reward / next_obs x done", names, got, ref, clean, masks(got))
        assert got[0][r[3]].tobytes() == rw[r[3]].tobytes()
    assert nonfinite > 0
    return nonfinite


def ddpg_target_table(run, n, rows):
    c = OC.conditioned(n, "init")
    case = dict(next_obs=c["obs"], reward=c["reward"], done=c["done"])
    return _target_rows(f"td_target n={n}", lambda no, rw, dn: (run.td_target(c["actor"], c["critic"], no, rw, dn, GAMMA),),
                        lambda no, rw, dn: (R.td_target(c["actor"], c["critic"], no, rw, dn, GAMMA),), case, rows, 0, ("y",))


def td3_rows(run, n, rows, rotation):
    c = TC.target_case(n, "init", POLICY_NOISE)
    pn, nc = POLICY_NOISE
    return _target_rows(f"td3_target n={n}", lambda no, rw, dn: run.td3_target(c["actor"], c["critics"], no, rw, dn, GAMMA, pn, nc, 0),
                        lambda no, rw, dn: T3.td3_target(c["actor"], c["critics"], no, rw, dn, GAMMA, pn, nc, SEED, 0), c, rows, rotation,
                        ("y", "next_action", "noise"))


def sac_act_rows(run, n, rows, rotation):
    c = SC.act_case(n, "init")
    obs_p, keep, all_rows = poison_obs(c["obs"], rows, rotation), rows_mask(n, rows), np.ones((n, 1), bool)
    nonfinite = 0
    for det in (False, True):
        clean, got = run.sac_act(c["actor"], c["obs"], c["step"], det), run.sac_act(c["actor"], obs_p, c["step"], det)
        ref = _ref(S.act, c["actor"], obs_p, SEED, 0, c["step"], deterministic=det)
        nonfinite += _compare(f"sac_act n={n} rotation={rotation} deterministic={int(det)}", ("action", "mu", "log_std", "noise"), got, ref, clean,
                              (keep, keep, keep, all_rows))
    assert nonfinite > 0
    return nonfinite


def sac_target_rows(run, n, rows, rotation):
    c = SC.target_case(n, "init")
    return _target_rows(f"sac_target n={n}", lambda no, rw, dn: run.sac_target(c["actor"], c["critics"], no, rw, dn, GAMMA, c["draw"]),
                        lambda no, rw, dn: S.sac_target(c["actor"], c["critics"], no, rw, dn, GAMMA, SEED, c["draw"]), c, rows, rotation,
                        ("y", "next_action", "logp", "noise"))


# ------------------------------------------------------------------------------------------------ forwards: poisoned weights
def _planted(vector, index, value):
    out = vector.copy()
    out[index] = value
    return out


def ddpg_actor_bias(run, value, sigma, n=SMALL_N):
    """actor b3[0] = NaN: column 0 of every row is NaN, column 1 has the clean run's bytes; +-inf: the action is +-1 through tanh_"""
    c = OC.conditioned(n, "init")
    actor_p = _planted(c["actor"], NA - 2, value)
    col1, everything = np.array([[False, True]]), np.ones((1, 2), bool)
    clean, got = run.act(c["actor"], c["obs"], 3, sigma), run.act(actor_p, c["obs"], 3, sigma)
    ref = _ref(R.act, actor_p, c["obs"], SEED, 0, 3, sigma)
    _compare(f"act b3[0]={value} sigma={sigma}", ("action", "mean", "noise"), got, ref, clean, (col1, col1, everything))
    if np.isnan(value):
        assert np.isnan(got[0][:, 0]).all() and np.isnan(got[1][:, 0]).all()
    else:
        assert np.all(got[1][:, 0] == np.sign(value)) and (sigma > 0 or np.all(got[0][:, 0] == np.sign(value)))
    # the same actor as the target actor: every row that bootstraps is NaN, a done row is its reward
    clean_y = run.td_target(c["actor"], c["critic"], c["obs"], c["reward"], c["done"], GAMMA)
    y64 = _where_done(c["done"], c["reward"], _ref(R.td_target, actor_p, c["critic"], c["obs"], c["reward"], c["done"], GAMMA))
    check_forward(f"td_target actor' b3[0]={value}", run.td_target(actor_p, c["critic"], c["obs"], c["reward"], c["done"], GAMMA), y64, clean_y, c["done"] != 0)
    assert not np.isnan(value) or np.isnan(y64[c["done"] == 0]).all()


def sac_actor_bias(run, which, value, det, n=SMALL_N):
    """which 0: the bias of mu[0]; which 2: the bias of log_std[0], where torch.clamp gives NaN, 2 and -20"""
    c = SC.act_case(n, "init")
    actor_p = _planted(c["actor"], SNA - 4 + which, value)
    col1, everything = np.array([[False, True]]), np.ones((1, 2), bool)
    clean, got = run.sac_act(c["actor"], c["obs"], c["step"], det), run.sac_act(actor_p, c["obs"], c["step"], det)
    ref = _ref(S.act, actor_p, c["obs"], SEED, 0, c["step"], deterministic=det)
    if which == 0:
        masks = (col1, col1, everything, everything)
    else:   # the deterministic action does not read log_std
        masks = (everything if det else col1, everything, col1, everything)
    _compare(f"sac_act b3[{which}]={value} deterministic={int(det)}", ("action", "mu", "log_std", "noise"), got, ref, clean, masks)
    if which == 2:
        want = {"nan": np.nan, "inf": S.LOG_STD_MAX, "-inf": S.LOG_STD_MIN}[repr(float(value))]
        assert np.array_equal(got[2][:, 0].astype(np.float64), np.full(n, want), equal_nan=True)


def target_critic_bias(run, n=SMALL_N):
    """b3 of target critic 1 = NaN in the TD3 and the SAC target, and log_ent_coef = NaN in the SAC target: every row with done == 0 is
    NaN, a done row keeps its reward's bytes, and nothing else moves"""
    pn, nc = POLICY_NOISE
    c = TC.target_case(n, "init", POLICY_NOISE)
    critics_p = _planted(c["critics"], 2 * NC - 1, NAN)
    ended = c["done"] != 0
    assert ended.any() and (~ended).any()
    clean = run.td3_target(c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, pn, nc, 0)
    got = run.td3_target(c["actor"], critics_p, c["next_obs"], c["reward"], c["done"], GAMMA, pn, nc, 0)
    ref = list(_ref(T3.td3_target, c["actor"], critics_p, c["next_obs"], c["reward"], c["done"], GAMMA, pn, nc, SEED, 0))
    ref[0] = _where_done(c["done"], c["reward"], ref[0])
    assert np.isnan(ref[0][~ended]).all()
    _compare("td3_target critic 1' b3=nan", ("y", "next_action", "noise"), got, ref, clean, (ended, np.ones((1, 2), bool), np.ones((1, 2), bool)))
    c = SC.target_case(n, "init")
    ended = c["done"] != 0
    clean = run.sac_target(c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, c["draw"])
    for what, actor_p, critics_p in (("critic 1' b3=nan", c["actor"], _planted(c["critics"], 2 * NC - 1, NAN)),
                                     ("log_ent_coef=nan", _planted(c["actor"], SNA, NAN), c["critics"])):
        got = run.sac_target(actor_p, critics_p, c["next_obs"], c["reward"], c["done"], GAMMA, c["draw"])
        ref = list(_ref(S.sac_target, actor_p, critics_p, c["next_obs"], c["reward"], c["done"], GAMMA, SEED, c["draw"]))
        ref[0] = _where_done(c["done"], c["reward"], ref[0])
        assert np.isnan(ref[0][~ended]).all()
        _compare(f"sac_target {what}", ("y", "next_action", "logp", "noise"), got, ref, clean,
                 (ended, np.ones((1, 2), bool), np.ones(1, bool), np.ones((1, 2), bool)))


# ------------------------------------------------------------------------------------------------ gradients
def _blocks(sizes, offset=0):
    return {k: slice(v.start + offset, v.stop + offset) for k, v in RL.block_slices(sizes).items()}


CRITIC_PLACES = {**_blocks(R.CRITIC_SIZES), "loss": NC, "mean_q": NC + 1}
ACTOR_PLACES = {**_blocks(R.ACTOR_SIZES), "loss": NA, "mean_a2": NA + 1}
TWIN_PLACES = {**{f"0.{k}": v for k, v in _blocks(R.CRITIC_SIZES).items()}, **{f"1.{k}": v for k, v in _blocks(R.CRITIC_SIZES, NC).items()},
               "loss0": 2 * NC, "mean_q0": 2 * NC + 1, "loss1": 2 * NC + 2, "mean_q1": 2 * NC + 3}
SAC_ACTOR_PLACES = {**_blocks(S.ACTOR_SIZES), "log_ent_coef": SNA, "loss": SNA + 1, "mean_logp": SNA + 2, "mean_qmin": SNA + 3, "ent_coef": SNA + 4}
ONPOLICY_PLACES = {**PL.block_slices(), "policy_loss": PL.NPARAM, "value_loss": PL.NPARAM + 1, "entropy": PL.NPARAM + 2, "kl": PL.NPARAM + 3,
                   "clipfrac": PL.NPARAM + 4}
_W = ("W1", "b1", "W2", "b2", "W3", "b3")
CRITIC_NEED = {"obs": _W + ("loss", "mean_q"), "y": _W + ("loss",), "act": _W + ("loss", "mean_q")}
TWIN_NEED = {k: tuple(f"{i}.{b}" for i in (0, 1) for b in _W) + tuple(s + str(i) for i in (0, 1) for s in v[6:]) for k, v in CRITIC_NEED.items()}
ACTOR_NEED = _W + ("loss", "mean_a2")
SAC_ACTOR_NEED = _W + ("log_ent_coef", "loss", "mean_logp", "mean_qmin")
_PI = tuple(PL.ACTOR_BLOCKS)
PPO_NEED = {"obs": tuple(n for n, _ in PL.BLOCKS) + ("policy_loss", "value_loss", "kl"), "adv": _PI + ("policy_loss",),
            "logp_old": _PI + ("policy_loss", "kl")}
A2C_NEED = {"obs": tuple(n for n, _ in PL.BLOCKS) + ("policy_loss", "value_loss"), "adv": _PI + ("policy_loss",)}


def critic_poisons(c, row):
    """-> [(name, obs, act, y)]: NaN in obs[0], in y, in act[1] of `row`, each on a copy"""
    out = []
    for name, key, index in (("obs", "obs", (row, 0)), ("y", "y", row), ("act", "act", (row, 1))):
        p = {k: c[k] for k in ("obs", "act", "y")}
        p[key] = _planted(c[key], index, NAN)
        out.append((name, p["obs"], p["act"], p["y"]))
    return out


def offpolicy_gradients(run, m):
    """the five off-policy gradient calls at m rows, row m - 1 poisoned: the poisoned cases first (so that the clean run that follows
    must not read what they left), then the clean case at its existing gates"""
    row = m - 1
    c, t, s = DC.learner_case(m, "init"), TC.twin_case(m, "init"), SC.grad_case(m, "init")
    for name, obs, act, y in critic_poisons(c, row):
        what, g64 = f"critic_grad m={m} NaN in {name}", _ref(RL.critic_grad, c["critic"], obs, act, y)
        reference_reaches(what, g64, CRITIC_PLACES, CRITIC_NEED[name])
        check_gradient_nans(what, run.critic_grad(c["critic"], obs, act, y), g64)
    for name, obs, act, y in critic_poisons(t, row):
        what, g64 = f"twin_critic_grad m={m} NaN in {name}", _ref(T3.twin_critic_grad, t["critics"], obs, act, y)
        reference_reaches(what, g64, TWIN_PLACES, TWIN_NEED[name])
        check_gradient_nans(what, run.twin_critic_grad(t["critics"], obs, act, y), g64)
    for name, obs, act, y in critic_poisons(s, row):
        what, g64 = f"sac_twin_critic_grad m={m} NaN in {name}", _ref(S.twin_critic_grad, s["critics"], obs, act, y)
        reference_reaches(what, g64, TWIN_PLACES, TWIN_NEED[name])
        check_gradient_nans(what, run.sac_twin_critic_grad(s["critics"], obs, act, y), g64)
    obs_p = _planted(c["obs"], (row, 0), NAN)
    what, g64 = f"actor_grad m={m} NaN in obs", _ref(RL.actor_grad, c["actor"], c["critic"], obs_p)
    reference_reaches(what, g64, ACTOR_PLACES, ACTOR_NEED)
    check_gradient_nans(what, run.actor_grad(c["actor"], c["critic"], obs_p), g64)
    obs_p = _planted(s["obs"], (row, 0), NAN)
    what, g64 = f"sac_actor_grad m={m} NaN in obs", _ref(S.actor_grad, s["actor"], s["critics"], obs_p, SEED, s["draw"], True, SC.TARGET_ENTROPY)
    reference_reaches(what, g64, SAC_ACTOR_PLACES, SAC_ACTOR_NEED)
    check_gradient_nans(what, run.sac_actor_grad(s["actor"], s["critics"], obs_p, s["draw"]), g64)
    # ---- the clean cases, after the poisoned ones, at the gates their own tests hold them to
    c64, a64, c32, a32 = DC.references(m, "init")
    DC.check_gradient(f"m={m} critic", run.critic_grad(c["critic"], c["obs"], c["act"], c["y"]), c64, c32, R.CRITIC_SIZES, OC.gate)
    DC.check_gradient(f"m={m} actor", run.actor_grad(c["actor"], c["critic"], c["obs"]), a64, a32, R.ACTOR_SIZES, OC.gate)
    t64, t32 = TC.twin_references(m, "init")
    g = run.twin_critic_grad(t["critics"], t["obs"], t["act"], t["y"])
    for k, (gk, rk, fk) in enumerate(zip(TC.split_twin(g), TC.split_twin(t64), TC.split_twin(t32))):
        DC.check_gradient(f"m={m} twin critic {k}", gk, rk, fk, R.CRITIC_SIZES, OC.gate)
    s64 = S.twin_critic_grad(s["critics"], s["obs"], s["act"], s["y"])
    s32 = S.twin_critic_grad(s["critics"], s["obs"], s["act"], s["y"], torch.float32)
    g = run.sac_twin_critic_grad(s["critics"], s["obs"], s["act"], s["y"])
    for k, (gk, rk, fk) in enumerate(zip(TC.split_twin(g), TC.split_twin(s64), TC.split_twin(s32))):
        DC.check_gradient(f"m={m} SAC twin critic {k}", gk, rk, fk, R.CRITIC_SIZES, OC.gate)
    g64, g32 = SC.references(m, "init")
    SC.check_actor_gradient(f"m={m} SAC actor", run.sac_actor_grad(s["actor"], s["critics"], s["obs"], s["draw"]), g64, g32, OC.gate)


def _poisoned_rollout(case, keys, key, row, col=None):
    """a copy of the rollout's arrays (nothing of the shared case is written) with NaN planted in `key` of rollout row `row`"""
    out = {k: (case[k].copy() if k in keys else case[k]) for k in case if k != "rng"}
    if col is None:
        out[key][row] = NAN
    else:
        out[key][row, col] = NAN
    return out


def onpolicy_poisons(algo):
    return (("obs", 1), ("adv", None)) + ((("logp_old", None),) if algo == "ppo" else ())


def onpolicy_gradients(run, algo):
    """brs_learner_grad / brs_a2c_grad at m = 257 on two workgroups: chunk 1 is one row, index 256, which points at a poisoned rollout
    row that no other index points at.  normalize_adv = 0 keeps the poison in its row on the reference side; one PPO case with
    normalize_adv = 1, where the reference makes every row NaN"""
    m = ONPOLICY_M
    ref, cases, need = (PL, LC, PPO_NEED) if algo == "ppo" else (A, AC, A2C_NEED)
    keys = ("obs", "act", "logp_old", "adv", "ret") if algo == "ppo" else A.KEYS
    grad = run.ppo_grad if algo == "ppo" else run.a2c_grad
    cfg = (PL.Cfg if algo == "ppo" else A.Cfg)(normalize_adv=0)
    case, idx = cases.conditioned(m, cfg)
    row = int(idx[m - 1])
    assert len(idx) == m and row not in idx[:m - 1], "the poisoned rollout row must be the lone sample of the second chunk"
    settings = [(cfg, case, idx, k, col) for k, col in onpolicy_poisons(algo)]
    if algo == "ppo":
        cfg1 = PL.Cfg(normalize_adv=1)
        case1, idx1 = cases.conditioned(m, cfg1)
        settings.append((cfg1, case1, idx1, "adv", None))
    for cf, cs, ix, key, col in settings:
        what = f"{algo} m={m} normalize_adv={cf.normalize_adv} NaN in {key}"
        bad = _poisoned_rollout(cs, keys, key, int(ix[m - 1]), col)
        g64 = _ref(ref.grad_buffer, bad, ix, cf)
        reference_reaches(what, g64, ONPOLICY_PLACES, need[key])
        check_gradient_nans(what, grad(bad, ix, cf, ONPOLICY_WG), g64)
    cases.gate(grad(case, idx, cfg, ONPOLICY_WG), ref.grad_buffer(case, idx, cfg), f"{algo} m={m} clean")
