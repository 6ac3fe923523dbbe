"""What the CPU and the GPU tests of SAC share (tests/test_sac_cpu.py, tests/test_sac_gpu.py): the weight sets, the gradient cases with
their conditions, the act / target cases, the branch-coverage assertion, the six-step chain case with the trajectory rule, and the
host build of the kernel source (tests/sachost).

Weight sets.  `init` and `x3` are the SAC actor drawn like offpolicy_cases' (torch's default init, times 1 or 3) with the critics of
td3_cases.weights; `spread` is `init` with the log-std head's two rows and biases scaled by SPREAD (and the biases shifted) so that the
raw log_std spans well past both clamps.  In `init` and `x3` the two log-std biases are shifted by LOG_STD_SHIFT = -2 (sigma around
0.13): with sigma around 1 the sign of a row's action is the sign of its z, the entropy term's share of the b3 gradient then sums
symmetric noise over the rows and cancels whatever the observations are, and z is the row's Philox block, not an input that could be
redrawn.  log_ent_coef is -0.5 / 0.3 / -1.0: an alpha of 1 would hide a missing factor.

Conditions of a gradient case, all checked on the fp64 yardstick alone, offending rows redrawn (never dropped) under the round limits
of ddpg_learner_cases: for the actor on obs and both critics on (obs, a(obs)) 25 % to 75 % of every hidden layer active, no
pre-activation within MARGIN[kind] of 0, fp32 torch's pre-activations within a tenth of that; |Q0 - Q1| >= MARGIN; the raw log_std at
least MARGIN from -20 and from 2; and no cancellation behind the b3 gradient (|sum t| >= 1/4 sum |t| for the four columns of
d La / d (actor output)) nor behind the temperature's (the same for logp + target_entropy).

The sample split: the rows, the handle of 8,448 and the sequence are ddpg_learner_cases' (SPLIT_*); which weight set goes to which row,
the bound of the comparison with the host build, the allocation's arithmetic (partial_storage) and the case with the last row alone
replaced (changed_last_row) are here, for both widths (tests/sac_arch_cases.py executes this source a second time)."""
import ctypes as C
import os

import numpy as np
import torch

import ref_ddpg_learner as RL
import ref_offpolicy as R
import ref_sac as S
import td3_cases as TC
from balance_robot_mujoco_rl_amd import _lib
from ddpg_learner_cases import (GRAD_GATE, SPLIT_BIG, SPLIT_LAST_REAL, SPLIT_ROWS, SPLIT_SEQUENCE, SPLIT_TABLE, SPLIT_X3_ROWS, _draw, _no_cancellation,
                                block_distances)
from hostbuild import ROOT, _ptr, compile_host
from offpolicy_cases import GAMMA, GATE, SEED, _active_ok, conditioned

HOST_DIR = os.path.join(ROOT, "tests", "sachost")
NA, NC = S.NACTOR, S.NCRITIC
WEIGHT_SETS = ("init", "x3", "spread")
MARGIN = {"init": 1e-5, "x3": 1e-4, "spread": 1e-5}
LOG_ENT_COEF = {"init": -0.5, "x3": 0.3, "spread": -1.0}
LOG_STD_SHIFT = -2.0
SPREAD, SPREAD_SHIFT = 60.0, -9.0          # the log-std head of `spread`: rows and biases x 60, biases - 9 (the middle of [-20, 2])
TARGET_ENTROPY = -2.0                      # SB3: -prod(action_space.shape)
ACT_ROWS_CPU = (1, 33, 257)
GRAD_ROWS_CPU = (1, 33, 257, 1000)
GPU_ROWS = (1, 31, 32, 33, 127, 128, 129, 257, 1000)
ACT_ROWS_GPU = (1, 31, 32, 33, 127, 128, 129, 257)
# The sample-split geometries (ddpg_learner_cases.SPLIT_TABLE: 385 to 8,193 rows, two to eight partial rows) as the SAC calls are taken
# through them.  `spread` -- the clamped log_std branches -- at 769 (the last split is ONE real row and 127 padding rows) and at 2,049
# (six splits, the last the short one); at 8,193 its [256, 256] case takes 7 s to condition, so it stops there.
SPLIT_SPREAD_ROWS = (769, 2049)
SPLIT_ACTOR_CASES = [(n, "init") for n in SPLIT_ROWS] + [(n, "x3") for n in SPLIT_X3_ROWS] + [(n, "spread") for n in SPLIT_SPREAD_ROWS]
SPLIT_TWIN_CASES = [(n, "init") for n in SPLIT_ROWS] + [(n, "x3") for n in SPLIT_X3_ROWS]
SPLIT_STAT_ROWS = (769, 8193)              # the statistics alone: a lone real row in the last of three splits; eight splits, uneven
MAX_SPLIT = max(nsplit for _, _, nsplit in SPLIT_TABLE.values())
assert MAX_SPLIT == 8 and SPLIT_LAST_REAL[769] == 1 and set(SPLIT_SPREAD_ROWS) | set(SPLIT_STAT_ROWS) <= set(SPLIT_ROWS)
# The host build's plain loops are compared at every split row where ONE host gradient takes under 5 s on a CPU.  Measured, one
# sh_actor_grad / one sh_twin_critic_grad: 1.2 s / 0.6 s at 2,049 rows, 4.7 s / 2.4 s at 8,193 -- every row of SPLIT_ROWS.  (At
# [256, 256], tests/sac_arch_cases.py: 1.8 s / 1.3 s and 6.6 s / 5.1 s, so the bound there is 2,049.)
HOST_ROWS_MAX = 8193
SAC_TAIL = 1 + S.NSTAT                   # what follows the actor's parameters in a row: the temperature's gradient, then the statistics
SAC_ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=0.005)
CHAIN_STEPS, CHAIN_ROWS = 6, 200
_LAYERS = np.cumsum([0, 300, 200, 200, 150, 200, 150])


def weights(kind):
    """actor VECTOR [NACTOR + 1], critics [2 NCRITIC]"""
    base = "init" if kind == "spread" else kind
    actor = R.init_params(S.ACTOR_SIZES, np.random.default_rng(17), {"init": 1.0, "x3": 3.0}[base])
    sl = RL.block_slices(S.ACTOR_SIZES)
    w3, b3 = actor[sl["W3"]].reshape(4, 200), actor[sl["b3"]]
    if kind != "spread":
        b3[2:] += np.float32(LOG_STD_SHIFT)
    else:
        w3[2:] *= np.float32(SPREAD)
        b3[2:] = b3[2:] * np.float32(SPREAD) + np.float32(SPREAD_SHIFT)
    return S.with_log_ent_coef(actor, LOG_ENT_COEF[kind]), TC.weights(base)[1]


# ------------------------------------------------------------------------------------------------ gradient cases
def _look(actor, critics, obs, z, dtype=torch.float64):
    """what the conditions are decided on: the hidden pre-activations of actor(obs), critic 0 and critic 1 on (obs, a(obs))
    [m][300 + 200 + 200 + 150 + 200 + 150], the two Q [m][2] and the raw log_std [m][2]"""
    with torch.no_grad():
        w, c, o, zz = S._t(actor, dtype), S._t(critics, dtype), S._t(obs, dtype), S._t(z, dtype)
        out, a1, a2 = RL.net(w[:NA], o, S.ACTOR_SIZES, False, hidden=True)
        a = torch.tanh(out[:, :2] + torch.clamp(out[:, 2:], S.LOG_STD_MIN, S.LOG_STD_MAX).exp() * zz)
        q0, c1, c2 = RL.q_of(c[:NC], o, a, hidden=True)
        q1, d1, d2 = RL.q_of(c[NC:], o, a, hidden=True)
        return torch.cat([a1, a2, c1, c2, d1, d2], dim=1).numpy(), torch.stack([q0, q1], dim=1).numpy(), out[:, 2:].numpy()


def _bad_rows(actor, critics, obs, z, margin):
    pre, q, raw = _look(actor, critics, obs, z)
    pre32 = _look(actor, critics, obs, z, torch.float32)[0]
    near = (np.abs(pre) < margin).any(axis=1)
    far = (np.abs(pre32 - pre) > 0.1 * margin).any(axis=1)
    tie = np.abs(q[:, 0] - q[:, 1]) < margin
    edge = ((np.abs(raw - S.LOG_STD_MIN) < margin) | (np.abs(raw - S.LOG_STD_MAX) < margin)).any(axis=1)
    return near | far | tie | edge | ~_active_ok(*[pre[:, a:b] for a, b in zip(_LAYERS[:-1], _LAYERS[1:])])


_CASES = {}


def grad_case(n, kind, draw=0):
    """obs [n][6], act [n][2], y [n] (float32; act and y for the critic gradient), the actor vector and the critics, z [n][2] of
    (SEED, draw) and the fp64 per-row quantities; computed once, never written afterwards"""
    key = (n, kind, draw)
    if key in _CASES:
        return _CASES[key]
    actor, critics = weights(kind)
    margin = MARGIN[kind]
    rng = np.random.default_rng(6000 + n)
    z = S.row_noise(S.TAG_PI, SEED, draw, n)
    obs, act = _draw(rng, n)
    for attempt in range(400):
        for rounds in range(200):
            bad = _bad_rows(actor, critics, obs, z, margin)
            if not bad.any():
                break
            obs[bad], act[bad] = _draw(rng, int(bad.sum()))
        else:
            raise AssertionError("could not condition the inputs")
        terms, q, logp = S.row_terms(actor, critics, obs, SEED, draw)
        columns = [terms[:, k] for k in range(4)] + [logp + TARGET_ENTROPY]
        ok = [_no_cancellation(t) for t in columns]
        if all(ok):
            break
        if attempt % 50 == 49:
            print(f"  n={n} {kind}: attempt {attempt}, columns without cancellation: {ok}")
        for t, good in zip(columns, ok):   # redraw the rows that pull a sum towards zero: those whose term has the minority sign
            if not good:
                minority = np.sign(t) != np.sign(t.sum())
                obs[minority], act[minority] = _draw(rng, int(minority.sum()))
    else:
        raise AssertionError("could not remove the cancellation")
    pre, q, raw = _look(actor, critics, obs, z)
    assert np.abs(pre).min() >= margin and np.abs(_look(actor, critics, obs, z, torch.float32)[0] - pre).max() <= 0.1 * margin, (n, kind)
    y = (R.critic(critics[:NC], obs, act) + 0.5 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    a, logp, parts = S.sample(actor, obs, z)
    _CASES[key] = dict(obs=obs, act=act, y=y, actor=actor, critics=critics, z=z, draw=draw, q=q, raw=raw, a=a, logp=logp,
                       one_minus_a2=parts["one_minus_a2"])
    return _CASES[key]


_REFS = {}


def references(n, kind, learn_alpha=True):
    """the fp64 actor gradient of grad_case(n, kind) and fp32 torch's on the same inputs"""
    key = (n, kind, learn_alpha)
    if key not in _REFS:
        c = grad_case(n, kind)
        args = (c["actor"], c["critics"], c["obs"], SEED, c["draw"], learn_alpha, TARGET_ENTROPY)
        _REFS[key] = (S.actor_grad(*args), S.actor_grad(*args, dtype=torch.float32))
    return _REFS[key]


def actor_block_distances(g, g64):
    """{block: ||g - g64|| / ||g64||} over the six parameter blocks and the temperature's slot (a block of its own; with a fixed
    ent_coef the reference is 0 and the distance is |g|)"""
    d = block_distances(g[:NA], g64[:NA], S.ACTOR_SIZES)
    ref = abs(float(g64[NA]))
    d["log_ent_coef"] = abs(float(g[NA]) - float(g64[NA])) / ref if ref > 0 else abs(float(g[NA]))
    return d


def check_actor_gradient(what, g, g64, g32, stat_gate):
    """ddpg_learner_cases.check_gradient's rule on the SAC buffer: every block, the temperature's slot among them, within GRAD_GATE of
    fp64, the statistics within offpolicy_cases.gate; prints the largest distance next to fp32 torch's; -> (mine, torch32)"""
    mine, t32 = actor_block_distances(g, g64), actor_block_distances(g32, g64)
    worst = max(mine, key=mine.get)
    print(f"{what}: largest block distance from fp64 {mine[worst]:.3g} ({worst}); fp32 torch {max(t32.values()):.3g} ({max(t32, key=t32.get)})")
    stat_gate(g[NA + 1:], g64[NA + 1:], what + " statistics")
    assert max(mine.values()) <= GRAD_GATE, (what, mine, t32)
    return max(mine.values()), max(t32.values())


_TWIN_REFS = {}


def twin_reference(n, kind):
    """the fp64 twin critic gradient [2 NC + 4] of grad_case(n, kind); computed once"""
    if (n, kind) not in _TWIN_REFS:
        c = grad_case(n, kind)
        _TWIN_REFS[(n, kind)] = S.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"])
    return _TWIN_REFS[(n, kind)]


# ------------------------------------------------------------------------------------------------ the sample split
def partial_storage(make):
    """make(max_batch) -> a learner handle.  -> (scratch rows, floats the handle keeps for partial rows), from the sizes of two
    allocations and nothing else: a handle's bytes are 4 (rows pad128(max_batch) + partial), so handles of 256 and of 128 rows
    differ by rows x 128 floats, and what the 128-row handle holds beyond rows x 128 floats is the partial storage.  Launches nothing."""
    sizes = []
    for max_batch in (128, 256):
        lrn = make(max_batch)
        sizes.append(lrn.scratch()[1])
        lrn.close()
    step = sizes[1] - sizes[0]
    assert step > 0 and step % (4 * 128) == 0 and sizes[0] % 4 == 0, sizes
    rows = step // (4 * 128)
    return rows, sizes[0] // 4 - rows * 128


def assert_partial_rows_fit(make, longest_row, what):
    """MAX_SPLIT partial rows of the longest row a call on the handle writes fit what the handle keeps for them (the SAC counterpart
    of bit 5 of ddpglearnerhost's dh_split_sweep); -> (scratch rows, partial floats)"""
    rows, partial = partial_storage(make)
    print(f"{what}: {rows} scratch rows, {partial} floats of partial storage = {partial / longest_row:.4f} rows of {longest_row} floats")
    assert rows > 0 and partial >= MAX_SPLIT * longest_row, (what, rows, partial, longest_row)
    return rows, partial


def moved(new, old):
    """|new - old| / max(1, |old|), element by element: the measure of offpolicy_cases.gate"""
    new, old = np.asarray(new, np.float64), np.asarray(old, np.float64)
    return np.abs(new - old) / np.maximum(1.0, np.abs(old))


ROW_SUMS = 4   # of the SAC_TAIL sums behind the actor's parameters the first four depend on the rows; the fifth, ent_coef, is alpha / m from every row
_CHANGED = {}


def changed_last_row(n, kind="init"):
    """grad_case(n, kind) with row n - 1 ALONE replaced (another observation, twice as far out, another action, y + 4), and the fp64
    actor and twin critic gradients of that.  The replacement is drawn until, on the fp64 reference, each of the four row-dependent
    tail sums and each of the twin call's four statistics has moved by more than 2 GATE in gate's measure: two results that are each
    within GATE of their reference then cannot be equal.  The changed row is held to no gradient condition: only the statistics of
    this case are compared.  -> (case, actor64, twin64); computed once"""
    if (n, kind) in _CHANGED:
        return _CHANGED[(n, kind)]
    c = grad_case(n, kind)
    a64, t64 = references(n, kind)[0], twin_reference(n, kind)
    rng = np.random.default_rng(9000 + n)
    for _ in range(50):
        obs, act, y = c["obs"].copy(), c["act"].copy(), c["y"].copy()
        o, a = _draw(rng, 1)
        obs[n - 1], act[n - 1], y[n - 1] = np.float32(2.0) * o[0], a[0], c["y"][n - 1] + np.float32(4.0)
        b64 = S.actor_grad(c["actor"], c["critics"], obs, SEED, c["draw"], True, TARGET_ENTROPY)
        u64 = S.twin_critic_grad(c["critics"], obs, act, y)
        shift = np.concatenate([moved(b64[NA:NA + ROW_SUMS], a64[NA:NA + ROW_SUMS]), moved(u64[2 * NC:], t64[2 * NC:])])
        if shift.min() > 2 * GATE:
            break
    else:
        raise AssertionError("no replacement of the last row moves every sum")
    assert np.array_equal(obs[:n - 1], c["obs"][:n - 1]) and np.array_equal(act[:n - 1], c["act"][:n - 1]) and np.array_equal(y[:n - 1], c["y"][:n - 1])
    _CHANGED[(n, kind)] = ({**c, "obs": obs, "act": act, "y": y}, b64, u64)
    return _CHANGED[(n, kind)]


# ------------------------------------------------------------------------------------------------ act and target cases
_TARGETS = {}
# How much the sample of a row amplifies what its inputs carry in fp32, on the fp64 reference.  z comes out of normal_pair (24-bit
# uniforms through logf, cosf and sinf) up to 3e-6 from its fp64 value -- the largest distance the z gate prints on these cases is
# 2.84e-6 -- and the actor's log_std output carries the forward's rounding.  Both enter u = mu + sigma z multiplied by sigma (by
# sigma |z| for log_std), up to e^2 = 7.4; a = tanh(u) receives that times 1 - a^2, logp receives it times |2 a g / (g + 1e-6)|.  A row
# near the middle of the tanh with a clamped-high sigma takes 2e-5 from z alone: no arithmetic of the tail could meet 1e-5 on it, and
# fp32 torch fed the SAME fp32 z would not either.  Rows whose amplification of either output (relative to max(1, |output|), as the
# gate measures) exceeds AMP = 1 are redrawn.  y receives logp's absolute error times gamma alpha, relative to max(1, |y|), which can be
# far smaller than |logp| (up to 50 here): it is held to the same bound.  AMP = 1: the kernels and the host build are compared at the
# same gate, their z differ from fp64 by up to 3e-6 each with either sign, so 2 x AMP x 3e-6 must leave room for the tails' own
# operations.
AMP = 1.0


def _sensitive_rows(actor, obs, z, y_of=None):
    """y_of: obs -> (gamma alpha [rows where done == 0, else 0], y): the target's own amplification is checked too"""
    a, logp, p = S.sample(actor, obs, z)
    g, reach = p["one_minus_a2"], np.exp(p["log_std"]) * np.maximum(1.0, np.abs(z))
    amp_a = (g * reach).max(axis=1)
    amp_abs = (np.abs(2.0 * a * g / (g + S.EPS)) * reach).sum(axis=1)
    bad = (amp_a > AMP) | (amp_abs / np.maximum(1.0, np.abs(logp)) > AMP)
    if y_of is not None:
        weight, y = y_of(obs)
        bad |= weight * amp_abs / np.maximum(1.0, np.abs(y)) > AMP
    return bad


def _sample_inputs(m, kind, z, seed, target_draw=None):
    """offpolicy_cases.conditioned(m, ...) with the rows whose sample under z is too sensitive to its fp32 inputs (above) redrawn;
    target_draw: z is the target's noise of that draw, and y is held to the bound too"""
    base = conditioned(m, "x3" if kind == "x3" else "init")
    actor, critics = weights(kind)
    obs, rng = base["obs"].copy(), np.random.default_rng(seed + m)
    y_of = None
    if target_draw is not None:
        weight = GAMMA * np.exp(np.float64(actor[NA])) * (base["done"] == 0)
        y_of = lambda o: (weight, S.sac_target(actor, critics, o, base["reward"], base["done"], GAMMA, SEED, target_draw)[0])
    for _ in range(200):
        bad = _sensitive_rows(actor, obs, z, y_of)
        if not bad.any():
            return obs, base["reward"], base["done"]
        obs[bad] = _draw(rng, int(bad.sum()))[0]
    raise AssertionError("could not condition the inputs")


def act_case(n, kind, step=0):
    """obs [n][6], the actor vector and the fp64 references of brs_sac_act at `step`, sampled and deterministic; computed once"""
    key = ("act", n, kind, step)
    if key not in _TARGETS:
        actor = weights(kind)[0]
        obs = _sample_inputs(n, kind, S.act(actor, np.zeros((n, 6)), SEED, 0, step)[3], 7100)[0]
        _TARGETS[key] = dict(obs=obs, actor=actor, step=step, act=S.act(actor, obs, SEED, 0, step), act_det=S.act(actor, obs, SEED, 0, step, deterministic=True))
    return _TARGETS[key]


def target_case(m, kind, draw=0):
    """next_obs [m][6], reward and done, the weights, and the fp64 reference of the target with what its branches are decided on;
    computed once"""
    key = (m, kind, draw)
    if key not in _TARGETS:
        actor, critics = weights(kind)
        next_obs, reward, done = _sample_inputs(m, kind, S.row_noise(S.TAG_TARGET, SEED, draw, m), 7000, target_draw=draw)
        y, a, logp, z, parts = S.sac_target(actor, critics, next_obs, reward, done, GAMMA, SEED, draw, parts=True)
        _TARGETS[key] = dict(next_obs=next_obs, reward=reward, done=done, actor=actor, critics=critics, y=y, a=a, logp=logp, z=z, draw=draw,
                             raw=parts["raw"], q=np.stack([parts["q0"], parts["q1"]], axis=1), one_minus_a2=parts["one_minus_a2"])
    return _TARGETS[key]


def branch_counts(case):
    """rows (log_std: elements) of every branch of the sample, the min-select and the combine, on the fp64 reference"""
    raw, q, g, a = case["raw"], case["q"], case["one_minus_a2"], case["a"]
    out = dict(log_std_low=int((raw < S.LOG_STD_MIN).sum()), log_std_high=int((raw > S.LOG_STD_MAX).sum()),
               log_std_in=int(((raw >= S.LOG_STD_MIN) & (raw <= S.LOG_STD_MAX)).sum()),
               min_from_0=int((q[:, 0] <= q[:, 1]).sum()), min_from_1=int((q[:, 1] < q[:, 0]).sum()),
               saturated=int((g < 1e-6).any(axis=1).sum()), unsaturated=int((np.abs(a) < 0.5).any(axis=1).sum()))
    if "done" in case:
        out.update(done_0=int((case["done"] == 0).sum()), done_1=int((case["done"] != 0).sum()))
    return out


def assert_branch_coverage():
    """`spread` at m = 33 takes every branch with at least 1 row, at m = 257 with at least 8: in the gradient case and in the target
    case; -> the four tables"""
    tables = {}
    for m, least in ((33, 1), (257, 8)):
        for name, case in (("gradient", grad_case(m, "spread")), ("target", target_case(m, "spread"))):
            t = branch_counts(case)
            print(f"branches of the {name} case, spread, m = {m}: {t}")
            assert all(v >= least for v in t.values()), (name, m, t)
            tables[(name, m)] = t
    return tables


# ------------------------------------------------------------------------------------------------ the six-step chain
_CHAIN = {}


def run_chain(t, case, steps=CHAIN_STEPS, on_step=None):
    """`t`: a TorchSAC; per step the target from the current actor and the critics' target (draw = the step's index), then the update
    with the same draw for the actor's noise"""
    for s in range(steps):
        sl = slice(s * CHAIN_ROWS, (s + 1) * CHAIN_ROWS)
        y = t.target(case["next_obs"][sl], case["reward"][sl], case["done"][sl], GAMMA, SEED, s)
        if on_step:
            on_step(sl, s)
        t.step(case["obs"][sl], case["act"][sl], y, SEED, s, between=(lambda: on_step(sl, s)) if on_step else None)
    return t.flats()


def chain_case(kind="init"):
    """six minibatches of 200 rows from the same initial weights such that no hidden pre-activation of the fp64 chain -- actor(obs),
    critic k(obs, a(obs)) and critic k(obs, act), before the critics' step and between it and the actor's pass -- comes within the
    margin of 0 and no |Q0 - Q1| within it (rows redrawn until that holds), and where that chain ends in fp64 and in fp32 torch"""
    if kind in _CHAIN:
        return _CHAIN[kind]
    actor, critics = weights(kind)
    n, margin, rng = CHAIN_STEPS * CHAIN_ROWS, MARGIN[kind], np.random.default_rng(277)
    obs, act = _draw(rng, n)
    case = dict(obs=obs, act=act, actor=actor, critics=critics, next_obs=_draw(rng, n)[0], reward=rng.standard_normal(n).astype(np.float32),
                done=(np.arange(n) % 3 == 1).astype(np.uint8))
    for _ in range(100):
        t = S.TorchSAC(actor, critics, target_entropy=TARGET_ENTROPY, **SAC_ADAM)
        bad = np.zeros(n, bool)

        def look(sl, s):
            f = t.flats()
            z = S.row_noise(S.TAG_PI, SEED, s, CHAIN_ROWS)
            pre, q, raw = _look(f["actor"], f["critics"], case["obs"][sl], z)
            given = np.concatenate([TC._critic_pre(f["critics"][k * NC:(k + 1) * NC], case["obs"][sl], case["act"][sl]) for k in (0, 1)], axis=1)
            bad[sl] |= (np.abs(pre).min(axis=1) < margin) | (np.abs(given).min(axis=1) < margin) | (np.abs(q[:, 0] - q[:, 1]) < margin)
        case["ref64"] = run_chain(t, case, on_step=look)
        if not bad.any():
            break
        case["obs"][bad], case["act"][bad] = _draw(rng, int(bad.sum()))
    else:
        raise AssertionError("could not condition the chain")
    case["ref32"] = run_chain(S.TorchSAC(actor, critics, torch.float32, target_entropy=TARGET_ENTROPY, **SAC_ADAM), case)
    _CHAIN[kind] = case
    return case


def check_chain(what, flats, case):
    """ddpg_learner_cases.check_trajectory's rule on the SAC vectors: per block of theta_end - theta_0 (the actor's six and the
    temperature as a block of the actor; each critic and each target a network of its own), the distance from the fp64 chain is at most
    4x fp32 torch's, the latter floored at its largest value over the blocks of the network; prints both"""
    worst = 0.0

    def dist(x, d64, sizes, start, temp):
        d = block_distances(np.asarray(x, np.float64)[:R.nparam(sizes)] - start[:R.nparam(sizes)], d64[:R.nparam(sizes)], sizes)
        if temp:
            d["log_ent_coef"] = abs(float(x[NA]) - float(start[NA]) - float(d64[NA])) / abs(float(d64[NA]))
        return d
    for netname, sizes, sl in (("actor", S.ACTOR_SIZES, slice(None)), ("critics", R.CRITIC_SIZES, slice(0, NC)), ("critics", R.CRITIC_SIZES, slice(NC, 2 * NC)),
                               ("critics_target", R.CRITIC_SIZES, slice(0, NC)), ("critics_target", R.CRITIC_SIZES, slice(NC, 2 * NC))):
        start = case[netname.split("_")[0]][sl].astype(np.float64)
        d64 = case["ref64"][netname][sl] - start
        temp = netname == "actor"
        mine = dist(np.asarray(flats[netname], np.float64)[sl], d64, sizes, start, temp)
        t32 = dist(case["ref32"][netname].astype(np.float64)[sl], d64, sizes, start, temp)
        floor = max(t32.values())
        label = netname + ("" if sl == slice(None) else f"[{sl.start // NC}]")
        for b in mine:
            print(f"{what} {label}.{b}: |d - d64| / |d64| = {mine[b]:.3g}, fp32 torch {t32[b]:.3g} (gate 4 x {floor:.3g})")
            worst = max(worst, mine[b] / floor)
        for b in mine:
            assert mine[b] <= 4 * floor, (what, label, b, mine[b], t32[b], floor)
    return worst


# ------------------------------------------------------------------------------------------------ the host build
def build_host(directory):
    """g++ -> libsachost.so in `directory`, with its signatures applied"""
    L = compile_host(directory, "libsachost.so", os.path.join(HOST_DIR, "sachost.cpp"))
    vp, i, f, u64, u32 = C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint32
    L.sh_act.restype, L.sh_act.argtypes = i, [vp, i, vp, u64, C.c_int64, u32, i, i, vp, vp, vp, vp]
    L.sh_target.restype, L.sh_target.argtypes = i, [vp, vp, i, vp, vp, vp, f, u64, u32, vp, vp, vp, vp]
    L.sh_twin_critic_grad.restype, L.sh_twin_critic_grad.argtypes = i, [vp, i, vp, vp, vp, f, vp]
    L.sh_actor_grad.restype, L.sh_actor_grad.argtypes = i, [vp, vp, i, vp, u64, u32, i, f, vp, vp]
    L.sh_apply.restype, L.sh_apply.argtypes = i, [i, vp, vp, vp, vp, vp, C.POINTER(_lib.BrsAdamConfig), C.c_int64, f]
    L.sh_td3_combine.restype, L.sh_td3_combine.argtypes = i, [i, vp, vp, f, vp, vp, vp]
    L.sh_q.restype, L.sh_q.argtypes = i, [vp, i, vp, vp, vp]
    L.sh_argument_error.restype, L.sh_argument_error.argtypes = C.c_char_p, [i, vp, vp, i, vp, vp, vp, f, vp, i]
    return L


def host_act(L, actor, obs, seed, base, step, deterministic=False, random=False, n=None, extras=True):
    n = len(obs) if n is None else n
    a, mu, ls, z = (np.zeros((n, 2), np.float32) for _ in range(4))
    assert L.sh_act(_ptr(actor), n, _ptr(obs), seed, base, step, int(deterministic), int(random), _ptr(a), *[_ptr(x) if extras else None for x in (mu, ls, z)]) == 0
    return a, mu, ls, z


def host_target(L, actor, critics_t, next_obs, reward, done, gamma, seed, draw, extras=True):
    m = len(next_obs)
    y, a, lp, z = np.zeros(m, np.float32), np.zeros((m, 2), np.float32), np.zeros(m, np.float32), np.zeros((m, 2), np.float32)
    assert L.sh_target(_ptr(actor), _ptr(critics_t), m, _ptr(next_obs), _ptr(reward), _ptr(done), gamma, seed, draw, _ptr(y),
                       *[_ptr(x) if extras else None for x in (a, lp, z)]) == 0
    return y, a, lp, z


def host_twin_critic_grad(L, critics, obs, act, y, loss_scale=0.5):
    g = np.zeros(2 * NC + 4, np.float32)
    assert L.sh_twin_critic_grad(_ptr(critics), len(obs), _ptr(obs), _ptr(act), _ptr(y), loss_scale, _ptr(g)) == 0
    return g


def host_actor_grad(L, actor, critics, obs, seed, draw, learn_alpha=True, target_entropy=TARGET_ENTROPY):
    g = np.zeros(NA + 1 + S.NSTAT, np.float32)
    assert L.sh_actor_grad(_ptr(actor), _ptr(critics), len(obs), _ptr(obs), seed, draw, int(learn_alpha), target_entropy, _ptr(g), None) == 0
    return g


class HostSAC:
    """tests/sachost behind DeviceSACLearner.step's surface, on numpy arrays"""

    def __init__(self, L, actor, critics, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=0.005, target_entropy=TARGET_ENTROPY, learn_alpha=True):
        self.L, self.cfg, self.tau = L, _lib.BrsAdamConfig(lr, betas[0], betas[1], eps), tau
        self.target_entropy, self.learn_alpha = target_entropy, learn_alpha
        self.flat = {"actor": actor.copy(), "critics": critics.copy(), "critics_target": critics.copy()}
        self.mom = {k: (np.zeros_like(self.flat[k]), np.zeros_like(self.flat[k])) for k in ("actor", "critics")}
        self.steps, self.grad = 0, {}

    def apply(self, name, grad, target):
        p, (m, v) = self.flat[name], self.mom[name]
        assert self.L.sh_apply(p.size, _ptr(p), _ptr(grad), _ptr(m), _ptr(v), _ptr(self.flat[name + "_target"]) if target else None,
                               C.byref(self.cfg), self.steps, self.tau) == 0

    def target(self, next_obs, reward, done, gamma, seed, draw):
        return host_target(self.L, self.flat["actor"], self.flat["critics_target"], next_obs, reward, done, gamma, seed, draw)[0]

    def step(self, obs, act, y, seed, draw):
        self.steps += 1
        self.grad["critics"] = host_twin_critic_grad(self.L, self.flat["critics"], obs, act, y)
        self.apply("critics", self.grad["critics"], True)
        self.grad["actor"] = host_actor_grad(self.L, self.flat["actor"], self.flat["critics"], obs, seed, draw, self.learn_alpha, self.target_entropy)
        self.apply("actor", self.grad["actor"], False)
