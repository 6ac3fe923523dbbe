"""What the CPU and the GPU tests of the PPO rollout kernels share (tests/test_policy_cases_cpu.py, tests/test_policy_kernels_gpu.py):
the rows, the weight sets, the cases with their admission conditions (computed once, never written afterwards), the fp32 numpy
restatement of the kernels' arithmetic that the conditions are decided on, and the checks themselves -- written on plain arrays, so
that the CPU file runs every one of them on the restatement and the GPU file on the kernels' outputs.

Rows.  ROWS hits the half-wave edge (32: the two N-tiles of a wave), the wave edge (64) and the workgroup edge (256); 513 is two full
workgroups plus one row.

Weight sets.  `init` is ref_learner.init_params; `x3` multiplies every weight and bias by 3 (the tanh saturates), log_std untouched;
log_std = (-0.3, 0.2) in both.  Observations are standard_normal x ref_learner.OBS_SCALE, float32.  An x10 set is deliberately absent:
there an fp32 numpy restatement of the towers is 6e-6 to 8e-6 from fp64 even with libm's tanh, too close to the gate to tell a bug from
rounding.

The gate is offpolicy_cases.gate: |x - ref| <= 1e-5 max(1, |ref|).

Admission of a forward case: forward32 below -- fp32 numpy with the kernel's tanh, 1 - 2 / (2^(2 x log2 e) + 1) -- stays within a third
of the gate of fp64 on it; rows that do not are redrawn, never dropped.  Every case with n >= 33 carries six saturated rows: saturated
row j has feature j set to +-1e30 (alternating sign), the other features ordinary.  One huge feature leaves no cancellation in a
layer-1 pre-activation: its sign is the weight's sign in any precision, the kernel's tanh takes its e = +inf and e = 0 ends, and the
fp64 reference gives exactly +-1 there.

Action, clipped action and logp are gated against fp64 arithmetic on the kernel's OWN returned z (widened), as the existing test does:
fp32 Box-Muller is up to 3e-6 from its fp64 value (see the note in sac_cases.py), which the gate of `noise` alone has to absorb.

Admission of a GAE case: the fp32 numpy recursion on the same inputs stays within half the gate of fp64; a case that does not is drawn
again.  The listed shapes reach at most 4.2e-6 at T = 64 and less at T = 32; a long, slowly discounted column such as
(128, 65, .999, .99) reaches 1.5e-5 in fp32 numpy alone and must not be added."""
import numpy as np

import ref_learner as RL
import ref_policy as P
from offpolicy_cases import GATE, gate

ROWS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
WEIGHT_SETS = ("init", "x3")
LOG_STD = (-0.3, 0.2)
SEED, BASE, STEP, GAMMA = 5, 1000, 3, 0.99
SATURATED, HUGE = 6, 1e30
ISOLATION_ROWS = (129, 257)
COUNTER_ROWS = 65
COUNTERS = {"carry into gid_hi": dict(env_index_base=2 ** 32 - 33), "gid_hi set": dict(env_index_base=2 ** 40 + 7),
            "step = 2^32 - 1": dict(step=2 ** 32 - 1), "seed with high bits": dict(seed=2 ** 63 + 12345)}
LONE = (0, 31, 32, 63, 64, 255, 256, 511, 512)
PATTERN_ROWS = 513
PATTERNS = tuple(f"lone{k}" for k in LONE) + ("none", "both", "mixed")
RANDOM_FLAG_ROWS = (1, 33, 257)
GAE_CASES = ((1, 1, .99, .95, .1), (37, 257, .99, .95, .08), (32, 257, 1., 1., .05), (32, 257, 1., 1., 0.), (64, 257, .99, 0., .08),
             (64, 257, 0., .95, .08))
CONTRACT_ROWS = 257
FLAG_VALUES = (1, 2, 255)                   # "set" is any non-zero byte
KEYS = ("action", "clipped", "logp", "value", "noise")


def weights(kind):
    flat = RL.init_params(np.random.default_rng(23))
    if kind == "x3":
        flat[:-2] *= np.float32(3.0)
    flat[-2:] = LOG_STD
    return flat


def distance(x, ref):
    """the gate's measure, per element"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return np.abs(x - ref) / np.maximum(1.0, np.abs(ref))


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def tanh32(x):
    """the kernel's tanh in float32: 1 - 2 / (e^(2x) + 1), e = +inf -> 1, e = 0 -> -1"""
    with np.errstate(over="ignore"):
        e = np.exp2(np.asarray(x, np.float32) * np.float32(2.8853900817779268))
    return np.float32(1.0) - np.float32(2.0) / (e + np.float32(1.0))


def forward32(flat, obs):
    """-> mean [n][2], value [n]: plain fp32 numpy, the kernel's tanh"""
    flat, obs = np.asarray(flat, np.float32), np.asarray(obs, np.float32)
    B = {name: flat[sl].reshape(shape) for (name, shape), sl in zip(RL.BLOCKS, RL.block_slices().values())}
    with np.errstate(invalid="ignore"):
        def tower(t):
            h = tanh32(obs @ B[t + ".W1"].T + B[t + ".b1"])
            h = tanh32(h @ B[t + ".W2"].T + B[t + ".b2"])
            return h @ B[t + ".W3"].T + B[t + ".b3"]
        return tower("pi"), tower("vf")[:, 0]


def noise32(seed, env_index_base, step, n):
    """Box-Muller on two 24-bit uniforms in float32"""
    w = P.words(seed, [int(env_index_base) + i for i in range(n)], step)
    f = np.float32
    u1, u2 = ((w[:, 0] >> 8).astype(f) + f(0.5)) * f(1.0 / 16777216.0), ((w[:, 1] >> 8).astype(f) + f(0.5)) * f(1.0 / 16777216.0)
    r, th = np.sqrt(f(-2.0) * np.log(u1)), f(6.283185307179586) * u2
    return np.stack([r * np.cos(th), r * np.sin(th)], axis=1).astype(f)


def act32(flat, obs, seed=SEED, env_index_base=BASE, step=STEP, deterministic=False):
    """brs_policy_act in fp32 numpy -> {action, clipped, logp, value, noise}"""
    f = np.float32
    mean, value = forward32(flat, obs)
    n, ls = len(obs), np.asarray(flat, f)[-2:]
    z = np.zeros((n, 2), f) if deterministic else noise32(seed, env_index_base, step, n)
    with np.errstate(invalid="ignore"):
        action = np.exp(ls) * z + mean
        clipped = np.clip(action, f(-1.0), f(1.0))
    logp = np.zeros(n, f)
    for k in range(2):
        logp = logp + (f(-0.5) * z[:, k] * z[:, k] - ls[k] - f(0.9189385332046727))
    return dict(action=action, clipped=clipped, logp=logp, value=value, noise=z)


def bootstrap32(flat, terminal_obs, terminated, truncated, gamma, reward):
    """brs_rollout_bootstrap in fp32 numpy: the value of EVERY row is computed, as in the kernel, and only the rows to be bootstrapped
    take it"""
    out, rows = np.asarray(reward, np.float32).copy(), P.bootstrapped(terminated, truncated)
    v = forward32(flat, terminal_obs)[1]
    out[rows] = np.float32(gamma) * v[rows] + out[rows]
    return out


def gae32(c):
    return P.gae(c["reward"], c["value"], c["episode_start"], c["last_value"], c["last_done"], c["gamma"], c["lam"], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ forward / act cases
def saturated_rows(n):
    """the six saturated rows of a case of n rows, the first and the last row among them"""
    return [j * (n - 1) // (SATURATED - 1) for j in range(SATURATED)] if n >= 33 else []


_CASES = {}


def forward_case(n, kind):
    """obs [n][6] float32, the flat parameters, mean / value in fp64, the restatement's distance from them (the admission condition)
    and the number of rows redrawn"""
    key = ("forward", n, kind)
    if key in _CASES:
        return _CASES[key]
    params, rng = weights(kind), np.random.default_rng(4000 + n)
    draw = lambda k: (rng.standard_normal((k, 6)) * np.array(RL.OBS_SCALE)).astype(np.float32)
    obs, sat, redrawn = draw(n), saturated_rows(n), 0
    for _ in range(50):
        for j, row in enumerate(sat):
            obs[row, j] = np.float32(HUGE if j % 2 == 0 else -HUGE)
        mean, value = P.forward(params, obs)
        m32, v32 = forward32(params, obs)
        d = np.maximum(distance(m32, mean).max(axis=1), distance(v32, value))
        bad = d > GATE / 3
        if not bad.any():
            break
        obs[bad] = draw(int(bad.sum()))
        redrawn += int(bad.sum())
    else:
        raise AssertionError("could not condition the inputs")
    _CASES[key] = dict(n=n, kind=kind, params=params, obs=obs, mean=mean, value=value, saturated=sat, restatement=float(d.max()), redrawn=redrawn,
                       z=P.noise(SEED, BASE, STEP, n))
    return _CASES[key]


def check_act(c, out, what, z=None):
    """the outputs of one sampled brs_policy_act call on case c (dict of float32 arrays under KEYS) against fp64; z: the fp64 noise of
    the call where it is not the case's own (SEED, BASE, STEP).  -> {quantity: largest distance}"""
    ls = P.log_std_of(c["params"])
    action, clipped, logp = P.act_from(c["mean"], ls, out["noise"].astype(np.float64))
    d = dict(value=gate(out["value"], c["value"], f"{what} value"), noise=gate(out["noise"], c["z"] if z is None else z, f"{what} noise"),
             action=gate(out["action"], action, f"{what} action"), clipped=gate(out["clipped"], clipped, f"{what} clipped action"),
             logp=gate(out["logp"], logp, f"{what} logp"))
    assert np.abs(out["clipped"]).max() <= 1.0
    inside = np.abs(out["action"]) <= 1.0
    assert out["clipped"][inside].tobytes() == out["action"][inside].tobytes(), f"{what}: an action inside [-1, 1] was changed by the clip"
    assert (out["clipped"][~inside] == np.sign(out["action"][~inside])).all()
    return d


def check_deterministic(c, det0, det7, sampled, what):
    """two deterministic calls (step 0, step 7) and the sampled call on the same case"""
    ls = P.log_std_of(c["params"])
    assert det0["action"].tobytes() == det7["action"].tobytes(), f"{what}: the deterministic action depends on the step"
    d = dict(mean=gate(det0["action"], c["mean"], f"{what} mean (the deterministic action)"),
             logp_det=gate(det0["logp"], np.full(c["n"], -(ls[0] + ls[1]) - 2.0 * P.HALF_LOG_2PI), f"{what} deterministic logp"))
    gate(det0["clipped"], np.clip(c["mean"], -1.0, 1.0), f"{what} deterministic clipped action")
    for o in (det0, det7):
        assert not o["noise"].any() and not np.signbit(o["noise"]).any(), f"{what}: the deterministic noise is not all zeros"
        assert o["value"].tobytes() == sampled["value"].tobytes() and o["logp"].tobytes() == det0["logp"].tobytes()
    return d


def poisoned(c, row, how):
    """the case's observations with `row` poisoned: "nan" = all six features NaN, "inf" = feature row % 6 +inf"""
    obs = c["obs"].copy()
    if how == "nan":
        obs[row] = np.nan
    else:
        obs[row, row % 6] = np.inf
    return obs


def check_isolation(c, row, how, base, out, what):
    """`out`: the call on poisoned(c, row, how), `base`: the call on the case itself.  Every other row keeps its bytes; the poisoned
    row's mean-dependent outputs (action, clipped action, value) are NaN for NaN features and meet the gate for a +inf feature; its
    noise and logp depend on no observation and keep their bytes"""
    others = np.arange(c["n"]) != row
    for k in KEYS:
        assert out[k][others].tobytes() == base[k][others].tobytes(), f"{what}: {k} of another row changed"
    assert out["noise"][row].tobytes() == base["noise"][row].tobytes() and out["logp"][row].tobytes() == base["logp"][row].tobytes()
    if how == "nan":
        for k in ("action", "clipped", "value"):
            assert np.isnan(out[k][row]).all(), f"{what}: {k} of the poisoned row is {out[k][row]}, not NaN"
        return 0.0
    obs = poisoned(c, row, how)[row:row + 1]
    mean, value = P.forward(c["params"], obs)
    assert np.isfinite(mean).all() and np.isfinite(value).all()
    action = P.act_from(mean, P.log_std_of(c["params"]), out["noise"][row:row + 1].astype(np.float64))[0]
    assert np.isfinite(out["action"][row]).all() and np.isfinite(out["value"][row])
    return max(gate(out["action"][row:row + 1], action, f"{what} action"), gate(out["value"][row:row + 1], value, f"{what} value"))


def counter_case(name):
    """forward_case(65, init) under another seed, step or env_index_base, with the fp64 noise of all its rows"""
    key = ("counter", name)
    if key not in _CASES:
        kw = {**dict(seed=SEED, env_index_base=BASE, step=STEP), **COUNTERS[name]}
        _CASES[key] = dict(kw=kw, z=P.noise(kw["seed"], kw["env_index_base"], kw["step"], COUNTER_ROWS))
    return _CASES[key]


# ------------------------------------------------------------------------------------------------ bootstrap cases
def _flags(pattern, n, rng):
    term, trunc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    if pattern.startswith("lone"):
        trunc[int(pattern[4:])] = 1
    elif pattern == "both":
        term[:], trunc[:] = 1, 1
    elif pattern == "mixed":   # every pair of (0, 1, 2, 255) over the rows, shifted so that no pair is tied to a lane position
        values = np.array((0,) + FLAG_VALUES, np.uint8)
        i = np.arange(n)
        term, trunc = values[(i // 4 + i // 64) % 4], values[i % 4]
    elif pattern == "random":  # row 0 is bootstrapped whatever the draw: n = 1 would otherwise test nothing
        term, trunc = (rng.uniform(size=n) < 0.3).astype(np.uint8), (rng.uniform(size=n) < 0.5).astype(np.uint8)
        term[0], trunc[0] = 0, 1
    else:
        assert pattern == "none"
    return np.ascontiguousarray(term), np.ascontiguousarray(trunc)


def bootstrap_case(pattern, n, kind):
    """terminal_obs [n][6] (forward_case's admitted rows where the bootstrap applies, NaN in every other row: whether the simulator
    defines those is not this test's business, the kernel must not let them leak), the two flag arrays, reward, and the fp64 result"""
    key = ("bootstrap", pattern, n, kind)
    if key in _CASES:
        return _CASES[key]
    f = forward_case(n, kind)
    rng = np.random.default_rng(5000 + n)
    term, trunc = _flags(pattern, n, rng)
    rows = P.bootstrapped(term, trunc)
    tobs = f["obs"].copy()
    tobs[~rows] = np.nan
    reward = rng.standard_normal(n).astype(np.float32)
    _CASES[key] = dict(n=n, kind=kind, pattern=pattern, params=f["params"], terminal_obs=tobs, terminated=term, truncated=trunc, reward=reward,
                       rows=rows, want=P.bootstrap(f["params"], tobs, term, trunc, GAMMA, reward))
    return _CASES[key]


BOOTSTRAP_CASES = [(p, PATTERN_ROWS, "init") for p in PATTERNS] + [("random", n, kind) for n in RANDOM_FLAG_ROWS for kind in WEIGHT_SETS]


def check_bootstrap(c, reward, inputs, what):
    """`reward`: the buffer after the call; `inputs`: terminal_obs, terminated, truncated as they are after the call"""
    rows = c["rows"]
    d = gate(reward[rows], c["want"][rows], f"{what} bootstrapped rows") if rows.any() else 0.0
    assert reward[~rows].tobytes() == c["reward"][~rows].tobytes(), f"{what}: the reward of a row that is not bootstrapped changed"
    if c["pattern"] in ("none", "both"):
        assert reward.tobytes() == c["reward"].tobytes()
    for x, k in zip(inputs, ("terminal_obs", "terminated", "truncated")):
        assert x.tobytes() == c[k].tobytes(), f"{what}: {k} was written"
    return d


# ------------------------------------------------------------------------------------------------ GAE cases
def gae_case(T, N, gamma, lam, p_start):
    """reward, value [T][N], episode_start [T][N] (set with probability p_start, as 1, 2 or 255), last_value, last_done [N], the fp64
    adv / ret and the fp32 numpy recursion's distance from them (the admission condition)"""
    key = ("gae", T, N, gamma, lam, p_start)
    if key in _CASES:
        return _CASES[key]
    for attempt in range(20):
        rng = np.random.default_rng(6000 + 1000 * attempt + 100 * GAE_CASES.index((T, N, gamma, lam, p_start)) + T)
        f32 = lambda *s: rng.standard_normal(s).astype(np.float32)
        flag = lambda p, *s: ((rng.uniform(size=s) < p) * rng.choice(np.array(FLAG_VALUES, np.uint8), size=s)).astype(np.uint8)
        c = dict(T=T, N=N, gamma=gamma, lam=lam, reward=f32(T, N), value=f32(T, N), episode_start=flag(p_start, T, N), last_value=f32(N),
                 last_done=flag(0.1, N), attempt=attempt)
        c["adv"], c["ret"] = P.gae(c["reward"], c["value"], c["episode_start"], c["last_value"], c["last_done"], gamma, lam)
        a32, r32 = gae32(c)
        c["restatement"] = float(max(distance(a32, c["adv"]).max(), distance(r32, c["ret"]).max()))
        if c["restatement"] <= GATE / 2:
            break
    else:
        raise AssertionError("could not condition the inputs")
    _CASES[key] = c
    return c


def check_gae(c, adv, ret, what):
    d = dict(adv=gate(adv, c["adv"], f"{what} adv"), ret=gate(ret, c["ret"], f"{what} ret"))
    # ret is adv + value rounded once: half a unit in the last place of ret
    slack = 0.5 * np.spacing(np.abs(ret)).astype(np.float64)
    assert (np.abs(ret.astype(np.float64) - adv.astype(np.float64) - c["value"].astype(np.float64)) <= slack).all(), f"{what}: ret - adv != value"
    return d


# ------------------------------------------------------------------------------------------------ the rollout / learner contract
def contract_case():
    """forward_case(257, init) with what the learner needs next to it (advantages and returns as ref_learner.make_case draws them)"""
    key = ("contract",)
    if key not in _CASES:
        f = forward_case(CONTRACT_ROWS, "init")
        rng = np.random.default_rng(77)
        n = f["n"]
        _CASES[key] = dict(f, adv=(0.3 + 2.0 * rng.standard_normal(n)).astype(np.float32), ret=(3.0 + rng.standard_normal(n)).astype(np.float32))
    return _CASES[key]


def reference_alone(c):
    """the cost of storing the action in fp32, on the fp64 reference alone: the exact action mean + sigma z rounded to float32, its
    log-probability recomputed from the rounded action, against the log-probability from z: half an ulp of |action| over sigma, times
    |z|.  -> the largest distance"""
    ls = P.log_std_of(c["params"])
    action, _, logp = P.act_from(c["mean"], ls, c["z"])
    return float(distance(P.logp_of_action(c["mean"], ls, action.astype(np.float32)), logp).max())


def check_contract(c, out, what):
    """the act call's logp against the fp64 log-probability of its own stored fp32 action under the same parameters"""
    return gate(out["logp"], P.logp_of_action(c["mean"], P.log_std_of(c["params"]), out["action"]), f"{what} logp against the learner's recomputation")


def contract_statistics(c, action, logp_old):
    """approx_kl and the clip fraction of ref_learner.minibatch_loss in fp64 on all rows, with the given stored action and logp_old"""
    case = dict(params=c["params"], obs=c["obs"], act=np.asarray(action, np.float32), logp_old=np.asarray(logp_old, np.float32), adv=c["adv"],
                ret=c["ret"])
    g = RL.grad_buffer(case, np.arange(c["n"]), RL.Cfg())
    return float(g[RL.NPARAM + 3]), float(g[RL.NPARAM + 4])
