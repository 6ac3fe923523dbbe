"""What the CPU and the GPU tests of TD3 share (tests/test_td3_cpu.py, tests/test_td3_gpu.py): the three weight vectors, the
gradient cases (ddpg_learner_cases.learner_case with its conditions extended to the second critic), the target cases
(offpolicy_cases.conditioned inputs used as next_obs) with the branch-coverage assertion, the six-step chain case, the trajectory rule
extended to the twin blocks, and the host build of the kernel source (tests/td3host).

The conditions of ddpg_learner_cases, for critic 1 on (obs, act) as for critic 0, checked on the fp64 yardstick alone, offending rows
redrawn jointly: 25 % to 75 % of every hidden layer active, no pre-activation within MARGIN[kind] of 0, fp32 torch's pre-activations
within a tenth of that, and no cancellation behind its b3 gradient (|sum t| >= 1/4 sum |t| for t = 2 (q1 - y) / m).  The target needs
no margin: every hard decision in it (both clamps, the minimum) is continuous in its inputs."""
import ctypes as C
import os

import numpy as np
import torch

import ref_ddpg_learner as RL
import ref_offpolicy as R
import ref_td3 as T3
from balance_robot_mujoco_rl_amd import _lib
from ddpg_learner_cases import ADAM, MARGIN, _bad_rows, _draw, _no_cancellation, block_distances, learner_case
from hostbuild import ROOT, _ptr, compile_host
from offpolicy_cases import GAMMA, SEED, _active_ok, conditioned, weights as _ddpg_weights

HOST_DIR = os.path.join(ROOT, "tests", "td3host")
NC, NA = R.NCRITIC, R.NACTOR
SB3_NOISE, TIGHT_NOISE = (0.2, 0.5), (0.2, 0.1)   # (policy_noise, noise_clip): SB3's defaults; a clip inside the noise's bulk
TARGET_ROWS_CPU = (1, 33, 257)
CHAIN_STEPS, CHAIN_ROWS, POLICY_DELAY = 6, 200, 2


def weights(kind):
    """actor [NACTOR], critics [2 NCRITIC]: actor and critic 0 are offpolicy_cases.weights(kind), critic 1 is drawn from seed 8"""
    actor, critic0 = _ddpg_weights(kind)
    critic1 = R.init_params(R.CRITIC_SIZES, np.random.default_rng(8), {"init": 1.0, "x3": 3.0}[kind])
    return actor, np.concatenate([critic0, critic1])


# ------------------------------------------------------------------------------------------------ gradient cases
def _critic_pre(critic, obs, act, dtype=torch.float64):
    """the hidden pre-activations of critic(obs, act) -> [m][200 + 150]"""
    with torch.no_grad():
        _, c1, c2 = RL.q_of(RL._t(critic, dtype), RL._t(obs, dtype), RL._t(act, dtype), hidden=True)
        return torch.cat([c1, c2], dim=1).numpy()


def _bad_rows_second(critic1, obs, act, margin):
    pre = _critic_pre(critic1, obs, act)
    near = (np.abs(pre) < margin).any(axis=1)
    far = (np.abs(_critic_pre(critic1, obs, act, torch.float32) - pre) > 0.1 * margin).any(axis=1)
    return near | far | ~_active_ok(pre[:, :200], pre[:, 200:])


_TWIN = {}


def twin_case(n, kind):
    """obs [n][6], act [n][2], y [n] (float32), actor and critics: learner_case(n, kind) with every condition holding for critic 1 too;
    computed once, never written afterwards"""
    key = (n, kind)
    if key in _TWIN:
        return _TWIN[key]
    base = learner_case(n, kind)
    actor, critics = weights(kind)
    assert actor.tobytes() == base["actor"].tobytes() and critics[:NC].tobytes() == base["critic"].tobytes()
    c0, c1, margin = critics[:NC], critics[NC:], MARGIN[kind]
    obs, act, y = base["obs"].copy(), base["act"].copy(), base["y"].copy()
    rng = np.random.default_rng(9000 + n)
    first = True
    for attempt in range(400):
        for rounds in range(200):
            bad = _bad_rows(actor, c0, obs, act, margin)[0] | _bad_rows_second(c1, obs, act, margin)
            if not bad.any():
                break
            first = False
            obs[bad], act[bad] = _draw(rng, int(bad.sum()))
        else:
            raise AssertionError("could not condition the inputs")
        if not first:   # rows changed: a y for them, by learner_case's rule
            y = (R.critic(c0, obs, act) + 0.5 + 0.5 * rng.standard_normal(n)).astype(np.float32)
        tq, tz = RL.row_terms(actor, c0, obs, act, y)
        tq1 = 2.0 * (R.critic(c1, obs, act) - y.astype(np.float64)) / n
        terms = (tq, tz[:, 0], tz[:, 1], tq1)
        ok = [_no_cancellation(t) for t in terms]
        if all(ok):
            break
        first = False
        if not ok[0]:
            continue   # a new z
        # redraw the rows that pull a sum towards zero: those whose term has the minority sign
        for t, good in zip(terms[1:], ok[1:]):
            if not good:
                minority = np.sign(t) != np.sign(t.sum())
                obs[minority], act[minority] = _draw(rng, int(minority.sum()))
    else:
        raise AssertionError("could not remove the cancellation")
    for c in (c0, c1):
        p64, p32 = _critic_pre(c, obs, act), _critic_pre(c, obs, act, torch.float32)
        assert np.abs(p64).min() >= margin and np.abs(p32 - p64).max() <= 0.1 * margin, (n, kind)
    _TWIN[key] = dict(obs=obs, act=act, y=y, actor=actor, critics=critics)
    return _TWIN[key]


_REFS = {}


def twin_references(n, kind):
    """the fp64 twin gradient of twin_case(n, kind) and fp32 torch's on the same inputs"""
    key = (n, kind)
    if key not in _REFS:
        c = twin_case(n, kind)
        _REFS[key] = (T3.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"]),
                      T3.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"], torch.float32))
    return _REFS[key]


def split_twin(g):
    """the twin buffer [2 NC + 4] -> the two single-critic buffers [NC + 2]"""
    g = np.asarray(g)
    return [np.concatenate([g[k * NC:(k + 1) * NC], g[2 * NC + 2 * k:2 * NC + 2 * k + 2]]) for k in (0, 1)]


# ------------------------------------------------------------------------------------------------ target cases
_TARGETS = {}


def target_case(m, kind, noise_pair, draw=0):
    """offpolicy_cases.conditioned(m, kind)'s obs as next_obs, its reward and done, the three weight vectors, and the fp64 reference
    (y, a', z and the quantities the branches are decided on); computed once"""
    key = (m, kind, noise_pair, draw)
    if key not in _TARGETS:
        c = conditioned(m, kind)
        actor, critics = weights(kind)
        y, a, z, parts = T3.td3_target(actor, critics, c["obs"], c["reward"], c["done"], GAMMA, noise_pair[0], noise_pair[1], SEED, draw, parts=True)
        _TARGETS[key] = dict(next_obs=c["obs"], reward=c["reward"], done=c["done"], actor=actor, critics=critics, y=y, a=a, z=z, parts=parts,
                             policy_noise=noise_pair[0], noise_clip=noise_pair[1], draw=draw)
    return _TARGETS[key]


def branch_counts(case):
    p, raw, clip, parts = case["parts"]["p"], case["parts"]["raw"], case["noise_clip"], case["parts"]
    return dict(noise_low=int((p < -clip).sum()), noise_high=int((p > clip).sum()), noise_in=int((np.abs(p) <= clip).sum()),
                action_low=int((raw < -1).sum()), action_high=int((raw > 1).sum()), action_in=int((np.abs(raw) <= 1).sum()),
                min_from_0=int((parts["q1"] < parts["q2"]).sum()), min_from_1=int((parts["q2"] < parts["q1"]).sum()),
                done_0=int((case["done"] == 0).sum()), done_1=int((case["done"] != 0).sum()))


def assert_branch_coverage(cases):
    """over `cases`, every branch of the target occurs on the fp64 reference: noise clipped low / high / not, action clamped low /
    high / not, the minimum from either critic, done 0 / 1"""
    total = {}
    for c in cases:
        for k, v in branch_counts(c).items():
            total[k] = total.get(k, 0) + v
    print("branches over the cases:", total)
    assert all(v > 0 for v in total.values()), total
    return total


def coverage_cases():
    """the two cases the issue found to cover every branch: x3 at m = 33 with the tight clip, x3 at m = 257 with SB3's pair"""
    return [target_case(33, "x3", TIGHT_NOISE), target_case(257, "x3", SB3_NOISE)]


# ------------------------------------------------------------------------------------------------ the six-step chain
_CHAIN = {}


def run_chain(t, case, noise_pair=SB3_NOISE, steps=CHAIN_STEPS, on_step=None):
    """`t`: a TorchTD3; the target of every step from the three targets as they are, draw = the step's index"""
    for s in range(steps):
        sl = slice(s * CHAIN_ROWS, (s + 1) * CHAIN_ROWS)
        y = t.td3_target(case["next_obs"][sl], case["reward"][sl], case["done"][sl], GAMMA, noise_pair[0], noise_pair[1], SEED, s)
        if on_step:
            on_step(sl)
        t.step(case["obs"][sl], case["act"][sl], y, between=(lambda: on_step(sl)) if on_step else None)
    return t.flats()


def chain_case(kind="init"):
    """six minibatches of 200 rows from the same initial weights such that no hidden pre-activation of the fp64 chain -- actor(obs),
    critic k(obs, act), critic 0(obs, actor(obs)), before the critics' pass and, on delayed steps, between it and the actor's --
    comes within the margin of 0 (rows redrawn until that holds), and where that chain ends in fp64 and in fp32 torch"""
    if kind in _CHAIN:
        return _CHAIN[kind]
    actor, critics = weights(kind)
    n, margin, rng = CHAIN_STEPS * CHAIN_ROWS, MARGIN[kind], np.random.default_rng(177)
    base = twin_case(1000, kind)
    extra = _draw(rng, n - 1000)
    case = dict(obs=np.concatenate([base["obs"], extra[0]]), act=np.concatenate([base["act"], extra[1]]), actor=actor, critics=critics,
                next_obs=_draw(rng, n)[0], reward=rng.standard_normal(n).astype(np.float32), done=(np.arange(n) % 3 == 1).astype(np.uint8))
    for _ in range(100):
        t = T3.TorchTD3(actor, critics, policy_delay=POLICY_DELAY, **ADAM)
        bad = np.zeros(n, bool)

        def look(sl):
            f = t.flats()
            pre0 = RL.preactivations(f["actor"], f["critics"][:NC], case["obs"][sl], case["act"][sl])
            pre1 = _critic_pre(f["critics"][NC:], case["obs"][sl], case["act"][sl])
            bad[sl] |= (np.abs(pre0).min(axis=1) < margin) | (np.abs(pre1).min(axis=1) < margin)
        case["ref64"] = run_chain(t, case, on_step=look)
        if not bad.any():
            break
        case["obs"][bad], case["act"][bad] = _draw(rng, int(bad.sum()))
    else:
        raise AssertionError("could not condition the chain")
    case["ref32"] = run_chain(T3.TorchTD3(actor, critics, torch.float32, policy_delay=POLICY_DELAY, **ADAM), case)
    _CHAIN[kind] = case
    return case


def check_chain(what, flats, case):
    """ddpg_learner_cases.check_trajectory's rule on the TD3 vectors, each critic a network of its own: per block of
    theta_end - theta_0, the distance from the fp64 chain is at most 4x fp32 torch's, the latter floored at its largest value over the
    blocks of the network; prints both"""
    worst = 0.0
    for netname, sizes, sl in (("actor", R.ACTOR_SIZES, slice(None)), ("critics", R.CRITIC_SIZES, slice(0, NC)), ("critics", R.CRITIC_SIZES, slice(NC, 2 * NC)),
                               ("actor_target", R.ACTOR_SIZES, slice(None)), ("critics_target", R.CRITIC_SIZES, slice(0, NC)),
                               ("critics_target", R.CRITIC_SIZES, slice(NC, 2 * NC))):
        start = case[netname.split("_")[0]][sl].astype(np.float64)
        d64 = case["ref64"][netname][sl] - start
        mine = block_distances(np.asarray(flats[netname], np.float64)[sl] - start, d64, sizes)
        t32 = block_distances(case["ref32"][netname][sl].astype(np.float64) - start, d64, sizes)
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
    """g++ -> libtd3host.so in `directory`, with its signatures applied"""
    L = compile_host(directory, "libtd3host.so", os.path.join(HOST_DIR, "td3host.cpp"))
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.th_td3_target.restype, L.th_td3_target.argtypes = i, [vp, vp, i, vp, vp, vp, f, f, f, C.c_uint64, C.c_uint32, vp, vp, vp]
    L.th_twin_critic_grad.restype, L.th_twin_critic_grad.argtypes = i, [vp, i, vp, vp, vp, vp]
    L.th_td_target.restype, L.th_td_target.argtypes = i, [vp, vp, i, vp, vp, vp, f, vp]
    L.th_critic_grad.restype, L.th_critic_grad.argtypes = i, [vp, i, vp, vp, vp, vp]
    L.th_actor_grad.restype, L.th_actor_grad.argtypes = i, [vp, vp, i, vp, vp]
    L.th_apply.restype, L.th_apply.argtypes = i, [i, vp, vp, vp, vp, vp, C.POINTER(_lib.BrsAdamConfig), C.c_int64, f]
    return L


def host_td3_target(L, actor_t, critics_t, next_obs, reward, done, gamma, policy_noise, noise_clip, seed, draw, extras=True):
    m = len(next_obs)
    y, a, z = np.zeros(m, np.float32), np.zeros((m, 2), np.float32), np.zeros((m, 2), np.float32)
    assert L.th_td3_target(_ptr(actor_t), _ptr(critics_t), m, _ptr(next_obs), _ptr(reward), _ptr(done), gamma, policy_noise, noise_clip, seed, draw,
                           _ptr(y), _ptr(a) if extras else None, _ptr(z) if extras else None) == 0
    return y, a, z


def host_twin_critic_grad(L, critics, obs, act, y):
    g = np.zeros(2 * NC + 4, np.float32)
    assert L.th_twin_critic_grad(_ptr(critics), len(obs), _ptr(obs), _ptr(act), _ptr(y), _ptr(g)) == 0
    return g


class HostTD3:
    """tests/td3host behind DeviceTD3Learner.step's surface, on numpy arrays"""

    def __init__(self, L, actor, critics, policy_delay=2, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005):
        self.L, self.cfg, self.tau, self.policy_delay = L, _lib.BrsAdamConfig(lr, betas[0], betas[1], eps), tau, policy_delay
        self.flat = {"actor": actor.copy(), "critics": critics.copy(), "actor_target": actor.copy(), "critics_target": critics.copy()}
        self.mom = {k: (np.zeros_like(self.flat[k]), np.zeros_like(self.flat[k])) for k in ("actor", "critics")}
        self.steps, self.n_updates = {"actor": 0, "critics": 0}, 0
        self.grad = {}

    def apply(self, name, grad, target):
        p, (m, v) = self.flat[name], self.mom[name]
        self.steps[name] += 1
        assert self.L.th_apply(p.size, _ptr(p), _ptr(grad), _ptr(m), _ptr(v), _ptr(self.flat[name + "_target"]) if target else None,
                               C.byref(self.cfg), self.steps[name], self.tau) == 0

    def td3_target(self, next_obs, reward, done, gamma, policy_noise, noise_clip, seed, draw):
        return host_td3_target(self.L, self.flat["actor_target"], self.flat["critics_target"], next_obs, reward, done, gamma, policy_noise,
                               noise_clip, seed, draw)[0]

    def step(self, obs, act, y):
        self.n_updates += 1
        delayed = self.n_updates % self.policy_delay == 0
        self.grad["critics"] = host_twin_critic_grad(self.L, self.flat["critics"], obs, act, y)
        self.apply("critics", self.grad["critics"], delayed)
        if delayed:
            g = np.zeros(NA + 2, np.float32)
            assert self.L.th_actor_grad(_ptr(self.flat["actor"]), _ptr(self.flat["critics"]), len(obs), _ptr(obs), _ptr(g)) == 0
            self.grad["actor"] = g
            self.apply("actor", g, True)
        return delayed
