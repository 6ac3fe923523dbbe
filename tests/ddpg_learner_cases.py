"""What the CPU and the GPU tests of the DDPG learner share (tests/test_ddpg_learner_cpu.py, tests/test_ddpg_learner_gpu.py): the
conditioned inputs (offpolicy_cases.conditioned plus the two conditions below, computed once per size and weight set), the
five-step trajectory case, the per-block distances, and the host build of the kernel source (tests/ddpglearnerhost).

Two conditions on top of offpolicy_cases.conditioned, both checked on the fp64 yardstick alone, offending rows redrawn:
  * no hidden pre-activation of actor(obs), critic(obs, act), critic(obs, actor(obs)) within MARGIN of 0, so that fp32 and fp64
    agree on every ReLU gate (one flipped gate moves a weight block by ~4e-3 of its norm: not a rounding error);
  * no cancellation in the sums behind the three b3 gradients: y = Q64(s, a) + 0.5 + 0.5 z, and |sum t| >= 1/4 sum |t| for
    t = 2 (q - y) / m and for the two components of d La / d (actor output before the tanh)."""
import ctypes as C
import os

import numpy as np
import torch

import ref_ddpg_learner as RL
import ref_offpolicy as R
from balance_robot_mujoco_rl_amd import _lib
from hostbuild import ROOT, _ptr, compile_host
from offpolicy_cases import _active_ok, conditioned

HOST_DIR = os.path.join(ROOT, "tests", "ddpglearnerhost")
MARGIN = {"init": 1e-5, "x3": 1e-4}
WEIGHT_SETS = ("init", "x3")
CPU_ROWS = (1, 33, 257, 1000)
GPU_ROWS = (1, 31, 32, 33, 127, 128, 129, 257, 1000)   # the wave edge, the workgroup edge, eight row-workgroups (and four splits)
# Where the weight-gradient kernels split the sample axis (brs_ddpg_learner.hpp: sample_split; mp = m padded to 128,
# nsplit = clamp(mp / 256, 1, 8), span = pad128(ceil(mp / nsplit)), nsplit recomputed as ceil(mp / span)):
#
#      m     mp   splits (rows each)   real rows in the last split   what it reaches
#  <= 384  <= 384  1                    -                             no split (GPU_ROWS up to 257)
#     385    512   256, 256             129                           first split size, two partial rows
#     513    640   384, 256             129                           uneven: the last split is shorter than span
#     769    896   384, 384, 128          1                           the last split is 127 padding rows and one real row
#    1000   1024   4 x 256              232                           the one split case of GPU_ROWS
#    1025   1152   3 x 384              257                           recomputed nsplit (3) below the requested 4
#    2049   2176   5 x 384, 256         129                           clamp at 8 requested, 6 launched, uneven
#    8192   8192   8 x 1024            1024                           MAX_SPLIT, the size DESIGN.md 7.6 / 7.7 quote timings for
#    8193   8320   7 x 1152, 256        129                           MAX_SPLIT and uneven
SPLIT_ROWS = (385, 513, 769, 1025, 2049, 8192, 8193)
SPLIT_X3_ROWS = (513, 2049, 8193)                      # the x3 weight set at the uneven geometries, at three depths
SPLIT_CASES = [(n, "init") for n in SPLIT_ROWS] + [(n, "x3") for n in SPLIT_X3_ROWS]
SPLIT_SEQUENCE = (8193, 513, 33, 2049, 769)            # 8 partial rows, then 2, none, 6, 3: what one handle is taken through
SPLIT_BIG = 8448                                       # max_batch of the large handle: ld != mp at every row of SPLIT_ROWS
HOST_ROWS_MAX = 2049                                   # the host build's plain loops are compared up to here (see the GPU tests)
SPLIT_TABLE = {384: (384, 384, 1), 385: (512, 256, 2), 513: (640, 384, 2), 769: (896, 384, 3), 1000: (1024, 256, 4),   # m: (mp, span, nsplit)
               1025: (1152, 384, 3), 2049: (2176, 384, 6), 8192: (8192, 1024, 8), 8193: (8320, 1152, 8)}
SPLIT_LAST_REAL = {385: 129, 513: 129, 769: 1, 1000: 232, 1025: 257, 2049: 129, 8192: 1024, 8193: 129}
GRAD_GATE = 1e-5            # per parameter block, ||g - g64|| / ||g64||: the project's learner tolerance
ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005)
_LAYERS = np.cumsum([0, 300, 200, 200, 150, 200, 150])   # the six hidden layers inside RL.preactivations' rows


def _draw(rng, k):
    return ((rng.standard_normal((k, 6)) * [1.5, 4.0, 0.5, 0.5, 0.5, 0.5]).astype(np.float32), rng.uniform(-1, 1, size=(k, 2)).astype(np.float32))


def _bad_rows(actor, critic, obs, act, margin):
    pre = RL.preactivations(actor, critic, obs, act)
    near = (np.abs(pre) < margin).any(axis=1)
    # a row on which fp32 torch itself is further than a tenth of the margin from fp64 (large inputs: the rounding of a
    # pre-activation of size 10 is 1e-6) is redrawn too, so that the assertion at the end of learner_case holds on what is left
    far = (np.abs(RL.preactivations(actor, critic, obs, act, torch.float32) - pre) > 0.1 * margin).any(axis=1)
    if far.any():
        print(f"  ({int(far.sum())} rows on which fp32 torch's pre-activations are more than {0.1 * margin:g} from fp64)")
    return near | far | ~_active_ok(*[pre[:, a:b] for a, b in zip(_LAYERS[:-1], _LAYERS[1:])]), int(near.sum())


def _no_cancellation(t):
    return abs(t.sum()) >= 0.25 * np.abs(t).sum()


_CASES = {}


def learner_case(n, kind):
    """obs [n][6], act [n][2], y [n] (float32) and the two weight vectors; computed once, never written afterwards"""
    key = (n, kind)
    if key in _CASES:
        return _CASES[key]
    base = conditioned(n, kind)
    actor, critic, margin = base["actor"], base["critic"], MARGIN[kind]
    obs, act = base["obs"].copy(), base["act"].copy()
    rng = np.random.default_rng(5000 + n)
    for attempt in range(400):
        for rounds in range(200):
            bad, near = _bad_rows(actor, critic, obs, act, margin)
            if rounds == 0 and attempt == 0:
                print(f"n={n} {kind}: {near} rows within {margin:g} of a ReLU's zero on the first draw")
            if not bad.any():
                break
            obs[bad], act[bad] = _draw(rng, int(bad.sum()))
        else:
            raise AssertionError("could not condition the inputs")
        q64 = R.critic(critic, obs, act)
        y = (q64 + 0.5 + 0.5 * rng.standard_normal(n)).astype(np.float32)
        tq, tz = RL.row_terms(actor, critic, obs, act, y)
        ok = _no_cancellation(tq), _no_cancellation(tz[:, 0]), _no_cancellation(tz[:, 1])
        if all(ok):
            break
        # redraw the rows that pull a sum towards zero: those whose term has the minority sign
        if not ok[0]:
            continue   # a new z
        for k in (0, 1):
            if not ok[k + 1]:
                minority = np.sign(tz[:, k]) != np.sign(tz[:, k].sum())
                obs[minority], act[minority] = _draw(rng, int(minority.sum()))
    else:
        raise AssertionError("could not remove the cancellation")
    # fp32 agrees with fp64 on every gate, with room: its pre-activations are within a tenth of the margin
    p64, p32 = RL.preactivations(actor, critic, obs, act), RL.preactivations(actor, critic, obs, act, torch.float32)
    assert np.abs(p32 - p64).max() <= 0.1 * margin, (n, kind, float(np.abs(p32 - p64).max()))
    _CASES[key] = dict(obs=obs, act=act, y=y, actor=actor, critic=critic)
    return _CASES[key]


def block_distances(g, g64, sizes):
    """{block: ||g - g64|| / ||g64||} over the six parameter blocks"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return {name: float(np.linalg.norm(g[sl] - g64[sl]) / np.linalg.norm(g64[sl])) for name, sl in RL.block_slices(sizes).items()}


_REFS = {}


def references(n, kind):
    """the fp64 gradients of learner_case(n, kind) and fp32 torch's on the same inputs: (critic64, actor64, critic32, actor32)"""
    key = (n, kind)
    if key not in _REFS:
        c = learner_case(n, kind)
        _REFS[key] = (RL.critic_grad(c["critic"], c["obs"], c["act"], c["y"]), RL.actor_grad(c["actor"], c["critic"], c["obs"]),
                      RL.critic_grad(c["critic"], c["obs"], c["act"], c["y"], torch.float32),
                      RL.actor_grad(c["actor"], c["critic"], c["obs"], torch.float32))
    return _REFS[key]


def check_gradient(what, g, g64, g32, sizes, stat_gate):
    """the gate of the issue: every block within GRAD_GATE of fp64, the two statistics within offpolicy_cases.gate; prints the largest
    distance next to fp32 torch's on the same inputs; -> (mine, torch32)"""
    n = R.nparam(sizes)
    mine, t32 = block_distances(g[:n], g64[:n], sizes), block_distances(g32[:n], g64[:n], sizes)
    worst = max(mine, key=mine.get)
    print(f"{what}: largest block distance from fp64 {mine[worst]:.3g} ({worst}); fp32 torch {max(t32.values()):.3g}")
    stat_gate(g[n:], g64[n:], what + " statistics")
    assert max(mine.values()) <= GRAD_GATE, (what, mine)
    return max(mine.values()), max(t32.values())


# ------------------------------------------------------------------------------------------------ the five-step case
STEP_ROWS, STEPS, GAMMA = 200, 5, 0.99
_TRAJ = {}


def _run_trajectory(t, case, chain, on_step=None):
    for s in range(STEPS):
        sl = slice(s * STEP_ROWS, (s + 1) * STEP_ROWS)
        y = t.td_target(case["next_obs"][sl], case["reward"][sl], case["done"][sl], GAMMA) if chain else case["y"][sl]
        if on_step:
            on_step(sl, "before")
        t.critic_step(case["obs"][sl], case["act"][sl], y)
        if on_step:
            on_step(sl, "between")   # the actor pass runs on the old actor and the updated critic
        t.actor_step(case["obs"][sl])
    return t.flats()


def trajectory_case(kind="init", chain=False):
    """five minibatches of 200 rows from the same initial weights such that no pre-activation of the fp64 trajectory comes within the
    margin of 0 in any step (rows redrawn until that holds), and where that trajectory ends in fp64 and in fp32 torch.  chain=False:
    y is given; chain=True: y of every step is the TD target of (next_obs, reward, done) from the two target networks as they are."""
    key = (kind, chain)
    if key in _TRAJ:
        return _TRAJ[key]
    c = learner_case(1000, kind)
    rng, margin = np.random.default_rng(77 + chain), MARGIN[kind]
    case = dict(obs=c["obs"].copy(), act=c["act"].copy(), y=c["y"].copy(), actor=c["actor"], critic=c["critic"],
                next_obs=_draw(rng, 1000)[0], reward=rng.standard_normal(1000).astype(np.float32), done=(np.arange(1000) % 3 == 1).astype(np.uint8))
    for _ in range(100):
        t = RL.TorchDDPG(c["actor"], c["critic"], **ADAM)
        bad = np.zeros(1000, bool)

        def look(sl, when):
            f = t.flats()
            bad[sl] |= np.abs(RL.preactivations(f["actor"], f["critic"], case["obs"][sl], case["act"][sl])).min(axis=1) < margin
        case["ref64"] = _run_trajectory(t, case, chain, look)
        if not bad.any():
            break
        k = int(bad.sum())
        case["obs"][bad], case["act"][bad] = _draw(rng, k)
        case["y"][bad] = (R.critic(c["critic"], case["obs"][bad], case["act"][bad]) + 0.5 + 0.5 * rng.standard_normal(k)).astype(np.float32)
    else:
        raise AssertionError("could not condition the trajectory")
    case["ref32"] = _run_trajectory(RL.TorchDDPG(c["actor"], c["critic"], torch.float32, **ADAM), case, chain)
    _TRAJ[key] = case
    return case


def check_trajectory(what, flats, case):
    """per block of theta_5 - theta_0: the distance from fp64 is at most 4x fp32 torch's on the same inputs, the latter floored at
    its own largest value over the blocks of the network (DESIGN.md 7.4's rule); prints both"""
    worst = 0.0
    for netname, sizes in (("actor", R.ACTOR_SIZES), ("critic", R.CRITIC_SIZES), ("actor_target", R.ACTOR_SIZES), ("critic_target", R.CRITIC_SIZES)):
        start = case[netname.split("_")[0]].astype(np.float64)
        d64 = case["ref64"][netname] - start
        mine = block_distances(np.asarray(flats[netname], np.float64) - start, d64, sizes)
        t32 = block_distances(case["ref32"][netname].astype(np.float64) - start, d64, sizes)
        floor = max(t32.values())
        for b in mine:
            print(f"{what} {netname}.{b}: |d - d64| / |d64| = {mine[b]:.3g}, fp32 torch {t32[b]:.3g} (gate 4 x {floor:.3g})")
            worst = max(worst, mine[b] / floor)
        for b in mine:
            assert mine[b] <= 4 * floor, (what, netname, b, mine[b], t32[b], floor)
    return worst


# ------------------------------------------------------------------------------------------------ the host build
def build_host(directory):
    """g++ -> libddpglearnerhost.so in `directory`, with its signatures applied"""
    L = compile_host(directory, "libddpglearnerhost.so", os.path.join(HOST_DIR, "ddpglearnerhost.cpp"))
    vp, i = C.c_void_p, C.c_int
    L.dh_critic_grad.restype, L.dh_critic_grad.argtypes = i, [vp, i, vp, vp, vp, vp]
    L.dh_actor_grad.restype, L.dh_actor_grad.argtypes = i, [vp, vp, i, vp, vp]
    L.dh_apply.restype, L.dh_apply.argtypes = i, [i, vp, vp, vp, vp, vp, C.POINTER(_lib.BrsAdamConfig), C.c_int64, C.c_float]
    L.dh_sample_split.restype, L.dh_sample_split.argtypes = None, [i, C.POINTER(i * 3)]
    L.dh_split_sweep.restype, L.dh_split_sweep.argtypes = C.c_longlong, [i, i, C.POINTER(i), C.POINTER(C.c_uint)]
    L.dh_adam_pair.restype, L.dh_adam_pair.argtypes = None, [i, vp, C.POINTER(_lib.BrsAdamConfig), C.c_int64] + [vp] * 6
    return L


def host_critic_grad(L, critic, obs, act, y):
    g = np.zeros(RL.NCRITIC + 2, np.float32)
    assert L.dh_critic_grad(_ptr(critic), len(obs), _ptr(obs), _ptr(act), _ptr(y), _ptr(g)) == 0
    return g


def host_actor_grad(L, actor, critic, obs):
    g = np.zeros(RL.NACTOR + 2, np.float32)
    assert L.dh_actor_grad(_ptr(actor), _ptr(critic), len(obs), _ptr(obs), _ptr(g)) == 0
    return g


def adam_config(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, **_):
    return _lib.BrsAdamConfig(lr, betas[0], betas[1], eps)


class HostDDPG:
    """tests/ddpglearnerhost behind DeviceDDPGLearner.step's surface, on numpy arrays"""

    def __init__(self, L, actor, critic, **adam):
        self.L, self.cfg, self.tau = L, adam_config(**adam), adam.get("tau", 0.005)
        self.flat = {"actor": actor.copy(), "critic": critic.copy(), "actor_target": actor.copy(), "critic_target": critic.copy()}
        self.mom = {k: (np.zeros_like(self.flat[k]), np.zeros_like(self.flat[k])) for k in ("actor", "critic")}
        self.steps = {"actor": 0, "critic": 0}

    def apply(self, name, grad, target=True):
        p, (m, v) = self.flat[name], self.mom[name]
        self.steps[name] += 1
        assert self.L.dh_apply(p.size, _ptr(p), _ptr(grad), _ptr(m), _ptr(v), _ptr(self.flat[name + "_target"]) if target else None,
                               C.byref(self.cfg), self.steps[name], self.tau) == 0

    def step(self, obs, act, y):
        self.apply("critic", host_critic_grad(self.L, self.flat["critic"], obs, act, y))
        self.apply("actor", host_actor_grad(self.L, self.flat["actor"], self.flat["critic"], obs))
