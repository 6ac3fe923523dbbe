"""tests/ref_sac.py and tests/sac_cases.py at the widths of BRS_ARCH_SAC_DEFAULT, SB3's default net_arch = [256, 256]:
what tests/test_sac_arch_cpu.py and tests/test_sac_arch_gpu.py share.

Both modules name their widths once, as module constants, and their functions look those up when they run.  So the restatement at
other widths is the SAME source executed a second time under another name, with the constants (and the two fixed-width helpers of
ref_offpolicy / ref_ddpg_learner they call, `critic` and `q_of`) replaced by the [256, 256] ones before anything is computed:

    S = the fp64 restatement (ref_sac's sample, act, sac_target, actor_grad, twin_critic_grad, TorchSAC, ...) on
        ref_offpolicy.forward(..., sizes) and ref_ddpg_learner.net(..., sizes)
    C = the cases (sac_cases' grad_case, act_case, target_case, chain_case, assert_branch_coverage, check_*, the Host* wrappers)

Every condition, margin, round limit and gate is therefore sac_cases' own, unchanged: 25-75 % of every hidden layer active, no
pre-activation within the margin of 0, |Q0 - Q1| >= margin, the raw log_std a margin from both clamps, no cancellation behind the b3
and temperature sums, the AMP rule of the act and target rows.  Only `weights` is written anew (sac_cases' reshapes the output layer
as [4][200]); it draws the same way -- torch's default init times 1 or 3 from the same seeds, the log-std biases shifted by -2, `spread`
with the log-std head times SPREAD and shifted by SPREAD_SHIFT (re-tuned for this head: see there).  The caches of the second
instance are its own, and the originals are not touched."""
import ctypes as C_
import importlib.util
import os
import sys
import types

import numpy as np

import ref_ddpg_learner as _RL
import ref_offpolicy as _R
from balance_robot_mujoco_rl_amd import _lib
from hostbuild import ROOT, compile_host

ARCH_ID, NET_ARCH = _lib.ARCH_SAC_DEFAULT, "sb3"
ACTOR_SIZES, CRITIC_SIZES = (_R.OBS, 256, 256, 2 * _R.ACT), (_R.OBS + _R.ACT, 256, 256, 1)
NA, NC = _R.nparam(ACTOR_SIZES), _R.nparam(CRITIC_SIZES)
assert (NA, NC) == (_lib.SAC256_NACTOR, _lib.SAC256_NCRITIC) == (68612, 68353)
HOST_DIR = os.path.join(ROOT, "tests", "sacarchhost")


def _second_instance(name, alias):
    """the source of module `name` executed again as module `alias`"""
    origin = importlib.util.find_spec(name).origin
    spec = importlib.util.spec_from_file_location(alias, origin)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[alias] = mod
    spec.loader.exec_module(mod)
    return mod


def _critic(flat, obs, act, hidden=False):
    x = np.concatenate([np.asarray(obs, np.float64), np.asarray(act, np.float64)], axis=1)
    r = _R.forward(flat, x, CRITIC_SIZES, False, hidden)
    return (r[0][:, 0], r[1], r[2]) if hidden else r[:, 0]


def _q_of(critic, obs, act, hidden=False):
    import torch
    r = _RL.net(critic, torch.cat([obs, act], dim=1), CRITIC_SIZES, False, hidden)
    return (r[0][:, 0], r[1], r[2]) if hidden else r[:, 0]


# ref_offpolicy and ref_ddpg_learner as the two modules see them: everything theirs, but the critic's fixed widths
R = types.SimpleNamespace(**{k: v for k, v in vars(_R).items() if not k.startswith("__")})
R.CRITIC_SIZES, R.NCRITIC, R.critic = CRITIC_SIZES, NC, _critic
RL = types.SimpleNamespace(**{k: v for k, v in vars(_RL).items() if not k.startswith("__")})
RL.NCRITIC, RL.q_of = NC, _q_of

S = _second_instance("ref_sac", "ref_sac_arch256")
S.R, S.RL, S.ACTOR_SIZES, S.NACTOR, S.NCRITIC = R, RL, ACTOR_SIZES, NA, NC

C = _second_instance("sac_cases", "sac_cases_arch256")
# SPREAD: the log-std head of `spread` is `init`'s times SPREAD, then shifted.  sac_cases' (60, -9) was tuned for the head of 200
# inputs: there the raw log_std of the conditioned rows has mean -5.3 and standard deviation 8.0, 3 % of the elements below -20 and
# 18 % above 2 (which is what saturates the tanh in enough rows).  The same factors on this head (256 inputs, another draw) give
# mean -11.3 and deviation 3.4: one element in 514 above the upper clamp, and assert_branch_coverage fails.  A larger scale reaches
# both clamps (x 200: deviation 11.7), but then the partial sums behind a raw log_std near 0 are tens in size, and plain fp32 -- this
# host build's k-ascending loop -- is up to 1.7e-5 from fp64 on the log_std output: a set on which no fp32 forward meets the gate.
# So the scale stays 60 and the SHIFT is one per component: -18 for the first, whose raw log_std then spreads around the lower
# clamp (a quarter of its elements below it), +6 for the second, most of which lies above the upper one: a row's tanh saturates
# where sigma is e^2 and |z| exceeds 1, a quarter of the rows.  That share has to be large: the redraws of the no-cancellation
# rule work against saturated rows, and which rows they leave differs between machines in the last bits of fp32 torch's
# pre-activations (with +3, one machine kept one saturated row of 33 and another none).  Tried on the fp64 reference's branch
# table alone: scales 60 to 300 with one shift, and 60 to 100 with pairs from (-15, -3) to (-18, 8); at (-18, 8) a gradient
# case cannot be conditioned.  The conditions and the round limits are sac_cases'.
SPREAD, SPREAD_SHIFT = 60.0, np.array([-18.0, 6.0], np.float32)
# The chain: with `init` as it is, about 8 % of the 1200 rows of a round have one of their 5120 pre-activations within the margin
# (6 % at the reference widths, with 3800), every redraw moves the later steps' weights by more than the margin, and 100 rounds
# do not end (the count goes from 110 to about 60).  The chain's set is `init` times CHAIN_SCALE with init's margin and
# temperature: the first layer's pre-activations are twice, the second's four times as far from 0 for the same margin.
CHAIN_KIND, CHAIN_SCALE = "init_x2", 2.0


SCALE = {"init": 1.0, "x3": 3.0, CHAIN_KIND: CHAIN_SCALE}
C.MARGIN[CHAIN_KIND], C.LOG_ENT_COEF[CHAIN_KIND] = C.MARGIN["init"], C.LOG_ENT_COEF["init"]


def _critic_pre(critic, obs, act, dtype=None):
    import torch
    dtype = torch.float64 if dtype is None else dtype
    with torch.no_grad():
        _, c1, c2 = _q_of(_RL._t(critic, dtype), _RL._t(obs, dtype), _RL._t(act, dtype), hidden=True)
        return torch.cat([c1, c2], dim=1).numpy()


def critic_weights(base):
    """critics [2 NC]: td3_cases.weights' draws (critic 0 after the actor from seed 7, critic 1 from seed 8) at these widths"""
    scale, rng = SCALE[base], np.random.default_rng(7)
    _R.init_params(_R.ACTOR_SIZES, rng, scale)   # (the DDPG actor's draw comes first in offpolicy_cases.weights)
    return np.concatenate([_R.init_params(CRITIC_SIZES, rng, scale), _R.init_params(CRITIC_SIZES, np.random.default_rng(8), scale)])


def weights(kind):
    """actor VECTOR [NA + 1], critics [2 NC]; sac_cases.weights at these widths"""
    base = "init" if kind == "spread" else kind
    actor = _R.init_params(ACTOR_SIZES, np.random.default_rng(17), SCALE[base])
    sl = _RL.block_slices(ACTOR_SIZES)
    w3, b3 = actor[sl["W3"]].reshape(4, ACTOR_SIZES[2]), actor[sl["b3"]]
    if kind != "spread":
        b3[2:] += np.float32(C.LOG_STD_SHIFT)
    else:
        w3[2:] *= np.float32(SPREAD)
        b3[2:] = b3[2:] * np.float32(SPREAD) + np.asarray(SPREAD_SHIFT, np.float32)
    return S.with_log_ent_coef(actor, C.LOG_ENT_COEF[kind]), critic_weights(base)


C.S, C.R, C.RL, C.NA, C.NC, C.HOST_DIR, C.weights = S, R, RL, NA, NC, HOST_DIR, weights
C.TC = types.SimpleNamespace(_critic_pre=_critic_pre)
C._LAYERS = np.cumsum([0, 256, 256, 256, 256, 256, 256])
# sac_cases.HOST_ROWS_MAX at these widths: one sh_actor_grad / one sh_twin_critic_grad of this host build takes 1.8 s / 1.3 s at 2,049
# rows and 6.6 s / 5.1 s at 8,193 on a CPU, over the 5 s a comparison may cost: the host build is compared up to 2,049 rows
C.HOST_ROWS_MAX = 2049


# ------------------------------------------------------------------------------------------------ the host build
def build_host(directory, arch="ArchSacDefault"):
    """g++ -> libsacarchhost.so of tests/sacarchhost for `arch` in `directory`, with sac_cases.build_host's signatures: the Host*
    wrappers of C drive it"""
    L = compile_host(directory, f"libsacarchhost_{arch}.so", os.path.join(HOST_DIR, "sacarchhost.cpp"), [f"SACARCH={arch}"])
    vp, i, f, u64, u32 = C_.c_void_p, C_.c_int, C_.c_float, C_.c_uint64, C_.c_uint32
    L.sh_act.restype, L.sh_act.argtypes = i, [vp, i, vp, u64, C_.c_int64, u32, i, i, vp, vp, vp, vp]
    L.sh_target.restype, L.sh_target.argtypes = i, [vp, vp, i, vp, vp, vp, f, u64, u32, vp, vp, vp, vp]
    L.sh_twin_critic_grad.restype, L.sh_twin_critic_grad.argtypes = i, [vp, i, vp, vp, vp, f, vp]
    L.sh_actor_grad.restype, L.sh_actor_grad.argtypes = i, [vp, vp, i, vp, u64, u32, i, f, vp, vp]
    L.sh_apply.restype, L.sh_apply.argtypes = i, [i, vp, vp, vp, vp, vp, C_.POINTER(_lib.BrsAdamConfig), C_.c_int64, f]
    L.sh_q.restype, L.sh_q.argtypes = i, [vp, i, vp, vp, vp]
    L.sh_argument_error.restype, L.sh_argument_error.argtypes = C_.c_char_p, [i, vp, vp, i, vp, vp, vp, f, vp, i]
    L.sh_sizes.restype, L.sh_sizes.argtypes = i, [C_.POINTER(i), C_.POINTER(i)]
    L.sh_known_arch.restype, L.sh_known_arch.argtypes = i, [i]
    return L


def host_q(L, critic, obs, act):
    q = np.zeros(len(obs), np.float32)
    assert L.sh_q(C._ptr(critic), len(obs), C._ptr(obs), C._ptr(act), C._ptr(q)) == 0
    return q


def edge_model(layer, unit, seed=5):
    """a model in which the layer after hidden layer `layer` (1 or 2) reads only `unit` of it, with a large weight: 256 has no padded
    unit, so the width's edge is the last real one.  -> actor vector, critics; the `init` weights with, for layer 1, every column of
    W2 but `unit` zeroed and that column times 8 (of the actor and both critics), for layer 2 the same on W3"""
    actor, critics = weights("init")
    actor, critics = actor.copy(), critics.copy()
    name = {1: "W2", 2: "W3"}[layer]
    for vec, sizes, at in ((actor, ACTOR_SIZES, 0), (critics, CRITIC_SIZES, 0), (critics, CRITIC_SIZES, NC)):
        sl = _RL.block_slices(sizes)[name]
        w = vec[at + sl.start:at + sl.stop].reshape(sizes[layer + 1], sizes[layer])
        keep = w[:, unit].copy() * np.float32(8.0)
        w[:] = 0.0
        w[:, unit] = keep
    return actor, critics
