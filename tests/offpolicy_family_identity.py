"""Inputs and runners of tests/test_offpolicy_family_identity_{gpu,cpu}.py and tools/gen_offpolicy_family_identity.py: every kernel of
the off-policy family (brs_offpolicy.hip, brs_ddpg_learner.hip) through the public Python classes, and every entry point of its host
mirrors (tests/offpolicyhost, ddpglearnerhost, td3host, sachost, sacarchhost at both SACARCH values), on the case builders the other
tests of this code use.  The sha256 of each output's bytes, recorded with one build, is the yardstick for a change that must keep every
floating-point operation with its operands and its order (tests/golden/offpolicy_family_identity_parent.json).  Test infrastructure.

Device groups (GROUPS), n = m = 257 (two workgroups and one row) unless said otherwise:
  act_q          DDPG act sampled with mean and noise, and random; SAC act sampled, deterministic and random; brs_ddpg_q; weight sets
                 init and x3; the SAC calls and q at both architectures
  targets        DDPG (init, x3), TD3 with next_action and noise (x3, SB3's noise pair), SAC with every optional output and with none
                 (spread: every branch of the sample), at both architectures
  critic_grads   m = 257 (no split) and 769 (three splits, ONE real row in the last) on handles of max_batch 896 and 8,448 (ld != mp):
                 critic_grad, twin_critic_grad on a twin handle, brs_sac_twin_critic_grad at both architectures
  actor_grads    the same rows and handles: the DDPG actor, the SAC actor with learn_alpha on and off at both architectures
  apply          one Adam + Polyak step from the m = 257 critic gradient, with a target and with target = null
  replay         add at n = 8 (the 16-byte path) and n = 6 (the scalar path), every combination of the two end flags among the envs;
                 sample m = 257 with idx
  sizes          brs_ddpg_learner_scratch's byte count for the four creates at max_batch 1, 129 and 8,448
Every input is offpolicy_cases.conditioned(rows, kind) -- obs, act, done, and its reward as reward and as y -- next to the weight vectors
of the case modules: those are decided by seeded numpy generators and fp64 numpy alone and come out the same on every machine, which
the gradient cases of ddpg_learner_cases / td3_cases / sac_cases (rows redrawn on what fp32 torch computes) do not.
Host groups (HOST_GROUPS): the same calls of the five host builds at rows 1, 33 and 257, the stand-alone programs' lines for a step of
each State, and the handle sizes as the sizing function of brs_sac.hpp (handle_size) returns them."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import ddpg_learner_cases as LC
import offpolicy_cases as OC
import sac_arch_cases as A
import sac_cases as SC
import td3_cases as TC

N = 257
KINDS = ("init", "x3")
GRAD_ROWS = (257, 769)
MAX_BATCHES = (896, LC.SPLIT_BIG)
SIZE_BATCHES = (1, 129, 8448)
HOST_ROWS = (1, 33, 257)
BASE = 5
GROUPS = ("act_q", "targets", "critic_grads", "actor_grads", "apply", "replay", "sizes")
HOST_GROUPS = ("offpolicyhost", "ddpglearnerhost", "td3host", "sachost", "sacarchhost/ArchReference", "sacarchhost/ArchSacDefault", "steps", "sizing")
# the SAC cases per architecture: (tag, case module, net_arch of the Python classes)
ARCHS = (("ref", SC, "reference"), ("sb3", A.C, "sb3"))
assert LC.SPLIT_TABLE[769] == (896, 384, 3) and LC.SPLIT_LAST_REAL[769] == 1


def inputs(n, kind="init"):
    """obs [n][6], act [n][2], reward (also used as y) [n], done [n] of offpolicy_cases.conditioned; `spread` takes init's rows"""
    c = OC.conditioned(n, "x3" if kind == "x3" else "init")
    return c["obs"], c["act"], c["reward"], c["done"]


def digest(a):
    return {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def _text(s):
    return np.frombuffer(s.encode(), np.uint8)


# ------------------------------------------------------------------------------------------------ the device
def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _empty(*shape):
    import torch
    return torch.empty(shape, dtype=torch.float32, device="cuda")


def act_q():
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGNets, DeviceSACNets
    out = {}
    ddpg = DeviceDDPGNets(device=0, seed=OC.SEED, env_index_base=BASE)
    for kind in KINDS:
        c = OC.conditioned(N, kind)
        obs, mean, noise = _cuda(c["obs"]), _empty(N, 2), _empty(N, 2)
        out[f"ddpg/{kind}/action"] = _np(ddpg.act(_cuda(c["actor"]), obs, 3, 0.1, mean=mean, noise=noise))
        out[f"ddpg/{kind}/mean"], out[f"ddpg/{kind}/noise"] = _np(mean), _np(noise)
        out[f"ddpg/{kind}/q"] = _np(ddpg.q(_cuda(c["critic"]), obs, _cuda(c["act"])))
    action, mean, noise = _empty(N, 2), _empty(N, 2), _empty(N, 2)
    ddpg.act(None, None, 3, 0.1, random=True, out=action, mean=mean, noise=noise)
    out.update({"ddpg/random/action": _np(action), "ddpg/random/mean": _np(mean), "ddpg/random/noise": _np(noise)})
    ddpg.close()
    for tag, cases, net_arch in ARCHS:
        nets = DeviceSACNets(device=0, seed=OC.SEED, env_index_base=BASE, net_arch=net_arch)
        for kind in KINDS:
            actor, obs = _cuda(cases.weights(kind)[0]), _cuda(inputs(N, kind)[0])
            extras = {k: _empty(N, 2) for k in ("mean", "log_std", "noise")}
            out[f"sac_{tag}/{kind}/sampled/action"] = _np(nets.act(actor, obs, 3, **extras))
            out.update({f"sac_{tag}/{kind}/sampled/{k}": _np(v) for k, v in extras.items()})
            out[f"sac_{tag}/{kind}/deterministic/action"] = _np(nets.act(actor, obs, 3, deterministic=True))
            critics = cases.weights(kind)[1]
            if tag != "ref":   # (the reference critic's q is ddpg/<kind>/q)
                out[f"sac_{tag}/{kind}/q"] = _np(nets.q(_cuda(critics[:cases.NC]), obs, _cuda(inputs(N, kind)[1])))
        extras = {k: _empty(N, 2) for k in ("out", "mean", "log_std", "noise")}
        nets.act(None, None, 3, random=True, **extras)
        out.update({f"sac_{tag}/random/{k}": _np(v) for k, v in extras.items()})
        nets.close()
    return out


def targets():
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGNets, DeviceSACNets
    out = {}
    ddpg = DeviceDDPGNets(device=0, seed=OC.SEED)
    for kind in KINDS:
        c = OC.conditioned(N, kind)
        out[f"ddpg/{kind}/y"] = _np(ddpg.td_target(_cuda(c["actor"]), _cuda(c["critic"]), _cuda(c["obs"]), _cuda(c["reward"]), _cuda(c["done"]), OC.GAMMA))
    obs, _, reward, done = inputs(N, "x3")
    args = [_cuda(a) for a in (*TC.weights("x3"), obs, reward, done)]
    next_action, noise = _empty(N, 2), _empty(N, 2)
    out["td3/y"] = _np(ddpg.td3_target(*args, OC.GAMMA, *TC.SB3_NOISE, 0, next_action=next_action, noise=noise))
    out["td3/next_action"], out["td3/noise"] = _np(next_action), _np(noise)
    out["td3/y_alone"] = _np(ddpg.td3_target(*args, OC.GAMMA, *TC.SB3_NOISE, 0))
    ddpg.close()
    for tag, cases, net_arch in ARCHS:
        nets = DeviceSACNets(device=0, seed=OC.SEED, net_arch=net_arch)
        obs, _, reward, done = inputs(N, "spread")
        args = [_cuda(a) for a in (*cases.weights("spread"), obs, reward, done)]
        extras = dict(next_action=_empty(N, 2), logp=_empty(N), noise=_empty(N, 2))
        out[f"sac_{tag}/y"] = _np(nets.sac_target(*args, OC.GAMMA, 0, **extras))
        out.update({f"sac_{tag}/{k}": _np(v) for k, v in extras.items()})
        out[f"sac_{tag}/y_alone"] = _np(nets.sac_target(*args, OC.GAMMA, 0))
        nets.close()
    return out


def _learners(max_batch):
    """the four kinds of handle at `max_batch`: DDPG, TD3 and SAC at both architectures"""
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGLearner, DeviceSACLearner, DeviceTD3Learner
    return DeviceDDPGLearner(device=0, max_batch=max_batch), DeviceTD3Learner(device=0, max_batch=max_batch), \
        {tag: DeviceSACLearner(device=0, max_batch=max_batch, seed=OC.SEED, net_arch=net_arch) for tag, _, net_arch in ARCHS}


def critic_grads():
    out = {}
    for max_batch in MAX_BATCHES:
        ddpg, td3, sac = _learners(max_batch)
        for m in GRAD_ROWS:
            rows = [_cuda(a) for a in inputs(m)[:3]]
            out[f"b{max_batch}/m{m}/ddpg"] = _np(ddpg.critic_grad(_cuda(OC.weights("init")[1]), *rows))
            out[f"b{max_batch}/m{m}/td3"] = _np(td3.twin_critic_grad(_cuda(TC.weights("init")[1]), *rows))
            for tag, cases, _ in ARCHS:
                out[f"b{max_batch}/m{m}/sac_{tag}"] = _np(sac[tag].twin_critic_grad(_cuda(cases.weights("init")[1]), *rows))
        for lrn in (ddpg, td3, *sac.values()):
            lrn.close()
    return out


def actor_grads():
    out = {}
    for max_batch in MAX_BATCHES:
        ddpg, td3, sac = _learners(max_batch)
        for m in GRAD_ROWS:
            obs = _cuda(inputs(m)[0])
            out[f"b{max_batch}/m{m}/ddpg"] = _np(ddpg.actor_grad(*[_cuda(w) for w in OC.weights("init")], obs))
            out[f"b{max_batch}/m{m}/td3"] = _np(td3.actor_grad(*[_cuda(w) for w in TC.weights("init")], obs))
            for tag, cases, _ in ARCHS:
                for kind in ("init",) + (("spread",) if m == N else ()):
                    args = [_cuda(w) for w in cases.weights(kind)]
                    for learn_alpha in (True, False):
                        sac[tag].learn_alpha = learn_alpha
                        out[f"b{max_batch}/m{m}/sac_{tag}/{kind}/alpha_{int(learn_alpha)}"] = _np(sac[tag].actor_grad(*args, obs, 0))
        for lrn in (ddpg, td3, *sac.values()):
            lrn.close()
    return out


def apply():
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGLearner
    out, w, rows = {}, OC.weights("init")[1], inputs(N)[:3]
    for name, with_target in (("target", True), ("null", False)):
        lrn = DeviceDDPGLearner(device=0, max_batch=N, **LC.ADAM)
        critic, target = _cuda(w), _cuda(w * np.float32(0.5))
        lrn.critic_grad(critic, *[_cuda(a) for a in rows])
        lrn.apply_critic(critic, target if with_target else None)
        out.update({f"{name}/params": _np(critic), f"{name}/m": _np(lrn.m_critic), f"{name}/v": _np(lrn.v_critic), f"{name}/polyak": _np(target)})
        lrn.close()
    return out


def replay():
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceReplayBuffer
    import torch
    out = {}
    for n in (8, 6):
        buf = DeviceReplayBuffer(n, 3, device=0, seed=OC.SEED)
        steps = OC.env_steps(n, 4)   # the buffer wraps once; the flags of env i at step t are combination (i + t) % 4
        assert all({(int(a), int(b)) for a, b in zip(s["terminated"] != 0, s["truncated"])} == {(0, 0), (0, 1), (1, 0), (1, 1)} for s in steps)
        for s in steps:
            buf.add(*[_cuda(s[k]) for k in OC.ADD_ORDER])
        for k in ("obs", "next_obs", "action", "reward", "done"):
            out[f"n{n}/{k}"] = _np(getattr(buf, k))
        idx = torch.empty((N, 2), dtype=torch.int32, device="cuda")
        for k, v in zip(("obs", "next_obs", "action", "reward", "done"), buf.sample(N, idx=idx)):
            out[f"n{n}/sample/{k}"] = _np(v)
        out[f"n{n}/sample/idx"] = _np(idx)
    return out


def sizes():
    from balance_robot_mujoco_rl_amd.offpolicy import DeviceDDPGLearner, DeviceSACLearner, DeviceTD3Learner
    makes = {"ddpg": lambda b: DeviceDDPGLearner(device=0, max_batch=b), "twin": lambda b: DeviceTD3Learner(device=0, max_batch=b),
             "sac_ref": lambda b: DeviceSACLearner(device=0, max_batch=b), "sac_sb3": lambda b: DeviceSACLearner(device=0, max_batch=b, net_arch="sb3")}
    out = {}
    for name, make in makes.items():
        got = []
        for b in SIZE_BATCHES:
            lrn = make(b)
            got.append(lrn.scratch()[1])
            lrn.close()
        out[name] = np.array(got, np.int64)
    return out


def run(group):
    """-> {output name: numpy array} of one group of GROUPS, on the device"""
    out = {"act_q": act_q, "targets": targets, "critic_grads": critic_grads, "actor_grads": actor_grads, "apply": apply, "replay": replay,
           "sizes": sizes}[group]()
    return {f"{group}/{k}": np.ascontiguousarray(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ the host mirrors
def _adam():
    return LC.adam_config(**LC.ADAM)


def _host_apply(fn, grad, n):
    """one Adam + Polyak step of `fn` (dh_apply, th_apply, sh_apply) on a ramp of parameters from the first n of `grad`"""
    p = np.linspace(-1, 1, n).astype(np.float32)
    m, v, t, cfg = np.zeros(n, np.float32), np.zeros(n, np.float32), (p * np.float32(0.5)).copy(), _adam()
    assert fn(n, OC._ptr(p), OC._ptr(grad), OC._ptr(m), OC._ptr(v), OC._ptr(t), C.byref(cfg), 1, 0.005) == 0
    return {"params": p, "m": m, "v": v, "polyak": t}


def host_offpolicy(directory):
    L, out = OC.build_host(directory), {}
    for n in HOST_ROWS:
        c = OC.conditioned(n, "init")
        for k, v in zip(("action", "mean", "noise"), OC.host_act(L, c["actor"], c["obs"], OC.SEED, BASE, 3, 0.1)):
            out[f"oh_act/n{n}/{k}"] = v
        for k, v in zip(("action", "mean", "noise"), OC.host_act(L, None, None, OC.SEED, BASE, 3, 0.1, random=True, n=n)):
            out[f"oh_act/n{n}/random/{k}"] = v
        out[f"oh_q/n{n}"] = OC.host_q(L, c["critic"], c["obs"], c["act"])
        out[f"oh_td_target/n{n}"] = OC.host_td_target(L, c["actor"], c["critic"], c["obs"], c["reward"], c["done"], OC.GAMMA)
    for n in (8, 6):
        buf = OC.HostBuffer(L, n, 3)
        for s in OC.env_steps(n, 4):
            buf.add(s)
        for k, v in zip(("obs", "next_obs", "action", "reward", "done"), buf.arrays):
            out[f"oh_replay_add/n{n}/{k}"] = v
        got, idx = buf.sample(N)
        for k, v in zip(("obs", "next_obs", "action", "reward", "done", "idx"), (*got, idx)):
            out[f"oh_replay_sample/n{n}/{k}"] = v
    return out


def host_ddpg_learner(directory):
    L, out = LC.build_host(directory), {}
    for n in HOST_ROWS:
        (actor, critic), (obs, act, y, _) = OC.weights("init"), inputs(n)
        out[f"dh_critic_grad/n{n}"] = LC.host_critic_grad(L, critic, obs, act, y)
        out[f"dh_actor_grad/n{n}"] = LC.host_actor_grad(L, actor, critic, obs)
    for k, v in _host_apply(L.dh_apply, out["dh_critic_grad/n257"], LC.RL.NCRITIC).items():
        out[f"dh_apply/{k}"] = v
    split = (C.c_int * 3)()
    rows = []
    for m in (1, 384, 385, 769, 8193, 1 << 22):
        L.dh_sample_split(m, C.byref(split))
        rows.append(list(split))
    out["dh_sample_split"] = np.array(rows, np.int32)
    first, mask = C.c_int(), C.c_uint()
    out["dh_split_sweep"] = np.array([L.dh_split_sweep(1, 1 << 16, C.byref(first), C.byref(mask)), first.value, mask.value], np.int64)
    return out


def host_td3(directory):
    L, out = TC.build_host(directory), {}
    for n in HOST_ROWS:
        (actor, critics), (obs, act, reward, done) = TC.weights("x3"), inputs(n, "x3")
        for extras in (True, False):
            got = TC.host_td3_target(L, actor, critics, obs, reward, done, OC.GAMMA, *TC.SB3_NOISE, OC.SEED, 0, extras=extras)
            for k, v in zip(("y", "next_action", "noise"), got):
                out[f"th_td3_target/n{n}/extras_{int(extras)}/{k}"] = v
        out[f"th_td_target/n{n}"] = np.zeros(n, np.float32)
        assert L.th_td_target(OC._ptr(actor), OC._ptr(critics), n, OC._ptr(obs), OC._ptr(reward), OC._ptr(done), OC.GAMMA,
                              OC._ptr(out[f"th_td_target/n{n}"])) == 0
        out[f"th_twin_critic_grad/n{n}"] = TC.host_twin_critic_grad(L, critics, obs, act, reward)
        out[f"th_critic_grad/n{n}"] = np.zeros(LC.RL.NCRITIC + 2, np.float32)
        assert L.th_critic_grad(OC._ptr(critics), n, OC._ptr(obs), OC._ptr(act), OC._ptr(reward), OC._ptr(out[f"th_critic_grad/n{n}"])) == 0
        out[f"th_actor_grad/n{n}"] = np.zeros(LC.RL.NACTOR + 2, np.float32)
        assert L.th_actor_grad(OC._ptr(actor), OC._ptr(critics), n, OC._ptr(obs), OC._ptr(out[f"th_actor_grad/n{n}"])) == 0
    for k, v in _host_apply(L.th_apply, out["th_twin_critic_grad/n257"], 2 * TC.NC).items():
        out[f"th_apply/{k}"] = v
    return out


def _host_sac(L, cases):
    """the sh_* interface that tests/sachost and tests/sacarchhost share, on the cases of `cases` (sac_cases at either width)"""
    out = {}
    for n in HOST_ROWS:
        (actor, critics), (obs, act, reward, done) = cases.weights("init"), inputs(n)
        for name, kw in (("sampled", {}), ("deterministic", dict(deterministic=True)), ("random", dict(random=True))):
            for k, v in zip(("action", "mu", "log_std", "z"), cases.host_act(L, actor, obs, OC.SEED, BASE, 3, **kw)):
                out[f"sh_act/n{n}/{name}/{k}"] = v
        spread = cases.weights("spread")[0]
        for extras in (True, False):
            got = cases.host_target(L, spread, critics, obs, reward, done, OC.GAMMA, OC.SEED, 0, extras=extras)
            for k, v in zip(("y", "next_action", "logp", "z"), got):
                out[f"sh_target/n{n}/extras_{int(extras)}/{k}"] = v
        q = np.zeros(n, np.float32)
        assert L.sh_q(OC._ptr(critics), n, OC._ptr(obs), OC._ptr(act), OC._ptr(q)) == 0
        out[f"sh_q/n{n}"] = q
        for scale in (0.5, 1.0):
            out[f"sh_twin_critic_grad/n{n}/scale_{scale}"] = cases.host_twin_critic_grad(L, critics, obs, act, reward, scale)
        for kind, learn_alpha in (("init", 1), ("init", 0), ("spread", 1)):
            g, dz3 = np.zeros(cases.NA + cases.SAC_TAIL, np.float32), np.zeros((n, 4), np.float32)
            assert L.sh_actor_grad(OC._ptr(cases.weights(kind)[0]), OC._ptr(critics), n, OC._ptr(obs), OC.SEED, 0, learn_alpha, cases.TARGET_ENTROPY,
                                   OC._ptr(g), OC._ptr(dz3)) == 0
            out[f"sh_actor_grad/n{n}/{kind}/alpha_{learn_alpha}"], out[f"sh_actor_grad/n{n}/{kind}/alpha_{learn_alpha}/dz3"] = g, dz3
    for k, v in _host_apply(L.sh_apply, out["sh_actor_grad/n257/init/alpha_1"], cases.NA + 1).items():
        out[f"sh_apply/{k}"] = v
    c, y = OC.conditioned(N, "init"), np.zeros(N, np.float32)
    assert L.sh_td3_combine(N, OC._ptr(c["reward"]), OC._ptr(c["done"]), C.c_float(OC.GAMMA), OC._ptr(c["obs"][:, 0].copy()), OC._ptr(c["obs"][:, 1].copy()), OC._ptr(y)) == 0
    out["sh_td3_combine"] = y
    return out


def _program(directory, source, name, args, defines=()):
    exe = os.path.join(str(directory), name)
    subprocess.check_call(OC.GXX + list(defines) + ["-o", exe, source])
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
    return _text(r.stdout)


def _case_file(path, head, floats, weights, kind, m, steps):
    """the case file td3host_main and sachost_main read (tests/test_td3_cpu.py, tests/test_sac_cpu.py write the same); step s takes rows
    [s m, (s + 1) m) of inputs(257, kind), next_obs the same rows counted from the end"""
    obs, act, reward, done = inputs(N, kind)
    with open(path, "wb") as f:
        f.write(np.array([m, steps, head], np.int32).tobytes()); f.write(np.array([5], np.uint32).tobytes())
        f.write(np.array([OC.SEED], np.uint64).tobytes()); f.write(np.array(floats, np.float32).tobytes())
        f.write(np.array([LC.ADAM["lr"], *LC.ADAM["betas"], LC.ADAM["eps"]], np.float64).tobytes())
        f.write(weights[0].tobytes()); f.write(weights[1].tobytes())
        for s in range(steps):
            sl = slice(s * m, (s + 1) * m)
            for a in (obs[sl], act[sl], obs[::-1][sl], reward[sl], done[sl]):
                f.write(np.ascontiguousarray(a).tobytes())
    return str(path)


def host_steps(directory):
    """what the stand-alone programs print after one step of each State (TD3: two, so that the delayed half of step() runs too)"""
    out, d = {}, str(directory)
    case = _case_file(os.path.join(d, "td3.bin"), 2, [LC.ADAM["tau"], OC.GAMMA, *TC.TIGHT_NOISE], TC.weights("x3"), "x3", 33, 2)
    out["td3host"] = _program(d, os.path.join(TC.HOST_DIR, "td3host_main.cpp"), "td3host_main", [case])
    case = _case_file(os.path.join(d, "sac.bin"), 1, [SC.SAC_ADAM["tau"], OC.GAMMA, SC.TARGET_ENTROPY], SC.weights("spread"), "spread", 33, 1)
    out["sachost"] = _program(d, os.path.join(SC.HOST_DIR, "sachost_main.cpp"), "sachost_main", [case])
    for arch in ("ArchReference", "ArchSacDefault"):
        out[f"sacarchhost/{arch}"] = _program(d, os.path.join(A.HOST_DIR, "sacarchhost_main.cpp"), f"sacarchhost_main_{arch}", ["33", "1"],
                                              [f"-DSACARCH={arch}"])
    return out


SIZING_ORDER = ("ddpg", "twin", "sac_ref", "sac_sb3")   # (twin, sac, arch) = (0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)
SIZING_MAIN = """
#include <stdio.h>
#include "brs_sac.hpp"
int main() {
  const int h[4][3] = {{0, 0, BRS_ARCH_REFERENCE}, {1, 0, BRS_ARCH_REFERENCE}, {1, 1, BRS_ARCH_REFERENCE}, {1, 1, BRS_ARCH_SAC_DEFAULT}};
  for (const auto& k : h) {
    const brs::sac::HandleSize s = brs::sac::handle_size(k[0] != 0, k[1] != 0, k[2]);
    printf("%d %d\\n", s.scratch_rows, s.partial_len);
  }
  return 0;
}
"""


def handle_bytes(rows, partial_len, max_batch):
    """what create() allocates: the scratch rows at ld = max_batch padded to 128, then MAX_SPLIT = 8 partial rows, in floats"""
    return 4 * (rows * ((max_batch + 127) // 128 * 128) + 8 * partial_len)


def host_sizing(directory):
    """(scratch rows, partial-row length) of the four kinds of handle, from the sizing function through a tiny host program"""
    src = os.path.join(str(directory), "sizing_main.cpp")
    with open(src, "w") as f:
        f.write(SIZING_MAIN)
    lines = bytes(_program(directory, src, "sizing_main", [])).decode().split("\n")
    return {name: np.array(line.split(), np.int64) for name, line in zip(SIZING_ORDER, lines)}


def run_host(group, directory):
    """-> {output name: numpy array} of one group of HOST_GROUPS; `directory` receives the builds"""
    if group.startswith("sacarchhost/"):
        arch = group.split("/")[1]
        out = _host_sac(A.build_host(directory, arch), SC if arch == "ArchReference" else A.C)
    else:
        out = {"offpolicyhost": host_offpolicy, "ddpglearnerhost": host_ddpg_learner, "td3host": host_td3,
               "sachost": lambda d: _host_sac(SC.build_host(d), SC), "steps": host_steps, "sizing": host_sizing}[group](directory)
    return {f"host/{group}/{k}": np.ascontiguousarray(v) for k, v in out.items()}
