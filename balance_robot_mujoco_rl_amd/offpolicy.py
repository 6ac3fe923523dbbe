"""DDPG's data path on the device (include/brs_policy.h: brs_ddpg_*, brs_replay_*).

The reference's algorithm_factory configures two algorithms by hand, PPO and DDPG (src/sb_rl.py:40-83); DDPG gets
net_arch = dict(pi=[300, 200], qf=[200, 150]) and NormalActionNoise(sigma=0.1).  Between two gradient steps SB3's DDPG runs the
deterministic actor, adds the noise, steps the env, stores the transition in a host-side numpy ReplayBuffer (terminal observation
and time-limit rules per env, in Python), samples a uniform minibatch and evaluates the two target networks.  `DeviceDDPGNets`,
`DeviceReplayBuffer` and `DeviceOffPolicyCollector` do all of that in HIP kernels of libbrs_hip.so on the simulator's own output
tensors.  The gradient step -- critic and actor gradient, Adam, Polyak update -- is `DeviceDDPGLearner` (brs_ddpg_learner_*;
DESIGN.md 7.6), or the caller's (tools/train_ddpg_torch.py does it in torch by default).  PyTorch only owns the buffers and the
stream."""
import ctypes as C

import torch

from . import _lib, nets
from ._handle import BrsError, DeviceObject, Handle, _need, _p
from .nets import ARCHS, REFERENCE

# the lengths and (weight, bias) shapes of the flat parameter vectors, all from the table of nets.py: the reference's widths ...
NACTOR, NCRITIC = REFERENCE.actor.count, REFERENCE.critic.count
ACTOR_SHAPES, CRITIC_SHAPES = REFERENCE.actor.shapes, REFERENCE.critic.shapes
SAC_NACTOR, SAC_GRAD_LEN = REFERENCE.nactor, REFERENCE.grad_len
# ... and SB3's default net_arch = [256, 256] (BRS_ARCH_SAC_DEFAULT)
NCRITIC256, SAC256_NACTOR = ARCHS["sb3"].ncritic, ARCHS["sb3"].nactor
# net_arch -> architecture, for the SAC path
SacArch, SAC_ARCHS, sac_arch = nets.Arch, ARCHS, nets.arch
# state_dict prefixes of the three Linear layers: SB3's TD3Policy and tools/train_ddpg_torch.py
NAMINGS = {"sb3": {"actor": "actor.mu.{}.", "critic": "critic.qf0.{}.", "actor_target": "actor_target.mu.{}.",
                   "critic_target": "critic_target.qf0.{}."},
           "tool": {"actor": "actor.{}.", "critic": "critic.{}.", "actor_target": "actor_target.{}.", "critic_target": "critic_target.{}."}}
# the two critics of TD3 inside one state_dict: SB3's ContinuousCritic (critic.qf0.0.weight, critic.qf1.0.weight) and
# tools/train_td3_torch.py, which holds them as an nn.ModuleList of two nn.Sequential (critic.0.0.weight, critic.1.0.weight)
TD3_CRITIC_NAMINGS = {"sb3": "{net}.qf{k}.{i}.", "tool": "{net}.{k}.{i}."}
# the SAC actor VECTOR [SAC_NACTOR + 1]: latent_pi's two layers, the mu and log_std heads stacked into one [4][200] layer, then
# log_ent_coef.  SB3's SACPolicy (actor.latent_pi.{0,2}, actor.mu, actor.log_std; log_ent_coef is the algorithm's, not the policy's,
# and is looked up under that name) and tools/train_sac_torch.py (actor.body.{0,2}, actor.mu, actor.log_std, log_ent_coef)
SAC_ACTOR_NAMINGS = {"sb3": ("actor.latent_pi.0.", "actor.latent_pi.2.", "actor.mu.", "actor.log_std."),
                     "tool": ("actor.body.0.", "actor.body.2.", "actor.mu.", "actor.log_std.")}


def naming_of(sd):
    """'sb3' or 'tool', by the keys of a state_dict"""
    keys = [k.split(".") for k in sd if isinstance(k, str)]
    if any(len(k) == 4 and k[0] in NAMINGS["sb3"] and k[1] in ("mu", "qf0") for k in keys):
        return "sb3"
    if any(len(k) == 3 and k[0] in NAMINGS["tool"] and k[1].isdigit() for k in keys):
        return "tool"
    raise ValueError("neither SB3's TD3Policy naming (actor.mu.0.weight) nor the tool's (actor.0.weight)")


def _layout(net, naming):
    return (REFERENCE.actor if net.startswith("actor") else REFERENCE.critic).layout(NAMINGS[naming][net])


def flatten_ddpg_state_dict(sd, net="actor"):
    """state_dict in either naming -> the flat float32 vector of `net` ('actor', 'critic', 'actor_target', 'critic_target')"""
    return nets.pack(sd, _layout(net, naming_of(sd)))


def unflatten_ddpg_state_dict(flat, net="actor", naming="sb3"):
    """the flat vector of `net` -> {name: tensor} in `naming`"""
    flat = nets.flat_array(flat)
    want = NACTOR if net.startswith("actor") else NCRITIC
    if flat.shape != (want,):
        raise ValueError(f"{net}: expected {want} parameters, got shape {flat.shape}")
    return nets.unpack(flat, _layout(net, naming))


def _td3_layout(net, naming, arch):
    if net not in ("critic", "critic_target"):
        raise ValueError(f"net must be 'critic' or 'critic_target', got {net!r}")
    if naming not in TD3_CRITIC_NAMINGS:
        raise ValueError(f"naming must be 'sb3' or 'tool', got {naming!r}")
    return [entry for k in (0, 1) for entry in arch.critic.layout(TD3_CRITIC_NAMINGS[naming].format(net=net, k=k, i="{}"))]


def _td3_naming_of(sd, net):
    keys = [k.split(".") for k in sd if isinstance(k, str)]
    if any(len(k) == 4 and k[0] == net and k[1] in ("qf0", "qf1") for k in keys):
        return "sb3"
    if any(len(k) == 4 and k[0] == net and k[1] in ("0", "1") and k[2].isdigit() for k in keys):
        return "tool"
    raise ValueError(f"neither SB3's naming ({net}.qf0.0.weight, {net}.qf1.0.weight) nor the TD3 tool's ({net}.0.0.weight, {net}.1.0.weight)")


def flatten_td3_critics(sd, net="critic"):
    """state_dict -> the flat float32 vector [2 NCRITIC] of TD3's two critics, critic 0 then critic 1, each in the critic's flat
    order.  `net`: 'critic' or 'critic_target'.  Two namings are understood: SB3's TD3Policy (critic.qf0.{0,2,4}.{weight,bias} and
    critic.qf1.*) and tools/train_td3_torch.py's, an nn.ModuleList of two nn.Sequential (critic.0.{0,2,4}.{weight,bias} and
    critic.1.*).  The widths are read off the shapes: qf=[200, 150], or SB3's default [256, 256] -> [2 NCRITIC256]."""
    naming = _td3_naming_of(sd, net)
    return nets.pack(sd, nets.widths_of(sd, [_td3_layout(net, naming, arch) for arch in ARCHS.values()], "the critics"))


def unflatten_td3_critics(flat, net="critic", naming="sb3"):
    """the flat vector [2 NCRITIC] (or [2 NCRITIC256]: the widths follow the length) of the two critics -> {name: tensor} in
    `naming` ('sb3' or 'tool', as flatten_td3_critics)"""
    flat = nets.flat_array(flat)
    arch = next((arch for arch in ARCHS.values() if flat.shape == (2 * arch.ncritic,)), None)
    if arch is None:
        raise ValueError(f"{net}: expected {' or '.join(str(2 * a.ncritic) for a in ARCHS.values())} parameters, got shape {flat.shape}")
    return nets.unpack(flat, _td3_layout(net, naming, arch))


def _sac_naming_of(sd):
    for naming, prefixes in SAC_ACTOR_NAMINGS.items():
        if prefixes[0] + "weight" in sd:
            return naming
    raise ValueError("neither SB3's SACPolicy naming (actor.latent_pi.0.weight) nor the SAC tool's (actor.body.0.weight)")


def flatten_sac_actor(sd):
    """state_dict in either naming, with a scalar `log_ent_coef` in it -> the flat float32 actor vector [SAC_NACTOR + 1], or
    [SAC256_NACTOR + 1] for SB3's default [256, 256]: the widths are read off the shapes"""
    prefixes = SAC_ACTOR_NAMINGS[_sac_naming_of(sd)]
    layout = nets.widths_of(sd, [arch.sac_actor_layout(prefixes) for arch in ARCHS.values()], "the SAC actor")
    if "log_ent_coef" not in sd:
        raise ValueError("log_ent_coef: missing")
    t = nets.flat_array(sd["log_ent_coef"])
    if t.size != 1:
        raise ValueError(f"log_ent_coef: expected one element, got shape {tuple(t.shape)}")
    return nets.pack({**sd, "log_ent_coef": t.reshape(1)}, layout + [("log_ent_coef", (1,))])


def unflatten_sac_actor(flat, naming="sb3"):
    """the actor vector [SAC_NACTOR + 1] (or [SAC256_NACTOR + 1]: the widths follow the length) -> {name: tensor} in `naming`
    ('sb3' or 'tool'), log_ent_coef as a tensor of shape (1,)"""
    flat = nets.flat_array(flat)
    arch = next((arch for arch in ARCHS.values() if flat.shape == (arch.nactor + 1,)), None)
    if arch is None:
        raise ValueError(f"expected {' or '.join(str(a.nactor + 1) for a in ARCHS.values())} elements, got shape {flat.shape}")
    if naming not in SAC_ACTOR_NAMINGS:
        raise ValueError(f"naming must be 'sb3' or 'tool', got {naming!r}")
    return nets.unpack(flat, arch.sac_actor_layout(SAC_ACTOR_NAMINGS[naming]) + [("log_ent_coef", (1,))])


class DeviceDDPGNets(Handle):
    """SB3's TD3Policy networks with the reference's widths, evaluated by the HIP kernels.  The parameter vectors are arguments of
    every call (flat float32 device tensors, read in place): the caller's optimiser and Polyak update write them."""
    _FAMILY, _WHAT, arch = "brs_ddpg", "the on-device DDPG networks have", REFERENCE

    def __init__(self, device=0, seed=0, env_index_base=0):
        self._attach(device)
        self._create("brs_ddpg_create", self.device.index)
        self.seed, self.env_index_base = int(seed), int(env_index_base)

    def act(self, actor_params, obs, step, sigma, random=False, out=None, mean=None, noise=None):
        """SB3 _sample_action: obs [n,6] -> action [n,2] = clip(mean + sigma z); `random`: the learning_starts phase (uniform mean,
        actor_params and obs may be None, n is then taken from `out`); mean / noise: optional [n,2] outputs"""
        d, f32 = self.device, torch.float32
        n = out.shape[0] if random and obs is None else obs.shape[0]
        if not random:
            _need(actor_params, "actor_params", f32, (NACTOR,), d); _need(obs, "obs", f32, (n, 6), d)
        if out is None:
            out = torch.empty((n, 2), dtype=f32, device=d)
        _need(out, "action", f32, (n, 2), d)
        for t, name in ((mean, "mean"), (noise, "noise")):
            if t is not None:
                _need(t, name, f32, (n, 2), d)
        self._check(self.L.brs_ddpg_act(self.h, None if random else _p(actor_params), n, None if random else _p(obs), self.seed,
                                        self.env_index_base, int(step) & 0xffffffff, float(sigma), int(bool(random)), _p(out), _p(mean),
                                        _p(noise), self._stream()), "brs_ddpg_act")
        return out

    def q(self, critic_params, obs, action, out=None):
        """Q(s, a) of one critic of this object's architecture: obs [n,6], action [n,2] -> [n]"""
        d, f32, n = self.device, torch.float32, obs.shape[0]
        _need(critic_params, "critic_params", f32, (self.arch.ncritic,), d); _need(obs, "obs", f32, (n, 6), d); _need(action, "action", f32, (n, 2), d)
        if out is None:
            out = torch.empty(n, dtype=f32, device=d)
        _need(out, "q", f32, (n,), d)
        self._check(self.L.brs_ddpg_q(self.h, _p(critic_params), n, _p(obs), _p(action), _p(out), self._stream()), "brs_ddpg_q")
        return out

    def td_target(self, actor_target_params, critic_target_params, next_obs, reward, done, gamma, out=None):
        """y = reward + (1 - done) gamma Q'(next_obs, pi'(next_obs)) from the two target networks: [m]"""
        d, f32, m = self.device, torch.float32, next_obs.shape[0]
        _need(actor_target_params, "actor_target_params", f32, (NACTOR,), d); _need(critic_target_params, "critic_target_params", f32, (NCRITIC,), d)
        _need(next_obs, "next_obs", f32, (m, 6), d); _need(reward, "reward", f32, (m,), d); _need(done, "done", torch.uint8, (m,), d)
        if out is None:
            out = torch.empty(m, dtype=f32, device=d)
        _need(out, "y", f32, (m,), d)
        self._check(self.L.brs_ddpg_td_target(self.h, _p(actor_target_params), _p(critic_target_params), m, _p(next_obs), _p(reward), _p(done),
                                              float(gamma), _p(out), self._stream()), "brs_ddpg_td_target")
        return out


    def td3_target(self, actor_target, critics_target, next_obs, reward, done, gamma, policy_noise, noise_clip, draw, out=None, next_action=None,
                   noise=None):
        """TD3's target from the three target networks, one launch: y = reward + (1 - done) gamma min(Q1', Q2')(next_obs, a') with
        a' = clamp(pi'(next_obs) + clamp(policy_noise z, -noise_clip, noise_clip), -1, 1); critics_target [2 NCRITIC]; `draw`: the
        counter of this call's noise (with the object's seed); next_action / noise: optional [m,2] outputs (a' and z) -> y [m]"""
        d, f32, m = self.device, torch.float32, next_obs.shape[0]
        _need(actor_target, "actor_target", f32, (NACTOR,), d); _need(critics_target, "critics_target", f32, (2 * NCRITIC,), d)
        _need(next_obs, "next_obs", f32, (m, 6), d); _need(reward, "reward", f32, (m,), d); _need(done, "done", torch.uint8, (m,), d)
        if out is None:
            out = torch.empty(m, dtype=f32, device=d)
        _need(out, "y", f32, (m,), d)
        for t, name in ((next_action, "next_action"), (noise, "noise")):
            if t is not None:
                _need(t, name, f32, (m, 2), d)
        self._check(self.L.brs_td3_td_target(self.h, _p(actor_target), _p(critics_target), m, _p(next_obs), _p(reward), _p(done), float(gamma),
                                             float(policy_noise), float(noise_clip), self.seed, int(draw) & 0xffffffff, _p(out), _p(next_action),
                                             _p(noise), self._stream()), "brs_td3_td_target")
        return out


def _storage(obs, next_obs, action, reward, done):
    return _lib.BrsReplayStorage(obs.data_ptr(), next_obs.data_ptr(), action.data_ptr(), reward.data_ptr(), done.data_ptr())


class DeviceReplayBuffer(DeviceObject):
    """SB3's ReplayBuffer for the n envs of a BatchedSim, resident in HBM, time-major: obs / next_obs [cap][n][6], action
    [cap][n][2], reward / done [cap][n].  add() and sample() each enqueue one kernel; `pos` and `full` are host integers."""

    _WHAT = "the on-device replay buffer has"

    def __init__(self, n_envs, capacity_steps, device=0, seed=0):
        self._attach(device)
        self.n, self.cap = int(n_envs), int(capacity_steps)
        if self.n < 1 or self.cap < 1 or self.n * self.cap > 2 ** 31 - 1:
            raise ValueError(f"need n_envs >= 1, capacity_steps >= 1 and their product <= 2^31 - 1, got {n_envs}, {capacity_steps}")
        d, n, cap = self.device, self.n, self.cap
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=d)
        self.obs, self.next_obs, self.action, self.reward = f(cap, n, 6), f(cap, n, 6), f(cap, n, 2), f(cap, n)
        self.done = torch.zeros((cap, n), dtype=torch.uint8, device=d)
        self._store = _storage(self.obs, self.next_obs, self.action, self.reward, self.done)
        self.pos, self.full, self.seed, self.draw = 0, False, int(seed), 0

    @property
    def rows(self):
        """valid rows (env steps): pos until the first wrap, then the capacity"""
        return self.cap if self.full else self.pos

    @property
    def size(self):
        """valid transitions"""
        return self.rows * self.n

    def __len__(self):
        return self.size

    def _check(self, rc, what):   # the replay calls take no handle: one error slot for the family
        if rc != 0:
            raise BrsError(f"{what} failed ({rc}): {self.L.brs_replay_last_error().decode()}")

    def add(self, last_obs, action, obs, terminal_obs, reward, terminated, truncated):
        """one env step of all envs into row `pos`: last_obs is what `action` was computed from, the other five are BatchedSim.step's
        outputs (consumed in stream order: the views may be overwritten by the next step afterwards)"""
        n, d, f32, u8 = self.n, self.device, torch.float32, torch.uint8
        _need(last_obs, "last_obs", f32, (n, 6), d); _need(action, "action", f32, (n, 2), d); _need(obs, "obs", f32, (n, 6), d)
        _need(terminal_obs, "terminal_obs", f32, (n, 6), d); _need(reward, "reward", f32, (n,), d)
        _need(terminated, "terminated", u8, (n,), d); _need(truncated, "truncated", u8, (n,), d)
        self._check(self.L.brs_replay_add(d.index, C.byref(self._store), n, self.cap, self.pos, _p(last_obs), _p(action), _p(obs), _p(reward),
                                          _p(terminated), _p(truncated), _p(terminal_obs), self._stream()), "brs_replay_add")
        self.pos = (self.pos + 1) % self.cap
        self.full = self.full or self.pos == 0

    def new_batch(self, m):
        d = self.device
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=d)
        return f(m, 6), f(m, 6), f(m, 2), f(m), torch.empty(m, dtype=torch.uint8, device=d)

    def sample(self, m, out=None, idx=None, normalize=None):
        """m uniform transitions -> (obs [m,6], next_obs [m,6], action [m,2], reward [m], done [m] uint8); `out`: the same five
        preallocated; idx: optional int32 [m,2] that receives (row, env).  Every call uses the next value of the draw counter.
        `normalize`: a DeviceVecNormalize on this device -- SB3's sample(batch_size, env=vec_normalize): the same cells, obs and
        next_obs through normalize_obs and reward through normalize_reward of its statistics as they stand, in the same single
        launch (brs_replay_sample_vecnorm)"""
        m = int(m)
        if self.rows < 1:
            raise ValueError("sample() from an empty buffer")
        if normalize is not None and getattr(normalize, "device", None) != self.device:
            raise ValueError(f"normalize: the normaliser lives on {getattr(normalize, 'device', None)}, the replay buffer on {self.device}")
        if out is None:
            out = self.new_batch(m)
        d, f32 = self.device, torch.float32
        o, no, a, r, dn = out
        _need(o, "obs", f32, (m, 6), d); _need(no, "next_obs", f32, (m, 6), d); _need(a, "action", f32, (m, 2), d); _need(r, "reward", f32, (m,), d)
        _need(dn, "done", torch.uint8, (m,), d)
        if idx is not None:
            _need(idx, "idx", torch.int32, (m, 2), d)
        dst = _storage(o, no, a, r, dn)
        if normalize is None:
            self._check(self.L.brs_replay_sample(d.index, C.byref(self._store), self.n, self.cap, self.rows, m, self.seed, self.draw & 0xffffffff,
                                                 C.byref(dst), _p(idx), self._stream()), "brs_replay_sample")
        else:   # the normaliser's handle: its statistics, its error slot
            normalize._check(self.L.brs_replay_sample_vecnorm(normalize.h, C.byref(self._store), self.n, self.cap, self.rows, m, self.seed,
                                                              self.draw & 0xffffffff, C.byref(dst), _p(idx), self._stream()),
                             "brs_replay_sample_vecnorm")
        self.draw += 1
        return out


class DeviceOffPolicyCollector:
    """SB3's OffPolicyAlgorithm.collect_rollouts on the device: collect() alternates brs_ddpg_act -> brs_step -> (monitor) ->
    brs_replay_add with no synchronisation and no allocation.  `actor_params`: the flat device tensor the learner updates in place.
    `monitor`: an EpisodeMonitor that is fed every step.  `normalize`: a DeviceVecNormalize for the simulator's envs (DESIGN.md
    7.14) -- SB3's off-policy rule: the actor acts on the normalised observation, the buffer stores the raw last observation and
    the simulator's raw outputs (sample(..., normalize=) normalises the minibatch), the monitor sees the env's own reward, and the
    statistics train on every step, the uniform warm-up included."""

    def __init__(self, sim, nets, actor_params, replay, sigma=0.1, monitor=None, normalize=None):
        self.sim, self.nets, self.actor_params, self.replay, self.sigma, self.monitor = sim, nets, actor_params, replay, float(sigma), monitor
        self.normalize = normalize
        if replay.n != sim.n:
            raise ValueError(f"the replay buffer holds {replay.n} envs, the simulator {sim.n}")
        if normalize is not None and normalize.n != sim.n:
            raise ValueError(f"the normaliser holds {normalize.n} envs, the simulator {sim.n}")
        self._action = torch.zeros((sim.n, 2), dtype=torch.float32, device=sim.device)
        self._last_obs = None   # a private copy: sim.step returns views that the next step overwrites
        self._last_norm_obs = None   # with a normaliser: what the actor sees (the normaliser's own tensor)
        self.step = 0

    def collect(self, steps, random=False):
        sim, nets, replay, normalize = self.sim, self.nets, self.replay, self.normalize
        if self._last_obs is None:
            self._last_obs = sim.reset().clone()
            if normalize is not None:
                self._last_norm_obs = normalize.reset(self._last_obs)
        for _ in range(int(steps)):
            nets.act(self.actor_params, self._last_obs if normalize is None else self._last_norm_obs, self.step, self.sigma, random=random,
                     out=self._action)
            self.step += 1
            obs, rew, term, trunc, tobs = sim.step(self._action)
            if self.monitor is not None:
                self.monitor.update(rew, term, trunc)
            if normalize is not None:
                self._last_norm_obs = normalize.step(obs, rew, term, trunc, tobs)[0]
            replay.add(self._last_obs, self._action, obs, tobs, rew, term, trunc)   # raw, with or without a normaliser
            self._last_obs.copy_(obs)
        return self


class _OffPolicyLearner(Handle):
    """what the learners on a brs_ddpg_learner handle share: its creation, Adam's settings, the one apply call, and the optimiser
    state as a state_dict.  `_TENSORS` / `_COUNTERS` name the attributes that state is made of."""
    _FAMILY = "brs_ddpg_learner"
    _TENSORS = _COUNTERS = ()

    def _create_learner(self, create, max_batch, lr, betas, eps, tau, *args):
        self.max_batch, self.tau = int(max_batch), float(tau)
        self.cfg = _lib.BrsAdamConfig(float(lr), float(betas[0]), float(betas[1]), float(eps))
        self._create(create, self.device.index, self.max_batch, *args)

    def _zeros(self, n):
        return torch.zeros(n, dtype=torch.float32, device=self.device)

    def scratch(self):
        """(device address, bytes) of the handle's one allocation"""
        ptr, size = C.c_void_p(), C.c_int64()
        self._check(self.L.brs_ddpg_learner_scratch(self.h, C.byref(ptr), C.byref(size)), "brs_ddpg_learner_scratch")
        return ptr.value, size.value

    def _apply(self, n, params, grad, grad_len, mom, vel, target, step, name):
        d, f32 = self.device, torch.float32
        _need(params, name, f32, (n,), d); _need(grad, "grad", f32, (grad_len,), d)
        _need(mom, "m_" + name, f32, (n,), d); _need(vel, "v_" + name, f32, (n,), d)
        if target is not None:
            _need(target, name + "_target", f32, (n,), d)
        self._check(self.L.brs_ddpg_learner_apply(self.h, n, _p(params), _p(grad), _p(mom), _p(vel), _p(target), C.byref(self.cfg), step,
                                                  self.tau, self._stream()), "brs_ddpg_learner_apply")

    def state_dict(self):
        return {**{k: getattr(self, k).clone() for k in self._TENSORS}, **{k: getattr(self, k) for k in self._COUNTERS}}

    def load_state_dict(self, sd):
        for k in self._TENSORS:
            t = getattr(self, k)
            src = torch.as_tensor(sd[k])
            if tuple(src.shape) != tuple(t.shape):
                raise ValueError(f"{k}: expected shape {tuple(t.shape)}, got {tuple(src.shape)}")
            t.copy_(src.to(device=self.device, dtype=torch.float32))
        for k in self._COUNTERS:
            setattr(self, k, int(sd[k]))


class DeviceDDPGLearner(_OffPolicyLearner):
    """SB3's TD3.train as DDPG uses it (one critic, no delay, no target noise) by the HIP kernels of brs_ddpg_learner_*: the
    gradient of mse(Q(s, a), y) w.r.t. the critic, the gradient of -mean Q(s, pi(s)) w.r.t. the actor, torch.optim.Adam's step and
    the Polyak update.  The four networks are the caller's flat float32 device tensors, updated in place; this object owns the two
    gradient buffers, the four moment vectors and the two step counters.  grad and apply are separate calls: a data-parallel
    caller all-reduces-and-divides `grad_critic` / `grad_actor` in between."""
    _WHAT = "the on-device DDPG learner has"
    _TENSORS, _COUNTERS = ("m_critic", "v_critic", "m_actor", "v_actor"), ("steps_critic", "steps_actor")

    def __init__(self, device=0, max_batch=256, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005):
        self._attach(device)
        self._create_learner("brs_ddpg_learner_create", max_batch, lr, betas, eps, tau)
        z = self._zeros
        self.grad_critic, self.grad_actor = z(NCRITIC + _lib.DDPG_NSTAT), z(NACTOR + _lib.DDPG_NSTAT)
        self.m_critic, self.v_critic, self.m_actor, self.v_actor = z(NCRITIC), z(NCRITIC), z(NACTOR), z(NACTOR)
        self.steps_critic = self.steps_actor = 0

    def critic_grad(self, critic, obs, action, y, out=None):
        """-> [NCRITIC + 2]: the gradient of Lc = mean (Q(s, a) - y)^2 in the critic's flat order, then Lc and mean Q"""
        d, f32, m = self.device, torch.float32, obs.shape[0]
        out = self.grad_critic if out is None else out
        _need(critic, "critic", f32, (NCRITIC,), d); _need(obs, "obs", f32, (m, 6), d); _need(action, "action", f32, (m, 2), d)
        _need(y, "y", f32, (m,), d); _need(out, "grad", f32, (NCRITIC + _lib.DDPG_NSTAT,), d)
        self._check(self.L.brs_ddpg_learner_critic_grad(self.h, _p(critic), m, _p(obs), _p(action), _p(y), _p(out), self._stream()),
                    "brs_ddpg_learner_critic_grad")
        return out

    def actor_grad(self, actor, critic, obs, out=None):
        """-> [NACTOR + 2]: the gradient of La = -mean Q(s, pi(s)) in the actor's flat order (through `critic`, which gets none),
        then La and the mean of pi(s)^2"""
        d, f32, m = self.device, torch.float32, obs.shape[0]
        out = self.grad_actor if out is None else out
        _need(actor, "actor", f32, (NACTOR,), d); _need(critic, "critic", f32, (NCRITIC,), d); _need(obs, "obs", f32, (m, 6), d)
        _need(out, "grad", f32, (NACTOR + _lib.DDPG_NSTAT,), d)
        self._check(self.L.brs_ddpg_learner_actor_grad(self.h, _p(actor), _p(critic), m, _p(obs), _p(out), self._stream()),
                    "brs_ddpg_learner_actor_grad")
        return out

    def apply_critic(self, critic, critic_target=None, grad=None):
        """Adam's step on `critic` from grad_critic (or `grad`), then critic_target += tau (critic - critic_target)"""
        self._apply(NCRITIC, critic, self.grad_critic if grad is None else grad, NCRITIC + _lib.DDPG_NSTAT, self.m_critic, self.v_critic,
                    critic_target, self.steps_critic + 1, "critic")
        self.steps_critic += 1

    def apply_actor(self, actor, actor_target=None, grad=None):
        self._apply(NACTOR, actor, self.grad_actor if grad is None else grad, NACTOR + _lib.DDPG_NSTAT, self.m_actor, self.v_actor,
                    actor_target, self.steps_actor + 1, "actor")
        self.steps_actor += 1

    def step(self, flat, obs, action, y):
        """the whole gradient step on a dict of the four flat vectors (actor, critic, actor_target, critic_target) in SB3's order:
        critic gradient and step, actor gradient WITH THE UPDATED CRITIC and step; each apply moves its own target"""
        self.critic_grad(flat["critic"], obs, action, y)
        self.apply_critic(flat["critic"], flat["critic_target"])
        self.actor_grad(flat["actor"], flat["critic"], obs)
        self.apply_actor(flat["actor"], flat["actor_target"])

    def stats(self):
        """the four means of the last two gradient calls, one device-to-host copy: critic_loss, mean_q, actor_loss, mean_action_sq"""
        s = torch.cat([self.grad_critic[NCRITIC:], self.grad_actor[NACTOR:]]).cpu().tolist()
        return dict(zip(("critic_loss", "mean_q", "actor_loss", "mean_action_sq"), s))


class _TwinCriticLearner(_OffPolicyLearner):
    """TD3's and SAC's side of it: two critics in one [2 NCRITIC] vector with one gradient buffer and one Adam, at the widths of
    `self.arch`.  `_TWIN_GRAD` is the C entry point of the twin critic gradient; the two differ only in the loss's factor."""
    arch, _TWIN_GRAD = REFERENCE, None
    _TENSORS = ("m_critics", "v_critics", "m_actor", "v_actor")

    def _twin_buffers(self):
        n = 2 * self.arch.ncritic
        self.grad_critics, self.m_critics, self.v_critics, self.steps_critics = self._zeros(n + _lib.TD3_NSTAT), self._zeros(n), self._zeros(n), 0

    def twin_critic_grad(self, critics, obs, action, y, out=None):
        """-> [2 NCRITIC + 4]: the gradient of c mse(Q1(s, a), y) w.r.t. critic 0, of c mse(Q2(s, a), y) w.r.t. critic 1, then c mse
        and the mean Q of critic 0 and of critic 1.  c = 1 for TD3, whose loss is mse(Q1, y) + mse(Q2, y); c = 0.5 for SAC, whose loss
        is SB3's 0.5 (mse(Q1, y) + mse(Q2, y))"""
        d, f32, m, n = self.device, torch.float32, obs.shape[0], 2 * self.arch.ncritic
        out = self.grad_critics if out is None else out
        _need(critics, "critics", f32, (n,), d); _need(obs, "obs", f32, (m, 6), d); _need(action, "action", f32, (m, 2), d)
        _need(y, "y", f32, (m,), d); _need(out, "grad", f32, (n + _lib.TD3_NSTAT,), d)
        self._check(getattr(self.L, self._TWIN_GRAD)(self.h, _p(critics), m, _p(obs), _p(action), _p(y), _p(out), self._stream()), self._TWIN_GRAD)
        return out

    def apply_critics(self, critics, critics_target=None, grad=None):
        """one Adam step over both critics from grad_critics (or `grad`); with critics_target, also its Polyak update (TD3 passes it
        on the delayed steps only: the critics do not change between their Adam step and the end of the update)"""
        n = 2 * self.arch.ncritic
        self._apply(n, critics, self.grad_critics if grad is None else grad, n + _lib.TD3_NSTAT, self.m_critics, self.v_critics,
                    critics_target, self.steps_critics + 1, "critics")
        self.steps_critics += 1


class DeviceTD3Learner(_TwinCriticLearner):
    """SB3's TD3.train by the HIP kernels, on the reference's DDPG widths (pi=[300, 200], qf=[200, 150]): the gradient of
    mse(Q1(s, a), y) + mse(Q2(s, a), y) w.r.t. both critics in one set of launches (brs_ddpg_learner_twin_critic_grad), one Adam
    over the [2 NCRITIC] vector, and every `policy_delay`-th update the actor's gradient through the first, updated critic, its
    Adam step and the Polyak update of all three targets.  The networks are the caller's flat float32 device tensors (actor
    [NACTOR], critics [2 NCRITIC] and their targets), updated in place; this object owns the twin gradient buffer, the actor's, the
    moment vectors, the step counters and n_updates."""
    _WHAT, _TWIN_GRAD = "the on-device TD3 learner has", "brs_ddpg_learner_twin_critic_grad"
    _COUNTERS = ("steps_critics", "steps_actor", "n_updates")

    def __init__(self, device=0, max_batch=256, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, tau=0.005, policy_delay=2):
        self._attach(device)
        if int(policy_delay) < 1:
            raise ValueError(f"policy_delay must be at least 1, got {policy_delay}")
        self.policy_delay = int(policy_delay)
        self._create_learner("brs_ddpg_learner_create_twin", max_batch, lr, betas, eps, tau)
        self._twin_buffers()
        self.grad_actor, self.m_actor, self.v_actor = self._zeros(NACTOR + _lib.DDPG_NSTAT), self._zeros(NACTOR), self._zeros(NACTOR)
        self.steps_actor = self.n_updates = 0

    def actor_grad(self, actor, critics, obs, out=None):
        """-> [NACTOR + 2]: the gradient of La = -mean Q1(s, pi(s)) through the FIRST critic of `critics` [2 NCRITIC], then La and
        the mean of pi(s)^2"""
        d, f32, m = self.device, torch.float32, obs.shape[0]
        out = self.grad_actor if out is None else out
        _need(actor, "actor", f32, (NACTOR,), d); _need(critics, "critics", f32, (2 * NCRITIC,), d); _need(obs, "obs", f32, (m, 6), d)
        _need(out, "grad", f32, (NACTOR + _lib.DDPG_NSTAT,), d)
        self._check(self.L.brs_ddpg_learner_actor_grad(self.h, _p(actor), _p(critics), m, _p(obs), _p(out), self._stream()),
                    "brs_ddpg_learner_actor_grad")
        return out

    def apply_actor(self, actor, actor_target=None, grad=None):
        self._apply(NACTOR, actor, self.grad_actor if grad is None else grad, NACTOR + _lib.DDPG_NSTAT, self.m_actor, self.v_actor,
                    actor_target, self.steps_actor + 1, "actor")
        self.steps_actor += 1

    def step(self, flat, obs, action, y):
        """one update of SB3's TD3.train on a dict of the four flat vectors actor, critics, actor_target, critics_target: the twin
        critic gradient and one Adam step; if n_updates (counted from 1) is a multiple of policy_delay, the actor's gradient through
        the updated first critic, its Adam step and the Polyak update of all targets; on the other updates no target moves.
        -> whether the actor was updated"""
        self.n_updates += 1
        delayed = self.n_updates % self.policy_delay == 0
        self.twin_critic_grad(flat["critics"], obs, action, y)
        self.apply_critics(flat["critics"], flat["critics_target"] if delayed else None)
        if delayed:
            self.actor_grad(flat["actor"], flat["critics"], obs)
            self.apply_actor(flat["actor"], flat["actor_target"])
        return delayed

    def stats(self):
        """one device-to-host copy: critic_loss (the sum of the two), mean_q1, mean_q2 of the last update, actor_loss and
        mean_action_sq of the last delayed one"""
        c0, q0, c1, q1, la, sq = torch.cat([self.grad_critics[2 * NCRITIC:], self.grad_actor[NACTOR:]]).cpu().tolist()
        return {"critic_loss": c0 + c1, "mean_q1": q0, "mean_q2": q1, "actor_loss": la, "mean_action_sq": sq}


# ------------------------------------------------------------------------------------------------ SAC
class DeviceSACNets(DeviceDDPGNets):
    """SB3's SACPolicy on the reference's DDPG widths, evaluated by the HIP kernels (brs_sac_act, brs_sac_td_target): the
    squashed-Gaussian actor [SAC_NACTOR + 1] (the last element is log_ent_coef) and the two target critics [2 NCRITIC].  act() has
    DeviceDDPGNets.act's surface, so DeviceOffPolicyCollector drives it unchanged.  net_arch='sb3': SB3's default [256, 256]
    (DESIGN.md 7.12), the vectors then [SAC256_NACTOR + 1] and [2 NCRITIC256]; the DDPG / TD3 calls are refused on such an object."""
    _WHAT = "the on-device SAC networks have"

    def __init__(self, device=0, seed=0, env_index_base=0, net_arch="reference"):
        self._attach(device)
        self.arch = sac_arch(net_arch)
        self._create("brs_ddpg_create_arch", self.device.index, self.arch.id)
        self.seed, self.env_index_base = int(seed), int(env_index_base)

    def act(self, actor_params, obs, step, sigma=None, random=False, deterministic=False, out=None, mean=None, log_std=None, noise=None):
        """obs [n,6] -> action [n,2] = tanh(mu + exp(clamp(log_std, -20, 2)) z); deterministic: tanh(mu); `random`: the learning_starts
        phase (uniform; actor_params and obs may be None, n is then taken from `out`); `sigma` is ignored (SAC has no action noise: the
        collector passes its own); mean / log_std / noise: optional [n,2] outputs (mu, the clamped log_std, z)"""
        d, f32 = self.device, torch.float32
        n = out.shape[0] if random and obs is None else obs.shape[0]
        if not random:
            _need(actor_params, "actor_params", f32, (self.arch.nactor + 1,), d); _need(obs, "obs", f32, (n, 6), d)
        if out is None:
            out = torch.empty((n, 2), dtype=f32, device=d)
        _need(out, "action", f32, (n, 2), d)
        for t, name in ((mean, "mean"), (log_std, "log_std"), (noise, "noise")):
            if t is not None:
                _need(t, name, f32, (n, 2), d)
        self._check(self.L.brs_sac_act(self.h, None if random else _p(actor_params), n, None if random else _p(obs), self.seed,
                                       self.env_index_base, int(step) & 0xffffffff, int(bool(deterministic)), int(bool(random)), _p(out),
                                       _p(mean), _p(log_std), _p(noise), self._stream()), "brs_sac_act")
        return out

    def sac_target(self, actor, critics_target, next_obs, reward, done, gamma, draw, out=None, next_action=None, logp=None, noise=None):
        """SAC's target, one launch: y = reward + (1 - done) gamma (min(Q1', Q2')(next_obs, a') - alpha logp') with a', logp' sampled
        from the CURRENT actor and alpha = exp(actor[-1]); `draw`: the counter of this call's noise (with the object's seed);
        next_action [m,2], logp [m], noise [m,2]: optional outputs -> y [m]"""
        d, f32, m = self.device, torch.float32, next_obs.shape[0]
        _need(actor, "actor", f32, (self.arch.nactor + 1,), d); _need(critics_target, "critics_target", f32, (2 * self.arch.ncritic,), d)
        _need(next_obs, "next_obs", f32, (m, 6), d); _need(reward, "reward", f32, (m,), d); _need(done, "done", torch.uint8, (m,), d)
        if out is None:
            out = torch.empty(m, dtype=f32, device=d)
        _need(out, "y", f32, (m,), d)
        for t, name, shape in ((next_action, "next_action", (m, 2)), (logp, "logp", (m,)), (noise, "noise", (m, 2))):
            if t is not None:
                _need(t, name, f32, shape, d)
        self._check(self.L.brs_sac_td_target(self.h, _p(actor), _p(critics_target), m, _p(next_obs), _p(reward), _p(done), float(gamma), self.seed,
                                             int(draw) & 0xffffffff, _p(out), _p(next_action), _p(logp), _p(noise), self._stream()),
                    "brs_sac_td_target")
        return out


class DeviceSACLearner(_TwinCriticLearner):
    """SB3's SAC.train by the HIP kernels, on the reference's DDPG widths: the gradient of 0.5 (mse(Q1, y) + mse(Q2, y)) w.r.t. both
    critics (brs_sac_twin_critic_grad), one Adam with the Polyak update over the [2 NCRITIC] vector, the actor's gradient through
    both UPDATED critics with the temperature's in the same buffer (brs_sac_actor_grad), and one Adam over the [SAC_NACTOR + 1]
    vector, actor and log_ent_coef together (SB3 gives both the same learning rate, and Adam is element-wise).  The vectors are the
    caller's flat float32 device tensors, updated in place; this object owns the two gradient buffers, the moment vectors and the
    step counter.  With learn_alpha=False the temperature's gradient is written as 0 and Adam leaves the element as it is.
    net_arch='sb3': SB3's default [256, 256]; every length below is then that architecture's (self.arch)."""
    _WHAT, _TWIN_GRAD = "the on-device SAC learner has", "brs_sac_twin_critic_grad"
    _COUNTERS = ("steps_critics", "steps_actor")

    def __init__(self, device=0, max_batch=256, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, tau=0.005, target_entropy=-2.0, learn_alpha=True, seed=0,
                 net_arch="reference"):
        self._attach(device)
        self.arch = sac_arch(net_arch)
        self.target_entropy, self.learn_alpha, self.seed = float(target_entropy), bool(learn_alpha), int(seed)
        self._create_learner("brs_ddpg_learner_create_sac_arch", max_batch, lr, betas, eps, tau, self.arch.id)
        self._twin_buffers()
        n = self.arch.nactor + 1
        self.grad_actor, self.m_actor, self.v_actor, self.steps_actor = self._zeros(self.arch.grad_len), self._zeros(n), self._zeros(n), 0

    def actor_grad(self, actor, critics, obs, draw, out=None):
        """-> [SAC_NACTOR + 1 + 4]: the gradient of La = mean(alpha logp - min(Q1, Q2)(s, a)) in the actor's flat order, the
        temperature's -(mean logp + target_entropy) (0 with learn_alpha=False), then La, mean logp, mean min Q and alpha; `draw`: the
        counter of this call's noise (with the object's seed)"""
        d, f32, m, arch = self.device, torch.float32, obs.shape[0], self.arch
        out = self.grad_actor if out is None else out
        _need(actor, "actor", f32, (arch.nactor + 1,), d); _need(critics, "critics", f32, (2 * arch.ncritic,), d); _need(obs, "obs", f32, (m, 6), d)
        _need(out, "grad", f32, (arch.grad_len,), d)
        self._check(self.L.brs_sac_actor_grad(self.h, _p(actor), _p(critics), m, _p(obs), self.seed, int(draw) & 0xffffffff, int(self.learn_alpha),
                                              self.target_entropy, _p(out), self._stream()), "brs_sac_actor_grad")
        return out

    def apply_actor(self, actor, grad=None):
        """one Adam step over the actor and log_ent_coef from grad_actor (or `grad`); SAC has no target actor"""
        self._apply(self.arch.nactor + 1, actor, self.grad_actor if grad is None else grad, self.arch.grad_len, self.m_actor, self.v_actor, None,
                    self.steps_actor + 1, "actor")
        self.steps_actor += 1

    def step(self, flat, obs, action, y, draw):
        """one update of SB3's SAC.train on a dict of the three flat vectors actor [SAC_NACTOR + 1], critics, critics_target, for a y
        computed from them BEFORE this call (DeviceSACNets.sac_target): critic gradient, critics' Adam and Polyak, the actor's
        gradient through the updated critics with the temperature of before the update, one Adam over actor and temperature"""
        self.twin_critic_grad(flat["critics"], obs, action, y)
        self.apply_critics(flat["critics"], flat["critics_target"])
        self.actor_grad(flat["actor"], flat["critics"], obs, draw)
        self.apply_actor(flat["actor"])

    def stats(self):
        """one device-to-host copy: critic_loss (SB3's 0.5 (mse1 + mse2)), mean_q1, mean_q2, actor_loss, mean_logp, mean_qmin and
        ent_coef (the alpha the last actor gradient used), ent_coef_grad"""
        c0, q0, c1, q1, ge, la, lp, qm, al = torch.cat([self.grad_critics[2 * self.arch.ncritic:], self.grad_actor[self.arch.nactor:]]).cpu().tolist()
        return {"critic_loss": c0 + c1, "mean_q1": q0, "mean_q2": q1, "actor_loss": la, "mean_logp": lp, "mean_qmin": qm, "ent_coef": al,
                "ent_coef_grad": ge}
