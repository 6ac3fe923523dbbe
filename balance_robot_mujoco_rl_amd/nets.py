"""The networks of the off-policy path (DDPG, TD3, SAC and their int8 actors), written down once: an MLP's layer shapes and
parameter count from its four widths, the table of architectures the kernels are built for, and the one pack / unpack pair
between a state_dict and a flat float32 parameter vector.  offpolicy.py and quant.py derive every shape, length and offset from here.

A third architecture (TD3's default [400, 300], say) is one row of ARCHS -- next to its kernels and its id in include/brs_policy.h."""
import numpy as np
import torch

from . import _lib
from ._handle import _numpy

_LAYER_INDEX = (0, 2, 4)   # Linear, ReLU, Linear, ReLU, Linear in an nn.Sequential


class Mlp:
    """n_in -> h0 -> h1 -> n_out, three Linear layers; the flat order is W b W b W b, W as [out][in]"""

    def __init__(self, n_in, h0, h1, n_out):
        self.sizes = ((n_in, h0), (h0, h1), (h1, n_out))                      # (in, out) per layer
        self.shapes = [((o, i), (o,)) for i, o in self.sizes]                 # (weight shape, bias shape) per layer
        self.count = sum(i * o + o for i, o in self.sizes)

    def layout(self, prefix):
        """[(name, shape)] in flat order; `prefix` has one {} for the layer's index in an nn.Sequential"""
        return [(prefix.format(i) + kind, shape) for i, pair in zip(_LAYER_INDEX, self.shapes) for kind, shape in zip(("weight", "bias"), pair)]


class Arch:
    """one network architecture (include/brs_policy.h, include/brs_qpolicy.h: BRS_ARCH_*): its id, the hidden widths of actor and
    critic, and what follows from them.  `nactor` / `ncritic` / `grad_len` are the lengths of the SAC path: the SAC actor without
    log_ent_coef, one critic, the actor's gradient buffer"""

    def __init__(self, name, arch_id, pi, qf):
        self.name, self.id, self.pi, self.qf = name, arch_id, tuple(pi), tuple(qf)
        self.actor = Mlp(6, *pi, 2)        # DDPG's and TD3's actor, and the int8 actor
        self.critic = Mlp(8, *qf, 1)
        self.sac_actor = Mlp(6, *pi, 4)    # the mu and log_std heads stacked into one [4][h1] layer
        self.nactor, self.ncritic = self.sac_actor.count, self.critic.count
        self.grad_len = self.nactor + 1 + _lib.SAC_NSTAT

    def sac_actor_layout(self, prefixes):
        """[(name, shape)] of the SAC actor in flat order, without log_ent_coef; `prefixes`: of the two body layers, mu and log_std.
        The stacked head is mu W, log_std W, mu b, log_std b: each head has the shapes of the DDPG actor's output layer"""
        (w0, b0), (w1, b1), (w2, b2) = self.actor.shapes
        p0, p1, mu, log_std = prefixes
        return [(p0 + "weight", w0), (p0 + "bias", b0), (p1 + "weight", w1), (p1 + "bias", b1),
                (mu + "weight", w2), (log_std + "weight", w2), (mu + "bias", b2), (log_std + "bias", b2)]

    def sac_mu_slices(self):
        """the three slices of the SAC actor vector that make the DDPG-layout actor tanh(mu(s)): the body, mu's weights, mu's bias"""
        n_in, n_out = self.actor.sizes[2]
        w = n_in * n_out
        body = self.actor.count - w - n_out
        return slice(0, body), slice(body, body + w), slice(body + 2 * w, body + 2 * w + n_out)


# 'reference' is the reference's DDPG widths pi=[300, 200], qf=[200, 150]; 'sb3' is SB3's default [256, 256], what SAC("MlpPolicy", env)
# builds
ARCHS = {a.name: a for a in (Arch("reference", _lib.ARCH_REFERENCE, (300, 200), (200, 150)),
                             Arch("sb3", _lib.ARCH_SAC_DEFAULT, (256, 256), (256, 256)))}
REFERENCE, SB3 = ARCHS["reference"], ARCHS["sb3"]
# _lib.py spells the header's arithmetic out (tests/test_c_abi.py holds it against include/brs_policy.h): the table must agree
assert (REFERENCE.actor.count, REFERENCE.critic.count, REFERENCE.nactor) == (_lib.DDPG_NACTOR, _lib.DDPG_NCRITIC, _lib.SAC_NACTOR)
assert (SB3.nactor, SB3.ncritic) == (_lib.SAC256_NACTOR, _lib.SAC256_NCRITIC)
assert all(sum(int(np.prod(s)) for _, s in a.sac_actor_layout("abcd")) == a.nactor for a in ARCHS.values())
ARCH_NAMES = " or ".join(repr(name) for name in ARCHS)


def arch(net_arch):
    if isinstance(net_arch, Arch):
        return net_arch
    if net_arch not in ARCHS:
        raise ValueError(f"net_arch must be {ARCH_NAMES}, got {net_arch!r}")
    return ARCHS[net_arch]


def pack(sd, layout):
    """the tensors or arrays `layout` [(name, shape)] names in `sd` -> one flat float32 vector in that order"""
    parts = []
    for name, shape in layout:
        if name not in sd:
            raise ValueError(f"{name}: missing")
        a = _numpy(sd[name])
        if tuple(a.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(a.shape)}")
        parts.append(a.astype(np.float32).ravel())
    return np.concatenate(parts)


def unpack(flat, layout):
    """the inverse: a flat float32 array of the layout's length -> {name: torch tensor (a copy)}"""
    out, at = {}, 0
    for name, shape in layout:
        k = int(np.prod(shape))
        out[name] = torch.from_numpy(flat[at:at + k].reshape(shape).copy())
        at += k
    return out


def flat_array(flat):
    """a flat vector as tensor or array -> contiguous float32 numpy"""
    return np.ascontiguousarray(_numpy(flat), dtype=np.float32)


def widths_of(sd, layouts, what):
    """the first of `layouts` (lists of (name, shape), one per row of ARCHS) whose every tensor is in `sd` with its shape; ValueError
    naming the first tensor that is missing or fits none of them"""
    for name, _ in layouts[0]:
        if name not in sd:
            raise ValueError(f"{name}: missing")
    for layout in layouts:
        if all(tuple(sd[name].shape) == shape for name, shape in layout):
            return layout
    for i, (name, shape) in enumerate(layouts[0]):
        if not any(tuple(sd[name].shape) == layout[i][1] for layout in layouts):
            expected = " or ".join(str(layout[i][1]) for layout in layouts)
            raise ValueError(f"{name}: expected shape {expected}, got {tuple(sd[name].shape)}")
    name = next(name for i, (name, shape) in enumerate(layouts[0]) if tuple(sd[name].shape) != shape)
    raise ValueError(f"{name}: shape {tuple(sd[name].shape)} mixes the widths of two architectures of {what}")
