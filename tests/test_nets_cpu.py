"""The one network table of the Python layer (balance_robot_mujoco_rl_amd/nets.py): what is derived from its two rows equals what
_lib.py, offpolicy.py and quant.py held by hand before it, written out here as literals."""
import numpy as np
import pytest

from balance_robot_mujoco_rl_amd import _lib, nets, offpolicy, quant

WIDTHS = {"reference": ((300, 200), (200, 150)), "sb3": ((256, 256), (256, 256))}
# (id, nactor, ncritic, grad_len) of offpolicy.SAC_ARCHS before the table
SAC_ARCHS = {"reference": (0, 63104, 32101, 63109), "sb3": (1, 68612, 68353, 68617)}


def test_derived_counts_equal_the_constants_of_lib():
    ref, sb3 = nets.ARCHS["reference"], nets.ARCHS["sb3"]
    assert (ref.actor.count, ref.critic.count, ref.nactor) == (_lib.DDPG_NACTOR, _lib.DDPG_NCRITIC, _lib.SAC_NACTOR) == (62702, 32101, 63104)
    assert (sb3.nactor, sb3.ncritic) == (_lib.SAC256_NACTOR, _lib.SAC256_NCRITIC) == (68612, 68353)
    assert (offpolicy.NACTOR, offpolicy.NCRITIC, offpolicy.NCRITIC256, offpolicy.SAC_NACTOR, offpolicy.SAC256_NACTOR, offpolicy.SAC_GRAD_LEN) == \
        (62702, 32101, 68353, 63104, 68612, 63104 + 1 + _lib.SAC_NSTAT)


def test_derived_shapes_equal_the_lists_offpolicy_held():
    assert offpolicy.ACTOR_SHAPES == [((300, 6), (300,)), ((200, 300), (200,)), ((2, 200), (2,))]
    assert offpolicy.CRITIC_SHAPES == [((200, 8), (200,)), ((150, 200), (150,)), ((1, 150), (1,))]
    assert nets.ARCHS["sb3"].critic.shapes == [((256, 8), (256,)), ((256, 256), (256,)), ((1, 256), (1,))]
    assert nets.REFERENCE.actor.layout("actor.mu.{}.")[:3] == [("actor.mu.0.weight", (300, 6)), ("actor.mu.0.bias", (300,)), ("actor.mu.2.weight", (200, 300))]


@pytest.mark.parametrize("name", ("reference", "sb3"))
def test_an_architecture_follows_from_its_widths(name):
    (p0, p1), (q0, q1) = WIDTHS[name]
    a = offpolicy.SAC_ARCHS[name]
    assert list(offpolicy.SAC_ARCHS) == ["reference", "sb3"] and a is nets.ARCHS[name] and isinstance(a, offpolicy.SacArch) and offpolicy.sac_arch(name) is a
    assert offpolicy.sac_arch(a) is a and (a.name, a.pi, a.qf) == (name, (p0, p1), (q0, q1))
    assert (a.id, a.nactor, a.ncritic, a.grad_len) == SAC_ARCHS[name]
    assert a.nactor == 6 * p0 + p0 + p0 * p1 + p1 + 4 * p1 + 4 and a.ncritic == 8 * q0 + q0 + q0 * q1 + q1 + q1 + 1
    # the SAC actor's four layers with the stacked head in its flat order
    names = [n for n, _ in a.sac_actor_layout(("b0.", "b1.", "mu.", "ls."))]
    assert names == ["b0.weight", "b0.bias", "b1.weight", "b1.bias", "mu.weight", "ls.weight", "mu.bias", "ls.bias"]
    shapes = [s for _, s in a.sac_actor_layout(("b0.", "b1.", "mu.", "ls."))]
    assert shapes == [(p0, 6), (p0,), (p1, p0), (p1,), (2, p1), (2, p1), (2,), (2,)] and sum(int(np.prod(s)) for s in shapes) == a.nactor
    # quant's layer sizes, and the slices that drop the log_std head
    assert quant._actor_sizes(name) == ((6, p0), (p0, p1), (p1, 2))
    n01 = 6 * p0 + p0 + p0 * p1 + p1
    assert a.sac_mu_slices() == (slice(0, n01), slice(n01, n01 + 2 * p1), slice(n01 + 4 * p1, n01 + 4 * p1 + 2))
    assert sum(s.stop - s.start for s in a.sac_mu_slices()) == a.actor.count


def test_unknown_architectures_are_named():
    for bad in ("td3", (400, 300)):
        with pytest.raises(ValueError, match="net_arch must be 'reference' or 'sb3'"):
            nets.arch(bad)


def test_pack_and_unpack_are_inverse_and_say_what_is_wrong():
    layout = [("a.weight", (3, 2)), ("a.bias", (3,)), ("s", (1,))]
    sd = {"a.weight": np.arange(6.0).reshape(3, 2), "a.bias": [6, 7, 8], "s": np.array([9.0]), "extra": np.zeros(4)}
    flat = nets.pack(sd, layout)
    assert flat.dtype == np.float32 and flat.tolist() == list(range(10))
    out = nets.unpack(flat, layout)
    assert list(out) == ["a.weight", "a.bias", "s"] and out["a.weight"].shape == (3, 2) and out["s"].shape == (1,)
    assert nets.pack(out, layout).tobytes() == flat.tobytes()
    out["a.bias"][0] = 100.0   # copies: the flat vector is not written through
    assert flat[6] == 6.0
    with pytest.raises(ValueError, match="^a.bias: missing$"):
        nets.pack({"a.weight": sd["a.weight"]}, layout)
    with pytest.raises(ValueError, match=r"^a.weight: expected shape \(3, 2\), got \(2, 3\)$"):
        nets.pack({**sd, "a.weight": np.zeros((2, 3))}, layout)
