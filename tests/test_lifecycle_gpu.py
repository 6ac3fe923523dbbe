"""The life of every object of the Python layer on a real device, at the smallest legal sizes: construct, one cheap call that needs
no trained weights, close(), close() again, delete.  The classes share one handle base (balance_robot_mujoco_rl_amd/_handle.py);
tests/test_handle_cpu.py holds the same lifecycle against a stub library."""
import numpy as np
import pytest
import torch

import balance_robot_mujoco_rl_amd as B
from balance_robot_mujoco_rl_amd import offpolicy, policy, quant

pytestmark = pytest.mark.gpu


def _dev(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device="cuda:0")


def _sim():
    s = B.BatchedSim("Env01-v1", 1)
    assert s.reset().shape == (1, 6) and s.step_kernel_name()
    return s


def _policy():
    p = policy.DevicePolicy()
    p.set_weights(np.zeros(policy.NPARAM, np.float32))
    return p


def _ppo():
    lrn = B.DevicePPOLearner()
    lrn.begin_iteration()
    assert lrn.stats().steps == 0
    return lrn


def _a2c():
    lrn = B.DeviceA2CLearner()
    assert lrn.stats().steps == 0
    return lrn


def _monitor():
    m = B.EpisodeMonitor(1)
    m.reset()
    assert m.stats().episodes == 0
    return m


def _qpolicy():
    q = B.QuantPolicy(quant.quantize_policy(np.random.default_rng(0).uniform(-0.5, 0.5, policy.NPARAM)))
    assert q.act(_dev(1, 6)).shape == (1, 2)
    return q


def _qactor():
    q = B.QuantActor(quant.quantize_actor(np.random.default_rng(0).uniform(-0.1, 0.1, offpolicy.NACTOR)))
    assert q.net_arch == "reference" and q.act(_dev(1, 6)).shape == (1, 2)
    return q


def _nets(cls, **kw):
    def make():
        n = cls(**kw)
        n.act(None, None, 0, 0.1, random=True, out=_dev(1, 2))   # the learning_starts phase: uniform, no weights read
        return n
    return make


def _learner(cls, **kw):
    def make():
        lrn = cls(max_batch=1, **kw)
        ptr, size = lrn.scratch()
        assert ptr and size > 0 and lrn.state_dict()["steps_actor"] == 0
        return lrn
    return make


def _replay():
    r = B.DeviceReplayBuffer(1, 1)
    r.add(_dev(1, 6), _dev(1, 2), _dev(1, 6), _dev(1, 6), _dev(1), _dev(1, dtype=torch.uint8), _dev(1, dtype=torch.uint8))
    assert len(r) == 1 and r.sample(1)[0].shape == (1, 6)
    return r


OBJECTS = {"BatchedSim": _sim, "DevicePolicy": _policy, "DevicePPOLearner": _ppo, "DeviceA2CLearner": _a2c, "EpisodeMonitor": _monitor,
           "QuantPolicy": _qpolicy, "QuantActor": _qactor, "DeviceDDPGNets": _nets(B.DeviceDDPGNets), "DeviceDDPGLearner": _learner(B.DeviceDDPGLearner),
           "DeviceTD3Learner": _learner(B.DeviceTD3Learner), "DeviceSACLearner": _learner(B.DeviceSACLearner),
           "DeviceSACLearner-sb3": _learner(B.DeviceSACLearner, net_arch="sb3"), "DeviceSACNets": _nets(B.DeviceSACNets),
           "DeviceSACNets-sb3": _nets(B.DeviceSACNets, net_arch="sb3"), "DeviceReplayBuffer": _replay}


@pytest.mark.parametrize("name", OBJECTS)
def test_construct_call_close_twice_delete(name):
    obj = OBJECTS[name]()
    torch.cuda.synchronize()
    assert obj.device == torch.device("cuda", 0) and type(obj).__name__ == name.split("-")[0]
    if name != "DeviceReplayBuffer":   # it owns tensors only: no handle, nothing to close
        assert obj.h
        obj.close()
        assert obj.h is None
        obj.close()
    del obj
