"""The one handle base of the Python layer (balance_robot_mujoco_rl_amd/_handle.py) without a GPU and without the library: a stub
library object records every call.  The lifecycle (create with the out-pointer last, destroy exactly once, a silent __del__),
_check's and a failed create's error texts, and the refusal of every class without a HIP device, before the library is loaded."""
import ctypes as C

import pytest
import torch

import balance_robot_mujoco_rl_amd as B
from balance_robot_mujoco_rl_amd import _handle, _lib, learner, policy


class StubLib:
    """every attribute is a C entry point that records its call; *_create* writes a handle through its last argument"""

    def __init__(self, create_rc=0):
        self.calls, self.create_rc = [], create_rc

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name.endswith("_last_error"):
                return b"stub: no handle" if not args or args[0] is None else b"stub: handle %x" % args[0].value
            if "_create" in name:
                if self.create_rc == 0:
                    args[-1]._obj.value = 0xbeef
                return self.create_rc
            return 0
        return call

    def names(self):
        return [name for name, _ in self.calls]


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    return lib


class Thing(_handle.Handle):
    _FAMILY, _WHAT = "brs_thing", "the thing has"

    def __init__(self, device=0, size=3):
        self._attach(device)
        self._create("brs_thing_create_sized", self.device.index, size)


def test_create_passes_the_out_pointer_last_and_close_destroys_once(stub):
    t = Thing("cuda:1", size=5)
    assert t.L is stub and t.device == torch.device("cuda", 1) and t.h.value == 0xbeef
    (name, args), = stub.calls
    assert name == "brs_thing_create_sized" and args[:2] == (1, 5) and len(args) == 3 and args[2]._obj is t.h
    t.close()
    assert stub.names()[1:] == ["brs_thing_destroy"] and stub.calls[1][1][0].value == 0xbeef and t.h is None
    t.close(); t.__del__(); del t
    assert stub.names() == ["brs_thing_create_sized", "brs_thing_destroy"]   # the second close and __del__ call nothing


@pytest.mark.parametrize("device,index", ((0, 0), (2, 2), ("cuda", 0), ("cuda:3", 3), (torch.device("cuda", 1), 1)))
def test_device_normalisation(stub, device, index):
    assert Thing(device).device == torch.device("cuda", index)


def test_del_is_silent_when_init_raised_before_the_handle_existed(stub):
    t = object.__new__(Thing)   # what Python is left with when __init__ raises in _attach
    t.__del__(); t.close()
    assert stub.calls == []

    class Broken(Thing):
        def close(self):
            raise RuntimeError("destroy failed")
    Broken().__del__()   # __del__ swallows whatever close raises


def test_check_is_silent_on_zero_and_reads_the_handles_error_otherwise(stub):
    t = Thing()
    t._check(0, "brs_thing_do")
    assert stub.names() == ["brs_thing_create_sized"]
    with pytest.raises(B.BrsError) as e:
        t._check(-3, "brs_thing_do")
    assert str(e.value) == "brs_thing_do failed (-3): stub: handle beef"
    assert stub.calls[-1][0] == "brs_thing_last_error" and stub.calls[-1][1][0] is t.h


def test_a_failing_create_raises_with_the_creates_error_and_leaves_no_handle(stub):
    stub.create_rc = -2
    t = object.__new__(Thing)
    with pytest.raises(B.BrsError) as e:
        t.__init__()
    assert str(e.value) == "brs_thing_create_sized failed (-2): stub: no handle"
    assert stub.calls[-1] == ("brs_thing_last_error", (None,)) and not hasattr(t, "h")
    t.close(); t.__del__()
    assert "brs_thing_destroy" not in stub.names()


def test_a_real_class_on_the_stub_calls_its_own_entry_points(stub):
    m = B.EpisodeMonitor(3, device=0, max_len=7, log_capacity=2)
    name, args = stub.calls[0]
    assert name == "brs_monitor_create" and args[:4] == (0, 3, 7, 2) and args[4]._obj is m.h
    stub.create_rc = -1
    with pytest.raises(B.BrsError, match=r"^brs_ddpg_learner_create_twin failed \(-1\): stub: no handle$"):
        B.DeviceTD3Learner()
    assert stub.calls[-2][0] == "brs_ddpg_learner_create_twin" and stub.calls[-1] == ("brs_ddpg_learner_last_error", (None,))
    m.close(); m.close()
    assert stub.names().count("brs_monitor_destroy") == 1


def test_stream_is_the_current_stream_of_the_objects_device(stub, monkeypatch):
    seen = []

    class Stream:
        cuda_stream = 0x51

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device: seen.append(device) or Stream())
    t = Thing(2)
    assert t._stream().value == 0x51 and seen == [torch.device("cuda", 2)]


# (constructor, the refusal's wording): every class that opens a handle, and the replay buffer, which takes only the helpers
REFUSALS = [(lambda: B.BatchedSim("Env01-v1", 1), "the batched simulator has no CPU fallback"),
            (lambda: policy.DevicePolicy(), "the on-device policy has no CPU fallback"),
            (lambda: learner._DeviceLearner()._open(0, 0), "the on-device learner has no CPU fallback"),
            (lambda: B.DevicePPOLearner(), "the on-device learner has no CPU fallback"),
            (lambda: B.DeviceA2CLearner(), "the on-device learner has no CPU fallback"),
            (lambda: B.EpisodeMonitor(1), "the episode monitor has no CPU fallback"),
            (lambda: B.QuantPolicy(None), "the int8 policy has no CPU fallback"),
            (lambda: B.QuantActor(None), "the int8 actor has no CPU fallback"),
            (lambda: B.DeviceDDPGNets(), "the on-device DDPG networks have no CPU fallback"),
            (lambda: B.DeviceDDPGLearner(), "the on-device DDPG learner has no CPU fallback"),
            (lambda: B.DeviceTD3Learner(), "TD3 learner has no CPU fallback"),
            (lambda: B.DeviceTD3Learner(policy_delay=0), "the on-device TD3 learner has no CPU fallback"),
            (lambda: B.DeviceSACLearner(), "SAC learner has no CPU fallback"),
            (lambda: B.DeviceSACLearner(net_arch="td3"), "the on-device SAC learner has no CPU fallback"),
            (lambda: B.DeviceSACNets(), "the on-device SAC networks have no CPU fallback"),
            (lambda: B.DeviceSACNets(net_arch="td3"), "the on-device SAC networks have no CPU fallback"),
            (lambda: B.DeviceReplayBuffer(1, 1), "the on-device replay buffer has no CPU fallback"),
            (lambda: B.DeviceReplayBuffer(0, 0), "the on-device replay buffer has no CPU fallback")]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_every_class_refuses_without_a_device_before_the_library_is_loaded(monkeypatch, k):
    """the arguments these classes check after the refusal today (policy_delay, net_arch, the buffer's sizes) still come after it"""
    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_lib, "lib", no_library)
    make, wording = REFUSALS[k]
    with pytest.raises(B.BrsError) as e:
        make()
    assert "no CPU fallback" in str(e.value) and wording in str(e.value)
    assert str(e.value).startswith("no HIP device visible to PyTorch: ")


def test_an_unknown_env_is_refused_before_the_device_is_asked_for(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(Exception) as e:
        B.BatchedSim("Env99-v0", 1)
    assert not isinstance(e.value, B.BrsError)


def test_argument_checks_after_the_refusal_raise_what_they_raised(stub):
    with pytest.raises(ValueError, match="policy_delay must be at least 1, got 0"):
        B.DeviceTD3Learner(policy_delay=0)
    with pytest.raises(ValueError, match="net_arch must be 'reference' or 'sb3', got 'td3'"):
        B.DeviceSACLearner(net_arch="td3")
    with pytest.raises(ValueError, match="net_arch must be 'reference' or 'sb3', got 'td3'"):
        B.DeviceSACNets(net_arch="td3")
    with pytest.raises(ValueError, match="need n_envs >= 1, capacity_steps >= 1"):
        B.DeviceReplayBuffer(0, 1)
    assert stub.calls == []   # nothing was created on the way


def test_no_class_but_the_bases_defines_the_lifecycle():
    import inspect
    from balance_robot_mujoco_rl_amd import monitor, offpolicy, quant, sim
    own = {}
    for mod in (sim, policy, learner, monitor, quant, offpolicy):
        for name, cls in inspect.getmembers(mod, inspect.isclass):
            if cls.__module__ == mod.__name__:
                own[name] = sorted(set(vars(cls)) & {"close", "__del__", "_check", "_stream"})
    assert {k: v for k, v in own.items() if v} == {"DeviceReplayBuffer": ["_check"]}
    for name in ("BatchedSim", "DevicePolicy", "_DeviceLearner", "EpisodeMonitor", "QuantPolicy", "QuantActor", "DeviceDDPGNets", "DeviceDDPGLearner",
                 "DeviceTD3Learner", "DeviceSACLearner", "DeviceSACNets"):
        cls = next(getattr(m, name) for m in (sim, policy, learner, monitor, quant, offpolicy) if hasattr(m, name))
        assert issubclass(cls, _handle.Handle) and cls._FAMILY and cls._WHAT, name
    assert issubclass(offpolicy.DeviceReplayBuffer, _handle.DeviceObject) and not issubclass(offpolicy.DeviceReplayBuffer, _handle.Handle)
    assert policy._p is _handle._p and policy._need is _handle._need and sim.BrsError is _handle.BrsError is B.BrsError
