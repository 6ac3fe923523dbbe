"""Every entry point of the C ABI runs on its HANDLE's device and leaves the caller's current device alone (the shared
DeviceGuard of csrc/brs_host.hpp): one short session over the simulator, both policies and the renderer, all handles on
device 0, run with current device 0 and -- where the machine has a second device -- with current device 1, and compared
bit for bit.  Env03-v2 at 65 envs: one full wave plus one lane, lane grouping on."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tests import qpolicy_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu

N = 65


def session(current):
    """the whole sequence with `current` as the current device; asserts after every call that it still is -> all results"""
    from balance_robot_mujoco_rl_amd import BatchedSim, _lib
    from balance_robot_mujoco_rl_amd.policy import DevicePolicy
    from balance_robot_mujoco_rl_amd.quant import QuantPolicy
    dev0 = torch.device("cuda", 0)
    out, calls = {}, []

    def after(call):
        calls.append(call)
        assert torch.cuda.current_device() == current, f"{call} left device {torch.cuda.current_device()} current, not {current}"

    def keep(name, *tensors):
        torch.cuda.synchronize(dev0)
        for k, t in enumerate(tensors):
            out[f"{name}/{k}"] = t.cpu().numpy().copy() if isinstance(t, torch.Tensor) else np.array(t, copy=True)

    torch.cuda.set_device(current)
    try:
        rng = np.random.default_rng(11)
        sim = BatchedSim("Env03-v2", N, device=0, seed=11); after("brs_create")
        pol = DevicePolicy(device=0, seed=3); after("brs_policy_create")
        pol.set_weights(rng.normal(0.0, 0.3, _lib.POLICY_NPARAM).astype(np.float32)); after("brs_policy_set_weights")
        qpol = QuantPolicy(K.quant_model(K.random_model(0)), device=0); after("brs_qpolicy_create / set_model")
        keep("reset", sim.reset()); after("brs_reset")
        for s in range(2):
            act = torch.from_numpy(rng.uniform(-1, 1, (N, 2)).astype(np.float32)).to(dev0)
            keep(f"step{s}", *sim.step(act)); after("brs_step")
        state = sim.get_state(); after("brs_get_state")
        keep("state", *state)
        sim.set_state(*state); after("brs_set_state")
        keep("state again", *sim.get_state(), sim.get_aux(), *sim.get_xpose()); after("brs_get_aux / brs_get_xpose")
        obs = sim.obs.clone()
        a = pol.act(obs, step=0); after("brs_policy_act")
        keep("policy", *a)
        keep("qpolicy", qpol.act(obs)); after("brs_qpolicy_act")
        keep("render", sim.render([N - 1], camera=dict(width=32, height=8))); after("brs_render")
        keep("step after set_state", *sim.step(a[1])); after("brs_step")   # the clipped actions of the policy
        keep("final state", *sim.get_state())
        sim.close(); pol.close(); qpol.close(); after("destroy")
    finally:
        torch.cuda.set_device(0)
    assert len(calls) == 15
    return out


@pytest.fixture(scope="module")
def from_device_0():
    return session(0)


def test_current_device_0_stays_current(from_device_0):
    out = from_device_0
    assert out["render/0"].shape == (1, 8, 32, 3) and out["policy/0"].shape == (N, 2) and out["qpolicy/0"].shape == (N, 2)
    # set_state normalises the quaternions it is given: unit ones move by rounding only
    assert np.abs(out["state/0"] - out["state again/0"]).max() < 1e-12, "get_state / set_state / get_state changed qpos"
    assert not np.array_equal(out["step1/0"], out["step after set_state/0"]), "the session did not advance"
    assert len(np.unique(out["render/0"])) > 2, "the image is blank"


def test_handles_on_device_0_with_device_1_current(from_device_0):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second device to be the current one")
    out = session(1)
    assert sorted(out) == sorted(from_device_0)
    for name, ref in from_device_0.items():
        assert out[name].dtype == ref.dtype and out[name].shape == ref.shape, name
        assert np.array_equal(out[name].view(np.uint8), ref.view(np.uint8)), f"{name} differs with another current device"
