"""The int8 off-policy actor on the GPU: brs_qpolicy_actor_act against the independent integer reference
(tests/ref_qactor.py), exactly -- int8 codes and float32 actions -- at the edges of its 64-env wave and 256-env workgroup tiling,
then the user's path through a file, then in closed loop with the simulator, then captured into a graph.  The random models are
the check the matrix-core operand layout needs (exact integer data, asymmetric weights, a non-zero zero point on every tensor);
the edge-unit models pin down the tile and padding edges of the two hidden layers."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tests import qactor_cases as K  # noqa: E402
from tests import ref_qactor as R  # noqa: E402

pytestmark = pytest.mark.gpu

# one lane; a wave's tail, a full wave, a second wave; a workgroup's tail, a full workgroup, a second one; a 17th with one env
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
GUARD, SENTINEL_F, SENTINEL_Q = 64, -777.0, 77
# closed loop: envs of 1,024 still up after 300 steps, measured once on an MI355X: float 1024, int8 1024.  The
# margin is twice the observed gap (0), but no less than 8 envs, so that a reseed does not fail it
ALIVE_MARGIN = 8


@pytest.fixture(scope="module")
def cases():
    """[(name, model dict, obs, reference actions, reference codes)], computed once at the largest size; the first rows are the
    special rows"""
    obs = np.concatenate([K.special_rows(), K.seeded_obs(max(SIZES))])[:max(SIZES)]
    return [(name, m, obs) + R.act(m, obs) for name, m in K.all_models()]


def run_guarded(pol, obs_np, n, want_q=True):
    """act on the first n rows with 64 guard rows of a sentinel behind row n of every output"""
    obs = torch.from_numpy(np.ascontiguousarray(obs_np[:n])).cuda()
    a = torch.full((n + GUARD, 2), SENTINEL_F, dtype=torch.float32, device="cuda")
    q = torch.full((n + GUARD, 2), SENTINEL_Q, dtype=torch.int8, device="cuda")
    out = pol.act(obs, out=a[:n], out_q=q[:n] if want_q else None)
    assert out.data_ptr() == a.data_ptr()
    torch.cuda.synchronize()
    a, q = a.cpu().numpy(), q.cpu().numpy()
    assert (a[n:] == SENTINEL_F).all() and (q[n:] == SENTINEL_Q).all(), f"n = {n}: a guard row was written"
    return a[:n], q[:n]


@pytest.mark.parametrize("which", range(17))
def test_kernel_equals_reference_at_the_tile_edges(cases, which):
    from balance_robot_mujoco_rl_amd import QuantActor
    name, model, obs, a_ref, q_ref = cases[which]
    pol = QuantActor(K.quant_model(model), device=0)
    for n in SIZES:
        a, q = run_guarded(pol, obs, n)
        bad = (q != q_ref[:n]).any(axis=1)
        assert not bad.any(), f"{name}, n = {n}: codes differ on {int(bad.sum())} rows, first {int(np.argmax(bad))}: {q[bad][0]} vs {q_ref[:n][bad][0]}"
        assert np.array_equal(a, a_ref[:n]), f"{name}, n = {n}: actions differ"
    a, q = run_guarded(pol, obs, 65, want_q=False)
    assert np.array_equal(a, a_ref[:65]) and (q == SENTINEL_Q).all(), "out_q = None"
    pol.close()


def test_user_path_through_a_file(tmp_path):
    """quantize_actor -> save -> QuantActorModel.load -> QuantActor.act allocating its own output"""
    from balance_robot_mujoco_rl_amd import QuantActor, QuantActorModel, quantize_actor
    path = str(tmp_path / "actor_int8.npz")
    quantize_actor(K.sb3_init_params(2)).save(path)
    model = QuantActorModel.load(path)
    obs = np.concatenate([K.special_rows(), K.in_box_obs(300)])[:300]
    a_ref, q_ref = R.act(K.as_ref_model(model), obs)
    pol = QuantActor(model, device=0)
    a = pol.act(torch.from_numpy(obs).cuda())
    assert a.shape == (300, 2) and a.dtype == torch.float32 and np.array_equal(a.cpu().numpy(), a_ref)
    assert len(np.unique(q_ref)) > 20
    pol.close()


def test_second_set_model_takes_effect_and_arguments_are_checked(cases):
    from balance_robot_mujoco_rl_amd import QuantActor
    from balance_robot_mujoco_rl_amd.sim import BrsError
    (_, m0, obs, a0, q0), (_, m1, _, a1, q1) = cases[0], cases[1]
    pol = QuantActor(K.quant_model(m0), device=0)
    assert np.array_equal(run_guarded(pol, obs, 65)[1], q0[:65])
    pol.set_model(K.quant_model(m1))
    a, q = run_guarded(pol, obs, 65)
    assert np.array_equal(q, q1[:65]) and np.array_equal(a, a1[:65]) and not np.array_equal(q0[:65], q1[:65])
    x = torch.zeros((8, 6), device="cuda")
    for bad in (x.cpu(), x.double(), x[:, :5], x.t().contiguous().t(), torch.zeros((8, 7), device="cuda")):
        with pytest.raises(ValueError):
            pol.act(bad)
    with pytest.raises(ValueError):
        pol.act(x, out=torch.zeros((8, 3), device="cuda"))
    with pytest.raises(ValueError):
        pol.act(x, out_q=torch.zeros((8, 2), dtype=torch.uint8, device="cuda"))
    with pytest.raises(BrsError):
        pol.act(torch.zeros((0, 6), device="cuda"))
    broken = K.quant_model(m0)
    broken.layers[1]["oz"] = 200
    with pytest.raises(BrsError, match="layer 1: out_zero"):
        pol.set_model(broken)
    assert np.array_equal(run_guarded(pol, obs, 65)[1], q1[:65]), "a rejected model leaves the loaded one in place"
    pol.close()


def test_closed_loop_on_the_device():
    """1,024 Env01-v1 envs for 300 steps under the quantised PD actor: every recorded step's codes and actions equal the integer
    reference evaluated on the host on the recorded observations, and the int8 actor keeps as many envs up as the float PD actor
    (DeviceDDPGNets.act, sigma 0) on the same seed, less ALIVE_MARGIN"""
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceDDPGNets, QuantActor, quantize_actor
    n, steps = 1024, 300
    flat = K.pd_actor_params()
    qm = quantize_actor(flat)

    def run(act):
        sim = BatchedSim("Env01-v1", n, device=0, seed=11, auto_reset=False)
        obs = sim.reset()
        alive = torch.ones(n, dtype=torch.bool, device="cuda")
        for k in range(steps):
            obs, _, te, _, _ = sim.step(act(k, obs))
            alive &= ~te.bool()
        up = int(alive.sum().item())
        sim.close()
        return up

    pol = QuantActor(qm, device=0)
    O = torch.empty((steps, n, 6), device="cuda")
    A, Q = torch.empty((steps, n, 2), device="cuda"), torch.empty((steps, n, 2), dtype=torch.int8, device="cuda")

    def act_int8(k, obs):
        O[k].copy_(obs)
        return pol.act(obs, out=A[k], out_q=Q[k])
    up_q = run(act_int8)
    pol.close()
    a_ref, q_ref = R.act(K.as_ref_model(qm), O.reshape(-1, 6).cpu().numpy())
    mismatches = int((Q.reshape(-1, 2).cpu().numpy() != q_ref).sum() + (A.reshape(-1, 2).cpu().numpy() != a_ref).sum())
    assert mismatches == 0, f"{mismatches} action components differ from the reference"
    assert len(np.unique(q_ref)) > 2, "a controller that balances pushes both ways: negative, zero and positive codes"

    nets = DeviceDDPGNets(device=0)
    params = torch.from_numpy(flat).cuda()
    a = torch.empty((n, 2), device="cuda")
    up_f = run(lambda k, obs: nets.act(params, obs, k, 0.0, out=a))
    nets.close()
    print(f"alive after {steps} steps of {n}: float {up_f}, int8 {up_q}")
    assert up_f >= 0.9 * n, f"the float PD actor keeps only {up_f} of {n} up: the gains are a bad input"
    assert up_q >= up_f - ALIVE_MARGIN, f"int8 {up_q} vs float {up_f}"


def test_act_and_step_replay_from_a_graph():
    """act -> sim.step captured on one stream (no parallel branches) replays to the actions and observations of the eager
    calls: brs_qpolicy_actor_act only enqueues"""
    from balance_robot_mujoco_rl_amd import BatchedSim, QuantActor, quantize_actor
    n, steps = 300, 12
    pol = QuantActor(quantize_actor(K.pd_actor_params()), device=0)

    def run(graph):
        sim = BatchedSim("Env01-v1", n, device=0, seed=5, auto_reset=False)
        obs = sim.reset()
        a, q = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 2), dtype=torch.int8, device="cuda")
        A, O = [], []

        def body():
            pol.act(obs, out=a, out_q=q)
            return sim.step(a)[0]
        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):   # warm-up outside the capture, as PyTorch asks
                    o = body(); A.append(a.clone()); O.append(o.clone())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    o = body()
                assert o.data_ptr() == obs.data_ptr(), "the step writes the observation buffer the actor reads"
                for _ in range(steps - 2):
                    g.replay(); A.append(a.clone()); O.append(o.clone())
            torch.cuda.current_stream().wait_stream(s)
        else:
            for _ in range(steps):
                o = body(); A.append(a.clone()); O.append(o.clone())
        torch.cuda.synchronize()
        sim.close()
        return torch.stack(A).cpu().numpy(), torch.stack(O).cpu().numpy()

    A0, O0 = run(False)
    A1, O1 = run(True)
    assert np.array_equal(A0, A1) and np.array_equal(O0, O1)
    assert len(np.unique(A0)) > 2, "the replayed steps are not a constant"
    pol.close()
