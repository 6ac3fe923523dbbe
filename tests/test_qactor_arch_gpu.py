"""The int8 off-policy actor at its second width set, 6 -> 256 -> 256 -> 2 (SB3's SAC default), on the GPU:
brs_qpolicy_actor_act on an arch-1 handle against the independent integer reference (tests/ref_qactor.py), exactly -- int8 codes
and float32 actions -- at the edges of its 64-env wave and 256-env workgroup tiling, then the user's path through a file, the
refusal of a model of the other widths, the reference widths through the same dispatch, the closed loop with the simulator next
to the float SAC actor of the same widths, graph capture, and the evaluation tool end to end.  The cases are
tests/qactor_cases.py's at these widths (tests/qactor_arch_cases.py): the random models check the matrix-core operand layout, the
edge-unit models the first and last unit of the first, second and last tile -- 255 being the last register of the last tile."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tests import qactor_arch_cases as A  # noqa: E402
from tests import qactor_cases as K0  # noqa: E402
from tests import ref_qactor as R  # noqa: E402

K = A.K
pytestmark = pytest.mark.gpu

# one lane; a wave's tail, a full wave, a second wave; a workgroup's tail, a full workgroup, a second one; a 17th with one env
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
GUARD, SENTINEL_F, SENTINEL_Q = 64, -777.0, 77
# closed loop: envs of 1,024 still up after 300 steps.  The rule is 7.11's: int8 >= float - max(8, twice the
# observed gap), so that a reseed does not fail it; the gap observed on an MI355X at these widths is 0 (float 1024, int8 1024)
ALIVE_MARGIN = 8


@pytest.fixture(scope="module")
def cases():
    """[(name, model dict, obs, reference actions, reference codes)], computed once at the largest size; the first rows are the
    special rows"""
    obs = np.concatenate([K.special_rows(), K.seeded_obs(max(SIZES))])[:max(SIZES)]
    return [(name, m, obs) + R.act(m, obs) for name, m in A.all_models()]


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
    assert pol.net_arch == "sb3"
    for n in SIZES:
        a, q = run_guarded(pol, obs, n)
        bad = (q != q_ref[:n]).any(axis=1)
        assert not bad.any(), f"{name}, n = {n}: codes differ on {int(bad.sum())} rows, first {int(np.argmax(bad))}: {q[bad][0]} vs {q_ref[:n][bad][0]}"
        assert np.array_equal(a, a_ref[:n]), f"{name}, n = {n}: actions differ"
    a, q = run_guarded(pol, obs, 65, want_q=False)
    assert np.array_equal(a, a_ref[:65]) and (q == SENTINEL_Q).all(), "out_q = None"
    pol.close()


def test_user_path_through_a_file(tmp_path):
    """quantize_actor(net_arch="sb3") -> save -> QuantActorModel.load -> QuantActor.act allocating its own output"""
    from balance_robot_mujoco_rl_amd import QuantActor, QuantActorModel, quantize_actor
    path = str(tmp_path / "actor256_int8.npz")
    quantize_actor(A.sac_vector(K.sb3_init_params(2)), head="sac", net_arch="sb3").save(path)
    model = QuantActorModel.load(path)
    assert model.net_arch == "sb3"
    obs = np.concatenate([K.special_rows(), K.in_box_obs(300)])[:300]
    a_ref, q_ref = R.act(K.as_ref_model(model), obs)
    pol = QuantActor(model, device=0)
    a = pol.act(torch.from_numpy(obs).cuda())
    assert a.shape == (300, 2) and a.dtype == torch.float32 and np.array_equal(a.cpu().numpy(), a_ref)
    assert len(np.unique(q_ref)) > 20
    pol.close()


def test_second_set_model_takes_effect(cases):
    from balance_robot_mujoco_rl_amd import QuantActor
    (_, m0, obs, a0, q0), (_, m1, _, a1, q1) = cases[0], cases[1]
    pol = QuantActor(K.quant_model(m0), device=0)
    assert np.array_equal(run_guarded(pol, obs, 65)[1], q0[:65])
    pol.set_model(K.quant_model(m1))
    a, q = run_guarded(pol, obs, 257)
    assert np.array_equal(q, q1[:257]) and np.array_equal(a, a1[:257]) and not np.array_equal(q0[:65], q1[:65])
    pol.close()


def test_a_model_of_the_other_widths_is_refused_and_the_loaded_one_stays(cases):
    """a reference-width model on an arch-1 handle, and the converse: BrsError with the library's message, which names the network
    the handle serves; the model set before still answers, byte for byte"""
    from balance_robot_mujoco_rl_amd import QuantActor
    from balance_robot_mujoco_rl_amd.sim import BrsError
    _, m256, obs, a256, q256 = cases[0]
    m300 = K0.random_model(0)
    a300, q300 = R.act(m300, obs[:257])
    for mine, other, a_ref, q_ref, network in ((m256, m300, a256, q256, "6-256-256-2"), (m300, m256, a300, q300, "6-300-200-2")):
        pol = QuantActor(K.quant_model(mine), device=0)
        before = run_guarded(pol, obs, 257)
        with pytest.raises(BrsError, match=f"layer 0: the network must be {network}"):
            pol.set_model(K.quant_model(other))
        after = run_guarded(pol, obs, 257)
        for x, y, ref in zip(before, after, (a_ref[:257], q_ref[:257])):
            assert x.tobytes() == y.tobytes() == np.ascontiguousarray(ref).tobytes(), network
        pol.close()


def test_the_reference_widths_go_through_the_same_dispatch():
    """one 6-300-200-2 model at n = 257 against ref_qactor: the rebuilt library's arch-0 path (tests/test_qactor_gpu.py is the gate
    for that instantiation)"""
    from balance_robot_mujoco_rl_amd import QuantActor
    model = K0.random_model(1)
    obs = np.concatenate([K0.special_rows(), K0.seeded_obs(257)])[:257]
    a_ref, q_ref = R.act(model, obs)
    pol = QuantActor(K0.quant_model(model), device=0)
    assert pol.net_arch == "reference"
    a, q = run_guarded(pol, obs, 257)
    assert np.array_equal(q, q_ref) and np.array_equal(a, a_ref)
    pol.close()


def test_closed_loop_on_the_device():
    """1,024 Env01-v1 envs for 300 steps under the quantised PD actor at [256, 256]: every recorded step's codes and actions equal
    the integer reference evaluated on the host on the recorded observations, and the int8 actor keeps as many envs up as the float
    SAC actor of the same widths (DeviceSACNets(net_arch="sb3").act, deterministic: the PD weights in the mu rows, zero log_std
    rows) on the same seed, less ALIVE_MARGIN"""
    from balance_robot_mujoco_rl_amd import BatchedSim, DeviceSACNets, QuantActor
    n, steps = 1024, 300
    flat = A.pd_actor_params()
    qm = A.quantize(flat)

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
    Aq, Q = torch.empty((steps, n, 2), device="cuda"), torch.empty((steps, n, 2), dtype=torch.int8, device="cuda")

    def act_int8(k, obs):
        O[k].copy_(obs)
        return pol.act(obs, out=Aq[k], out_q=Q[k])
    up_q = run(act_int8)
    pol.close()
    a_ref, q_ref = R.act(K.as_ref_model(qm), O.reshape(-1, 6).cpu().numpy())
    mismatches = int((Q.reshape(-1, 2).cpu().numpy() != q_ref).sum() + (Aq.reshape(-1, 2).cpu().numpy() != a_ref).sum())
    assert mismatches == 0, f"{mismatches} action components differ from the reference"
    assert len(np.unique(q_ref)) > 2, "a controller that balances pushes both ways: negative, zero and positive codes"

    nets = DeviceSACNets(device=0, net_arch="sb3")
    params = torch.from_numpy(A.sac_vector(flat)).cuda()
    a = torch.empty((n, 2), device="cuda")
    up_f = run(lambda k, obs: nets.act(params, obs, k, deterministic=True, out=a))
    nets.close()
    print(f"alive after {steps} steps of {n}: float {up_f}, int8 {up_q}")
    assert up_f >= 0.9 * n, f"the float PD actor keeps only {up_f} of {n} up: the gains are a bad input"
    assert up_q >= up_f - ALIVE_MARGIN, f"int8 {up_q} vs float {up_f}"


def test_act_and_step_replay_from_a_graph():
    """act -> sim.step captured on one stream (no parallel branches) replays to the actions and observations of the eager
    calls: brs_qpolicy_actor_act on an arch-1 handle only enqueues"""
    from balance_robot_mujoco_rl_amd import BatchedSim, QuantActor
    n, steps = 300, 12
    pol = QuantActor(A.quantize(A.pd_actor_params()), device=0)

    def run(graph):
        sim = BatchedSim("Env01-v1", n, device=0, seed=5, auto_reset=False)
        obs = sim.reset()
        a, q = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 2), dtype=torch.int8, device="cuda")
        As, Os = [], []

        def body():
            pol.act(obs, out=a, out_q=q)
            return sim.step(a)[0]
        if graph:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):   # warm-up outside the capture, as PyTorch asks
                    o = body(); As.append(a.clone()); Os.append(o.clone())
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    o = body()
                assert o.data_ptr() == obs.data_ptr(), "the step writes the observation buffer the actor reads"
                for _ in range(steps - 2):
                    g.replay(); As.append(a.clone()); Os.append(o.clone())
            torch.cuda.current_stream().wait_stream(s)
        else:
            for _ in range(steps):
                o = body(); As.append(a.clone()); Os.append(o.clone())
        torch.cuda.synchronize()
        sim.close()
        return torch.stack(As).cpu().numpy(), torch.stack(Os).cpu().numpy()

    A0, O0 = run(False)
    A1, O1 = run(True)
    assert np.array_equal(A0, A1) and np.array_equal(O0, O1)
    assert len(np.unique(A0)) > 2, "the replayed steps are not a constant"
    pol.close()


def test_eval_tool_reads_a_256_wide_actor_file(tmp_path):
    """tools/eval_quant_policy.py --actor FILE --algo sac on a [256, 256] actor vector as tools/train_sac_torch.py --net-arch sb3
    --save-actor writes it: three JSON lines (float, int8, difference), each naming net_arch 'sb3'; the saved int8 model loads as
    one"""
    from balance_robot_mujoco_rl_amd import QuantActorModel
    path, saved = str(tmp_path / "actor256.npy"), str(tmp_path / "actor256_int8.npz")
    np.save(path, A.sac_vector(A.pd_actor_params(), log_ent_coef=-1.0))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_quant_policy.py"), "--env", "Env01-v1", "--envs", "256", "--steps", "200",
                        "--actor", path, "--algo", "sac", "--save", saved], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 3 and all(line["net_arch"] == "sb3" and line["envs"] == 256 for line in lines)
    assert [line["network"] for line in lines] == ["float (DeviceSACNets, deterministic)", "int8 (QuantActor)", "int8 - float"]
    assert lines[0]["mean_reward_per_step"] is not None and lines[1]["mean_reward_per_step"] is not None
    assert QuantActorModel.load(saved).net_arch == "sb3"
