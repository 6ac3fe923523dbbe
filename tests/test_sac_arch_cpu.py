"""SAC at SB3's default widths [256, 256] (BRS_ARCH_SAC_DEFAULT) without a GPU: the host build of the kernel source for
that architecture (tests/sacarchhost) against the fp64 restatement and the cases of tests/sac_arch_cases.py (ref_sac.py and sac_cases.py
at these widths, every condition and gate theirs); the six-step chain; the same host code as a program under the sanitizers; the new
create calls and the refused DDPG / TD3 calls of the C ABI; flatten / unflatten for both architectures and both namings; the int8
quantiser's refusal.

Largest distances reached here by the host build, next to each gate (fp32 torch on the same case in brackets):
  act / target outputs, gate 1e-5: log_std 8.5e-6 (spread: the output layer's rows are x 60 and cancel), a' 5.1e-6, action 2.8e-6,
    z 2.8e-6, Q0(s', a') 2.7e-6, y 1.9e-6, mu 1.7e-6, logp' 1.6e-6
  actor gradient blocks, gate 1e-5: init 2.6e-7 [fp32 torch 2.8e-7], x3 8.8e-7 [3.9e-3], spread 5.6e-6 [4.4e-1]; statistics 7.5e-7.
    fp32 torch misses the gate on x3 and spread by the way SB3 writes the loss (tests/test_sac_cpu.py says why)
  twin critic gradient blocks, gate 1e-5: 2.9e-6
  six chained steps: every block at 1.0x fp32 torch's floored distance (gate 4x)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ref_sac as S0
import sac_arch_cases as A
import sac_cases as SC0
from balance_robot_mujoco_rl_amd import _lib, offpolicy, quant
from offpolicy_cases import GAMMA, GXX, ROOT, SEED, gate

SC, S = A.C, A.S
NA, NC = A.NA, A.NC
ERR_ARG, ERR_HIP = -1, -2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return A.build_host(tmp_path_factory.mktemp("sacarchhost"))


# --------------------------------------------------------------------------------------- 1. cases, act, target
def test_the_second_instance_has_its_own_widths_and_leaves_the_first_alone(host):
    na, nc = C.c_int(), C.c_int()
    assert host.sh_sizes(C.byref(na), C.byref(nc)) == 0 and (na.value, nc.value) == (NA, NC) == (68612, 68353) and host.sh_arch() == 1
    assert (S.NACTOR, S.NCRITIC, SC.NA, SC.NC) == (NA, NC, NA, NC) and (S0.NACTOR, SC0.NC) == (63104, 32101)
    actor, critics = SC.weights("init")
    assert actor.shape == (NA + 1,) and critics.shape == (2 * NC,) and SC0.weights("init")[0].shape == (63105,)
    assert all(SC.MARGIN[k] == v for k, v in SC0.MARGIN.items()) and SC.AMP == SC0.AMP and SC.GRAD_GATE == SC0.GRAD_GATE and SC._CASES is not SC0._CASES


def test_conditioning_converges_and_the_cases_cover_every_branch():
    """sac_cases' conditions, under its round limits, on the [256, 256] weight sets; `spread` with the factors of sac_arch_cases"""
    tables = SC.assert_branch_coverage()
    assert tables[("gradient", 33)]["log_std_low"] >= 1 and tables[("target", 257)]["saturated"] >= 8
    for kind in SC.WEIGHT_SETS:
        c = SC.grad_case(257, kind)
        assert c["obs"].shape == (257, 6) and np.abs(c["q"][:, 0] - c["q"][:, 1]).min() >= SC.MARGIN[kind]
        assert min(np.abs(c["raw"] - S.LOG_STD_MIN).min(), np.abs(c["raw"] - S.LOG_STD_MAX).min()) >= SC.MARGIN[kind]
    raw = SC.grad_case(257, "spread")["raw"]
    assert raw.min() < -23 and raw.max() > 5   # three units and more past both clamps


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("n", SC.ACT_ROWS_CPU)
def test_host_act_against_fp64(host, n, kind):
    c = SC.act_case(n, kind)
    a, mu, ls, z = SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0)
    for x, ref, name in zip((a, mu, ls, z), c["act"], ("action", "mu", "log_std", "z")):
        gate(x, ref, f"n={n} {kind} {name}")
    assert np.abs(a).max() <= 1.0 and ls.min() >= S.LOG_STD_MIN and ls.max() <= S.LOG_STD_MAX
    assert SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0, extras=False)[0].tobytes() == a.tobytes()
    d0, mu0 = SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0, deterministic=True)[:2]
    assert d0.tobytes() == SC.host_act(host, c["actor"], c["obs"], SEED, 0, 5, deterministic=True)[0].tobytes() and mu0.tobytes() == mu.tobytes()
    gate(d0, c["act_det"][0], f"n={n} {kind} deterministic action")
    r, rmu, rls, rz = SC.host_act(host, None, None, SEED, 0, 0, random=True, n=n)
    assert np.array_equal(r.astype(np.float64), S.act(None, None, SEED, 0, 0, random=True, n=n)[0]) and not rls.any() and rz.tobytes() == z.tobytes()
    assert SC.host_act(host, c["actor"], c["obs"], SEED, 0, 1)[3].tobytes() != z.tobytes()   # another step, another z


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("m", SC.ACT_ROWS_CPU)
def test_host_target_against_fp64(host, m, kind):
    c = SC.target_case(m, kind)
    y, a, lp, z = SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 0)
    for x, name in ((z, "z"), (a, "a"), (lp, "logp"), (y, "y")):
        gate(x, c[name], f"m={m} {kind} {name}")
    ended = c["done"] != 0
    assert y[ended].tobytes() == c["reward"][ended].tobytes() and np.abs(a).max() <= 1.0
    assert SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 0, extras=False)[0].tobytes() == y.tobytes()
    assert SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 1)[3].tobytes() != z.tobytes()
    q = A.host_q(host, c["critics"][:NC], c["next_obs"], a)
    gate(q, S.R.critic(c["critics"][:NC], c["next_obs"], a.astype(np.float64)), f"m={m} {kind} Q0(s', a')")


# --------------------------------------------------------------------------------------- 2. gradients
@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("n", SC.GRAD_ROWS_CPU)
def test_host_actor_gradient_against_fp64(host, n, kind):
    c = SC.grad_case(n, kind)
    g64, g32 = SC.references(n, kind)
    g = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, c["draw"])
    assert g.shape == (NA + 1 + 4,)
    SC.check_actor_gradient(f"n={n} {kind}", g, g64, g32, gate)
    assert abs(g[NA + 4] - np.exp(np.float64(c["actor"][NA]))) <= 1e-6


@pytest.mark.parametrize("kind", ("init", "x3"))
@pytest.mark.parametrize("n", SC.GRAD_ROWS_CPU)
def test_host_twin_critic_gradient_against_fp64(host, n, kind):
    """SB3's critic loss 0.5 (mse(Q1, y) + mse(Q2, y)) per block of each critic; the rows are those of the gradient case, whose
    conditions cover both critics' hidden layers on (obs, a(obs)); on the buffer's (obs, act) the margin is asserted here"""
    c = SC.grad_case(n, kind)
    for k in (0, 1):
        assert np.abs(A._critic_pre(c["critics"][k * NC:(k + 1) * NC], c["obs"], c["act"])).min() > 0
    g = SC.host_twin_critic_grad(host, c["critics"], c["obs"], c["act"], c["y"])
    g64 = S.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"])
    for k in (0, 1):
        d = SC.block_distances(g[k * NC:(k + 1) * NC], g64[k * NC:(k + 1) * NC], A.CRITIC_SIZES)
        print(f"n={n} {kind} critic {k}: largest block distance from fp64 {max(d.values()):.3g}")
        assert max(d.values()) <= SC.GRAD_GATE, d
    gate(g[2 * NC:], g64[2 * NC:], "statistics")


def test_fixed_temperature_gets_a_zero_gradient(host):
    c = SC.grad_case(33, "init")
    g = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, 0, learn_alpha=False)
    learned = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, 0, learn_alpha=True)
    assert g[NA] == 0.0 and learned[NA] != 0.0 and np.delete(g, NA).tobytes() == np.delete(learned, NA).tobytes()


@pytest.mark.parametrize("layer,unit", ((1, 255), (1, 0), (2, 255), (2, 0)))
def test_width_edge_models_on_the_host_build(host, layer, unit):
    """the layer after hidden layer `layer` reads only `unit` of it, with a large weight: 255 is the last unit of the last tile"""
    actor, critics = A.edge_model(layer, unit)
    c = SC.grad_case(33, "init")
    a, mu, ls, z = SC.host_act(host, actor, c["obs"], SEED, 0, 0)
    ref = S.act(actor, c["obs"], SEED, 0, 0)
    gate(mu, ref[1], f"layer {layer} unit {unit} mu"); gate(ls, ref[2], "log_std")
    g = SC.host_twin_critic_grad(host, critics, c["obs"], c["act"], c["y"])
    g64 = S.twin_critic_grad(critics, c["obs"], c["act"], c["y"])
    d = SC.block_distances(g[:NC], g64[:NC], A.CRITIC_SIZES)
    print(f"layer {layer} unit {unit}: critic block distances {d}")
    assert max(d.values()) <= SC.GRAD_GATE
    name = {1: "W2", 2: "W3"}[layer]
    sl = S.RL.block_slices(A.CRITIC_SIZES)[name]
    w64 = g64[sl].reshape(A.CRITIC_SIZES[layer + 1], 256)
    assert np.abs(w64[:, unit]).max() > 0   # the column that is read carries the gradient the block is judged on


# --------------------------------------------------------------------------------------- 3. the chain
def test_six_chained_steps_against_the_fp64_chain(host):
    case = SC.chain_case(A.CHAIN_KIND)
    h = SC.HostSAC(host, case["actor"], case["critics"], **SC.SAC_ADAM)
    for s in range(SC.CHAIN_STEPS):
        sl = slice(s * SC.CHAIN_ROWS, (s + 1) * SC.CHAIN_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        before = h.flat["actor"][NA]
        h.step(obs, act, h.target(no, rew, done, GAMMA, SEED, s), SEED, s)
        assert h.flat["actor"][NA] != before   # the temperature moves in every step
    worst = SC.check_chain("host chain", h.flat, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| after six chained steps = {worst:.3g}")


# --------------------------------------------------------------------------------------- 4. the same code under the sanitizers
def test_stand_alone_program_is_clean_under_asan_and_ubsan(tmp_path):
    """sacarchhost_main.cpp has its own main: nothing sanitized is loaded into Python.  act -> target -> both gradients -> apply at
    m = 33, two steps; both builds print the same digests"""
    out = {}
    for name, flags in (("plain", []), ("san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(tmp_path / f"sacarchhost_{name}")
        subprocess.check_call(GXX + flags + ["-o", exe, os.path.join(A.HOST_DIR, "sacarchhost_main.cpp")])
        r = subprocess.run([exe, "33", "2"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (name, r.returncode, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["plain"] == out["san"] and out["plain"].startswith("arch=1 m=33 steps=2 actor=")


# --------------------------------------------------------------------------------------- 5. C ABI without a device
def test_symbols_sizes_and_table():
    L = _lib.lib()
    for name in ("brs_ddpg_create_arch", "brs_ddpg_learner_create_sac_arch"):
        assert hasattr(L, name) and name in _lib.SIGNATURES["brs_policy.h"] and name in _lib.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "brs_policy.h")).read()
    assert "#define BRS_ARCH_REFERENCE 0" in hdr and "#define BRS_ARCH_SAC_DEFAULT 1" in hdr
    assert (_lib.ARCH_REFERENCE, _lib.ARCH_SAC_DEFAULT) == (0, 1) and (_lib.SAC256_NACTOR, _lib.SAC256_NCRITIC) == (68612, 68353)
    assert "#define BRS_SAC256_NACTOR (256 * 6 + 256 + 256 * 256 + 256 + 4 * 256 + 4)" in hdr
    assert "#define BRS_SAC256_NCRITIC (256 * 8 + 256 + 256 * 256 + 256 + 1 * 256 + 1)" in hdr
    a = offpolicy.SAC_ARCHS
    assert (a["reference"].id, a["reference"].nactor, a["reference"].ncritic) == (0, 63104, 32101)
    assert (a["sb3"].id, a["sb3"].nactor, a["sb3"].ncritic, a["sb3"].grad_len) == (1, NA, NC, NA + 5)
    for bad in ("td3", (400, 300)):
        with pytest.raises(ValueError, match="net_arch must be 'reference' or 'sb3'"):
            offpolicy.sac_arch(bad)


def test_create_argument_errors_and_refused_calls_without_a_device(host):
    L = _lib.lib()
    err, lerr = (lambda: L.brs_ddpg_last_error(None)), (lambda: L.brs_ddpg_learner_last_error(None))
    h = C.c_void_p(1)
    assert L.brs_ddpg_create_arch(0, 1, None) == ERR_ARG and err() == b"brs_ddpg_create_arch: null argument"
    for bad in (-1, 2, 7):
        assert L.brs_ddpg_create_arch(0, bad, C.byref(h)) == ERR_ARG and h.value is None and err() == b"brs_ddpg_create_arch: unknown architecture"
        h = C.c_void_p(1)
        assert L.brs_ddpg_learner_create_sac_arch(0, 256, bad, C.byref(h)) == ERR_ARG and h.value is None
        assert lerr() == b"brs_ddpg_learner_create_sac_arch: unknown architecture"
        assert host.sh_known_arch(bad) == 0
    assert host.sh_known_arch(0) == 1 and host.sh_known_arch(1) == 1
    assert L.brs_ddpg_learner_create_sac_arch(0, 256, 1, None) == ERR_ARG and lerr() == b"brs_ddpg_learner_create_sac_arch: null argument"
    for bad in (0, (1 << 22) + 1):
        assert L.brs_ddpg_learner_create_sac_arch(0, bad, 1, C.byref(h)) == ERR_ARG and lerr() == b"brs_ddpg_learner_create_sac_arch: max_batch must be in [1, 2^22]"
    # the calls an arch-1 handle refuses check their arguments first, as before: a NULL handle is told apart from a wrong one
    buf = C.c_void_p(64)
    assert L.brs_ddpg_act(None, buf, 4, buf, 11, 0, 0, 0.1, 0, buf, None, None, None) == ERR_ARG and err() == b"brs_ddpg_act: null handle"
    assert L.brs_ddpg_td_target(None, buf, buf, 4, buf, buf, buf, 0.99, buf, None) == ERR_ARG and err() == b"brs_ddpg_td_target: null handle"
    assert L.brs_td3_td_target(None, buf, buf, 4, buf, buf, buf, 0.99, 0.2, 0.5, 11, 0, buf, None, None, None) == ERR_ARG
    assert err() == b"brs_td3_td_target: null handle"
    assert L.brs_ddpg_learner_critic_grad(None, buf, 4, buf, buf, buf, buf, None) == ERR_ARG and lerr() == b"brs_ddpg_learner_critic_grad: null handle"
    assert L.brs_ddpg_learner_twin_critic_grad(None, buf, 4, buf, buf, buf, buf, None) == ERR_ARG
    assert lerr() == b"brs_ddpg_learner_twin_critic_grad: null handle"
    assert L.brs_ddpg_learner_actor_grad(None, buf, buf, 4, buf, buf, None) == ERR_ARG and lerr() == b"brs_ddpg_learner_actor_grad: null handle"


def test_arch_one_fails_loudly_without_a_device():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is for machines without one")
    L = _lib.lib()
    h = C.c_void_p(1)
    assert L.brs_ddpg_learner_create_sac_arch(0, 256, 1, C.byref(h)) == ERR_HIP and h.value is None
    assert L.brs_ddpg_learner_last_error(None).startswith(b"brs_ddpg_learner_create_sac_arch: no HIP device (")
    assert L.brs_ddpg_create_arch(0, 1, C.byref(h)) == ERR_HIP and L.brs_ddpg_last_error(None).startswith(b"brs_ddpg_create_arch: no HIP device (")
    from balance_robot_mujoco_rl_amd import BrsError, DeviceSACLearner, DeviceSACNets
    with pytest.raises(BrsError, match="SAC learner has no CPU fallback"):
        DeviceSACLearner(net_arch="sb3")
    with pytest.raises(BrsError):
        DeviceSACNets(net_arch="sb3")


# --------------------------------------------------------------------------------------- 6. the Python layer
def _sb3_state_dict():
    """SAC("MlpPolicy", env).policy.state_dict()'s actor and critic tensors, filled so that every element names its place"""
    sd, at = {}, 0

    def fill(name, shape):
        nonlocal at
        k = int(np.prod(shape))
        sd[name] = torch.arange(at, at + k, dtype=torch.float32).reshape(shape)
        at += k
    for name, shape in (("actor.latent_pi.0.weight", (256, 6)), ("actor.latent_pi.0.bias", (256,)), ("actor.latent_pi.2.weight", (256, 256)),
                        ("actor.latent_pi.2.bias", (256,)), ("actor.mu.weight", (2, 256)), ("actor.log_std.weight", (2, 256)), ("actor.mu.bias", (2,)),
                        ("actor.log_std.bias", (2,))):
        fill(name, shape)
    sd["log_ent_coef"] = torch.tensor([-0.25])
    for net in ("critic", "critic_target"):
        for k in (0, 1):
            for i, (o, n) in zip((0, 2, 4), ((256, 8), (256, 256), (1, 256))):
                fill(f"{net}.qf{k}.{i}.weight", (o, n)); fill(f"{net}.qf{k}.{i}.bias", (o,))
    return sd


def test_a_hand_built_sb3_state_dict_lands_in_the_documented_flat_order():
    sd = _sb3_state_dict()
    flat = offpolicy.flatten_sac_actor(sd)
    # W1 b1 W2 b2, then W3[4][256] = mu's rows, log_std's rows, then b3[4] = mu's bias, log_std's bias, then log_ent_coef: filled in
    # exactly that order, so the vector counts up
    assert flat.shape == (NA + 1,) and np.array_equal(flat[:NA], np.arange(NA, dtype=np.float32)) and flat[NA] == np.float32(-0.25)
    for net in ("critic", "critic_target"):
        c = offpolicy.flatten_td3_critics(sd, net)
        start = NA + (0 if net == "critic" else 2 * NC)
        assert c.shape == (2 * NC,) and np.array_equal(c, np.arange(start, start + 2 * NC, dtype=np.float32))


@pytest.mark.parametrize("arch", ("reference", "sb3"))
@pytest.mark.parametrize("naming", ("sb3", "tool"))
def test_flatten_round_trip_for_both_archs_and_namings(arch, naming):
    actor, critics = (SC0 if arch == "reference" else SC).weights("spread")
    h1, h2 = (300, 200) if arch == "reference" else (256, 256)
    sd = offpolicy.unflatten_sac_actor(actor, naming)
    first = {"sb3": "actor.latent_pi.0.weight", "tool": "actor.body.0.weight"}[naming]
    assert len(sd) == 9 and sd[first].shape == (h1, 6) and sd["actor.log_std.weight"].shape == (2, h2) and float(sd["log_ent_coef"][0]) == actor[-1]
    assert offpolicy.flatten_sac_actor(sd).tobytes() == actor.tobytes()
    cd = offpolicy.unflatten_td3_critics(critics, "critic", naming)
    q = {"sb3": "critic.qf1.2.weight", "tool": "critic.1.2.weight"}[naming]
    assert len(cd) == 12 and cd[q].shape == ((150, 200) if arch == "reference" else (256, 256))
    assert offpolicy.flatten_td3_critics(cd, "critic").tobytes() == critics.tobytes()


def test_shapes_of_neither_architecture_are_named():
    sd = offpolicy.unflatten_sac_actor(SC.weights("init")[0], "sb3")
    with pytest.raises(ValueError, match=r"actor\.latent_pi\.2\.weight: expected shape \(200, 300\) or \(256, 256\), got \(400, 300\)"):
        offpolicy.flatten_sac_actor({**sd, "actor.latent_pi.2.weight": torch.zeros(400, 300)})
    with pytest.raises(ValueError, match=r"actor\.latent_pi\.0\.weight: shape \(256, 6\) mixes"):   # each tensor fits one of the two, not the same one
        offpolicy.flatten_sac_actor({**sd, "actor.mu.weight": torch.zeros(2, 200)})
    cd = offpolicy.unflatten_td3_critics(SC.weights("init")[1], "critic", "sb3")
    with pytest.raises(ValueError, match=r"critic\.qf1\.0\.weight: expected shape \(200, 8\) or \(256, 8\), got \(400, 8\)"):
        offpolicy.flatten_td3_critics({**cd, "critic.qf1.0.weight": torch.zeros(400, 8)})
    with pytest.raises(ValueError, match="critic.qf0.4.bias: missing"):
        offpolicy.flatten_td3_critics({k: v for k, v in cd.items() if k != "critic.qf0.4.bias"})
    with pytest.raises(ValueError, match="expected 63105 or 68613 elements"):
        offpolicy.unflatten_sac_actor(np.zeros(70000, np.float32))
    with pytest.raises(ValueError, match="expected 64202 or 136706 parameters"):
        offpolicy.unflatten_td3_critics(np.zeros(NC, np.float32))


def test_quantize_actor_refuses_a_256_wide_actor():
    actor = SC.weights("init")[0]
    for params in (actor, actor[:NA], offpolicy.unflatten_sac_actor(actor, "sb3")):
        with pytest.raises(ValueError, match=r"\[256, 256\] SAC actor .* reference widths pi=\[300, 200\]"):
            quant.quantize_actor(params, head="sac")
    quant.quantize_actor(SC0.weights("init")[0], head="sac")   # the reference widths are served as before
