"""SAC on the device (include/brs_policy.h: brs_sac_act, brs_sac_td_target, brs_ddpg_learner_create_sac,
brs_sac_twin_critic_grad, brs_sac_actor_grad): the HIP kernels against the fp64 restatement (tests/ref_sac.py), fp32 torch on the same
inputs and the host build of the same source (tests/sachost), on the cases of tests/sac_cases.py at the kernels' own tile edges.  Every
output sits between guard zones that must stay untouched, the handle's scratch is filled with NaN before a call, and the critic
gradient must be 0.5 x the TD3 call's result byte for byte.

Largest distances reached on an MI355X, next to each gate (fp32 torch on the same case in brackets):
  act / target outputs against fp64, gate 1e-5: log_std 8.6e-6 (spread: the output layer's rows are x 60 and cancel), a' 5.0e-6, mu 4.1e-6,
    logp' 3.9e-6, action 3.7e-6, y 3.3e-6, z 2.8e-6; against the host build: log_std 5.7e-6, logp' 4.1e-6, mu 3.1e-6, y 2.5e-6, z 2.2e-7
  actor gradient blocks against fp64, gate 1e-5: init 2.5e-7 [fp32 torch 4.5e-7], x3 3.9e-6 [2.0e-2], spread 3.8e-6 [7.6e-2]; against the
    host build 3.4e-6; statistics 7.9e-7 (gate 1e-5).  fp32 torch misses the gate on x3 and spread by the way SB3 writes the loss (see
    tests/test_sac_cpu.py); the kernels meet it on the same cases
  critic gradient against fp64: 9.5e-7; six chained steps: every block at 1.0x fp32 torch's floored distance (gate 4x).

The sample split (ddpg_learner_cases.SPLIT_TABLE; the allocation's arithmetic is asserted first, launching nothing: 1,544 scratch rows
and 8.0000 partial rows of 64,206 floats on a SAC handle, exactly a TD3 twin handle's).  Largest block distance from fp64 per row, on
a fresh handle of max_batch == m and on the NaN-filled one of 8,448 rows (identical bytes), gate 1e-5:
  actor gradient, init: 385 1.2e-7, 513 1.6e-7, 769 1.4e-7, 1,025 1.1e-7, 2,049 9.3e-8, 8,192 1.1e-7, 8,193 1.3e-7 [fp32 torch up to
    8.3e-7]; x3: 513 3.9e-7, 2,049 3.3e-7, 8,193 1.5e-7 [1.7e-3]; spread: 769 1.3e-6, 2,049 6.8e-7 [5.6e-2]; against the host build
    (every row: sac_cases.HOST_ROWS_MAX) 2.1e-6 (769 spread), init and x3 at most 2.6e-7; statistics 1.4e-7
  critic gradient, 0.5 x the TD3 call byte for byte on the SAC handle, against fp64: init 1.1e-7 (385), 1.5e-7 (513), 1.4e-7 (769),
    1.1e-7 (1,025), 8.5e-8 (2,049), 1.1e-7 (8,192), 1.3e-7 (8,193); x3 3.4e-7 (513), 1.4e-7 (2,049), 1.4e-7 (8,193)
  the five tail sums / the twin call's four statistics under `gate`: 769 rows 1.4e-8 / 6.9e-9, 8,193 rows 8.9e-8 / 8.0e-9; with row 768
    of 769 replaced (the sums move by 1.8e-4 to 1.2e-3, the twin statistics by 1.8e-4 to 1.0e-2) 6.3e-8 / 1.4e-8."""
import os
import sys

import numpy as np
import pytest

import ref_offpolicy as R
import ref_sac as S
import sac_cases as SC
import td3_cases as TC
from ddpg_learner_cases import GRAD_GATE, SPLIT_CASES, block_distances
from offpolicy_cases import GAMMA, ROOT, SEED, gate
from test_ddpg_learner_gpu import _poison
from test_offpolicy_gpu import Guarded, _cuda

pytestmark = pytest.mark.gpu
NA, NC = SC.NA, SC.NC
GLEN, TLEN = NA + 1 + S.NSTAT, 2 * NC + 4
UNTOUCHED = np.float32(-3.25)   # Guarded's float32 sentinel


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return SC.build_host(tmp_path_factory.mktemp("sachost"))


@pytest.fixture(scope="module")
def nets():
    from balance_robot_mujoco_rl_amd import DeviceSACNets
    d = DeviceSACNets(device=0, seed=SEED)
    yield d
    d.close()


def _sac(max_batch, **kw):
    from balance_robot_mujoco_rl_amd import DeviceSACLearner
    return DeviceSACLearner(device=0, max_batch=max_batch, seed=SEED, **{**SC.SAC_ADAM, "target_entropy": SC.TARGET_ENTROPY, **kw})


@pytest.fixture(scope="module")
def big():
    lrn = _sac(1024)
    yield lrn
    lrn.close()


# --------------------------------------------------------------------------------------- 0. the allocation, launching nothing
def _assert_partial_rows_fit():
    rows, _ = SC.assert_partial_rows_fit(_sac, max(NA + SC.SAC_TAIL, TLEN), "SAC handle")
    assert rows >= 2 * 544 + 4 + 1 + S.NSTAT   # the actor's image (test_existing_calls_return_the_same_bytes_on_a_sac_handle)


def test_eight_partial_rows_fit_the_allocation():
    """first in the file: the arithmetic of the handle's one allocation is known before any launch with eight workgroup rows.  A
    TD3 twin handle is the control: its sizes are known exactly (tests/test_td3_gpu.py runs it at every split geometry)"""
    from balance_robot_mujoco_rl_amd import DeviceTD3Learner
    from ddpg_learner_cases import ADAM
    assert SC.SPLIT_TABLE[8193][2] == SC.SPLIT_TABLE[8192][2] == SC.MAX_SPLIT
    twin = SC.assert_partial_rows_fit(lambda mb: DeviceTD3Learner(device=0, max_batch=mb, **ADAM), max(TLEN, R.NACTOR + 2), "TD3 twin handle")
    assert twin == (2 * 772, SC.MAX_SPLIT * TLEN)
    _assert_partial_rows_fit()


# --------------------------------------------------------------------------------------- 1. act
def _act(nets, actor, obs, step, extras=True, **kw):
    import torch
    n = len(obs)
    a, mu, ls, z = (Guarded((n, 2)) for _ in range(4))
    nets.act(actor, obs, step, out=a.t, mean=mu.t if extras else None, log_std=ls.t if extras else None, noise=z.t if extras else None, **kw)
    torch.cuda.synchronize()
    assert all(x.intact() for x in (a, mu, ls, z)), "the kernel wrote outside its outputs"
    return a.np(), mu.np(), ls.np(), z.np()


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("n", SC.ACT_ROWS_GPU)
def test_act_against_fp64_and_the_host_build(nets, host, n, kind):
    c = SC.act_case(n, kind)
    actor, obs = _cuda(c["actor"]), _cuda(c["obs"])
    out = _act(nets, actor, obs, 0)
    hout = SC.host_act(host, c["actor"], c["obs"], SEED, 0, 0)
    for x, ref, h, name in zip(out, c["act"], hout, ("action", "mu", "log_std", "z")):
        gate(x, ref, f"n={n} {kind} {name}"); gate(x, h, f"n={n} {kind} {name} against the host build")
    assert np.abs(out[0]).max() <= 1.0
    bare = _act(nets, actor, obs, 0, extras=False)
    assert bare[0].tobytes() == out[0].tobytes() and all((x == UNTOUCHED).all() for x in bare[1:])   # NULL outputs: nothing written
    again, other = _act(nets, actor, obs, 0), _act(nets, actor, obs, 1)
    assert all(x.tobytes() == w.tobytes() for x, w in zip(out, again)) and other[3].tobytes() != out[3].tobytes()
    det = _act(nets, actor, obs, 0, deterministic=True)
    gate(det[0], c["act_det"][0], f"n={n} {kind} deterministic action")
    assert det[0].tobytes() == _act(nets, actor, obs, 7, deterministic=True)[0].tobytes() and det[1].tobytes() == out[1].tobytes()
    a = Guarded((n, 2))
    nets.act(None, None, 0, random=True, out=a.t)
    assert np.array_equal(a.np().astype(np.float64), S.act(None, None, SEED, 0, 0, random=True, n=n)[0]) and a.intact()


# --------------------------------------------------------------------------------------- 2. the target
def _target(nets, dev, draw, extras=True):
    import torch
    m = len(dev["next_obs"])
    y, a, lp, z = Guarded((m,)), Guarded((m, 2)), Guarded((m,)), Guarded((m, 2))
    nets.sac_target(dev["actor"], dev["critics"], dev["next_obs"], dev["reward"], dev["done"], GAMMA, draw, out=y.t, next_action=a.t if extras else None,
                    logp=lp.t if extras else None, noise=z.t if extras else None)
    torch.cuda.synchronize()
    assert all(x.intact() for x in (y, a, lp, z)), "the kernel wrote outside its outputs"
    return y.np(), a.np(), lp.np(), z.np()


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("m", SC.GPU_ROWS)
def test_target_against_fp64_and_the_host_build(nets, host, m, kind):
    SC.assert_branch_coverage()   # a condition on the inputs, on the fp64 reference, before anything is compared
    c = SC.target_case(m, kind)
    dev = {k: _cuda(c[k]) for k in ("actor", "critics", "next_obs", "reward", "done")}
    y, a, lp, z = _target(nets, dev, 0)
    hy, ha, hlp, hz = SC.host_target(host, c["actor"], c["critics"], c["next_obs"], c["reward"], c["done"], GAMMA, SEED, 0)
    for x, name, h in ((z, "z", hz), (a, "a", ha), (lp, "logp", hlp), (y, "y", hy)):
        gate(x, c[name], f"m={m} {kind} {name}"); gate(x, h, f"m={m} {kind} {name} against the host build")
    ended = c["done"] != 0
    assert y[ended].tobytes() == c["reward"][ended].tobytes() and np.abs(a).max() <= 1.0
    bare = _target(nets, dev, 0, extras=False)
    assert bare[0].tobytes() == y.tobytes() and all((x == UNTOUCHED).all() for x in bare[1:])
    again, other = _target(nets, dev, 0), _target(nets, dev, 1)
    assert all(x.tobytes() == w.tobytes() for x, w in zip((y, a, lp, z), again))
    assert other[3].tobytes() != z.tobytes() and (m == 1 or other[0].tobytes() != y.tobytes())


# --------------------------------------------------------------------------------------- 3. the critic gradient
@pytest.fixture(scope="module")
def wide():
    """max_batch = 8,448: ld != mp at every row of ddpg_learner_cases.SPLIT_ROWS; the allocation's arithmetic is asserted first"""
    _assert_partial_rows_fit()
    lrn = _sac(SC.SPLIT_BIG)
    yield lrn
    lrn.close()


@pytest.mark.parametrize("n", (1, 33, 129, 1000))
def test_critic_gradient_is_half_the_td3_call_byte_for_byte(big, n):
    _check_half_the_td3_call(big, n, "x3")


@pytest.mark.parametrize("n,kind", SPLIT_CASES)
def test_critic_gradient_is_half_the_td3_call_at_every_split_geometry(wide, n, kind):
    """the same identity at the rows of ddpg_learner_cases.SPLIT_ROWS on the NaN-filled SAC handle of 8,448, whose partial rows are
    sized for the SAC actor's row, not the twin one (the TD3 side is held to fp64 at these rows by tests/test_td3_gpu.py)"""
    _check_half_the_td3_call(wide, n, kind)


def _check_half_the_td3_call(big, n, kind):
    import torch
    c = TC.twin_case(n, kind)
    dev = {k: _cuda(c[k]) for k in ("obs", "act", "y", "critics")}
    _poison(big)
    td3, sac = Guarded((2 * NC + 4,)), Guarded((2 * NC + 4,))
    assert big.L.brs_ddpg_learner_twin_critic_grad(big.h, dev["critics"].data_ptr(), n, dev["obs"].data_ptr(), dev["act"].data_ptr(), dev["y"].data_ptr(),
                                                   td3.t.data_ptr(), None) == 0
    big.twin_critic_grad(dev["critics"], dev["obs"], dev["act"], dev["y"], out=sac.t)
    torch.cuda.synchronize()
    t, s = td3.np(), sac.np()
    assert td3.intact() and sac.intact() and np.isfinite(t).all() and np.isfinite(s).all()
    halved = np.concatenate([np.arange(2 * NC), [2 * NC, 2 * NC + 2]])
    sel = halved[np.abs(t[halved]) >= 2.0 ** -125]
    assert (np.float32(0.5) * t[sel]).tobytes() == s[sel].tobytes() and len(sel) > 1000
    assert t[[2 * NC + 1, 2 * NC + 3]].tobytes() == s[[2 * NC + 1, 2 * NC + 3]].tobytes()
    g64 = S.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"])
    for k in (0, 1):
        d = block_distances(s[k * NC:(k + 1) * NC], g64[k * NC:(k + 1) * NC], R.CRITIC_SIZES)
        print(f"n={n} critic {k}: largest block distance from fp64 {max(d.values()):.3g}")
        assert max(d.values()) <= GRAD_GATE
    gate(s[2 * NC:], g64[2 * NC:], "statistics")


# --------------------------------------------------------------------------------------- 4. the actor gradient
def _actor_grad(lrn, dev, draw=0):
    g = Guarded((GLEN,))
    lrn.actor_grad(dev["actor"], dev["critics"], dev["obs"], draw, out=g.t)
    out = g.np()
    assert g.intact(), "a kernel wrote outside the gradient buffer"
    return out


def _dev(c):
    return {k: _cuda(c[k]) for k in ("obs", "actor", "critics")}


def _check_actor_gradient(host, big, n, kind, with_host=True):
    c = SC.grad_case(n, kind)
    g64, g32 = SC.references(n, kind)
    dev = _dev(c)
    own = _sac(n)                           # max_batch == m, fresh
    g = _actor_grad(own, dev)
    own.close()
    _poison(big)                            # a larger max_batch, every word of its allocation NaN
    g_big = _actor_grad(big, dev)
    assert np.isfinite(g).all() and g.tobytes() == g_big.tobytes()   # nothing stale read, the handle's size does not matter
    SC.check_actor_gradient(f"n={n} {kind}", g, g64, g32, gate)
    if with_host:
        hg = SC.host_actor_grad(host, c["actor"], c["critics"], c["obs"], SEED, 0)
        d = SC.actor_block_distances(g, hg)
        print(f"n={n} {kind}: largest block distance from the host build {max(d.values()):.3g}")
        assert max(d.values()) <= GRAD_GATE
        gate(g[NA + 1:], hg[NA + 1:], "statistics against the host build")


@pytest.mark.parametrize("kind", SC.WEIGHT_SETS)
@pytest.mark.parametrize("n", SC.GPU_ROWS)
def test_actor_gradient_against_fp64_fp32_torch_and_the_host_build(host, big, n, kind):
    _check_actor_gradient(host, big, n, kind)


@pytest.mark.parametrize("n,kind", SC.SPLIT_ACTOR_CASES)
def test_actor_gradient_at_every_split_geometry(host, wide, n, kind):
    """the assertions of test_actor_gradient_against_fp64_fp32_torch_and_the_host_build at the rows of ddpg_learner_cases.SPLIT_ROWS
    (`init` at all seven, `x3` at 513, 2,049 and 8,193, `spread` at 769 and 2,049): two to eight partial rows of 63,104 + 5 floats
    behind the two-launch chain, whose padded rows must add exact zeros; a fresh handle of max_batch == m against the NaN-filled one of
    8,448, byte for byte; the host build up to sac_cases.HOST_ROWS_MAX"""
    _check_actor_gradient(host, wide, n, kind, with_host=n <= SC.HOST_ROWS_MAX)


def _twin(lrn, dev):
    import torch
    g = Guarded((TLEN,))
    lrn.twin_critic_grad(dev["critics"], dev["obs"], dev["act"], dev["y"], out=g.t)
    torch.cuda.synchronize()
    assert g.intact(), "a kernel wrote outside the gradient buffer"
    return g.np()


def _full_dev(c):
    return {k: _cuda(c[k]) for k in ("obs", "act", "y", "actor", "critics")}


def _fresh(n, call, dev):
    own = _sac(n)
    g = call(own, dev)
    own.close()
    return g


def test_no_leftover_between_split_geometries_and_calls_on_one_handle(wide):
    """8,193 -> 513 -> 33 -> 2,049 -> 769 rows on the NaN-filled handle of 8,448 (8 partial rows, then 2, none, 6 and 3), at each m the
    twin critic gradient and then the actor gradient, whose partial rows lie at different strides in the same storage: every result
    is what a fresh handle of exactly that size returns, byte for byte; the sequence a second time returns the same bytes; another
    draw at 2,049 rows changes the actor gradient"""
    devs = {n: _full_dev(SC.grad_case(n, "init")) for n in SC.SPLIT_SEQUENCE}
    fresh = {n: (_fresh(n, _twin, devs[n]), _fresh(n, _actor_grad, devs[n])) for n in SC.SPLIT_SEQUENCE}
    assert all(np.isfinite(t).all() and np.isfinite(a).all() for t, a in fresh.values())
    _poison(wide)
    for run in range(2):
        for n in SC.SPLIT_SEQUENCE:
            t = _twin(wide, devs[n])
            a = _actor_grad(wide, devs[n])
            assert t.tobytes() == fresh[n][0].tobytes(), (run, n, "twin critic gradient")
            assert a.tobytes() == fresh[n][1].tobytes(), (run, n, "actor gradient")
    other = _actor_grad(wide, devs[2049], draw=1)
    assert np.isfinite(other).all() and other[:NA].tobytes() != fresh[2049][1][:NA].tobytes()   # another draw, another sample


# --------------------------------------------------------------------------------------- 4b. the statistics at a split
@pytest.mark.parametrize("n", SC.SPLIT_STAT_ROWS)
def test_statistics_at_a_split(wide, n):
    """the five sums behind the actor's parameters and the twin call's four statistics against fp64, each under `gate`, at 769 rows
    (three splits, the last holds one real row) and 8,193 (eight, the last short)"""
    c = SC.grad_case(n, "init")
    dev = _full_dev(c)
    _poison(wide)
    a, t = _actor_grad(wide, dev), _twin(wide, dev)
    gate(a[NA:], SC.references(n, "init")[0][NA:], f"n={n} the actor call's five tail sums")
    gate(t[2 * NC:], SC.twin_reference(n, "init")[2 * NC:], f"n={n} the twin call's four statistics")


def test_statistics_see_the_lone_row_of_the_last_split(wide):
    """769 rows: row 768 is the one real row of the third split.  With that row alone replaced (sac_cases.changed_last_row: on the
    fp64 reference every row-dependent sum moves by more than 2 GATE) every such statistic of both calls changes, and is within
    `gate` of the changed case's fp64 reference; ent_coef, the same alpha / m from every row, keeps its bytes"""
    n = 769
    assert SC.SPLIT_LAST_REAL[n] == 1 and SC.SPLIT_TABLE[n][2] == 3
    c, (changed, b64, u64) = SC.grad_case(n, "init"), SC.changed_last_row(n, "init")
    a64, t64 = SC.references(n, "init")[0], SC.twin_reference(n, "init")
    rs = SC.ROW_SUMS
    assert SC.moved(b64[NA:NA + rs], a64[NA:NA + rs]).min() > 2 * SC.GATE and SC.moved(u64[2 * NC:], t64[2 * NC:]).min() > 2 * SC.GATE   # on the reference, first
    _poison(wide)
    a0, t0 = _actor_grad(wide, _full_dev(c)), _twin(wide, _full_dev(c))
    a1, t1 = _actor_grad(wide, _full_dev(changed)), _twin(wide, _full_dev(changed))
    print(f"n={n}: the replaced row moves the tail sums by {SC.moved(a1[NA:], a0[NA:])} and the twin statistics by {SC.moved(t1[2 * NC:], t0[2 * NC:])}")
    assert (a1[NA:NA + rs] != a0[NA:NA + rs]).all() and a1[NA + rs:].tobytes() == a0[NA + rs:].tobytes()
    assert (t1[2 * NC:] != t0[2 * NC:]).all()
    gate(a1[NA:], b64[NA:], f"n={n} the tail sums with row {n - 1} replaced")
    gate(t1[2 * NC:], u64[2 * NC:], f"n={n} the twin statistics with row {n - 1} replaced")


def test_no_leftover_scratch_between_sizes(big):
    """1,000 rows and then 33 on the same handle return what a fresh handle returns for the 33; two runs return identical bytes"""
    d1000, d33 = _dev(SC.grad_case(1000, "spread")), _dev(SC.grad_case(33, "spread"))
    _poison(big)
    first, second = _actor_grad(big, d1000), _actor_grad(big, d1000)
    assert first.tobytes() == second.tobytes()
    after = _actor_grad(big, d33)
    fresh_handle = _sac(33)
    fresh = _actor_grad(fresh_handle, d33)
    fresh_handle.close()
    assert after.tobytes() == fresh.tobytes()
    assert _actor_grad(big, d33, draw=1).tobytes() != after.tobytes()   # another draw, another sample


def test_fixed_temperature_on_the_device(big):
    import torch
    c = SC.grad_case(33, "init")
    dev = _dev(c)
    fixed = _sac(64, learn_alpha=False)
    g, learned = _actor_grad(fixed, dev), _actor_grad(big, dev)
    assert g[NA] == 0.0 and learned[NA] != 0.0 and np.delete(g, NA).tobytes() == np.delete(learned, NA).tobytes()
    actor = dev["actor"].clone()
    fixed.actor_grad(actor, dev["critics"], dev["obs"], 0)
    fixed.apply_actor(actor)
    torch.cuda.synchronize()
    after = actor.cpu().numpy()
    assert after[NA:].tobytes() == c["actor"][NA:].tobytes() and not np.array_equal(after[:NA], c["actor"][:NA])
    fixed.close()


# --------------------------------------------------------------------------------------- 5. handles
def test_sac_calls_need_a_sac_handle_and_respect_max_batch():
    import torch
    from balance_robot_mujoco_rl_amd import BrsError, DeviceDDPGLearner, DeviceTD3Learner, _lib
    from balance_robot_mujoco_rl_amd.policy import _p
    L = _lib.lib()
    z = lambda *s: torch.zeros(s, device="cuda")
    for other in (DeviceDDPGLearner(device=0, max_batch=64), DeviceTD3Learner(device=0, max_batch=64)):
        assert L.brs_sac_actor_grad(other.h, _p(z(NA + 1)), _p(z(2 * NC)), 8, _p(z(8, 6)), 11, 0, 1, -2.0, _p(z(GLEN)), None) == -1
        assert L.brs_ddpg_learner_last_error(other.h) == b"brs_sac_actor_grad: the handle was not created with brs_ddpg_learner_create_sac"
        assert L.brs_sac_twin_critic_grad(other.h, _p(z(2 * NC)), 8, _p(z(8, 6)), _p(z(8, 2)), _p(z(8)), _p(z(2 * NC + 4)), None) == -1
        assert L.brs_ddpg_learner_last_error(other.h) == b"brs_sac_twin_critic_grad: the handle was not created with brs_ddpg_learner_create_sac"
        other.close()
    sac = _sac(32)
    with pytest.raises(BrsError, match="brs_sac_actor_grad: m exceeds the handle's max_batch"):
        sac.actor_grad(z(NA + 1), z(2 * NC), z(33, 6), 0)
    with pytest.raises(BrsError, match="brs_sac_twin_critic_grad: m exceeds the handle's max_batch"):
        sac.twin_critic_grad(z(2 * NC), z(33, 6), z(33, 2), z(33))
    with pytest.raises(ValueError):
        sac.actor_grad(z(NA), z(2 * NC), z(8, 6), 0)
    sac.close()


def test_existing_calls_return_the_same_bytes_on_a_sac_handle():
    """critic_grad, twin_critic_grad, actor_grad and apply of DDPG / TD3 on a SAC handle against an ordinary and a twin one; their
    allocations keep their sizes"""
    import ctypes as C
    import torch
    from balance_robot_mujoco_rl_amd import DeviceDDPGLearner, DeviceTD3Learner, _lib
    from balance_robot_mujoco_rl_amd.policy import _p
    from ddpg_learner_cases import ADAM
    c = TC.twin_case(257, "x3")
    dev = {k: _cuda(c[k]) for k in ("obs", "act", "y", "actor", "critics")}
    plain, twin, sac = DeviceDDPGLearner(device=0, max_batch=257, **ADAM), DeviceTD3Learner(device=0, max_batch=257, **ADAM), _sac(257)
    ddpg_na = R.NACTOR
    assert plain.scratch()[1] == 4 * (1092 * 384 + 8 * (ddpg_na + 2)) and twin.scratch()[1] == 4 * (2 * 772 * 384 + 8 * (2 * NC + 4))
    assert sac.scratch()[1] >= 4 * ((2 * 544 + 4 + 1 + S.NSTAT) * 384 + 8 * max(GLEN, 2 * NC + 4))
    L, cfg = _lib.lib(), _lib.BrsAdamConfig(1e-3, 0.9, 0.999, 1e-8)
    results = []
    for lrn in (plain, twin, sac):
        gc, ga, gt = Guarded((NC + 2,)), Guarded((ddpg_na + 2,)), Guarded((2 * NC + 4,))
        assert L.brs_ddpg_learner_critic_grad(lrn.h, _p(dev["critics"]), 257, _p(dev["obs"]), _p(dev["act"]), _p(dev["y"]), _p(gc.t), None) == 0
        crit = gc.np()
        assert L.brs_ddpg_learner_actor_grad(lrn.h, _p(dev["actor"]), _p(dev["critics"]), 257, _p(dev["obs"]), _p(ga.t), None) == 0
        act = ga.np()
        rc = L.brs_ddpg_learner_twin_critic_grad(lrn.h, _p(dev["critics"]), 257, _p(dev["obs"]), _p(dev["act"]), _p(dev["y"]), _p(gt.t), None)
        assert rc == (-1 if lrn is plain else 0)
        tw = gt.np()
        p, m, v, tg = (Guarded((NC,), fill=f) for f in (0.25, 0.0, 0.0, 0.25))
        assert L.brs_ddpg_learner_apply(lrn.h, NC, _p(p.t), _p(gc.t), _p(m.t), _p(v.t), _p(tg.t), C.byref(cfg), 1, 0.005, None) == 0
        torch.cuda.synchronize()
        assert all(x.intact() for x in (gc, ga, gt, p, m, v, tg))
        results.append([crit, act, p.np(), m.np(), v.np(), tg.np(), tw])
    for k, (a, b, s) in enumerate(zip(*results)):
        assert b.tobytes() == s.tobytes() and np.isfinite(s).all(), f"result {k} differs between a twin and a SAC handle"
        if k < 6:   # the twin call is refused on the ordinary handle: its buffer stays untouched
            assert a.tobytes() == s.tobytes(), f"result {k} differs between an ordinary and a SAC handle"
    assert (results[0][6] == UNTOUCHED).all() and not np.array_equal(results[2][2], np.full(NC, 0.25, np.float32))
    plain.close(); twin.close(); sac.close()


# --------------------------------------------------------------------------------------- 6. whole steps
def test_six_chained_steps_with_the_temperature_moving(nets, host):
    """brs_sac_td_target from the current actor and the critics' target -> DeviceSACLearner.step, six times, on the kernels and on the
    host build, each against the same chain in fp64 by the trajectory rule"""
    case = SC.chain_case("init")
    h = SC.HostSAC(host, case["actor"], case["critics"], **SC.SAC_ADAM)
    lrn = _sac(SC.CHAIN_ROWS)
    flat = {k: _cuda(case[k.split("_")[0]]) for k in ("actor", "critics", "critics_target")}
    for s in range(SC.CHAIN_STEPS):
        sl = slice(s * SC.CHAIN_ROWS, (s + 1) * SC.CHAIN_ROWS)
        obs, act, no, rew, done = (np.ascontiguousarray(case[k][sl]) for k in ("obs", "act", "next_obs", "reward", "done"))
        before = {k: v.cpu().numpy() for k, v in flat.items()}
        y = nets.sac_target(flat["actor"], flat["critics_target"], _cuda(no), _cuda(rew), _cuda(done), GAMMA, s)
        lrn.step(flat, _cuda(obs), _cuda(act), y, s)
        h.step(obs, act, h.target(no, rew, done, GAMMA, SEED, s), SEED, s)
        after = {k: v.cpu().numpy() for k, v in flat.items()}
        assert all(after[k].tobytes() != before[k].tobytes() for k in flat) and after["actor"][NA] != before["actor"][NA]
    mine = {k: v.cpu().numpy() for k, v in flat.items()}
    worst_h = SC.check_chain("host chain", h.flat, case)
    worst = SC.check_chain("kernels", mine, case)
    print(f"largest |d - d64| / (floored) |d32torch - d64| after six chained steps: kernels {worst:.3g}, host build {worst_h:.3g}")
    s = lrn.stats()
    assert all(np.isfinite(v) for v in s.values()) and s["critic_loss"] > 0 and abs(s["ent_coef"] - float(np.exp(before["actor"][NA]))) < 1e-5
    assert (lrn.steps_critics, lrn.steps_actor) == (6, 6) and lrn.state_dict()["m_actor"].shape == (NA + 1,)
    lrn.close()


def test_tool_with_device_learner_end_to_end():
    """tools/train_sac_torch.py --envs 64 --steps 40 --batch 64 --device-data --device-learner: it trains, everything is finite, all
    vectors and log_ent_coef moved.  No learning-quality gate."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_sac_torch as T
    log = T.main(["--envs", "64", "--steps", "40", "--batch", "64", "--device-data", "--device-learner"])
    assert log["updates"] == 39   # 100 transitions are in after two steps of 64 envs
    assert log["finite"] and log["learner"] == "device" and log["data_path"] == "device"
    assert all(log["moved"][k] > 0 for k in ("actor", "critics", "critics_target", "log_ent_coef")), log["moved"]
    assert log["moved"]["critics_target"] < log["moved"]["critics"]
    assert np.isfinite(log["critic_loss_last"]) and log["critic_loss_last"] > 0 and np.isfinite(log["actor_loss_last"])
    assert np.isfinite(log["ent_coef"]) and log["ent_coef"] > 0 and log["ent_coef"] != 1.0
