"""SAC at SB3's default widths [256, 256] on the device (BRS_ARCH_SAC_DEFAULT): the [256, 256] instantiations of the HIP
kernels behind brs_sac_act, brs_sac_td_target, brs_ddpg_q, brs_sac_twin_critic_grad and brs_sac_actor_grad against the fp64
restatement, fp32 torch on the same inputs and the host build of the same source (tests/sacarchhost), on the cases of
tests/sac_arch_cases.py (sac_cases.py at these widths, every condition and gate its own) at the kernels' tile edges.  Every output sits
between guard zones that must stay untouched, the handle's scratch is filled with NaN before a call, and the DDPG / TD3 calls are
refused on such a handle.

Largest distances reached on an MI355X, next to each gate (fp32 torch on the same case in brackets):
  act / target outputs against fp64, gate 1e-5: log_std 8.6e-6 (spread: the output layer's rows are x 60 and cancel), a' 5.9e-6, y 4.5e-6,
    logp' 4.2e-6, action 3.1e-6, z 2.8e-6, mu 1.8e-6; against the host build: log_std 6.2e-6, logp' 3.4e-6, y 3.3e-6, a' 2.5e-6, mu 1.7e-6,
    z 2.2e-7; brs_ddpg_q on the [256, 256] critic 3.4e-6 (host build 2.8e-6)
  actor gradient blocks against fp64, gate 1e-5: init 2.5e-7 [fp32 torch 4.0e-7], x3 1.2e-6 [5.4e-3], spread 5.0e-6 [3.3e-1]; against the
    host build 1.6e-6; statistics 3.5e-7 (host build 8.1e-7)
  twin critic gradient blocks against fp64 3.4e-6, against the host build 2.8e-6
  the width-edge models (unit 255 / unit 0 alone behind either hidden layer): critic blocks 4.4e-7, actor blocks 3.8e-7
  six chained steps: every block at 1.0x fp32 torch's floored distance, kernels and host build (gate 4x).

The sample split (ddpg_learner_cases.SPLIT_TABLE; the allocation's arithmetic is asserted first, launching nothing: 2,056 scratch rows
and 8.0000 partial rows of 136,710 floats).  Largest block distance from fp64 per row, on a fresh handle of max_batch == m and on the
NaN-filled one of 8,448 rows (identical bytes), gate 1e-5:
  actor gradient, init: 385 1.3e-7, 513 1.5e-7, 769 1.4e-7, 1,025 1.1e-7, 2,049 9.0e-8, 8,192 1.1e-7, 8,193 1.2e-7 [fp32 torch up to
    9.9e-7]; x3: 513 2.7e-7, 2,049 1.1e-7, 8,193 1.5e-7 [2.2e-3]; spread: 769 6.5e-7, 2,049 2.5e-7 [6.4e-2]; against the host build (up
    to 2,049 rows: HOST_ROWS_MAX of sac_arch_cases) 4.0e-7; statistics 1.4e-7
  twin critic gradient, both critics, init: 385 1.2e-7, 513 1.5e-7, 769 1.4e-7, 1,025 1.1e-7, 2,049 8.5e-8, 8,192 1.2e-7, 8,193 1.3e-7;
    x3: 513 3.9e-7, 2,049 2.3e-7, 8,193 1.7e-7; against the host build 7.2e-7 (513 x3); statistics 1.2e-7
  the five tail sums / the twin call's four statistics under `gate`: 769 rows 3.5e-8 / 1.3e-8, 8,193 rows 6.6e-8 / 7.5e-9; with row 768
    of 769 replaced (the sums move by 9.7e-5 to 2.4e-4, the twin statistics by 2.3e-4 to 1.3e-2) 2.8e-8 / 2.2e-8."""
import os
import sys

import numpy as np
import pytest

import nonfinite_cases as NF
import sac_arch_cases as A
from offpolicy_cases import GAMMA, ROOT, SEED, gate
from test_ddpg_learner_gpu import _poison
from test_offpolicy_gpu import Guarded, _cuda

pytestmark = pytest.mark.gpu
SC, S = A.C, A.S
NA, NC = A.NA, A.NC
GLEN, TLEN = NA + 1 + S.NSTAT, 2 * NC + 4
GRAD_GATE = SC.GRAD_GATE
UNTOUCHED = np.float32(-3.25)   # Guarded's float32 sentinel
REFUSED = "the handle's architecture does not serve this call (DDPG and TD3 run at BRS_ARCH_REFERENCE only)"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return A.build_host(tmp_path_factory.mktemp("sacarchhost"))


@pytest.fixture(scope="module")
def nets():
    from balance_robot_mujoco_rl_amd import DeviceSACNets
    d = DeviceSACNets(device=0, seed=SEED, net_arch="sb3")
    yield d
    d.close()


def _sac(max_batch, **kw):
    from balance_robot_mujoco_rl_amd import DeviceSACLearner
    return DeviceSACLearner(device=0, max_batch=max_batch, seed=SEED, net_arch="sb3", **{**SC.SAC_ADAM, "target_entropy": SC.TARGET_ENTROPY, **kw})


@pytest.fixture(scope="module")
def big():
    lrn = _sac(1024)
    yield lrn
    lrn.close()


# --------------------------------------------------------------------------------------- 0. the allocation, launching nothing
def _assert_partial_rows_fit():
    rows, _ = SC.assert_partial_rows_fit(_sac, max(NA + SC.SAC_TAIL, TLEN), "[256, 256] SAC handle")
    assert rows >= 2 * 512 + 4 + 1 + S.NSTAT   # two critic images side by side, and the actor's


def test_eight_partial_rows_fit_the_allocation():
    """first in the file: the arithmetic of the handle's one allocation is known before any launch with eight workgroup rows"""
    assert SC.SPLIT_TABLE[8193][2] == SC.SPLIT_TABLE[8192][2] == SC.MAX_SPLIT
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


# --------------------------------------------------------------------------------------- 2. the target and the critic's forward
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


@pytest.mark.parametrize("m", (1, 33, 129, 257))
def test_q_on_the_wide_critic(nets, host, m):
    import torch
    c = SC.grad_case(m, "x3")
    for k in (0, 1):
        critic = np.ascontiguousarray(c["critics"][k * NC:(k + 1) * NC])
        q = Guarded((m,))
        nets.q(_cuda(critic), _cuda(c["obs"]), _cuda(c["act"]), out=q.t)
        torch.cuda.synchronize()
        assert q.intact()
        gate(q.np(), S.R.critic(critic, c["obs"], c["act"]), f"m={m} Q{k}"); gate(q.np(), A.host_q(host, critic, c["obs"], c["act"]), f"m={m} Q{k} against the host build")


# --------------------------------------------------------------------------------------- 3. the critic gradient
def _twin(lrn, dev):
    import torch
    g = Guarded((TLEN,))
    lrn.twin_critic_grad(dev["critics"], dev["obs"], dev["act"], dev["y"], out=g.t)
    torch.cuda.synchronize()
    assert g.intact(), "a kernel wrote outside the gradient buffer"
    return g.np()


@pytest.mark.parametrize("kind", ("init", "x3"))
@pytest.mark.parametrize("n", (1, 33, 129, 1000))
def test_twin_critic_gradient_against_fp64(host, big, n, kind):
    c = SC.grad_case(n, kind)
    dev = {k: _cuda(c[k]) for k in ("obs", "act", "y", "critics")}
    _poison(big)
    g = _twin(big, dev)
    assert np.isfinite(g).all() and _twin(big, dev).tobytes() == g.tobytes()
    g64 = S.twin_critic_grad(c["critics"], c["obs"], c["act"], c["y"])
    hg = SC.host_twin_critic_grad(host, c["critics"], c["obs"], c["act"], c["y"])
    for k in (0, 1):
        sl = slice(k * NC, (k + 1) * NC)
        d, dh = SC.block_distances(g[sl], g64[sl], A.CRITIC_SIZES), SC.block_distances(g[sl], hg[sl], A.CRITIC_SIZES)
        print(f"n={n} {kind} critic {k}: largest block distance from fp64 {max(d.values()):.3g}, from the host build {max(dh.values()):.3g}")
        assert max(d.values()) <= GRAD_GATE and max(dh.values()) <= GRAD_GATE, (d, dh)
    gate(g[2 * NC:], g64[2 * NC:], "statistics")


@pytest.fixture(scope="module")
def wide():
    """max_batch = 8,448: ld != mp at every row of ddpg_learner_cases.SPLIT_ROWS; the allocation's arithmetic is asserted first"""
    _assert_partial_rows_fit()
    lrn = _sac(SC.SPLIT_BIG)
    yield lrn
    lrn.close()


def _twin_dev(c):
    return {k: _cuda(c[k]) for k in ("obs", "act", "y", "critics")}


@pytest.mark.parametrize("n,kind", SC.SPLIT_TWIN_CASES)
def test_twin_critic_gradient_at_every_split_geometry(host, wide, n, kind):
    """the block gates of test_twin_critic_gradient_against_fp64 on both critics at the rows of ddpg_learner_cases.SPLIT_ROWS: two to
    eight partial rows of 2 x 68,353 + 4 floats, on a fresh handle of max_batch == m and on the NaN-filled one of 8,448, byte for byte;
    the host build up to sac_cases.HOST_ROWS_MAX"""
    c = SC.grad_case(n, kind)
    dev = _twin_dev(c)
    own = _sac(n)                           # max_batch == m, fresh
    g = _twin(own, dev)
    own.close()
    _poison(wide)                           # a larger max_batch, every word of its allocation NaN
    g_big = _twin(wide, dev)
    assert np.isfinite(g).all() and g.tobytes() == g_big.tobytes()   # nothing stale read, the handle's size does not matter
    g64 = SC.twin_reference(n, kind)
    hg = SC.host_twin_critic_grad(host, c["critics"], c["obs"], c["act"], c["y"]) if n <= SC.HOST_ROWS_MAX else None
    for k in (0, 1):
        sl = slice(k * NC, (k + 1) * NC)
        d = SC.block_distances(g[sl], g64[sl], A.CRITIC_SIZES)
        print(f"n={n} {kind} critic {k}: largest block distance from fp64 {max(d.values()):.3g}")
        assert max(d.values()) <= GRAD_GATE, d
        if hg is not None:
            dh = SC.block_distances(g[sl], hg[sl], A.CRITIC_SIZES)
            print(f"n={n} {kind} critic {k}: largest block distance from the host build {max(dh.values()):.3g}")
            assert max(dh.values()) <= GRAD_GATE, dh
    gate(g[2 * NC:], g64[2 * NC:], f"n={n} {kind} twin statistics")
    if hg is not None:
        gate(g[2 * NC:], hg[2 * NC:], f"n={n} {kind} twin statistics against the host build")


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
    if not with_host:
        return
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
    (`init` at all seven, `x3` at 513, 2,049 and 8,193, `spread` at 769 and 2,049): two to eight partial rows of 68,612 + 5 floats
    behind the two-launch chain, whose padded rows must add exact zeros; a fresh handle of max_batch == m against the NaN-filled one of
    8,448, byte for byte; the host build up to sac_cases.HOST_ROWS_MAX"""
    _check_actor_gradient(host, wide, n, kind, with_host=n <= SC.HOST_ROWS_MAX)


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
    c = SC.grad_case(33, "init")
    dev = _dev(c)
    fixed = _sac(64, learn_alpha=False)
    g, learned = _actor_grad(fixed, dev), _actor_grad(big, dev)
    fixed.close()
    assert g[NA] == 0.0 and learned[NA] != 0.0 and np.delete(g, NA).tobytes() == np.delete(learned, NA).tobytes()


# --------------------------------------------------------------------------------------- 5. the width's edge
@pytest.mark.parametrize("layer,unit", ((1, 255), (1, 0), (2, 255), (2, 0)))
def test_width_edge_models(nets, big, layer, unit):
    """256 has no padded unit: the edge of the width is the last real unit.  The layer after hidden layer `layer` reads only `unit`
    of it (255: the last register of the last tile; 0: the first), with a large weight, in the actor and both critics"""
    actor, critics = A.edge_model(layer, unit)
    c = SC.grad_case(33, "init")
    out = _act(nets, _cuda(actor), _cuda(c["obs"]), 0)
    ref = S.act(actor, c["obs"], SEED, 0, 0)
    for x, r, name in zip(out, ref, ("action", "mu", "log_std", "z")):
        gate(x, r, f"layer {layer} unit {unit} {name}")
    assert np.abs(ref[1]).max() > 1e-3   # the unit is alive in some row: the outputs are not the biases alone
    dev = {"critics": _cuda(critics), **{k: _cuda(c[k]) for k in ("obs", "act", "y")}}
    g = _twin(big, dev)
    g64 = S.twin_critic_grad(critics, c["obs"], c["act"], c["y"])
    name = {1: "W2", 2: "W3"}[layer]
    for k in (0, 1):
        d = SC.block_distances(g[k * NC:(k + 1) * NC], g64[k * NC:(k + 1) * NC], A.CRITIC_SIZES)
        print(f"layer {layer} unit {unit} critic {k}: block distances {d}")
        assert max(d.values()) <= GRAD_GATE
        sl = S.RL.block_slices(A.CRITIC_SIZES)[name]
        rows = A.CRITIC_SIZES[layer + 1]
        last, last64 = (x[k * NC + sl.start:k * NC + sl.stop].reshape(rows, 256)[rows - 1] for x in (g, g64))   # the last weight row
        assert np.linalg.norm(last64) > 0 and np.linalg.norm(last - last64) <= GRAD_GATE * np.linalg.norm(last64)
    ag = _actor_grad(big, {"obs": dev["obs"], "actor": _cuda(actor), "critics": dev["critics"]})
    a64 = S.actor_grad(actor, critics, c["obs"], SEED, 0, True, SC.TARGET_ENTROPY)
    d = SC.actor_block_distances(ag, a64)
    print(f"layer {layer} unit {unit} actor: block distances {d}")
    assert max(d.values()) <= GRAD_GATE


# --------------------------------------------------------------------------------------- 6. the refused calls
def test_ddpg_and_td3_calls_are_refused_on_an_arch_one_handle(nets, big):
    import torch
    from balance_robot_mujoco_rl_amd.policy import _p
    L = nets.L
    z = lambda *s: torch.zeros(s, device="cuda")
    out = Guarded((8, 2)); y = Guarded((8,)); g = Guarded((TLEN,))
    calls = (("brs_ddpg_act", lambda: L.brs_ddpg_act(nets.h, _p(z(NA + 1)), 8, _p(z(8, 6)), 11, 0, 0, 0.1, 0, _p(out.t), None, None, None), out),
             ("brs_ddpg_td_target", lambda: L.brs_ddpg_td_target(nets.h, _p(z(NA + 1)), _p(z(NC)), 8, _p(z(8, 6)), _p(z(8)), _p(z(8).to(torch.uint8)), 0.99,
                                                                 _p(y.t), None), y),
             ("brs_td3_td_target", lambda: L.brs_td3_td_target(nets.h, _p(z(NA + 1)), _p(z(2 * NC)), 8, _p(z(8, 6)), _p(z(8)), _p(z(8).to(torch.uint8)), 0.99,
                                                               0.2, 0.5, 11, 0, _p(y.t), None, None, None), y))
    for name, call, guard in calls:
        assert call() == -1 and L.brs_ddpg_last_error(nets.h).decode() == f"{name}: {REFUSED}"
        torch.cuda.synchronize()
        assert guard.intact() and (guard.np() == UNTOUCHED).all(), name
    lcalls = (("brs_ddpg_learner_critic_grad", lambda: L.brs_ddpg_learner_critic_grad(big.h, _p(z(NC)), 8, _p(z(8, 6)), _p(z(8, 2)), _p(z(8)), _p(g.t), None)),
              ("brs_ddpg_learner_twin_critic_grad", lambda: L.brs_ddpg_learner_twin_critic_grad(big.h, _p(z(2 * NC)), 8, _p(z(8, 6)), _p(z(8, 2)), _p(z(8)),
                                                                                                 _p(g.t), None)),
              ("brs_ddpg_learner_actor_grad", lambda: L.brs_ddpg_learner_actor_grad(big.h, _p(z(NA + 1)), _p(z(NC)), 8, _p(z(8, 6)), _p(g.t), None)))
    for name, call in lcalls:
        assert call() == -1 and L.brs_ddpg_learner_last_error(big.h).decode() == f"{name}: {REFUSED}"
        torch.cuda.synchronize()
        assert g.intact() and (g.np() == UNTOUCHED).all(), name
    # the handle still serves its own calls, and Python refuses the reference lengths before the library is asked
    c = SC.grad_case(33, "init")
    assert np.isfinite(_actor_grad(big, _dev(c))).all()
    with pytest.raises(ValueError):
        big.actor_grad(z(63105), z(2 * NC), z(8, 6), 0)
    with pytest.raises(ValueError):
        nets.sac_target(z(NA + 1), z(2 * 32101), z(8, 6), z(8), z(8).to(torch.uint8), 0.99, 0)
    assert big.scratch()[1] >= 4 * ((2 * 512 + 4 + 1 + S.NSTAT) * 1024 + 8 * max(GLEN, TLEN)) and big.state_dict()["m_actor"].shape == (NA + 1,)


# --------------------------------------------------------------------------------------- 7. non-finite rows
def test_a_nan_observation_row_at_129(nets, big):
    """a NaN planted in one observation row at m = 129: act, target and both gradients come back in the class the fp64 reference
    reports; for act and target every other row is byte-identical to the clean run"""
    import torch
    m, row = 129, 128   # the lone row of the second workgroup
    c, t = SC.act_case(m, "init"), SC.target_case(m, "init")
    clean_mask = NF.rows_mask(m, [row])
    obs = c["obs"].copy(); obs[row, 5] = np.nan
    actor = _cuda(c["actor"])
    clean, out = _act(nets, actor, _cuda(c["obs"]), 0), _act(nets, actor, _cuda(obs), 0)
    with np.errstate(all="ignore"):
        ref = S.act(c["actor"], obs, SEED, 0, 0)
    for x, r, cl, name in zip(out, ref, clean, ("action", "mu", "log_std", "z")):
        NF.check_forward(f"act {name}", x, r, cl, clean_mask)
    assert np.isnan(out[0][row]).all() and np.isfinite(out[3]).all()   # the action is a NaN for the simulator's guard to see; z is not
    nobs = t["next_obs"].copy(); nobs[row, 0] = np.nan
    dev = {k: _cuda(t[k]) for k in ("actor", "critics", "next_obs", "reward", "done")}
    clean_t = _target(nets, dev, 0)
    out_t = _target(nets, {**dev, "next_obs": _cuda(nobs)}, 0)
    with np.errstate(all="ignore"):
        y64, a64, lp64, z64 = S.sac_target(t["actor"], t["critics"], nobs, t["reward"], t["done"], GAMMA, SEED, 0)
    if t["done"][row]:
        y64 = y64.copy(); y64[row] = t["reward"][row]   # a done row returns its reward, whatever Q' is
    for x, r, cl, name in zip(out_t, (y64, a64, lp64, z64), clean_t, ("y", "a", "logp", "z")):
        NF.check_forward(f"target {name}", x, r, cl, clean_mask if x.ndim == 2 else clean_mask[:, 0])
    g = SC.grad_case(m, "init")
    gobs = g["obs"].copy(); gobs[row, 2] = np.nan
    gdev = {"critics": _cuda(g["critics"]), "actor": _cuda(g["actor"]), "obs": _cuda(gobs), "act": _cuda(g["act"]), "y": _cuda(g["y"])}
    with np.errstate(all="ignore"):
        tw64 = S.twin_critic_grad(g["critics"], gobs, g["act"], g["y"])
        ag64 = S.actor_grad(g["actor"], g["critics"], gobs, SEED, 0, True, SC.TARGET_ENTROPY)
    assert np.isnan(tw64[:2 * NC]).any() and np.isnan(ag64[:NA]).any()   # the poison reaches the reference: the case proves something
    NF.check_gradient_nans("twin critic gradient", _twin(big, gdev), tw64)
    NF.check_gradient_nans("actor gradient", _actor_grad(big, gdev), ag64)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------- 8. whole steps
def test_six_chained_steps_with_the_temperature_moving(nets, host):
    """brs_sac_td_target from the current actor and the critics' target -> DeviceSACLearner.step, six times, on the kernels and on the
    host build, each against the same chain in fp64 by the trajectory rule"""
    case = SC.chain_case(A.CHAIN_KIND)
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
    """tools/train_sac_torch.py --net-arch sb3 --envs 64 --steps 40 --batch 64 --device-data --device-learner: it trains, everything
    is finite, all vectors and log_ent_coef moved, the target less than the critics.  No learning-quality gate."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_sac_torch as T
    log = T.main(["--net-arch", "sb3", "--envs", "64", "--steps", "40", "--batch", "64", "--device-data", "--device-learner"])
    assert log["updates"] == 39 and log["args"]["net_arch"] == "sb3"   # 100 transitions are in after two steps of 64 envs
    assert log["finite"] and log["learner"] == "device" and log["data_path"] == "device"
    assert all(log["moved"][k] > 0 for k in ("actor", "critics", "critics_target", "log_ent_coef")), log["moved"]
    assert log["moved"]["critics_target"] < log["moved"]["critics"]
    assert np.isfinite(log["critic_loss_last"]) and log["critic_loss_last"] > 0 and np.isfinite(log["actor_loss_last"])
    assert np.isfinite(log["ent_coef"]) and log["ent_coef"] > 0 and log["ent_coef"] != 1.0
