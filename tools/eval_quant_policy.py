#!/usr/bin/env python3
"""Does a policy survive int8?  The reference answers this with its `test-tflite-quant` command (src/sb_rl.py:285-364): one
env, the TFLite interpreter, a person watching the viewer.  This tool runs the same deployment check on a registered id of
THIS simulator for thousands of envs without leaving the GPU: once with the float network (DevicePolicy, deterministic) and
once with the int8 network (QuantPolicy, the bit-exact integer kernel of include/brs_qpolicy.h), same seed, and prints the
episode statistics of tools/eval_reference_policy.py for both, then their differences.  Both runs apply the network's raw
output, unclipped, as the reference does (envs/RobotMoveBaseEnv.py:178-208).

    python tools/eval_quant_policy.py --env Env01-v3 --envs 4096 --steps 1500                    # the reference's own export
    python tools/eval_quant_policy.py --env Env03-v2 --params policy.npy --save policy_int8.npz  # a policy trained here

--npz PATH     an int8 export in the key set of tests/golden/robot_move_policy.npz (default: that file); the float run uses
               its dequantised weights
--params PATH  a float parameter vector (.npy, the order of include/brs_policy.h): quantised here with quantize_policy and
               the reference's calibration rows; the float run uses the vector itself
--actor PATH   an OFF-POLICY actor, 6-300-200-2 or (SAC) 6-256-256-2: the flat vector (.npy) or the state_dict (.pt) that
               tools/train_ddpg_torch.py, train_td3_torch.py or train_sac_torch.py write with --save-actor; --algo ddpg|td3|sac
               says how to read it.  Quantised here with quantize_actor; the float run is DeviceDDPGNets.act with sigma 0, or
               DeviceSACNets.act deterministic, and the int8 run QuantActor (for SAC: the deterministic action tanh(mu)).
               With --algo sac the widths are read off the file: the reference's pi=[300, 200], or SB3's default [256, 256] --
               what tools/train_sac_torch.py --net-arch sb3 --save-actor writes, or an SB3 SAC state_dict;
               both runs then use that architecture, and the JSON lines name it (net_arch)

    python tools/eval_quant_policy.py --env Env01-v1 --actor actor.npy --algo td3 --save actor_int8.npz
"""
import argparse, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor, QuantModel, QuantPolicy, _lib, quantize_policy  # noqa: E402
from balance_robot_mujoco_rl_amd.policy import DevicePolicy  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "robot_move_policy.npz")


def evaluate(env, n, steps, act, seed=123):
    """deterministic evaluation with auto-reset; act(obs, t) -> actions [n, 2].  Every episode that ends within `steps` steps
    counts (an EpisodeMonitor without targets)"""
    sim = BatchedSim(env, n, device=0, seed=seed, auto_reset=True)
    mon = EpisodeMonitor(n, device=0, max_len=sim.max_episode_steps)
    obs = sim.reset()
    for t in range(steps):
        obs, r, te, tr, _ = sim.step(act(obs, t))
        mon.update(r, te, tr)
    s, median = mon.stats(), mon.median_len(lower=True)
    sim.close(); mon.close()
    return dict(episodes=s.episodes, first_episode_still_running=s.first_running, fell=s.terminated, reached_time_limit=s.time_limit,
                mean_ep_len=s.mean_len, median_ep_len=median, mean_reward_per_step=(s.sum_ret + s.running_ret) / (n * steps))


def read_actor(path):
    """a .pt state_dict or a .npy flat vector, as the train tools' --save-actor writes them"""
    return torch.load(path, map_location="cpu", weights_only=True) if path.endswith(".pt") else np.load(path).astype(np.float32).ravel()


def read_sac_actor(path):
    """-> (what the file holds, the flat SAC actor vector with log_ent_coef [nactor + 1], net_arch): the widths are those of the
    tensors' shapes (flatten_sac_actor) or of the vector's length"""
    from balance_robot_mujoco_rl_amd import flatten_sac_actor
    params = read_actor(path)
    flat = flatten_sac_actor(params) if isinstance(params, dict) else params
    net_arch = {_lib.SAC_NACTOR: "reference", _lib.SAC256_NACTOR: "sb3"}.get(flat.size, None) or \
               {_lib.SAC_NACTOR + 1: "reference", _lib.SAC256_NACTOR + 1: "sb3"}.get(flat.size, None)
    if net_arch is None:
        raise ValueError(f"{path}: a SAC actor has {_lib.SAC_NACTOR} (+ 1) elements at pi=[300, 200] or {_lib.SAC256_NACTOR} (+ 1) at [256, 256], "
                         f"this one {flat.size}")
    if flat.size in (_lib.SAC_NACTOR, _lib.SAC256_NACTOR):
        flat = np.concatenate([flat, np.zeros(1, np.float32)])   # log_ent_coef: unused by act
    return params, np.ascontiguousarray(flat, np.float32), net_arch


def evaluate_actor(a):
    """--actor: the same three lines for the off-policy actor"""
    from balance_robot_mujoco_rl_amd import DeviceDDPGNets, DeviceSACNets, QuantActor, quantize_actor
    sac = a.algo == "sac"
    params, flat, net_arch = read_sac_actor(a.actor) if sac else (read_actor(a.actor), None, "reference")
    if a.vec_normalize:
        # an actor trained behind a normaliser (--vec-normalize of the train tools): its statistics folded into the first layer, so
        # that the quantiser, the int8 kernel and both runs below take the simulator's raw observations
        from balance_robot_mujoco_rl_amd import fold_vecnormalize
        with np.load(a.vec_normalize) as z:
            params = flat = fold_vecnormalize(flat if sac else ddpg_flat(params), dict(z), net_arch=net_arch)
    qm = quantize_actor(params, head="sac" if sac else "ddpg", net_arch=net_arch)
    if a.save:
        qm.save(a.save)
    if sac:
        nets = DeviceSACNets(device=0, net_arch=net_arch)
        weights = torch.from_numpy(np.ascontiguousarray(flat, np.float32)).cuda()
        float_act, name = (lambda obs, t: nets.act(weights, obs, t, deterministic=True)), "float (DeviceSACNets, deterministic)"
    else:
        nets = DeviceDDPGNets(device=0)
        weights = torch.from_numpy(ddpg_flat(params)).cuda()
        float_act, name = (lambda obs, t: nets.act(weights, obs, t, 0.0)), "float (DeviceDDPGNets, sigma 0)"
    qact = QuantActor(qm, device=0)
    common = dict(env=a.env, envs=a.envs, steps=a.steps, policy=f"{os.path.basename(a.actor)} ({a.algo} actor, quantised here)",
                  net_arch=net_arch, build_id=_lib.build_id())
    f = evaluate(a.env, a.envs, a.steps, float_act)
    print(json.dumps(dict(common, network=name, **f)))
    q = evaluate(a.env, a.envs, a.steps, lambda obs, t: qact.act(obs))
    print(json.dumps(dict(common, network="int8 (QuantActor)", **q)))
    diff = {k: (None if f[k] is None or q[k] is None else q[k] - f[k]) for k in f}
    print(json.dumps(dict(common, network="int8 - float", **diff)))


def ddpg_flat(params):
    """a DDPG / TD3 actor, flat or as a state_dict -> the flat float32 vector"""
    from balance_robot_mujoco_rl_amd import flatten_ddpg_state_dict
    return np.ascontiguousarray(flatten_ddpg_state_dict(params) if isinstance(params, dict) else params, np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--env", default="Env01-v3"); ap.add_argument("--envs", type=int, default=4096); ap.add_argument("--steps", type=int, default=1500)
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--npz"); src.add_argument("--params"); src.add_argument("--actor")
    ap.add_argument("--algo", choices=("ddpg", "td3", "sac"), default="ddpg", help="how --actor is read")
    ap.add_argument("--head", choices=("mean", "actions"), default="mean")
    ap.add_argument("--save", help="write the int8 model that was evaluated to this .npz")
    ap.add_argument("--vec-normalize", metavar="NPZ", help="with --actor: the .vecnormalize.npz a train tool wrote next to the actor; its "
                                                          "observation statistics are folded into the actor's first layer before quantising")
    a = ap.parse_args(argv)
    if a.vec_normalize and not a.actor:
        ap.error("--vec-normalize goes with --actor")
    if a.actor:
        return evaluate_actor(a)
    if a.params:
        flat = np.load(a.params).astype(np.float32).ravel()
        qm, what = quantize_policy(flat), f"{os.path.basename(a.params)} (quantised here)"
    else:
        qm = QuantModel.load(a.npz or FIXTURE, a.head)
        flat, what = qm.float_params(), f"{os.path.basename(a.npz or FIXTURE)} ({a.head} output)"
    if a.save:
        qm.save(a.save)
    fpol = DevicePolicy(device=0); fpol.set_weights(flat)
    qpol = QuantPolicy(qm, device=0)
    common = dict(env=a.env, envs=a.envs, steps=a.steps, policy=what, build_id=_lib.build_id())
    f = evaluate(a.env, a.envs, a.steps, lambda obs, t: fpol.act(obs, t, deterministic=True)[0])
    print(json.dumps(dict(common, network="float (DevicePolicy, deterministic)", **f)))
    q = evaluate(a.env, a.envs, a.steps, lambda obs, t: qpol.act(obs))
    print(json.dumps(dict(common, network="int8 (QuantPolicy)", **q)))
    diff = {k: (None if f[k] is None or q[k] is None else q[k] - f[k]) for k in f}
    print(json.dumps(dict(common, network="int8 - float", **diff)))


if __name__ == "__main__":
    main()
