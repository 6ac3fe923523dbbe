#!/usr/bin/env python3
"""How does the policy the reference ships (envs/RobotMovePolicy.tflite -> tests/golden/robot_move_policy.npz, dequantised
weights through the on-device policy kernels) fare on a registered id of THIS simulator?  Deterministic evaluation, episode
statistics as tools/train_ppo_torch.py's evaluate() prints them.  A reading aid for config 5: what a policy trained against
MuJoCo by the reference's author achieves on the envs the curriculum uses.

    python tools/eval_reference_policy.py --env Env01-v2 --envs 4096 --steps 1500
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from balance_robot_mujoco_rl_amd import BatchedSim, EpisodeMonitor  # noqa: E402
from balance_robot_mujoco_rl_amd.policy import DevicePolicy  # noqa: E402
from quant_policy import QuantMovePolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="Env01-v2"); ap.add_argument("--envs", type=int, default=4096); ap.add_argument("--steps", type=int, default=1500)
    a = ap.parse_args()
    pol = DevicePolicy(device=0); pol.set_weights(QuantMovePolicy().float_params("mean"))
    sim = BatchedSim(a.env, a.envs, device=0, seed=123, auto_reset=True)
    mon = EpisodeMonitor(a.envs, device=0, max_len=sim.max_episode_steps)   # every episode that ends within --steps counts
    obs = sim.reset()
    n = a.envs
    for t in range(a.steps):
        _, ac, _, _ = pol.act(obs, t, deterministic=True)
        obs, r, te, tr, _ = sim.step(ac)
        mon.update(r, te, tr)
    s = mon.stats()
    print(json.dumps(dict(env=a.env, envs=n, steps=a.steps, policy="reference RobotMovePolicy (dequantised, mean output)", episodes=s.episodes,
                          first_episode_still_running=s.first_running, fell=s.terminated, reached_time_limit=s.time_limit,
                          mean_ep_len=s.mean_len, median_ep_len=mon.median_len(lower=True))))


if __name__ == "__main__":
    main()
