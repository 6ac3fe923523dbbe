"""MI355X-native batched simulator of the two-wheel balance-robot environments (Env01 / Env03 families).

The hot path -- Env.step()/reset() of lachlanhurst/balance-robot-mujoco-rl, i.e. 250 MuJoCo substeps plus reward /
observation / termination / block state machine per env step -- runs as hand-written HIP kernels behind the C ABI in
include/brs.h (libbrs_hip.so).  This package is the host-side mirror of the reference's env interface:

    registry.make_vec(id, num_envs, ...)   ~ gym.make(id)  (src/balance_robot/__init__.py:5-52 of the reference)
    BalanceVecEnv                          ~ the SB3 VecEnv that sb_rl.py's PPO consumes (sb_rl.py:63-71, 552)
    BatchedSim                             zero-copy torch-tensor interface to the kernels
    policy.DevicePolicy / DeviceRollout    SB3 MlpPolicy forward + sampling, time-limit bootstrap and GAE as HIP kernels
                                           (include/brs_policy.h): the rollout side of sb_rl.py:63-71, 552-556 on the GPU
    monitor.EpisodeMonitor / evaluate_policy
                                           SB3's Monitor and evaluate_policy (sb_rl.py:501, 536-543): episode returns and lengths
                                           accumulated by a HIP kernel per env step (include/brs_policy.h: brs_monitor_*)
    learner.DevicePPOLearner               SB3's PPO.train() minibatch body -- clipped-surrogate gradient, clip_grad_norm_, Adam -- as HIP
                                           kernels (include/brs_policy.h: brs_learner_*): the learner side of sb_rl.py:552-556
    learner.DeviceA2CLearner               SB3's A2C.train() -- one -adv log pi gradient over the whole rollout, clip_grad_norm_,
                                           RMSpropTFLike -- on the same handle (include/brs_policy.h: brs_a2c_*): sb_rl.py's `-a A2C`
    offpolicy.DeviceDDPGNets / DeviceReplayBuffer / DeviceOffPolicyCollector
                                           SB3's DDPG between two gradient steps -- actor with action noise, replay buffer with the
                                           terminal-observation and time-limit rules, uniform sampling, TD targets -- as HIP kernels
                                           (include/brs_policy.h: brs_ddpg_*, brs_replay_*): the data path of sb_rl.py:72-83
    offpolicy.DeviceDDPGLearner            SB3's TD3.train as DDPG uses it -- critic and actor gradient, Adam, Polyak update -- as HIP
                                           kernels (include/brs_policy.h: brs_ddpg_learner_*): the learner side of sb_rl.py:72-83
    offpolicy.DeviceTD3Learner / DeviceDDPGNets.td3_target
                                           TD3's three changes to that recipe -- smoothed twin-critic target, twin critic gradient,
                                           delayed actor and target updates -- (include/brs_policy.h: brs_td3_td_target,
                                           brs_ddpg_learner_twin_critic_grad): sb_rl.py's `-a TD3` with the DDPG net_arch
    offpolicy.DeviceSACNets / DeviceSACLearner
                                           SAC on the same widths -- squashed-Gaussian actor, entropy target, the actor's chain through
                                           both critics, the learned temperature -- (include/brs_policy.h: brs_sac_*,
                                           brs_ddpg_learner_create_sac): sb_rl.py's `-a SAC` with the DDPG net_arch, or with
                                           net_arch="sb3" on SB3's default [256, 256], what `-a SAC` itself builds
    vecnorm.DeviceVecNormalize             SB3's VecNormalize -- running mean and variance of the observations and of the discounted
                                           return in fp64, clipping -- as HIP kernels between the simulator and the algorithm
                                           (include/brs_policy.h: brs_vecnorm_*); for DDPG, TD3 and SAC the collector
                                           takes it as `normalize=`, DeviceReplayBuffer.sample(..., normalize=) normalises the minibatch
                                           in the sampling kernel, and vecnorm.fold_vecnormalize folds the statistics into an actor's
                                           first layer for deployment on raw observations
    quant.quantize_policy / QuantPolicy    int8 post-training quantisation of the actor and the int8 network as a HIP kernel
                                           (include/brs_qpolicy.h): quantize_tflite.py and sb_rl.py:285-364 on the GPU
    quant.quantize_actor / QuantActor      the same deployment check for the actor DDPG, TD3 and SAC train, 6-300-200-2 with ReLU and
                                           a tanh output (include/brs_qpolicy.h: brs_qpolicy_actor_*)

There is no CPU fallback: creating a sim without a HIP device raises.
"""
from .registry import ENV_SPECS, make_vec, spec  # noqa: F401
from .learner import DeviceA2CLearner, DevicePPOLearner, LearnerStats  # noqa: F401
from .offpolicy import (DeviceDDPGLearner, DeviceDDPGNets, DeviceOffPolicyCollector, DeviceReplayBuffer, DeviceSACLearner,  # noqa: F401
                        DeviceSACNets, DeviceTD3Learner, flatten_ddpg_state_dict, flatten_sac_actor, flatten_td3_critics,
                        unflatten_ddpg_state_dict, unflatten_sac_actor, unflatten_td3_critics)
from .monitor import EpisodeMonitor, EpisodeStats, episode_count_targets, evaluate_policy  # noqa: F401
from .quant import (REFERENCE_CALIBRATION, QuantActor, QuantActorModel, QuantModel, QuantPolicy, quantize_actor,  # noqa: F401
                    quantize_policy)
from .sim import BatchedSim, BrsError  # noqa: F401
from .vec_env import BalanceVecEnv  # noqa: F401
from .vecnorm import DeviceVecNormalize, fold_vecnormalize  # noqa: F401

__all__ = ["BatchedSim", "BalanceVecEnv", "BrsError", "DeviceA2CLearner", "DeviceDDPGLearner", "DeviceDDPGNets", "DeviceOffPolicyCollector", "DevicePPOLearner", "DeviceReplayBuffer", "DeviceSACLearner", "DeviceSACNets", "DeviceTD3Learner", "DeviceVecNormalize", "ENV_SPECS", "EpisodeMonitor", "EpisodeStats", "LearnerStats",
           "QuantActor", "QuantActorModel", "QuantModel", "QuantPolicy",
           "REFERENCE_CALIBRATION", "episode_count_targets", "evaluate_policy", "flatten_ddpg_state_dict", "flatten_sac_actor", "flatten_td3_critics", "fold_vecnormalize", "make_vec", "quantize_actor", "quantize_policy", "spec",
           "unflatten_ddpg_state_dict", "unflatten_sac_actor", "unflatten_td3_critics"]
