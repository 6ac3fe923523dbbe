"""ctypes binding of libbrs_hip.so (C ABI: include/brs.h).  Loading never needs a GPU; brs_create does."""
import ctypes as C
import glob
import hashlib
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libbrs_hip.so")
_CSRC, _INCLUDE = os.path.join(_PKG, "csrc"), os.path.join(os.path.dirname(_PKG), "include")
BASE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]
# step kernels: -ffast-math on the DEVICE side only (the host-side state conversion keeps IEEE semantics): no IEEE
# division/sqrt expansions and free reassociation inside the fp32 force path (parity budget is 1e-4, rounding noise 1e-7);
# NaN detection in the kernel is done on the bit pattern.
SIM_FLAGS = ["-Xarch_device", "-ffast-math", "-Xarch_device", "-fgpu-flush-denormals-to-zero",
             # the dense algebra is packed by hand (V2 -> v_pk_fma_f32); the SLP vectoriser's extra packing of the scalar
             # code only adds pack/unpack moves (measured: +13 % env-steps/s without it)
             "-Xarch_device", "-fno-slp-vectorize",
             # one wave per SIMD at 512 registers: there is no occupancy to protect, yet the default strategy schedules
             # for register pressure and leaves serial chains (a dependent VALU instruction issues ~1.7x slower than
             # an independent one for a lone wave).  The ILP strategy: +4.3 % Env03, +2.7 % Env01 (same-box A/B)
             "-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]
# the translation units of libbrs_hip.so: (source, its own flags, in the build id).  Policy / GAE kernels, renderer and int8 actors
# keep IEEE math (checked against fp32 torch at rtol 1e-5 / bit for bit against their host builds under tests/), and so does the
# episode monitor, the PPO learner (fp64 torch autograd at 1e-5 per parameter block), the DDPG data path (fp64 numpy at 1e-5) and
# the DDPG learner (fp64 torch autograd at 1e-5 per block); the build id names the step and policy kernels that committed profiles
# were measured on, so the other eight units stay out of it.  VecNormalize (fp64 statistics, byte for byte against its host build) is
# the eighth.
UNITS = [("brs_kernels.hip", SIM_FLAGS, True), ("brs_policy.hip", [], True), ("brs_render.hip", [], False), ("brs_qpolicy.hip", [], False),
         ("brs_monitor.hip", [], False), ("brs_learner.hip", [], False), ("brs_offpolicy.hip", [], False),
         ("brs_ddpg_learner.hip", [], False), ("brs_qactor.hip", [], False), ("brs_vecnorm.hip", [], False)]
SRC = os.path.join(_CSRC, UNITS[0][0])  # the unit that takes the A/B flags and the build id stamp
# what the build id hashes next to the sources of its units; brs_host.hpp holds no kernel code and stays out of it.  The policy
# kernels take their tower tiling from brs_policy_tile.hpp and, through it, the parameter layout from brs_learner.hpp
HEADERS = [os.path.join(_CSRC, h) for h in ("brs_core.hpp", "brs_model.hpp", "brs_state.hpp", "brs_nan.hpp", "brs_policy_tile.hpp",
                                            "brs_learner.hpp")] + \
          [os.path.join(_INCLUDE, h) for h in ("brs.h", "brs_policy.h")]

POLICY_NPARAM = (64 * 6 + 64 + 64 * 64 + 64 + 2 * 64 + 2) + (64 * 6 + 64 + 64 * 64 + 64 + 64 + 1) + 2
DDPG_NACTOR = 300 * 6 + 300 + 200 * 300 + 200 + 2 * 200 + 2     # BRS_DDPG_NACTOR
DDPG_NCRITIC = 200 * 8 + 200 + 150 * 200 + 150 + 1 * 150 + 1    # BRS_DDPG_NCRITIC
DDPG_TAG_ACT, DDPG_TAG_SAMPLE = 0x44445047, 0x5245504c
TD3_TAG_NOISE = 0x5444334e                                      # BRS_TD3_TAG_NOISE
SAC_NACTOR = 300 * 6 + 300 + 200 * 300 + 200 + 4 * 200 + 4      # BRS_SAC_NACTOR; the actor vector holds one more, log_ent_coef
SAC_TAG_ACT, SAC_TAG_TARGET, SAC_TAG_PI = 0x53414341, 0x53414354, 0x53414350
ARCH_REFERENCE, ARCH_SAC_DEFAULT = 0, 1                         # BRS_ARCH_*: pi=[300, 200] qf=[200, 150]; SB3's default [256, 256]
SAC256_NACTOR = 256 * 6 + 256 + 256 * 256 + 256 + 4 * 256 + 4   # BRS_SAC256_NACTOR; the actor vector holds one more, log_ent_coef
SAC256_NCRITIC = 256 * 8 + 256 + 256 * 256 + 256 + 1 * 256 + 1  # BRS_SAC256_NCRITIC


class BrsConfig(C.Structure):
    _fields_ = [("variant", C.c_int32), ("num_envs", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("seed", C.c_uint64), ("env_index_base", C.c_int64), ("max_episode_steps", C.c_int32),
                ("substeps", C.c_int32), ("timestep", C.c_double), ("block_threads", C.c_int32), ("reserved", C.c_int32)]


class BrsCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fovy_deg", C.c_float), ("distance", C.c_float),
                ("azimuth_deg", C.c_float), ("elevation_deg", C.c_float)]


class BrsEpisodeStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("episodes", "ended", "terminated", "time_limit", "sum_len", "sum_len2", "steps")] + \
               [(k, C.c_double) for k in ("sum_ret", "sum_ret2", "min_ret", "max_ret", "running_ret")] + \
               [(k, C.c_int32) for k in ("min_len", "max_len", "first_running", "pending")]


LEARNER_NSTAT = 5
DDPG_NSTAT = 2                                                  # BRS_DDPG_NSTAT
TD3_NSTAT = 4                                                   # BRS_TD3_NSTAT
SAC_NSTAT = 4                                                   # BRS_SAC_NSTAT


class BrsPpoConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("lr", "beta1", "beta2", "eps")] + \
               [(k, C.c_float) for k in ("clip_range", "vf_coef", "ent_coef", "max_grad_norm_pi", "max_grad_norm_vf", "target_kl", "ret_scale")] + \
               [(k, C.c_int32) for k in ("normalize_adv", "actor_on", "joint_norm")]


class BrsA2cConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("lr", "alpha", "eps")] + \
               [(k, C.c_float) for k in ("vf_coef", "ent_coef", "max_grad_norm_pi", "max_grad_norm_vf", "ret_scale")] + \
               [(k, C.c_int32) for k in ("normalize_adv", "actor_on", "joint_norm")]


class BrsAdamConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("lr", "beta1", "beta2", "eps")]


class BrsLearnerInfo(C.Structure):
    _fields_ = [("steps", C.c_int64), ("stopped", C.c_int32), ("bad_index", C.c_int32), ("stat", C.c_float * LEARNER_NSTAT),
                ("grad_norm_pi", C.c_float), ("grad_norm_vf", C.c_float)]


class BrsReplayStorage(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("obs", "next_obs", "action", "reward", "done")]


class BrsVecnormConfig(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("gamma", "epsilon", "clip_obs", "clip_reward")] + [(k, C.c_int32) for k in ("norm_obs", "norm_reward")]


class BrsVecnormStats(C.Structure):
    _fields_ = [(k, C.c_double * 6) for k in ("obs_mean", "obs_var", "obs_count")] + [(k, C.c_double) for k in ("ret_mean", "ret_var", "ret_count")]


class BrsQLayer(C.Structure):
    _fields_ = [("n_in", C.c_int32), ("n_out", C.c_int32), ("weight", C.c_void_p), ("bias", C.c_void_p), ("bias_scale", C.c_void_p),
                ("out_scale", C.c_double), ("out_zero", C.c_int32), ("tanh_zero", C.c_int32), ("tanh_table", C.c_void_p)]


class BrsQModel(C.Structure):
    _fields_ = [("input_scale", C.c_double), ("input_zero", C.c_int32), ("reserved", C.c_int32), ("layer", BrsQLayer * 3)]


class BrsQActorModel(C.Structure):
    _fields_ = [("input_scale", C.c_double), ("input_zero", C.c_int32), ("action_zero", C.c_int32), ("action_scale", C.c_double),
                ("layer", BrsQLayer * 3)]


FLAG_AUTO_RESET, FLAG_NOISE_ON, FLAG_NOISE_OFF, FLAG_NO_LANE_GROUPING = 1, 2, 4, 8


def hipcc_path():
    for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if p and (os.path.sep not in p or os.path.exists(p)):
            return p
    return "hipcc"


def build(force=False, verbose=False, out=None, extra_flags=()):
    """compile the HIP kernels + C ABI for gfx950 in-tree (hipcc cross-compiles without a GPU).  `out` / `extra_flags`: an A/B
    build next to the product library (tools/ab_build.py; loaded only when BRS_HIP_LIB points at it)"""
    if out is not None:
        return _compile(out, verbose, list(extra_flags), tag="_" + os.path.splitext(os.path.basename(out))[0])
    srcs = glob.glob(os.path.join(_CSRC, "*.h*")) + glob.glob(os.path.join(_INCLUDE, "*.h"))  # every .hip, .hpp and ABI header
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if not (force or stale):
        return LIB_PATH
    return _compile(LIB_PATH, verbose, [], tag="")


def _build_id(sim_flags):
    """hash of every source of the step and policy kernels + the flags: ties a committed rocprof summary to the code that ran"""
    hsh = hashlib.sha256()
    for f in sorted([os.path.join(_CSRC, u[0]) for u in UNITS if u[2]] + HEADERS):
        hsh.update(open(f, "rb").read())
    hsh.update(" ".join(BASE_FLAGS + [a for a in sim_flags if not a.startswith("-Rpass")]).encode())
    return hsh.hexdigest()[:16]


def _compile(lib_path, verbose, extra_flags, tag):
    hipcc, objs = hipcc_path(), []
    # BRS_EXTRA_HIPCC_FLAGS: builds with a compile-time switch (e.g. -DBRS_NO_COUPLED); not for production
    sim_flags = SIM_FLAGS + os.environ.get("BRS_EXTRA_HIPCC_FLAGS", "").split() + extra_flags
    for name, flags, _ in UNITS:
        src, obj = os.path.join(_CSRC, name), os.path.join(_CSRC, os.path.splitext(name)[0] + tag + ".o")
        if src == SRC:
            flags = sim_flags + [f'-DBRS_BUILD_ID="{_build_id(sim_flags)}"']
        remarks = ["-Rpass-analysis=kernel-resource-usage"] if verbose else []
        subprocess.check_call([hipcc] + BASE_FLAGS + flags + remarks + ["-c", "-o", obj, src])
        objs.append(obj)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib_path] + objs)
    return lib_path


_vp, _i32, _f32, _dp, _i32p = C.c_void_p, C.c_int32, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_int32)
# the C ABI, header by header: name -> (restype, argtypes).  lib() applies it; tests/test_c_abi.py holds it against the headers
SIGNATURES = {
    "brs.h": {
        "brs_create": (C.c_int, [C.POINTER(BrsConfig), C.POINTER(_vp)]),
        "brs_destroy": (C.c_int, [_vp]),
        "brs_last_error": (C.c_char_p, [_vp]),
        "brs_sizes": (C.c_int, [_i32, _i32p, _i32p, _i32p, _i32p]),
        "brs_reset": (C.c_int, [_vp, _vp, _vp, _vp]),
        "brs_step": (C.c_int, [_vp] * 8),
        "brs_physics": (C.c_int, [_vp, _vp, _i32, _vp]),
        "brs_get_state": (C.c_int, [_vp, _dp, _dp, _dp, _dp]),
        "brs_set_state": (C.c_int, [_vp, _dp, _dp, _dp, _dp]),
        "brs_get_aux": (C.c_int, [_vp, _dp]),
        "brs_set_aux": (C.c_int, [_vp, _dp]),
        "brs_get_xpose": (C.c_int, [_vp, _dp, _dp]),
        "brs_set_xpose": (C.c_int, [_vp, _dp, _dp]),
        "brs_get_lane_map": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
        "brs_step_bytes_per_env": (C.c_int64, [_vp]),
        "brs_step_kernel_name": (C.c_char_p, [_vp]),
        "brs_build_id": (C.c_char_p, []),
    },
    "brs_policy.h": {
        "brs_policy_create": (C.c_int, [_i32, C.POINTER(_vp)]),
        "brs_policy_destroy": (C.c_int, [_vp]),
        "brs_policy_last_error": (C.c_char_p, [_vp]),
        "brs_policy_set_weights": (C.c_int, [_vp, C.POINTER(C.c_float)]),
        "brs_policy_use_device_weights": (C.c_int, [_vp, _vp]),
        "brs_policy_act": (C.c_int, [_vp, _i32, _vp, C.c_uint64, C.c_int64, C.c_uint32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
        "brs_policy_value": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
        "brs_rollout_bootstrap": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _f32, _vp, _vp]),
        "brs_gae": (C.c_int, [_i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp]),
        "brs_monitor_create": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_vp)]),
        "brs_monitor_destroy": (C.c_int, [_vp]),
        "brs_monitor_last_error": (C.c_char_p, [_vp]),
        "brs_monitor_reset": (C.c_int, [_vp, _i32p, _vp]),
        "brs_monitor_update": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
        "brs_monitor_stats": (C.c_int, [_vp, C.POINTER(BrsEpisodeStats), _vp]),
        "brs_monitor_histogram": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp]),
        "brs_monitor_episodes": (C.c_int, [_vp, _i32p, _dp, _i32p, C.POINTER(C.c_uint8), _vp]),
        "brs_learner_create": (C.c_int, [_i32, _i32, C.POINTER(_vp)]),
        "brs_learner_destroy": (C.c_int, [_vp]),
        "brs_learner_last_error": (C.c_char_p, [_vp]),
        "brs_learner_begin_iteration": (C.c_int, [_vp, _vp]),
        "brs_learner_grad": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, C.POINTER(BrsPpoConfig), _vp, _vp]),
        "brs_learner_apply": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.POINTER(BrsPpoConfig), _vp]),
        "brs_learner_stats": (C.c_int, [_vp, C.POINTER(BrsLearnerInfo), _vp]),
        "brs_a2c_grad": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, C.POINTER(BrsA2cConfig), _vp, _vp]),
        "brs_a2c_apply": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(BrsA2cConfig), _vp]),
        "brs_ddpg_create": (C.c_int, [_i32, C.POINTER(_vp)]),
        "brs_ddpg_destroy": (C.c_int, [_vp]),
        "brs_ddpg_last_error": (C.c_char_p, [_vp]),
        "brs_ddpg_act": (C.c_int, [_vp, _vp, _i32, _vp, C.c_uint64, C.c_int64, C.c_uint32, _f32, _i32, _vp, _vp, _vp, _vp]),
        "brs_ddpg_q": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp]),
        "brs_ddpg_td_target": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _vp, _vp]),
        "brs_td3_td_target": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _f32, _f32, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp]),
        "brs_replay_add": (C.c_int, [_i32, C.POINTER(BrsReplayStorage), _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
        "brs_replay_sample": (C.c_int, [_i32, C.POINTER(BrsReplayStorage), _i32, _i32, _i32, _i32, C.c_uint64, C.c_uint32,
                                        C.POINTER(BrsReplayStorage), _vp, _vp]),
        "brs_replay_last_error": (C.c_char_p, []),
        "brs_ddpg_learner_create": (C.c_int, [_i32, _i32, C.POINTER(_vp)]),
        "brs_ddpg_learner_destroy": (C.c_int, [_vp]),
        "brs_ddpg_learner_last_error": (C.c_char_p, [_vp]),
        "brs_ddpg_learner_scratch": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_int64)]),
        "brs_ddpg_learner_critic_grad": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
        "brs_ddpg_learner_actor_grad": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
        "brs_ddpg_learner_apply": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, C.POINTER(BrsAdamConfig), C.c_int64, _f32, _vp]),
        "brs_ddpg_learner_create_twin": (C.c_int, [_i32, _i32, C.POINTER(_vp)]),
        "brs_ddpg_learner_twin_critic_grad": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
        "brs_sac_act": (C.c_int, [_vp, _vp, _i32, _vp, C.c_uint64, C.c_int64, C.c_uint32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
        "brs_sac_td_target": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _f32, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
        "brs_ddpg_learner_create_sac": (C.c_int, [_i32, _i32, C.POINTER(_vp)]),
        "brs_sac_twin_critic_grad": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
        "brs_sac_actor_grad": (C.c_int, [_vp, _vp, _vp, _i32, _vp, C.c_uint64, C.c_uint32, _i32, _f32, _vp, _vp]),
        "brs_ddpg_create_arch": (C.c_int, [_i32, _i32, C.POINTER(_vp)]),
        "brs_ddpg_learner_create_sac_arch": (C.c_int, [_i32, _i32, _i32, C.POINTER(_vp)]),
        "brs_vecnorm_create": (C.c_int, [_i32, _i32, C.POINTER(BrsVecnormConfig), C.POINTER(_vp)]),
        "brs_vecnorm_destroy": (C.c_int, [_vp]),
        "brs_vecnorm_last_error": (C.c_char_p, [_vp]),
        "brs_vecnorm_reset": (C.c_int, [_vp, _vp, _i32, _vp, _vp]),
        "brs_vecnorm_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
        "brs_vecnorm_normalize_obs": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
        "brs_vecnorm_normalize_reward": (C.c_int, [_vp, _i32, _vp, _vp, _vp]),
        "brs_vecnorm_get_stats": (C.c_int, [_vp, C.POINTER(BrsVecnormStats), _vp]),
        "brs_vecnorm_set_stats": (C.c_int, [_vp, C.POINTER(BrsVecnormStats), _vp]),
        "brs_vecnorm_get_returns": (C.c_int, [_vp, _dp, _vp]),
        "brs_replay_sample_vecnorm": (C.c_int, [_vp, C.POINTER(BrsReplayStorage), _i32, _i32, _i32, _i32, C.c_uint64, C.c_uint32,
                                                C.POINTER(BrsReplayStorage), _vp, _vp]),
    },
    "brs_render.h": {
        "brs_render_default_camera": (None, [C.POINTER(BrsCamera)]),
        "brs_render": (C.c_int, [_i32, _i32, _i32, _vp, C.POINTER(BrsCamera), _vp, _vp, _vp, _vp]),
        "brs_render_last_error": (C.c_char_p, []),
    },
    "brs_qpolicy.h": {
        "brs_qpolicy_create": (C.c_int, [_i32, C.POINTER(_vp)]),
        "brs_qpolicy_destroy": (C.c_int, [_vp]),
        "brs_qpolicy_last_error": (C.c_char_p, [_vp]),
        "brs_qpolicy_quantize_multiplier": (C.c_int, [C.c_double, _i32p, _i32p]),
        "brs_qpolicy_set_model": (C.c_int, [_vp, C.POINTER(BrsQModel)]),
        "brs_qpolicy_act": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
        "brs_qpolicy_actor_create": (C.c_int, [_i32, C.POINTER(_vp)]),
        "brs_qpolicy_actor_destroy": (C.c_int, [_vp]),
        "brs_qpolicy_actor_last_error": (C.c_char_p, [_vp]),
        "brs_qpolicy_actor_set_model": (C.c_int, [_vp, C.POINTER(BrsQActorModel)]),
        "brs_qpolicy_actor_act": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _vp]),
        "brs_qpolicy_actor_create_arch": (C.c_int, [_i32, _i32, C.POINTER(_vp)]),
        "brs_qpolicy_actor_check_model": (C.c_int, [_i32, C.POINTER(BrsQActorModel)]),
    },
}
SYMBOLS = list(SIGNATURES["brs.h"]) + list(SIGNATURES["brs_policy.h"])
RENDER_SYMBOLS = list(SIGNATURES["brs_render.h"])
QPOLICY_SYMBOLS = list(SIGNATURES["brs_qpolicy.h"])

_lib = None


def lib():
    """load the shared library (raises if it has not been built: the product has no fallback path)"""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("BRS_HIP_LIB") or LIB_PATH  # BRS_HIP_LIB: another BUILD of the same HIP library (same-box A/B runs)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = C.CDLL(path)
    for functions in SIGNATURES.values():
        for name, (restype, argtypes) in functions.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def build_id():
    """id of the loaded library's build (include/brs.h: brs_build_id)"""
    return lib().brs_build_id().decode()
