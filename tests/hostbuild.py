"""How the off-policy case modules (offpolicy_cases, ddpg_learner_cases, td3_cases, sac_cases, sac_arch_cases) build a host mirror of the
kernel source with g++ and hand numpy arrays to it.  Each module keeps the ctypes signatures of its own library."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = ["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", os.path.join(ROOT, "balance_robot_mujoco_rl_amd", "csrc")]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def compile_host(directory, lib_name, source, defines=()):
    """g++ -> `lib_name` in `directory` from `source` with -D<define> for every entry of `defines`; -> the loaded library"""
    so = os.path.join(str(directory), lib_name)
    subprocess.check_call(GXX + [f"-D{d}" for d in defines] + ["-fPIC", "-shared", "-o", so, source])
    return C.CDLL(so)
