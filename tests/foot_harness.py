"""Build + load the CPU harness of the footprint statistics' per-ray term (tests/native/foot_harness.cpp), as
native_harness.py builds math_harness.cpp.  TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "foot_harness.cpp")
OUT = os.path.join(HERE, "native", "_build", "libfoot_harness.so")
DEPS = [SRC, os.path.join(HERE, "..", "ray_trace_pb_amd", "csrc", "rtpb_foot.h"),
        os.path.join(HERE, "..", "ray_trace_pb_amd", "csrc", "rtpb_math.h"),
        os.path.join(HERE, "..", "include", "rtpb.h")]

_lib = None


def harness():
    global _lib
    if _lib is None:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        import fcntl
        with open(OUT + ".lock", "w") as lk:        # several test processes may race to (re)build
            fcntl.flock(lk, fcntl.LOCK_EX)
            if not os.path.exists(OUT) or any(os.path.getmtime(OUT) < os.path.getmtime(d) for d in DEPS):
                tmp = f"{OUT}.{os.getpid()}.tmp"
                subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                                "-I", os.path.join(HERE, "..", "include"), "-o", tmp, SRC], check=True)
                os.replace(tmp, OUT)
        _lib = ctypes.CDLL(OUT)
        _lib.foot_harness_stats.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                            ctypes.c_void_p, ctypes.c_void_p]
        _lib.foot_harness_stats.restype = ctypes.c_int
        _lib.foot_harness_col.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_double]
        _lib.foot_harness_col.restype = ctypes.c_double
    return _lib


def foot_stats(history, group_size, frames):
    """(n_groups, S, 8) from a (1 + 2 S, N, 8) float64 history and (S, 9) frames, by foot_ray / foot_merge on the CPU."""
    history = np.ascontiguousarray(history, dtype=np.float64)
    frames = np.ascontiguousarray(frames, dtype=np.float64)
    S = (history.shape[0] - 1) // 2
    G = history.shape[1] // group_size
    assert history.shape[1] == G * group_size and frames.shape == (S, 9)
    out = np.empty((G, S, 8))
    assert harness().foot_harness_stats(history.ctypes.data, group_size, G, S, frames.ctypes.data, out.ctypes.data) == 0
    return out
