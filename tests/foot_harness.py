"""Load the CPU harness of the footprint statistics' per-ray term (tests/native/foot_harness.cpp; built by
native_harness.load).  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import native_harness


def harness():
    lib = native_harness.load("foot_harness")
    lib.foot_harness_stats.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                       ctypes.c_void_p, ctypes.c_void_p]
    lib.foot_harness_stats.restype = ctypes.c_int
    lib.foot_harness_col.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_double]
    lib.foot_harness_col.restype = ctypes.c_double
    return lib


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
