"""Build + load the CPU harness of the wavefront map's per-ray rule (tests/native/wavemap_harness.cpp), as
foot_harness.py builds foot_harness.cpp.  TEST INFRASTRUCTURE ONLY."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "wavemap_harness.cpp")
OUT = os.path.join(HERE, "native", "_build", "libwavemap_harness.so")
DEPS = [SRC, os.path.join(HERE, "..", "ray_trace_pb_amd", "csrc", "rtpb_wavemap.h"),
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
        P = ctypes.c_void_p
        _lib.wavemap_harness_map.argtypes = [P, ctypes.c_int64, ctypes.c_int64, P, P, ctypes.c_int32, ctypes.c_int32,
                                             ctypes.c_int32, ctypes.c_double, P, P, P, P, P]
        _lib.wavemap_harness_map.restype = ctypes.c_int
        _lib.wavemap_harness_bound.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_int64]
        _lib.wavemap_harness_bound.restype = ctypes.c_int
    return _lib


def wavemap(plane, group_size, refs, windows, bins, q_bits, w_lim):
    """(count (G, ny, nx) int32, sum (G, ny, nx) int64, outside (G,), clipped (G,), farthest (G, 2)) of an (N, 8)
    float64 plane by wave_ray / wavemap_ray on the CPU."""
    plane = np.ascontiguousarray(plane, dtype=np.float64)
    refs = np.ascontiguousarray(refs, dtype=np.float64).reshape(-1, 8)
    windows = np.ascontiguousarray(windows, dtype=np.float64).reshape(-1, 4)
    nx, ny = bins
    G = plane.shape[0] // group_size
    assert plane.shape == (G * group_size, 8) and refs.shape[0] == G and windows.shape[0] == G
    count = np.empty((G, ny, nx), dtype=np.int32)
    total = np.empty((G, ny, nx), dtype=np.int64)
    outside, clipped = np.empty(G, dtype=np.int32), np.empty(G, dtype=np.int32)
    farthest = np.empty((G, 2))
    assert harness().wavemap_harness_map(plane.ctypes.data, group_size, G, refs.ctypes.data, windows.ctypes.data, nx,
                                         ny, q_bits, w_lim, count.ctypes.data, total.ctypes.data, outside.ctypes.data,
                                         clipped.ctypes.data, farthest.ctypes.data) == 0
    return count, total, outside, clipped, farthest
