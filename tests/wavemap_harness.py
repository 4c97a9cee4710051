"""Load the CPU harness of the wavefront map's per-ray rule (tests/native/wavemap_harness.cpp; built by
native_harness.load).  TEST INFRASTRUCTURE ONLY."""
import ctypes

import numpy as np

import native_harness


def harness():
    lib = native_harness.load("wavemap_harness")
    P = ctypes.c_void_p
    lib.wavemap_harness_map.argtypes = [P, ctypes.c_int64, ctypes.c_int64, P, P, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_int32, ctypes.c_double, P, P, P, P, P]
    lib.wavemap_harness_map.restype = ctypes.c_int
    lib.wavemap_harness_bound.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_int64]
    lib.wavemap_harness_bound.restype = ctypes.c_int
    return lib


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
