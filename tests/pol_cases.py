"""The transmission tests' cases (the footprint tests' seven and c5_far) for the polarisation statistics, and the
restatement's answer for each (not a test module): the polariser axis of every case, pol_oracle's columns on the
oracle's histories with the oracle's own indices, the collimated beams of two of the cases, and the loader of the CPU
harness of csrc/rtpb_pol.h (tests/native/pol_harness.cpp).  tests/test_polarisation_host.py checks on the CPU what
tests/test_gpu_polarisation.py assumes about them.  TEST INFRASTRUCTURE ONLY."""
import ctypes
import functools

import numpy as np

from ray_trace_pb_amd import polarisation as P
from oracle import rt_numpy as O
import ray_trace_pb_amd.raytrace as rt
import native_harness
import pol_oracle as PO
import sweep_cases as SC
import trans_cases as TC
from foot_cases import CASES as FOOT_CASES, NT, NPH, case_histories

CASES = FOOT_CASES + ("c5_far",)
Q_BITS = 24
# the polariser axis of every case (the analyser is the polariser unless a test says otherwise): with it c2, stress,
# c4, c5_wide, tir and xz have valid == pass everywhere, tangent has rays that pass without a state, c5_far is empty
# (tests/test_polarisation_host.py checks each statement with the oracle alone)
POLARISER = {name: (1.0, 0.0, 0.0) for name in CASES}
# a second pair: a tilted polariser and an analyser that is not the polariser
PAIR2 = ((0.3, 1.0, 0.2), (1.0, -0.5, 0.1))


def harness():
    lib = native_harness.load("pol_harness", headers=("rtpb_pol.h", "rtpb_trans.h", "rtpb_foot.h", "rtpb_math.h"))
    V = ctypes.c_void_p
    lib.pol_harness_stats.argtypes = [V, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, V, V, V, V, ctypes.c_int32,
                                      V, V]
    lib.pol_harness_stats.restype = ctypes.c_int
    lib.pol_harness_amplitudes.argtypes = [V, V, V, V, ctypes.c_int64, V]
    lib.pol_harness_amplitudes.restype = None
    lib.pol_harness_launch.argtypes = [V, V, ctypes.c_int64, V]
    lib.pol_harness_launch.restype = None
    lib.pol_harness_surface.argtypes = [V, V, V, V, ctypes.c_double, ctypes.c_double, ctypes.c_int64, V]
    lib.pol_harness_surface.restype = None
    return lib


def _f64(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]


def harness_stats(history, group_size, media, coatings, u, w_an, q_bits=Q_BITS):
    """(states, columns) = ((S, N, 2, 3), (n_groups, S, 6)) by pol_launch / pol_surface / pol_term on the CPU; u and
    w_an are unit vectors."""
    history, media, coatings, u, w_an = _f64(history, media, coatings, u, w_an)
    S, N = (history.shape[0] - 1) // 2, history.shape[1]
    G = N // group_size
    assert N == G * group_size and media.shape == (G, S + 1) and coatings.shape == (S, 2)
    states, out = np.empty((S, N, 2, 3)), np.empty((G, S, 6))
    assert harness().pol_harness_stats(history.ctypes.data, group_size, G, S, media.ctypes.data, coatings.ctypes.data,
                                       u.ctypes.data, w_an.ctypes.data, q_bits, states.ctypes.data,
                                       out.ctypes.data) == 0
    return states, out


def harness_amplitudes(n1, n2, dA, dB):
    """(ts, tp) of pol_amplitudes (FRESNEL) for rows of indices (n,) and directions (n, 3)."""
    dA, dB = _f64(np.atleast_2d(dA), np.atleast_2d(dB))
    n = dA.shape[0]
    n1, n2 = _f64(np.broadcast_to(np.asarray(n1, dtype=np.float64), (n,)),
                  np.broadcast_to(np.asarray(n2, dtype=np.float64), (n,)))
    out = np.empty((n, 2))
    harness().pol_harness_amplitudes(n1.ctypes.data, n2.ctypes.data, dA.ctypes.data, dB.ctypes.data, n,
                                     out.ctypes.data)
    return out[:, 0], out[:, 1]


def harness_launch(d, u):
    """(n, 2, 3): pol_launch of directions (n, 3) behind the unit polariser u."""
    d, u = _f64(np.atleast_2d(d), u)
    out = np.empty((d.shape[0], 2, 3))
    harness().pol_harness_launch(d.ctypes.data, u.ctypes.data, d.shape[0], out.ctypes.data)
    return out


def harness_surface(states, dA, dB, n1, n2, mode, value):
    """(n, 2, 3): one passing pol_surface step of the states (n, 2, 3) with the coating (mode, value)."""
    states, dA, dB = _f64(np.array(states, dtype=np.float64), np.atleast_2d(dA), np.atleast_2d(dB))
    n = dA.shape[0]
    n1, n2 = _f64(np.broadcast_to(np.asarray(n1, dtype=np.float64), (n,)),
                  np.broadcast_to(np.asarray(n2, dtype=np.float64), (n,)))
    assert states.shape == (n, 2, 3) and dB.shape == (n, 3)
    harness().pol_harness_surface(dA.ctypes.data, dB.ctypes.data, n1.ctypes.data, n2.ctypes.data, mode, value, n,
                                  states.ctypes.data)
    return states


def axes(name, polariser=None, analyser=None):
    """The unit polariser and analyser axes of a case, as the Python layer normalises them."""
    u = PO.unit(POLARISER[name] if polariser is None else polariser)
    return u, u if analyser is None else PO.unit(analyser)


@functools.lru_cache(maxsize=None)
def case_columns(name, nt=NT, nph=NPH, theta=None, q_bits=Q_BITS, coatings=None, polariser=None, analyser=None):
    """The restatement's (n_fields, n_wavelengths, S, 6) of a case on the oracle's histories, with the default
    coatings or the given ones (a tuple of (mode, value) pairs), the case's polariser or the given axes (tuples)."""
    c = SC.case(name)
    coat = P.default_coatings(c.system) if coatings is None else np.array(coatings)
    media = TC.group_media(c)
    u, w = axes(name, polariser, analyser)
    out = np.stack([PO.pol_columns(h, media[g], coat, u, w, q_bits)[0]
                    for g, h in enumerate(case_histories(name, nt, nph, theta))])
    out = out.reshape(len(c.fields), len(c.wls), len(c.S), 6)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def beam_case(name):
    """The transmission tests' beams (trans_cases.beam_case: two field normals x two wavelengths of 43 x 7 rays) and
    the restatement's columns on the oracle's trace of get_collimated_rays' beams."""
    args, pt, _ = TC.beam_case(name)
    c = SC.case(name)
    normals, wls, dmax = args[3], args[4], args[5]
    coat = P.default_coatings(c.system)
    media = TC.oracle_media(c, wls)
    u, w = axes(name)
    cols = np.stack([PO.pol_columns(O.ray_trace(c.S, c.M, rt.get_collimated_rays(pt, dmax, NT, wl, NPH, 0.3, n)),
                                    media[k], coat, u, w, Q_BITS)[0]
                     for n in normals for k, wl in enumerate(wls)]).reshape(2, 2, len(c.S), 6)
    return args, pt, cols
