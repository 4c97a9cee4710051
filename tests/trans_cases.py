"""The footprint tests' cases (tests/foot_cases.py) for the transmission statistics, and the restatement's answer for
each (not a test module): the media from the oracle's own materials, trans_oracle's columns on the oracle's
histories, the collimated beams of two of the cases, and the loader of the CPU harness of csrc/rtpb_trans.h
(tests/native/trans_harness.cpp).  tests/test_transmission_host.py checks on the CPU what
tests/test_gpu_transmission.py assumes about them.  TEST INFRASTRUCTURE ONLY."""
import ctypes
import functools

import numpy as np

from ray_trace_pb_amd import transmission as T
from oracle import rt_numpy as O
import ray_trace_pb_amd.raytrace as rt
import beam_cases as BC
import native_harness
import sweep_cases as SC
import trans_oracle as TO
from foot_cases import CASES as FOOT_CASES, NT, NPH, case_histories

# none of the footprint tests' seven cases has a (group, surface) that no ray passes: c5_far, whose every row dies at
# the first sphere, is the empty cell (tests/test_transmission_host.py checks both statements)
CASES = FOOT_CASES + ("c5_far",)
Q_BITS = 24


def harness():
    lib = native_harness.load("trans_harness", headers=("rtpb_trans.h", "rtpb_math.h"))
    P = ctypes.c_void_p
    lib.trans_harness_stats.argtypes = [P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, P, P, ctypes.c_int32, P, P,
                                        P]
    lib.trans_harness_stats.restype = ctypes.c_int
    lib.trans_harness_fresnel.argtypes = [P, P, P, P, ctypes.c_int64, P, P]
    lib.trans_harness_fresnel.restype = None
    lib.trans_harness_col.argtypes = [ctypes.c_int32, ctypes.c_double, ctypes.c_double]
    lib.trans_harness_col.restype = ctypes.c_double
    lib.trans_harness_max_q_bits.argtypes = [ctypes.c_int64]
    lib.trans_harness_max_q_bits.restype = ctypes.c_int32
    return lib


def harness_stats(history, group_size, media, coatings, q_bits=Q_BITS):
    """(t, cum, columns) = ((S, N), (S, N), (n_groups, S, 5)) by trans_ray / trans_merge on the CPU."""
    history = np.ascontiguousarray(history, dtype=np.float64)
    media = np.ascontiguousarray(media, dtype=np.float64)
    coatings = np.ascontiguousarray(coatings, dtype=np.float64)
    S, N = (history.shape[0] - 1) // 2, history.shape[1]
    G = N // group_size
    assert N == G * group_size and media.shape == (G, S + 1) and coatings.shape == (S, 2)
    t, cum, out = np.empty((S, N)), np.empty((S, N)), np.empty((G, S, 5))
    assert harness().trans_harness_stats(history.ctypes.data, group_size, G, S, media.ctypes.data,
                                         coatings.ctypes.data, q_bits, t.ctypes.data, cum.ctypes.data,
                                         out.ctypes.data) == 0
    return t, cum, out


def harness_fresnel(n1, n2, dA, dB):
    """(t, rs, rp) of trans_fresnel / trans_ratios for rows of indices (n,) and directions (n, 3)."""
    dA, dB = (np.ascontiguousarray(np.atleast_2d(d), dtype=np.float64) for d in (dA, dB))
    n = dA.shape[0]
    n1, n2 = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for v in (n1, n2))
    assert dA.shape == dB.shape == (n, 3)
    t, r = np.empty(n), np.empty((n, 2))
    harness().trans_harness_fresnel(n1.ctypes.data, n2.ctypes.data, dA.ctypes.data, dB.ctypes.data, n, t.ctypes.data,
                                    r.ctypes.data)
    return t, r[:, 0], r[:, 1]


def oracle_media(c, wls):
    """(len(wls), S + 1): n of the case's materials at each wavelength, from the oracle's own dispersion formulas."""
    return np.array([[float(O.refractive_index(m, np.float64(w))) for m in c.M] for w in wls])


def group_media(c, wls=None):
    """(n_fields * n_wavelengths, S + 1), group = field * nw + wavelength."""
    return np.tile(oracle_media(c, c.wls if wls is None else wls), (len(c.fields), 1))


@functools.lru_cache(maxsize=None)
def case_columns(name, nt=NT, nph=NPH, theta=None, q_bits=Q_BITS, coatings=None):
    """The restatement's (n_fields, n_wavelengths, S, 5) of a case on the oracle's histories, with the default
    coatings or the given ones (a tuple of (mode, value) pairs)."""
    c = SC.case(name)
    coat = T.default_coatings(c.system) if coatings is None else np.array(coatings)
    media = group_media(c)
    out = np.stack([TO.trans_columns(h, media[g], coat, q_bits)[0]
                    for g, h in enumerate(case_histories(name, nt, nph, theta))])
    out = out.reshape(len(c.fields), len(c.wls), len(c.S), 5)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def beam_case(name):
    """Two field normals x two wavelengths of 43 x 7 = 301 rays on a named sweep case's system (the footprint tests'
    beams), and the restatement's columns on the oracle's trace of get_collimated_rays' beams."""
    c = SC.case(name)
    normals = np.array([[0.0, 0.0, 1.0], BC.unit([0.01, 0.0, 1.0])])
    pt, dmax = ([0.0, 0.0, -5.0], 30.0) if name == "c2" else ([0.0, 0.0, -1.0], 2.0)
    wls = list(c.wls[:2])
    coat = T.default_coatings(c.system)
    media = oracle_media(c, wls)
    cols = np.stack([TO.trans_columns(O.ray_trace(c.S, c.M, rt.get_collimated_rays(pt, dmax, NT, w, NPH, 0.3, n)),
                                      media[k], coat, Q_BITS)[0]
                     for n in normals for k, w in enumerate(wls)]).reshape(2, 2, len(c.S), 5)
    return (c.system, c.m0, c.m1, normals, wls, dmax, NT, NPH, 0.3), pt, cols


def assert_same_summary(got, exp):
    """Two summarize_transmission summaries with the same entries: types, shapes and values, NaN in the same places."""
    assert sorted(got) == sorted(exp)
    for k, e in exp.items():
        assert got[k].dtype == e.dtype and got[k].shape == e.shape, k
        assert np.array_equal(got[k], e, equal_nan=e.dtype.kind == "f"), k
