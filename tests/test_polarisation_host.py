"""Polarisation statistics on the host: the rule of csrc/rtpb_pol.h run on the CPU (tests/native/pol_harness.cpp) against
the NumPy restatement (tests/pol_oracle.py), the physics of the restatement on the named cases and on hand-made rows,
analysis-level summaries and refusals (no GPU is touched), the argument checks of the four C entry points, and what
tests/test_gpu_polarisation.py assumes about the named cases, checked with the oracle alone."""
import inspect

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
from ray_trace_pb_amd import polarisation as P
from ray_trace_pb_amd import transmission as T
import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
import pol_cases as PC
import pol_oracle as PO
import sweep_cases as SC
import trans_cases as TC
import trans_oracle as TO
from flat_plans import flat_plan
from foot_cases import NT, NPH, case_histories

PER = NT * NPH


def same_bits(a, b):
    """NaN in the same places and the same bits elsewhere (zero signs included)."""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and \
        np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def whole_case(name):
    """(history of all groups, media, default coatings) of a case at the tests' fan shape."""
    c = SC.case(name)
    return np.concatenate(case_histories(name), axis=1), TC.group_media(c), P.default_coatings(c.system)


def refraction(n1, n2, theta1, phi=0.0):
    """(dA, dB): float64 unit directions of refractions at the plane z = 0, incidence angles theta1 in the plane of
    azimuth phi."""
    th = np.atleast_1d(np.asarray(theta1, dtype=np.float64))
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), th.shape)
    s1 = np.sin(th)
    s2 = n1 * s1 / n2
    dA = np.stack((s1 * np.cos(phi), s1 * np.sin(phi), np.cos(th)), axis=-1)
    dB = np.stack((s2 * np.cos(phi), s2 * np.sin(phi), np.sqrt(1 - s2 * s2)), axis=-1)
    return dA, dB


# ---- the rule against the restatement ----

@pytest.mark.parametrize("name", PC.CASES)
def test_pol_rule_on_the_host_matches_the_restatement(name):
    """pol_launch / pol_surface / pol_term / pol_merge compiled for the CPU, applied to the oracle's histories of the
    case's fans with the oracle's media, give the restatement's states (NaN pattern and zero signs included) and
    columns bit for bit -- with the default coatings and the case's polariser, with a CONSTANT 0.25, a MIRROR 0.81 and
    q_bits at both ends, and with the second axis pair."""
    c = SC.case(name)
    hist, media, coat = whole_case(name)
    u, w = PC.axes(name)
    states, cols = PC.harness_stats(hist, PER, media, coat, u, w)
    assert same_bits(states, PO.pol_rays(hist, media, coat, u, w, PER)[0])
    exp = PO.pol_columns(hist, media, coat, u, w, PC.Q_BITS, PER)
    assert cols.shape == exp.shape == (len(c.fields) * len(c.wls), len(c.S), 6)
    assert np.array_equal(cols, exp)
    assert np.array_equal(exp.reshape(PC.case_columns(name).shape), PC.case_columns(name))
    coat2 = coat.copy()
    coat2[0] = (PO.CONSTANT, 0.25)
    coat2[-1] = (PO.MIRROR, 0.81)
    u2, w2 = PC.axes(name, *PC.PAIR2)
    for q in (1, 40):
        states, cols = PC.harness_stats(hist, PER, media, coat2, u2, w2, q)
        assert same_bits(states, PO.pol_rays(hist, media, coat2, u2, w2, PER)[0])
        assert np.array_equal(cols, PO.pol_columns(hist, media, coat2, u2, w2, q, PER))


def test_edge_rows():
    """An empty set is six zeros; rows with NaN or infinite positions in A or B do not pass and lose their state for
    good; a ray along the polariser has no state but passes; an analyser along the outgoing ray makes no ray valid."""
    h = np.zeros((5, 5, 8))
    h[:, :, 5] = 1.0
    h[1, 1, 0] = np.nan
    h[2, 2, 1] = np.inf
    h[:, 3, 3:6] = (1.0, 0.0, 0.0)
    coat = np.array([[1.0, 0.0], [1.0, 0.0]])
    media = [[1.0, 1.5, 1.0]]
    x, z = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    states, cols = PC.harness_stats(h, 5, media, coat, x, x)
    assert np.isnan(states[:, 1:4]).all() and not np.isnan(states[:, [0, 4]]).any()
    assert cols[0, :, 0].tolist() == [3.0, 5.0] and cols[0, :, 1].tolist() == [2.0, 2.0]
    assert np.array_equal(cols, PO.pol_columns(h, media, coat, x, x, PC.Q_BITS, 5))
    q96 = np.rint(0.96 * 2.0 ** 24)
    assert cols[0, 0].tolist() == [3.0, 2.0, 2 * q96, 2 * q96, 0.0, 2 * q96]
    y = np.array([0.0, 1.0, 0.0])
    _, cols = PC.harness_stats(h, 5, media, coat, y, z)
    assert cols[0, :, 1].tolist() == [1.0, 1.0]         # only the ray along x has an x = b x w_an
    assert np.array_equal(cols, PO.pol_columns(h, media, coat, y, z, PC.Q_BITS, 5))
    empty = np.full((3, 4, 8), np.nan)
    assert not PC.harness_stats(empty, 4, [[1.0, 1.5]], coat[:1], x, x)[1].any()
    assert not PO.pol_columns(empty, [[1.0, 1.5]], coat[:1], x, x, PC.Q_BITS, 4).any()


# ---- what the GPU tests assume about the cases, from the oracle alone ----

@pytest.mark.parametrize("name", ["c2", "stress", "c4", "c5_wide", "tir", "xz"])
def test_no_passing_ray_of_these_cases_loses_its_state(name):
    cols = PC.case_columns(name)
    assert np.array_equal(cols[..., 0], cols[..., 1]) and cols[..., 1].max() > 0
    assert (cols[..., 2:4] <= cols[..., 1:2] * 2.0 ** PC.Q_BITS).all() and (cols[..., 4:6] <= cols[..., 2:4]).all()
    assert PC.POLARISER[name] == (1.0, 0.0, 0.0)


def test_tangent_has_rays_that_pass_without_a_state():
    cols = PC.case_columns("tangent")
    assert ((cols[..., 1] > 0) & (cols[..., 1] < cols[..., 0])).any()
    assert PC.POLARISER["tangent"] == (1.0, 0.0, 0.0)


def test_c5_far_is_the_empty_cell():
    assert PC.CASES == TC.CASES
    assert not [n for n in PC.CASES[:-1] if (PC.case_columns(n)[..., 0] == 0).any()]
    far = PC.case_columns("c5_far")
    assert not far.any()
    s = P.summarize_polarisation(far, PER, PC.Q_BITS)
    assert (s["throughput"] == 0).all() and np.isnan(s["transmittance"]).all() and np.isnan(s["cross_leakage"]).all()
    assert np.isnan(s["diattenuation"]).all()


def test_c4_leaks_between_crossed_polarisers_and_tir_is_diattenuating():
    """The figures the feature exists for: the PerfectLens relays of c4 turn an x-polarised pupil (cross-polar leakage
    of a few per cent), the prism's throughput depends on the input state."""
    c4 = P.summarize_polarisation(PC.case_columns("c4"), PER, PC.Q_BITS)
    assert 0.02 < c4["cross_leakage"][0, 0, -1, 0] < 0.08
    tir = P.summarize_polarisation(PC.case_columns("tir"), PER, PC.Q_BITS)
    assert (np.abs(tir["diattenuation"][..., -1]) > 0.05).any()


# ---- the physics, on the restatement ----

@pytest.mark.parametrize("name", PC.CASES[:-1])
def test_states_stay_perpendicular_to_the_ray(name):
    """|E_i . b| <= 1e-12 after every surface (measured 5.2e-15 over up to 14 surfaces: a sanity check on the
    accumulated steps, not a parity check)."""
    hist, media, coat = whole_case(name)
    states = PO.pol_rays(hist, media, coat, *PC.axes(name), PER)[0]
    worst = 0.0
    for s in range(states.shape[0]):
        b = hist[2 * s + 2][:, 3:6]
        for i in range(2):
            d = np.abs(PO.dot(states[s][:, i], b))
            worst = max(worst, np.max(d[~np.isnan(d)], initial=0.0))
    print(f"{name}: max |E . b| = {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", PC.CASES[:-1])
def test_mean_energy_at_the_first_refraction_is_the_unpolarised_transmittance(name):
    """At the first surface that refracts (FRESNEL between two media; every surface before it is lossless) the mean of
    |E1|^2 and |E2|^2 equals trans_oracle's t within 1e-14 for every ray with a state (measured 6.7e-16)."""
    c = SC.case(name)
    hist, media, coat = whole_case(name)
    first = next(s for s in range(len(c.S)) if coat[s, 0] == PO.FRESNEL and (media[:, s] != media[:, s + 1]).all())
    assert all(coat[s].tolist() in ([PO.CONSTANT, 1.0], [PO.MIRROR, 1.0]) or (media[:, s] == media[:, s + 1]).all()
               for s in range(first))
    states, _, _, valid = PO.pol_rays(hist, media, coat, *PC.axes(name), PER)
    t = TO.trans_rays(hist, media, T.default_coatings(c.system), PER)[0][first]
    e = states[first]
    mean = 0.5 * (PO.dot(e[:, 0], e[:, 0]) + PO.dot(e[:, 1], e[:, 1]))
    ok = valid[first]
    assert ok.sum() > 100
    err = np.abs(mean[ok] - t[ok]).max()
    print(f"{name}: surface {first}, max |mean energy - t| = {err:.3e}")
    assert err <= 1e-14


def test_on_axis_c2_has_equal_throughput_for_both_states():
    """The on-axis field of c2, an axially symmetric system: columns 2 and 3 agree within the quantisation.

    On a ray at polar angle theta and azimuth phi the launch puts (E1 . s)^2 = sin^2 phi / D and (E1 . p)^2 = cos^2
    theta cos^2 phi / D on the s and p directions, D = 1 - sin^2 theta cos^2 phi, and E2 has the two exchanged; the
    rays stay meridional, so s and p never mix, and column 2 - column 3 = 2^q sum (Ts - Tp)(theta) (sin^2 phi - cos^2
    theta cos^2 phi) / D with Ts, Tp the products of the squared amplitudes.  Over the fan's 14 evenly spaced azimuths
    sin^2 phi - cos^2 phi sums to zero; what is left is of order sin^2 theta (Ts - Tp), and Ts - Tp itself of order
    sin^2 theta: theta^4 in all.  So the statement is one about paraxial fans, and it is checked on one: half-angle
    1e-4, where theta^4 2^24 301 < 1e-6 of a unit.  The roundings: each ray's two terms are rounded to a unit, half a
    unit each at the most, so |column 2 - column 3| <= valid + 1.  The case's own fan (half-angle 0.05) is printed:
    its difference is that theta^4 term, some 500 units of 2^-24 in 301 rays (1e-7 of the throughput)."""
    tiny = PC.case_columns("c2", theta=1e-4)
    assert SC.case("c2").fields[0][:2].tolist() == [0.0, 0.0] and (tiny[0, :, :, 1] == PER).all()
    diff = np.abs(tiny[0, :, :, 2] - tiny[0, :, :, 3])
    print("half-angle 1e-4:", diff.max(), "; the case's fan:",
          np.abs(PC.case_columns("c2")[0, :, :, 2] - PC.case_columns("c2")[0, :, :, 3]).max())
    assert (diff <= tiny[0, :, :, 1] + 1).all()
    s = P.summarize_polarisation(PC.case_columns("c2"), PER, PC.Q_BITS)
    assert np.allclose(s["throughput"][0, :, -1, 0], s["throughput"][0, :, -1, 1], rtol=0, atol=1e-6)
    assert ((s["throughput"][0, :, -1] > 0.8) & (s["throughput"][0, :, -1] < 0.9)).all()
    assert (np.abs(s["diattenuation"][1, :, -1]) > 5e-5).all()          # ... and the off-axis field is not


def test_brewster_angle_passes_p_whole():
    """Air -> 1.5 at atan(1.5) on a single flat: tp = 1 to 1e-15 and ts < 1."""
    dA, dB = refraction(1.0, 1.5, np.arctan(1.5))
    ts, tp = PC.harness_amplitudes(1.0, 1.5, dA, dB)
    assert abs(tp[0] - 1.0) <= 1e-15 and 0.9 < ts[0] < 0.93
    ets, etp = PO.amplitudes(1.0, 1.5, dA, dB)
    assert ts.tobytes() == ets.tobytes() and tp.tobytes() == etp.tobytes()
    # a state along s loses ts^2, a state in the plane of incidence nothing
    e = PC.harness_launch(dA, [0.0, 1.0, 0.0])
    out = PC.harness_surface(e, dA, dB, 1.0, 1.5, PO.FRESNEL, 0.0)
    assert abs(PO.dot(out[:, 0], out[:, 0])[0] - ts[0] ** 2) <= 1e-15
    assert abs(PO.dot(out[:, 1], out[:, 1])[0] - 1.0) <= 1e-15


def test_mirror_at_normal_incidence_negates_the_state_exactly():
    a, b = np.array([[0.0, 0.0, 1.0]]), np.array([[0.0, 0.0, -1.0]])
    e = PC.harness_launch(a, [1.0, 0.0, 0.0])
    assert e.tolist() == [[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]]
    out = PC.harness_surface(e, a, b, 1.0, 1.0, PO.MIRROR, 1.0)
    assert np.array_equal(out, -e)
    assert np.array_equal(PO.mirror(e, a, b, 1.0), -e)
    half = PC.harness_surface(e, a, b, 1.0, 1.0, PO.MIRROR, 0.25)
    assert np.array_equal(half, -0.5 * e)
    # nothing reflected: no state
    assert np.isnan(PC.harness_surface(e, a, a, 1.0, 1.0, PO.MIRROR, 1.0)).all()


def test_reversal_gives_the_same_amplitudes_bitwise():
    """(n1, a) <-> (n2, b): both ratios change sign, so ts and tp are the same bits."""
    rng = np.random.default_rng(11)
    for n1, n2 in [(1.0, 1.5), (1.5, 1.0), (1.0, 1.33), (1.52, 1.0003), (1.7, 1.5), (1.0, 2.4)]:
        crit = np.arcsin(min(1.0, n2 / n1))
        dA, dB = refraction(n1, n2, rng.uniform(0, 0.999 * crit, 2000), rng.uniform(0, 2 * np.pi, 2000))
        ts, tp = PC.harness_amplitudes(n1, n2, dA, dB)
        ts2, tp2 = PC.harness_amplitudes(n2, n1, dB, dA)
        assert ts.tobytes() == ts2.tobytes() and tp.tobytes() == tp2.tobytes()
        assert ((ts > 0) & (ts <= 1) & (tp > 0) & (tp <= 1)).all() and (tp >= ts - 1e-15).all()
        ets, etp = PO.amplitudes(n1, n2, dA, dB)
        assert ts.tobytes() == ets.tobytes() and tp.tobytes() == etp.tobytes()
    same = PC.harness_amplitudes(1.4375, 1.4375, dA, dB)
    assert (same[0] == 1.0).all() and (same[1] == 1.0).all()


def test_launch():
    """E1 is the polariser projected across the ray, E2 = ray x E1, both unit; a ray along the polariser (or within
    2^-20 of it) has none."""
    rng = np.random.default_rng(12)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    u = PO.unit([0.3, 1.0, 0.2])
    e = PC.harness_launch(d, u)
    assert same_bits(e, PO.launch(d, u))
    assert np.abs(PO.dot(e[:, 0], d)).max() < 1e-14 and np.abs(PO.dot(e[:, 1], d)).max() < 1e-14
    assert np.abs(PO.dot(e[:, 0], e[:, 0]) - 1).max() < 1e-14 and np.abs(PO.dot(e[:, 0], e[:, 1])).max() < 1e-14
    assert (PO.dot(e[:, 0], np.broadcast_to(u, d.shape)) > 0).all()
    along = np.array([[1.0, 0.0, 0.0], [1.0, 2.0 ** -21, 0.0], [1.0, 2.0 ** -19, 0.0], [np.nan, 0.0, 1.0]])
    got = PC.harness_launch(along, [1.0, 0.0, 0.0])
    assert np.isnan(got[[0, 1, 3]]).all() and not np.isnan(got[2]).any()


# ---- the C entry points' checks ----

def test_polarisation_entry_points_validate_without_a_gpu():
    """NULL pointers, non-positive sizes, a coating that is not finite, has a mode outside 0, 1, 2 or a value outside
    [0, 1], an axis that is not finite or is zero, a coating count that is not the plan's, q_bits outside 1 ... 40, a
    short workspace and anything float32 are RTPB_E_INVALID; more than 65535 groups, more than RTPB_MAX_SURFACES
    surfaces and a q_bits too large for the group RTPB_E_LIMIT -- all before any device work."""
    lib = C.lib()
    buf = np.zeros(4096)
    p = buf.ctypes.data
    per, G, tiles, S = 300, 2, 2, 3
    coat = np.tile([1.0, 0.0], (S, 1))
    coat[1] = (2.0, 0.5)
    x = np.array([1.0, 0.0, 0.0])

    def coatings(row, mode, value):
        bad = coat.copy()
        bad[row] = (mode, value)
        return bad

    bads = [coatings(2, np.inf, 0.0), coatings(0, 1.0, np.nan), coatings(1, 3.0, 0.5), coatings(1, 0.5, 0.5),
            coatings(0, 0.0, 1.5), coatings(2, 2.0, -0.1)]
    bad_axes = [np.zeros(3), np.array([1.0, np.nan, 0.0]), np.array([np.inf, 0.0, 0.0])]
    ok = dict(device=0, dtype=C.RTPB_F64, history=p, group_size=per, n_groups=G, nsurf=S, media=p,
              coatings=coat.ctypes.data, polariser=x.ctypes.data, analyser=x.ctypes.data, q_bits=24, workspace=p,
              workspace_len=G * tiles * S * 6, stats_out=p, stream=None)
    assert len(ok) == len(C.SIGNATURES["rtpb_polarisation_stats"][1]) == 15
    for bad in [dict(history=None), dict(media=None), dict(coatings=None), dict(polariser=None), dict(analyser=None),
                dict(workspace=None), dict(stats_out=None), dict(group_size=0), dict(n_groups=0), dict(n_groups=-1),
                dict(nsurf=0), dict(dtype=7), dict(q_bits=0), dict(q_bits=41)] + \
            [dict(coatings=b.ctypes.data) for b in bads] + [dict(polariser=b.ctypes.data) for b in bad_axes] + \
            [dict(analyser=b.ctypes.data) for b in bad_axes]:
        assert lib.rtpb_polarisation_stats(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"polarisation-stats" in lib.rtpb_last_error(), bad
    assert lib.rtpb_polarisation_stats(*dict(ok, dtype=C.RTPB_F32).values()) == C.RTPB_E_INVALID
    assert b"float64 histories only" in lib.rtpb_last_error()
    assert lib.rtpb_polarisation_stats(*dict(ok, workspace_len=G * tiles * S * 6 - 1).values()) == C.RTPB_E_INVALID
    assert b"workspace too small" in lib.rtpb_last_error() and b"* nsurf * 6 doubles" in lib.rtpb_last_error()
    assert lib.rtpb_polarisation_stats(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
    big = np.tile([1.0, 0.0], (64, 1))
    assert lib.rtpb_polarisation_stats(*dict(ok, nsurf=64, coatings=big.ctypes.data,
                                             workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
    assert lib.rtpb_polarisation_stats(*dict(ok, group_size=8193, q_bits=40,
                                             workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
    assert b"q_bits at most 39" in lib.rtpb_last_error()

    ray = dict(device=0, dtype=C.RTPB_F64, history=p, group_size=per, n_groups=G, nsurf=S, media=p,
               coatings=coat.ctypes.data, polariser=x.ctypes.data, out=p, stream=None)
    assert len(ray) == len(C.SIGNATURES["rtpb_ray_polarisation"][1]) == 11
    for bad in [dict(history=None), dict(media=None), dict(coatings=None), dict(polariser=None), dict(out=None),
                dict(group_size=0), dict(n_groups=0), dict(nsurf=0), dict(dtype=7), dict(dtype=C.RTPB_F32)] + \
            [dict(coatings=b.ctypes.data) for b in bads] + [dict(polariser=b.ctypes.data) for b in bad_axes]:
        assert lib.rtpb_ray_polarisation(*dict(ray, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"ray-polarisation" in lib.rtpb_last_error(), bad
    assert lib.rtpb_ray_polarisation(*dict(ray, n_groups=65536).values()) == C.RTPB_E_LIMIT
    assert lib.rtpb_ray_polarisation(*dict(ray, nsurf=64, coatings=big.ctypes.data).values()) == C.RTPB_E_LIMIT

    plan, plan32 = flat_plan(C.RTPB_F64), flat_plan(C.RTPB_F32)           # one surface
    one = np.array([[2.0, 0.9]])
    one_bads = [np.array([row]) for row in ([1.0, np.nan], [-np.inf, 0.0], [3.0, 0.0], [0.0, 1.0000001])]
    blocks = 1                                                              # 300 rays: two tiles, one block
    try:
        fan = dict(plan=plan, device=0, n_groups=G, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                   theta_cos_sin=p, phi_cos_sin=p, coatings=one.ctypes.data, n_coatings=1, polariser=x.ctypes.data,
                   analyser=x.ctypes.data, q_bits=24, workspace=p, workspace_len=G * blocks * 1 * 6, stats_out=p,
                   stream=None)
        beam = dict(plan=plan, device=0, n_groups=G, group_params=p, group_frames=p, n_disps=30, nphis=10, offsets=p,
                    phi_cos_sin=p, coatings=one.ctypes.data, n_coatings=1, polariser=x.ctypes.data,
                    analyser=x.ctypes.data, q_bits=24, workspace=p, workspace_len=G * blocks * 1 * 6, stats_out=p,
                    stream=None)
        for fn, ok, nulls in ((lib.rtpb_polarisation_sweep, fan, ("group_params", "center_ray", "ex", "ey",
                                                                   "theta_cos_sin", "phi_cos_sin")),
                              (lib.rtpb_polarisation_sweep_collimated, beam, ("group_params", "group_frames",
                                                                              "offsets", "phi_cos_sin"))):
            assert len(ok) == len(C.SIGNATURES[fn.__name__][1])
            assert fn(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
            assert b"plan is NULL" in lib.rtpb_last_error()
            first = "n_thetas" if "n_thetas" in ok else "n_disps"
            for bad in [{k: None} for k in nulls + ("coatings", "polariser", "analyser", "workspace", "stats_out")] + [
                    dict(n_groups=0), {first: 0}, dict(nphis=-3), dict(n_coatings=2), dict(n_coatings=0),
                    dict(q_bits=0), dict(q_bits=41)] + [dict(coatings=b.ctypes.data) for b in one_bads] + \
                    [dict(polariser=b.ctypes.data) for b in bad_axes] + \
                    [dict(analyser=b.ctypes.data) for b in bad_axes]:
                assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
                assert b"polarisation-sweep" in lib.rtpb_last_error(), bad
            assert fn(*dict(ok, workspace_len=G * blocks * 6 - 1).values()) == C.RTPB_E_INVALID
            assert b"workspace too small" in lib.rtpb_last_error() and b"* nsurf * 6 doubles" in lib.rtpb_last_error()
            assert fn(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
            assert fn(*dict(ok, **{first: 8193, "nphis": 1, "q_bits": 40, "workspace_len": 1 << 40}).values()) == \
                C.RTPB_E_LIMIT
            assert b"q_bits at most 39" in lib.rtpb_last_error()
            assert fn(*dict(ok, plan=plan32).values()) == C.RTPB_E_INVALID
            assert b"float64 plans only" in lib.rtpb_last_error()
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0 and lib.rtpb_plan_destroy(plan32) == 0
    assert C.lib().rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    assert len(P.POL_STAT_NAMES) == 6 == PO.NCOLS


# ---- the Python layer ----

def test_the_module_s_public_names_and_signatures():
    public = {n for n, f in inspect.getmembers(P, inspect.isfunction) if f.__module__ == P.__name__
              and not n.startswith("_")}
    assert public == {"polarisation_sweep", "collimated_polarisation_sweep", "polarisation_stats_raw",
                      "polarisation_stats", "summarize_polarisation", "ray_polarisation", "default_coatings"}
    assert P.T.system_media is T.system_media
    fan, trans = inspect.signature(P.polarisation_sweep), inspect.signature(T.transmission_sweep)
    assert [n for n in fan.parameters if n not in ("polariser", "analyser")] == list(trans.parameters)
    assert list(fan.parameters).index("polariser") == list(trans.parameters).index("coatings")
    assert fan.parameters["polariser"].default == (1, 0, 0) and fan.parameters["analyser"].default is None
    assert fan.parameters["q_bits"].default == 24
    beam, btrans = inspect.signature(P.collimated_polarisation_sweep), inspect.signature(
        T.collimated_transmission_sweep)
    assert [n for n in beam.parameters if n not in ("polariser", "analyser")] == list(btrans.parameters)


def test_default_coatings_give_a_plane_mirror_its_mode():
    lens = rt.PerfectLens(15, [0, 0, 10], [0, 0, 1], 0.8)
    system = rt.System([rt.FlatSurface([0, 0, 0], [0, 0, 1], 10.0), rt.SphericalSurface.get_on_axis(20.0, 5.0, 10.0),
                        lens, rt.PlaneMirror([0, 0, 30], [0, 0, 1], 10.0)],
                       [mat.Bk7(), mat.Vacuum(), mat.Vacuum()])
    assert P.default_coatings(system).tolist() == [[1.0, 0.0], [1.0, 0.0], [0.0, 1.0], [2.0, 1.0]]
    stress = SC.case("stress").system
    ours, theirs = P.default_coatings(stress), T.default_coatings(stress)
    mirrors = [type(s).__name__ == "PlaneMirror" for s in stress.surfaces]
    assert any(mirrors) and (ours[mirrors] == (2.0, 1.0)).all()
    assert np.array_equal(ours[~np.array(mirrors)], theirs[~np.array(mirrors)])


def test_summary_of_a_hand_made_table():
    q = 4
    raw = np.array([[[4, 4, 48, 32, 12, 24], [4, 2, 16, 8, 0, 8], [3, 0, 0, 0, 0, 0]]], dtype=float)
    s = P.summarize_polarisation(raw, 5, q)
    assert s["passed"].dtype == np.int64 and s["passed"].tolist() == [[4, 4, 3]] and s["valid"].tolist() == [[4, 2, 0]]
    assert s["transmittance"][0, :2].tolist() == [[48 / 64, 32 / 64], [16 / 32, 8 / 32]]
    assert s["throughput"][0].tolist() == [[48 / 80, 32 / 80], [16 / 80, 8 / 80], [0.0, 0.0]]
    t = [[48 / 80, 32 / 80], [16 / 80, 8 / 80]]
    assert s["unpolarised_throughput"][0].tolist() == [0.5 * (a + b) for a, b in t] + [0.0]
    assert s["diattenuation"][0, :2].tolist() == [(a - b) / (a + b) for a, b in t]
    assert np.allclose(s["diattenuation"][0, :2], [0.2, 1 / 3], rtol=1e-15)
    assert s["cross_leakage"][0, :2].tolist() == [[12 / 48, 8 / 32], [0.0, 0.0]]
    assert np.isnan(s["transmittance"][0, 2]).all() and np.isnan(s["cross_leakage"][0, 2]).all()
    assert np.isnan(s["diattenuation"][0, 2])
    assert set(s) == {"raw", "passed", "valid", "transmittance", "throughput", "unpolarised_throughput",
                      "diattenuation", "cross_leakage"}
    with pytest.raises(ValueError):
        P.summarize_polarisation(np.zeros((3, 5)), 5, q)


FAN = ([[0.0, 0.0, -5.0]], [0.5, 0.6], 0.05, 5, 3)
BEAM = ([[0.0, 0.0, 1.0]], [0.5, 0.6], 1.0, 5, 3)
FAULTS = [(dict(coatings=np.zeros((2, 2))), "coatings must have shape 1 x 2"),
          (dict(coatings=np.array([[1.0, np.nan]])), "coatings must be finite"),
          (dict(coatings=np.array([[3.0, 0.5]])), "mode must be 0 (CONSTANT), 1 (FRESNEL) or 2 (MIRROR)"),
          (dict(coatings=np.array([[2.0, 1.5]])), "value must lie in [0, 1]"),
          (dict(polariser=(0, 0, 0)), "polariser must be three finite numbers, not all zero"),
          (dict(polariser=(1, np.nan, 0)), "polariser must be three finite numbers"),
          (dict(polariser=(1, 0)), "polariser must be three finite numbers"),
          (dict(analyser=(0, 0, 0)), "analyser must be three finite numbers, not all zero"),
          (dict(analyser=(np.inf, 0, 0)), "analyser must be three finite numbers"),
          (dict(q_bits=0), "q_bits must be an integer in 1 ... 40"), (dict(q_bits=41), "q_bits must be an integer"),
          (dict(q_bits=2.5), "q_bits must be an integer"), (dict(devices=[0], fused=False), "devices=")]


@pytest.mark.parametrize("fault,word", FAULTS, ids=[str(k) for k in range(len(FAULTS))])
def test_the_pair_refuses_one_fault_with_one_text(monkeypatch, fault, word):
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    flat = rt.System([rt.FlatSurface([0, 0, 0], [0, 0, 1], 10.0)], [])
    said = []
    for fn, source in ((P.polarisation_sweep, FAN), (P.collimated_polarisation_sweep, BEAM)):
        with pytest.raises(ValueError) as err:
            fn(flat, None, None, *source, **fault)
        said.append(str(err.value))
    assert said[0] == said[1] and word in said[0]


def test_python_entry_points_refuse_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    c = SC.case("c2")
    S = len(c.S)
    coat, media = P.default_coatings(c.system), np.ones((2, S + 1))
    h64 = torch.zeros((2 * S + 1, 8, 8), dtype=torch.float64)
    for fn in (P.polarisation_stats_raw, P.ray_polarisation, P.polarisation_stats):
        with pytest.raises(ValueError, match="float64 only"):
            fn(torch.zeros((2 * S + 1, 8, 8), dtype=torch.float32), 4, media, coat)
        with pytest.raises(ValueError, match="float64 only"):
            fn(h64, 4, media.astype(np.float32), coat)
        with pytest.raises(ValueError, match="history must have shape"):
            fn(torch.zeros((2 * S, 8, 8), dtype=torch.float64), 4, media, coat)
        with pytest.raises(ValueError, match=f"coatings must have shape {S} x 2"):
            fn(h64, 4, media, coat[:-1])
        with pytest.raises(ValueError, match=f"media must have shape 2 x {S + 1}"):
            fn(h64, 4, media[:1], coat)
        with pytest.raises(ValueError, match="multiple of group_size"):
            fn(h64, 3, media, coat)
        with pytest.raises(ValueError, match="polariser must be three finite numbers"):
            fn(h64, 4, media, coat, polariser=(0, 0, 0))
    with pytest.raises(ValueError, match="largest admissible q_bits is 39"):
        P.polarisation_stats_raw(torch.zeros((2 * S + 1, 8193, 8), dtype=torch.float64), 8193, media[:1], coat,
                                 q_bits=40)
    with pytest.raises(ValueError, match="float64 only"):
        P.polarisation_sweep(c.system, c.m0, c.m1, np.zeros((1, 3), dtype=np.float32), [0.5], 0.1, 5, 3)
    with pytest.raises(ValueError, match="float64 only"):
        P.collimated_polarisation_sweep(c.system, c.m0, c.m1, np.array([[0, 0, 1]], dtype=np.float32), [0.5], 1.0, 5,
                                        3)
    with pytest.raises(ValueError, match="float64 only"):
        P.polarisation_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3,
                             polariser=np.array([1, 0, 0], dtype=np.float32))
    with pytest.raises(TypeError):
        P.polarisation_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, dtype="float32")
    with pytest.raises(ValueError, match="largest admissible q_bits is 39"):
        P.polarisation_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 8193, 1, q_bits=40)
    seen = []
    monkeypatch.setattr(analysis, "_sweep", lambda *a: seen.append(a[0]) or (
        "summary", a[0].entry, a[4].suffix, a[6], a[0].planes, a[0].ncols, a[0].group_doubles, a[0].tables))
    assert P.polarisation_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 30, 10,
                                polariser=(0, 3, 4)) == (
        "summary", "rtpb_polarisation_sweep", "", "float64", "all", None, 2 * S * 6, ())
    assert P.collimated_polarisation_sweep(c.system, c.m0, c.m1, [[0, 0, 1]], [0.5], 1.0, 19, 27,
                                           analyser=(2, 0, 0))[:7] == (
        "summary", "rtpb_polarisation_sweep", "_collimated", "float64", "all", None, 3 * S * 6)
    # the axes reach the calls normalised; analyser=None is the polariser
    assert seen[0].consts[2].tolist() == [0.0, 0.6, 0.8] == seen[0].consts[3].tolist()
    assert seen[1].consts[2].tolist() == [1.0, 0.0, 0.0] == seen[1].consts[3].tolist()
    assert np.array_equal(seen[0].consts[0], coat) and seen[0].consts[1] == S and seen[0].consts[4] == 24
