"""Footprint statistics on the host: the argument checks of rtpb_footprint_stats / rtpb_footprint_sweep[_collimated]
(no GPU is touched), the Python entry points' refusals, foot_ray / foot_merge (ray_trace_pb_amd/csrc/rtpb_foot.h) run
on the CPU against the NumPy restatement (tests/foot_oracle.py), analysis.summarize_footprint against a direct per-ray
calculation, and what tests/test_gpu_footprint.py assumes about the named sweep cases, checked with the oracle alone."""
import math

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import _engine as E
from ray_trace_pb_amd import analysis
import ray_trace_pb_amd.raytrace as rt
import foot_harness as FH
import foot_oracle as FO
from native_harness import harness_trace
import sweep_cases as SC
from flat_plans import flat_plan
from foot_cases import CASES, NT, NPH, case_columns, case_fans, case_histories, tilted_frames


def test_footprint_entry_points_validate_without_a_gpu():
    """NULL pointers, non-positive sizes, a non-finite frame, a frame count that is not the plan's, a short workspace
    and anything float32 are RTPB_E_INVALID, more than 65535 groups RTPB_E_LIMIT, all before any device work (the
    pointers here are host memory, never read except the frames)."""
    lib = C.lib()
    buf = np.zeros(4096)
    p = buf.ctypes.data
    frames = np.zeros((3, 9))
    bad_frames = frames.copy()
    bad_frames[2, 4] = np.inf
    nan_frames = frames.copy()
    nan_frames[0, 0] = np.nan
    per, G, tiles, S = 300, 2, 2, 3
    ok = dict(device=0, dtype=C.RTPB_F64, history=p, group_size=per, n_groups=G, nsurf=S, frames=frames.ctypes.data,
              workspace=p, workspace_len=G * tiles * S * 8, stats_out=p, stream=None)
    for bad in (dict(history=None), dict(frames=None), dict(workspace=None), dict(stats_out=None), dict(group_size=0),
                dict(n_groups=0), dict(n_groups=-1), dict(nsurf=0), dict(dtype=7),
                dict(frames=bad_frames.ctypes.data), dict(frames=nan_frames.ctypes.data)):
        assert lib.rtpb_footprint_stats(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"footprint-stats" in lib.rtpb_last_error(), bad
    assert lib.rtpb_footprint_stats(*dict(ok, dtype=C.RTPB_F32).values()) == C.RTPB_E_INVALID
    assert b"float64 histories only" in lib.rtpb_last_error()
    assert lib.rtpb_footprint_stats(*dict(ok, workspace_len=G * tiles * S * 8 - 1).values()) == C.RTPB_E_INVALID
    assert b"workspace too small" in lib.rtpb_last_error() and b"* nsurf * 8 doubles" in lib.rtpb_last_error()
    assert lib.rtpb_footprint_stats(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
    big = np.zeros((64, 9))
    assert lib.rtpb_footprint_stats(*dict(ok, nsurf=64, frames=big.ctypes.data,
                                          workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT

    plan, plan32 = flat_plan(C.RTPB_F64), flat_plan(C.RTPB_F32)           # one surface
    one = np.zeros((1, 9))
    one_bad = one.copy()
    one_bad[0, 8] = -np.inf
    blocks = 1                                                              # 300 rays: two tiles, one block
    try:
        fan = dict(plan=plan, device=0, n_groups=G, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                   theta_cos_sin=p, phi_cos_sin=p, frames=one.ctypes.data, n_frames=1, workspace=p,
                   workspace_len=G * blocks * 1 * 8, stats_out=p, stream=None)
        beam = dict(plan=plan, device=0, n_groups=G, group_params=p, group_frames=p, n_disps=30, nphis=10, offsets=p,
                    phi_cos_sin=p, frames=one.ctypes.data, n_frames=1, workspace=p,
                    workspace_len=G * blocks * 1 * 8, stats_out=p, stream=None)
        for fn, ok, nulls in ((lib.rtpb_footprint_sweep, fan, ("group_params", "center_ray", "ex", "ey",
                                                                "theta_cos_sin", "phi_cos_sin")),
                              (lib.rtpb_footprint_sweep_collimated, beam, ("group_params", "group_frames", "offsets",
                                                                           "phi_cos_sin"))):
            assert len(ok) == len(C.SIGNATURES[fn.__name__][1])
            assert fn(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
            assert b"plan is NULL" in lib.rtpb_last_error()
            first = "n_thetas" if "n_thetas" in ok else "n_disps"
            for bad in [{k: None} for k in nulls + ("frames", "workspace", "stats_out")] + [
                    dict(n_groups=0), {first: 0}, dict(nphis=-3), dict(n_frames=2), dict(n_frames=0),
                    dict(frames=one_bad.ctypes.data)]:
                assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
                assert b"footprint-sweep" in lib.rtpb_last_error(), bad
            assert fn(*dict(ok, workspace_len=G * blocks * 8 - 1).values()) == C.RTPB_E_INVALID
            assert b"workspace too small" in lib.rtpb_last_error() and b"* nsurf * 8 doubles" in lib.rtpb_last_error()
            assert fn(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
            assert fn(*dict(ok, plan=plan32).values()) == C.RTPB_E_INVALID
            assert b"float64 plans only" in lib.rtpb_last_error()
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0 and lib.rtpb_plan_destroy(plan32) == 0


def test_signatures_cover_the_footprint_calls_and_the_abi_version_stays():
    assert len(C.SIGNATURES["rtpb_footprint_stats"][1]) == 11
    assert len(C.SIGNATURES["rtpb_footprint_sweep"][1]) == 17
    assert len(C.SIGNATURES["rtpb_footprint_sweep_collimated"][1]) == 15
    assert C.lib().rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    assert len(analysis.FOOT_STAT_NAMES) == 8 == FO.NCOLS


def test_python_entry_points_refuse_float32_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    c = SC.case("c2")
    S = len(c.S)
    with pytest.raises(ValueError, match="float64 only"):
        analysis.footprint_stats_raw(torch.zeros((2 * S + 1, 8, 8), dtype=torch.float32), 4, np.zeros((S, 9)))
    with pytest.raises(ValueError, match="float64 only"):
        analysis.footprint_stats_raw(torch.zeros((2 * S + 1, 8, 8), dtype=torch.float64), 4,
                                     np.zeros((S, 9), dtype=np.float32))
    with pytest.raises(ValueError, match="float64 only"):
        analysis.footprint_sweep(c.system, c.m0, c.m1, np.zeros((1, 3), dtype=np.float32), [0.5], 0.1, 5, 3)
    with pytest.raises(ValueError, match="float64 only"):
        analysis.footprint_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3,
                                 frames=np.zeros((S, 9), dtype=np.float32))
    with pytest.raises(ValueError, match="float64 only"):
        analysis.collimated_footprint_sweep(c.system, c.m0, c.m1, np.array([[0, 0, 1]], dtype=np.float32), [0.5],
                                            1.0, 5, 3)
    with pytest.raises(TypeError):
        analysis.footprint_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, dtype="float32")
    with pytest.raises(ValueError, match=f"frames must have shape {S} x 9"):
        analysis.footprint_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, frames=np.zeros((S, 8)))
    with pytest.raises(ValueError, match="frames must be finite"):
        analysis.footprint_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3,
                                 frames=np.full((S, 9), np.nan))
    with pytest.raises(ValueError, match=r"history must have shape"):
        analysis.footprint_stats_raw(torch.zeros((2 * S, 8, 8), dtype=torch.float64), 4, np.zeros((S, 9)))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: ("summary", a[0].entry, a[4].suffix, a[6]))
    assert analysis.footprint_sweep(c.system, c.m0, c.m1, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3) == (
        "summary", "rtpb_footprint_sweep", "", "float64")
    assert analysis.collimated_footprint_sweep(c.system, c.m0, c.m1, [[0, 0, 1]], [0.5], 1.0, 5, 3) == (
        "summary", "rtpb_footprint_sweep", "_collimated", "float64")


def test_footprint_frames_of_an_axial_system_are_center_x_y():
    for name in ("c2", "c5_wide"):
        c = SC.case(name)
        fr = analysis.footprint_frames(c.system)
        assert fr.shape == (len(c.S), 9) and fr.dtype == np.float64
        assert np.array_equal(fr, FO.default_frames(c.S))
        assert not np.signbit(fr[:, 3:]).any()
    # a tilted axis: an orthonormal basis across it, finite along y too
    c = SC.case("xz")
    fr = analysis.footprint_frames(c.system)
    axes = np.array([s.input_axis for s in c.system.surfaces], dtype=float)
    for a, f in zip(axes, fr):
        m = np.stack((f[3:6], f[6:9], a / np.linalg.norm(a)))
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-15)
    y = rt.System([rt.FlatSurface([0, 0, 0], [0, 1, 0], 10.0)], [])
    assert np.isfinite(analysis.footprint_frames(y)).all()


def test_batch_sizing_counts_the_mode_s_bytes():
    """The default batch holds the partials and the statistics of its groups within the sweeps' workspace bound."""
    per, S = 23177, 14
    mode = analysis._foot_mode(np.zeros((S, 9)), per, np.ones(S))
    blocks = -(-91 // 2)
    assert mode.group_doubles == (blocks + 1) * S * 8
    gpb, _, launches = analysis._sweep_plan(20000, 7, per, 1, None, mode.ncols, mode.group_doubles)
    assert gpb * mode.group_doubles <= 1 << 26 < (gpb + 7) * mode.group_doubles and gpb % 7 == 0
    assert launches[0] == (0, 0, gpb)
    # a small sweep is one batch, and the other modes' plans are what they were
    assert analysis._sweep_plan(3, 3, 301, 1, None, None, mode.group_doubles)[0] == 9
    assert analysis._sweep_plan(64, 7, per, 1, None, 7) == analysis._sweep_plan(64, 7, per, 1, None, 7, None)


@pytest.mark.parametrize("name", ["c2", "stress", "c4", "tir"])
def test_foot_ray_on_the_host_matches_the_restatement(name):
    """foot_ray / foot_merge compiled for the CPU, applied to the CPU harness's histories of the case's fans, give the
    restatement's columns bit for bit -- with the default frames and with tilted, off-axis ones."""
    c = SC.case(name)
    rays = np.concatenate(case_fans(name))
    low = E.lower(c.system.surfaces, [c.m0] + list(c.system.materials) + [c.m1], lambda: np.unique(rays[:, 7]),
                  C.RTPB_F64)
    hist = harness_trace(low, rays)
    per = NT * NPH
    for fr in (analysis.footprint_frames(c.system), tilted_frames(c.system)):
        got = FH.foot_stats(hist, per, fr)
        exp = FO.foot_columns(hist, fr, per)
        assert got.shape == (len(c.fields) * len(c.wls), len(c.S), 8)
        assert np.array_equal(got, exp)
    if name != "c2":
        assert (got[..., 1] < got[..., 0]).any()                 # rays arrive that do not pass


def test_foot_ray_edge_rows_and_columns():
    """An empty set is -inf / +inf; rows with NaN or infinite positions do not arrive; a row whose rho2 overflows to
    inf is kept as inf; a row whose u is inf - inf = NaN still counts and is skipped by the comparisons; the column
    combination is a sum, a maximum or a minimum."""
    S = 1
    fr = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]])
    h = np.zeros((3, 6, 8))
    h[1, :, 0:3] = [[1.0, 2.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1e200, 1e200, 0.0], [-3.0, 0.5, 0.0],
                    [0.0, 0.0, -np.inf]]
    h[2] = h[1]
    h[2, 4, 0] = np.nan                                           # arrives, does not pass
    got = FH.foot_stats(h, 6, fr)
    assert np.array_equal(got, FO.foot_columns(h, fr))
    assert got[0, 0].tolist() == [3.0, 2.0, np.inf, np.inf, 1.0, 1e200, 2.0, 1e200]
    h[1:, 3, 0:2] = [1.7e308, 1.7e308]
    fr2 = fr.copy()
    fr2[0, 3:6] = [8.0, -8.0, 0.0]                                # row 3: u = inf - inf = NaN, rho2 NaN, v finite
    nan_u = FH.foot_stats(h, 6, fr2)
    assert np.array_equal(nan_u, FO.foot_columns(h, fr2))
    assert nan_u[0, 0].tolist() == [3.0, 2.0, 784.25, 68.0, -8.0, -8.0, 2.0, 1.7e308]
    empty = FH.foot_stats(np.full((3, 4, 8), np.nan), 4, fr)
    assert empty[0, 0].tolist() == [0.0, 0.0, -np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf]
    assert np.array_equal(empty, FO.foot_columns(np.full((3, 4, 8), np.nan), fr))
    col = FH.harness().foot_harness_col
    assert [col(k, 2.0, 5.0) for k in range(8)] == [7.0, 7.0, 5.0, 5.0, 2.0, 5.0, 2.0, 5.0]
    assert col(3, -np.inf, 1.0) == 1.0 and col(4, np.inf, 1.0) == 1.0
    assert S == 1


def direct_summary(hist, frames, per, aperture_rads):
    """One group's figures ray by ray, in plain Python: counts, losses, radii and boxes per surface."""
    S = len(frames)
    out = dict(arrive=[], passed=[], semi=[], need=[], box=[])
    for s in range(S):
        o, e1, e2 = frames[s, 0:3], frames[s, 3:6], frames[s, 6:9]
        arrive = passed = 0
        r_arr, r_pass, us, vs = [], [], [], []
        for j in range(per):
            A, B = hist[2 * s + 1, j, 0:3], hist[2 * s + 2, j, 0:3]
            if not all(math.isfinite(x) for x in A):
                continue
            q = A - o
            u = (q[0] * e1[0] + q[1] * e1[1]) + q[2] * e1[2]
            v = (q[0] * e2[0] + q[1] * e2[1]) + q[2] * e2[2]
            r = math.sqrt(u * u + v * v)
            arrive += 1
            r_arr.append(r)
            if all(math.isfinite(x) for x in B):
                passed += 1
                r_pass.append(r)
                us.append(u)
                vs.append(v)
        out["arrive"].append(arrive)
        out["passed"].append(passed)
        out["need"].append(max(r_arr) if r_arr else np.nan)
        out["semi"].append(max(r_pass) if r_pass else np.nan)
        out["box"].append([min(us), max(us), min(vs), max(vs)] if us else [np.nan] * 4)
    return {k: np.array(v) for k, v in out.items()}


@pytest.mark.parametrize("name", CASES)
def test_summary_against_a_direct_per_ray_calculation(name):
    """summarize_footprint of the restatement's columns against plain per-ray Python on the oracle's histories (the
    first two fields, first wavelength, 301 rays), and the figures the GPU tests assume of the cases -- all from the
    oracle, none from the library under test."""
    c = SC.case(name)
    per, nw = NT * NPH, len(c.wls)
    frames = analysis.footprint_frames(c.system)
    ap = analysis._aperture_rads(c.system)
    raw = np.array(case_columns(name))[:2, :1]
    summ = analysis.summarize_footprint(raw, per, ap)
    assert summ["arrive"].dtype == np.int64 and summ["passed"].dtype == np.int64
    assert summ["raw"].shape == (2, 1, len(c.S), 8)
    for f in range(2):
        hist = case_histories(name)[f * nw]
        d = direct_summary(hist, frames, per, ap)
        assert np.array_equal(summ["arrive"][f, 0], d["arrive"])
        assert np.array_equal(summ["passed"][f, 0], d["passed"])
        before = np.concatenate(([per], d["passed"][:-1]))
        assert np.array_equal(summ["missed"][f, 0], before - d["arrive"])
        assert np.array_equal(summ["clipped"][f, 0], d["arrive"] - d["passed"])
        assert np.array_equal(summ["semi_diameter"][f, 0], d["semi"], equal_nan=True)
        assert np.array_equal(summ["semi_diameter_needed"][f, 0], d["need"], equal_nan=True)
        assert np.array_equal(summ["box"][f, 0], d["box"], equal_nan=True)
        assert np.array_equal(summ["fill"][f, 0], d["semi"] / ap, equal_nan=True)
        lost = (before - d["arrive"]) + (d["arrive"] - d["passed"])
        assert summ["limiting_surface"][f, 0] == (lost.argmax() if lost.max() > 0 else -1)
        # passed[last] is the spot count of the final plane
        assert summ["passed"][f, 0, -1] == SC.alive(hist[-1]).sum()
        # the rays a surface passes lie within its aperture where the frame is the aperture's own (axial spheres and
        # flats; a PerfectLens is limited by its numerical aperture instead)
        if name in ("c2", "tangent"):
            with np.errstate(invalid="ignore"):
                assert not (summ["fill"][f, 0] > 1 + 1e-12).any()
    missed, clipped = summ["missed"][:, 0], summ["clipped"][:, 0]
    if name == "c2":
        assert not missed.any() and not clipped.any() and (summ["limiting_surface"] == -1).all()
    elif name == "tir":
        assert not missed.any() and clipped.tolist() == [[0, 227, 0], [0, 227, 0]]
    elif name == "stress":
        assert not missed[0].any() and clipped[0].tolist() == [0, 0, 0, 0, 0, 0, 144, 0, 99, 0, 5]
        assert clipped[1, 6] > 0 and clipped[1, 8] > 0 and clipped[1, 10] > 0
    elif name == "c4":
        for f in range(2):
            assert clipped[f].tolist() == [2, 0, 0, 0, 0, 12, 0, 0, 0, 0, 0]
            assert missed[f].tolist() == [0, 0, 0, 0, 0, 0, 12, 0, 0, 0, 0]
    elif name == "c5_wide":
        assert not missed.any() and (clipped[:, -1] > 0).all() and ((clipped[:, :-1] > 0).sum(axis=1) >= 2).all()
        assert (summ["semi_diameter_needed"][..., 0] > summ["semi_diameter"][..., 0]).all()
    elif name == "tangent":
        assert missed.tolist() == [[147, 0], [168, 0]] and (clipped[:, 0] == 0).all() and (clipped[:, 1] > 0).all()
    elif name == "xz":
        assert not missed.any() and (clipped[:, 3] > 0).all() and not np.delete(clipped, 3, axis=1).any()
        assert (summ["limiting_surface"] == 3).all()


def test_summary_of_an_empty_group_and_shapes():
    raw = np.zeros((2, 3, 8))
    raw[..., 2:] = [-np.inf, -np.inf, np.inf, -np.inf, np.inf, -np.inf]
    raw[1] = [[5, 4, 9.0, 4.0, -1.0, 2.0, -0.5, 0.25], [4, 4, 1.0, 1.0, -1.0, 1.0, 0.0, 0.0],
              [3, 0, 16.0, -np.inf, np.inf, -np.inf, np.inf, -np.inf]]
    s = analysis.summarize_footprint(raw, 6, [2.0, 2.0, 2.0])
    assert s["missed"].tolist() == [[6, 0, 0], [1, 0, 1]] and s["clipped"].tolist() == [[0, 0, 0], [1, 0, 3]]
    assert s["limiting_surface"].tolist() == [0, 2]
    assert np.isnan(s["semi_diameter"][0]).all() and np.isnan(s["box"][0]).all() and np.isnan(s["fill"][0]).all()
    assert s["semi_diameter"][1].tolist()[:2] == [2.0, 1.0] and np.isnan(s["semi_diameter"][1, 2])
    assert s["semi_diameter_needed"][1].tolist() == [3.0, 1.0, 4.0]
    assert s["fill"][1, 0] == 1.0 and s["box"][1, 0].tolist() == [-1.0, 2.0, -0.5, 0.25]
    with pytest.raises(ValueError):
        analysis.summarize_footprint(raw, 6, [2.0, 2.0])
