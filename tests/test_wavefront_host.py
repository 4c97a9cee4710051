"""Wavefront statistics on the host: the argument checks of rtpb_wavefront_stats / rtpb_wavefront_sweep (no GPU is
touched), analysis.summarize_wavefront / rms_opd_at against a direct per-ray calculation on oracle-traced fans, and
what tests/test_gpu_wavefront.py assumes about the named sweep cases, checked with the oracle alone.

Tolerance of the summary (derived from the data, on the variance): Var(w) = S_ww / n - (S_w / n)^2 with S_ww a sum of
n rounded products of size at most max|w|^2; accumulated in any order the rounding errors add like a random walk,
eps * max|w|^2 * sqrt(n), and the division and the subtraction add a few eps * max|w|^2 more.  With a factor 16 of
slack  |Var - exact| <= 16 * eps * max|w|^2 * sqrt(n).  The best-reference variance adds 2 kf delta . cov_we +
kf^2 delta' cov_ee delta, moments of kf delta . e, which cancels w and is of its size: the same bound holds it."""

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
from oracle import rt_numpy as O
import ray_trace_pb_amd.raytrace as rt
from flat_plans import flat_plan
import sweep_cases as SC
from wave_refs import ALIVE, case_refs
import wave_oracle as W

EPS = 2.0 ** -52
# of wave_refs.ALIVE (every group has a finite chief ray and counts rays), the cases with dead rows beside them
WITH_DEAD_ROWS = ("xz", "c5_wide", "c4", "tangent")


def case_counts(name, refs):
    c = SC.case(name)
    terms = W.wave_terms(SC.oracle_finals(name), c.nt * c.nph, refs)
    return terms[..., 0].sum(axis=1).reshape(len(c.fields), len(c.wls))


def test_wavefront_entry_points_validate_without_a_gpu():
    """rtpb_wavefront_stats / rtpb_wavefront_sweep: NULL pointers, non-positive sizes, a short workspace and anything
    float32 are RTPB_E_INVALID, more than 65535 groups RTPB_E_LIMIT, all before any device work (the pointers here
    are host memory, never read)."""
    lib = C.lib()
    buf = np.zeros(4096)
    p = buf.ctypes.data
    per, G, tiles = 300, 2, 2
    ok = dict(device=0, dtype=C.RTPB_F64, plane=p, group_size=per, n_groups=G, refs=p, workspace=p,
              workspace_len=G * tiles * 15, stats_out=p, stream=None)
    for bad in (dict(plane=None), dict(refs=None), dict(workspace=None), dict(stats_out=None), dict(group_size=0),
                dict(n_groups=0), dict(n_groups=-1), dict(dtype=7)):
        assert lib.rtpb_wavefront_stats(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
        assert b"wavefront-stats" in lib.rtpb_last_error(), bad
    assert lib.rtpb_wavefront_stats(*dict(ok, dtype=C.RTPB_F32).values()) == C.RTPB_E_INVALID
    assert b"float64 planes only" in lib.rtpb_last_error() and b"float32 phase" in lib.rtpb_last_error()
    assert lib.rtpb_wavefront_stats(*dict(ok, workspace_len=G * tiles * 15 - 1).values()) == C.RTPB_E_INVALID
    assert b"workspace too small" in lib.rtpb_last_error() and b"* 15 doubles" in lib.rtpb_last_error()
    assert lib.rtpb_wavefront_stats(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT

    plan, plan32 = flat_plan(C.RTPB_F64), flat_plan(C.RTPB_F32)
    try:
        ok = dict(plan=plan, device=0, n_groups=G, group_params=p, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                  theta_cos_sin=p, phi_cos_sin=p, refs=p, workspace=p, workspace_len=G * tiles * 15, stats_out=p,
                  stream=None)
        assert lib.rtpb_wavefront_sweep(*dict(ok, plan=None).values()) == C.RTPB_E_INVALID
        assert b"plan is NULL" in lib.rtpb_last_error()
        for bad in (dict(group_params=None), dict(center_ray=None), dict(ex=None), dict(ey=None),
                    dict(theta_cos_sin=None), dict(phi_cos_sin=None), dict(refs=None), dict(workspace=None),
                    dict(stats_out=None), dict(n_groups=0), dict(n_thetas=0), dict(nphis=-3)):
            assert lib.rtpb_wavefront_sweep(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, bad
            assert b"wavefront-sweep" in lib.rtpb_last_error(), bad
        assert lib.rtpb_wavefront_sweep(*dict(ok, workspace_len=G * tiles * 15 - 1).values()) == C.RTPB_E_INVALID
        assert b"workspace too small" in lib.rtpb_last_error() and b"* 15 doubles" in lib.rtpb_last_error()
        assert lib.rtpb_wavefront_sweep(*dict(ok, n_groups=65536, workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
        assert lib.rtpb_wavefront_sweep(*dict(ok, plan=plan32).values()) == C.RTPB_E_INVALID
        assert b"float64 plans only" in lib.rtpb_last_error() and b"float32 phase" in lib.rtpb_last_error()
    finally:
        assert lib.rtpb_plan_destroy(plan) == 0 and lib.rtpb_plan_destroy(plan32) == 0


def test_signatures_cover_the_wavefront_calls():
    assert len(C.SIGNATURES["rtpb_wavefront_stats"][1]) == 10
    assert len(C.SIGNATURES["rtpb_wavefront_sweep"][1]) == 16
    assert len(analysis.WAVE_STAT_NAMES) == 15 == W.NS and analysis.WAVE_STAT_NAMES[0] == "count"


def test_python_entry_points_refuse_float32_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    with pytest.raises(ValueError, match="float64"):
        analysis.wavefront_stats_raw(torch.zeros((8, 8), dtype=torch.float32), 4, np.zeros((2, 8)))
    with pytest.raises(ValueError, match="float64"):
        analysis.wavefront_sweep(None, None, None, [[0.0, 0.0, 0.0]], [0.5], 0.1, 5, 3, refs=np.zeros((1, 1, 8)),
                                 dtype="float32")
    with pytest.raises(ValueError, match="refs must have shape 2 x 8"):
        analysis.wavefront_stats_raw(torch.zeros((8, 8), dtype=torch.float64), 4, np.zeros((3, 8)))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: ("summary", a[0].entry))
    with pytest.raises(ValueError, match="refs must have shape 1 x 2 x 8"):
        analysis.wavefront_sweep(None, None, None, [[0.0, 0.0, 0.0]], [0.5, 0.6], 0.1, 5, 3, refs=np.zeros((2, 8)))
    assert analysis.wavefront_sweep(None, None, None, [[0.0, 0.0, 0.0]], [0.5, 0.6], 0.1, 5, 3,
                                    refs=np.zeros((1, 2, 8))) == ("summary", "rtpb_wavefront_sweep")


def direct(fin, ref):
    """Per-ray figures of one group, two-pass: the rays that count, their OPD w about C0 and their directions."""
    ok = np.isfinite(fin[:, :7]).all(axis=1)
    g = fin[ok]
    P, d, ph = g[:, :3], g[:, 3:6], g[:, 6]
    w = (ph - ref[6]) / (2 * np.pi) + ((ref[0:3] - P) * d).sum(axis=1) * ref[7]
    return w, d


def test_summary_against_a_direct_per_ray_calculation_on_c2():
    """summarize_wavefront / rms_opd_at from raw sums built here (np.sum's pairwise order, not the kernels') against
    the per-ray figures of oracle-traced C2 fans, 61 x 12 rays: rms_opd is w.std(), rms_opd_best the standard
    deviation of w + kf d . shift, rms_opd_at(shift) is rms_opd_best, and the best reference is better."""
    c = SC.case("c2")
    nt, nph = 61, 12
    fin = np.concatenate([O.ray_trace(c.S, c.M, rt.get_ray_fan(f, c.theta, nt, wl, nphis=nph))[-1]
                          for f in c.fields for wl in c.wls])
    refs = W.oracle_refs(c.S, c.M, c.m1, c.fields, c.wls, fin)
    assert np.isfinite(refs).all()
    raw = W.wave_terms(fin, nt * nph, refs).sum(axis=1).reshape(len(c.fields), len(c.wls), 15)
    summ = analysis.summarize_wavefront(raw, refs)
    assert (summ["count"] == nt * nph).all()
    fin = fin.reshape(len(c.fields), len(c.wls), nt * nph, 8)
    worst = 0.0
    for i in range(len(c.fields)):
        for j in range(len(c.wls)):
            w, d = direct(fin[i, j], refs[i, j])
            n, kf, shift = len(w), refs[i, j, 7], summ["shift"][i, j]
            tol = 16 * EPS * np.sqrt(n) * np.abs(w).max() ** 2
            dev = abs(summ["rms_opd"][i, j] ** 2 - w.var())
            best = (w + kf * d @ shift).var()
            dev_best = abs(summ["rms_opd_best"][i, j] ** 2 - best)
            print(f"group {i},{j}: rms_opd {summ['rms_opd'][i, j]:.6e} (variance off by {dev:.2e}, bound {tol:.2e}); "
                  f"best {summ['rms_opd_best'][i, j]:.6e} (off by {dev_best:.2e}); "
                  f"shift {shift}")
            worst = max(worst, dev / tol, dev_best / tol)
            assert dev <= tol and dev_best <= tol
            assert abs(summ["mean_opd"][i, j] - w.mean()) <= 16 * EPS * np.abs(w).max()
            assert summ["rms_opd_best"][i, j] < summ["rms_opd"][i, j]
    print("largest deviation / bound:", worst)
    assert np.array_equal(analysis.rms_opd_at(summ, summ["shift"]), summ["rms_opd_best"])
    assert np.array_equal(analysis.rms_opd_at(summ, np.zeros(3)), summ["rms_opd"])
    assert np.array_equal(summ["reference_best"], refs[..., 0:3] + summ["shift"])
    assert np.array_equal(summ["strehl"], np.exp(-(2 * np.pi * summ["rms_opd"]) ** 2))
    assert (summ["strehl_best"] > summ["strehl"]).all() and (summ["strehl_best"] <= 1).all()
    # one displacement for every group, and one per group
    one = analysis.rms_opd_at(summ, [0.0, 0.0, 1e-3])
    per = analysis.rms_opd_at(summ, np.broadcast_to([0.0, 0.0, 1e-3], summ["shift"].shape))
    assert one.shape == summ["rms_opd"].shape and np.array_equal(one, per)


def test_summary_of_empty_and_collimated_groups():
    """A group without rays is NaN throughout; a collimated bundle (every e on a line: cov_ee of rank 1) gets a
    shift along that line only, the unconstrained components 0 and not garbage."""
    rng = np.random.default_rng(3)
    n = 500
    t = rng.normal(size=n) * 1e-3
    e = np.stack((t, np.zeros(n), np.zeros(n)), axis=1)             # directions differ along x only
    kf = 2.0
    w = 0.25 * kf * t + 1e-9 * rng.normal(size=n)                   # a tilt: the reference is 0.25 off in -x
    cols = [np.ones(n), w, w * w, e[:, 0], e[:, 1], e[:, 2], w * e[:, 0], w * e[:, 1], w * e[:, 2], e[:, 0] ** 2,
            e[:, 1] ** 2, e[:, 2] ** 2, e[:, 0] * e[:, 1], e[:, 0] * e[:, 2], e[:, 1] * e[:, 2]]
    raw = np.stack((np.array([c.sum() for c in cols]), np.zeros(15)))
    refs = np.zeros((2, 8))
    refs[:, 7] = kf
    refs[1] = np.nan
    summ = analysis.summarize_wavefront(raw, refs)
    assert summ["shift"][0, 1] == 0 and summ["shift"][0, 2] == 0
    assert abs(summ["shift"][0, 0] + 0.25) < 1e-5
    assert summ["rms_opd_best"][0] < 1e-2 * summ["rms_opd"][0]
    for k in ("mean_opd", "rms_opd", "strehl", "shift", "reference_best", "rms_opd_best", "strehl_best", "cov_we",
              "cov_ee"):
        assert np.isnan(summ[k][1]).all(), k
    assert summ["count"][1] == 0
    assert np.isnan(analysis.rms_opd_at(summ, [0.0, 0.0, 1.0])[1])


@pytest.mark.parametrize("name", ALIVE)
def test_cases_with_live_chief_rays(name):
    """What test_gpu_wavefront.py assumes of these cases at the fan shape it sweeps: every group's chief ray is
    finite and every group counts rays; the ones listed have dead rows beside them."""
    c = SC.case(name)
    refs = case_refs(name)
    assert np.isfinite(refs).all()
    counts = case_counts(name, refs)
    assert counts.min() > 0
    assert np.array_equal(counts, SC.oracle_counts(name))            # every ray the spot statistics count, counts
    if name in WITH_DEAD_ROWS:
        assert (counts < c.nt * c.nph).any()


def test_cases_with_dead_chief_rays():
    """tir: every group's chief ray is dead (every reference NaN, no ray counts).  stress: some groups' chief rays
    are dead and some are not, and exactly the live ones count rays."""
    refs = case_refs("tir")
    assert np.isnan(refs).all() and (case_counts("tir", refs) == 0).all()
    refs = case_refs("stress")
    dead = np.isnan(refs).any(axis=-1)
    assert dead.any() and not dead.all()
    assert np.array_equal(np.isnan(refs).all(axis=-1), dead)
    assert np.array_equal(case_counts("stress", refs) == 0, dead)
