"""The variant wavefront sweeps on the host: the argument checks of rtpb_wavefront_sweep_variants[_collimated] and
rtpb_final_rays_variants[_collimated] (no GPU is touched) and their ctypes signatures, what the Python wrappers refuse
before any device call and what they hand to the single driver, and that the oracle's answers of
tests/variant_wave_cases.py can tell the variants of each case apart."""
import ctypes

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import analysis
import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
import systems
import variant_cases as vc
import variant_wave_cases as vw
from flat_plans import _systems

WAVE = ("rtpb_wavefront_sweep_variants", "rtpb_wavefront_sweep_variants_collimated")
RAYS = ("rtpb_final_rays_variants", "rtpb_final_rays_variants_collimated")


def _calls(V, G, tiles, surf, mats, gv, p, n_a=30, n_b=10):
    head = dict(surfaces=ctypes.addressof(surf), nsurf=1, materials=ctypes.addressof(mats), n_variants=V, device=0,
                n_groups=G, group_params=p, group_variant=gv.ctypes.data)
    fan = dict(n_thetas=n_a, nphis=n_b, center_ray=p, ex=p, ey=p, theta_cos_sin=p, phi_cos_sin=p)
    beam = dict(group_frames=p, n_disps=n_a, nphis=n_b, offsets=p, phi_cos_sin=p)
    wave = dict(refs=p, workspace=p, workspace_len=G * tiles * 15, stats_out=p, stream=None)
    rays = dict(rays_out=p, stream=None)
    return {WAVE[0]: dict(head, **fan, **wave), WAVE[1]: dict(head, **beam, **wave),
            RAYS[0]: dict(head, **dict(fan, n_thetas=5, nphis=3), **rays),
            RAYS[1]: dict(head, **dict(beam, n_disps=5, nphis=3), **rays)}


def test_entry_points_validate_without_a_gpu():
    """Every refusal the header states for the four calls, before any device work (the data pointers are host memory;
    the device index of the last call names no device): NULL pointers, non-positive sizes and a short workspace are
    RTPB_E_INVALID, a group_variant entry out of range RTPB_E_INVALID naming the group, a POLY6 material RTPB_E_INVALID
    saying RTPB_TABLE; nsurf > RTPB_MAX_SURFACES, more than 65535 groups, more than 256 rays per group in the
    final-rays calls and an upload beyond the stated cap RTPB_E_LIMIT."""
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    buf = np.zeros(1 << 16)
    p = buf.ctypes.data
    V, G, tiles = 3, 4, 2                     # 30 x 10 rays: two tiles
    surf, mats = _systems(V)
    gv = np.array([0, 2, 1, 2], dtype=np.int32)
    for name, ok in _calls(V, G, tiles, surf, mats, gv, p).items():
        fn = getattr(lib, name)
        fan, wave = "n_thetas" in ok, name in WAVE
        what = b"wavefront-sweep-variants" if wave else b"final-rays-variants"
        own = b"bad wavefront-sweep arguments" if wave else b"bad final-rays arguments"
        sizes = ("n_thetas", "nphis") if fan else ("n_disps", "nphis")
        ptrs = ("center_ray", "ex", "ey", "theta_cos_sin", "phi_cos_sin") if fan else \
            ("group_frames", "offsets", "phi_cos_sin")
        outs = ("refs", "workspace", "stats_out") if wave else ("rays_out",)
        for bad in [dict(surfaces=None), dict(materials=None), dict(group_variant=None), dict(nsurf=0),
                    dict(nsurf=-1), dict(n_variants=0), dict(n_variants=-5)]:
            assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, (name, bad)
            assert b"bad " + what + b" arguments" in lib.rtpb_last_error(), (name, bad)
        bads = [dict(group_params=None), dict(n_groups=0), dict(n_groups=-1)] + [{k: None} for k in outs] + \
            [{k: None} for k in ptrs] + [{k: 0} for k in sizes] + [{k: -2} for k in sizes]
        for bad in bads:
            assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, (name, bad)
            assert own in lib.rtpb_last_error(), (name, bad)
        if wave:
            assert fn(*dict(ok, workspace_len=G * tiles * 15 - 1).values()) == C.RTPB_E_INVALID
            msg = lib.rtpb_last_error()
            assert b"workspace too small" in msg and b"* 15 doubles" in msg
            assert (b"n_thetas*nphis" if fan else b"n_disps*nphis") in msg
        else:
            # one tile of rays per group at the most: 256 is taken (and reaches the device check), 257 is not
            for a, b in ((257, 1), (1, 257), (16, 17), (1 << 31, 1 << 31), (1 << 62, 4)):
                assert fn(*dict(ok, **{sizes[0]: a, sizes[1]: b}).values()) == C.RTPB_E_LIMIT, (name, a, b)
                assert b"more than 256 rays per group" in lib.rtpb_last_error()
            assert fn(*dict(ok, **{sizes[0]: 16, sizes[1]: 16}, device=1 << 20).values()) in \
                (C.RTPB_E_NODEV, C.RTPB_E_INVALID, C.RTPB_E_HIP)
            assert b"final-rays" not in lib.rtpb_last_error()
        for g, v in ((1, V), (3, -1), (0, 1 << 30)):
            bad_gv = gv.copy()
            bad_gv[g] = v
            assert fn(*dict(ok, group_variant=bad_gv.ctypes.data).values()) == C.RTPB_E_INVALID
            msg = lib.rtpb_last_error()
            assert what + b": group %d names variant" % g in msg
        surf2, mats2 = _systems(V)
        mats2[2 * 1 + 1].kind = C.RTPB_POLY6
        assert fn(*dict(ok, materials=ctypes.addressof(mats2)).values()) == C.RTPB_E_INVALID
        msg = lib.rtpb_last_error()
        assert b"POLY6" in msg and b"RTPB_TABLE" in msg and b"variant 1" in msg and b"material 1" in msg
        surf2[2].kind = 17
        assert fn(*dict(ok, surfaces=ctypes.addressof(surf2)).values()) == C.RTPB_E_INVALID
        assert b"variant 2" in lib.rtpb_last_error() and b"unknown kind" in lib.rtpb_last_error()
        assert fn(*dict(ok, nsurf=C.RTPB_MAX_SURFACES + 1).values()) == C.RTPB_E_LIMIT
        assert b"RTPB_MAX_SURFACES" in lib.rtpb_last_error()
        big = np.zeros(65536, dtype=np.int32)
        assert fn(*dict(ok, n_groups=65536, group_variant=big.ctypes.data,
                        **(dict(workspace_len=1 << 40) if wave else {})).values()) == C.RTPB_E_LIMIT
        # 280 bytes per descriptor: 2^20 variants of 63 surfaces are 18 GB, beyond the 256 MiB of the header
        assert fn(*dict(ok, nsurf=63, n_variants=1 << 20).values()) == C.RTPB_E_LIMIT
        msg = lib.rtpb_last_error()
        assert b"RTPB_MAX_VARIANT_UPLOAD" in msg and what in msg
        # a good call reaches the device check and nothing else
        assert fn(*dict(ok, device=1 << 20).values()) in (C.RTPB_E_NODEV, C.RTPB_E_INVALID, C.RTPB_E_HIP)
        assert b"variant" not in lib.rtpb_last_error() and b"sweep" not in lib.rtpb_last_error()


def test_the_wavefront_upload_bound_counts_the_references():
    """The header's formula: 16 (n_a + n_b) + G (8 (4 S + 5) + 12) + 280 V S, plus 64 G + 8 for the wavefront call.
    With S = 1 and tables of 1 x 1 rays, V is the largest count the focus formula admits: the references' bytes put
    the wavefront calls over the cap, and they say so before a descriptor is read (only one exists here)."""
    lib = C.lib()
    cap = 256 << 20
    S, G = 1, 4
    base = 16 * (1 + 1) + G * (8 * (4 * S + 5) + 12)
    V = (cap - base) // 280                                   # the largest V the focus formula admits
    assert base + 280 * V <= cap < base + 280 * V + 64 * G + 8
    p = np.zeros(64).ctypes.data
    gv = np.zeros(G, dtype=np.int32)
    surf, mats = _systems(1)
    head = (ctypes.addressof(surf), S, ctypes.addressof(mats), V, 0, G, p, gv.ctypes.data)
    rc = lib.rtpb_wavefront_sweep_variants(*head, 1, 1, p, p, p, p, p, p, p, G * 15, p, None)
    assert rc == C.RTPB_E_LIMIT and b"RTPB_MAX_VARIANT_UPLOAD" in lib.rtpb_last_error()
    rc = lib.rtpb_wavefront_sweep_variants_collimated(*head, p, 1, 1, p, p, p, p, G * 15, p, None)
    assert rc == C.RTPB_E_LIMIT and b"RTPB_MAX_VARIANT_UPLOAD" in lib.rtpb_last_error()


def test_signatures_cover_the_four_calls():
    sig = C.SIGNATURES
    head = sig["rtpb_focus_sweep_variants"][1][:9]
    head = head[:4] + head[5:]                                   # no dtype: the calls are float64
    assert sig[WAVE[0]][1] == head + sig["rtpb_wavefront_sweep"][1][4:] and len(sig[WAVE[0]][1]) == 20
    assert sig[WAVE[1]][1] == head + sig["rtpb_wavefront_sweep_collimated"][1][4:] and len(sig[WAVE[1]][1]) == 18
    # the source's arguments (the wavefront sweep's up to refs), then rays_out and the stream
    assert sig[RAYS[0]][1] == head + sig["rtpb_wavefront_sweep"][1][4:11] + [ctypes.c_void_p] * 2
    assert sig[RAYS[1]][1] == head + sig["rtpb_wavefront_sweep_collimated"][1][4:9] + [ctypes.c_void_p] * 2
    for name in WAVE + RAYS:
        assert hasattr(C.lib(), name) and sig[name][0] is ctypes.c_int


def test_wrappers_refuse_bad_arguments_before_any_device_call(monkeypatch):
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    c2 = systems.c2_system(rt, mat)
    short = rt.System(c2.surfaces[:2] + c2.surfaces[-1:], c2.materials[:2])
    flat = c2.surfaces[0]
    long_ = rt.System([flat] * (C.RTPB_MAX_SURFACES + 1), [mat.Vacuum()] * C.RTPB_MAX_SURFACES)
    vac = mat.Vacuum()
    fan = ([[0.0, 0.0, -5.0]], [0.5, 0.6], 0.05, 5, 3)
    beam = ([[0.0, 0.0, 1.0]], [0.5, 0.6], 1.0, 5, 3)
    good = np.zeros((2, 1, 2, 8))
    for fn, src in ((analysis.variant_wavefront_sweep, fan), (analysis.collimated_variant_wavefront_sweep, beam)):
        with pytest.raises(ValueError, match="float64 only"):
            fn([c2, c2], vac, vac, *src, refs=good, dtype="float32")
        with pytest.raises(ValueError, match="systems is empty"):
            fn([], vac, vac, *src)
        with pytest.raises(ValueError, match="same, non-zero number of surfaces"):
            fn([c2, short], vac, vac, *src)
        with pytest.raises(ValueError, match="same, non-zero number of surfaces"):
            fn([rt.System([], [])], vac, vac, *src)
        with pytest.raises(ValueError, match="at most %d surfaces" % C.RTPB_MAX_SURFACES):
            fn([long_], vac, vac, *src)
        with pytest.raises(ValueError, match="devices= needs the fused sweep"):
            fn([c2, c2], vac, vac, *src, refs=good, fused=False, devices=[0])
        for bad in (np.zeros((1, 2, 8)), np.zeros((2, 2, 1, 8)), np.zeros((2, 1, 2, 7)), np.zeros((3, 1, 2, 8))):
            with pytest.raises(ValueError, match="refs must have shape 2 x 1 x 2 x 8"):
                fn([c2, c2], vac, vac, *src, refs=bad)
    with pytest.raises(ValueError, match="center_ray must be a unit vector"):
        analysis.variant_wavefront_sweep([c2], vac, vac, *fan, center_ray=(0, 0, 2))
    with pytest.raises(ValueError, match="normal must be a normalized vector"):
        analysis.collimated_variant_wavefront_sweep([c2], vac, vac, [[0.0, 0.1, 1.0]], [0.5], 1.0, 5, 3)
    for fn, src in ((analysis.variant_wavefront_refs, fan[:2]), (analysis.collimated_variant_wavefront_refs, beam[:2])):
        with pytest.raises(ValueError, match="systems is empty"):
            fn([], vac, vac, *src, spot_summary={"centroid": np.zeros((0, 1, 2, 3))})
        with pytest.raises(ValueError, match="spot_summary must be a variant_focus_sweep summary"):
            fn([c2, c2], vac, vac, *src, spot_summary={"centroid": np.zeros((1, 2, 3))})
    # good arguments with references reach the single driver once, with a wave mode over a variant source whose
    # entry point takes no dtype
    monkeypatch.setattr(analysis, "_sweep", lambda *a: ({"got": a}, {"seconds": 1.0}))
    out, timing = analysis.variant_wavefront_sweep([c2, c2, c2], vac, vac, *fan, refs=np.zeros((3, 1, 2, 8)))
    mode, system, _, _, src, _, dtype, gpb = out["got"][:8]
    assert system is None and (src.nf, src.nw, src.per, src.suffix, src.nsurf) == (3, 2, 15, "_variants", 5)
    assert mode.entry + src.suffix == "rtpb_wavefront_sweep_variants" and mode.ncols == 15 and dtype == "float64"
    assert timing["variants"] == 3 and timing["refs_seconds"] == 0.0 and "lower_seconds" in timing
    assert gpb == 6                                      # (all six groups: far below the upload and workspace bounds)
    low = src.lower(np.array([0.5, 0.6]), C.RTPB_F64)
    assert len(src.lead(low, 0, 6)) == 4 and src.lead(low, 2, 4)[3] == 1
    out, _ = analysis.collimated_variant_wavefront_sweep([c2, c2], vac, vac, *beam, refs=good)
    assert out["got"][4].suffix == "_variants_collimated" and out["got"][4].nf == 2


def test_the_default_batch_stays_under_the_upload_and_workspace_bounds():
    """_variant_batch with the wavefront sweep's 64 bytes more per group and 15 columns: the header's count of the
    largest batch, with every variant it can touch, stays under RTPB_MAX_VARIANT_UPLOAD, and its workspace under
    _sweep_plan's 2^26 doubles; the focus sweep's default is what it was."""
    cap = 256 << 20
    for V, S, nf, nw, per in ((2000, 5, 3, 3, 4096), (100000, 63, 1, 1, 64), (50000, 12, 9, 3, 1 << 20),
                              (7, 5, 2, 3, 1541)):
        b = analysis._variant_batch(V, S, nf, nw, per, 15, 64)
        assert 1 <= b <= min(V * nf * nw, 65535)
        variants = min(V, -(-b // (nf * nw)) + 1)               # a batch may start and end inside a variant
        count = 16 * (2 * per) + b * (8 * (4 * S + 5) + 12 + 72) + 280 * variants * S + 64 * b + 8
        assert count <= cap, (V, S, nf, nw, per, b, count)
        assert b * -(-per // 256) * 15 <= 1 << 26 or b == 1
        focus = analysis._variant_batch(V, S, nf, nw, per, 16)
        per_group = 8 * (4 * S + 5) + 12 + 72 + -(-280 * S // (nf * nw))
        was = max(1, min(V * nf * nw, 65535, cap // 2 // per_group, (1 << 26) // (-(-per // 256) * 16)))
        assert focus == (was - was % nw if was >= nw else was)


def test_variant_sources_share_one_lowering():
    """The refs pass and the sweep use one lowering of the systems: sources made with ``shared`` return the owner's
    lowered descriptors and add nothing to its lower_seconds."""
    c2 = systems.c2_system(rt, mat)
    moved = [analysis.rigid_move(c2, [1, 2, 3], shift=(0.01 * k, 0.0, 0.0)) for k in range(3)]
    vac = mat.Vacuum()
    wls = np.array([0.5, 0.6])
    inner = analysis._fan_source([[0.0, 0.0, -5.0]], wls, 0.05, 5, 3, (0, 0, 1))
    chief = analysis._fan_source([[0.0, 0.0, -5.0]], wls, 0.0, 1, 1, (0, 0, 1))
    owner = analysis._variant_source(moved, vac, vac, inner)
    a = analysis._variant_source(moved, vac, vac, chief, shared=owner, typed=False)
    b = analysis._variant_source(moved, vac, vac, inner, shared=owner, typed=False)
    low = a.lower(wls, C.RTPB_F64)
    took = owner.lower_seconds
    assert took > 0 and a.lower_seconds == 0
    assert b.lower(wls, C.RTPB_F64) is low and owner.lower(wls, C.RTPB_F64) is low and owner.lower_seconds == took
    assert (a.per, b.per) == (1, 15) and owner.lead(low, 0, 6)[:4] == a.lead(low, 0, 6)
    assert owner.lead(low, 0, 6)[4] == C.RTPB_F64


@pytest.mark.parametrize("name", vw.NAMES)
def test_the_oracle_answer_tells_the_variants_apart(name):
    """In each case no two variants of a live group give the same 15 sums, nor the same reference; the dead-chief
    groups (the off-axis field of the C2 cases' stopped-down variant, the C4 variant whose stop sits off the axis) have
    a NaN reference and count 0, and they are the only ones."""
    c = vc.case(name)
    o = vw.oracle(name)
    V = len(c.systems)
    assert o.sums.shape == (V, c.nf, len(c.wls), 15) and o.refs.shape == (V, c.nf, len(c.wls), 8)
    dead = np.isnan(o.refs).any(axis=-1)
    assert np.array_equal(dead, np.isnan(o.refs).all(axis=-1))
    assert np.array_equal(dead, ~np.isfinite(o.chief[..., :7]).all(axis=-1))
    assert (o.sums[dead] == 0).all()
    exp = np.zeros_like(dead)
    if name in ("c2_fan", "c2_beam"):
        # the stopped-down flat: the fan about (1, -2) lies wholly outside its aperture of 0.15, the beam about x = 6
        # outside 1; the same variant's axial field is cut, not killed
        exp[4, 1] = True
        assert (0 < o.sums[4, 0, :, 0]).all() and (o.sums[4, 0, :, 0] < o.sums[0, 0, :, 0]).all()
    else:
        exp[3] = True                   # the pupil stop 100 off the axis passes nothing
    assert np.array_equal(dead, exp)
    assert (o.sums[~dead][:, 0] > 0).all()
    for f in range(c.nf):
        for w in range(len(c.wls)):
            live = [v for v in range(V) if not dead[v, f, w]]
            for i, a in enumerate(live):
                for b in live[i + 1:]:
                    assert not np.array_equal(o.sums[a, f, w], o.sums[b, f, w]), (name, f, w, a, b)
                    assert not np.array_equal(o.refs[a, f, w], o.refs[b, f, w]), (name, f, w, a, b)
