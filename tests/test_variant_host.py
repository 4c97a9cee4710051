"""The variant sweeps on the host: the bundle-row key with the groups' variants and the upload layout
(csrc/rtpb_sweep_host.h through tests/sweep_rows.py), the argument checks of rtpb_focus_sweep_variants /
_variants_collimated (no GPU is touched) and their ctypes signatures, analysis.rigid_move, and what the Python wrappers
refuse before any device call."""
import ctypes

import numpy as np
import pytest

from ray_trace_pb_amd import _capi as C
from ray_trace_pb_amd import _engine as E
from ray_trace_pb_amd import analysis
import ray_trace_pb_amd.materials as mat
import ray_trace_pb_amd.raytrace as rt
from flat_plans import _systems
import sweep_rows
from sweep_rows import MAX_BUNDLE, RPL, native
import systems


def row_lists(params, frames=None, variants=None, trailing=2):
    """(bundles, rows, singles) of plan_sweep_rows as lists; ``trailing=1`` leaves its variant argument out,
    ``trailing=0`` its frames too."""
    return tuple(a.tolist() for a in sweep_rows.plan_rows(params, frames, variants, trailing=trailing))


def _mixed():
    """Three points (one of them twice, apart) with 1, 3, 9 and 2 wavelengths, in an order that is not the key's."""
    rng = np.random.default_rng(7)
    pts = np.array([[0.5, 0.0, -1.0], [-2.0, 1.0, -1.0], [0.0, 0.0, -1.0]])
    which = [1] + [0] * 3 + [2] * 9 + [1] * 2
    params = np.zeros((len(which), 4))
    params[:, :3] = pts[which]
    params[:, 3] = rng.uniform(0.4, 0.8, len(which))
    frames = rng.normal(size=(3, 9))[which]
    return params, frames


def test_rows_without_the_variant_argument_are_todays():
    """The call every other sweep makes -- no variant argument -- gives on a mixed input exactly the recorded rows,
    with and without frames (without them also with the frames left to their default, the fan sweeps' call); a NULL
    variant argument and one with all variants equal give them too."""
    params, frames = _mixed()
    # the rows the commit before the variant key gave on this input, recorded from its build (keys in the order of
    # their bit patterns: the point (0, 0, -1) first, then (0.5, 0, -1), then (-2, 1, -1))
    recorded = ([4, 5, 6, 7, 8, 9, 10, 11, 1, 2, 0, 13], [0, 8, 8, 2, 10, 2], [3, 12, 14])
    for fr in (None, frames):
        old = row_lists(params, fr, trailing=1)
        assert old == recorded
        if fr is None:
            assert row_lists(params, trailing=0) == old
        assert row_lists(params, fr, None) == old
        assert row_lists(params, fr, np.zeros(len(params))) == old
        assert row_lists(params, fr, np.full(len(params), 6)) == old
    # the point's rows, spelled out: nine wavelengths are a row of eight and a single, three a row of two and a single
    bundles, rows, singles = row_lists(params, None, trailing=1)
    assert sorted(rows[1::2]) == [2, 2, 8] and sorted(bundles + singles) == list(range(len(params)))


def test_no_bundle_row_mixes_variants_and_every_group_appears_once():
    params, frames = _mixed()
    G = len(params)
    rng = np.random.default_rng(11)
    for fr in (None, frames):
        for variants in (np.arange(G) % 2, np.arange(G) % 3, rng.integers(0, 4, G), np.arange(G)):
            bundles, rows, singles = row_lists(params, fr, variants)
            assert sorted(bundles + singles) == list(range(G))
            assert singles == sorted(singles) and len(rows) % 2 == 0
            offs, lens = rows[0::2], rows[1::2]
            assert offs == np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(int).tolist() if rows else True
            assert sum(lens) == len(bundles)
            for o, n in zip(offs, lens):
                gs = bundles[o:o + n]
                assert RPL <= n <= MAX_BUNDLE and n % RPL == 0
                assert len({int(variants[g]) for g in gs}) == 1, "a row with two variants"
                assert len({params[g, :3].tobytes() for g in gs}) == 1
                if fr is not None:
                    assert len({fr[g].tobytes() for g in gs}) == 1
    # one variant per group: nothing can share a row
    assert row_lists(params, None, np.arange(G))[1] == []
    # the sweep's own order, group = (variant * fields + field) * wavelengths + wavelength: a row per (variant, field)
    V, nf, nw = 3, 2, 3
    p = np.zeros((V * nf * nw, 4))
    p[:, 0] = np.tile(np.repeat([0.0, 1.0], nw), V)
    p[:, 3] = np.tile([0.5, 0.6, 0.7], V * nf)
    bundles, rows, singles = row_lists(p, None, np.repeat(np.arange(V), nf * nw))
    assert rows[1::2] == [2] * (V * nf) and len(singles) == V * nf
    assert row_lists(p, None, trailing=1)[1][1::2] == [8, 8]          # (the point alone would merge the variants)


def test_upload_layout_keeps_its_offsets_and_places_the_descriptors():
    lib = native()

    def layout(*a):
        out = np.zeros(8, dtype=np.int64)
        lib.variant_sweep_layout(*a, out.ctypes.data)
        return dict(zip("grp gn img win frm dsc idx bytes".split(), out.tolist()))
    n_a, n_b, G, media, n_idx = 67, 23, 30, 21, 45
    for frames in (0, 9):
        plain = layout(n_a, n_b, G, media, n_idx, frames, 0)
        assert plain["grp"] == 16 * (n_a + n_b) and plain["gn"] == plain["grp"] + 32 * G
        assert plain["frm"] == plain["gn"] + 8 * media * G and plain["idx"] == plain["frm"] + 8 * frames * G
        assert plain["dsc"] == plain["idx"] and plain["bytes"] == plain["idx"] + 4 * n_idx
        desc = 5 * 5 * 280
        var = layout(n_a, n_b, G, media, n_idx + G, frames, desc)
        assert {k: var[k] for k in ("grp", "gn", "img", "win", "frm", "dsc")} == \
            {k: plain[k] for k in ("grp", "gn", "img", "win", "frm", "dsc")}
        assert var["dsc"] % 8 == 0 and var["idx"] == var["dsc"] + desc and var["bytes"] == var["idx"] + 4 * (n_idx + G)


def test_entry_points_validate_without_a_gpu():
    """Every refusal of include/rtpb.h, before any device work (the data pointers here are host memory; the device
    index of the last call names no device): NULL pointers, non-positive sizes and a short workspace are
    RTPB_E_INVALID with the focus sweeps' messages, a group_variant entry out of range RTPB_E_INVALID naming the
    group, a POLY6 material RTPB_E_INVALID saying RTPB_TABLE, a bad descriptor RTPB_E_INVALID naming the variant;
    nsurf > RTPB_MAX_SURFACES, more than 65535 groups and an upload beyond the stated cap RTPB_E_LIMIT."""
    lib = C.lib()
    assert lib.rtpb_abi_version() == 10 == C.RTPB_ABI_VERSION
    buf = np.zeros(1 << 16)
    p = buf.ctypes.data
    V, G, tiles = 3, 4, 2                     # 30 x 10 rays: two tiles
    surf, mats = _systems(V)
    gv = np.array([0, 2, 1, 2], dtype=np.int32)
    head = dict(surfaces=ctypes.addressof(surf), nsurf=1, materials=ctypes.addressof(mats), n_variants=V,
                dtype=C.RTPB_F64, device=0, n_groups=G, group_params=p, group_variant=gv.ctypes.data)
    tail = dict(workspace=p, workspace_len=G * tiles * 16, stats_out=p, stream=None)
    calls = {"rtpb_focus_sweep_variants": dict(head, n_thetas=30, nphis=10, center_ray=p, ex=p, ey=p,
                                               theta_cos_sin=p, phi_cos_sin=p, **tail),
             "rtpb_focus_sweep_variants_collimated": dict(head, group_frames=p, n_disps=30, nphis=10, offsets=p,
                                                          phi_cos_sin=p, **tail)}
    for name, ok in calls.items():
        fn = getattr(lib, name)
        fan = "n_thetas" in ok
        sizes = ("n_thetas", "nphis") if fan else ("n_disps", "nphis")
        ptrs = ("center_ray", "ex", "ey", "theta_cos_sin", "phi_cos_sin") if fan else \
            ("group_frames", "offsets", "phi_cos_sin")
        for bad in [dict(surfaces=None), dict(materials=None), dict(group_variant=None), dict(nsurf=0),
                    dict(nsurf=-1), dict(n_variants=0), dict(n_variants=-5)]:
            assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, (name, bad)
            assert b"bad focus-sweep-variants arguments" in lib.rtpb_last_error(), (name, bad)
        bads = [dict(group_params=None), dict(workspace=None), dict(stats_out=None), dict(n_groups=0),
                dict(n_groups=-1)] + [{k: None} for k in ptrs] + [{k: 0} for k in sizes] + [{k: -2} for k in sizes]
        for bad in bads:
            assert fn(*dict(ok, **bad).values()) == C.RTPB_E_INVALID, (name, bad)
            assert b"bad focus-sweep arguments" in lib.rtpb_last_error(), (name, bad)
        assert fn(*dict(ok, dtype=2).values()) == C.RTPB_E_INVALID
        assert b"dtype must be" in lib.rtpb_last_error()
        assert fn(*dict(ok, workspace_len=G * tiles * 16 - 1).values()) == C.RTPB_E_INVALID
        msg = lib.rtpb_last_error()
        assert b"workspace too small" in msg and b"* 16 doubles" in msg
        assert (b"n_thetas*nphis" if fan else b"n_disps*nphis") in msg
        # a group_variant entry out of range, either side: the message names the group
        for g, v in ((1, V), (3, -1), (0, 1 << 30)):
            bad_gv = gv.copy()
            bad_gv[g] = v
            assert fn(*dict(ok, group_variant=bad_gv.ctypes.data).values()) == C.RTPB_E_INVALID
            assert b"group %d " % g in lib.rtpb_last_error() and b"variant" in lib.rtpb_last_error()
        # a POLY6 material in any variant
        surf2, mats2 = _systems(V)
        mats2[2 * 1 + 1].kind = C.RTPB_POLY6
        assert fn(*dict(ok, materials=ctypes.addressof(mats2)).values()) == C.RTPB_E_INVALID
        msg = lib.rtpb_last_error()
        assert b"POLY6" in msg and b"RTPB_TABLE" in msg and b"variant 1" in msg and b"material 1" in msg
        # a descriptor rtpb_plan_create would refuse, with its message and the variant
        surf2[2].kind = 17
        assert fn(*dict(ok, surfaces=ctypes.addressof(surf2)).values()) == C.RTPB_E_INVALID
        assert b"variant 2" in lib.rtpb_last_error() and b"unknown kind" in lib.rtpb_last_error()
        mats3 = _systems(V)[1]
        mats3[0].kind = C.RTPB_TABLE
        assert fn(*dict(ok, materials=ctypes.addressof(mats3)).values()) == C.RTPB_E_INVALID
        assert b"variant 0" in lib.rtpb_last_error() and b"empty table" in lib.rtpb_last_error()
        # the limits (checked before any descriptor is read: these counts describe arrays that do not exist)
        assert fn(*dict(ok, nsurf=C.RTPB_MAX_SURFACES + 1).values()) == C.RTPB_E_LIMIT
        assert b"RTPB_MAX_SURFACES" in lib.rtpb_last_error()
        big = np.zeros(65536, dtype=np.int32)
        assert fn(*dict(ok, n_groups=65536, group_variant=big.ctypes.data,
                        workspace_len=1 << 40).values()) == C.RTPB_E_LIMIT
        assert fn(*dict(ok, **{sizes[0]: 1 << 31, sizes[1]: 1 << 10}, workspace_len=1 << 60).values()) == \
            C.RTPB_E_LIMIT
        # 280 bytes per descriptor: 2^20 variants of 63 surfaces are 18 GB, beyond the 256 MiB of the header
        assert fn(*dict(ok, nsurf=63, n_variants=1 << 20).values()) == C.RTPB_E_LIMIT
        assert b"RTPB_MAX_VARIANT_UPLOAD" in lib.rtpb_last_error()
        # ... and just inside it the call goes on to read the descriptors (here: 3 real ones, then a bad count caught
        # as a bad variant is -- so stay with the real arrays): a good call reaches the device check and nothing else
        assert fn(*dict(ok, device=1 << 20).values()) in (C.RTPB_E_NODEV, C.RTPB_E_INVALID, C.RTPB_E_HIP)
        assert b"variant" not in lib.rtpb_last_error() and b"sweep" not in lib.rtpb_last_error()


def test_signatures_cover_the_variant_calls():
    fan, beam = C.SIGNATURES["rtpb_focus_sweep_variants"][1], C.SIGNATURES["rtpb_focus_sweep_variants_collimated"][1]
    # the head (surfaces, nsurf, materials, n_variants, dtype, device, n_groups, group_params, group_variant), then
    # rtpb_focus_sweep's arguments from n_thetas (rtpb_focus_sweep_collimated's from group_frames)
    assert len(fan) == 9 + len(C.SIGNATURES["rtpb_focus_sweep"][1]) - 4 == 20
    assert len(beam) == 9 + len(C.SIGNATURES["rtpb_focus_sweep_collimated"][1]) - 4 == 18
    assert fan[9:] == C.SIGNATURES["rtpb_focus_sweep"][1][4:]
    assert beam[9:] == C.SIGNATURES["rtpb_focus_sweep_collimated"][1][4:]
    assert fan[:9] == beam[:9]
    for name in ("rtpb_focus_sweep_variants", "rtpb_focus_sweep_variants_collimated"):
        assert hasattr(C.lib(), name) and C.SIGNATURES[name][0] is ctypes.c_int


def _lowered(system, m0=None, m1=None):
    m0, m1 = m0 or mat.Vacuum(), m1 or mat.Vacuum()
    return E._lower(system.surfaces, [m0] + list(system.materials) + [m1], lambda: np.array([0.5]), C.RTPB_F64)


def _codes(system):
    lib, low = native(), _lowered(system)
    return [lib.variant_surface_code(ctypes.byref(low.surfaces[k])) for k in range(low.nsurf)]


def _snapshot(system):
    return [(type(s), {k: np.array(v, copy=True) for k, v in vars(s).items()}) for s in system.surfaces]


def _same_snapshot(a, b):
    return len(a) == len(b) and all(
        ta is tb and da.keys() == db.keys() and all(np.array_equal(da[k], db[k]) and
                                                    np.asarray(da[k]).tobytes() == np.asarray(db[k]).tobytes()
                                                    for k in da)
        for (ta, da), (tb, db) in zip(a, b))


def test_rigid_move_zero_is_the_same_descriptors_bit_for_bit():
    for system in (systems.c2_system(rt, mat), systems.c4_system(rt, mat), systems.stress_system(rt, mat)):
        n = len(system.surfaces)
        before = _snapshot(system)
        moved = analysis.rigid_move(system, range(n))
        also = analysis.rigid_move(system, [1, 2], shift=(0.0, -0.0, 0.0), tilt=(0.0, -0.0), pivot=(1.0, 2.0, 3.0))
        for m in (moved, also):
            assert bytes(_lowered(m).surfaces) == bytes(_lowered(system).surfaces)
            assert m is not system and m.materials == system.materials and m.materials is not system.materials
        assert all(a is not b for a, b in zip(moved.surfaces, system.surfaces))
        assert also.surfaces[0] is system.surfaces[0] and also.surfaces[1] is not system.surfaces[1]
        assert _same_snapshot(before, _snapshot(system))


def test_rigid_move_shift_moves_center_only_and_leaves_the_input_alone():
    system = systems.c2_system(rt, mat)
    before = _snapshot(system)
    ref = _lowered(system)
    shift = np.array([0.3, -0.2, 0.05])
    moved = analysis.rigid_move(system, [1, 2, 3], shift=shift)
    assert _same_snapshot(before, _snapshot(system)), "the input system changed"
    assert bytes(_lowered(system).surfaces) == bytes(ref.surfaces)
    low = _lowered(moved)
    for k in range(5):
        a, b = ref.surfaces[k], low.surfaces[k]
        exp = np.array(a.center[:]) + (shift if k in (1, 2, 3) else 0.0)
        assert np.array_equal(np.array(b.center[:]), exp), k
        b.center[:] = a.center[:]
        assert bytes(b) == bytes(a), "a shift changed more than the center of surface %d" % k
    assert moved.surfaces[0] is system.surfaces[0] and moved.surfaces[4] is system.surfaces[4]
    for k in (1, 2, 3):
        assert np.array_equal(moved.surfaces[k].paraxial_center, system.surfaces[k].paraxial_center + shift)


def test_rigid_move_tilt_rotates_the_body_about_its_pivot():
    system = systems.c2_system(rt, mat)
    ax, ay = 0.01, -0.02
    moved = analysis.rigid_move(system, [1, 2, 3], tilt=(ax, ay))
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rot = ry @ rx                                       # about x, then about y
    pivot = system.surfaces[1].center
    for k in (1, 2, 3):
        s, m = system.surfaces[k], moved.surfaces[k]
        assert np.allclose(m.center, pivot + rot @ (s.center - pivot), rtol=0, atol=1e-12)
        assert np.allclose(m.input_axis, rot @ s.input_axis, rtol=0, atol=1e-15)
        assert abs(np.linalg.norm(m.input_axis) - 1) < 1e-15
        # rigid: distances within the body are kept
        assert abs(np.linalg.norm(m.center - moved.surfaces[1].center) -
                   np.linalg.norm(s.center - system.surfaces[1].center)) < 1e-12
    assert np.array_equal(moved.surfaces[1].center, system.surfaces[1].center)          # the pivot stays
    other = analysis.rigid_move(system, [0], tilt=(0.0, 0.1), pivot=(0.0, 0.0, 10.0))
    assert np.allclose(other.surfaces[0].normal, [np.sin(0.1), 0, np.cos(0.1)], atol=1e-15)
    assert np.allclose(other.surfaces[0].center, [-10 * np.sin(0.1), 0, 10 - 10 * np.cos(0.1)], atol=1e-12)
    for bad in (dict(surfaces=[]), dict(surfaces=[5]), dict(surfaces=[0], shift=(1, 2)),
                dict(surfaces=[0], tilt=(1, 2, 3)), dict(surfaces=[0], pivot=(0, 0))):
        with pytest.raises(ValueError, match="rigid_move"):
            analysis.rigid_move(system, **bad)


def test_a_decentred_axial_sphere_lowers_to_the_general_form():
    """The library's own lowering (lower_surface, surface_code) on the Python side's descriptors: C2's spheres and
    flats are axial (code 3 * kind + 1); decentred spheres are general (3 * kind), the surfaces that did not move
    keep their form, and a tilted flat is general too.  So one variant call holds both forms of a surface."""
    system = systems.c2_system(rt, mat)
    FLAT, SPHERE = 3 * C.RTPB_FLAT, 3 * C.RTPB_SPHERE
    assert _codes(system) == [FLAT + 1, SPHERE + 1, SPHERE + 1, SPHERE + 1, FLAT + 1]
    assert _codes(analysis.rigid_move(system, [1, 2, 3], shift=(0.3, -0.2, 0.0))) == \
        [FLAT + 1, SPHERE, SPHERE, SPHERE, FLAT + 1]
    assert _codes(analysis.rigid_move(system, [1, 2, 3], shift=(0.0, 0.0, 0.5))) == _codes(system)     # despaced
    assert _codes(analysis.rigid_move(system, [0, 1, 2, 3], tilt=(0.004, -0.007))) == \
        [FLAT, SPHERE, SPHERE, SPHERE, FLAT + 1]
    assert _codes(analysis.rigid_move(system, [0], tilt=(0.0, 0.01))) == [FLAT + 2, SPHERE + 1, SPHERE + 1,
                                                                           SPHERE + 1, FLAT + 1]     # in the x-z plane


def test_wrappers_refuse_bad_systems_before_any_device_call(monkeypatch):
    monkeypatch.setattr(C, "lib", lambda: pytest.fail("a device call"))
    monkeypatch.setattr(analysis, "_sweep", lambda *a: pytest.fail("the sweep"))
    c2 = systems.c2_system(rt, mat)
    short = rt.System(c2.surfaces[:2] + c2.surfaces[-1:], c2.materials[:2])
    no_plane = rt.System(c2.surfaces[:4] + c2.surfaces[3:4], c2.materials)          # (ends on a sphere)
    vac = mat.Vacuum()
    fan = ([[0.0, 0.0, -5.0]], [0.5, 0.6], 0.05, 5, 3)
    beam = ([[0.0, 0.0, 1.0]], [0.5, 0.6], 1.0, 5, 3)
    for fn, src in ((analysis.variant_focus_sweep, fan), (analysis.collimated_variant_focus_sweep, beam)):
        with pytest.raises(ValueError, match="systems is empty"):
            fn([], vac, vac, *src)
        with pytest.raises(ValueError, match="same, non-zero number of surfaces"):
            fn([c2, short], vac, vac, *src)
        with pytest.raises(ValueError, match="same, non-zero number of surfaces"):
            fn([rt.System([], [])], vac, vac, *src)
        with pytest.raises(ValueError, match="append an image plane"):
            fn([c2, no_plane, no_plane], vac, vac, *src)
        with pytest.raises(ValueError, match="devices= needs the fused sweep"):
            fn([c2, c2], vac, vac, *src, fused=False, devices=[0])
    with pytest.raises(ValueError, match="center_ray must be a unit vector"):
        analysis.variant_focus_sweep([c2], vac, vac, *fan, center_ray=(0, 0, 2))
    with pytest.raises(ValueError, match="normal must be a normalized vector"):
        analysis.collimated_variant_focus_sweep([c2], vac, vac, [[0.0, 0.1, 1.0]], [0.5], 1.0, 5, 3)
    # good arguments reach the driver with a variant source: the systems' groups side by side
    monkeypatch.setattr(analysis, "_sweep", lambda *a: ({"got": a}, {"seconds": 1.0}))
    out, timing = analysis.variant_focus_sweep([c2, c2, c2], vac, vac, *fan)
    mode, system, _, _, src = out["got"][:5]
    assert system is None and (src.nf, src.nw, src.per, src.suffix, src.nsurf) == (3, 2, 15, "_variants", 5)
    assert mode.entry + src.suffix == "rtpb_focus_sweep_variants" and timing["variants"] == 3
    out, _ = analysis.collimated_variant_focus_sweep([c2, c2], vac, vac, *beam)
    assert out["got"][4].suffix == "_variants_collimated" and out["got"][4].nf == 2


def test_variant_source_passes_each_batch_its_own_variants():
    """A batch that starts inside the variant list gets the descriptors from its first variant on and group_variant
    counted from there; the group parameters are the inner source's, once per variant."""
    c2 = systems.c2_system(rt, mat)
    moved = [analysis.rigid_move(c2, [1, 2, 3], shift=(0.01 * k, 0.0, 0.0)) for k in range(4)]
    vac = mat.Vacuum()
    inner = analysis._fan_source([[0.0, 0.0, -5.0], [1.0, 0.0, -5.0]], [0.5, 0.6, 0.7], 0.05, 5, 3, (0, 0, 1))
    src = analysis._variant_source(moved, vac, vac, inner)
    low = src.lower(np.array([0.5, 0.6, 0.7]), C.RTPB_F64)
    assert src.lower_seconds > 0
    S = 5
    for v, s in enumerate(moved):
        one = _lowered(s)
        assert bytes(low.surf)[v * low.ns:(v + 1) * low.ns] == bytes(one.surfaces)
        assert bytes(low.mats)[v * low.nm:(v + 1) * low.nm] == bytes(one.materials)
    head = src.head()
    for b0, b1, v0, nv in ((0, 24, 0, 4), (9, 18, 1, 2), (7, 8, 1, 1), (6, 13, 1, 2), (15, 24, 2, 2)):
        lead = src.lead(low, b0, b1)
        assert lead == (ctypes.addressof(low.surf) + v0 * low.ns, S, ctypes.addressof(low.mats) + v0 * low.nm, nv,
                        C.RTPB_F64)
        args, keep = head(b0, b1)
        gv = np.ctypeslib.as_array(ctypes.cast(args[1], ctypes.POINTER(ctypes.c_int32)), (b1 - b0,))
        assert gv.tolist() == [g // 6 - v0 for g in range(b0, b1)] and 0 <= gv.min() and gv.max() == nv - 1
        gp = np.ctypeslib.as_array(ctypes.cast(args[0], ctypes.POINTER(ctypes.c_double)), (b1 - b0, 4))
        exp = [[float((g % 6) // 3), 0.0, -5.0, [0.5, 0.6, 0.7][g % 3]] for g in range(b0, b1)]
        assert gp.tolist() == exp
        assert args[2:4] == (5, 3)
        del keep
