"""The single-surface and ray-utility kernels behind rtpb_propagate_plane, rtpb_front_side, rtpb_interact and
rtpb_intersect_rays (include/rtpb.h), called through the C ABI on sentinel-padded device buffers in both storage
types and compared bit for bit (NaN pattern included) with expectations that involve no device output:

  * the NumPy oracle (oracle/rt_numpy.py: to_plane, snell, mirror, refractive_index) for the three tile kernels,
  * the package's NumPy intersect_rays (pinned to the reference's golden vectors by tests/test_api.py).

float32 storage: the inputs are widened exactly, the arithmetic is float64 and each stored value is rounded once,
so the expectation is the oracle on x.astype(float32).astype(float64), then .astype(float32); ts_out is float64
and compared unrounded; table keys are the widened wavelengths.

Sizes straddle the 64-ray tile (a float32 tile is half full) and the 256-thread block; every input is the first
n rows of one 4200-row pool, taken as built and after a roll, so the hand-placed odd rows visit other lanes.
Every output is a slice big[PAD : PAD + n] of a sentinel-filled tensor whose other rows must stay untouched.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ray_trace_pb_amd.materials as mat  # noqa: E402
import ray_trace_pb_amd.raytrace as rt  # noqa: E402
from ray_trace_pb_amd import _capi as C  # noqa: E402
from ray_trace_pb_amd import _engine as E  # noqa: E402
from oracle import rt_numpy as O  # noqa: E402
from parity import same_bits  # noqa: E402
from serialize import material_to_dict  # noqa: E402
import systems  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 13                    # sentinel rows before and after every output (13 rows of 32 or 64 bytes keep 16-byte alignment)
SENTINEL = 12345.0
WS_PAD, WS_FILL = 256, 0xA5  # sentinel bytes around the propagate-plane workspace
CODES = [C.RTPB_F64, C.RTPB_F32]
CODE_ID = {C.RTPB_F64: "f64", C.RTPB_F32: "f32"}
TORCH_DT = {C.RTPB_F64: torch.float64, C.RTPB_F32: torch.float32}
NP_DT = {C.RTPB_F64: np.float64, C.RTPB_F32: np.float32}
NPOOL = 4200
ROLL = 37                   # rows the pools are rolled by: the hand-placed rows 0..20 move to lanes 37..57
TILE_SIZES = (1, 63, 64, 65, 127, 128, 129, NPOOL)      # 64-ray tiles
BLOCK_SIZES = (1, 255, 256, 257, NPOOL)                  # 256-thread blocks
# the broadcast plane of the propagate-plane cases, in float32 numbers (the normal is not a unit vector, which
# propagate_ray2plane does not ask for): 0.75 * 0.5 - 0.5 * 0.75 is exact, so directions with d . N0 == 0 exist in both
# storage types
N0 = np.array([0.0, 0.5, 0.75])
C0 = np.array([0.5, -0.25, -6.0])


# ----------------------------------------------------------------------------------------- helpers
def _widen(x, code):
    return x if code == C.RTPB_F64 else x.astype(np.float32).astype(np.float64)


def _store(x, code):
    """A float64 expectation as the storage type holds it: rounded once."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(NP_DT[code]))


def _to_dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)       # (a copy: the pools are read-only)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _padded(n, cols, tdt):
    """(big, view): a sentinel-filled (n + 2 PAD [, cols]) tensor and its rows PAD .. PAD + n."""
    shape = (n + 2 * PAD,) if cols is None else (n + 2 * PAD, cols)
    big = torch.full(shape, SENTINEL, dtype=tdt, device=DEV)
    return big, big[PAD:PAD + n]


def _pad_ok(big, n):
    h = big.cpu().numpy()
    return bool((h[:PAD] == SENTINEL).all() and (h[PAD + n:] == SENTINEL).all())


def _variants(n_sizes):
    """(roll, n) for every size, on the pool as built and rolled."""
    return list(itertools.product((0, ROLL), n_sizes))


def _rolled(a, roll):
    return np.roll(a, roll, axis=0) if roll else a


def _oracle_n(m):
    d = material_to_dict(m)

    def n_of(wl):
        with np.errstate(all="ignore"):
            return np.asarray(O.refractive_index(d, wl), dtype=np.float64)
    return n_of


def _table_n(keys, vals):
    """Exact-match lookup in a caller's (key, value) table: NaN finds a NaN key, a wavelength that is no key gets NaN."""
    def n_of(wl):
        out = np.full(np.shape(wl), np.nan)
        for k, v in zip(keys, vals):
            out[np.isnan(wl) if np.isnan(k) else wl == k] = v
        return out
    return n_of


def _table_material(keys, vals):
    d = C.Material()
    tab = np.ascontiguousarray(np.stack((keys, vals), axis=1).ravel())
    d.kind = C.RTPB_TABLE
    d.table_len = len(keys)
    d.table = tab.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    d._keep = tab
    return d


def _rays_of(a):
    return O.Rays.from_array(a)


def _unit_rows(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


# ----------------------------------------------------------------------------------------- pools
@functools.lru_cache(maxsize=None)
def _ray_pool():
    """stress_rays (zero direction, a ray parallel to the first flat, NaN wavelength, an all-NaN row in rows 0..7)
    plus hand-placed rows 8..15 for the plane (N0, C0): starts on the plane with d . N0 > 0 (t = -0) and < 0
    (t = +0), d . N0 == 0 off the plane (t = +-inf) in both orders of the cancelling products, an infinite position,
    wavelength 0 (n of Vacuum is NaN there), a ray on the plane with d . N0 == 0 (t = NaN)."""
    rays = systems.stress_rays(NPOOL, seed=21)
    hand = np.array([[*C0, 0.0, 0.0, 1.0, 1.5, 0.5],
                     [*C0, 0.0, 0.0, -1.0, 1.5, 0.6328],
                     [1.0, 2.0, -9.0, 1.0, 0.0, 0.0, 2.5, 1.0],
                     [1.0, 2.0, -3.0, 0.0, 0.75, -0.5, 2.5, 0.405],
                     [np.inf, 0.0, -10.0, 0.0, 0.0, 1.0, 0.25, 0.5],
                     [0.5, 0.5, -10.0, 0.0, 0.0, 1.0, 3.0, 0.0],
                     [*C0, 1.0, 0.0, 0.0, 0.0, 0.5],
                     [0.0, 0.0, -10.0, 0.0, -0.5, -0.75, 4.0, 1.0]])
    rays[8:8 + len(hand)] = hand
    rays.setflags(write=False)
    return rays


HAND = slice(8, 16)


@functools.lru_cache(maxsize=None)
def _plane_pool():
    """Per-ray plane normals (half near +z with std 0.4 transverse, half isotropic) and centers around the rays'
    start (z = -8 +- 2 against the rays' -10 +- 1: a good part of the planes lies behind its ray); the hand-placed
    rows get the broadcast plane, so they are special in all four per-ray / broadcast combinations."""
    rng = np.random.default_rng(211)
    near = np.stack((rng.normal(scale=0.4, size=NPOOL), rng.normal(scale=0.4, size=NPOOL), np.ones(NPOOL)), axis=1)
    iso = rng.normal(size=(NPOOL, 3))
    nrm = _unit_rows(np.where((np.arange(NPOOL) % 2 == 0)[:, None], near, iso))
    ctr = np.stack((rng.normal(scale=3.0, size=NPOOL), rng.normal(scale=3.0, size=NPOOL),
                    -8.0 + rng.normal(scale=2.0, size=NPOOL)), axis=1)
    nrm[HAND], ctr[HAND] = N0, C0
    nrm.setflags(write=False)
    ctr.setflags(write=False)
    return nrm, ctr


@functools.lru_cache(maxsize=None)
def _hit_pool():
    """The `hits` of the hook kernels: another bundle than _ray_pool (a kernel that reads the wrong one fails),
    with its own odd rows."""
    hits = systems.stress_rays(NPOOL, seed=22)
    hits[:, 0:3] += np.random.default_rng(22).normal(scale=0.5, size=(NPOOL, 3))
    hits[8] = [np.inf, 0.0, 1.0, 0.0, 0.0, 1.0, 0.5, 0.5]
    hits[9] = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.0, 0.405]
    hits.setflags(write=False)
    return hits


@functools.lru_cache(maxsize=None)
def _normal_pool():
    """get_normal results for _ray_pool used as hits: half near +z (std 0.4 transverse), half isotropic, and by hand
    a normal exactly equal to the direction (normal incidence, zero cross product), its negative, a zero normal and
    a NaN normal -- on rows whose direction is a plain unit vector."""
    rng = np.random.default_rng(212)
    near = np.stack((rng.normal(scale=0.4, size=NPOOL), rng.normal(scale=0.4, size=NPOOL), np.ones(NPOOL)), axis=1)
    iso = rng.normal(size=(NPOOL, 3))
    nrm = _unit_rows(np.where((np.arange(NPOOL) % 2 == 0)[:, None], near, iso))
    d = _ray_pool()[:, 3:6]
    nrm[16], nrm[17] = d[16], -d[17]
    nrm[18] = 0.0
    nrm[19] = np.nan
    nrm[20] = [0.0, np.nan, 1.0]
    nrm[0] = d[0]                  # the on-axis ray of stress_rays at normal incidence on (0, 0, 1)
    nrm.setflags(write=False)
    return nrm


@functools.lru_cache(maxsize=None)
def _on_pool():
    """is_pt_on_surface results as bytes: about 10 % zeros; the others are any non-zero byte."""
    rng = np.random.default_rng(213)
    on = rng.choice(np.array([1, 1, 1, 2, 128, 255], dtype=np.uint8), size=NPOOL)
    on[rng.random(NPOOL) < 0.10] = 0
    on.setflags(write=False)
    return on


def _keys(col):
    return np.asarray(E.distinct_wavelengths(col), dtype=np.float64)


# ----------------------------------------------------------------------------------------- rtpb_propagate_plane
def _zero_sellmeier(keys):
    d = C.Material()
    d.kind = C.RTPB_SELLMEIER
    return d


def _descending_missing(keys):
    """The Cauchy table handed over in descending key order (NaN first) without the colour 0.6328."""
    drop = keys[np.nanargmin(np.abs(keys - 0.6328))]
    assert abs(drop - 0.6328) < 1e-6
    kept = keys[keys != drop][::-1].copy()
    with np.errstate(all="ignore"):
        vals = np.asarray(systems.cauchy_class(mat)().n(kept), dtype=np.float64)
    return kept, vals, drop


def _lowered(m):
    def build(keys):
        with np.errstate(all="ignore"):
            return E.lower_material(m, lambda: keys)
    return build


PLANE_MATERIALS = {
    "constant": lambda: (_lowered(mat.Constant(1.33)), lambda keys: _oracle_n(mat.Constant(1.33))),
    "vacuum": lambda: (_lowered(mat.Vacuum()), lambda keys: _oracle_n(mat.Vacuum())),
    "bk7": lambda: (_lowered(mat.Bk7()), lambda keys: _oracle_n(mat.Bk7())),
    "zero_sellmeier": lambda: (_zero_sellmeier, lambda keys: _oracle_n(mat.Vacuum())),
    "ebaf11_table": lambda: (_lowered(mat.Ebaf11()), lambda keys: _oracle_n(mat.Ebaf11())),
    "cauchy_table": lambda: (_lowered(systems.cauchy_class(mat)()), lambda keys: _oracle_n(systems.cauchy_class(mat)())),
    "descending_missing_key": lambda: ((lambda keys: _table_material(*_descending_missing(keys)[:2])),
                                       (lambda keys: _table_n(*_descending_missing(keys)[:2]))),
}
PLANE_KINDS = {"constant": C.RTPB_CONSTANT, "vacuum": C.RTPB_SELLMEIER, "bk7": C.RTPB_SELLMEIER,
               "zero_sellmeier": C.RTPB_SELLMEIER, "ebaf11_table": C.RTPB_TABLE, "cauchy_table": C.RTPB_TABLE,
               "descending_missing_key": C.RTPB_TABLE}


def _plane_expect(rays_w, nrm, ctr, n_vals, exclude):
    out, t = O.to_plane(_rays_of(rays_w), O._bcast3(nrm, len(rays_w)), O._bcast3(ctr, len(rays_w)), n_vals, exclude)
    return out.to_array(), np.asarray(t, dtype=np.float64)


def _workspace(table_len):
    """The documented minimum, 256 + 16 * max(table_len, 1) bytes, between sentinel bytes."""
    need = 256 + 16 * max(table_len, 1)
    big = torch.full((need + 2 * WS_PAD,), WS_FILL, dtype=torch.uint8, device=DEV)
    return big, big[WS_PAD:WS_PAD + need], need


def _ws_ok(big, need):
    h = big.cpu().numpy()
    return bool((h[:WS_PAD] == WS_FILL).all() and (h[WS_PAD + need:] == WS_FILL).all())


def _plane_setup(code, material, roll):
    """Inputs, lowered material and the oracle's answer for all eight flag combinations on the whole pool, with the
    coverage the comparison needs asserted on the oracle side.  No device work."""
    build, n_for = PLANE_MATERIALS[material]()
    nrm_pool, ctr_pool = _plane_pool()
    rays_w = _widen(_rolled(_ray_pool(), roll), code)
    nrm_pr, ctr_pr = _rolled(nrm_pool, roll), _rolled(ctr_pool, roll)
    wl = rays_w[:, 7]
    keys = _keys(wl)
    low = build(keys)
    assert low.kind == PLANE_KINDS[material]
    n_vals = n_for(keys)(wl)
    odd_wl = (wl == 0) | np.isnan(wl)
    if material in ("vacuum", "zero_sellmeier"):
        # n of the all-zero Sellmeier: 1, and NaN at wavelength 0 and NaN
        assert (wl == 0).any() and np.isnan(wl).any()
        assert np.isnan(n_vals[odd_wl]).all() and (n_vals[~odd_wl] == 1.0).all()
    plain = ~np.isnan(rays_w).any(axis=1) & ~odd_wl
    expects = {}
    for n_per, c_per, exclude in itertools.product((0, 1), (0, 1), (0, 1)):
        exp_rays, exp_t = _plane_expect(rays_w, nrm_pr if n_per else N0, ctr_pr if c_per else C0, n_vals, bool(exclude))
        exp_rays = _store(exp_rays, code)
        moved = plain & np.isfinite(exp_t)
        if n_per and c_per:
            # backward rows, non-finite t, and rows that stay alive
            assert (exp_t < 0).sum() >= 0.05 * NPOOL and (~np.isfinite(exp_t)).sum() >= 2
            assert (~np.isnan(exp_rays).any(axis=1)).sum() >= 0.25 * NPOOL
        if exclude:
            assert (exp_t < 0).any() and np.isnan(exp_rays[exp_t < 0]).all()
        elif material == "descending_missing_key":
            # a table miss is n = NaN: NaN phase, position kept; the colours that are keys keep their phase
            miss = moved & (wl == _descending_missing(keys)[2])
            assert miss.sum() >= 0.1 * NPOOL
            assert np.isnan(exp_rays[miss, 6]).all() and not np.isnan(exp_rays[miss, 0:3]).any()
            assert not np.isnan(exp_rays[moved & ~miss, 6]).any() and (moved & ~miss).sum() >= 0.5 * NPOOL
        expects[n_per, c_per, exclude] = (exp_rays, exp_t)
    return rays_w, nrm_pr, ctr_pr, low, expects


@pytest.mark.parametrize("material", list(PLANE_MATERIALS))
@pytest.mark.parametrize("code", CODES, ids=CODE_ID.get)
def test_propagate_plane(code, material):
    lib = C.lib()
    checked = 0
    for roll in (0, ROLL):
        rays_w, nrm_pr, ctr_pr, low, expects = _plane_setup(code, material, roll)
        x = _to_dev(rays_w.astype(NP_DT[code]))
        nrm_d = {0: _to_dev(N0), 1: _to_dev(nrm_pr)}
        ctr_d = {0: _to_dev(C0), 1: _to_dev(ctr_pr)}
        ws_big, ws, need = _workspace(low.table_len)
        for (n_per, c_per, exclude), (exp_rays, exp_t) in expects.items():
            for n in TILE_SIZES:
                for with_ts in (True, False):
                    big, out = _padded(n, 8, TORCH_DT[code])
                    ts_big, ts = _padded(n, None, torch.float64)
                    C.check(lib.rtpb_propagate_plane(0, code, x.data_ptr(), n, nrm_d[n_per].data_ptr(), n_per,
                                                     ctr_d[c_per].data_ptr(), c_per, ctypes.byref(low), exclude,
                                                     out.data_ptr(), ts.data_ptr() if with_ts else None,
                                                     ws.data_ptr(), need, _stream()))
                    torch.cuda.synchronize(DEV)
                    key = (CODE_ID[code], material, roll, n_per, c_per, exclude, n, with_ts)
                    assert same_bits(out.cpu().numpy(), exp_rays[:n]), key
                    assert _pad_ok(big, n), key
                    if with_ts:
                        assert same_bits(ts.cpu().numpy(), exp_t[:n]), key
                        assert _pad_ok(ts_big, n), key
                    else:
                        assert bool((ts_big.cpu().numpy() == SENTINEL).all()), key
                    checked += 1
        assert _ws_ok(ws_big, need)
        # the inputs are not modified
        assert same_bits(x.cpu().numpy(), rays_w.astype(NP_DT[code]))
        assert same_bits(nrm_d[1].cpu().numpy(), nrm_pr) and same_bits(ctr_d[1].cpu().numpy(), ctr_pr)
        assert same_bits(nrm_d[0].cpu().numpy(), N0) and same_bits(ctr_d[0].cpu().numpy(), C0)
    assert checked == 2 * 8 * len(TILE_SIZES) * 2


def test_propagate_plane_hand_rows():
    """The hand-placed rows do what they were placed for (oracle side, both widened types)."""
    for code in CODES:
        rays_w = _widen(_ray_pool(), code)
        _, t = _plane_expect(rays_w, N0, C0, np.ones(NPOOL), False)
        h = t[HAND]
        assert h[0] == 0 and np.signbit(h[0]) and h[1] == 0 and not np.signbit(h[1])       # t = -0, +0
        assert np.isinf(h[2]) and np.isinf(h[3]) and np.isnan(h[6])                          # d . n == 0
        assert np.isinf(t[3])                                                               # zero direction


# ----------------------------------------------------------------------------------------- rtpb_front_side / rtpb_interact
AXES = {"+z": (0.0, 0.0, 1.0), "-z": (0.0, 0.0, -1.0), "oblique": tuple(systems.unit([0.3, -0.2, 1.0]))}


def _hook_plan(axis, m1, m2, keys, code):
    with np.errstate(all="ignore"):
        low = E.lower([rt._AxisOnly(axis)], [m1, m2], lambda: keys, code)
    return E.plan_ref(low)


def _front_setup(code, axis, roll):
    """rays, hits and the expectation: hits with whole rows NaN where d . axis < 0 on the widened rays."""
    rays_w = _widen(_rolled(_ray_pool(), roll), code)
    hits_w = _widen(_rolled(_hit_pool(), roll), code)
    with np.errstate(invalid="ignore"):
        back = O._dot(_rays_of(rays_w).d, tuple(np.float64(AXES[axis]))) < 0
    expect = _store(_rays_of(hits_w).kill(back).to_array(), code)
    assert back.sum() >= 0.02 * NPOOL and (~back).sum() >= 0.02 * NPOOL
    assert (~np.isnan(hits_w[back]).any(axis=1)).sum() >= 0.02 * NPOOL         # the kill changes rows
    return rays_w, hits_w, expect


@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("code", CODES, ids=CODE_ID.get)
def test_front_side(code, axis):
    lib = C.lib()
    checked = 0
    for roll in (0, ROLL):
        rays_w, hits_w, expect = _front_setup(code, axis, roll)
        rays_d = _to_dev(rays_w.astype(NP_DT[code]))
        hits_np = hits_w.astype(NP_DT[code])
        hits_d = _to_dev(hits_np)
        with _hook_plan(AXES[axis], mat.Vacuum(), mat.Vacuum(), _keys(hits_w[:, 7]), code) as plan:
            for n in TILE_SIZES:
                for alias in (False, True):
                    big, out = _padded(n, 8, TORCH_DT[code])
                    if alias:                                           # hits_out == hits
                        out.copy_(hits_d[:n])
                        src = out
                    else:
                        src = hits_d
                    C.check(lib.rtpb_front_side(plan, 0, rays_d.data_ptr(), src.data_ptr(), n, out.data_ptr(),
                                                _stream()))
                    torch.cuda.synchronize(DEV)
                    key = (CODE_ID[code], axis, roll, n, alias)
                    assert same_bits(out.cpu().numpy(), expect[:n]), key
                    assert _pad_ok(big, n), key
                    checked += 1
        assert same_bits(rays_d.cpu().numpy(), rays_w.astype(NP_DT[code]))
        assert same_bits(hits_d.cpu().numpy(), hits_np)                # a separate output leaves hits intact
    assert checked == 2 * len(TILE_SIZES) * 2


def _cauchy():
    return systems.cauchy_class(mat)()


# name -> (material 1, material 2, key dropped from the tables or None)
MEDIA = {
    "dense_to_rare": lambda: (mat.Constant(1.7), mat.Constant(1.0), None),
    "rare_to_dense": lambda: (mat.Constant(1.0), mat.Constant(1.7), None),
    "equal": lambda: (mat.Constant(1.5), mat.Constant(1.5), None),
    "bk7_to_ebaf11": lambda: (mat.Bk7(), mat.Ebaf11(), None),
    "vacuum_to_table_missing_key": lambda: (mat.Vacuum(), _cauchy(), 0.6328),
}


def _interact_setup(code, mode, media, roll):
    """hits, normals (storage type), on-surface bytes, table keys, media and the oracle's answer with and without the
    on-surface mask, with the coverage asserted on the oracle side.  No device work."""
    m1, m2, drop = MEDIA[media]()
    hits_w = _widen(_rolled(_ray_pool(), roll), code)
    nrm_np = _rolled(_normal_pool(), roll).astype(NP_DT[code])      # the kernel reads the normals in storage type
    nrm_w = nrm_np.astype(np.float64)
    on_np = np.ascontiguousarray(_rolled(_on_pool(), roll))
    wl = hits_w[:, 7]
    keys = _keys(wl)
    if drop is not None:
        dropped = keys[np.nanargmin(np.abs(keys - drop))]
        assert abs(dropped - drop) < 1e-6
        keys = keys[keys != dropped]
    ri = _rays_of(hits_w)
    normals = tuple(nrm_w[:, k].copy() for k in range(3))
    if mode == C.RTPB_REFRACT:
        n1 = _oracle_n(m1)(wl)
        if drop is None:
            n2 = _oracle_n(m2)(wl)
        else:
            with np.errstate(all="ignore"):
                n2 = _table_n(keys, np.asarray(m2.n(keys), dtype=np.float64))(wl)
        ro = O.snell(ri, normals, n1, n2)
    else:
        ro = O.mirror(ri, normals)
    full = ro.to_array()
    live = ~np.isnan(full[:, 3])
    clean = ~np.isnan(hits_w).any(axis=1) & ~np.isnan(nrm_w).any(axis=1) & (wl != 0)
    assert live.sum() >= 0.10 * NPOOL
    if media == "dense_to_rare" and mode == C.RTPB_REFRACT:
        tir = clean & ~live
        assert tir.sum() >= 0.10 * NPOOL
        assert np.isnan(full[tir, 0:3]).all() and not np.isnan(full[tir, 6:8]).any()   # TIR: position NaN only
    if drop is not None and mode == C.RTPB_REFRACT:
        miss = clean & (wl == dropped)
        assert miss.sum() >= 0.10 * NPOOL and not live[miss].any()
        assert np.isnan(full[miss, 0:3]).all() and not np.isnan(full[miss, 6:8]).any()
    assert 0.05 * NPOOL <= (on_np == 0).sum() <= 0.2 * NPOOL and (on_np > 1).sum() >= 0.2 * NPOOL
    assert (live & (on_np == 0)).sum() >= 0.01 * NPOOL                 # the mask kills rows that were alive
    expect = {True: _store(ro.kill(on_np == 0).to_array(), code), False: _store(full, code)}
    return hits_w, nrm_np, on_np, keys, m1, m2, expect


def _interact_case(code, mode, media):
    lib = C.lib()
    checked = 0
    for roll in (0, ROLL):
        hits_w, nrm_np, on_np, keys, m1, m2, expect = _interact_setup(code, mode, media, roll)
        hits_d = _to_dev(hits_w.astype(NP_DT[code]))
        nrm_d = _to_dev(nrm_np)
        on_d = _to_dev(on_np)
        with _hook_plan((0.0, 0.0, 1.0), m1, m2, keys, code) as plan:
            for n in TILE_SIZES:
                for with_on in (True, False):
                    big, out = _padded(n, 8, TORCH_DT[code])
                    C.check(lib.rtpb_interact(plan, 0, mode, hits_d.data_ptr(), nrm_d.data_ptr(),
                                              on_d.data_ptr() if with_on else None, n, out.data_ptr(), _stream()))
                    torch.cuda.synchronize(DEV)
                    key = (CODE_ID[code], mode, media, roll, n, with_on)
                    assert same_bits(out.cpu().numpy(), expect[with_on][:n]), key
                    assert _pad_ok(big, n), key
                    checked += 1
        assert same_bits(hits_d.cpu().numpy(), hits_w.astype(NP_DT[code]))
        assert same_bits(nrm_d.cpu().numpy(), nrm_np)
        assert np.array_equal(on_d.cpu().numpy(), on_np)
    assert checked == 2 * len(TILE_SIZES) * 2


@pytest.mark.parametrize("media", list(MEDIA))
@pytest.mark.parametrize("code", CODES, ids=CODE_ID.get)
def test_interact_refract(code, media):
    _interact_case(code, C.RTPB_REFRACT, media)


@pytest.mark.parametrize("code", CODES, ids=CODE_ID.get)
def test_interact_reflect(code):
    _interact_case(code, C.RTPB_REFLECT, "bk7_to_ebaf11")


def test_interact_hand_rows():
    """The hand-placed normals do what they were placed for (oracle side, both widened types)."""
    for code in CODES:
        hits_w = _widen(_ray_pool(), code)
        nrm_w = _normal_pool().astype(NP_DT[code]).astype(np.float64)
        d = hits_w[:, 3:6]
        assert np.array_equal(nrm_w[16], d[16]) and np.array_equal(nrm_w[17], -d[17]) and np.array_equal(nrm_w[0], d[0])
        cross = np.cross(d[[0, 16, 17]], nrm_w[[0, 16, 17]])
        assert not cross.any()                                          # normal incidence: zero cross product
        assert not nrm_w[18].any() and np.isnan(nrm_w[19]).all()


# ----------------------------------------------------------------------------------------- rtpb_intersect_rays
GENERAL, IN_XY, IN_YZ, ALONG_X = 0, 1, 2, 3
MEET, SKEW, PARALLEL = 0, 1, 2


def _dyadic(rng, size, step, top):
    """Non-zero multiples of `step` up to `top` in magnitude."""
    return rng.integers(1, int(top / step) + 1, size) * step * rng.choice([-1.0, 1.0], size)


@functools.lru_cache(maxsize=None)
def _isect_pool():
    """Pairs of rays that really meet: a meeting point P, two directions, origins stepped back along them.  Every
    coordinate is a multiple of 2^-4 of magnitude at most 32 (directions and steps are multiples of 2^-2 up to 2), so
    float32 holds the pool exactly and the solve is exact.  Four direction classes take every solver branch; about
    25 % of the pairs are made skew (origin 2 moved along d1 x d2) and 5 % exactly parallel; a few rows carry NaN
    or infinity.  Returns (ray1, ray2, class, kind, P)."""
    rng = np.random.default_rng(31)
    n = NPOOL
    cls = rng.permutation(np.arange(n) % 4)
    flat_x = (cls == ALONG_X) & (rng.random(n) < 0.5)       # ray 1 along x and ray 2 in the x-y plane: det_xy, dx1

    def shape(d1, d2):
        d1[cls == IN_XY, 2] = 0.0
        d2[cls == IN_XY, 2] = 0.0
        d1[cls == IN_YZ, 0] = 0.0
        d2[cls == IN_YZ, 0] = 0.0
        d1[cls == ALONG_X, 1:3] = 0.0
        d2[flat_x, 2] = 0.0

    d1 = _dyadic(rng, (n, 3), 0.25, 2.0)
    d2 = _dyadic(rng, (n, 3), 0.25, 2.0)
    shape(d1, d2)
    for _ in range(64):
        bad = ~np.cross(d1, d2).any(axis=1)                              # parallel
        bad |= (cls == GENERAL) & (d2[:, 0] * d1[:, 2] - d2[:, 2] * d1[:, 0] == 0)
        if not bad.any():
            break
        d2[bad] = _dyadic(rng, (int(bad.sum()), 3), 0.25, 2.0)
        shape(d1, d2)
    assert not bad.any()
    u = rng.random(n)
    kind = np.where(u < 0.25, SKEW, np.where(u < 0.30, PARALLEL, MEET))
    P = rng.integers(-64, 65, (n, 3)) / 16.0
    a = _dyadic(rng, n, 0.25, 2.0)
    b = _dyadic(rng, n, 0.25, 2.0)
    par = kind == PARALLEL
    d2[par] = d1[par] * rng.choice([1.0, -1.0, 2.0, -2.0], int(par.sum()))[:, None]
    o1 = P - a[:, None] * d1
    o2 = P - b[:, None] * d2
    skew = kind == SKEW
    o2[skew] += np.cross(d1[skew], d2[skew])
    off = par & (rng.random(n) < 0.5)                                   # the other parallel pairs are collinear
    o2[off] += _dyadic(rng, (int(off.sum()), 3), 0.25, 2.0)
    r1 = np.concatenate((o1, d1, rng.integers(0, 64, (n, 1)) / 8.0, np.full((n, 1), 0.5)), axis=1)
    r2 = np.concatenate((o2, d2, rng.integers(0, 64, (n, 1)) / 8.0, np.full((n, 1), 0.75)), axis=1)
    kind = kind.copy()
    r1[5, 3] = np.nan
    r2[6, 0] = np.inf
    r1[7] = np.nan
    r2[9, 5] = np.nan
    r1[10, 2] = -np.inf
    kind[[5, 6, 7, 9, 10]] = -1
    both = np.concatenate((r1[:, :6], r2[:, :6]))
    fin = np.isfinite(both)
    assert (np.abs(both[fin]) <= 32).all() and (both[fin] * 16 == np.round(both[fin] * 16)).all()
    for arr in (r1, r2, cls, kind, P):
        arr.setflags(write=False)
    return r1, r2, cls, kind, P


@functools.lru_cache(maxsize=None)
def _isect_fan():
    """One ray against many: rays that meet the single ray (0, 0, 0) + a (1/4, 1/2, 1) at a = multiples of 1/4, half of
    them moved off along the cross product.  Returns (single (1, 8), many (NPOOL, 8))."""
    rng = np.random.default_rng(32)
    n = NPOOL
    single = np.array([[0.0, 0.0, 0.0, 0.25, 0.5, 1.0, 0.0, 0.5]])
    d1 = single[0, 3:6]
    P = _dyadic(rng, n, 0.25, 4.0)[:, None] * d1[None, :]
    d2 = _dyadic(rng, (n, 3), 0.25, 2.0)
    for _ in range(64):
        bad = ~np.cross(d1[None, :], d2).any(axis=1) | (d2[:, 0] * d1[2] - d2[:, 2] * d1[0] == 0)
        if not bad.any():
            break
        d2[bad] = _dyadic(rng, (int(bad.sum()), 3), 0.25, 2.0)
    assert not bad.any()
    o2 = P - _dyadic(rng, n, 0.25, 2.0)[:, None] * d2
    skew = rng.random(n) < 0.5
    o2[skew] += np.cross(d1[None, :], d2[skew])
    many = np.concatenate((o2, d2, np.zeros((n, 1)), np.full((n, 1), 0.5)), axis=1)
    assert (np.abs(many[:, :6]) <= 32).all() and (many * 16 == np.round(many * 16)).all()
    single.setflags(write=False)
    many.setflags(write=False)
    return single, many


def _isect_expect(r1, r2, code):
    return _store(rt.intersect_rays(_widen(r1, code), _widen(r2, code)), code)


def _isect_call(code, r1, r2):
    """rtpb_intersect_rays on device copies of r1, r2 -> (points, padding untouched?, inputs untouched?)."""
    n1, n2 = len(r1), len(r2)
    n = max(n1, n2)
    a, b = r1.astype(NP_DT[code]), r2.astype(NP_DT[code])
    a_d, b_d = _to_dev(a), _to_dev(b)
    big, out = _padded(n, 3, TORCH_DT[code])
    C.check(C.lib().rtpb_intersect_rays(0, code, a_d.data_ptr(), n1, b_d.data_ptr(), n2, out.data_ptr(), _stream()))
    torch.cuda.synchronize(DEV)
    kept = same_bits(a_d.cpu().numpy(), a) and same_bits(b_d.cpu().numpy(), b)
    return out.cpu().numpy(), _pad_ok(big, n), kept


def test_intersect_pool_coverage():
    """Oracle side: the pool survives float32 unchanged, every class takes its solver branch, meets where it was
    built to meet (at P, exactly) and misses where it was built to miss, in both widened types."""
    r1, r2, cls, kind, P = _isect_pool()
    d1, d2 = r1[:, 3:6], r2[:, 3:6]
    ok = kind >= 0
    det_xz = d2[:, 0] * d1[:, 2] - d2[:, 2] * d1[:, 0]
    det_xy = d2[:, 0] * d1[:, 1] - d2[:, 1] * d1[:, 0]
    det_yz = d2[:, 2] * d1[:, 1] - d2[:, 1] * d1[:, 2]
    lines = ok & (kind != PARALLEL)
    assert (det_xz[lines & (cls == GENERAL)] != 0).all() and (d1[lines & (cls == GENERAL), 2] != 0).all()
    m = lines & (cls == IN_XY)
    assert (det_xz[m] == 0).all() and (det_xy[m] != 0).all() and (d1[m, 2] == 0).all() and (d1[m, 1] != 0).all()
    m = lines & (cls == IN_YZ)
    assert (det_xz[m] == 0).all() and (det_xy[m] == 0).all() and (det_yz[m] != 0).all()
    m = lines & (cls == ALONG_X)
    assert (d1[m, 2] == 0).all() and (d1[m, 1] == 0).all() and (d1[m, 0] != 0).all()
    assert (det_xz[m] == 0).sum() >= 100 and (det_xz[m] != 0).sum() >= 100      # det_xy and det_xz, both with dx1
    m = ok & (kind == PARALLEL)
    assert m.sum() >= 0.03 * NPOOL and not (det_xz[m].any() or det_xy[m].any() or det_yz[m].any())
    for code in CODES:
        for r in (r1, r2):
            assert same_bits(_widen(r, code), r)
        res = rt.intersect_rays(_widen(r1, code), _widen(r2, code))
        met = ~np.isnan(res).any(axis=1) & ok
        assert np.array_equal(met[ok], ~np.isnan(res[ok, 0]))
        assert np.array_equal(met[ok], kind[ok] == MEET)
        assert np.array_equal(res[met], P[met])
        for c in (GENERAL, IN_XY, IN_YZ, ALONG_X):
            assert (met & (cls == c)).sum() >= 100 and (~met & ok & (cls == c)).sum() >= 100, (code, c)
        single, many = _isect_fan()
        res = rt.intersect_rays(_widen(single, code), _widen(many, code))
        met = ~np.isnan(res[:, 0])
        assert met.sum() >= 0.25 * NPOOL and (~met).sum() >= 0.25 * NPOOL


@pytest.mark.parametrize("code", CODES, ids=CODE_ID.get)
def test_intersect_rays(code):
    r1p, r2p = _isect_pool()[:2]
    checked = 0
    for roll, n in _variants(BLOCK_SIZES):
        r1, r2 = _rolled(r1p, roll)[:n], _rolled(r2p, roll)[:n]
        for a, b in ((r1, r2), (r2, r1)):
            got, pad_ok, kept = _isect_call(code, a, b)
            assert same_bits(got, _isect_expect(a, b, code)), (CODE_ID[code], roll, n)
            assert pad_ok and kept, (CODE_ID[code], roll, n)
            checked += 1
    assert checked == 2 * len(BLOCK_SIZES) * 2


@pytest.mark.parametrize("code", CODES, ids=CODE_ID.get)
def test_intersect_rays_broadcast(code):
    """n1 == 1 and n2 == 1: the single ray on either argument, against the fan built to meet it and against pool rays."""
    single, many = _isect_fan()
    r1p, r2p = _isect_pool()[:2]
    checked = 0
    for roll, n in _variants(BLOCK_SIZES):
        m = _rolled(many, roll)[:n]
        for a, b in ((single, m), (m, single), (r1p[roll:roll + 1], _rolled(r2p, roll)[:n]),
                     (_rolled(r1p, roll)[:n], r2p[roll:roll + 1])):
            got, pad_ok, kept = _isect_call(code, a, b)
            assert got.shape == (n, 3)
            assert same_bits(got, _isect_expect(a, b, code)), (CODE_ID[code], roll, n, len(a), len(b))
            assert pad_ok and kept, (CODE_ID[code], roll, n, len(a), len(b))
            checked += 1
    assert checked == 2 * len(BLOCK_SIZES) * 4


def test_intersect_rays_wrapper_float32():
    """rt.intersect_rays on float32 CUDA tensors: a float32 CUDA tensor, the same expectation."""
    r1, r2 = _isect_pool()[:2]
    got = rt.intersect_rays(_to_dev(r1.astype(np.float32)), _to_dev(r2.astype(np.float32)))
    torch.cuda.synchronize(DEV)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (NPOOL, 3)
    assert same_bits(got.cpu().numpy(), _isect_expect(r1, r2, C.RTPB_F32))
    single, many = _isect_fan()
    got = rt.intersect_rays(_to_dev(single.astype(np.float32)), _to_dev(many.astype(np.float32)))
    assert got.is_cuda and got.dtype == torch.float32
    assert same_bits(got.cpu().numpy(), _isect_expect(single, many, C.RTPB_F32))


# ----------------------------------------------------------------------------------------- argument checks
def test_error_paths_and_empty_calls():
    """Every bad call returns its documented code before any launch, with a message; n == 0 is RTPB_OK with NULL
    buffers."""
    lib = C.lib()
    n = 64
    s = _stream()

    def refused(rc, what):
        assert rc == C.RTPB_E_INVALID, (what, rc)
        assert lib.rtpb_last_error(), what

    vac = E.lower_material(mat.Vacuum(), lambda: np.array([0.5]))
    tab = E.lower_material(_cauchy(), lambda: np.array([0.5, 0.6]))
    nrm_d, ctr_d = _to_dev(N0), _to_dev(C0)
    ws = torch.zeros(256 + 16 * 2, dtype=torch.uint8, device=DEV)
    bufs = {}
    for code in CODES:
        x = torch.zeros((n + 1, 8), dtype=TORCH_DT[code], device=DEV)
        x[:, 5] = 1.0
        x[:, 7] = 0.5
        out = torch.full((n + 1, 8), SENTINEL, dtype=TORCH_DT[code], device=DEV)
        bufs[code] = (x, out)

    def plane(code=C.RTPB_F64, n_rays=n, rays_in=None, rays_out=None, material=vac, ws_bytes=ws.numel(), normal=nrm_d,
              ws_ptr=ws.data_ptr()):
        x, out = bufs[code if code in bufs else C.RTPB_F64]
        return lib.rtpb_propagate_plane(0, code, x.data_ptr() if rays_in is None else rays_in, n_rays,
                                        normal.data_ptr() if normal is not None else None, 0, ctr_d.data_ptr(), 0,
                                        ctypes.byref(material), 0, out.data_ptr() if rays_out is None else rays_out,
                                        None, ws_ptr, ws_bytes, s)

    assert plane() == C.RTPB_OK                                         # the base call is a good one
    refused(plane(code=7), "plane: bad dtype")
    refused(plane(n_rays=-1), "plane: n < 0")
    for code in CODES:
        x, out = bufs[code]
        refused(plane(code=code, rays_in=x.data_ptr() + 8), "plane: misaligned input")
        refused(plane(code=code, rays_out=out.data_ptr() + 8), "plane: misaligned output")
    assert plane(ws_bytes=256 + 16) == C.RTPB_OK                        # the documented minimum without a table
    refused(plane(ws_bytes=256 + 16 - 1), "plane: workspace one byte too small")
    assert plane(material=tab) == C.RTPB_OK                             # ... and with a table of two keys
    refused(plane(material=tab, ws_bytes=256 + 16 * 2 - 1), "plane: table workspace one byte too small")
    empty = C.Material()
    empty.kind, empty.table_len = C.RTPB_TABLE, 0
    empty.table = tab.table
    refused(plane(material=empty), "plane: TABLE with table_len == 0")
    bad_kind = C.Material()
    bad_kind.kind = 9
    refused(plane(material=bad_kind), "plane: bad material kind")
    refused(plane(normal=None), "plane: NULL normal")
    refused(plane(ws_ptr=None), "plane: NULL workspace")

    x64 = bufs[C.RTPB_F64][0]
    pts = torch.full((n, 3), SENTINEL, dtype=torch.float64, device=DEV)
    refused(lib.rtpb_intersect_rays(0, 7, x64.data_ptr(), n, x64.data_ptr(), n, pts.data_ptr(), s), "intersect: bad dtype")
    refused(lib.rtpb_intersect_rays(0, C.RTPB_F64, x64.data_ptr(), -1, x64.data_ptr(), -1, pts.data_ptr(), s),
            "intersect: n < 0")
    refused(lib.rtpb_intersect_rays(0, C.RTPB_F64, x64.data_ptr(), 3, x64.data_ptr(), 2, pts.data_ptr(), s),
            "intersect: mismatched n1 / n2")
    refused(lib.rtpb_intersect_rays(0, C.RTPB_F64, None, n, x64.data_ptr(), n, pts.data_ptr(), s), "intersect: NULL rays")

    on = torch.ones(n, dtype=torch.uint8, device=DEV)
    for code in CODES:
        x, out = bufs[code]
        nrm = torch.zeros((n, 3), dtype=TORCH_DT[code], device=DEV)
        nrm[:, 2] = 1.0
        with _hook_plan((0.0, 0.0, 1.0), mat.Vacuum(), mat.Vacuum(), np.array([0.5]), code) as plan:
            assert lib.rtpb_front_side(plan, 0, x.data_ptr(), x.data_ptr(), n, out.data_ptr(), s) == C.RTPB_OK
            assert lib.rtpb_interact(plan, 0, C.RTPB_REFRACT, x.data_ptr(), nrm.data_ptr(), on.data_ptr(), n,
                                     out.data_ptr(), s) == C.RTPB_OK
            refused(lib.rtpb_interact(plan, 0, 5, x.data_ptr(), nrm.data_ptr(), on.data_ptr(), n, out.data_ptr(), s),
                    "interact: bad mode")
            refused(lib.rtpb_front_side(plan, 0, x.data_ptr(), x.data_ptr(), -1, out.data_ptr(), s), "front_side: n < 0")
            refused(lib.rtpb_interact(plan, 0, C.RTPB_REFLECT, x.data_ptr(), nrm.data_ptr(), None, -1, out.data_ptr(), s),
                    "interact: n < 0")
            for k, name in enumerate(("rays", "hits", "hits_out")):
                p = [x.data_ptr(), x.data_ptr(), out.data_ptr()]
                p[k] += 8
                refused(lib.rtpb_front_side(plan, 0, p[0], p[1], n, p[2], s), "front_side: misaligned " + name)
            refused(lib.rtpb_interact(plan, 0, C.RTPB_REFRACT, x.data_ptr() + 8, nrm.data_ptr(), None, n, out.data_ptr(),
                                      s), "interact: misaligned hits")
            refused(lib.rtpb_interact(plan, 0, C.RTPB_REFRACT, x.data_ptr(), nrm.data_ptr(), None, n,
                                      out.data_ptr() + 8, s), "interact: misaligned out")
            refused(lib.rtpb_interact(plan, 0, C.RTPB_REFRACT, x.data_ptr(), None, None, n, out.data_ptr(), s),
                    "interact: NULL normals")
            refused(lib.rtpb_front_side(plan, 0, None, x.data_ptr(), n, out.data_ptr(), s), "front_side: NULL rays")
            # n == 0: RTPB_OK with NULL buffers
            assert lib.rtpb_front_side(plan, 0, None, None, 0, None, s) == C.RTPB_OK
            assert lib.rtpb_interact(plan, 0, C.RTPB_REFRACT, None, None, None, 0, None, s) == C.RTPB_OK
            assert lib.rtpb_interact(plan, 0, C.RTPB_REFLECT, None, None, None, 0, None, s) == C.RTPB_OK
        refused(lib.rtpb_front_side(None, 0, x.data_ptr(), x.data_ptr(), n, out.data_ptr(), s), "front_side: NULL plan")
        refused(lib.rtpb_interact(None, 0, C.RTPB_REFRACT, x.data_ptr(), nrm.data_ptr(), None, n, out.data_ptr(), s),
                "interact: NULL plan")
        # a plan with no surface and one material
        one = ctypes.c_void_p()
        mats = (C.Material * 1)(vac)
        C.check(lib.rtpb_plan_create(None, 0, mats, 1, code, ctypes.byref(one)))
        try:
            refused(lib.rtpb_front_side(one, 0, x.data_ptr(), x.data_ptr(), n, out.data_ptr(), s),
                    "front_side: plan with one material")
            refused(lib.rtpb_interact(one, 0, C.RTPB_REFRACT, x.data_ptr(), nrm.data_ptr(), None, n, out.data_ptr(), s),
                    "interact: plan with one material")
        finally:
            C.check(lib.rtpb_plan_destroy(one))
        assert lib.rtpb_propagate_plane(0, code, None, 0, nrm_d.data_ptr(), 0, ctr_d.data_ptr(), 0, ctypes.byref(vac), 0,
                                        None, None, None, 0, s) == C.RTPB_OK
        assert lib.rtpb_intersect_rays(0, code, None, 0, None, 0, None, s) == C.RTPB_OK
    torch.cuda.synchronize(DEV)
    # no refused call launched anything: the outputs it was handed are untouched
    assert bool((pts.cpu().numpy() == SENTINEL).all())
    for code in CODES:
        assert bool((bufs[code][1][n:].cpu().numpy() == SENTINEL).all())
