"""Table-miss flag (rtpb_trace_checked) and the optimistic table keys of the torch path.

Tabulated materials (Ebaf11, user Material subclasses: MAT:39-44, 128-144) hold n() at a key set of
wavelengths.  rtpb_trace_checked flags any ray whose wavelength is not a key (its n would be NaN); the
torch front end traces with the previous bundle's keys and scans the wavelength column only on a miss.
Every result is compared bit for bit with the NumPy oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ray_trace_pb_amd.materials as mat  # noqa: E402
import ray_trace_pb_amd.raytrace as rt  # noqa: E402
from ray_trace_pb_amd import _capi as C  # noqa: E402
from ray_trace_pb_amd import _engine as E  # noqa: E402
import systems  # noqa: E402
from parity import oracle_trace, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _system(cauchy=None):
    return rt.System([rt.FlatSurface([0, 0, 0], [0, 0, 1], 50),
                      rt.SphericalSurface.get_on_axis(40.0, 5.0, 30.0),
                      rt.FlatSurface([0, 0, 12], systems.unit([0.1, 0, 1]), 50)],
                     [mat.Ebaf11(), cauchy or systems.cauchy_class(mat)()])


def _rays(n, wls, seed):
    rng = np.random.default_rng(seed)
    rays = np.zeros((n, 8))
    rays[:, 0:2] = rng.uniform(-8, 8, (n, 2))
    rays[:, 2] = -1.0
    d = np.stack((rng.normal(scale=0.05, size=n), rng.normal(scale=0.05, size=n), np.ones(n)), axis=1)
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1)[:, None]
    rays[:, 7] = np.asarray(wls)[rng.integers(0, len(wls), n)]
    return rays


@pytest.mark.parametrize("variant", ["indexed", "lds", "global"])
def test_miss_flag_every_table_variant(variant):
    """The flag is 0 when every ray's wavelength is a key and 1 otherwise (a foreign wavelength, or a NaN
    wavelength without a NaN key), for the indexed-material, LDS-table and global-table kernels."""
    system, m0, m1 = _system(), mat.Vacuum(), mat.Vacuum()
    nkeys = 200 if variant == "global" else 5          # 2 tables x 200 pairs > the 256-pair LDS copy
    keys = np.linspace(0.45, 1.3, nkeys)
    lib = C.lib()
    E.clear_plan_cache()
    C.check(lib.rtpb_set_tuning(b"indexed_materials", 1 if variant == "indexed" else 0))
    try:
        mats = [m0] + list(system.materials) + [m1]
        low = E.lower(system.surfaces, mats, lambda: keys, C.RTPB_F64)
        sel = E.resolve_planes("all", len(system.surfaces))
        rays = _rays(3001, keys, 11)
        x = torch.from_numpy(rays).to(DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = E.trace_device(low, x, sel, miss=flag)
        assert int(flag.item()) == 0
        assert same_bits(out.cpu().numpy(), oracle_trace(system, m0, m1, rays))
        for bad in (0.5123, np.nan):
            r2 = rays.copy()
            r2[1777, 7] = bad
            flag.zero_()
            E.trace_device(low, torch.from_numpy(r2).to(DEV), sel, miss=flag)
            assert int(flag.item()) == 1, bad
        # a NaN key makes NaN wavelengths hits
        keys_nan = np.append(keys, np.nan)
        low_nan = E.lower(system.surfaces, mats, lambda: keys_nan, C.RTPB_F64)
        r3 = rays.copy()
        r3[5, 7] = np.nan
        flag.zero_()
        out3 = E.trace_device(low_nan, torch.from_numpy(r3).to(DEV), sel, miss=flag)
        assert int(flag.item()) == 0
        assert same_bits(out3.cpu().numpy(), oracle_trace(system, m0, m1, r3))
        # no flag pointer: the plain launch
        E.trace_device(low, x, sel)
    finally:
        C.check(lib.rtpb_set_tuning(b"indexed_materials", 1))
        E.clear_plan_cache()


def test_optimistic_keys_reused_and_rescanned_on_a_miss(monkeypatch):
    """Bundle A caches its keys; bundle B (a subset of A's wavelengths) traces with them and never scans;
    bundle C (a new wavelength) misses, is scanned and re-traced; a changed material attribute is a new
    fingerprint.  Every history is bit-identical to the oracle."""
    cauchy = systems.cauchy_class(mat)()
    system, m0, m1 = _system(cauchy), mat.Vacuum(), mat.Vacuum()
    scans = []
    real = E.distinct_wavelengths
    monkeypatch.setattr(E, "distinct_wavelengths", lambda col: scans.append(1) or real(col))
    E._KEYS.clear()

    def check(rays, dtype=None):
        got = system.ray_trace(torch.from_numpy(rays).to(DEV), m0, m1, dtype=dtype).cpu().numpy()
        ref = oracle_trace(system, m0, m1, rays)
        assert same_bits(got, ref if dtype is None else ref.astype(np.float32))

    check(_rays(2049, [0.5, 0.6, 0.7], 1))
    assert len(scans) == 1
    check(_rays(2049, [0.6], 2))
    check(_rays(999, [0.7, 0.5], 3), dtype="float32")
    assert len(scans) == 1                                  # keys of bundle A reused, no column scan
    check(_rays(2049, [0.6, 0.9], 4))                        # 0.9 is no key: miss, scan, re-trace
    assert len(scans) == 2
    check(_rays(2049, [0.9], 5))
    assert len(scans) == 2
    cauchy.b = 0.005                                        # new n(): new fingerprint, fresh keys
    check(_rays(2049, [0.9], 6))
    assert len(scans) == 3
    # 3-D input (history extension) and final-plane output take the same path
    rays = _rays(513, [0.9], 7)
    hist = system.ray_trace(torch.from_numpy(rays).to(DEV), m0, m1)
    ext = system.ray_trace(hist, m0, m1).cpu().numpy()
    ref = oracle_trace(system, m0, m1, rays)
    assert same_bits(ext[:ref.shape[0]], ref) and ext.shape[0] == 2 * ref.shape[0] - 1
    fin = system.ray_trace(torch.from_numpy(rays).to(DEV), m0, m1, planes="final").cpu().numpy()
    assert same_bits(fin[0], ref[-1])
    assert len(scans) == 3
