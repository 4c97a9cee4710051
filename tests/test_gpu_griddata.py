"""GPU: grid_interp_kernel (rtpb_grid_interpolate, GridInterpolator) against the exact restatement of
griddata_oracle.py -- the lowest-index accepting simplex, found by brute force -- bit for bit, on layouts with grid
points on vertices and shared edges, duplicate points, a single triangle, ragged one-row / one-column grids and
point sets that strain the host-built cell index; and the pupil field path element by element."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from ray_trace_pb_amd import _capi as C  # noqa: E402
from ray_trace_pb_amd import analysis  # noqa: E402
import griddata_oracle as G  # noqa: E402
from parity import bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("plain", "high")


@functools.lru_cache(maxsize=None)
def _interpolator(name):
    return analysis.GridInterpolator(G.case(name).points, DEV)


def _explain(c, values, got, want):
    """The first grid point whose bits differ: the simplices that accept it and the one the kernel's value matches."""
    acc, c0, c1, c2 = c.acc_c
    k = int(np.flatnonzero(bits(got).ravel() != bits(want).ravel())[0])
    iy, ix = divmod(k, len(c.xs))
    accepting = np.flatnonzero(acc[k])
    v = values[c.tri.simplices[accepting]]
    each = ((0.0 + c0[k, accepting] * v[:, 0]) + c1[k, accepting] * v[:, 1]) + c2[k, accepting] * v[:, 2]
    used = accepting[bits(each) == bits(got).ravel()[k]]
    return (f"{c.name}: grid point {k} (ix {ix}, iy {iy}) = ({c.xs[ix]!r}, {c.ys[iy]!r}): kernel {got.ravel()[k]!r}, "
            f"restatement {want.ravel()[k]!r}; accepted by simplices {accepting.tolist()}, the kernel's value is "
            f"that of {used.tolist()}; {int((bits(got) != bits(want)).sum())} points differ")


def _assert_phase(c, kind, got):
    want = c.phase(kind)
    assert got.shape == want.shape
    if not np.array_equal(bits(got), bits(want)):
        raise AssertionError(_explain(c, G.values_for(c.points, kind), got, want))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", G.NAMES)
def test_phase_is_the_first_listed_accepting_simplex_bit_for_bit(name, kind):
    """No tolerance and no exempt share: NaN positions included, every grid point has the bits of the restatement.
    Pins the kernel's arithmetic, the cell index and the rule "on a shared edge the first listed triangle is used"."""
    c = G.case(name)
    got = _interpolator(name).set_values(G.values_for(c.points, kind))(c.xs, c.ys)[0].cpu().numpy()
    _assert_phase(c, kind, got)


def test_set_values_swaps_the_values_of_a_reused_triangulation():
    c = G.case("polar_fan")
    gi = analysis.GridInterpolator(c.points, DEV)
    for kind in ("plain", "high", "plain"):
        _assert_phase(c, kind, gi.set_values(G.values_for(c.points, kind))(c.xs, c.ys)[0].cpu().numpy())
    # and the one-call wrapper
    _assert_phase(c, "high", analysis.griddata_linear(c.points, G.values_for(c.points, "high"), c.xs, c.ys,
                                                      device=DEV).cpu().numpy())


def _radius(c):
    """The lattice's grid has nodes exactly on the circle of radius 0.625 ((+-0.375, +-0.5) and transposed), where
    `>` must be false; elsewhere the median distance of the grid from the origin, so both sides are populated."""
    if c.name == "lattice":
        return 0.625
    xx, yy = np.meshgrid(c.xs, c.ys)
    return float(np.median(np.sqrt(xx * xx + yy * yy)))


@pytest.mark.parametrize("name", G.NAMES)
def test_pupil_field_mask_phase_and_values(name):
    """`radius` given, with phase=False (phase_out NULL) and phase=True: the field is exactly 0 where the restatement
    says so (strictly outside the radius, or undefined phase) and nowhere else; the phase has the bits of the
    phase-only call; both calls give the same field.  Non-zero field values: cos and sin of the phase, with an
    absolute error against long-double cos/sin of the same (exactly widened) phase of at most
    4 * max(NumPy's own largest error on these arguments, 2^-53).  The factor 4 is chosen, not derived: room for a
    2-ulp device routine beside a sub-ulp host one, none for a lost argument reduction (wrong in the 9th digit at
    1e7 rad)."""
    c = G.case(name)
    gi = _interpolator(name)
    radius = _radius(c)
    xx, yy = np.meshgrid(c.xs, c.ys)
    if name == "lattice":
        on = np.sqrt(xx * xx + yy * yy) == radius
        assert on.sum() >= 8 and on[np.isclose(np.abs(xx), 0.375) & np.isclose(np.abs(yy), 0.5)].all()
    for kind in KINDS:
        gi.set_values(G.values_for(c.points, kind))
        none, fld0 = gi(c.xs, c.ys, radius=radius, phase=False)
        ph1, fld1 = gi(c.xs, c.ys, radius=radius, phase=True)
        assert none is None
        fld0, fld1, ph1 = fld0.cpu().numpy(), fld1.cpu().numpy(), ph1.cpu().numpy()
        _assert_phase(c, kind, ph1)
        assert np.array_equal(bits(fld0.view(np.float64)), bits(fld1.view(np.float64)))
        off = G.field_off(c.phase(kind), c.xs, c.ys, radius)
        assert off.any() and not off.all()
        if name == "lattice":
            assert not off[on].any()
        assert np.array_equal(fld0 == 0, off), np.argwhere((fld0 == 0) != off)[:5]
        assert not bits(fld0.view(np.float64).reshape(off.shape + (2,))[off]).any()      # +0.0, both components
        ph = ph1[~off]
        dev = np.stack((fld0.real[~off], fld0.imag[~off]))
        host = np.stack((np.cos(ph), np.sin(ph)))
        wide = ph.astype(np.longdouble)
        exact = np.stack((np.cos(wide), np.sin(wide)))
        e_dev = float(np.max(np.abs(dev.astype(np.longdouble) - exact)))
        e_host = float(np.max(np.abs(host.astype(np.longdouble) - exact)))
        print(f"{name}/{kind}: {ph.size} field points, max |cos, sin error| device {e_dev / 2.0 ** -53:.3f}, "
              f"NumPy {e_host / 2.0 ** -53:.3f} (units of 2^-53); {int((dev != host).sum())} of {dev.size} values "
              f"differ from NumPy, by at most {float(np.max(np.abs(dev - host))) / 2.0 ** -53:.3f}")
        if np.finfo(np.longdouble).nmant == 63:                 # x87 extended: 11 bits beyond double
            assert e_dev <= 4.0 * max(e_host, 2.0 ** -53), (e_dev, e_host)
        else:
            print("long double is no wider than needed here: the error bound is not applied")


def test_argument_errors_return_before_any_launch():
    c = G.case("one_triangle")
    gi = _interpolator("one_triangle").set_values(G.values_for(c.points))
    lib = C.lib()
    xs = torch.as_tensor(c.xs).to(DEV)
    ys = torch.as_tensor(c.ys).to(DEV)
    out = torch.full((len(c.ys), len(c.xs)), 7.0, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    tri = ctypes.byref(gi.desc)
    call = lib.rtpb_grid_interpolate
    assert call(0, tri, xs.data_ptr(), 0, ys.data_ptr(), len(c.ys), 0.0, out.data_ptr(), None, stream) \
        == C.RTPB_E_INVALID
    assert call(0, None, xs.data_ptr(), len(c.xs), ys.data_ptr(), len(c.ys), 0.0, out.data_ptr(), None, stream) \
        == C.RTPB_E_INVALID
    for field in ("transform", "simplices", "values", "cell_start", "cell_tris"):      # a NULL array in the descriptor
        bad = C.Triangulation.from_buffer_copy(gi.desc)
        setattr(bad, field, None)
        assert call(0, ctypes.byref(bad), xs.data_ptr(), len(c.xs), ys.data_ptr(), len(c.ys), 0.0, out.data_ptr(),
                    None, stream) == C.RTPB_E_INVALID, field
    assert call(0, tri, xs.data_ptr(), len(c.xs), ys.data_ptr(), len(c.ys), 0.0, None, None, stream) == C.RTPB_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    # the same arguments with an output do launch
    assert call(0, tri, xs.data_ptr(), len(c.xs), ys.data_ptr(), len(c.ys), 0.0, out.data_ptr(), None, stream) \
        == C.RTPB_OK
    _assert_phase(c, "plain", out.cpu().numpy())
