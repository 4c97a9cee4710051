"""The restatement of rtpb_grid_interpolate that test_gpu_griddata.py holds the kernel to (griddata_oracle.py),
checked on the host: against scipy.interpolate.griddata, and against the kernel's own search through
GridInterpolator's cell index, on every layout.  No GPU."""
import numpy as np
import pytest

import griddata_oracle as G
from parity import same_bits


@pytest.mark.parametrize("name", G.NAMES)
def test_restatement_matches_scipy_griddata(name):
    """Same NaN (outside-hull) mask as scipy, values within the project's bound for griddata (1e-12 of max|ref|,
    test_gpu_griddata_matches_scipy), and different from scipy only where two or more simplices accept the grid
    point: there scipy's walk may end in another simplex than the first listed, one rounding away."""
    from scipy.interpolate import griddata
    c = G.case(name)
    xx, yy = np.meshgrid(c.xs, c.ys)
    for kind in ("plain", "high"):
        ours = c.phase(kind)
        ref = griddata(c.points, G.values_for(c.points, kind), np.stack((xx.ravel(), yy.ravel()), 1)).reshape(xx.shape)
        assert np.array_equal(np.isnan(ours), np.isnan(ref))
        fin = ~np.isnan(ref)
        assert fin.any()
        differs = fin & (ours != ref)
        worst = np.max(np.abs(ours[fin] - ref[fin]))
        print(f"{name}/{kind}: {int(differs.sum())} of {int(fin.sum())} finite points differ from scipy, "
              f"largest {worst:.3g} = {worst / np.max(np.abs(ref[fin])):.3g} of max|ref|")
        assert worst <= 1e-12 * np.max(np.abs(ref[fin]))
        assert (c.n_accepting[differs] >= 2).all(), np.argwhere(differs & (c.n_accepting < 2))[:5]
        assert (c.n_accepting[fin] >= 1).all() and (c.n_accepting[~fin] == 0).all()


def _kernel_search(gi, c, values):
    """grid_interp_kernel's search, statement by statement: the grid point's cell, that cell's simplices in listed
    order, the first that accepts (the acceptance and the coordinates are the restatement's own)."""
    d = gi.desc
    start, listed = gi._start.numpy(), gi._cells.numpy()
    acc, c0, c1, c2 = c.acc_c
    xx, yy = np.meshgrid(c.xs, c.ys)
    x, y = xx.ravel(), yy.ravel()
    fx, fy = (x - d.x0) / d.cell_w, (y - d.y0) / d.cell_h
    inside = (fx >= 0.0) & (fy >= 0.0) & (fx < float(d.cells_x)) & (fy < float(d.cells_y))
    out = np.full(x.shape, np.nan)
    for k in np.flatnonzero(inside):
        cell = int(fy[k]) * d.cells_x + int(fx[k])
        for s in listed[start[cell]:start[cell + 1]]:
            if acc[k, s]:
                v = values[c.tri.simplices[s]]
                out[k] = ((0.0 + c0[k, s] * v[0]) + c1[k, s] * v[1]) + c2[k, s] * v[2]
                break
    return out.reshape(xx.shape), inside.reshape(xx.shape)


@pytest.mark.parametrize("name", G.NAMES)
def test_cell_index_search_equals_brute_force(name):
    """GridInterpolator's cell index (built on the host; here on the CPU device) loses no accepting simplex and lists
    each cell's in index order: the kernel's search through it gives the brute-force result bit for bit."""
    from ray_trace_pb_amd.analysis import GridInterpolator
    c = G.case(name)
    gi = GridInterpolator(c.points, device="cpu")
    assert np.array_equal(gi._simplices.numpy(), c.tri.simplices)
    assert same_bits(gi._transform.numpy(), c.tri.transform.reshape(-1, 6))
    got, inside = _kernel_search(gi, c, G.values_for(c.points, "plain"))
    assert same_bits(got, c.phase("plain"))
    assert (c.n_accepting[~inside] == 0).all()


def test_layouts_reach_the_edges_they_are_meant_for():
    """The layouts are not vacuous: grid points that several simplices accept, grid points off every side of the
    cell index's box, and one-row / one-column grids that are no multiple of the 256-thread block."""
    from ray_trace_pb_amd.analysis import GridInterpolator
    assert len(G.NAMES) == 9
    for name in ("lattice", "fan_dup_centre"):
        assert int((G.case(name).n_accepting >= 2).sum()) >= 100, name
    fan = G.case("fan_dup_centre")
    assert (np.abs(fan.points).sum(axis=1) == 0).sum() == 8             # the duplicated centre
    assert G.case("one_triangle").tri.simplices.shape[0] == 1
    row, col = G.case("one_row"), G.case("one_column")
    assert (len(row.xs), len(row.ys)) == (259, 1) and (len(col.xs), len(col.ys)) == (1, 259)
    assert np.isfinite(row.phase()).sum() > 200 and np.isfinite(col.phase()).sum() > 200
    c = G.case("lattice")
    d = GridInterpolator(c.points, device="cpu").desc
    x1, y1 = d.x0 + d.cells_x * d.cell_w, d.y0 + d.cells_y * d.cell_h
    assert c.xs.min() < d.x0 and c.xs.max() > x1 and c.ys.min() < d.y0 and c.ys.max() > y1
    # and on the lattice the grid holds every node: all vertices of the triangulation are grid points
    assert set(map(tuple, c.points)) <= {(x, y) for x in c.xs for y in c.ys}
