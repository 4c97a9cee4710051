"""Brute-force restatement of ``rtpb_grid_interpolate`` (GridInterpolator) in NumPy, and the layouts its tests share.

The rule: a grid point takes the lowest-index simplex of ``scipy.spatial.Delaunay(points)`` whose three barycentric
coordinates all lie in [-eps, 1 + eps], eps = 100 * DBL_EPSILON (scipy's own acceptance test); the coordinates come
from ``tri.transform`` in the kernel's operation order, every step one rounded IEEE operation:

    c0 = (0 + T0 * (x - T4)) + T1 * (y - T5)
    c1 = (0 + T2 * (x - T4)) + T3 * (y - T5)
    c2 = (1 - c0) - c1
    value = ((0 + c0 * v0) + c1 * v1) + c2 * v2          NaN where no simplex accepts the point

Every grid point is tested against every simplex: the cell index that the kernel searches never enters, so a
simplex missing from a cell, or listed out of order, shows as a difference.
"""
import numpy as np

EPS = 100.0 * np.finfo(np.float64).eps


def accepted(tri, xs, ys):
    """(accept (G, S) bool, c0, c1, c2 (G, S)) for the G = len(ys) * len(xs) points of meshgrid(xs, ys), row-major
    (x fastest, as the kernel numbers them), against the S simplices of `tri`."""
    xx, yy = np.meshgrid(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64))
    x, y = xx.reshape(-1, 1), yy.reshape(-1, 1)
    T = tri.transform.reshape(-1, 6)
    with np.errstate(invalid="ignore"):                            # a degenerate simplex has a NaN transform
        dx, dy = x - T[:, 4], y - T[:, 5]
        c0 = (0.0 + T[:, 0] * dx) + T[:, 1] * dy
        c1 = (0.0 + T[:, 2] * dx) + T[:, 3] * dy
        c2 = (1.0 - c0) - c1
        acc = np.ones(c0.shape, dtype=bool)
        for c in (c0, c1, c2):
            acc &= (-EPS <= c) & (c <= 1.0 + EPS)
    return acc, c0, c1, c2


def interpolate(tri, values, xs, ys, acc_c=None):
    """The restated phase on meshgrid(xs, ys), (len(ys), len(xs)) float64."""
    acc, c0, c1, c2 = acc_c if acc_c is not None else accepted(tri, xs, ys)
    values = np.asarray(values, dtype=np.float64)
    hit = acc.any(axis=1)
    g = np.flatnonzero(hit)
    s = acc.argmax(axis=1)[g]                                      # the first (lowest-index) accepting simplex
    v = values[tri.simplices[s]]                                   # (n_hit, 3)
    out = np.full(acc.shape[0], np.nan)
    out[g] = ((0.0 + c0[g, s] * v[:, 0]) + c1[g, s] * v[:, 1]) + c2[g, s] * v[:, 2]
    return out.reshape(len(ys), len(xs))


def field_off(phase, xs, ys, radius):
    """Where the pupil field is zero: outside `radius` (strictly) or where the phase is undefined."""
    xx, yy = np.meshgrid(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64))
    return (np.sqrt(xx * xx + yy * yy) > radius) | np.isnan(phase)


def field(phase, xs, ys, radius):
    """The restated pupil field, (len(ys), len(xs)) complex128: 0 where `field_off`, else cos(phase) + i sin(phase)."""
    off = field_off(phase, xs, ys, radius)
    with np.errstate(invalid="ignore"):
        return np.where(off, 0.0, np.cos(phase)) + 1j * np.where(off, 0.0, np.sin(phase))


def values_for(points, kind="plain", seed=5):
    """Vertex values.  "plain": the form of test_gpu_griddata_matches_scipy, 1e4 + 3x^2 - 2y + noise (3e12 for the
    far-offset layout).  "high": phases near 1e7 rad -- about a metre of optical path at 0.5 um, the largest a pupil
    phase of this project's systems gets -- with a slope of hundreds of radians across the layout."""
    p = np.asarray(points, dtype=np.float64)
    rng = np.random.default_rng(seed)
    if kind == "plain":
        return 1e4 + 3.0 * p[:, 0] ** 2 - 2.0 * p[:, 1] + rng.normal(scale=1e-3, size=len(p))
    lo, span = p.min(axis=0), np.maximum(np.ptp(p, axis=0), 1e-300)
    u = 4.0 * (p - lo) / span - 2.0                                # [-2, 2]^2 whatever the layout's scale and offset
    return 1e7 + 500.0 * u[:, 0] ** 2 - 300.0 * u[:, 1] + rng.normal(scale=1.0, size=len(p))


def _centred(step, n):
    x = step * np.arange(n)
    return x - x.mean()


def layouts():
    """name -> (points (N, 2), xs, ys).  Small on purpose: every grid point meets every simplex in the restatement."""
    rng = np.random.default_rng(11)
    out = {}
    # a square lattice with the grid on its nodes, edge midpoints and cell centres (all on a diagonal or an edge),
    # and one ring of grid points outside the hull; every coordinate is exact in binary
    n = np.linspace(-1.0, 1.0, 17)
    out["lattice"] = (np.stack(np.meshgrid(n, n), axis=-1).reshape(-1, 2), np.linspace(-1.125, 1.125, 37),
                      np.linspace(-1.125, 1.125, 37))
    # 8 spokes x 9 radii from r = 0: the centre (a fan's chief ray) is listed 8 times; the grid has points on the
    # spokes y = 0, x = 0 and x = +-y
    r, ph = np.meshgrid(np.linspace(0.0, 1.0, 9), np.arange(8) * (np.pi / 4))
    out["fan_dup_centre"] = (np.stack((r * np.cos(ph), r * np.sin(ph)), axis=-1).reshape(-1, 2),
                             np.linspace(-1.125, 1.125, 37), np.linspace(-1.125, 1.125, 37))
    # a single triangle, with grid points on its vertices and edges
    out["one_triangle"] = (np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.linspace(-0.25, 1.25, 13),
                           np.linspace(-0.25, 1.25, 7))
    # one-row and one-column grids, 259 points: one full 256-thread block and a ragged second one
    scat = rng.uniform(-1.0, 1.0, (150, 2))
    out["one_row"] = (scat, np.linspace(-1.1, 1.1, 259), np.array([0.0371]))
    out["one_column"] = (scat, np.array([-0.0213]), np.linspace(-1.1, 1.1, 259))
    # a strip 1e-6 thin: cells a million times wider than high
    strip = rng.uniform(0.0, 1.0, (120, 2)) * np.array([1.0, 1e-6])
    out["thin_strip"] = (strip, np.linspace(-0.05, 1.05, 45), np.linspace(-0.1e-6, 1.1e-6, 25))
    # far from the origin: the cell index subtracts a large origin
    off = np.array([1e6, -1e6])
    far = rng.uniform(-1.0, 1.0, (150, 2)) + off
    out["far_offset"] = (far, off[0] + np.linspace(-1.1, 1.1, 41), off[1] + np.linspace(-1.1, 1.1, 29))
    # a square hull with collinear points along its edges (flat hull triangles), grid on the hull's edges
    e = np.linspace(-1.0, 1.0, 9)
    edge = np.concatenate([np.stack((e, np.full(9, -1.0)), 1), np.stack((e, np.full(9, 1.0)), 1),
                           np.stack((np.full(7, -1.0), e[1:-1]), 1), np.stack((np.full(7, 1.0), e[1:-1]), 1)])
    out["square_hull"] = (np.concatenate([edge, rng.uniform(-0.95, 0.95, (60, 2))]), np.linspace(-1.25, 1.25, 41),
                          np.linspace(-1.25, 1.25, 21))
    # the polar fan of test_gpu_griddata_matches_scipy, 21 rings x 13 spokes
    th, ph = np.meshgrid(np.linspace(-1, 1, 21), np.arange(13) * 2 * np.pi / 13)
    rr = 2.0 * np.sin(1.1 * th) / np.sin(1.1)
    out["polar_fan"] = (np.stack((rr * np.cos(ph), rr * np.sin(ph)), axis=-1).reshape(-1, 2), _centred(0.11, 45),
                        _centred(0.11, 45)[::2].copy())
    return out


class Case:
    """One layout, triangulated and tested against every simplex once; `phase(kind)` is the restated result for
    `values_for(points, kind)`.  Shared by the host and the GPU tests and never modified."""

    def __init__(self, name, points, xs, ys):
        from scipy.spatial import Delaunay
        self.name, self.points, self.xs, self.ys = name, points, xs, ys
        self.tri = Delaunay(points)
        self.acc_c = accepted(self.tri, xs, ys)
        self.n_accepting = self.acc_c[0].sum(axis=1).reshape(len(ys), len(xs))
        self._phase = {}

    def phase(self, kind="plain"):
        if kind not in self._phase:
            p = interpolate(self.tri, values_for(self.points, kind), self.xs, self.ys, self.acc_c)
            p.setflags(write=False)
            self._phase[kind] = p
        return self._phase[kind]


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name, *layouts()[name])
    return _CASES[name]


NAMES = tuple(layouts())
