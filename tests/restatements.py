"""The kernels' rules and reduction orders restated in NumPy (not a test module): the oracles the bitwise GPU tests
rest on.  Each function says which kernel it restates; the host tests named there check it on values worked out by
hand (tests/test_image_host.py, test_energy_host.py, test_wavemap_host.py, test_psf_host.py), the GPU tests compare
the kernels with it.  wave_oracle.py (the wavefront terms and their sums), foot_oracle.py (the footprint columns) and
griddata_oracle.py are restatements too, each with its own module.

Tolerance of the PSF comparison (``bound``; derived, not measured).  Device and ``psf_of_plane`` differ only in (1)
the sine and cosine: the device's sincospi is within 2 ulp, NumPy rounds 2 pi fr once (a relative 2^-53 of an argument
of at most pi: at most 3.5e-16 absolute in a function of slope at most 1) and is then within 1 ulp: together under
1.3e-15 per term of size at most 1; (2) the rounded product with a, 2^-53 relative; (3) the rounding of a sum of N
terms, at most N * 2^-53 times the sum of the terms' magnitudes in any order.  So each of re and im may differ by at
most norm_abs * (8e-15 + 4 * N * 2^-53) with norm_abs the sum of |a| over the counting rays and N the group size: the
constant is about six times the per-term bound, the factor 4 covers both sides' sums twice over."""
import numpy as np

from ray_trace_pb_amd import analysis
from parity import bits
import wave_oracle as W

CHUNK_ELEMS = 1 << 22                   # the (rays x pixels) temporaries of psf_of_plane stay under 32 MiB


def fixed_order_sums(plane, group_size, tile=256):
    """The spot kernels' reduction restated in NumPy, operation for operation (csrc/rtpb_analysis.hip
    spot_partial_kernel + spot_final_kernel, csrc/rtpb_sweep.hip sweep_kernel): per 256-ray tile a pairwise tree
    (red[t] += red[t + w], w = 128 ... 1) of (1, x, y, z, x*x, y*y, x*y) over rays with finite x and y;
    per group, thread t adds tiles t, t + 256, ... in order, then the same tree over the 256 threads."""
    p = np.asarray(plane, dtype=np.float64).reshape(-1, group_size, plane.shape[-1])
    G = p.shape[0]
    tiles = -(-group_size // tile)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(invalid="ignore"):
        ok = (x - x == 0.0) & (y - y == 0.0)
    v = np.zeros((G, tiles * tile, 7))
    with np.errstate(invalid="ignore", over="ignore"):
        terms = np.stack((np.ones_like(x), x, y, z, x * x, y * y, x * y), -1)
    v[:, :group_size] = np.where(ok[..., None], terms, 0.0)
    v = v.reshape(G, tiles, tile, 7)
    w = tile // 2
    while w:
        v[:, :, :w] = v[:, :, :w] + v[:, :, w:2 * w]
        w //= 2
    part = v[:, :, 0]                                            # (G, tiles, 7)
    acc = np.zeros((G, tile, 7))
    for c in range(0, tiles, tile):
        blk = part[:, c:c + tile]
        acc[:, :blk.shape[1]] = acc[:, :blk.shape[1]] + blk
    w = tile // 2
    while w:
        acc[:, :w] = acc[:, :w] + acc[:, w:2 * w]
        w //= 2
    return acc[:, 0]


def fixed_order_focus_sums(plane, group_size, tile=256):
    """The focus kernels' reduction restated in NumPy, operation for operation (csrc/rtpb_stats.h focus_ray /
    focus_term, rtpb_analysis.hip focus_partial_kernel + spot_final_kernel, rtpb_sweep.hip sweep_kernel):
    u = dx / dz, v = dy / dz; a ray counts when x, y, u and v are finite; per 256-ray tile a pairwise tree
    (red[t] += red[t + w], w = 128 ... 1) of the sixteen terms; per group, thread t adds tiles t, t + 256, ... in order, then the same tree over the 256 threads."""
    p = np.asarray(plane, dtype=np.float64).reshape(-1, group_size, plane.shape[-1])
    G = p.shape[0]
    tiles = -(-group_size // tile)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u, v = p[..., 3] / p[..., 5], p[..., 4] / p[..., 5]
        ok = (x - x == 0.0) & (y - y == 0.0) & (u - u == 0.0) & (v - v == 0.0)
        terms = np.stack((np.ones_like(x), x, y, z, x * x, y * y, x * y, u, v, u * u, v * v, u * v, x * u, y * v,
                          x * v, y * u), -1)
    acc = np.zeros((G, tiles * tile, 16))
    acc[:, :group_size] = np.where(ok[..., None], terms, 0.0)
    acc = acc.reshape(G, tiles, tile, 16)
    w = tile // 2
    while w:
        acc[:, :, :w] = acc[:, :, :w] + acc[:, :, w:2 * w]
        w //= 2
    part = acc[:, :, 0]                                           # (G, tiles, 16)
    fin = np.zeros((G, tile, 16))
    for c in range(0, tiles, tile):
        blk = part[:, c:c + tile]
        fin[:, :blk.shape[1]] = fin[:, :blk.shape[1]] + blk
    w = tile // 2
    while w:
        fin[:, :w] = fin[:, :w] + fin[:, w:2 * w]
        w //= 2
    return fin[:, 0]


def image_of_plane(plane, group_size, windows, nx, ny):
    """(image (G, ny, nx) int32, outside (G,) int32) of an (N, 8) plane (float64 values: a float32 plane widened),
    N = G * group_size, with windows (G, 4) float64."""
    plane = np.asarray(plane, dtype=np.float64)
    w = np.asarray(windows, dtype=np.float64).reshape(-1, 4)
    G = plane.shape[0] // group_size
    assert plane.shape[0] == G * group_size and w.shape[0] == G
    x, y = plane[:, 0].reshape(G, group_size), plane[:, 1].reshape(G, group_size)
    image = np.zeros((G, ny, nx), dtype=np.int32)
    outside = np.zeros(G, dtype=np.int32)
    with np.errstate(all="ignore"):
        counts = np.isfinite(x) & np.isfinite(y)
        tx = (x - w[:, 0:1]) * w[:, 2:3]
        ty = (y - w[:, 1:2]) * w[:, 3:4]
        inside = counts & (tx >= 0) & (tx < nx) & (ty >= 0) & (ty < ny)
    for g in range(G):
        ix = tx[g, inside[g]].astype(np.int64)           # (truncation, as the C cast; the values are in [0, nx))
        iy = ty[g, inside[g]].astype(np.int64)
        np.add.at(image[g], (iy, ix), 1)
        outside[g] = np.count_nonzero(counts[g] & ~inside[g])
    return image, outside


def energy_of_plane(plane, group_size, params, nr):
    """(hist (G, 2, nr) int32, outside (G, 2) int32, farthest (G, 2) float64) of an (N, 8) plane (float64 values: a
    float32 plane widened), N = G * group_size, with params (G, 4) float64."""
    plane = np.asarray(plane, dtype=np.float64)
    p = np.asarray(params, dtype=np.float64).reshape(-1, 4)
    G = plane.shape[0] // group_size
    assert plane.shape[0] == G * group_size and p.shape[0] == G
    x, y = plane[:, 0].reshape(G, group_size), plane[:, 1].reshape(G, group_size)
    hist = np.zeros((G, 2, nr), dtype=np.int32)
    outside = np.zeros((G, 2), dtype=np.int32)
    farthest = np.zeros((G, 2))
    with np.errstate(all="ignore"):
        counts = np.isfinite(x) & np.isfinite(y)
        centred = np.isfinite(p[:, 0:1]) & np.isfinite(p[:, 1:2])
        dx, dy = x - p[:, 0:1], y - p[:, 1:2]
        rho = np.sqrt(dx * dx + dy * dy)
        m = np.maximum(np.abs(dx), np.abs(dy))
        dist = np.stack((rho, m), axis=1)                               # (G, 2, group_size)
        t = dist * p[:, 2].reshape(G, 1, 1)
        inside = (counts & centred)[:, None, :] & (t >= 0) & (t < nr)
    for g in range(G):
        for k in range(2):
            sel = inside[g, k]
            np.add.at(hist[g, k], t[g, k, sel].astype(np.int64), 1)     # (truncation, as the C cast; in [0, nr))
            outside[g, k] = np.count_nonzero(counts[g] & ~sel)
            if centred[g, 0] and counts[g].any():
                farthest[g, k] = dist[g, k, counts[g]].max()
    return hist, outside, farthest


def wavemap_of_plane(plane, group_size, refs, windows, bins, q_bits, w_lim):
    """(count (G, ny, nx) int32, sum (G, ny, nx) int64, outside (G,) int32, clipped (G,) int32, farthest (G, 2)) of an
    (N, 8) float64 plane, N = G * group_size, against refs (G, 8) and windows (G, 4)."""
    nx, ny = bins
    t = W.wave_terms(plane, group_size, refs)
    G = t.shape[0]
    win = np.asarray(windows, dtype=np.float64).reshape(G, 1, 4)
    n, w, ex, ey = t[..., 0] != 0.0, t[..., 1], t[..., 3], t[..., 4]
    with np.errstate(all="ignore"):
        tx, ty = (ex - win[..., 0]) * win[..., 2], (ey - win[..., 1]) * win[..., 3]
        inside = n & (tx >= 0.0) & (tx < nx) & (ty >= 0.0) & (ty < ny)
        keep = inside & (np.abs(w) <= w_lim)
        q = np.rint(w * 2.0 ** q_bits)
    count = np.zeros((G, ny * nx), dtype=np.int32)
    total = np.zeros((G, ny * nx), dtype=np.int64)
    farthest = np.zeros((G, 2))
    for g in range(G):
        k = keep[g]
        b = ty[g, k].astype(np.int64) * nx + tx[g, k].astype(np.int64)     # (truncation, as the C cast)
        np.add.at(count[g], b, 1)
        np.add.at(total[g], b, q[g, k].astype(np.int64))
        if n[g].any():
            farthest[g] = (np.maximum(np.abs(ex[g, n[g]]), np.abs(ey[g, n[g]])).max(), np.abs(w[g, n[g]]).max())
    outside = (n & ~inside).sum(axis=1).astype(np.int32)
    clipped = (inside & ~keep).sum(axis=1).astype(np.int32)
    return count.reshape(G, ny, nx), total.reshape(G, ny, nx), outside, clipped, farthest


def same_map(got, exp):
    """count, sum, outside and clipped == as integers of the right types, farthest the same bits."""
    return (got[0].dtype == np.int32 and got[1].dtype == np.int64 and all(np.array_equal(a, b) for a, b in
                                                                           zip(got[:4], exp[:4])) and
            got[4].shape == exp[4].shape and np.array_equal(bits(got[4]), bits(exp[4])))


def two_pass(plane, group_size, refs, bins):
    """The sweeps' default window, limit and q_bits, from the restatement's own first pass: (windows, w_lim, q_bits)."""
    G = plane.shape[0] // group_size
    unit = np.tile([-1.0, -1.0, 0.5, 0.5], (G, 1))
    far = wavemap_of_plane(plane, group_size, refs, unit, (1, 1), 0, 0.0)[4]
    w_lim = max(1.0, float(far[:, 1].max()))
    return analysis.wavefront_map_windows(far[:, 0], bins), w_lim, analysis.wavefront_map_q_bits(group_size, w_lim)


def psf_of_plane(plane, group_size, refs, windows, weights, nx, ny):
    """The rule of rtpb_huygens_psf in NumPy: (field (G, ny, nx) complex128, norm (G,), norm_abs (G,), count (G,)) of
    an (N, 8) float64 plane against refs (G, 8) and windows (G, 4); weights (group_size,) or None.  norm_abs is the
    sum of |a| over the counting rays (what the tolerance scales with), count their number."""
    terms = W.wave_terms(plane, group_size, refs)                     # (G, per, 15): n, w, ., ex, ey
    refs = np.asarray(refs, dtype=np.float64).reshape(-1, 8)
    windows = np.asarray(windows, dtype=np.float64).reshape(-1, 4)
    G = terms.shape[0]
    wt = np.ones(group_size) if weights is None else np.asarray(weights, dtype=np.float64)
    field = np.zeros((G, ny, nx), dtype=np.complex128)
    norm, norm_abs, count = np.zeros(G), np.zeros(G), np.zeros(G, dtype=np.int64)
    ix, iy = np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64)
    for g in range(G):
        counts = terms[g, :, 0] == 1.0
        kf = refs[g, 7]
        with np.errstate(invalid="ignore", over="ignore"):
            a = (terms[g, :, 0] * wt)[counts]                          # (a ray that does not count is skipped)
            w = terms[g, counts, 1]
            qx, qy = terms[g, counts, 3] * kf, terms[g, counts, 4] * kf
            X = (ix - windows[g, 0]) * windows[g, 2]
            Y = (iy - windows[g, 1]) * windows[g, 3]
            re, im = np.zeros((ny, nx)), np.zeros((ny, nx))
            rows = max(1, CHUNK_ELEMS // (nx * ny))
            for k in range(0, a.size, rows):
                s = slice(k, k + rows)
                t = (w[s, None, None] + qx[s, None, None] * X[None, None, :]) + qy[s, None, None] * Y[None, :, None]
                fr = t - np.rint(t)
                re += (a[s, None, None] * np.cos(2 * np.pi * fr)).sum(axis=0)
                im += (a[s, None, None] * np.sin(2 * np.pi * fr)).sum(axis=0)
        field[g] = re + 1j * im
        norm[g], norm_abs[g], count[g] = a.sum(), np.abs(a).sum(), a.size
    return field, norm, norm_abs, count


def bound(norm_abs, group_size):
    """The derived bound on |device - restatement| of re and of im (the module docstring)."""
    return norm_abs * (8e-15 + 4 * group_size * 2.0 ** -53)
