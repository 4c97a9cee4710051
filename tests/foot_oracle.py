"""The footprint statistics restated in NumPy (not a test module): the eight columns of include/rtpb.h's
rtpb_footprint_stats from a (1 + 2 S, rays, 8) history and (S, 9) frames, in the operation order the header gives.

For surface s and one ray, A is the row in plane 2 s + 1 and B the row in plane 2 s + 2; the frame is (o, e1, e2).
The ray arrives when A.xyz is finite and passes when B.xyz is finite too;  q = A.xyz - o,
u = (q.x e1.x + q.y e1.y) + q.z e1.z, v likewise with e2, rho2 = u u + v v.  Columns: arrivals, passes, max rho2 over
the arrivals, max rho2 over the passes, min / max u and min / max v over the passes; -inf / +inf for an empty set,
NaN skipped (np.fmax / np.fmin).  Counts, maxima and minima: no column depends on the order of the rays.
"""
import numpy as np

NCOLS = 8


def default_frames(S_dicts):
    """(S, 9) frames of axial systems from the oracle's surface dicts: the centre, x and y (what
    analysis.footprint_frames gives for an input_axis of (0, 0, 1))."""
    out = np.zeros((len(S_dicts), 9))
    for k, s in enumerate(S_dicts):
        out[k, 0:3] = s["center"]
        out[k, 3:6] = (1.0, 0.0, 0.0)
        out[k, 6:9] = (0.0, 1.0, 0.0)
    return out


def _fmax(values, mask):
    return np.fmax.reduce(np.where(mask, values, -np.inf), axis=-1, initial=-np.inf)


def _fmin(values, mask):
    return np.fmin.reduce(np.where(mask, values, np.inf), axis=-1, initial=np.inf)


def foot_columns(history, frames, group_size=None):
    """(n_groups, S, 8) float64 from a (1 + 2 S, N, 8) history, N = n_groups * group_size (one group by default)."""
    history = np.asarray(history, dtype=np.float64)
    frames = np.asarray(frames, dtype=np.float64)
    S = (history.shape[0] - 1) // 2
    assert history.shape[0] == 2 * S + 1 and frames.shape == (S, 9)
    N = history.shape[1]
    group_size = N if group_size is None else group_size
    assert N % group_size == 0
    G = N // group_size
    out = np.empty((G, S, NCOLS))
    with np.errstate(all="ignore"):
        for s in range(S):
            A = history[2 * s + 1, :, 0:3].reshape(G, group_size, 3)
            B = history[2 * s + 2, :, 0:3].reshape(G, group_size, 3)
            o, e1, e2 = frames[s, 0:3], frames[s, 3:6], frames[s, 6:9]
            arrive = np.isfinite(A).all(axis=-1)
            passed = arrive & np.isfinite(B).all(axis=-1)
            qx, qy, qz = A[..., 0] - o[0], A[..., 1] - o[1], A[..., 2] - o[2]
            u = (qx * e1[0] + qy * e1[1]) + qz * e1[2]
            v = (qx * e2[0] + qy * e2[1]) + qz * e2[2]
            rho2 = u * u + v * v
            out[:, s, 0] = arrive.sum(axis=-1)
            out[:, s, 1] = passed.sum(axis=-1)
            out[:, s, 2] = _fmax(rho2, arrive)
            out[:, s, 3] = _fmax(rho2, passed)
            out[:, s, 4] = _fmin(u, passed)
            out[:, s, 5] = _fmax(u, passed)
            out[:, s, 6] = _fmin(v, passed)
            out[:, s, 7] = _fmax(v, passed)
    return out
