"""The transmission statistics restated in NumPy (not a test module): the rule of include/rtpb.h's
rtpb_transmission_stats from a (1 + 2 S, rays, 8) history, the groups' media (n_groups, S + 1) and the coatings
(S, 2), one ufunc per rounded operation, in the order the header gives.

For surface s and one ray, A is the row in plane 2 s + 1 and B the row in plane 2 s + 2; the ray passes when A.xyz
and B.xyz are finite.  CONSTANT: t = value.  FRESNEL: t = 1 where n1 == n2, else g = n1 dA - n2 dB,
p1 = |(dA.x g.x + dA.y g.y) + dA.z g.z|, p2 likewise with dB, rs = (n1 p1 - n2 p2) / (n1 p1 + n2 p2),
rp = (n2 p1 - n1 p2) / (n2 p1 + n1 p2), t = 1 - 0.5 (rs rs + rp rp), 0 where that is NaN or outside [0, 1].
cum = cum * t over the surfaces; qt = rint(t 2^q), qc = rint(cum 2^q).  Columns: passes, sum qt, sum qc, min qc,
max qc.  The sums are sums of integers below 2^53: no column depends on the order of the rays.
"""
import numpy as np

NCOLS = 5
CONSTANT, FRESNEL = 0.0, 1.0


def fresnel_t(n1, n2, dA, dB):
    """t of the FRESNEL rule for arrays of indices (...,) and directions (..., 3)."""
    n1, n2 = np.broadcast_arrays(np.asarray(n1, dtype=np.float64), np.asarray(n2, dtype=np.float64))
    with np.errstate(all="ignore"):
        g = [n1 * dA[..., k] - n2 * dB[..., k] for k in range(3)]
        p1 = np.abs((dA[..., 0] * g[0] + dA[..., 1] * g[1]) + dA[..., 2] * g[2])
        p2 = np.abs((dB[..., 0] * g[0] + dB[..., 1] * g[1]) + dB[..., 2] * g[2])
        rs = (n1 * p1 - n2 * p2) / (n1 * p1 + n2 * p2)
        rp = (n2 * p1 - n1 * p2) / (n2 * p1 + n1 * p2)
        t = 1.0 - 0.5 * (rs * rs + rp * rp)
        t = np.where((t >= 0.0) & (t <= 1.0), t, 0.0)
    return np.where(n1 == n2, 1.0, t)


def trans_rays(history, media, coatings, group_size=None):
    """(t, cum), each (S, N) float64: per surface and ray the surface's transmittance and the product so far, NaN
    where the ray does not pass the surface."""
    history = np.asarray(history, dtype=np.float64)
    coatings = np.asarray(coatings, dtype=np.float64)
    S = (history.shape[0] - 1) // 2
    N = history.shape[1]
    group_size = N if group_size is None else group_size
    media = np.asarray(media, dtype=np.float64).reshape(N // group_size, S + 1)
    assert history.shape[0] == 2 * S + 1 and coatings.shape == (S, 2) and N % group_size == 0
    t_all, cum_all = np.empty((S, N)), np.empty((S, N))
    cum = np.ones(N)
    for s in range(S):
        A, B = history[2 * s + 1], history[2 * s + 2]
        passed = np.isfinite(A[:, 0:3]).all(axis=-1) & np.isfinite(B[:, 0:3]).all(axis=-1)
        n1, n2 = np.repeat(media[:, s], group_size), np.repeat(media[:, s + 1], group_size)
        if coatings[s, 0] == CONSTANT:
            t = np.full(N, coatings[s, 1])
        else:
            t = fresnel_t(n1, n2, A[:, 3:6], B[:, 3:6])
        t = np.where(passed, t, np.nan)
        cum = cum * t
        t_all[s], cum_all[s] = t, cum
    return t_all, cum_all


def trans_columns(history, media, coatings, q_bits, group_size=None):
    """(n_groups, S, 5) float64 from a (1 + 2 S, N, 8) history, N = n_groups * group_size (one group by default)."""
    t, cum = trans_rays(history, media, coatings, group_size)
    S, N = t.shape
    group_size = N if group_size is None else group_size
    G = N // group_size
    scale = np.ldexp(1.0, q_bits)
    passed = ~np.isnan(t)                   # (a passing ray's t is a number: FRESNEL's NaN becomes 0)
    with np.errstate(invalid="ignore"):
        qt = np.where(passed, np.rint(t * scale), 0.0).reshape(S, G, group_size)
        qc = np.rint(cum * scale).reshape(S, G, group_size)
    passed = passed.reshape(S, G, group_size)
    out = np.empty((G, S, NCOLS))
    out[..., 0] = passed.sum(axis=-1).T
    out[..., 1] = qt.sum(axis=-1).T
    out[..., 2] = np.where(passed, qc, 0.0).sum(axis=-1).T
    out[..., 3] = np.where(passed, qc, np.inf).min(axis=-1).T
    out[..., 4] = np.where(passed, qc, -np.inf).max(axis=-1).T
    return out
