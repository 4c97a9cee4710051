"""The polarisation statistics restated in NumPy (not a test module): the rule of csrc/rtpb_pol.h's comment from a
(1 + 2 S, rays, 8) history, the groups' media (n_groups, S + 1), the coatings (S, 2) = (mode, value) and the two axes,
one ufunc per rounded operation, in the order the header gives.  Written from that text, not from the C++.

Each ray carries E1 and E2, or no state (NaN).  Launch from the first direction a (plane 0) and the polariser u:
c = a x u, cc = c . c, no state unless cc >= 2^-40; w = c x a, E1 = w / sqrt(w . w), E2 = a x E1.  At surface s, A is
the row in plane 2 s + 1 and B the row in plane 2 s + 2, a = A.dxyz, b = B.dxyz; the ray passes when A.xyz and B.xyz
are finite, and a ray that does not pass has no state from then on.  CONSTANT: ts = tp = sqrt(value); FRESNEL: ts = tp
= 1 where n1 == n2, else sqrt(1 - rs rs), sqrt(1 - rp rp) with the transmission rule's ratios; then c = a x b, k =
(ts - tp) ((E . c) / cc) where cc >= 2^-900 else 0, E' = tp E + k c, E_out = E' - (a + b) ((E' . b) / (1 + a . b)),
no state unless 1 + a . b >= 2^-20.  MIRROR: m = a - b, E_out = sqrt(value) ((2 ((E . m) / mm)) m - E), no state unless
mm >= 2^-40.  Analyser: x = b x w_an, l_i = (E_i . x)^2 / xx; valid = passes, six finite components, xx >= 2^-40.
Columns: passes, valid, then over the valid rays the sums of rint(min(v, 1) 2^q) for v = |E1|^2, |E2|^2, l1, l2.
"""
import numpy as np

NCOLS = 6
CONSTANT, FRESNEL, MIRROR = 0.0, 1.0, 2.0
LAUNCH_MIN, PLANE_MIN, TURN_MIN = 2.0 ** -40, 2.0 ** -900, 2.0 ** -20


def dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def cross(p, q):
    return np.stack((p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]), axis=-1)


def unit(v):
    """An axis as the Python layer normalises it: v / sqrt(v . v), componentwise."""
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(dot(v, v))


def ratios(n1, n2, a, b):
    """(rs, rp) of the transmission rule (trans_ratios) for indices (...,) and directions (..., 3)."""
    g = np.stack([n1 * a[..., k] - n2 * b[..., k] for k in range(3)], axis=-1)
    p1, p2 = np.abs(dot(a, g)), np.abs(dot(b, g))
    return (n1 * p1 - n2 * p2) / (n1 * p1 + n2 * p2), (n2 * p1 - n1 * p2) / (n2 * p1 + n1 * p2)


def amplitudes(n1, n2, a, b):
    """(ts, tp) of a FRESNEL surface."""
    n1, n2 = np.broadcast_arrays(np.asarray(n1, dtype=np.float64), np.asarray(n2, dtype=np.float64))
    with np.errstate(all="ignore"):
        rs, rp = ratios(n1, n2, a, b)
        ts, tp = np.sqrt(1.0 - rs * rs), np.sqrt(1.0 - rp * rp)
    same = n1 == n2
    return np.where(same, 1.0, ts), np.where(same, 1.0, tp)


def launch(a, u):
    """(N, 2, 3): E1 and E2 of rays with directions a (N, 3) behind a polariser along the unit vector u."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        c = cross(a, np.broadcast_to(u, a.shape))
        cc = dot(c, c)
        w = cross(c, a)
        e1 = w / np.sqrt(dot(w, w))[:, None]
        e2 = cross(a, e1)
    e = np.stack((e1, e2), axis=1)
    e[~(cc >= LAUNCH_MIN)] = np.nan
    return e


def refract(e, a, b, ts, tp):
    """A CONSTANT or FRESNEL surface: e (N, 2, 3) in, (N, 2, 3) out."""
    with np.errstate(all="ignore"):
        c = cross(a, b)
        cc = dot(c, c)
        d = 1.0 + dot(a, b)
        s = a + b
        out = np.empty_like(e)
        for i in range(2):
            E = e[:, i]
            k = np.where(cc >= PLANE_MIN, (ts - tp) * (dot(E, c) / cc), 0.0)
            P = tp[:, None] * E + k[:, None] * c
            f = dot(P, b) / d
            out[:, i] = P - s * f[:, None]
    out[~(d >= TURN_MIN)] = np.nan
    return out


def mirror(e, a, b, amp):
    with np.errstate(all="ignore"):
        m = a - b
        mm = dot(m, m)
        out = np.empty_like(e)
        for i in range(2):
            E = e[:, i]
            g2 = 2.0 * (dot(E, m) / mm)
            out[:, i] = amp * (g2[:, None] * m - E)
    out[~(mm >= LAUNCH_MIN)] = np.nan
    return out


def pol_rays(history, media, coatings, u, w_an, group_size=None):
    """(states, l, passed, valid): per surface and ray the state after the surface (S, N, 2, 3), NaN for none; the two
    crossed-analyser energies (S, N, 2); whether the ray passes and whether it is valid (S, N)."""
    history = np.asarray(history, dtype=np.float64)
    coatings = np.asarray(coatings, dtype=np.float64)
    w_an = np.asarray(w_an, dtype=np.float64)
    S = (history.shape[0] - 1) // 2
    N = history.shape[1]
    group_size = N if group_size is None else group_size
    media = np.asarray(media, dtype=np.float64).reshape(N // group_size, S + 1)
    assert history.shape[0] == 2 * S + 1 and coatings.shape == (S, 2) and N % group_size == 0
    states, ls = np.empty((S, N, 2, 3)), np.empty((S, N, 2))
    passed_all, valid_all = np.empty((S, N), dtype=bool), np.empty((S, N), dtype=bool)
    e = launch(history[0][:, 3:6], u)
    for s in range(S):
        A, B = history[2 * s + 1], history[2 * s + 2]
        a, b = A[:, 3:6], B[:, 3:6]
        passed = np.isfinite(A[:, 0:3]).all(axis=-1) & np.isfinite(B[:, 0:3]).all(axis=-1)
        mode, value = coatings[s]
        if mode == MIRROR:
            e = mirror(e, a, b, np.sqrt(value))
        else:
            if mode == CONSTANT:
                ts = tp = np.full(N, np.sqrt(value))
            else:
                ts, tp = amplitudes(np.repeat(media[:, s], group_size), np.repeat(media[:, s + 1], group_size), a, b)
            e = refract(e, a, b, ts, tp)
        e[~passed] = np.nan
        with np.errstate(all="ignore"):
            x = cross(b, np.broadcast_to(w_an, b.shape))
            xx = dot(x, x)
            p = np.stack((dot(e[:, 0], x), dot(e[:, 1], x)), axis=-1)
            ls[s] = (p * p) / xx[:, None]
        states[s] = e
        passed_all[s] = passed
        valid_all[s] = passed & np.isfinite(e).all(axis=(1, 2)) & (xx >= LAUNCH_MIN)
    return states, ls, passed_all, valid_all


def quant(v, scale):
    with np.errstate(invalid="ignore"):
        return np.rint(np.where(v <= 1.0, v, 1.0) * scale)


def pol_columns(history, media, coatings, u, w_an, q_bits, group_size=None):
    """(n_groups, S, 6) float64 from a (1 + 2 S, N, 8) history, N = n_groups * group_size (one group by default)."""
    states, ls, passed, valid = pol_rays(history, media, coatings, u, w_an, group_size)
    S, N = passed.shape
    group_size = N if group_size is None else group_size
    G = N // group_size
    scale = np.ldexp(1.0, q_bits)
    with np.errstate(all="ignore"):
        terms = [dot(states[:, :, 0], states[:, :, 0]), dot(states[:, :, 1], states[:, :, 1]), ls[..., 0], ls[..., 1]]
    out = np.empty((G, S, NCOLS))
    out[..., 0] = passed.reshape(S, G, group_size).sum(axis=-1).T
    out[..., 1] = valid.reshape(S, G, group_size).sum(axis=-1).T
    for k, v in enumerate(terms):
        out[..., 2 + k] = np.where(valid, quant(v, scale), 0.0).reshape(S, G, group_size).sum(axis=-1).T
    return out
