// rtpb_pol.h -- the polarisation statistics' per-ray rule (rtpb_polarisation_stats / rtpb_polarisation_sweep /
// rtpb_ray_polarisation), free of HIP so that a plain C++ build can run it (tests/native/pol_harness.cpp); the
// kernels get it through rtpb_stats.h.
//
// Each ray carries two real field vectors E1 and E2 (six doubles: the STATE), both perpendicular to the ray, or NO
// state (all six NaN).  |E|^2 is energy.  The call gives a unit POLARISER axis u and a unit ANALYSER axis w_an.  For
// one surface s and one ray: A is the ray's row in history plane 2s + 1 (the position at the surface and the INCOMING
// direction a = A.dxyz), B its row in plane 2s + 2 (the OUTGOING direction b = B.dxyz), n1 and n2 the indices before
// and after the surface at the group's wavelength.  The surface's COATING is kTransCoat doubles {mode, amplitude}.
// float64 only, every operation one rounded IEEE operation in this order (no FMA); with
//   p . q = (p.x q.x + p.y q.y) + p.z q.z
//   p x q = (p.y q.z - p.z q.y,  p.z q.x - p.x q.z,  p.x q.y - p.y q.x)
// and sqrt the correctly rounded root (tsqrt<double>):
//   LAUNCH from the ray's first direction a (history plane 0; the fused sweep: the generated ray's):
//       c = a x u,  cc = c . c;  !(cc >= 2^-40): no state (a ray along the polariser axis, or a NaN direction).  Else
//       w = c x a,  r = sqrt(w . w),  E1 = w / r (three divisions),  E2 = a x E1
//   the ray PASSES exactly when the footprint and transmission statistics say so: A.xyz finite and B.xyz finite; a ray
//   that does not pass has no state from then on
//   mode 0 (CONSTANT; the host uploads amplitude = sqrt(value)) and mode 1 (FRESNEL, uncoated; amplitude ignored):
//       CONSTANT: ts = tp = amplitude.  FRESNEL where n1 == n2: ts = tp = 1.  FRESNEL else: rs, rp = trans_ratios
//       (rtpb_trans.h, unchanged), ts = sqrt(1 - rs rs), tp = sqrt(1 - rp rp): the flux-normalised amplitudes
//       c = a x b,  cc = c . c,  d = 1 + a . b;  !(d >= 2^-20): no state (a reversal).  Else for E = E1 and E = E2:
//       k  = (ts - tp) ((E . c) / cc) where cc >= 2^-900, else 0
//       E' = tp E + k c                                   (componentwise: tp E.x + k c.x)
//       f  = (E' . b) / d,   E_out = E' - (a + b) f       (componentwise: E'.x - (a.x + b.x) f)
//     first the two transmission amplitudes along s (c, the normal of the plane of incidence) and p, then the minimal
//     rotation that takes a to b; E_out . b = 0 by construction, also where b equals a up to rounding.
//   mode 2 (MIRROR; the host uploads amplitude = sqrt(reflectance)):
//       m = a - b,  mm = m . m;  !(mm >= 2^-40): no state (nothing was reflected).  Else for E = E1 and E = E2:
//       g = (E . m) / mm,   E_out = amplitude ((2 g) m - E)   (componentwise: amplitude ((2 g) m.x - E.x))
//   a state that was NaN stays NaN through either form.
//   the ANALYSER, after the surface:  x = b x w_an,  xx = x . x;  for i = 1, 2:  p = E_i . x,  l_i = (p p) / xx: the
//   energy of state i behind an analyser CROSSED with w_an
//   the ray is VALID at s when it passes, all six components of E_out are finite and xx >= 2^-40
//   q(v) = rint((v <= 1 ? v : 1) 2^q_bits)
// The kPolCols statistics of a (group, surface): 0 the rays that pass, 1 the valid rays, 2 ... 5 the sums over the valid
// rays of q(E1 . E1), q(E2 . E2), q(l1), q(l2).  All integer-valued: with group_size * 2^q_bits <= 2^53 every sum is
// exact in any order.
// No normal, no surface kind.  Real amplitudes only: no retardance (total internal reflection, metal mirrors), no thin
// films, no birefringence.
#pragma once

#include "rtpb_trans.h"

namespace rtpb {

constexpr int kPolCols = 6;
constexpr int kPolState = 6;               // E1.xyz, E2.xyz
constexpr double kCoatMirror = 2.0;
constexpr double kPolLaunchMin = 0x1p-40;  // c . c of the launch, m . m of a mirror, x . x of the analyser
constexpr double kPolPlaneMin = 0x1p-900;  // c . c below which a refraction has no plane of incidence
constexpr double kPolTurnMin = 0x1p-20;    // 1 + a . b
struct PolRay {
    double v[kPolCols];
};

RTPB_HD PolRay pol_none() { return PolRay{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}}; }

// What the host uploads for a coating {mode, value}: the amplitude sqrt(value) of a CONSTANT or a MIRROR, once per
// call (FRESNEL ignores it)
RTPB_HD double pol_coat_amplitude(double mode, double value) {
    return mode == kCoatFresnel ? value : tsqrt<double>(value);
}

RTPB_HD double pol_dot(double px, double py, double pz, double qx, double qy, double qz) {
    return (px * qx + py * qy) + pz * qz;
}

RTPB_HD void pol_cross(double px, double py, double pz, double qx, double qy, double qz, double& x, double& y,
                       double& z) {
    x = py * qz - pz * qy;
    y = pz * qx - px * qz;
    z = px * qy - py * qx;
}

RTPB_HD void pol_clear(double (&e)[kPolState]) {
#pragma unroll
    for (int k = 0; k < kPolState; ++k) e[k] = __builtin_nan("");
}

// The launch: the state of a ray with direction a behind a polariser along u
RTPB_HD void pol_launch(double ax, double ay, double az, const double (&u)[3], double (&e)[kPolState]) {
    double cx, cy, cz;
    pol_cross(ax, ay, az, u[0], u[1], u[2], cx, cy, cz);
    const double cc = pol_dot(cx, cy, cz, cx, cy, cz);
    if (!(cc >= kPolLaunchMin)) {
        pol_clear(e);
        return;
    }
    double wx, wy, wz;
    pol_cross(cx, cy, cz, ax, ay, az, wx, wy, wz);
    const double r = tsqrt<double>(pol_dot(wx, wy, wz, wx, wy, wz));
    e[0] = wx / r;
    e[1] = wy / r;
    e[2] = wz / r;
    pol_cross(ax, ay, az, e[0], e[1], e[2], e[3], e[4], e[5]);
}

// The two transmission amplitudes of a CONSTANT or FRESNEL surface
RTPB_HD void pol_amplitudes(double n1, double n2, double ax, double ay, double az, double bx, double by, double bz,
                            double coat_mode, double coat_amp, double& ts, double& tp) {
    if (coat_mode == kCoatConstant) {
        ts = tp = coat_amp;
    } else if (n1 == n2) {
        ts = tp = 1.0;
    } else {
        double rs, rp;
        trans_ratios(n1, n2, ax, ay, az, bx, by, bz, rs, rp);
        ts = tsqrt<double>(1.0 - rs * rs);
        tp = tsqrt<double>(1.0 - rp * rp);
    }
}

// One surface for one ray: a and b the incoming and outgoing directions; e the state coming in and going out.
// `passes`: A.xyz and B.xyz are finite.
RTPB_HD void pol_surface(bool passes, double ax, double ay, double az, double bx, double by, double bz, double n1,
                         double n2, double coat_mode, double coat_amp, double (&e)[kPolState]) {
    if (!passes) {
        pol_clear(e);
        return;
    }
    if (coat_mode == kCoatMirror) {
        const double mx = ax - bx, my = ay - by, mz = az - bz;
        const double mm = pol_dot(mx, my, mz, mx, my, mz);
        if (!(mm >= kPolLaunchMin)) {
            pol_clear(e);
            return;
        }
#pragma unroll
        for (int i = 0; i < kPolState; i += 3) {
            const double g = pol_dot(e[i], e[i + 1], e[i + 2], mx, my, mz) / mm;
            const double g2 = 2.0 * g;
            e[i] = coat_amp * (g2 * mx - e[i]);
            e[i + 1] = coat_amp * (g2 * my - e[i + 1]);
            e[i + 2] = coat_amp * (g2 * mz - e[i + 2]);
        }
        return;
    }
    double ts, tp;
    pol_amplitudes(n1, n2, ax, ay, az, bx, by, bz, coat_mode, coat_amp, ts, tp);
    double cx, cy, cz;
    pol_cross(ax, ay, az, bx, by, bz, cx, cy, cz);
    const double cc = pol_dot(cx, cy, cz, cx, cy, cz);
    const double d = 1.0 + pol_dot(ax, ay, az, bx, by, bz);
    if (!(d >= kPolTurnMin)) {
        pol_clear(e);
        return;
    }
    const double sx = ax + bx, sy = ay + by, sz = az + bz;
    const double dt = ts - tp;
#pragma unroll
    for (int i = 0; i < kPolState; i += 3) {
        double k = 0.0;
        if (cc >= kPolPlaneMin) k = dt * (pol_dot(e[i], e[i + 1], e[i + 2], cx, cy, cz) / cc);
        const double px = tp * e[i] + k * cx, py = tp * e[i + 1] + k * cy, pz = tp * e[i + 2] + k * cz;
        const double f = pol_dot(px, py, pz, bx, by, bz) / d;
        e[i] = px - sx * f;
        e[i + 1] = py - sy * f;
        e[i + 2] = pz - sz * f;
    }
}

RTPB_HD double pol_quant(double v, double scale) { return __builtin_rint((v <= 1.0 ? v : 1.0) * scale); }

// A passing ray's term after the surface: b the outgoing direction, w the analyser axis, scale = 2^q_bits
RTPB_HD PolRay pol_term(const double (&e)[kPolState], double bx, double by, double bz, const double (&w)[3],
                        double scale) {
    PolRay o = pol_none();
    o.v[0] = 1.0;
    double qx, qy, qz;                          // x = b x w_an
    pol_cross(bx, by, bz, w[0], w[1], w[2], qx, qy, qz);
    const double xx = pol_dot(qx, qy, qz, qx, qy, qz);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < kPolState; ++k) finite = finite && e[k] - e[k] == 0.0;
    if (!(finite && xx >= kPolLaunchMin)) return o;
    o.v[1] = 1.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double ex = e[3 * i], ey = e[3 * i + 1], ez = e[3 * i + 2];
        const double p = pol_dot(ex, ey, ez, qx, qy, qz);
        o.v[2 + i] = pol_quant(pol_dot(ex, ey, ez, ex, ey, ez), scale);
        o.v[4 + i] = pol_quant((p * p) / xx, scale);
    }
    return o;
}

RTPB_HD void pol_merge(PolRay& a, const PolRay& b) {
#pragma unroll
    for (int c = 0; c < kPolCols; ++c) a.v[c] = a.v[c] + b.v[c];
}

}  // namespace rtpb
