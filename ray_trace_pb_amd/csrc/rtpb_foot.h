// rtpb_foot.h -- the footprint statistics' per-ray term (rtpb_footprint_stats / rtpb_footprint_sweep), free of HIP so
// that a plain C++ build can run it (tests/native/foot_harness.cpp); the kernels get it through rtpb_stats.h.
//
// For one surface s and one ray: A is the ray's row in history plane 2s + 1 (at the surface: the intersection point,
// which the reference keeps where the ray falls outside the aperture), B its row in plane 2s + 2 (after it).  The
// surface's FRAME is kFootFrame doubles: an origin o and two unit vectors e1, e2.  float64 only, every operation one
// rounded IEEE operation in this order (no FMA):
//   the ray ARRIVES when A.x, A.y and A.z are finite, and PASSES when it arrives and B.x, B.y and B.z are finite
//   q = A.xyz - o;  u = (q.x e1.x + q.y e1.y) + q.z e1.z;  v likewise with e2;  rho2 = u u + v v
// The kFootCols statistics of a (group, surface): 0 the rays that arrive, 1 the rays that pass, 2 max rho2 over the
// arriving rays, 3 max rho2 over the passing rays, 4 / 5 min / max u and 6 / 7 min / max v over the passing rays.
// Counts, maxima and minima only: no statistic depends on the order of the rays.  An empty set gives -inf for a
// maximum and +inf for a minimum; a NaN u, v or rho2 (overflow only: A is finite) is skipped by the comparisons, the
// ray still counts.
// foot_ray gives one ray's term with the neutral element wherever it has nothing to say (foot_none: 0, 0, -inf, -inf,
// +inf, -inf, +inf, -inf), so no NaN reaches foot_merge, which combines two terms column by column.
#pragma once

#include "rtpb_math.h"

namespace rtpb {

constexpr int kFootCols = 8;
constexpr int kFootFrame = 9;              // o, e1, e2
struct FootRay {
    double v[kFootCols];
};

RTPB_HD FootRay foot_none() {
    const double inf = __builtin_inf();
    return FootRay{{0.0, 0.0, -inf, -inf, inf, -inf, inf, -inf}};
}

RTPB_HD bool foot_finite3(double x, double y, double z) { return x - x == 0.0 && y - y == 0.0 && z - z == 0.0; }

RTPB_HD FootRay foot_ray(double ax, double ay, double az, double bx, double by, double bz,
                         const double (&f)[kFootFrame]) {
    FootRay o = foot_none();
    if (!foot_finite3(ax, ay, az)) return o;
    const double qx = ax - f[0], qy = ay - f[1], qz = az - f[2];
    const double u = (qx * f[3] + qy * f[4]) + qz * f[5];
    const double v = (qx * f[6] + qy * f[7]) + qz * f[8];
    const double rho2 = u * u + v * v;
    o.v[0] = 1.0;
    if (rho2 == rho2) o.v[2] = rho2;
    if (foot_finite3(bx, by, bz)) {
        o.v[1] = 1.0;
        if (rho2 == rho2) o.v[3] = rho2;
        if (u == u) o.v[4] = o.v[5] = u;
        if (v == v) o.v[6] = o.v[7] = v;
    }
    return o;
}

// Column c of two terms combined: a sum of integer-valued doubles, a maximum or a minimum (no NaN: see foot_ray)
RTPB_HD double foot_col(int c, double a, double b) {
    if (c < 2) return a + b;
    if (c == 4 || c == 6) return __builtin_fmin(a, b);
    return __builtin_fmax(a, b);
}

RTPB_HD void foot_merge(FootRay& a, const FootRay& b) {
    a.v[0] = a.v[0] + b.v[0];
    a.v[1] = a.v[1] + b.v[1];
    a.v[2] = __builtin_fmax(a.v[2], b.v[2]);
    a.v[3] = __builtin_fmax(a.v[3], b.v[3]);
    a.v[4] = __builtin_fmin(a.v[4], b.v[4]);
    a.v[5] = __builtin_fmax(a.v[5], b.v[5]);
    a.v[6] = __builtin_fmin(a.v[6], b.v[6]);
    a.v[7] = __builtin_fmax(a.v[7], b.v[7]);
}

}  // namespace rtpb
