// rtpb_trans.h -- the transmission statistics' per-ray rule (rtpb_transmission_stats / rtpb_transmission_sweep /
// rtpb_ray_transmission), free of HIP so that a plain C++ build can run it (tests/native/trans_harness.cpp); the
// kernels get it through rtpb_stats.h.
//
// For one surface s and one ray: A is the ray's row in history plane 2s + 1 (the position at the surface and the
// INCOMING direction), B its row in plane 2s + 2 (the OUTGOING direction), n1 and n2 the indices before and after the
// surface at the group's wavelength.  The surface's COATING is kTransCoat doubles {mode, value}.  float64 only, every
// operation one rounded IEEE operation in this order (no FMA):
//   the ray PASSES exactly when the footprint statistics say so: A.xyz finite and B.xyz finite
//   mode 0 (CONSTANT): t = value (0 <= value <= 1, checked by the host)
//   mode 1 (FRESNEL, uncoated, unpolarised; value ignored): t = 1 where n1 == n2, else with dA = A.dxyz, dB = B.dxyz
//       g  = n1 dA - n2 dB                      (componentwise; by Snell's law g lies along the normal)
//       p1 = |(dA.x g.x + dA.y g.y) + dA.z g.z|,  p2 likewise with dB
//       rs = (n1 p1 - n2 p2) / (n1 p1 + n2 p2),  rp = (n2 p1 - n1 p2) / (n2 p1 + n1 p2)
//       t  = 1 - 0.5 (rs rs + rp rp);  a t that is NaN or outside [0, 1] becomes 0
//   cum_s = cum_(s-1) * t_s in surface order, cum_(-1) = 1: defined for a ray that passes s (it has passed every
//   earlier surface); a ray that does not pass leaves the rule with t = cum = NaN
//   qt = rint(t 2^q_bits), qc = rint(cum 2^q_bits)
// No normal, no surface kind, no square root, no normalisation: |g| cancels in both ratios, so the rule holds for
// every surface that refracts by Snell's law.  Exchanging (n1, dA) with (n2, dB) negates g, exchanges p1 and p2 and
// negates both ratios exactly: t is the same bits in either direction.
// The kTransCols statistics of a (group, surface): 0 the rays that pass, 1 the sum of qt and 2 the sum of qc over
// them, 3 / 4 the minimum / maximum of qc over them (+inf / -inf for none).  All integer-valued: with group_size *
// 2^q_bits <= 2^53 every sum is exact in any order.
#pragma once

#include "rtpb_foot.h"

namespace rtpb {

constexpr int kTransCols = 5;
constexpr int kTransCoat = 2;              // mode, value
constexpr int kTransMaxQBits = 40;
constexpr double kCoatConstant = 0.0, kCoatFresnel = 1.0;
struct TransRay {
    double v[kTransCols];
};

RTPB_HD TransRay trans_none() {
    const double inf = __builtin_inf();
    return TransRay{{0.0, 0.0, 0.0, inf, -inf}};
}

// The amplitude reflection ratios of one refraction (n1 != n2) from its two directions and two indices
RTPB_HD void trans_ratios(double n1, double n2, double ax, double ay, double az, double bx, double by, double bz,
                          double& rs, double& rp) {
    const double gx = n1 * ax - n2 * bx, gy = n1 * ay - n2 * by, gz = n1 * az - n2 * bz;
    const double p1 = __builtin_fabs((ax * gx + ay * gy) + az * gz);
    const double p2 = __builtin_fabs((bx * gx + by * gy) + bz * gz);
    rs = (n1 * p1 - n2 * p2) / (n1 * p1 + n2 * p2);
    rp = (n2 * p1 - n1 * p2) / (n2 * p1 + n1 * p2);
}

// The unpolarised Fresnel transmittance of that refraction
RTPB_HD double trans_fresnel(double n1, double n2, double ax, double ay, double az, double bx, double by, double bz) {
    if (n1 == n2) return 1.0;
    double rs, rp;
    trans_ratios(n1, n2, ax, ay, az, bx, by, bz, rs, rp);
    const double t = 1.0 - 0.5 * (rs * rs + rp * rp);
    return t >= 0.0 && t <= 1.0 ? t : 0.0;
}

// One surface for one ray: A = (a, da), B = (b, db).  Returns whether the ray passes; t is the surface's
// transmittance for it and cum, the product over the earlier surfaces coming in, the product including this one --
// both NaN for a ray that does not pass.
RTPB_HD bool trans_ray(double ax, double ay, double az, double dax, double day, double daz, double bx, double by,
                       double bz, double dbx, double dby, double dbz, double n1, double n2, double coat_mode,
                       double coat_value, double& t, double& cum) {
    if (!(foot_finite3(ax, ay, az) && foot_finite3(bx, by, bz))) {
        t = cum = __builtin_nan("");
        return false;
    }
    t = coat_mode == kCoatConstant ? coat_value : trans_fresnel(n1, n2, dax, day, daz, dbx, dby, dbz);
    cum = cum * t;
    return true;
}

// A passing ray's term: scale = 2^q_bits
RTPB_HD TransRay trans_term(double t, double cum, double scale) {
    const double qt = __builtin_rint(t * scale), qc = __builtin_rint(cum * scale);
    return TransRay{{1.0, qt, qc, qc, qc}};
}

// Column c of two terms combined: a sum of integer-valued doubles, a minimum or a maximum (no NaN reaches it)
RTPB_HD double trans_col(int c, double a, double b) {
    if (c < 3) return a + b;
    return c == 3 ? __builtin_fmin(a, b) : __builtin_fmax(a, b);
}

RTPB_HD void trans_merge(TransRay& a, const TransRay& b) {
    a.v[0] = a.v[0] + b.v[0];
    a.v[1] = a.v[1] + b.v[1];
    a.v[2] = a.v[2] + b.v[2];
    a.v[3] = __builtin_fmin(a.v[3], b.v[3]);
    a.v[4] = __builtin_fmax(a.v[4], b.v[4]);
}

// The largest q_bits a group of group_size rays admits (every sum stays an exact integer: group_size * 2^q_bits <=
// 2^53), at most kTransMaxQBits; 0 where not even q_bits = 1 fits
RTPB_HD int trans_max_q_bits(long long group_size) {
    int q = kTransMaxQBits;
    while (q > 0 && group_size > (1ll << (53 - q))) --q;
    return q;
}

}  // namespace rtpb
