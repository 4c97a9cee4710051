// rtpb_wavemap.h -- the wavefront map's per-ray rule (rtpb_wavefront_map / rtpb_wavefront_map_sweep), free of HIP so
// that a plain C++ build can run it (tests/native/wavemap_harness.cpp); the kernels get it through rtpb_stats.h.  The
// two definitions it is built on live here with it for that reason: wave_ray, a ray's optical path difference against
// its group's reference (the wavefront statistics' rule), and image_bin, a point's cell in a window (the spot
// image's).
//
// The MAP of a group is the optical path difference over the exit pupil: the pupil coordinate of a ray is its
// direction offset (ex, ey) from the chief ray, and each of the nx x ny cells of the group's window holds how many rays
// fell into it (count, int32) and the sum of their OPDs as integers (sum, int64): the OPD in units of 2^-q_bits waves,
// rounded to nearest-even.  Integers, so the map does not depend on the order in which rays arrive.  Per ray, with the
// group's reference ref (kWaveRef doubles), its window win {ex_lo, ey_lo, x_scale, y_scale}, scale = 2^q_bits and
// w_lim, every step one rounded IEEE operation (no FMA):
//   f = wave_ray(...); a ray with f.n == 0 contributes nothing anywhere
//   far_e = max(|ex|, |ey|), far_w = |w|: both enter the group's two maxima, whatever the window and the limit say
//   b = image_bin(ex, ey, win, nx, ny); a ray that is not inside is OUTSIDE and goes no further
//   a ray that is inside and fails |w| <= w_lim is CLIPPED (a failed comparison: a NaN limit passes no ray)
//   otherwise tq = w * scale (exact: a power of two) and q = (int64) rint(tq); count[b] += 1, sum[b] += q
// Every counting ray is in exactly one of count, outside or clipped, and a cell's sum / 2^q_bits / count is within
// 2^-(q_bits + 1) waves of the true mean OPD of its rays.
#pragma once

#include "rtpb_math.h"

namespace rtpb {

// Wavefront statistics (rtpb_wavefront_stats / rtpb_wavefront_sweep): the moments of the optical path difference.
// A group's reference is kWaveRef doubles (C0x, C0y, C0z, d0x, d0y, d0z, p0, kf): the reference point, the pivot
// direction and the pivot phase (radians) of the group's chief ray, and kf = n_final / wavelength.  The optical path
// of a ray to the foot of the perpendicular from C0 is linear in C0, so the variance of the OPD about a displaced
// reference C0 + delta is an exact quadratic in delta whose coefficients are the first and second moments of
// (w, e) below (analysis.summarize_wavefront).  The pivots are subtracted per ray before anything is squared: the
// phase is 1e4 ... 1e7 rad and the OPD a fraction of a wave, and un-pivoted sums cancel to a few per cent.
// The one definition of a ray's contribution, for the plane kernel and the fused sweep alike, float64 only, every
// operation one rounded IEEE operation in this order (no FMA):
//   ex = dx - d0x, ey = dy - d0y, ez = dz - d0z
//   s  = ((C0x - x) * dx + (C0y - y) * dy) + (C0z - z) * dz
//   w  = (ph - p0) * kInv2Pi + s * kf                              (the OPD in waves)
// A ray counts when x and y are finite (the spot statistics' rule) and w, ex, ey and ez are all finite.  wave_ray
// gives the counted ray as (n, w, ex, ey, ez) with n = 1, or all +0 for a ray that does not count.
constexpr int kWaveRef = 8;
constexpr double kInv2Pi = 0.15915494309189535;
struct WaveRay {
    double n, w, ex, ey, ez;
};
RTPB_HD WaveRay wave_ray(double x, double y, double z, double dx, double dy, double dz, double ph,
                         const double (&ref)[kWaveRef]) {
    const double ex = dx - ref[3], ey = dy - ref[4], ez = dz - ref[5];
    const double s = ((ref[0] - x) * dx + (ref[1] - y) * dy) + (ref[2] - z) * dz;
    const double w = (ph - ref[6]) * kInv2Pi + s * ref[7];
    if (x - x == 0.0 && y - y == 0.0 && w - w == 0.0 && ex - ex == 0.0 && ey - ey == 0.0 && ez - ez == 0.0)
        return WaveRay{1.0, w, ex, ey, ez};
    return WaveRay{0.0, 0.0, 0.0, 0.0, 0.0};
}

// Spot images (rtpb_spot_image / rtpb_image_sweep): a 2-D histogram of the final positions per group, int32 counts,
// so the result is exact and independent of the order of arrival.  The one definition of a ray's contribution, for
// the plane kernel and the fused sweep alike: x and y are the ray's final position rounded to the storage type, w the
// group's window {x_lo, y_lo, x_scale, y_scale}.  A ray counts when the spot statistics count it (x and y finite; the
// sweep adds its own dead-row rule before calling).  tx = (x - x_lo) * x_scale and ty likewise, each one rounded
// subtract and one rounded multiply; the ray is inside iff 0 <= tx < nx and 0 <= ty < ny, compared in floating point
// (a NaN or infinite window, or an overflowing tx, is outside), and only then are tx and ty converted to integers:
// no index exists for a ray that failed the test.  Returns the bin iy * nx + ix, kImageOutside for a counting ray
// that is not inside, kImageSkip for a ray that does not count.  nx, ny <= RTPB_MAX_IMAGE_SIDE, so a bin fits an int.
constexpr int kImageSkip = -1, kImageOutside = -2;
RTPB_HD int image_bin(double x, double y, const double (&w)[4], int nx, int ny) {
    if (!(x - x == 0.0 && y - y == 0.0)) return kImageSkip;
    const double tx = (x - w[0]) * w[2], ty = (y - w[1]) * w[3];
    if (tx >= 0.0 && tx < double(nx) && ty >= 0.0 && ty < double(ny))
        return static_cast<int>(ty) * nx + static_cast<int>(tx);
    return kImageOutside;
}

// One ray's term of its group's map: bin is the cell iy * nx + ix, kImageOutside, kMapClipped, or kImageSkip for a
// ray that does not count; q is the OPD in units of 1 / scale waves (0 unless bin >= 0); far_e and far_w are finite
// and non-negative, +0 for a ray that does not count, so they order as their bit patterns.
constexpr int kMapClipped = -3;
constexpr int kMapWin = 4;                 // a group's window: ex_lo, ey_lo, x_scale, y_scale
struct MapRay {
    int bin;
    long long q;
    double far_e, far_w;
};
RTPB_HD MapRay wavemap_ray(const WaveRay& f, const double (&win)[kMapWin], int nx, int ny, double scale,
                           double w_lim) {
    if (f.n == 0.0) return MapRay{kImageSkip, 0, 0.0, 0.0};
    const double ax = __builtin_fabs(f.ex), ay = __builtin_fabs(f.ey), aw = __builtin_fabs(f.w);
    MapRay m{image_bin(f.ex, f.ey, win, nx, ny), 0, ax > ay ? ax : ay, aw};
    if (m.bin < 0) return m;
    if (!(aw <= w_lim)) {
        m.bin = kMapClipped;
        return m;
    }
    const double tq = f.w * scale;
    m.q = static_cast<long long>(__builtin_rint(tq));
    return m;
}

// What the entry points refuse before a device is touched: 0 (fine), 1 (invalid: q_bits outside 0 ... 52, or a w_lim
// that is not finite and >= 0) or 2 (limit: a cell's sum could leave int64).  With ldexp(w_lim, q_bits) + 1 <=
// 2^62 / group_size every |q| <= w_lim 2^q_bits + 1/2, so group_size of them stay inside int64 by a factor of two,
// which covers the rounding of this check itself.
inline int wavemap_bound(int q_bits, double w_lim, int64_t group_size) {
    if (q_bits < 0 || q_bits > 52 || !(w_lim >= 0.0) || !(w_lim - w_lim == 0.0)) return 1;
    if (!(std::ldexp(w_lim, q_bits) + 1.0 <= std::ldexp(1.0, 62) / double(group_size))) return 2;
    return 0;
}

}  // namespace rtpb
