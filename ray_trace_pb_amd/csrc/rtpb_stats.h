// rtpb_stats.h -- what the plane kernels (rtpb_analysis.hip, rtpb_image.hip, rtpb_energy.hip, rtpb_psf.hip,
// rtpb_wavemap.hip) and the fused sweep (rtpb_sweep.hip) share: the statistics sets, the one definition of a ray's
// contribution to the focus statistics, to the wavefront statistics, to the Huygens PSF, to a spot image and to the
// energy curves, the footprint statistics' term (rtpb_foot.h, plain C++ so that the host can run it) and its wave and
// block reductions, the transmission and polarisation rules (rtpb_trans.h, rtpb_pol.h) with their wave reductions, the
// wavefront map's rule (rtpb_wavemap.h, plain C++ likewise) and its wave-level adds, the wave's aggregated image adds, the reduction's argument block and its block-wide tree.  Everything here has
// internal linkage, as it had inside the one unit: each unit's kernels take its own SpotArgs.
#pragma once

#include "rtpb_internal.h"

#include "rtpb_foot.h"
#include "rtpb_pol.h"
#include "rtpb_trans.h"
#include "rtpb_wavemap.h"

namespace {

// Spot statistics of one history plane, per contiguous group of `gsize` rays (per
// (field, wavelength) spot diagrams).  Rays whose x or y is not finite are skipped.  Deterministic:
// pass 1 reduces each 256-ray tile of a group in a fixed tree order into partials[group][tile];
// pass 2 sums a group's partials in a fixed order.  Stats: n, Sx, Sy, Sz, Sxx, Syy, Sxy.
constexpr int kStats = 7;

// Focus statistics (through-focus analysis): the seven spot sums, then the sums of u, v, u u, v v, u v, x u, y v,
// x v, y u with the slopes u = dx / dz and v = dy / dz (IEEE division).  On a plane displaced by delta along z the ray
// is at (x + u delta, y + v delta), so the RMS spot radius is an exact quadratic in delta whose coefficients are these
// second moments: best focus, the line foci and the through-focus curve follow on the host (analysis.summarize_focus).
// The one definition of a ray's contribution, for the plane kernel and the fused sweep alike: the arguments are the
// ray's final state rounded to the storage type; a ray counts when x, y, u and v are all finite (dz = 0 and NaN or
// infinite directions drop it); each product is one rounded multiply.
// focus_ray gives the counted ray as (n, x, y, z, u, v) with n = 1, or all +0 for a ray that does not count, and
// focus_term its k-th statistic: a dropped ray's products are +0 * +0 = +0, so the kernels carry six values per ray
// to the reduction and form the products chunk by chunk instead of holding sixteen.
constexpr int kFocusStats = 16;
struct FocusRay {
    double n, x, y, z, u, v;
};
RTPB_HD FocusRay focus_ray(double x, double y, double z, double dx, double dy, double dz) {
    const double u = dx / dz, v = dy / dz;
    if (x - x == 0.0 && y - y == 0.0 && u - u == 0.0 && v - v == 0.0) return FocusRay{1.0, x, y, z, u, v};
    return FocusRay{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
}
RTPB_HD double focus_term(const FocusRay& f, int k) {
    switch (k) {
    case 0: return f.n;
    case 1: return f.x;
    case 2: return f.y;
    case 3: return f.z;
    case 4: return f.x * f.x;
    case 5: return f.y * f.y;
    case 6: return f.x * f.y;
    case 7: return f.u;
    case 8: return f.v;
    case 9: return f.u * f.u;
    case 10: return f.v * f.v;
    case 11: return f.u * f.v;
    case 12: return f.x * f.u;
    case 13: return f.y * f.v;
    case 14: return f.x * f.v;
    default: return f.y * f.u;
    }
}

// Wavefront statistics (rtpb_wavefront_stats / rtpb_wavefront_sweep): the moments of the optical path difference
// against the group's reference.  The one definition of a ray's contribution is wave_ray (rtpb_wavemap.h, plain C++
// so that the host can run it): the counted ray as (n, w, ex, ey, ez) with n = 1, or all +0 for a ray that does not
// count.  wave_term is its k-th statistic, each product one rounded multiply: n, w, w w, ex, ey, ez, w ex, w ey, w ez,
// ex ex, ey ey, ez ez, ex ey, ex ez, ey ez (k past the set: +0, the padding of the last chunk of eight).
constexpr int kWaveStats = 15;
using rtpb::kWaveRef;
using rtpb::kInv2Pi;
using rtpb::WaveRay;
using rtpb::wave_ray;
RTPB_HD double wave_term(const WaveRay& f, int k) {
    switch (k) {
    case 0: return f.n;
    case 1: return f.w;
    case 2: return f.w * f.w;
    case 3: return f.ex;
    case 4: return f.ey;
    case 5: return f.ez;
    case 6: return f.w * f.ex;
    case 7: return f.w * f.ey;
    case 8: return f.w * f.ez;
    case 9: return f.ex * f.ex;
    case 10: return f.ey * f.ey;
    case 11: return f.ez * f.ez;
    case 12: return f.ex * f.ey;
    case 13: return f.ex * f.ez;
    case 14: return f.ey * f.ez;
    default: return 0.0;
    }
}

// Huygens PSF (rtpb_huygens_psf): the field at the image-plane point C0 + (X, Y, 0) is the coherent sum of the rays'
// plane wavelets, E = sum a exp(2 pi i (w + kf (ex X + ey Y))), with w and e wave_ray's OPD and direction offset
// against the group's reference: nothing new is asked of a ray, and the counting rule is wave_ray's.  The one
// definition of a ray's contribution, every operation one rounded IEEE operation in this order (no FMA):
//   a = n * weight, qx = ex * kf, qy = ey * kf                     per ray (psf_ray; n is wave_ray's 1 or 0)
//   t = (w + qx * X) + qy * Y,  fr = t - rint(t)                   per (ray, pixel) (psf_frac)
// and the pixel adds a cospi(2 fr) and a sinpi(2 fr).  fr is exact (t and rint(t) are within a factor two of each
// other, or t is below 1/2), |fr| <= 1/2, and removing whole waves before the sine keeps its argument small whatever
// the OPD.  A ray that does not count adds nothing and is skipped, not multiplied by zero: its a is 0 * weight, NaN
// for a NaN weight, and its t NaN in a NaN window.  A counting ray has a finite w, so psf_ray marks the others with a
// NaN w (psf_counts) and the tile needs no fifth value.
struct PsfRay {
    double a, w, qx, qy;
};
RTPB_HD PsfRay psf_ray(double x, double y, double z, double dx, double dy, double dz, double ph,
                       const double (&ref)[kWaveRef], double weight) {
    const WaveRay f = wave_ray(x, y, z, dx, dy, dz, ph, ref);
    if (f.n == 0.0) return PsfRay{0.0, __builtin_nan(""), 0.0, 0.0};
    return PsfRay{f.n * weight, f.w, f.ex * ref[7], f.ey * ref[7]};
}
RTPB_HD bool psf_counts(const PsfRay& f) { return f.w == f.w; }
RTPB_HD double psf_frac(const PsfRay& f, double X, double Y) {
    const double t = (f.w + f.qx * X) + f.qy * Y;
    return t - __builtin_rint(t);
}

// Spot images (rtpb_spot_image / rtpb_image_sweep): a 2-D histogram of the final positions per group, int32 counts,
// so the result is exact and independent of the order of arrival.  The one definition of a ray's contribution is
// image_bin (rtpb_wavemap.h, beside the map rule that bins the pupil with it): the bin iy * nx + ix, kImageOutside for
// a counting ray that is not inside, kImageSkip for a ray that does not count.
using rtpb::kImageSkip;
using rtpb::kImageOutside;
using rtpb::image_bin;

// One wave's contributions to one group's image (image: the group's ny * nx counters, outside: its one; both
// wave-uniform), bin from image_bin.  Every lane of the wave must call it.  Per-ray atomics would serialise on the
// few hot bins of a tight spot, so the wave aggregates first: while a lane is pending, the first pending lane's bin is
// broadcast, the lanes that share it are counted with one ballot, that lane issues one no-return atomic add of the
// count and the matched lanes retire; the outside rays take one add per wave.  Integer adds: any order, same image.
__device__ __forceinline__ void wave_image_add(int bin, int32_t* __restrict__ image, int32_t* __restrict__ outside) {
    const int lane = static_cast<int>(__lane_id());
    const unsigned long long out = __ballot(bin == kImageOutside);
    if (out != 0 && lane == __ffsll(out) - 1) atomicAdd(outside, __popcll(out));
    unsigned long long pending = __ballot(bin >= 0);
    while (pending != 0) {
        const int leader = __ffsll(pending) - 1;
        const int b = __builtin_amdgcn_readlane(bin, leader);
        // (a retired lane's bin differs from b: every lane that shares a bin retires with it)
        const unsigned long long same = __ballot(bin == b);
        if (lane == leader) atomicAdd(image + b, __popcll(same));
        pending &= ~same;
    }
}

// Encircled / ensquared energy (rtpb_spot_energy / rtpb_energy_sweep): two radial histograms of the final positions
// per group, int32 counts, and the farthest ray of each.  The one definition of a ray's contribution, for the plane
// kernel and the fused sweep alike: x and y are the ray's final position rounded to the storage type, p the group's
// parameters {cx, cy, scale, 0} with scale = nr / r_max.  A ray counts when the spot statistics count it (x and y
// finite).  dx = x - cx, dy = y - cy, rho = sqrt(dx dx + dy dy) (the correctly rounded root, tsqrt), m = max(|dx|,
// |dy|), tc = rho * scale, ts = m * scale, each one rounded operation; the ray is inside the circle curve iff
// 0 <= tc < nr and inside the square curve iff 0 <= ts < nr, compared in floating point (a NaN or infinite scale, or
// an overflowing product, is outside), and only then is the value converted to an integer.  bin[k] is the bin,
// kImageOutside for a counting ray that is not inside, kImageSkip for a ray that does not count (k = 0 the circle,
// 1 the square); far[k] is rho and m, +0 for a ray that does not count.  A centre that is not finite (NaN or
// infinite cx or cy) puts every counting ray outside both curves with far = +0: it leaves the group's farthest
// untouched.  With a finite centre rho and m are never NaN and never negative (+inf where a product overflows), so
// they order as their bit patterns.
struct EnergyRay {
    int bin[2];
    double far[2];
};
RTPB_HD EnergyRay energy_bins(double x, double y, const double (&p)[4], int nr) {
    if (!(x - x == 0.0 && y - y == 0.0)) return EnergyRay{{kImageSkip, kImageSkip}, {0.0, 0.0}};
    if (!(p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0)) return EnergyRay{{kImageOutside, kImageOutside}, {0.0, 0.0}};
    const double dx = x - p[0], dy = y - p[1];
    const double rho = rtpb::tsqrt<double>(dx * dx + dy * dy);
    const double ax = __builtin_fabs(dx), ay = __builtin_fabs(dy);      // (a -0.0 offset is +0 from here on)
    const double m = ax > ay ? ax : ay;
    const double tc = rho * p[2], ts = m * p[2];
    EnergyRay e{{kImageOutside, kImageOutside}, {rho, m}};
    if (tc >= 0.0 && tc < double(nr)) e.bin[0] = static_cast<int>(tc);
    if (ts >= 0.0 && ts < double(nr)) e.bin[1] = static_cast<int>(ts);
    return e;
}

// One wave's largest v into *out, v >= +0 and not NaN (so the doubles order as their bit patterns, and +0 is all zero
// bits: the cleared output).  Every lane of the wave must call it; a lane with nothing to add passes +0.  The wave is
// reduced first and one lane issues one unsigned 64-bit atomic max -- and only when the wave's maximum is above what
// *out holds already: the value only ever grows, so a stale read can cost a redundant atomic and never a lost one, and
// all but a group's first few waves leave the one address alone (+0, the cleared value, is never above it).
__device__ __forceinline__ void wave_max_bits(double v, double* __restrict__ out) {
    unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        const unsigned long long o = __shfl_xor(b, w, 64);
        b = o > b ? o : b;
    }
    unsigned long long* const p = reinterpret_cast<unsigned long long*>(out);
    if (__lane_id() == 0 && b > __builtin_nontemporal_load(p)) atomicMax(p, b);
}

// One wave's contributions to one group's energy curves (hist: the group's 2 * nr counters, outside and farthest: its
// two of each; all wave-uniform), e from energy_bins.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_energy_add(const EnergyRay& e, int nr, int32_t* __restrict__ hist,
                                                int32_t* __restrict__ outside, double* __restrict__ farthest) {
    wave_image_add(e.bin[0], hist, outside);
    wave_image_add(e.bin[1], hist + nr, outside + 1);
    wave_max_bits(e.far[0], farthest);
    wave_max_bits(e.far[1], farthest + 1);
}

// Wavefront map (rtpb_wavefront_map / rtpb_wavefront_map_sweep; the rule: rtpb_wavemap.h wavemap_ray).  One wave's
// contributions to one group's map (count and sum: the group's ny * nx cells; outside and clipped: its one of each;
// farthest: its two maxima; all wave-uniform).  Every lane of the wave must call it.  wave_image_add extended by the
// 64-bit sum: per distinct cell in the wave the leader issues one no-return add of the lane count and one 64-bit
// integer add of the sum of q over the lanes that share the cell -- a masked butterfly over the wave, which every lane
// runs (the loop is wave-uniform); a cell held by a single lane needs no reduction.  (Two adds per lane instead
// take 1.7 to 3.5 times as long on the C5 workload: DESIGN.md, profiles/r16/per_lane_adds.patch.)  Integer adds and
// maxima: any order, the same map.
using rtpb::MapRay;
using rtpb::kMapClipped;
using rtpb::kMapWin;
using rtpb::wavemap_ray;
__device__ __forceinline__ void wave_map_add(const MapRay& m, int32_t* __restrict__ count,
                                             long long* __restrict__ sum, int32_t* __restrict__ outside,
                                             int32_t* __restrict__ clipped, double* __restrict__ farthest) {
    const int lane = static_cast<int>(__lane_id());
    const unsigned long long out = __ballot(m.bin == kImageOutside);
    if (out != 0 && lane == __ffsll(out) - 1) atomicAdd(outside, __popcll(out));
    const unsigned long long clip = __ballot(m.bin == kMapClipped);
    if (clip != 0 && lane == __ffsll(clip) - 1) atomicAdd(clipped, __popcll(clip));
    unsigned long long* const usum = reinterpret_cast<unsigned long long*>(sum);
    unsigned long long pending = __ballot(m.bin >= 0);
    while (pending != 0) {
        const int leader = __ffsll(pending) - 1;
        const int b = __builtin_amdgcn_readlane(m.bin, leader);
        // (a retired lane's bin differs from b: every lane that shares a bin retires with it)
        const unsigned long long same = __ballot(m.bin == b);
        const int n = __popcll(same);
        // two's complement: the unsigned sum of the lanes' q is the signed one
        unsigned long long s = static_cast<unsigned long long>(m.q);
        if (n > 1) {
            s = m.bin == b ? s : 0ull;
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
        }
        if (lane == leader) {
            atomicAdd(count + b, n);
            atomicAdd(usum + b, s);
        }
        pending &= ~same;
    }
    wave_max_bits(m.far_e, farthest);
    wave_max_bits(m.far_w, farthest + 1);
}

struct SpotArgs {
    const void* __restrict__ plane;
    double* __restrict__ partials;
    double* __restrict__ stats;
    int64_t gsize, ngroups, tiles;
};

// Sums of R values over a block's 256 lanes in one fixed tree order -- red[t] += red[t + w] for t < w, w = 128, 64,
// ..., 1 -- valid in thread 0.  The two levels that cross waves go through LDS (buf rows, slots 64..255; two
// barriers), the six inside wave 0 through lane shuffles: the same additions of the same operands, without the
// barrier, store and load of every level of an all-LDS tree.
template <int R>
__device__ __forceinline__ void block_tree_sum(double (&v)[R], double (*buf)[rtpbi::kBlock]) {
    static_assert(rtpbi::kBlock == 256, "four waves");
    const int t = threadIdx.x;
    if (t >= 128) {
#pragma unroll
        for (int j = 0; j < R; ++j) buf[j][t] = v[j];
    }
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = v[j] + buf[j][t + 128];
        if (t >= 64) {
#pragma unroll
            for (int j = 0; j < R; ++j) buf[j][t] = v[j];
        }
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int j = 0; j < R; ++j) v[j] = v[j] + buf[j][t + 64];
        // lanes >= w add values no later level reads
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
#pragma unroll
            for (int j = 0; j < R; ++j) v[j] = v[j] + __shfl_down(v[j], w, 64);
        }
    }
}

// Footprint statistics (rtpb_foot.h: foot_ray, foot_merge).  One term per lane combined over the wave, the result in
// every lane: the four steps inside a row of 16 lanes are DPP moves (lane ^ 1 and lane ^ 2 by quad permutation, then the
// row rotated by 4 and by 8: every quad then holds all four quads), the two across rows lane shuffles.  Sums of small
// integers, maxima and minima: any order gives the same bits.
template <int CTRL>
__device__ __forceinline__ double foot_dpp(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp(static_cast<int>(b), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_mov_dpp(static_cast<int>(b >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned int>(lo));
}
template <int CTRL>
__device__ __forceinline__ void foot_dpp_step(rtpb::FootRay& f) {
    rtpb::FootRay o;
#pragma unroll
    for (int c = 0; c < rtpb::kFootCols; ++c) o.v[c] = foot_dpp<CTRL>(f.v[c]);
    rtpb::foot_merge(f, o);
}
__device__ __forceinline__ void foot_wave_reduce(rtpb::FootRay& f) {
    foot_dpp_step<0xB1>(f);         // quad_perm [1, 0, 3, 2]
    foot_dpp_step<0x4E>(f);         // quad_perm [2, 3, 0, 1]
    foot_dpp_step<0x124>(f);        // row_ror 4
    foot_dpp_step<0x128>(f);        // row_ror 8
#pragma unroll
    for (int w = 16; w <= 32; w <<= 1) {
        rtpb::FootRay o;
#pragma unroll
        for (int c = 0; c < rtpb::kFootCols; ++c) o.v[c] = __shfl_xor(f.v[c], w, 64);
        rtpb::foot_merge(f, o);
    }
}

// ... and over a block's four waves through tab (LDS, [4][kFootCols]); the result is valid in threads 0 ... 7, thread
// c holding column c (returned).  One barrier; tab is free again after the next one.
__device__ __forceinline__ double foot_block_reduce(rtpb::FootRay& f, double (*tab)[rtpb::kFootCols]) {
    static_assert(rtpbi::kBlock == 256, "four waves");
    const int t = threadIdx.x;
    foot_wave_reduce(f);
    if ((t & 63) == 0) {
#pragma unroll
        for (int c = 0; c < rtpb::kFootCols; ++c) tab[t >> 6][c] = f.v[c];
    }
    __syncthreads();
    double v = 0.0;
    if (t < rtpb::kFootCols) {
        v = tab[0][t];
#pragma unroll
        for (int w = 1; w < 4; ++w) v = rtpb::foot_col(t, v, tab[w][t]);
    }
    return v;
}

// Transmission statistics (rtpb_trans.h: trans_ray, trans_merge): the footprints' wave reduction with another merge.
// Sums of integers that stay exact, a minimum and a maximum: any order gives the same bits.
template <int CTRL>
__device__ __forceinline__ void trans_dpp_step(rtpb::TransRay& f) {
    rtpb::TransRay o;
#pragma unroll
    for (int c = 0; c < rtpb::kTransCols; ++c) o.v[c] = foot_dpp<CTRL>(f.v[c]);
    rtpb::trans_merge(f, o);
}
__device__ __forceinline__ void trans_wave_reduce(rtpb::TransRay& f) {
    trans_dpp_step<0xB1>(f);        // quad_perm [1, 0, 3, 2]
    trans_dpp_step<0x4E>(f);        // quad_perm [2, 3, 0, 1]
    trans_dpp_step<0x124>(f);       // row_ror 4
    trans_dpp_step<0x128>(f);       // row_ror 8
#pragma unroll
    for (int w = 16; w <= 32; w <<= 1) {
        rtpb::TransRay o;
#pragma unroll
        for (int c = 0; c < rtpb::kTransCols; ++c) o.v[c] = __shfl_xor(f.v[c], w, 64);
        rtpb::trans_merge(f, o);
    }
}

// Polarisation statistics (rtpb_pol.h: pol_surface, pol_term, pol_merge): the same wave reduction, every column a sum
// of integers that stays exact.
template <int CTRL>
__device__ __forceinline__ void pol_dpp_step(rtpb::PolRay& f) {
    rtpb::PolRay o;
#pragma unroll
    for (int c = 0; c < rtpb::kPolCols; ++c) o.v[c] = foot_dpp<CTRL>(f.v[c]);
    rtpb::pol_merge(f, o);
}
__device__ __forceinline__ void pol_wave_reduce(rtpb::PolRay& f) {
    pol_dpp_step<0xB1>(f);          // quad_perm [1, 0, 3, 2]
    pol_dpp_step<0x4E>(f);          // quad_perm [2, 3, 0, 1]
    pol_dpp_step<0x124>(f);         // row_ror 4
    pol_dpp_step<0x128>(f);         // row_ror 8
#pragma unroll
    for (int w = 16; w <= 32; w <<= 1) {
        rtpb::PolRay o;
#pragma unroll
        for (int c = 0; c < rtpb::kPolCols; ++c) o.v[c] = __shfl_xor(f.v[c], w, 64);
        rtpb::pol_merge(f, o);
    }
}

}  // namespace
