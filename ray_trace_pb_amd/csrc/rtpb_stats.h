// rtpb_stats.h -- what the plane statistics (rtpb_analysis.hip) and the fused sweep (rtpb_sweep.hip) share: the
// statistics sets, the one definition of a ray's contribution to the focus statistics, the reduction's argument
// block and its block-wide tree.  Everything here has internal linkage, as it had inside the one unit: each unit's
// kernels take its own SpotArgs.
#pragma once

#include "rtpb_internal.h"

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

}  // namespace
