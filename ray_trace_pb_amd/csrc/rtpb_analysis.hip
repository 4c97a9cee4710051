// rtpb_analysis.hip -- device analysis around the trace: intersect_rays
// (RT:164-238), the per-group spot, focus and wavefront statistics of a plane, and griddata-style interpolation of pupil phases onto a grid.
#include "rtpb_stats.h"

#include <algorithm>
#include <cstring>

using namespace rtpbi;

namespace {

// intersect_rays (RT:164-238): closest-approach solve from the first non-singular 2x2 sub-system,
// verified to 1e-12.  NaN determinants count as "non-zero" exactly like numpy's truthiness.
struct IsectArgs {
    const void* __restrict__ r1;
    const void* __restrict__ r2;
    void* __restrict__ out;
    int64_t n, n1, n2;
};

template <typename T>
__global__ __launch_bounds__(kBlock) void intersect_kernel(IsectArgs a) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const T* p = static_cast<const T*>(a.r1) + (a.n1 == 1 ? 0 : i) * 8;
    const T* q = static_cast<const T*>(a.r2) + (a.n2 == 1 ? 0 : i) * 8;
    const double x1 = p[0], y1 = p[1], z1 = p[2], dx1 = p[3], dy1 = p[4], dz1 = p[5];
    const double x2 = q[0], y2 = q[1], z2 = q[2], dx2 = q[3], dy2 = q[4], dz2 = q[5];
    const double nan = qnan<double>();
    const double det_xz = dx2 * dz1 - dz2 * dx1, det_xy = dx2 * dy1 - dy2 * dx1, det_yz = dz2 * dy1 - dy2 * dz1;
    double s = nan;
    if (det_xz != 0.0) s = ((z2 - z1) * dx1 - (x2 - x1) * dz1) / det_xz;
    else if (det_xy != 0.0) s = ((y2 - y1) * dx1 - (x2 - x1) * dy1) / det_xy;
    else if (det_yz != 0.0) s = ((y2 - y1) * dz1 - (z2 - z1) * dy1) / det_yz;
    double t;
    if (dz1 != 0.0) t = (z2 + s * dz2 - z1) / dz1;
    else if (dy1 != 0.0) t = (y2 + s * dy2 - y1) / dy1;
    else t = (x2 + s * dx2 - x1) / dx1;
    double o[3] = {x1 + t * dx1, y1 + t * dy1, z1 + t * dz1};
    const double e[3] = {o[0] - (x2 + s * dx2), o[1] - (y2 + s * dy2), o[2] - (z2 + s * dz2)};
    // numpy.max over the 3 |differences| propagates NaN, and NaN > 1e-12 is false
    double m = tabs(e[0]);
    for (int k = 1; k < 3; ++k) {
        const double v = tabs(e[k]);
        if (is_nan(m)) break;
        if (is_nan(v) || v > m) m = v;
    }
    if (m > 1e-12) o[0] = o[1] = o[2] = nan;
    T* out = static_cast<T*>(a.out) + i * 3;
    out[0] = T(o[0]); out[1] = T(o[1]); out[2] = T(o[2]);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void spot_partial_kernel(SpotArgs a) {
    __shared__ double red[kStats][kBlock];
    const int64_t g = blockIdx.y, tile = blockIdx.x;
    const int64_t j = tile * kBlock + threadIdx.x;
    double v[kStats] = {0, 0, 0, 0, 0, 0, 0};
    if (j < a.gsize) {
        const T* r = static_cast<const T*>(a.plane) + (g * a.gsize + j) * 8;
        const double x = r[0], y = r[1], z = r[2];
        if (x - x == 0.0 && y - y == 0.0) {
            v[0] = 1.0; v[1] = x; v[2] = y; v[3] = z; v[4] = x * x; v[5] = y * y; v[6] = x * y;
        }
    }
    block_tree_sum<kStats>(v, red);
    if (threadIdx.x == 0) {
        for (int k = 0; k < kStats; ++k) a.partials[(g * a.tiles + tile) * kStats + k] = v[k];
    }
}

// The focus statistics of an (N, 8) plane: spot_partial_kernel's tiles and tree, eight statistics at a time (16 KB
// of LDS instead of 32)
template <typename T>
__global__ __launch_bounds__(kBlock) void focus_partial_kernel(SpotArgs a) {
    constexpr int kRows = 8;
    __shared__ double red[kRows][kBlock];
    const int64_t g = blockIdx.y, tile = blockIdx.x;
    const int64_t j = tile * kBlock + threadIdx.x;
    FocusRay f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < a.gsize) {
        const T* r = static_cast<const T*>(a.plane) + (g * a.gsize + j) * 8;
        f = focus_ray(r[0], r[1], r[2], r[3], r[4], r[5]);
    }
#pragma unroll
    for (int k0 = 0; k0 < kFocusStats; k0 += kRows) {
        double u[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) u[k] = focus_term(f, k0 + k);
        // (no barrier between chunks: a tree's stores to slots 128..255 and 64..127 each follow a barrier that every
        // reader of the chunk before has passed, as in the sweep's reduce)
        block_tree_sum<kRows>(u, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < kRows; ++k) a.partials[(g * a.tiles + tile) * kFocusStats + k0 + k] = u[k];
        }
    }
}

// The wavefront statistics of an (N, 8) float64 plane (rtpb_wavefront_stats): focus_partial_kernel's structure with
// wave_ray / wave_term and the group's reference; the fifteen statistics go in two chunks of eight, the last padded
struct WaveArgs {
    SpotArgs s;
    const double* __restrict__ refs;    // per group: C0 (3), d0 (3), p0, kf
};

__global__ __launch_bounds__(kBlock) void wave_partial_kernel(WaveArgs wa) {
    constexpr int kRows = 8;
    __shared__ double red[kRows][kBlock];
    const SpotArgs& a = wa.s;
    const int64_t g = blockIdx.y, tile = blockIdx.x;
    const int64_t j = tile * kBlock + threadIdx.x;
    WaveRay f{0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < a.gsize) {
        const double* r = static_cast<const double*>(a.plane) + (g * a.gsize + j) * 8;
        const double* q = wa.refs + kWaveRef * g;
        const double ref[kWaveRef] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
        f = wave_ray(r[0], r[1], r[2], r[3], r[4], r[5], r[6], ref);
    }
#pragma unroll
    for (int k0 = 0; k0 < kWaveStats; k0 += kRows) {
        double u[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) u[k] = wave_term(f, k0 + k);
        // (no barrier between chunks, as in focus_partial_kernel)
        block_tree_sum<kRows>(u, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < kRows; ++k)
                if (k0 + k < kWaveStats) a.partials[(g * a.tiles + tile) * kWaveStats + k0 + k] = u[k];
        }
    }
}

// NS statistics per group (kStats, kFocusStats or kWaveStats): thread t adds tiles t, t + 256, ... in order, then one tree over
// the 256 threads
template <int NS>
__global__ __launch_bounds__(kBlock) void spot_final_kernel(SpotArgs a) {
    __shared__ double red[NS][kBlock];
    const int64_t g = blockIdx.x;
    double v[NS] = {};
    for (int64_t t = threadIdx.x; t < a.tiles; t += kBlock)
        for (int k = 0; k < NS; ++k) v[k] += a.partials[(g * a.tiles + t) * NS + k];
    for (int k = 0; k < NS; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int k = 0; k < NS; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < NS) a.stats[g * NS + threadIdx.x] = red[threadIdx.x][0];
}

// griddata(method='linear') on a regular grid + the pupil field of the PSF script (rtpb_grid_interpolate).
__global__ __launch_bounds__(kBlock) void grid_interp_kernel(rtpb_triangulation t, const double* __restrict__ xs,
                                                             int64_t nx, const double* __restrict__ ys, int64_t ny,
                                                             double radius, double* __restrict__ phase_out,
                                                             double* __restrict__ field_out) {
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= nx * ny) return;
    const int64_t iy = k / nx, ix = k % nx;
    const double x = xs[ix], y = ys[iy];
    constexpr double eps = 100.0 * 2.220446049250313e-16;      // scipy qhull: 100 * DBL_EPSILON
    double phase = __builtin_nan("");
    const double fx = (x - t.x0) / t.cell_w, fy = (y - t.y0) / t.cell_h;
    if (fx >= 0.0 && fy >= 0.0 && fx < double(t.cells_x) && fy < double(t.cells_y)) {
        const int64_t cell = int64_t(fy) * t.cells_x + int64_t(fx);
        for (int32_t q = t.cell_start[cell]; q < t.cell_start[cell + 1]; ++q) {
            const int32_t s = t.cell_tris[q];
            const double* T = t.transform + 6 * int64_t(s);
            // scipy/spatial/_qhull.pyx _barycentric_inside / _barycentric_coordinates (ndim = 2)
            double c0 = 0.0;
            c0 += T[0] * (x - T[4]);
            c0 += T[1] * (y - T[5]);
            double c1 = 0.0;
            c1 += T[2] * (x - T[4]);
            c1 += T[3] * (y - T[5]);
            const double c2 = (1.0 - c0) - c1;
            if (!(-eps <= c0 && c0 <= 1.0 + eps) || !(-eps <= c1 && c1 <= 1.0 + eps) ||
                !(-eps <= c2 && c2 <= 1.0 + eps))
                continue;
            // scipy/interpolate/_interpnd.pyx LinearNDInterpolator._do_evaluate
            const int32_t* v = t.simplices + 3 * int64_t(s);
            double o = 0.0;
            o = o + c0 * t.values[v[0]];
            o = o + c1 * t.values[v[1]];
            o = o + c2 * t.values[v[2]];
            phase = o;
            break;
        }
    }
    if (phase_out) phase_out[k] = phase;
    if (field_out) {
        const bool off = sqrt(x * x + y * y) > radius || phase != phase;
        field_out[2 * k] = off ? 0.0 : cos(phase);
        field_out[2 * k + 1] = off ? 0.0 : sin(phase);
    }
}

// rtpb_spot_stats (NS = kStats) and rtpb_focus_stats (NS = kFocusStats): the argument checks ...
template <int NS>
int plane_stats_check(int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups, double* workspace,
                      int64_t workspace_len, double* stats_out) {
    constexpr bool kFocus = NS == kFocusStats;
    if (dtype != RTPB_F64 && dtype != RTPB_F32) return fail(RTPB_E_INVALID, "bad dtype");
    if (group_size <= 0 || n_groups <= 0 || !plane || !stats_out || !workspace)
        return fail(RTPB_E_INVALID, kFocus ? "bad focus-stats arguments" : "bad spot-stats arguments");
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (workspace_len < n_groups * tiles * NS)
        return fail(RTPB_E_INVALID, kFocus ? "workspace too small: need n_groups * ceil(group_size/256) * 16 doubles"
                                           : "workspace too small: need n_groups * ceil(group_size/256) * 7 doubles");
    if (tiles > 65535 * 16384ll || n_groups > 65535) return fail(RTPB_E_LIMIT, "too many groups");
    return RTPB_OK;
}

// ... and the two launches (checked arguments)
template <int NS>
int plane_stats_launch(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                       double* workspace, double* stats_out, void* stream) {
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    SpotArgs a{plane, workspace, stats_out, group_size, n_groups, tiles};
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups));
    if constexpr (NS == kStats) {
        if (dtype == RTPB_F64) hipLaunchKernelGGL(spot_partial_kernel<double>, grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL(spot_partial_kernel<float>, grid, dim3(kBlock), 0, st, a);
    } else {
        if (dtype == RTPB_F64) hipLaunchKernelGGL(focus_partial_kernel<double>, grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL(focus_partial_kernel<float>, grid, dim3(kBlock), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return launch_stats_final(NS, workspace, stats_out, n_groups, tiles, st);
}

}  // namespace

// (spot_final_kernel reads only the partials, the tile count and the output of its arguments)
int rtpbi::launch_stats_final(int n_stats, double* partials, double* stats, int64_t n_groups, int64_t tiles,
                              hipStream_t st) {
    SpotArgs a{nullptr, partials, stats, 0, n_groups, tiles};
    const dim3 grid(static_cast<unsigned>(n_groups));
    if (n_stats == kStats) hipLaunchKernelGGL(spot_final_kernel<kStats>, grid, dim3(kBlock), 0, st, a);
    else if (n_stats == kWaveStats) hipLaunchKernelGGL(spot_final_kernel<kWaveStats>, grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(spot_final_kernel<kFocusStats>, grid, dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

extern "C" {

int rtpb_intersect_rays(int32_t device, int32_t dtype, const void* ray1, int64_t n1, const void* ray2, int64_t n2,
                        void* pts_out, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    if (dtype != RTPB_F64 && dtype != RTPB_F32) return fail(RTPB_E_INVALID, "bad dtype");
    if (n1 < 0 || n2 < 0 || (n1 != n2 && n1 != 1 && n2 != 1))
        return fail(RTPB_E_INVALID, "ray1 and ray2 must be the same length");
    const int64_t n = std::max(n1, n2);
    if (n == 0) return RTPB_OK;
    if (!ray1 || !ray2 || !pts_out) return fail(RTPB_E_INVALID, "NULL pointer");
    IsectArgs a{ray1, ray2, pts_out, n, n1, n2};
    DeviceGuard g(device);
    const unsigned blocks = static_cast<unsigned>((n + kBlock - 1) / kBlock);
    if (dtype == RTPB_F64)
        hipLaunchKernelGGL(intersect_kernel<double>, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(intersect_kernel<float>, dim3(blocks), dim3(kBlock), 0, static_cast<hipStream_t>(stream), a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

int rtpb_spot_stats(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                    double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    rc = plane_stats_check<kStats>(dtype, plane, group_size, n_groups, workspace, workspace_len, stats_out);
    if (rc) return rc;
    return plane_stats_launch<kStats>(device, dtype, plane, group_size, n_groups, workspace, stats_out, stream);
}

int rtpb_focus_stats(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                     double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    int rc = plane_stats_check<kFocusStats>(dtype, plane, group_size, n_groups, workspace, workspace_len, stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return plane_stats_launch<kFocusStats>(device, dtype, plane, group_size, n_groups, workspace, stats_out, stream);
}

int rtpb_wavefront_stats(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                         const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                         void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (dtype == RTPB_F32)
        return fail(RTPB_E_INVALID, "wavefront-stats: float64 planes only (a float32 phase of 1e4 ... 1e7 rad has an "
                                    "ulp of a milliradian to a radian: its wavefront is noise)");
    if (dtype != RTPB_F64) return fail(RTPB_E_INVALID, "bad wavefront-stats arguments: dtype");
    if (group_size <= 0 || n_groups <= 0 || !plane || !refs || !stats_out || !workspace)
        return fail(RTPB_E_INVALID, "bad wavefront-stats arguments");
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (tiles > 65535 * 16384ll || n_groups > 65535) return fail(RTPB_E_LIMIT, "wavefront-stats: too many groups");
    if (workspace_len < n_groups * tiles * kWaveStats)
        return fail(RTPB_E_INVALID,
                    "wavefront-stats: workspace too small: need n_groups * ceil(group_size/256) * 15 doubles");
    int rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the references: one small stream-ordered upload, as the sweeps' per-group tables
    const size_t bytes = size_t(n_groups) * kWaveRef * sizeof(double);
    StreamScratch dref;
    rc = dref.alloc(bytes, st);
    if (rc) return rc;
    PinnedStaging& pin = pinned_staging();
    rc = pin.reserve(bytes);
    if (rc) return rc;
    std::memcpy(pin.buf, refs, bytes);
    rc = pin.upload(dref.p, bytes, st);
    if (rc) return rc;
    const WaveArgs a{SpotArgs{plane, workspace, stats_out, group_size, n_groups, tiles},
                     static_cast<const double*>(dref.p)};
    hipLaunchKernelGGL(wave_partial_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    rc = launch_stats_final(kWaveStats, workspace, stats_out, n_groups, tiles, st);
    if (rc) return rc;
    return dref.release();
}

int rtpb_grid_interpolate(int32_t device, const rtpb_triangulation* tri, const double* xs, int64_t nx,
                          const double* ys, int64_t ny, double radius, double* phase_out, double* field_out,
                          void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    if (!tri || !xs || !ys || nx <= 0 || ny <= 0) return fail(RTPB_E_INVALID, "bad grid-interpolate arguments");
    if (tri->n_tri < 0 || (tri->n_tri > 0 && (!tri->transform || !tri->simplices || !tri->values)) ||
        tri->cells_x <= 0 || tri->cells_y <= 0 || !tri->cell_start || !tri->cell_tris || !(tri->cell_w > 0.0) ||
        !(tri->cell_h > 0.0))
        return fail(RTPB_E_INVALID, "bad triangulation descriptor");
    if (!phase_out && !field_out) return RTPB_OK;
    DeviceGuard g(device);
    const int64_t total = nx * ny;
    hipLaunchKernelGGL(grid_interp_kernel, dim3(static_cast<unsigned>((total + kBlock - 1) / kBlock)), dim3(kBlock),
                       0, static_cast<hipStream_t>(stream), *tri, xs, nx, ys, ny, radius, phase_out, field_out);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

}  // extern "C"
