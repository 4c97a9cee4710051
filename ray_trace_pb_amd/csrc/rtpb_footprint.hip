// rtpb_footprint.hip -- the footprint statistics of a stored history (rtpb_footprint_stats: the unfused path, and the
// way to use the feature on a history one already has) and the second pass they share with the fused footprint sweep
// (launch_foot_final).  The per-ray term and its combination are rtpb_foot.h's, the wave and block reductions
// rtpb_stats.h's.
#include "rtpb_stats.h"

#include <cstring>

using namespace rtpbi;

namespace {

struct FootArgs {
    const double* __restrict__ hist;        // [1 + 2 nsurf][n_groups * gsize][8]
    const double* __restrict__ frames;      // [nsurf][kFootFrame]
    double* __restrict__ partials;          // [n_groups][tiles][nsurf][kFootCols]
    int64_t gsize, ngroups, tiles;
    int32_t nsurf;
};

// Block (tile, group, surface): the tile's rays at that surface, planes 2 s + 1 and 2 s + 2 of the history
__global__ __launch_bounds__(kBlock) void foot_partial_kernel(FootArgs a) {
    __shared__ double tab[kBlock / 64][kFootCols];
    const int64_t tile = blockIdx.x, g = blockIdx.y;
    const int s = blockIdx.z;
    const int64_t j = tile * kBlock + threadIdx.x;
    FootRay f = foot_none();
    if (j < a.gsize) {
        const int64_t n = a.ngroups * a.gsize;
        const double* A = a.hist + ((2 * s + 1) * n + g * a.gsize + j) * 8;
        const double* B = A + n * 8;
        const double* q = a.frames + kFootFrame * s;
        const double fr[kFootFrame] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
        f = foot_ray(A[0], A[1], A[2], B[0], B[1], B[2], fr);
    }
    const double v = foot_block_reduce(f, tab);
    if (threadIdx.x < kFootCols)
        a.partials[((g * a.tiles + tile) * a.nsurf + s) * kFootCols + threadIdx.x] = v;
}

struct FootFinalArgs {
    const double* __restrict__ partials;    // [n_groups][blocks][nsurf][kFootCols]
    double* __restrict__ stats;             // [n_groups][nsurf][kFootCols]
    int64_t blocks;
    int32_t nsurf;
};

// Block (surface, group): thread t combines the group's partials t, t + 256, ..., then one reduction over the block
__global__ __launch_bounds__(kBlock) void foot_final_kernel(FootFinalArgs a) {
    __shared__ double tab[kBlock / 64][kFootCols];
    const int s = blockIdx.x;
    const int64_t g = blockIdx.y;
    FootRay f = foot_none();
    for (int64_t b = threadIdx.x; b < a.blocks; b += kBlock) {
        const double* p = a.partials + ((g * a.blocks + b) * a.nsurf + s) * kFootCols;
        FootRay o;
#pragma unroll
        for (int c = 0; c < kFootCols; ++c) o.v[c] = p[c];
        foot_merge(f, o);
    }
    const double v = foot_block_reduce(f, tab);
    if (threadIdx.x < kFootCols) a.stats[(g * a.nsurf + s) * kFootCols + threadIdx.x] = v;
}

}  // namespace

int rtpbi::launch_foot_final(const double* partials, double* stats, int64_t n_groups, int64_t blocks, int32_t nsurf,
                             hipStream_t st) {
    const FootFinalArgs a{partials, stats, blocks, nsurf};
    hipLaunchKernelGGL(foot_final_kernel, dim3(static_cast<unsigned>(nsurf), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

extern "C" {

int rtpb_footprint_stats(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                         int32_t nsurf, const double* frames, double* workspace, int64_t workspace_len,
                         double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (dtype == RTPB_F32)
        return fail(RTPB_E_INVALID, "footprint-stats: float64 histories only (the statistics are defined on the "
                                    "float64 history)");
    if (dtype != RTPB_F64) return fail(RTPB_E_INVALID, "bad footprint-stats arguments: dtype");
    if (group_size <= 0 || n_groups <= 0 || nsurf <= 0 || !history || !frames || !stats_out || !workspace)
        return fail(RTPB_E_INVALID, "bad footprint-stats arguments");
    if (nsurf > RTPB_MAX_SURFACES) return fail(RTPB_E_LIMIT, "footprint-stats: more than RTPB_MAX_SURFACES surfaces");
    for (int64_t k = 0; k < int64_t(nsurf) * kFootFrame; ++k)
        if (!(frames[k] - frames[k] == 0.0))
            return fail(RTPB_E_INVALID, "footprint-stats: frame " + std::to_string(k / kFootFrame) + " is not finite");
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (tiles > 0x7fffffffll || n_groups > 65535) return fail(RTPB_E_LIMIT, "footprint-stats: too many groups");
    if (workspace_len / (int64_t(nsurf) * kFootCols) / tiles < n_groups)
        return fail(RTPB_E_INVALID,
                    "footprint-stats: workspace too small: need n_groups * ceil(group_size/256) * nsurf * 8 doubles");
    int rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the frames: one small stream-ordered upload, as the wavefront references
    const size_t bytes = size_t(nsurf) * kFootFrame * sizeof(double);
    StreamScratch dfr;
    rc = dfr.alloc(bytes, st);
    if (rc) return rc;
    PinnedStaging& pin = pinned_staging();
    rc = pin.reserve(bytes);
    if (rc) return rc;
    std::memcpy(pin.buf, frames, bytes);
    rc = pin.upload(dfr.p, bytes, st);
    if (rc) return rc;
    const FootArgs a{static_cast<const double*>(history), static_cast<const double*>(dfr.p), workspace, group_size,
                     n_groups, tiles, nsurf};
    hipLaunchKernelGGL(foot_partial_kernel,
                       dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups), static_cast<unsigned>(nsurf)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    rc = launch_foot_final(workspace, stats_out, n_groups, tiles, nsurf, st);
    if (rc) return rc;
    return dfr.release();
}

}  // extern "C"
