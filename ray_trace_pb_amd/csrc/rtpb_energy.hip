// rtpb_energy.hip -- the encircled / ensquared energy of a stored plane (rtpb_spot_energy): per group, the two radial
// histograms of the final positions and the farthest ray of each.  The contribution rule and the wave's aggregated
// adds and maxima are rtpb_stats.h, shared with the fused sweep's energy mode (rtpb_sweep_energy.hip).
#include "rtpb_stats.h"

using namespace rtpbi;

namespace {

struct EnergyArgs {
    const void* __restrict__ plane;
    const double* __restrict__ params;    // per group: cx, cy, scale, 0
    int32_t* __restrict__ hist;           // [ngroups][2][nr]
    int32_t* __restrict__ outside;        // [ngroups][2]
    double* __restrict__ farthest;        // [ngroups][2]
    int64_t gsize;
    int32_t nr;
};

// spot_image_kernel's grid: block (tile, g) covers rays 256 tile ... of group g, one ray per lane.  Lanes past the
// group's end carry kImageSkip and +0, so whole waves reach wave_energy_add.
template <typename T>
__global__ __launch_bounds__(kBlock) void spot_energy_kernel(EnergyArgs a) {
    const int64_t g = blockIdx.y;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    EnergyRay e{{kImageSkip, kImageSkip}, {0.0, 0.0}};
    if (j < a.gsize) {
        const T* r = static_cast<const T*>(a.plane) + (g * a.gsize + j) * 8;
        const double p[4] = {a.params[4 * g], a.params[4 * g + 1], a.params[4 * g + 2], a.params[4 * g + 3]};
        e = energy_bins(r[0], r[1], p, a.nr);
    }
    wave_energy_add(e, a.nr, a.hist + g * 2 * a.nr, a.outside + 2 * g, a.farthest + 2 * g);
}

}  // namespace

int rtpbi::energy_check(const char* call, int32_t nr, int64_t group_size, int64_t n_groups, const void* params,
                        const void* hist_out, const void* outside_out, const void* farthest_out) {
    if (nr <= 0 || group_size <= 0 || n_groups <= 0 || !params || !hist_out || !outside_out || !farthest_out)
        return fail(RTPB_E_INVALID, std::string("bad ") + call + " arguments");
    if (nr > RTPB_MAX_ENERGY_BINS)
        return fail(RTPB_E_LIMIT, std::string(call) + ": nr is at most RTPB_MAX_ENERGY_BINS (4096)");
    if (group_size > 0x7fffffffll)
        return fail(RTPB_E_LIMIT, std::string(call) + ": more than 2^31 - 1 rays per group (the counters are int32)");
    return RTPB_OK;
}

int rtpbi::energy_clear(int32_t* hist_out, int32_t* outside_out, double* farthest_out, int64_t n_groups, int32_t nr,
                        hipStream_t st) {
    HIP_TRY(hipMemsetAsync(hist_out, 0, size_t(n_groups) * 2 * size_t(nr) * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(outside_out, 0, size_t(n_groups) * 2 * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(farthest_out, 0, size_t(n_groups) * 2 * sizeof(double), st));     // (+0.0 is all zero bits)
    return RTPB_OK;
}

extern "C" {

int rtpb_spot_energy(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                     const double* params, int32_t nr, int32_t* hist_out, int32_t* outside_out, double* farthest_out,
                     void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (dtype != RTPB_F64 && dtype != RTPB_F32) return fail(RTPB_E_INVALID, "bad spot-energy arguments: dtype");
    if (!plane) return fail(RTPB_E_INVALID, "bad spot-energy arguments");
    int rc = energy_check("spot-energy", nr, group_size, n_groups, params, hist_out, outside_out, farthest_out);
    if (rc) return rc;
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, "spot-energy: too many groups");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = energy_clear(hist_out, outside_out, farthest_out, n_groups, nr, st);
    if (rc) return rc;
    const EnergyArgs a{plane, params, hist_out, outside_out, farthest_out, group_size, nr};
    const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups));
    if (dtype == RTPB_F64) hipLaunchKernelGGL(spot_energy_kernel<double>, grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(spot_energy_kernel<float>, grid, dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

}  // extern "C"
