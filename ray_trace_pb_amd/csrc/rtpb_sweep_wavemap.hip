// rtpb_sweep_wavemap.hip -- the fused wavefront map sweep of point-source fans: rtpb_wavefront_map_sweep, and with it
// the fan instantiations of the sweep kernel's map mode (rtpb_sweep_kernel.h, NS = kMapStats;
// rtpb_sweep_wavemap_beam.hip: the collimated beams; rtpb_wavemap.hip: the plane kernel and the shared checks).
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_wavefront_map_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                             int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                             const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                             const double* refs, const double* windows, int32_t nx, int32_t ny, int32_t q_bits,
                             double w_lim, int32_t* count_out, int64_t* sum_out, int32_t* outside_out,
                             int32_t* clipped_out, double* farthest_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    int rc = map_sweep_check(plan, n_groups, group_params, src, refs, windows, nx, ny, q_bits, w_lim, count_out,
                             sum_out, outside_out, clipped_out, farthest_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    const MapCall mp{refs, windows, nx, ny, q_bits, w_lim, count_out, reinterpret_cast<long long*>(sum_out),
                     outside_out, clipped_out, farthest_out};
    return sweep_impl<kMapStats>(plan, device, n_groups, group_params, src, nullptr, nullptr, stream, nullptr, nullptr,
                                 nullptr, nullptr, &mp);
}

}  // extern "C"
