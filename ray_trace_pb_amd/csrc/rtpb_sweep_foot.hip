// rtpb_sweep_foot.hip -- the fused footprint sweep of point-source fans: rtpb_footprint_sweep, and with it the fan
// instantiations of the sweep kernel's footprint mode (rtpb_sweep_kernel.h, NS = kFootStats; rtpb_sweep_foot_beam.hip:
// the collimated beams; rtpb_footprint.hip: the reducer of a stored history and the second pass).
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_footprint_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                         int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                         const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                         const double* frames, int32_t n_frames, double* workspace, int64_t workspace_len,
                         double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    int rc = foot_sweep_check<kSrcFan>(plan, n_groups, group_params, src, frames, n_frames, workspace, workspace_len,
                                       stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kFootStats>(plan, device, n_groups, group_params, src, workspace, stats_out, stream, nullptr,
                                  frames);
}

}  // extern "C"
