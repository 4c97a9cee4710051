// rtpb_sweep.hip -- the fused sweeps of point-source fans: rtpb_spot_sweep, rtpb_focus_sweep, rtpb_image_sweep and
// rtpb_wavefront_sweep, and with them the fan instantiations of the sweep kernel (rtpb_sweep_kernel.h: the kernel, the
// argument checks and the host driver; rtpb_sweep_beam.hip: the collimated beams).
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_spot_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                    int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                    const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                    int64_t workspace_len, double* stats_out, void* stream) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    int rc = check_device(device);
    if (rc) return rc;
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    rc = sweep_check<kStats>(n_groups, group_params, src, workspace, workspace_len, stats_out);
    if (rc) return rc;
    return sweep_impl<kStats>(plan, device, n_groups, group_params, src, workspace, stats_out, stream);
}

int rtpb_focus_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                     int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                     const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                     int64_t workspace_len, double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    int rc = sweep_check<kFocusStats>(n_groups, group_params, src, workspace, workspace_len, stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kFocusStats>(plan, device, n_groups, group_params, src, workspace, stats_out, stream);
}

int rtpb_wavefront_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                         int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                         const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                         const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                         void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    if (plan->dtype != RTPB_F64)
        return fail(RTPB_E_INVALID, "wavefront-sweep: float64 plans only (a float32 phase of 1e4 ... 1e7 rad has an "
                                    "ulp of a milliradian to a radian: its wavefront is noise)");
    if (!refs) return fail(RTPB_E_INVALID, "bad wavefront-sweep arguments");
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    int rc = sweep_check<kWaveStats>(n_groups, group_params, src, workspace, workspace_len, stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kWaveStats>(plan, device, n_groups, group_params, src, workspace, stats_out, stream, nullptr,
                                  refs);
}

int rtpb_image_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                     int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                     const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                     const double* windows, int32_t nx, int32_t ny, int32_t* image_out, int32_t* outside_out,
                     void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    int rc = image_sweep_check("image-sweep", "image-sweep: too many groups", n_groups, group_params, src, windows,
                               nx, ny, image_out, outside_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    const ImageCall im{windows, nx, ny, image_out, outside_out};
    return sweep_impl<kImageStats>(plan, device, n_groups, group_params, src, nullptr, nullptr, stream, &im);
}

}  // extern "C"
