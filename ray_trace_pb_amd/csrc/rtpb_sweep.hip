// rtpb_sweep.hip -- point-source fans: the spot, focus, wavefront and image modes over a plan.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_spot_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                    int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                    const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                    int64_t workspace_len, double* stats_out, void* stream) {
    // (the one entry point that looks for the device before its arguments: sweep_entry's kDeviceFirst)
    return sweep_entry<kStats, kSrcFan, true>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {workspace, workspace_len, stats_out}, stream);
}

int rtpb_focus_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                     int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                     const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                     int64_t workspace_len, double* stats_out, void* stream) {
    return sweep_entry<kFocusStats, kSrcFan>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {workspace, workspace_len, stats_out}, stream);
}

int rtpb_wavefront_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                         int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                         const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                         const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                         void* stream) {
    return sweep_entry<kWaveStats, kSrcFan>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {{workspace, workspace_len, stats_out}, refs}, stream);
}

int rtpb_image_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                     int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                     const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                     const double* windows, int32_t nx, int32_t ny, int32_t* image_out, int32_t* outside_out,
                     void* stream) {
    return sweep_entry<kImageStats, kSrcFan>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {windows, nx, ny, image_out, outside_out}, stream);
}

}  // extern "C"
