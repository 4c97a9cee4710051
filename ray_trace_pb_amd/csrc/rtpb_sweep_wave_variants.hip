// rtpb_sweep_wave_variants.hip -- point-source fans: the wavefront and final-rays modes over variants.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_wavefront_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                  int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                                  const int32_t* group_variant, int64_t n_thetas, int64_t nphis,
                                  const double center_ray[3], const double ex[3], const double ey[3],
                                  const double* theta_cos_sin, const double* phi_cos_sin, const double* refs,
                                  double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    return sweep_variants_entry<kWaveStats, kSrcFan>(
        surfaces, nsurf, materials, n_variants, RTPB_F64, device, n_groups, group_params, group_variant,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {{workspace, workspace_len, stats_out}, refs}, stream);
}

int rtpb_final_rays_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                             int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                             const int32_t* group_variant, int64_t n_thetas, int64_t nphis,
                             const double center_ray[3], const double ex[3], const double ey[3],
                             const double* theta_cos_sin, const double* phi_cos_sin, double* rays_out, void* stream) {
    return sweep_variants_entry<kFinalRays, kSrcFan>(
        surfaces, nsurf, materials, n_variants, RTPB_F64, device, n_groups, group_params, group_variant,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin), {rays_out}, stream);
}

}  // extern "C"
