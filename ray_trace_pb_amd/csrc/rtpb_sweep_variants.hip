// rtpb_sweep_variants.hip -- point-source fans: the focus mode over variants.
#include "rtpb_sweep_call.h"

static_assert(sizeof(DevSurface<double>) == 280, "rtpb.h states the upload's size with this figure");

extern "C" {

int rtpb_focus_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                              int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                              const double* group_params, const int32_t* group_variant, int64_t n_thetas,
                              int64_t nphis, const double center_ray[3], const double ex[3], const double ey[3],
                              const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                              int64_t workspace_len, double* stats_out, void* stream) {
    return sweep_variants_entry<kFocusStats, kSrcFan>(
        surfaces, nsurf, materials, n_variants, dtype, device, n_groups, group_params, group_variant,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {workspace, workspace_len, stats_out}, stream);
}

}  // extern "C"
