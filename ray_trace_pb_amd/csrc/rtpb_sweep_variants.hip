// rtpb_sweep_variants.hip -- the variant sweep of point-source fans: rtpb_focus_sweep_variants, many perturbed copies
// of a system in one fused pass, and with it the fan instantiations of the sweep kernel's variant form
// (rtpb_sweep_kernel.h, SRC | kSrcVariant: focus statistics, host-evaluated media).  A unit of its own, so that it
// compiles beside rtpb_sweep.hip; rtpb_sweep_variants_beam.hip holds the collimated beams.
#include "rtpb_sweep_kernel.h"

static_assert(sizeof(DevSurface<double>) == 280, "rtpb.h states the upload's size with this figure");

extern "C" {

int rtpb_focus_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                              int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                              const double* group_params, const int32_t* group_variant, int64_t n_thetas,
                              int64_t nphis, const double center_ray[3], const double ex[3], const double ey[3],
                              const double* theta_cos_sin, const double* phi_cos_sin, double* workspace,
                              int64_t workspace_len, double* stats_out, void* stream) {
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    return focus_sweep_variants<kSrcFan>(surfaces, nsurf, materials, n_variants, dtype, device, n_groups, group_params,
                                         group_variant, src, workspace, workspace_len, stats_out, stream);
}

}  // extern "C"
