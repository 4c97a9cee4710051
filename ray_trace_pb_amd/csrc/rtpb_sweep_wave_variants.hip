// rtpb_sweep_wave_variants.hip -- the wavefront sweep of point-source fans over many systems,
// rtpb_wavefront_sweep_variants, and the final rays of small fans through each group's variant,
// rtpb_final_rays_variants, which gives such a sweep its chief rays in one launch; with them the fan instantiations of
// the sweep kernel's variant form with the trace kernel's full steps (rtpb_sweep_kernel.h, SRC | kSrcVariant with
// NS = kWaveStats / kFinalRays).  A unit of its own, so that it compiles beside the other sweep units;
// rtpb_sweep_wave_variants_beam.hip holds the collimated beams.
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_wavefront_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                  int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                                  const int32_t* group_variant, int64_t n_thetas, int64_t nphis,
                                  const double center_ray[3], const double ex[3], const double ey[3],
                                  const double* theta_cos_sin, const double* phi_cos_sin, const double* refs,
                                  double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    return wavefront_sweep_variants<kSrcFan>(surfaces, nsurf, materials, n_variants, device, n_groups, group_params,
                                             group_variant, src, refs, workspace, workspace_len, stats_out, stream);
}

int rtpb_final_rays_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                             int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                             const int32_t* group_variant, int64_t n_thetas, int64_t nphis,
                             const double center_ray[3], const double ex[3], const double ey[3],
                             const double* theta_cos_sin, const double* phi_cos_sin, double* rays_out, void* stream) {
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    return final_rays_variants<kSrcFan>(surfaces, nsurf, materials, n_variants, device, n_groups, group_params,
                                        group_variant, src, rays_out, stream);
}

}  // extern "C"
