// rtpb_sweep_wave_variants_beam.hip -- the wavefront sweep of collimated beams over many systems,
// rtpb_wavefront_sweep_variants_collimated, and the final rays of small beams through each group's variant,
// rtpb_final_rays_variants_collimated; with them the beam instantiations of the sweep kernel's variant form with the
// trace kernel's full steps (rtpb_sweep_kernel.h).  A unit of its own, so that it compiles beside
// rtpb_sweep_wave_variants.hip and not after it.
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_wavefront_sweep_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf,
                                             const rtpb_material* materials, int32_t n_variants, int32_t device,
                                             int64_t n_groups, const double* group_params,
                                             const int32_t* group_variant, const double* group_frames,
                                             int64_t n_disps, int64_t nphis, const double* offsets,
                                             const double* phi_cos_sin, const double* refs, double* workspace,
                                             int64_t workspace_len, double* stats_out, void* stream) {
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    return wavefront_sweep_variants<kSrcBeam>(surfaces, nsurf, materials, n_variants, device, n_groups, group_params,
                                              group_variant, src, refs, workspace, workspace_len, stats_out, stream);
}

int rtpb_final_rays_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                        int32_t n_variants, int32_t device, int64_t n_groups,
                                        const double* group_params, const int32_t* group_variant,
                                        const double* group_frames, int64_t n_disps, int64_t nphis,
                                        const double* offsets, const double* phi_cos_sin, double* rays_out,
                                        void* stream) {
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    return final_rays_variants<kSrcBeam>(surfaces, nsurf, materials, n_variants, device, n_groups, group_params,
                                         group_variant, src, rays_out, stream);
}

}  // extern "C"
