// rtpb_sweep_wave_variants_beam.hip -- collimated beams: the wavefront and final-rays modes over variants.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_wavefront_sweep_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf,
                                             const rtpb_material* materials, int32_t n_variants, int32_t device,
                                             int64_t n_groups, const double* group_params,
                                             const int32_t* group_variant, const double* group_frames,
                                             int64_t n_disps, int64_t nphis, const double* offsets,
                                             const double* phi_cos_sin, const double* refs, double* workspace,
                                             int64_t workspace_len, double* stats_out, void* stream) {
    return sweep_variants_entry<kWaveStats, kSrcBeam>(
        surfaces, nsurf, materials, n_variants, RTPB_F64, device, n_groups, group_params, group_variant,
        beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
        {{workspace, workspace_len, stats_out}, refs}, stream);
}

int rtpb_final_rays_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                        int32_t n_variants, int32_t device, int64_t n_groups,
                                        const double* group_params, const int32_t* group_variant,
                                        const double* group_frames, int64_t n_disps, int64_t nphis,
                                        const double* offsets, const double* phi_cos_sin, double* rays_out,
                                        void* stream) {
    return sweep_variants_entry<kFinalRays, kSrcBeam>(
        surfaces, nsurf, materials, n_variants, RTPB_F64, device, n_groups, group_params, group_variant,
        beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin), {rays_out}, stream);
}

}  // extern "C"
