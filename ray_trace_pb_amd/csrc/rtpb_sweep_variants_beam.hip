// rtpb_sweep_variants_beam.hip -- the variant sweep of collimated beams: rtpb_focus_sweep_variants_collimated, and with
// it the beam instantiations of the sweep kernel's variant form (rtpb_sweep_kernel.h, SRC | kSrcVariant).  A unit of
// its own, so that it compiles beside rtpb_sweep_variants.hip and not after it.
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_focus_sweep_variants_collimated(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                                         int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                                         const double* group_params, const int32_t* group_variant,
                                         const double* group_frames, int64_t n_disps, int64_t nphis,
                                         const double* offsets, const double* phi_cos_sin, double* workspace,
                                         int64_t workspace_len, double* stats_out, void* stream) {
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    return focus_sweep_variants<kSrcBeam>(surfaces, nsurf, materials, n_variants, dtype, device, n_groups,
                                          group_params, group_variant, src, workspace, workspace_len, stats_out,
                                          stream);
}

}  // extern "C"
