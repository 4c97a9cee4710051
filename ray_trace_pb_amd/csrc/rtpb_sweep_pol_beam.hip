// rtpb_sweep_pol_beam.hip -- collimated beams: the polarisation mode.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_polarisation_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                       const double* group_params, const double* group_frames, int64_t n_disps,
                                       int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                       const double* coatings, int32_t n_coatings, const double polariser[3],
                                       const double analyser[3], int32_t q_bits, double* workspace,
                                       int64_t workspace_len, double* stats_out, void* stream) {
    const int rc = trans_plan_check("polarisation-sweep", plan);
    if (rc) return rc;
    return sweep_entry<kPolStats, kSrcBeam>(
        plan, device, n_groups, group_params, beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
        {{workspace, workspace_len, stats_out}, coatings, n_coatings, polariser, analyser, q_bits}, stream);
}

}  // extern "C"
