// rtpb_sweep_foot_beam.hip -- collimated beams: the footprint mode.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_footprint_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                    const double* group_params, const double* group_frames, int64_t n_disps,
                                    int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                    const double* frames, int32_t n_frames, double* workspace, int64_t workspace_len,
                                    double* stats_out, void* stream) {
    return sweep_entry<kFootStats, kSrcBeam>(plan, device, n_groups, group_params,
                                             beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
                                             {{workspace, workspace_len, stats_out}, frames, n_frames}, stream);
}

}  // extern "C"
