// rtpb_sweep_foot_beam.hip -- the fused footprint sweep of collimated beams: rtpb_footprint_sweep_collimated, and with
// it the beam instantiations of the sweep kernel's footprint mode (rtpb_sweep_kernel.h, NS = kFootStats).  A unit of
// its own, so that it compiles beside rtpb_sweep_foot.hip and not after it.
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_footprint_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                    const double* group_params, const double* group_frames, int64_t n_disps,
                                    int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                    const double* frames, int32_t n_frames, double* workspace, int64_t workspace_len,
                                    double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = foot_sweep_check<kSrcBeam>(plan, n_groups, group_params, src, frames, n_frames, workspace, workspace_len,
                                        stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kFootStats, kSrcBeam>(plan, device, n_groups, group_params, src, workspace, stats_out, stream,
                                            nullptr, frames);
}

}  // extern "C"
