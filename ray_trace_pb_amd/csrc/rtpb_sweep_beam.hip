// rtpb_sweep_beam.hip -- the fused sweeps of collimated beams (objects at infinity): rtpb_spot_sweep_collimated,
// rtpb_focus_sweep_collimated, rtpb_image_sweep_collimated and rtpb_wavefront_sweep_collimated, and with them the beam
// instantiations of the sweep kernel (rtpb_sweep_kernel.h).  A unit of its own, so that it compiles beside
// rtpb_sweep.hip and not after it.
#include "rtpb_sweep_kernel.h"

extern "C" {

// (in all four the arguments come first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)

int rtpb_spot_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                               const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                               const double* phi_cos_sin, double* workspace, int64_t workspace_len,
                               double* stats_out, void* stream) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = sweep_check<kStats, kSrcBeam>(n_groups, group_params, src, workspace, workspace_len, stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kStats, kSrcBeam>(plan, device, n_groups, group_params, src, workspace, stats_out, stream);
}

int rtpb_focus_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                const double* phi_cos_sin, double* workspace, int64_t workspace_len,
                                double* stats_out, void* stream) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = sweep_check<kFocusStats, kSrcBeam>(n_groups, group_params, src, workspace, workspace_len, stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kFocusStats, kSrcBeam>(plan, device, n_groups, group_params, src, workspace, stats_out, stream);
}

int rtpb_wavefront_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                    const double* group_params, const double* group_frames, int64_t n_disps,
                                    int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                    const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                                    void* stream) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    if (plan->dtype != RTPB_F64)
        return fail(RTPB_E_INVALID, "wavefront-sweep: float64 plans only (a float32 phase of 1e4 ... 1e7 rad has an "
                                    "ulp of a milliradian to a radian: its wavefront is noise)");
    if (!refs) return fail(RTPB_E_INVALID, "bad wavefront-sweep arguments");
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = sweep_check<kWaveStats, kSrcBeam>(n_groups, group_params, src, workspace, workspace_len, stats_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kWaveStats, kSrcBeam>(plan, device, n_groups, group_params, src, workspace, stats_out, stream,
                                            nullptr, refs);
}

int rtpb_image_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                const double* phi_cos_sin, const double* windows, int32_t nx, int32_t ny,
                                int32_t* image_out, int32_t* outside_out, void* stream) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = image_sweep_check<kSrcBeam>("image-sweep-collimated", "image-sweep-collimated: too many groups", n_groups,
                                         group_params, src, windows, nx, ny, image_out, outside_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    const ImageCall im{windows, nx, ny, image_out, outside_out};
    return sweep_impl<kImageStats, kSrcBeam>(plan, device, n_groups, group_params, src, nullptr, nullptr, stream,
                                             &im);
}

}  // extern "C"
