// rtpb_sweep_beam.hip -- collimated beams (objects at infinity): the spot, focus, wavefront and image modes.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_spot_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                               const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                               const double* phi_cos_sin, double* workspace, int64_t workspace_len,
                               double* stats_out, void* stream) {
    return sweep_entry<kStats, kSrcBeam>(plan, device, n_groups, group_params,
                                         beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
                                         {workspace, workspace_len, stats_out}, stream);
}

int rtpb_focus_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                const double* phi_cos_sin, double* workspace, int64_t workspace_len,
                                double* stats_out, void* stream) {
    return sweep_entry<kFocusStats, kSrcBeam>(plan, device, n_groups, group_params,
                                              beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
                                              {workspace, workspace_len, stats_out}, stream);
}

int rtpb_wavefront_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                    const double* group_params, const double* group_frames, int64_t n_disps,
                                    int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                    const double* refs, double* workspace, int64_t workspace_len, double* stats_out,
                                    void* stream) {
    return sweep_entry<kWaveStats, kSrcBeam>(plan, device, n_groups, group_params,
                                             beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
                                             {{workspace, workspace_len, stats_out}, refs}, stream);
}

int rtpb_image_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                const double* phi_cos_sin, const double* windows, int32_t nx, int32_t ny,
                                int32_t* image_out, int32_t* outside_out, void* stream) {
    return sweep_entry<kImageStats, kSrcBeam>(plan, device, n_groups, group_params,
                                              beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
                                              {windows, nx, ny, image_out, outside_out}, stream);
}

}  // extern "C"
