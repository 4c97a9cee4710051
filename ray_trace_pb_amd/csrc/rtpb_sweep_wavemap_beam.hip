// rtpb_sweep_wavemap_beam.hip -- the fused wavefront map sweep of collimated beams:
// rtpb_wavefront_map_sweep_collimated, and with it the beam instantiations of the sweep kernel's map mode
// (rtpb_sweep_kernel.h, NS = kMapStats).  A unit of its own, so that it compiles beside rtpb_sweep_wavemap.hip and not
// after it.
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_wavefront_map_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                        const double* group_params, const double* group_frames, int64_t n_disps,
                                        int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                        const double* refs, const double* windows, int32_t nx, int32_t ny,
                                        int32_t q_bits, double w_lim, int32_t* count_out, int64_t* sum_out,
                                        int32_t* outside_out, int32_t* clipped_out, double* farthest_out,
                                        void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = map_sweep_check<kSrcBeam>(plan, n_groups, group_params, src, refs, windows, nx, ny, q_bits, w_lim,
                                       count_out, sum_out, outside_out, clipped_out, farthest_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    const MapCall mp{refs, windows, nx, ny, q_bits, w_lim, count_out, reinterpret_cast<long long*>(sum_out),
                     outside_out, clipped_out, farthest_out};
    return sweep_impl<kMapStats, kSrcBeam>(plan, device, n_groups, group_params, src, nullptr, nullptr, stream,
                                           nullptr, nullptr, nullptr, nullptr, &mp);
}

}  // extern "C"
