// rtpb_sweep_wavemap_beam.hip -- collimated beams: the wavefront map mode.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_wavefront_map_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups,
                                        const double* group_params, const double* group_frames, int64_t n_disps,
                                        int64_t nphis, const double* offsets, const double* phi_cos_sin,
                                        const double* refs, const double* windows, int32_t nx, int32_t ny,
                                        int32_t q_bits, double w_lim, int32_t* count_out, int64_t* sum_out,
                                        int32_t* outside_out, int32_t* clipped_out, double* farthest_out,
                                        void* stream) {
    return sweep_entry<kMapStats, kSrcBeam>(
        plan, device, n_groups, group_params, beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
        {refs, windows, nx, ny, q_bits, w_lim, count_out, reinterpret_cast<long long*>(sum_out), outside_out,
         clipped_out, farthest_out},
        stream);
}

}  // extern "C"
