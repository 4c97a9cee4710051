// rtpb_sweep_energy_beam.hip -- collimated beams: the energy mode.
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_energy_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                 const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                 const double* phi_cos_sin, const double* params, int32_t nr, int32_t* hist_out,
                                 int32_t* outside_out, double* farthest_out, void* stream) {
    return sweep_entry<kEnergyStats, kSrcBeam>(plan, device, n_groups, group_params,
                                               beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin),
                                               {params, nr, hist_out, outside_out, farthest_out}, stream);
}

}  // extern "C"
