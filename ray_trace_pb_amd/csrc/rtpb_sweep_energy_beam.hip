// rtpb_sweep_energy_beam.hip -- the fused encircled / ensquared energy sweep of collimated beams:
// rtpb_energy_sweep_collimated, and with it the beam instantiations of the sweep kernel's energy mode
// (rtpb_sweep_kernel.h, NS = kEnergyStats).  A unit of its own, so that it compiles beside rtpb_sweep_energy.hip and
// not after it.
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_energy_sweep_collimated(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                                 const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                                 const double* phi_cos_sin, const double* params, int32_t nr, int32_t* hist_out,
                                 int32_t* outside_out, double* farthest_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = beam_source(group_frames, n_disps, nphis, offsets, phi_cos_sin);
    int rc = energy_sweep_check<kSrcBeam>("energy-sweep-collimated", "energy-sweep-collimated: too many groups",
                                          n_groups, group_params, src, params, nr, hist_out, outside_out,
                                          farthest_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    const EnergyCall en{params, nr, hist_out, outside_out, farthest_out};
    return sweep_impl<kEnergyStats, kSrcBeam>(plan, device, n_groups, group_params, src, nullptr, nullptr, stream,
                                              nullptr, nullptr, nullptr, &en);
}

}  // extern "C"
