// rtpb_sweep_energy.hip -- the fused encircled / ensquared energy sweep of point-source fans: rtpb_energy_sweep, and
// with it the fan instantiations of the sweep kernel's energy mode (rtpb_sweep_kernel.h, NS = kEnergyStats;
// rtpb_sweep_energy_beam.hip: the collimated beams; rtpb_energy.hip: the plane kernel and the shared checks).
#include "rtpb_sweep_kernel.h"

extern "C" {

int rtpb_energy_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                      int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                      const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                      const double* params, int32_t nr, int32_t* hist_out, int32_t* outside_out,
                      double* farthest_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    const SweepSource src = fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin);
    int rc = energy_sweep_check("energy-sweep", "energy-sweep: too many groups", n_groups, group_params, src, params,
                                nr, hist_out, outside_out, farthest_out);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    const EnergyCall en{params, nr, hist_out, outside_out, farthest_out};
    return sweep_impl<kEnergyStats>(plan, device, n_groups, group_params, src, nullptr, nullptr, stream, nullptr,
                                    nullptr, nullptr, &en);
}

}  // extern "C"
