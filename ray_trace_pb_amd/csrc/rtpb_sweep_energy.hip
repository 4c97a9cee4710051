// rtpb_sweep_energy.hip -- point-source fans: the energy mode (the shared checks: rtpb_energy.hip).
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_energy_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                      int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                      const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                      const double* params, int32_t nr, int32_t* hist_out, int32_t* outside_out,
                      double* farthest_out, void* stream) {
    return sweep_entry<kEnergyStats, kSrcFan>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {params, nr, hist_out, outside_out, farthest_out}, stream);
}

}  // extern "C"
