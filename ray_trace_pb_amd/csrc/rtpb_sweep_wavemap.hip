// rtpb_sweep_wavemap.hip -- point-source fans: the wavefront map mode (the shared checks: rtpb_wavemap.hip).
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_wavefront_map_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                             int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                             const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                             const double* refs, const double* windows, int32_t nx, int32_t ny, int32_t q_bits,
                             double w_lim, int32_t* count_out, int64_t* sum_out, int32_t* outside_out,
                             int32_t* clipped_out, double* farthest_out, void* stream) {
    return sweep_entry<kMapStats, kSrcFan>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {refs, windows, nx, ny, q_bits, w_lim, count_out, reinterpret_cast<long long*>(sum_out), outside_out,
         clipped_out, farthest_out},
        stream);
}

}  // extern "C"
