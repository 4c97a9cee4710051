// rtpb_sweep_pol.hip -- point-source fans: the polarisation mode (its second pass: rtpb_polarisation.hip).
#include "rtpb_sweep_call.h"

extern "C" {

int rtpb_polarisation_sweep(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                            int64_t n_thetas, int64_t nphis, const double center_ray[3], const double ex[3],
                            const double ey[3], const double* theta_cos_sin, const double* phi_cos_sin,
                            const double* coatings, int32_t n_coatings, const double polariser[3],
                            const double analyser[3], int32_t q_bits, double* workspace, int64_t workspace_len,
                            double* stats_out, void* stream) {
    const int rc = trans_plan_check("polarisation-sweep", plan);
    if (rc) return rc;
    return sweep_entry<kPolStats, kSrcFan>(
        plan, device, n_groups, group_params,
        fan_source(n_thetas, nphis, center_ray, ex, ey, theta_cos_sin, phi_cos_sin),
        {{workspace, workspace_len, stats_out}, coatings, n_coatings, polariser, analyser, q_bits}, stream);
}

}  // extern "C"
