// CPU harness of the transmission statistics' per-ray rule (ray_trace_pb_amd/csrc/rtpb_trans.h: trans_fresnel,
// trans_ray, trans_term, trans_merge), built with g++ -ffp-contract=off by tests/trans_cases.py.  TEST INFRASTRUCTURE
// ONLY.
#include "../../ray_trace_pb_amd/csrc/rtpb_trans.h"

using namespace rtpb;

extern "C" {

// history: [1 + 2 nsurf][n_groups * group_size][8] float64; media: [n_groups][nsurf + 1]; coatings: [nsurf][2].
// t_out, cum_out: [nsurf][n_groups * group_size] (per ray: trans_ray's t and cum, NaN where the ray does not pass);
// stats_out: [n_groups][nsurf][5], a group's rays combined one after another from trans_none.
int trans_harness_stats(const double* history, int64_t group_size, int64_t n_groups, int32_t nsurf,
                        const double* media, const double* coatings, int32_t q_bits, double* t_out, double* cum_out,
                        double* stats_out) {
    const int64_t n = group_size * n_groups;
    const double scale = __builtin_ldexp(1.0, q_bits);
    for (int64_t g = 0; g < n_groups; ++g) {
        for (int32_t s = 0; s < nsurf; ++s) {
            TransRay acc = trans_none();
            for (int c = 0; c < kTransCols; ++c) stats_out[(g * nsurf + s) * kTransCols + c] = acc.v[c];
        }
        for (int64_t j = 0; j < group_size; ++j) {
            const int64_t i = g * group_size + j;
            double cum = 1.0;
            for (int32_t s = 0; s < nsurf; ++s) {
                const double* A = history + ((2 * s + 1) * n + i) * 8;
                const double* B = A + n * 8;
                const double* m = media + g * (nsurf + 1) + s;
                double t;
                const bool pass = trans_ray(A[0], A[1], A[2], A[3], A[4], A[5], B[0], B[1], B[2], B[3], B[4], B[5],
                                            m[0], m[1], coatings[2 * s], coatings[2 * s + 1], t, cum);
                t_out[s * n + i] = t;
                cum_out[s * n + i] = cum;
                if (pass) {
                    TransRay acc;
                    double* row = stats_out + (g * nsurf + s) * kTransCols;
                    for (int c = 0; c < kTransCols; ++c) acc.v[c] = row[c];
                    trans_merge(acc, trans_term(t, cum, scale));
                    for (int c = 0; c < kTransCols; ++c) row[c] = acc.v[c];
                }
            }
        }
    }
    return 0;
}

// trans_fresnel on n rows of (n1, n2, dA, dB): out[i] = t, and rs_rp[2 i], rs_rp[2 i + 1] the two ratios as the rule
// forms them (trans_ratios; rows with n1 == n2 give NaN there: the rule forms none)
void trans_harness_fresnel(const double* n1, const double* n2, const double* dA, const double* dB, int64_t n,
                           double* out, double* rs_rp) {
    for (int64_t i = 0; i < n; ++i) {
        const double* a = dA + 3 * i;
        const double* b = dB + 3 * i;
        out[i] = trans_fresnel(n1[i], n2[i], a[0], a[1], a[2], b[0], b[1], b[2]);
        rs_rp[2 * i] = rs_rp[2 * i + 1] = __builtin_nan("");
        if (n1[i] != n2[i])
            trans_ratios(n1[i], n2[i], a[0], a[1], a[2], b[0], b[1], b[2], rs_rp[2 * i], rs_rp[2 * i + 1]);
    }
}

// One column of two terms combined (trans_col), as the kernels combine waves and blocks
double trans_harness_col(int32_t c, double a, double b) { return trans_col(c, a, b); }

int32_t trans_harness_max_q_bits(int64_t group_size) { return trans_max_q_bits(group_size); }

}  // extern "C"
