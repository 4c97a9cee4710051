// CPU harness of the polarisation statistics' per-ray rule (ray_trace_pb_amd/csrc/rtpb_pol.h: pol_launch, pol_surface,
// pol_term, pol_merge), built with g++ -ffp-contract=off by tests/pol_cases.py.  TEST INFRASTRUCTURE ONLY.
#include "../../ray_trace_pb_amd/csrc/rtpb_pol.h"

using namespace rtpb;

extern "C" {

// history: [1 + 2 nsurf][n_groups * group_size][8] float64; media: [n_groups][nsurf + 1]; coatings: [nsurf][2] as the
// caller gives them, {mode, value}; u, w: the two unit axes.  states_out: [nsurf][n_groups * group_size][6] (per ray
// the state after the surface, NaN for none); stats_out: [n_groups][nsurf][6], a group's rays combined one after
// another from pol_none.
int pol_harness_stats(const double* history, int64_t group_size, int64_t n_groups, int32_t nsurf, const double* media,
                      const double* coatings, const double* u, const double* w, int32_t q_bits, double* states_out,
                      double* stats_out) {
    const int64_t n = group_size * n_groups;
    const double scale = __builtin_ldexp(1.0, q_bits);
    const double uu[3] = {u[0], u[1], u[2]}, ww[3] = {w[0], w[1], w[2]};
    for (int64_t k = 0; k < n_groups * nsurf * kPolCols; ++k) stats_out[k] = 0.0;
    for (int64_t g = 0; g < n_groups; ++g) {
        for (int64_t j = 0; j < group_size; ++j) {
            const int64_t i = g * group_size + j;
            double e[kPolState];
            pol_launch(history[i * 8 + 3], history[i * 8 + 4], history[i * 8 + 5], uu, e);
            for (int32_t s = 0; s < nsurf; ++s) {
                const double* A = history + ((2 * s + 1) * n + i) * 8;
                const double* B = A + n * 8;
                const double* m = media + g * (nsurf + 1) + s;
                const double mode = coatings[2 * s];
                const bool pass = foot_finite3(A[0], A[1], A[2]) && foot_finite3(B[0], B[1], B[2]);
                pol_surface(pass, A[3], A[4], A[5], B[3], B[4], B[5], m[0], m[1], mode,
                            pol_coat_amplitude(mode, coatings[2 * s + 1]), e);
                for (int c = 0; c < kPolState; ++c) states_out[(s * n + i) * kPolState + c] = e[c];
                if (pass) {
                    PolRay acc;
                    double* row = stats_out + (g * nsurf + s) * kPolCols;
                    for (int c = 0; c < kPolCols; ++c) acc.v[c] = row[c];
                    pol_merge(acc, pol_term(e, B[3], B[4], B[5], ww, scale));
                    for (int c = 0; c < kPolCols; ++c) row[c] = acc.v[c];
                }
            }
        }
    }
    return 0;
}

// pol_amplitudes of a FRESNEL surface on n rows of (n1, n2, dA, dB): ts_tp[2 i], ts_tp[2 i + 1]
void pol_harness_amplitudes(const double* n1, const double* n2, const double* dA, const double* dB, int64_t n,
                            double* ts_tp) {
    for (int64_t i = 0; i < n; ++i) {
        const double* a = dA + 3 * i;
        const double* b = dB + 3 * i;
        pol_amplitudes(n1[i], n2[i], a[0], a[1], a[2], b[0], b[1], b[2], kCoatFresnel, 0.0, ts_tp[2 * i],
                       ts_tp[2 * i + 1]);
    }
}

// pol_launch on n directions: states[6 i ...]
void pol_harness_launch(const double* d, const double* u, int64_t n, double* states) {
    const double uu[3] = {u[0], u[1], u[2]};
    for (int64_t i = 0; i < n; ++i) {
        double e[kPolState];
        pol_launch(d[3 * i], d[3 * i + 1], d[3 * i + 2], uu, e);
        for (int c = 0; c < kPolState; ++c) states[6 * i + c] = e[c];
    }
}

// One passing pol_surface step on n rows: states in place; the coating {mode, value} is the same for all rows
void pol_harness_surface(const double* dA, const double* dB, const double* n1, const double* n2, double mode,
                         double value, int64_t n, double* states) {
    for (int64_t i = 0; i < n; ++i) {
        double e[kPolState];
        for (int c = 0; c < kPolState; ++c) e[c] = states[6 * i + c];
        pol_surface(true, dA[3 * i], dA[3 * i + 1], dA[3 * i + 2], dB[3 * i], dB[3 * i + 1], dB[3 * i + 2], n1[i],
                    n2[i], mode, pol_coat_amplitude(mode, value), e);
        for (int c = 0; c < kPolState; ++c) states[6 * i + c] = e[c];
    }
}

}  // extern "C"
