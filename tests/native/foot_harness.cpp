// CPU harness of the footprint statistics' per-ray term (ray_trace_pb_amd/csrc/rtpb_foot.h: foot_ray, foot_merge),
// built with g++ -ffp-contract=off by tests/foot_harness.py.  TEST INFRASTRUCTURE ONLY.
#include "../../ray_trace_pb_amd/csrc/rtpb_foot.h"

using namespace rtpb;

extern "C" {

// history: [1 + 2 nsurf][n_groups * group_size][8] float64; frames: [nsurf][9]; out: [n_groups][nsurf][8].
// The rays of a group are combined one after another, from foot_none.
int foot_harness_stats(const double* history, int64_t group_size, int64_t n_groups, int32_t nsurf,
                       const double* frames, double* out) {
    const int64_t n = group_size * n_groups;
    for (int64_t g = 0; g < n_groups; ++g) {
        for (int32_t s = 0; s < nsurf; ++s) {
            const double* q = frames + kFootFrame * s;
            const double fr[kFootFrame] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]};
            FootRay acc = foot_none();
            for (int64_t j = 0; j < group_size; ++j) {
                const double* A = history + ((2 * s + 1) * n + g * group_size + j) * 8;
                const double* B = A + n * 8;
                foot_merge(acc, foot_ray(A[0], A[1], A[2], B[0], B[1], B[2], fr));
            }
            for (int c = 0; c < kFootCols; ++c) out[(g * nsurf + s) * kFootCols + c] = acc.v[c];
        }
    }
    return 0;
}

// One column of two terms combined (foot_col), as the kernels combine waves and blocks
double foot_harness_col(int32_t c, double a, double b) { return foot_col(c, a, b); }

}  // extern "C"
