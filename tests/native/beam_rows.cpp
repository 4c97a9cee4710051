// beam_rows.cpp -- CPU harness of the sweep's block rows with the beams' frames (rtpb_sweep_host.h plan_sweep_rows):
// tests/test_beam_host.py.  TEST INFRASTRUCTURE ONLY.
#include <algorithm>
#include <cstdint>

#include "rtpb.h"
#include "../../ray_trace_pb_amd/csrc/rtpb_sweep_host.h"

// bundles and singles hold up to n_groups entries, rows up to n_groups; counts = the three lengths.  frames: n_groups
// x 9 (normal, n1, n2), or NULL for a fan sweep's call
extern "C" void beam_sweep_rows(const double* group_params, const double* frames, int64_t n_groups, int bundles_allowed,
                                int rays_per_lane, int max_bundle, int32_t* bundles, int32_t* rows, int32_t* singles,
                                int64_t* counts) {
    const rtpbi::SweepRows r = rtpbi::plan_sweep_rows(group_params, n_groups, bundles_allowed != 0, rays_per_lane,
                                                      max_bundle, frames);
    std::copy(r.bundles.begin(), r.bundles.end(), bundles);
    std::copy(r.rows.begin(), r.rows.end(), rows);
    std::copy(r.singles.begin(), r.singles.end(), singles);
    counts[0] = static_cast<int64_t>(r.bundles.size());
    counts[1] = static_cast<int64_t>(r.rows.size());
    counts[2] = static_cast<int64_t>(r.singles.size());
}
