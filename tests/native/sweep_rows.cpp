// sweep_rows.cpp -- CPU harness of the sweep's block rows (rtpb_sweep_host.h plan_sweep_rows), with and without the
// beams' frames and the groups' variants, and of a variant call's upload layout (SweepLayout) and surface codes:
// tests/sweep_rows.py.  TEST INFRASTRUCTURE ONLY.
#include <algorithm>
#include <cstdint>

#include "rtpb.h"
#include "../../ray_trace_pb_amd/csrc/rtpb_math.h"
#include "../../ray_trace_pb_amd/csrc/rtpb_sweep_host.h"

// bundles and singles hold up to n_groups entries, rows up to n_groups (a row has at least two groups); counts = the
// three lengths.  frames: n_groups x 9 (normal, n1, n2) or NULL; variants: n_groups int32 or NULL.  n_trailing = how
// many of plan_sweep_rows' trailing arguments the call passes: 0 leaves frames and variants to their defaults (the
// fan sweeps' call), 1 passes the frames (the collimated sweeps'), 2 the frames and the variants (the variant sweeps')
extern "C" void sweep_rows(const double* group_params, const double* frames, const int32_t* variants, int n_trailing,
                           int64_t n_groups, int bundles_allowed, int rays_per_lane, int max_bundle, int32_t* bundles,
                           int32_t* rows, int32_t* singles, int64_t* counts) {
    const rtpbi::SweepRows r =
        n_trailing == 2 ? rtpbi::plan_sweep_rows(group_params, n_groups, bundles_allowed != 0, rays_per_lane,
                                                 max_bundle, frames, variants)
        : n_trailing == 1 ? rtpbi::plan_sweep_rows(group_params, n_groups, bundles_allowed != 0, rays_per_lane,
                                                   max_bundle, frames)
                          : rtpbi::plan_sweep_rows(group_params, n_groups, bundles_allowed != 0, rays_per_lane,
                                                   max_bundle);
    std::copy(r.bundles.begin(), r.bundles.end(), bundles);
    std::copy(r.rows.begin(), r.rows.end(), rows);
    std::copy(r.singles.begin(), r.singles.end(), singles);
    counts[0] = static_cast<int64_t>(r.bundles.size());
    counts[1] = static_cast<int64_t>(r.rows.size());
    counts[2] = static_cast<int64_t>(r.singles.size());
}

// the (kind, geometry form) code the kernels dispatch a surface on, from the library's own lowering (rtpb_math.h
// lower_surface, surface_code): 3 * kind + {0 general, 1 axial, 2 x-z plane}
extern "C" int variant_surface_code(const rtpb_surface* s) {
    const rtpb::DevSurface<double> d = rtpb::lower_surface(*s);
    return rtpb::surface_code<double>(d.kind, d.rcp_ok);
}

// the byte offsets of a sweep's upload: out = {grp, gn, img, win, frm, dsc, idx, bytes}
extern "C" void variant_sweep_layout(int64_t n_a, int64_t n_b, int64_t n_groups, int64_t media_doubles, int64_t n_idx,
                                     int64_t frame_doubles, int64_t desc_bytes, int64_t* out) {
    const rtpbi::SweepLayout l(n_a, n_b, n_groups, size_t(media_doubles), size_t(n_idx), 0, 4, size_t(frame_doubles),
                               size_t(desc_bytes));
    const size_t v[8] = {l.grp, l.gn, l.img, l.win, l.frm, l.dsc, l.idx, l.bytes};
    for (int k = 0; k < 8; ++k) out[k] = static_cast<int64_t>(v[k]);
}
