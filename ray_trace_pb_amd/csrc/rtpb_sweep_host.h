// rtpb_sweep_host.h -- the host arithmetic of the fused sweep (rtpb_sweep.hip), free of HIP so that a plain C++
// build can test it (tests/native/math_harness.cpp): which groups share a block row, every medium at every group's
// wavelength, and where each part of the one upload lies.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "rtpb_math.h"

namespace rtpbi {

// Block rows of a sweep: bundle row y covers groups bundles[rows[2y]] ... of which there are rows[2y + 1]; single
// row y covers group singles[y] (ascending).
struct SweepRows {
    std::vector<int32_t> bundles, rows, singles;
};

// Groups of one field point (the bit patterns of x, y, z; group_params holds x, y, z, wavelength per group) go into
// bundle rows of rays_per_lane ... max_bundle groups, multiples of rays_per_lane (see sweep_kernel); a point's
// leftover groups are single rows.  Without bundles (they need the host-evaluated media) every group is single.
// A collimated-beam sweep passes its groups' frames (normal, n1, n2: 9 doubles per group): a row's groups then share
// the whole beam, the bit patterns of the point and of the frame together -- fields at one point that differ in
// their normal, the ordinary case, never share a row.  Without frames the key's other words are 0, and the rows and
// their order are those of the point alone.
// A variant sweep passes its groups' variants (one int32 per group): a row's groups then share the system as well, so
// a block reads one set of surface descriptors.  The variant is the key's last word: without variants it is 0, and
// with all variants equal it is one value, so in both cases the rows and their order are those of the source alone.
inline SweepRows plan_sweep_rows(const double* group_params, int64_t n_groups, bool bundles_allowed,
                                 int rays_per_lane, int max_bundle, const double* frames = nullptr,
                                 const int32_t* variants = nullptr) {
    SweepRows r;
    std::map<std::array<uint64_t, 13>, std::vector<int32_t>> by_point;   // source (bit patterns) -> groups
    for (int64_t gi = 0; gi < n_groups; ++gi) {
        std::array<uint64_t, 13> key{};
        std::memcpy(key.data(), group_params + 4 * gi, 3 * sizeof(double));
        if (frames) std::memcpy(key.data() + 3, frames + 9 * gi, 9 * sizeof(double));
        if (variants) key[12] = static_cast<uint32_t>(variants[gi]);
        if (bundles_allowed) by_point[key].push_back(static_cast<int32_t>(gi));
        else r.singles.push_back(static_cast<int32_t>(gi));
    }
    for (const auto& kv : by_point) {
        const auto& gs = kv.second;
        size_t k = 0;
        while (gs.size() - k >= size_t(rays_per_lane)) {
            const size_t left = gs.size() - k;
            const size_t nb = std::min<size_t>(max_bundle, left - left % rays_per_lane);
            r.rows.push_back(static_cast<int32_t>(r.bundles.size()));
            r.rows.push_back(static_cast<int32_t>(nb));
            r.bundles.insert(r.bundles.end(), gs.begin() + k, gs.begin() + k + nb);
            k += nb;
        }
        for (; k < gs.size(); ++k) r.singles.push_back(gs[k]);
    }
    std::sort(r.singles.begin(), r.singles.end());
    return r;
}

// out[n_groups][n_mats + 3 S], S = n_mats - 1 surfaces: per group, n of every material at the group's wavelength --
// material_n on the host, i.e. the kernel's own arithmetic (-ffp-contract=off, IEEE division and sqrt), at the
// wavelength the kernel would see (rounded to the storage type) -- then per surface n_s / n_s+1, 1 / n_s+1 and
// host_rcp_ok(n_s+1) as 0 / 1.  No POLY6 material.
inline void fill_group_media(const rtpb::DevMaterial<double>* mats, size_t n_mats, const double* table,
                             const double* group_params, int64_t n_groups, int32_t dtype, double* out) {
    const size_t M = n_mats, S = n_mats - 1;
    for (int64_t gi = 0; gi < n_groups; ++gi) {
        const double w = group_params[4 * gi + 3];
        const double wl = dtype == RTPB_F32 ? double(float(w)) : w;
        double* q = out + gi * (M + 3 * S);
        for (size_t k = 0; k < M; ++k) q[k] = rtpb::material_n<double, false, true>(mats[k], wl, table);
        for (size_t k = 0; k < S; ++k) {
            q[M + k] = q[k] / q[k + 1];
            q[M + S + k] = 1.0 / q[k + 1];
            q[M + 2 * S + k] = rtpb::host_rcp_ok(q[k + 1]) ? 1.0 : 0.0;
        }
    }
}

// The one upload of a sweep, as byte offsets (for the pinned host copy and the device block alike): the trig tables
// ((cos, sin) pairs: thetas, then phis) at 0, the group parameters, the media table (media_doubles per group, or 0),
// the image or wavefront sweep's block (head_doubles for its header, then per_group doubles per group: the image's
// windows, 4, or the wavefront references, 8; nothing for the other sweeps), the beams' frames (frame_doubles per
// group: normal, n1, n2; 0 for fans), then the int32 index block (bundles, singles, rows).  A beam sweep's tables
// are the phis' pairs and then its offsets as plain doubles: it passes ceil(n_disps / 2) pair slots for them.
// A variant sweep's surface descriptors (desc_bytes: n_variants x nsurf DevSurface<double>, a multiple of 8 bytes) lie
// between the frames and the index block, and its groups' variants (n_groups int32, counted in n_idx) end that block.
struct SweepLayout {
    size_t grp, gn, img, win, frm, dsc, idx, bytes;
    SweepLayout(int64_t n_thetas, int64_t nphis, int64_t n_groups, size_t media_doubles, size_t n_idx,
                size_t head_doubles = 0, size_t per_group = 4, size_t frame_doubles = 0, size_t desc_bytes = 0) {
        grp = size_t(n_thetas + nphis) * 2 * sizeof(double);
        gn = grp + size_t(4 * n_groups) * sizeof(double);
        img = gn + size_t(n_groups) * media_doubles * sizeof(double);
        win = img + head_doubles * sizeof(double);
        frm = win + (head_doubles ? per_group * size_t(n_groups) * sizeof(double) : 0);
        dsc = frm + frame_doubles * size_t(n_groups) * sizeof(double);
        idx = dsc + desc_bytes;
        bytes = idx + n_idx * sizeof(int32_t);
    }
};

}  // namespace rtpbi
