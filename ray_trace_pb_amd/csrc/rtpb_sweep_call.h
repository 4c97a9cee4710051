// rtpb_sweep_call.h -- the host side of the fused sweep: what a call says about its rays (SweepSource), each mode's
// host hooks (SweepHost<NS>, on top of the mode's device descriptor SweepMode<NS> of rtpb_sweep_kernel.h), the one
// driver (sweep_impl), the one entry prologue (sweep_entry) and the variant calls' lowering and prologue.
#pragma once

#include <type_traits>

#include "rtpb_sweep_kernel.h"

namespace {

// What a call says about its groups' rays besides group_params, as the entry points received it (host pointers).
// Ray j of a group takes entry j % n_a of tab_a and entry j / n_a of tab_b.
//   fan (rtpb_*_sweep):             n_a = n_thetas, tab_a the thetas' (cos, sin); n_b = nphis, tab_b the phis'
//                                   (cos, sin); c, ex, ey the axis and its basis
//   beam (rtpb_*_sweep_collimated): n_a = nphis, tab_a the phis' (cos, sin); n_b = n_disps, tab_b the offsets;
//                                   frames n_groups x kFrame
struct SweepSource {
    int64_t n_a, n_b;
    const double* tab_a;
    const double* tab_b;
    const double* c;
    const double* ex;
    const double* ey;
    const double* frames;
    bool complete(int src) const {
        return n_a > 0 && n_b > 0 && tab_a && tab_b && (src == kSrcBeam ? frames != nullptr : c && ex && ey);
    }
    // rays per group, for the checks that hold it to int32: a product past int64 is past the limit too
    int64_t gsize_clamped() const { return n_a > 0x7fffffffll / n_b ? 0x80000000ll : n_a * n_b; }
};

inline SweepSource fan_source(int64_t n_thetas, int64_t nphis, const double* center_ray, const double* ex,
                              const double* ey, const double* theta_cos_sin, const double* phi_cos_sin) {
    return SweepSource{n_thetas, nphis, theta_cos_sin, phi_cos_sin, center_ray, ex, ey, nullptr};
}

inline SweepSource beam_source(const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                               const double* phi_cos_sin) {
    return SweepSource{nphis, n_disps, phi_cos_sin, offsets, nullptr, nullptr, nullptr, group_frames};
}

// The messages name the two counts of a group's rays as the call's source does
template <int SRC>
constexpr const char* rays_of() { return SRC == kSrcBeam ? "n_disps*nphis" : "n_thetas*nphis"; }

// A mode's host hooks, beside its device descriptor: Call (the call's own arguments as the entry point received
// them), f64_only<SRC>() (!kF32 modes: the refusal of a float32 plan), check<SRC>(nsurf, ...) (the argument checks, in
// the source's wording; no device is touched), head_doubles(nsurf) (the header and what follows it per call, in
// doubles; kPerGroup doubles per group follow those), fill(call, ..., head, tail) (both into the staging buffer),
// clear(call, n_groups, st) (the outputs the kernel adds to), partials(call) (modes without a header:
// SweepArgs::partials) and finish(call, ..., st) (the launch after the sweep).
template <int NS>
struct SweepHost;

// The statistics modes' arguments: the tile partials' workspace and the statistics
struct StatsCall {
    double* workspace;
    int64_t workspace_len;
    double* stats_out;
};

// Spot and focus statistics (and the wavefront statistics' common part): kCols columns per tile partial in the
// workspace, reduced by launch_stats_final.  kName names the mode in the messages.
template <int NS>
struct StatsHost : SweepMode<NS> {
    using Call = StatsCall;
    static constexpr const char* kName = NS == kStats ? "spot" : NS == kFocusStats ? "focus" : "wavefront";
    template <int SRC>
    static int check(int32_t, int64_t n_groups, const double* group_params, const SweepSource& s, const StatsCall& c,
                     bool extra_ok = true) {
        if (!extra_ok || n_groups <= 0 || !s.complete(SRC) || !group_params || !c.workspace || !c.stats_out)
            return fail(RTPB_E_INVALID, std::string("bad ") + kName + "-sweep arguments");
        const int64_t tiles = (s.n_a * s.n_b + kBlock - 1) / kBlock;
        if (c.workspace_len < n_groups * tiles * NS)
            return fail(RTPB_E_INVALID, std::string("workspace too small: need n_groups * ceil(") + rays_of<SRC>() +
                                            "/256) * " + std::to_string(NS) + " doubles");
        if (tiles > 0x7fffffffll || n_groups > 65535) return fail(RTPB_E_LIMIT, "too many groups or rays per group");
        return RTPB_OK;
    }
    static size_t head_doubles(int32_t) { return 0; }
    static void fill(const StatsCall&, int64_t, int32_t, char*, char*) {}
    static int clear(const StatsCall&, int64_t, hipStream_t) { return RTPB_OK; }
    static double* partials(const StatsCall& c) { return c.workspace; }
    static int finish(const StatsCall& c, int64_t n_groups, int64_t tiles, int32_t, hipStream_t st) {
        return launch_stats_final(NS, c.workspace, c.stats_out, n_groups, tiles, st);
    }
};

template <>
struct SweepHost<kStats> : StatsHost<kStats> {};

template <>
struct SweepHost<kFocusStats> : StatsHost<kFocusStats> {
    static constexpr const char* kVariantCall = "focus-sweep-variants";
};

// Wavefront statistics: the groups' references (host, n_groups x kWaveRef) join the upload behind the SweepWave word
template <>
struct SweepHost<kWaveStats> : StatsHost<kWaveStats> {
    struct Call : StatsCall {
        const double* refs;
    };
    static constexpr const char* kVariantCall = "wavefront-sweep-variants";
    template <int SRC>
    static const char* f64_only() {
        return "wavefront-sweep: float64 plans only (a float32 phase of 1e4 ... 1e7 rad has an ulp of a milliradian "
               "to a radian: its wavefront is noise)";
    }
    template <int SRC>
    static int check(int32_t nsurf, int64_t n_groups, const double* group_params, const SweepSource& s,
                     const Call& c) {
        return StatsHost::check<SRC>(nsurf, n_groups, group_params, s, c, c.refs != nullptr);
    }
    static size_t head_doubles(int32_t) { return sizeof(SweepWave) / sizeof(double); }
    static void fill(const Call& c, int64_t n_groups, int32_t, char* head, char* tail) {
        const SweepWave h{c.workspace};
        std::memcpy(head, &h, sizeof(h));
        std::memcpy(tail, c.refs, size_t(kWaveRef * n_groups) * sizeof(double));
    }
};

// Final rays: no workspace and no reduction; rays_out is n_groups x gsize x 8, written by the kernel, and a group
// holds one tile of rays at the most
template <>
struct SweepHost<kFinalRays> : SweepMode<kFinalRays> {
    struct Call {
        double* rays_out;
    };
    static constexpr const char* kVariantCall = "final-rays-variants";
    template <int SRC>
    static int check(int32_t, int64_t n_groups, const double* group_params, const SweepSource& s, const Call& c) {
        if (n_groups <= 0 || !s.complete(SRC) || !group_params || !c.rays_out)
            return fail(RTPB_E_INVALID, "bad final-rays arguments");
        if (s.n_a > kBlock || s.n_b > kBlock || s.n_a * s.n_b > kBlock)
            return fail(RTPB_E_LIMIT, std::string("final-rays: more than 256 rays per group (") + rays_of<SRC>() + ")");
        if (n_groups > 65535) return fail(RTPB_E_LIMIT, "too many groups or rays per group");
        return RTPB_OK;
    }
    static size_t head_doubles(int32_t) { return 0; }
    static void fill(const Call&, int64_t, int32_t, char*, char*) {}
    static int clear(const Call&, int64_t, hipStream_t) { return RTPB_OK; }
    static double* partials(const Call& c) { return c.rays_out; }
    static int finish(const Call&, int64_t, int64_t, int32_t, hipStream_t) { return RTPB_OK; }
};

// Footprints: one finite frame per surface of the plan (host, nsurf x kFootFrame) behind the SweepFoot word -- nothing
// per group; the workspace holds one partial per block of kSweepRays tiles (n_groups x blocks x nsurf x kFootCols) and
// stats_out is n_groups x nsurf x kFootCols, combined by launch_foot_final
template <>
struct SweepHost<kFootStats> : SweepMode<kFootStats> {
    struct Call : StatsCall {
        const double* frames;
        int32_t n_frames;
    };
    template <int SRC>
    static const char* f64_only() {
        return "footprint-sweep: float64 plans only (the statistics are defined on the float64 history)";
    }
    template <int SRC>
    static int check(int32_t nsurf, int64_t n_groups, const double* group_params, const SweepSource& s,
                     const Call& c) {
        if (n_groups <= 0 || !s.complete(SRC) || !group_params || !c.frames || !c.workspace || !c.stats_out)
            return fail(RTPB_E_INVALID, "bad footprint-sweep arguments");
        if (c.n_frames != nsurf)
            return fail(RTPB_E_INVALID, "footprint-sweep: n_frames (" + std::to_string(c.n_frames) +
                                            ") is not the plan's number of surfaces (" + std::to_string(nsurf) + ")");
        for (int64_t k = 0; k < int64_t(c.n_frames) * kFootFrame; ++k)
            if (!(c.frames[k] - c.frames[k] == 0.0))
                return fail(RTPB_E_INVALID,
                            "footprint-sweep: frame " + std::to_string(k / kFootFrame) + " is not finite");
        if (nsurf > RTPB_MAX_SURFACES)
            return fail(RTPB_E_LIMIT, "footprint-sweep: more than RTPB_MAX_SURFACES surfaces");
        if (n_groups > 65535) return fail(RTPB_E_LIMIT, "footprint-sweep: too many groups or rays per group");
        // (n_a * n_b: a product past int64 is past the limit too)
        if (s.n_a > (0x7fffffffll * kBlock) / s.n_b)
            return fail(RTPB_E_LIMIT, "footprint-sweep: too many groups or rays per group");
        const int64_t tiles = (s.n_a * s.n_b + kBlock - 1) / kBlock;
        const int64_t blocks = (tiles + kSweepRays - 1) / kSweepRays;
        if (c.workspace_len / (int64_t(c.n_frames) * kFootCols) / blocks < n_groups)
            return fail(RTPB_E_INVALID, std::string("footprint-sweep: workspace too small: need n_groups * ceil(ceil(") +
                                            rays_of<SRC>() + "/256)/2) * nsurf * 8 doubles");
        return RTPB_OK;
    }
    static size_t head_doubles(int32_t nsurf) {
        return sizeof(SweepFoot) / sizeof(double) + size_t(nsurf) * kFootFrame;
    }
    static void fill(const Call& c, int64_t, int32_t nsurf, char* head, char*) {
        const SweepFoot h{c.workspace};
        std::memcpy(head, &h, sizeof(h));
        std::memcpy(head + sizeof(h), c.frames, size_t(nsurf) * kFootFrame * sizeof(double));
    }
    static int clear(const Call&, int64_t, hipStream_t) { return RTPB_OK; }
    static int finish(const Call& c, int64_t n_groups, int64_t tiles, int32_t nsurf, hipStream_t st) {
        return launch_foot_final(c.workspace, c.stats_out, n_groups, (tiles + kSweepRays - 1) / kSweepRays, nsurf, st);
    }
};

// Transmission: one coating per surface of the plan (host, nsurf x kTransCoat) behind the SweepTrans words -- nothing
// per group; the workspace holds one partial per block of kSweepRays tiles (n_groups x blocks x nsurf x kTransCols) and
// stats_out is n_groups x nsurf x kTransCols, combined by launch_trans_final.  The checks of the coatings and of q_bits
// are rtpb_transmission_stats's (trans_check).
template <>
struct SweepHost<kTransStats> : SweepMode<kTransStats> {
    struct Call : StatsCall {
        const double* coatings;
        int32_t n_coatings, q_bits;
    };
    template <int SRC>
    static const char* f64_only() {
        return "transmission-sweep: float64 plans only (the statistics are defined on the float64 history)";
    }
    template <int SRC>
    static int check(int32_t nsurf, int64_t n_groups, const double* group_params, const SweepSource& s,
                     const Call& c) {
        if (n_groups <= 0 || !s.complete(SRC) || !group_params || !c.coatings || !c.workspace || !c.stats_out)
            return fail(RTPB_E_INVALID, "bad transmission-sweep arguments");
        if (c.n_coatings != nsurf)
            return fail(RTPB_E_INVALID, "transmission-sweep: n_coatings (" + std::to_string(c.n_coatings) +
                                            ") is not the plan's number of surfaces (" + std::to_string(nsurf) + ")");
        if (nsurf > RTPB_MAX_SURFACES)
            return fail(RTPB_E_LIMIT, "transmission-sweep: more than RTPB_MAX_SURFACES surfaces");
        if (n_groups > 65535) return fail(RTPB_E_LIMIT, "transmission-sweep: too many groups or rays per group");
        // (n_a * n_b: a product past int64 is past the limit too)
        if (s.n_a > (0x7fffffffll * kBlock) / s.n_b)
            return fail(RTPB_E_LIMIT, "transmission-sweep: too many groups or rays per group");
        int rc = trans_check("transmission-sweep", c.coatings, nsurf, c.q_bits, s.n_a * s.n_b);
        if (rc) return rc;
        const int64_t tiles = (s.n_a * s.n_b + kBlock - 1) / kBlock;
        const int64_t blocks = (tiles + kSweepRays - 1) / kSweepRays;
        if (c.workspace_len / (int64_t(nsurf) * kTransCols) / blocks < n_groups)
            return fail(RTPB_E_INVALID,
                        std::string("transmission-sweep: workspace too small: need n_groups * ceil(ceil(") +
                            rays_of<SRC>() + "/256)/2) * nsurf * 5 doubles");
        return RTPB_OK;
    }
    static size_t head_doubles(int32_t nsurf) {
        return sizeof(SweepTrans) / sizeof(double) + size_t(nsurf) * kTransCoat;
    }
    static void fill(const Call& c, int64_t, int32_t nsurf, char* head, char*) {
        const SweepTrans h{c.workspace, std::ldexp(1.0, c.q_bits)};
        std::memcpy(head, &h, sizeof(h));
        std::memcpy(head + sizeof(h), c.coatings, size_t(nsurf) * kTransCoat * sizeof(double));
    }
    static int clear(const Call&, int64_t, hipStream_t) { return RTPB_OK; }
    static int finish(const Call& c, int64_t n_groups, int64_t tiles, int32_t nsurf, hipStream_t st) {
        return launch_trans_final(c.workspace, c.stats_out, n_groups, (tiles + kSweepRays - 1) / kSweepRays, nsurf, st);
    }
};

// Polarisation: the transmission mode's call with the two unit axes (host, three doubles each); behind the SweepPol
// words the coatings ride as {mode, amplitude} (pol_coat_amplitude, once per call).  The workspace holds one partial
// per block of kSweepRays tiles (n_groups x blocks x nsurf x kPolCols) and stats_out is n_groups x nsurf x kPolCols,
// combined by launch_pol_final.  The checks of the coatings, the axes and q_bits are rtpb_polarisation_stats's
// (pol_check).
template <>
struct SweepHost<kPolStats> : SweepMode<kPolStats> {
    struct Call : StatsCall {
        const double* coatings;
        int32_t n_coatings;
        const double* polariser;
        const double* analyser;
        int32_t q_bits;
    };
    template <int SRC>
    static const char* f64_only() {
        return "polarisation-sweep: float64 plans only (the statistics are defined on the float64 history)";
    }
    template <int SRC>
    static int check(int32_t nsurf, int64_t n_groups, const double* group_params, const SweepSource& s,
                     const Call& c) {
        if (n_groups <= 0 || !s.complete(SRC) || !group_params || !c.coatings || !c.polariser || !c.analyser ||
            !c.workspace || !c.stats_out)
            return fail(RTPB_E_INVALID, "bad polarisation-sweep arguments");
        if (c.n_coatings != nsurf)
            return fail(RTPB_E_INVALID, "polarisation-sweep: n_coatings (" + std::to_string(c.n_coatings) +
                                            ") is not the plan's number of surfaces (" + std::to_string(nsurf) + ")");
        if (nsurf > RTPB_MAX_SURFACES)
            return fail(RTPB_E_LIMIT, "polarisation-sweep: more than RTPB_MAX_SURFACES surfaces");
        if (n_groups > 65535) return fail(RTPB_E_LIMIT, "polarisation-sweep: too many groups or rays per group");
        // (n_a * n_b: a product past int64 is past the limit too)
        if (s.n_a > (0x7fffffffll * kBlock) / s.n_b)
            return fail(RTPB_E_LIMIT, "polarisation-sweep: too many groups or rays per group");
        int rc = pol_check("polarisation-sweep", c.coatings, nsurf, c.polariser, c.analyser, c.q_bits, s.n_a * s.n_b);
        if (rc) return rc;
        const int64_t tiles = (s.n_a * s.n_b + kBlock - 1) / kBlock;
        const int64_t blocks = (tiles + kSweepRays - 1) / kSweepRays;
        if (c.workspace_len / (int64_t(nsurf) * kPolCols) / blocks < n_groups)
            return fail(RTPB_E_INVALID,
                        std::string("polarisation-sweep: workspace too small: need n_groups * ceil(ceil(") +
                            rays_of<SRC>() + "/256)/2) * nsurf * 6 doubles");
        return RTPB_OK;
    }
    static size_t head_doubles(int32_t nsurf) {
        return sizeof(SweepPol) / sizeof(double) + size_t(nsurf) * kTransCoat;
    }
    static void fill(const Call& c, int64_t, int32_t nsurf, char* head, char*) {
        const SweepPol h{c.workspace, std::ldexp(1.0, c.q_bits),
                         {c.polariser[0], c.polariser[1], c.polariser[2]},
                         {c.analyser[0], c.analyser[1], c.analyser[2]}};
        std::memcpy(head, &h, sizeof(h));
        double* const coat = reinterpret_cast<double*>(head + sizeof(h));
        for (int32_t k = 0; k < nsurf; ++k) {
            coat[kTransCoat * k] = c.coatings[kTransCoat * k];
            coat[kTransCoat * k + 1] = pol_coat_amplitude(c.coatings[kTransCoat * k], c.coatings[kTransCoat * k + 1]);
        }
    }
    static int clear(const Call&, int64_t, hipStream_t) { return RTPB_OK; }
    static int finish(const Call& c, int64_t n_groups, int64_t tiles, int32_t nsurf, hipStream_t st) {
        return launch_pol_final(c.workspace, c.stats_out, n_groups, (tiles + kSweepRays - 1) / kSweepRays, nsurf, st);
    }
};

// The counter modes have no workspace, no statistics and nothing after the sweep: the kernel adds into the call's
// outputs, which the call clears first.  Their checks are the plane calls' between the sweep's own.
struct CounterHost {
    // plane(what, gsize): the plane call's check; gsize is held to int32 there
    template <int SRC, typename PlaneCheck>
    static int check(const char* mode, int64_t n_groups, const double* group_params, const SweepSource& s,
                     PlaneCheck plane) {
        const std::string what = std::string(mode) + (SRC == kSrcBeam ? "-sweep-collimated" : "-sweep");
        if (n_groups <= 0 || !s.complete(SRC) || !group_params)
            return fail(RTPB_E_INVALID, "bad " + what + " arguments");
        int rc = plane(what.c_str(), s.gsize_clamped());
        if (rc) return rc;
        if (n_groups > 65535) return fail(RTPB_E_LIMIT, what + ": too many groups");
        return RTPB_OK;
    }
    template <typename Call>
    static int finish(const Call&, int64_t, int64_t, int32_t, hipStream_t) {
        return RTPB_OK;
    }
};

// Image: the groups' windows (host, n_groups x 4) behind SweepImage
template <>
struct SweepHost<kImageStats> : SweepMode<kImageStats>, CounterHost {
    struct Call {
        const double* windows;
        int32_t nx, ny;
        int32_t* image_out;
        int32_t* outside_out;
    };
    template <int SRC>
    static int check(int32_t, int64_t n_groups, const double* group_params, const SweepSource& s, const Call& c) {
        return CounterHost::check<SRC>("image", n_groups, group_params, s, [&](const char* what, int64_t gsize) {
            return image_check(what, c.nx, c.ny, gsize, n_groups, c.windows, c.image_out, c.outside_out);
        });
    }
    static size_t head_doubles(int32_t) { return sizeof(SweepImage) / sizeof(double); }
    static void fill(const Call& c, int64_t n_groups, int32_t, char* head, char* tail) {
        const SweepImage h{c.image_out, c.outside_out, c.nx, c.ny};
        std::memcpy(head, &h, sizeof(h));
        std::memcpy(tail, c.windows, size_t(4 * n_groups) * sizeof(double));
    }
    static int clear(const Call& c, int64_t n_groups, hipStream_t st) {
        return image_clear(c.image_out, c.outside_out, n_groups, c.nx, c.ny, st);
    }
};

// Energy curves: the groups' parameters (host, n_groups x 4: cx, cy, scale, 0) behind SweepEnergy
template <>
struct SweepHost<kEnergyStats> : SweepMode<kEnergyStats>, CounterHost {
    struct Call {
        const double* params;
        int32_t nr;
        int32_t* hist_out;
        int32_t* outside_out;
        double* farthest_out;
    };
    template <int SRC>
    static int check(int32_t, int64_t n_groups, const double* group_params, const SweepSource& s, const Call& c) {
        return CounterHost::check<SRC>("energy", n_groups, group_params, s, [&](const char* what, int64_t gsize) {
            return energy_check(what, c.nr, gsize, n_groups, c.params, c.hist_out, c.outside_out, c.farthest_out);
        });
    }
    static size_t head_doubles(int32_t) { return sizeof(SweepEnergy) / sizeof(double); }
    static void fill(const Call& c, int64_t n_groups, int32_t, char* head, char* tail) {
        const SweepEnergy h{c.hist_out, c.outside_out, c.farthest_out, c.nr, 0};
        std::memcpy(head, &h, sizeof(h));
        std::memcpy(tail, c.params, size_t(4 * n_groups) * sizeof(double));
    }
    static int clear(const Call& c, int64_t n_groups, hipStream_t st) {
        return energy_clear(c.hist_out, c.outside_out, c.farthest_out, n_groups, c.nr, st);
    }
};

// Wavefront map: per group its reference and its window (host, n_groups x kWaveRef and n_groups x kMapWin; kMapPar
// doubles per group in the upload) behind SweepMap
template <>
struct SweepHost<kMapStats> : SweepMode<kMapStats>, CounterHost {
    struct Call {
        const double* refs;
        const double* windows;
        int32_t nx, ny, q_bits;
        double w_lim;
        int32_t* count_out;
        long long* sum_out;
        int32_t* outside_out;
        int32_t* clipped_out;
        double* farthest_out;
    };
    template <int SRC>
    static std::string f64_only() {
        return std::string(SRC == kSrcBeam ? "wavefront-map-sweep-collimated" : "wavefront-map-sweep") +
               ": float64 plans only (a float32 phase of 1e4 ... 1e7 rad has an ulp of a milliradian to a radian: its "
               "wavefront is noise)";
    }
    template <int SRC>
    static int check(int32_t, int64_t n_groups, const double* group_params, const SweepSource& s, const Call& c) {
        auto plane = [&](const char* what, int64_t gsize) {
            return wavemap_check(what, c.nx, c.ny, c.q_bits, c.w_lim, gsize, n_groups, c.refs, c.windows, c.count_out,
                                 c.sum_out, c.outside_out, c.clipped_out, c.farthest_out);
        };
        return CounterHost::check<SRC>("wavefront-map", n_groups, group_params, s, plane);
    }
    static size_t head_doubles(int32_t) { return sizeof(SweepMap) / sizeof(double); }
    static void fill(const Call& c, int64_t n_groups, int32_t, char* head, char* tail) {
        const SweepMap h{c.count_out, c.sum_out, c.outside_out, c.clipped_out, c.farthest_out,
                         std::ldexp(1.0, c.q_bits), c.w_lim, c.nx, c.ny};
        std::memcpy(head, &h, sizeof(h));
        double* const par = reinterpret_cast<double*>(tail);
        for (int64_t gi = 0; gi < n_groups; ++gi) {
            std::memcpy(par + kMapPar * gi, c.refs + kWaveRef * gi, kWaveRef * sizeof(double));
            std::memcpy(par + kMapPar * gi + kWaveRef, c.windows + kMapWin * gi, kMapWin * sizeof(double));
        }
    }
    static int clear(const Call& c, int64_t n_groups, hipStream_t st) {
        return wavemap_clear(c.count_out, c.sum_out, c.outside_out, c.clipped_out, c.farthest_out, n_groups, c.nx,
                             c.ny, st);
    }
};

// A variant sweep's systems (SRC | kSrcVariant), lowered on the host (lower_variant_call): no plan and no device blob,
// the descriptors ride in the call's upload.  All variants have nsurf surfaces and nsurf + 1 materials.
struct VariantCall {
    int32_t nsurf = 0, n_variants = 0, dtype = RTPB_F64;
    int feat = 0;                                   // 1: some variant holds a PerfectLens (FEAT 17 for the call)
    const int32_t* group_variant = nullptr;         // host, n_groups, each in [0, n_variants)
    std::vector<DevSurface<double>> desc;           // [n_variants][nsurf], as a plan's blob holds them
    std::vector<DevMaterial<double>> mats;          // [n_variants][nsurf + 1]
    std::vector<std::vector<double>> tables;        // per variant: its TABLE materials' (wavelength, n) pairs
};

// The sweep itself (checked arguments): plan the block rows, lay the one upload out, fill its common parts and the
// mode's, clear the mode's outputs, send it, launch the sweep kernels, then the mode's launch after them.  vc (SRC |
// kSrcVariant, and then no plan): a group's media are its own variant's, its block row is keyed on the variant too, and
// the descriptors and the groups' variants join the upload -- independent of what the mode adds to it.
template <int NS, int SRC>
int sweep_impl(const rtpb_plan* plan_c, int32_t device, int64_t n_groups, const double* group_params,
               const SweepSource& src, const typename SweepHost<NS>::Call& call, void* stream,
               const VariantCall* vc = nullptr) {
    using Mode = SweepHost<NS>;
    constexpr bool kBeam = (SRC & ~kSrcVariant) == kSrcBeam, kVar = (SRC & kSrcVariant) != 0;
    static_assert(kVar ? Mode::kVariants : Mode::kPlans, "the mode takes no such systems");
    auto* plan = const_cast<rtpb_plan*>(plan_c);
    const int64_t gsize = src.n_a * src.n_b;
    const int64_t tiles = (gsize + kBlock - 1) / kBlock;
    DeviceGuard g(device);
    void* blob = nullptr;
    int rc = RTPB_OK;
    if constexpr (!kVar) {
        rc = plan_device_blob(plan, device, &blob);
        if (rc) return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    // bundle rows need the host-evaluated media, which a POLY6 material rules out
    const bool pre_n = kVar || (plan->feat & 2) == 0;
    const int32_t nsurf = kVar ? vc->nsurf : plan->nsurf;
    const int32_t dtype = kVar ? vc->dtype : plan->dtype;
    const int feat = kVar ? vc->feat : plan->feat;
    const size_t M = size_t(nsurf) + 1;
    const SweepRows pr = plan_sweep_rows(group_params, n_groups, pre_n && Mode::kBundles, kSweepRays, kMaxBundle,
                                         kBeam ? src.frames : nullptr, kVar ? vc->group_variant : nullptr);
    // (a beam's second table is its offsets, plain doubles: half as many pair slots)
    const SweepLayout lay(src.n_a, kBeam ? (src.n_b + 1) / 2 : src.n_b, n_groups, pre_n ? M + 3 * (M - 1) : 0,
                          pr.bundles.size() + pr.singles.size() + pr.rows.size() + (kVar ? size_t(n_groups) : 0),
                          Mode::head_doubles(nsurf), Mode::kPerGroup, kBeam ? kFrame : 0,
                          kVar ? vc->desc.size() * sizeof(DevSurface<double>) : 0);
    StreamScratch dbuf;
    rc = dbuf.alloc(lay.bytes, st);
    if (rc) return rc;
    PinnedStaging& g_pinned = pinned_staging();
    rc = g_pinned.reserve(lay.bytes);
    if (rc) return rc;
    char* const h = reinterpret_cast<char*>(g_pinned.buf);
    std::memcpy(h, src.tab_a, size_t(2 * src.n_a) * sizeof(double));
    std::memcpy(h + size_t(2 * src.n_a) * sizeof(double), src.tab_b, size_t((kBeam ? 1 : 2) * src.n_b) * sizeof(double));
    std::memcpy(h + lay.grp, group_params, size_t(4 * n_groups) * sizeof(double));
    if constexpr (kBeam) std::memcpy(h + lay.frm, src.frames, size_t(kFrame * n_groups) * sizeof(double));
    if constexpr (kVar) {
        // each group's media from its own variant's materials and table
        double* const gn = reinterpret_cast<double*>(h + lay.gn);
        for (int64_t gi = 0; gi < n_groups; ++gi) {
            const size_t v = size_t(vc->group_variant[gi]);
            fill_group_media(vc->mats.data() + v * M, M, vc->tables[v].data(), group_params + 4 * gi, 1, dtype,
                             gn + gi * (M + 3 * (M - 1)));
        }
        std::memcpy(h + lay.dsc, vc->desc.data(), vc->desc.size() * sizeof(DevSurface<double>));
    } else if (pre_n) {
        std::vector<DevMaterial<double>> dm(M);
        for (size_t k = 0; k < M; ++k) dm[k] = device_material(*plan, k);
        fill_group_media(dm.data(), M, plan->table.data(), group_params, n_groups, dtype,
                         reinterpret_cast<double*>(h + lay.gn));
    }
    Mode::fill(call, n_groups, nsurf, h + lay.img, h + lay.win);
    rc = Mode::clear(call, n_groups, st);
    if (rc) return rc;
    int32_t* hidx = reinterpret_cast<int32_t*>(h + lay.idx);
    hidx = std::copy(pr.bundles.begin(), pr.bundles.end(), hidx);
    hidx = std::copy(pr.singles.begin(), pr.singles.end(), hidx);
    hidx = std::copy(pr.rows.begin(), pr.rows.end(), hidx);
    if constexpr (kVar) std::copy(vc->group_variant, vc->group_variant + n_groups, hidx);
    rc = g_pinned.upload(dbuf.p, lay.bytes, st);
    if (rc) return rc;
    const char* const d = static_cast<const char*>(dbuf.p);
    SweepArgs a{};
    const int32_t* didx = reinterpret_cast<const int32_t*>(d + lay.idx);
    if constexpr (kVar) {
        a.surf = reinterpret_cast<const DevSurface<double>*>(d + lay.dsc);
        a.variant = didx + pr.bundles.size() + pr.singles.size() + pr.rows.size();
    } else {
        a.surf = static_cast<const DevSurface<double>*>(blob);
        a.mats = reinterpret_cast<const DevMaterial<double>*>(static_cast<char*>(blob) + plan->off_mats);
        a.table = reinterpret_cast<const double*>(static_cast<char*>(blob) + plan->off_table);
    }
    a.tab = reinterpret_cast<const double2*>(d);
    a.grp = reinterpret_cast<const double*>(d + lay.grp);
    a.gn = reinterpret_cast<const double*>(d + lay.gn);
    if constexpr (std::is_void_v<typename Mode::Head>) a.partials = Mode::partials(call);
    else a.block = d + lay.img;
    a.n_thetas = src.n_a;
    a.nphis = src.n_b;
    a.gsize = gsize;
    a.tiles = tiles;
    if constexpr (kBeam) {
        a.frm = reinterpret_cast<const double*>(d + lay.frm);
    } else {
        for (int j = 0; j < 3; ++j) {
            a.c[j] = src.c[j]; a.ex[j] = src.ex[j]; a.ey[j] = src.ey[j];
        }
    }
    a.nsurf = nsurf;
    sweep_divisor(src.n_a, gsize, a.nt_mul, a.nt_shift);
    auto go = [&](auto tag) {
        using TS = decltype(tag);
        const int f = feat & 3;                       // lens / POLY6 code (no pre_n: POLY6); tables always compiled in
        if constexpr (Mode::kBundles) {
            if (!pr.rows.empty()) {
                SweepArgs ap = a;
                ap.gidx = didx;
                ap.rows = didx + pr.bundles.size() + pr.singles.size();
                const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(pr.rows.size() / 2));
                if (f == 0) hipLaunchKernelGGL((sweep_kernel<TS, 16, true, NS, SRC>), grid, dim3(kBlock), 0, st, ap);
                else hipLaunchKernelGGL((sweep_kernel<TS, 17, true, NS, SRC>), grid, dim3(kBlock), 0, st, ap);
            }
        }
        if (!pr.singles.empty()) {
            SweepArgs as = a;
            as.gidx = didx + pr.bundles.size();
            const dim3 grid(static_cast<unsigned>((tiles + kSweepRays - 1) / kSweepRays),
                            static_cast<unsigned>(pr.singles.size()));
            if (pre_n && f == 0) hipLaunchKernelGGL((sweep_kernel<TS, 16, false, NS, SRC>), grid, dim3(kBlock), 0, st, as);
            else if (pre_n) hipLaunchKernelGGL((sweep_kernel<TS, 17, false, NS, SRC>), grid, dim3(kBlock), 0, st, as);
            else if constexpr (!kVar && !Mode::kHostMedia)                                                   // POLY6 media
                hipLaunchKernelGGL((sweep_kernel<TS, 3, false, NS, SRC>), grid, dim3(kBlock), 0, st, as);
        }
    };
    if (!Mode::kF32 || dtype == RTPB_F64) go(double{});
    else if constexpr (Mode::kF32) go(float{});
    HIP_TRY(hipGetLastError());
    rc = Mode::finish(call, n_groups, tiles, nsurf, st);
    if (rc) return rc;
    return dbuf.release();
}

// Every plan-based entry point: the plan, the mode's dtype rule and checks -- the arguments before the device, so a bad
// call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU -- then the device and the sweep.  kDeviceFirst:
// rtpb_spot_sweep alone looks for the device before its arguments (tests/test_sweep_host.py holds it to that).
template <int NS, int SRC, bool kDeviceFirst = false>
int sweep_entry(const rtpb_plan* plan, int32_t device, int64_t n_groups, const double* group_params,
                const SweepSource& src, const typename SweepHost<NS>::Call& call, void* stream) {
    using Mode = SweepHost<NS>;
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    int rc = RTPB_OK;
    if constexpr (kDeviceFirst) {
        rc = check_device(device);
        if (rc) return rc;
    }
    if constexpr (!Mode::kF32) {
        if (plan->dtype != RTPB_F64) return fail(RTPB_E_INVALID, Mode::template f64_only<SRC>());
    }
    rc = Mode::template check<SRC>(plan->nsurf, n_groups, group_params, src, call);
    if (rc) return rc;
    if constexpr (!kDeviceFirst) {
        rc = check_device(device);
        if (rc) return rc;
    }
    return sweep_impl<NS, SRC>(plan, device, n_groups, group_params, src, call, stream);
}

// The bound the variant calls hold their upload to (RTPB_MAX_VARIANT_UPLOAD), from the counts alone: the tables, per
// group its parameters, media, frame (beams) and at most three index words (a slot in bundles or singles, at most one
// row pair between two groups, its variant), and the descriptors.
inline size_t variant_upload_bound(int src, const SweepSource& s, int64_t n_groups, int32_t nsurf,
                                   int32_t n_variants) {
    const size_t G = size_t(n_groups), S = size_t(nsurf);
    return size_t(s.n_a + s.n_b) * 2 * sizeof(double) +
           G * (4 + 4 * S + 1 + (src == kSrcBeam ? kFrame : 0)) * sizeof(double) +
           size_t(n_variants) * S * sizeof(DevSurface<double>) + 3 * G * sizeof(int32_t);
}

// What the variant calls share before the device is touched (SRC = kSrcFan / kSrcBeam): the checks of the systems'
// arguments, then `own`, the mode's checks of the call's groups, source and outputs, the range of group_variant and
// the upload bound (extra_upload: what the call's mode adds to variant_upload_bound), then each variant through
// rtpb_plan_create's own lowering (plan_fill, plan_surface, device_material) into vc.  `what` names the call in the
// messages.
template <int SRC, typename OwnCheck>
int lower_variant_call(const std::string& what, const rtpb_surface* surfaces, int32_t nsurf,
                       const rtpb_material* materials, int32_t n_variants, int32_t dtype, int64_t n_groups,
                       const int32_t* group_variant, const SweepSource& src, size_t extra_upload, OwnCheck own,
                       VariantCall& vc) {
    if (!surfaces || !materials || !group_variant || nsurf <= 0 || n_variants <= 0)
        return fail(RTPB_E_INVALID, "bad " + what + " arguments");
    if (dtype != RTPB_F64 && dtype != RTPB_F32) return fail(RTPB_E_INVALID, "dtype must be RTPB_F64 or RTPB_F32");
    if (nsurf > RTPB_MAX_SURFACES)
        return fail(RTPB_E_LIMIT, "more than RTPB_MAX_SURFACES (" + std::to_string(RTPB_MAX_SURFACES) + ") surfaces");
    int rc = own();
    if (rc) return rc;
    for (int64_t gi = 0; gi < n_groups; ++gi)
        if (group_variant[gi] < 0 || group_variant[gi] >= n_variants)
            return fail(RTPB_E_INVALID, what + ": group " + std::to_string(gi) + " names variant " +
                                            std::to_string(group_variant[gi]) + " of " + std::to_string(n_variants));
    if (variant_upload_bound(SRC, src, n_groups, nsurf, n_variants) + extra_upload > size_t(RTPB_MAX_VARIANT_UPLOAD))
        return fail(RTPB_E_LIMIT, what + ": the upload (descriptors, media, indices) exceeds "
                                         "RTPB_MAX_VARIANT_UPLOAD; split the call");
    vc.nsurf = nsurf;
    vc.n_variants = n_variants;
    vc.dtype = dtype;
    vc.group_variant = group_variant;
    const size_t S = size_t(nsurf), M = S + 1;
    vc.desc.resize(size_t(n_variants) * S);
    vc.mats.resize(size_t(n_variants) * M);
    vc.tables.resize(size_t(n_variants));
    for (int32_t v = 0; v < n_variants; ++v) {
        rtpb_plan p;
        rc = plan_fill(p, surfaces + size_t(v) * S, nsurf, materials + size_t(v) * M, nsurf + 1, dtype);
        if (rc) return fail(rc, "variant " + std::to_string(v) + ": " + g_last_error);
        for (size_t k = 0; k < M; ++k)
            if (p.mats[k].kind == RTPB_POLY6)
                return fail(RTPB_E_INVALID, "variant " + std::to_string(v) + ", material " + std::to_string(k) +
                                                ": POLY6 media are not host-evaluated; lower it as RTPB_TABLE");
        vc.feat |= p.feat & 1;
        for (size_t k = 0; k < S; ++k) vc.desc[size_t(v) * S + k] = plan_surface(p, k);
        for (size_t k = 0; k < M; ++k) vc.mats[size_t(v) * M + k] = device_material(p, k);
        vc.tables[size_t(v)].swap(p.table);
    }
    return RTPB_OK;
}

// Every variant entry point: the lowering with the mode's checks, the device, the sweep.  dtype: the call's own for the
// focus statistics, RTPB_F64 for the float64 modes.  The mode's block of the upload counts on top of the bound.
template <int NS, int SRC>
int sweep_variants_entry(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                         int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                         const double* group_params, const int32_t* group_variant, const SweepSource& src,
                         const typename SweepHost<NS>::Call& call, void* stream) {
    using Mode = SweepHost<NS>;
    VariantCall vc;
    const size_t extra =
        n_groups > 0 ? (Mode::head_doubles(nsurf) + size_t(n_groups) * Mode::kPerGroup) * sizeof(double) : 0;
    int rc = lower_variant_call<SRC>(
        Mode::kVariantCall, surfaces, nsurf, materials, n_variants, dtype, n_groups, group_variant, src, extra,
        [&] { return Mode::template check<SRC>(nsurf, n_groups, group_params, src, call); }, vc);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<NS, SRC | kSrcVariant>(nullptr, device, n_groups, group_params, src, call, stream, &vc);
}

}  // namespace
