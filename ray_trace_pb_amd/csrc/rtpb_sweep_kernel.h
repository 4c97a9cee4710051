// rtpb_sweep_kernel.h -- the fused spot-diagram / through-focus / spot-image / wavefront sweep:
// generate + trace + reduce in one kernel.  The kernel and its host driver are templates on the SOURCE of a group's
// rays; each source's entry points instantiate them in a translation unit of their own, so the units compile side by
// side: rtpb_sweep.hip (point-source fans: rtpb_spot_sweep, rtpb_focus_sweep, rtpb_image_sweep, rtpb_wavefront_sweep)
// and rtpb_sweep_beam.hip (collimated beams: the same four with _collimated); rtpb_sweep_variants.hip and
// rtpb_sweep_variants_beam.hip hold the focus sweep over many systems (rtpb_focus_sweep_variants[_collimated]),
// rtpb_sweep_wave_variants.hip and rtpb_sweep_wave_variants_beam.hip the wavefront sweep over many systems and the
// final rays of small groups (rtpb_wavefront_sweep_variants[_collimated], rtpb_final_rays_variants[_collimated]);
// rtpb_sweep_foot.hip and rtpb_sweep_foot_beam.hip the footprint sweep (rtpb_footprint_sweep[_collimated]);
// rtpb_sweep_energy.hip and rtpb_sweep_energy_beam.hip the energy sweep (rtpb_energy_sweep[_collimated]);
// rtpb_sweep_wavemap.hip and rtpb_sweep_wavemap_beam.hip the wavefront map sweep
// (rtpb_wavefront_map_sweep[_collimated]).
// What the sweep shares with the plane kernels (the statistics, the image's contribution rule) is rtpb_stats.h, the
// host arithmetic of a call (row planning, media table, upload layout) rtpb_sweep_host.h.
#pragma once

#include "rtpb_stats.h"
#include "rtpb_sweep_host.h"

using namespace rtpbi;

namespace {

// Spot-diagram sweep, fused (C5).  Group g is the fan get_ray_fan(pt_g, ..., wl_g)
// (RT:45-96, same per-ray arithmetic as ray_fan_kernel, angles from the caller's tables); each ray is
// generated in registers, traced through the plan keeping only its final state, and reduced into the
// same 256-ray tile partials as spot_partial_kernel.  spot_final_kernel then produces statistics
// bit-identical to generating, tracing (planes='final') and reducing separately -- without the
// 3 x 64 B per ray of HBM traffic and the launches in between.
//
// Collimated-beam sweep (kSrcBeam).  Group g is the beam get_collimated_rays(pt_g, ..., wl_g, normal_g) (RT:99-161,
// the per-ray arithmetic of collimated_kernel, offsets and angles from the caller's tables): ray k = idisp * nphis +
// iphi, position pt + n1 (off cos phi) + n2 (off sin phi), direction normal, phase 0.  Only the generator differs:
// the index split, the trace and the reductions are the fan's, with the two tables in each other's place -- the
// table indexed by the remainder (the fan's thetas, the beam's phis) first, the one indexed by the quotient second.
//
// Variant sweep (SRC | kSrcVariant; rtpb_focus_sweep_variants, rtpb_wavefront_sweep_variants, rtpb_final_rays_variants
// and their _collimated forms).  Group g traces through the surface descriptors desc + variant[g] * nsurf of the
// call's own upload instead of a plan's blob: many perturbed copies of one system in one launch.  A block row's groups share their variant (plan_sweep_rows keys on it), so the base of a
// block's descriptors is one more block-uniform pointer and every descriptor load stays a scalar load; the kinds and
// geometry codes of a surface may differ from variant to variant.  Host-evaluated media only (FEAT 16 / 17), which
// arrive per group as before.  The flag is folded into SRC, so the instantiations without it are the code they were.
constexpr int kSrcFan = 0, kSrcBeam = 1, kSrcVariant = 2;
constexpr int kFrame = 9;               // a beam's frame: normal, n1, n2
struct SweepImage;
struct SweepWave;
struct SweepFoot;
struct SweepEnergy;
struct SweepMap;
struct SweepArgs {
    const DevSurface<double>* __restrict__ surf;     // the plan's surfaces; variant sweeps: desc [n_variants][nsurf]
    union {
        const DevMaterial<double>* __restrict__ mats;
        // variant sweeps (FEAT bit 4: mats and table are never read): per group, its variant
        const int32_t* __restrict__ variant;
    };
    const double* __restrict__ table;
    // fan: (cos, sin) of the thetas [n_thetas], then of the phis [nphis].  Beam: (cos, sin) of the phis [n_thetas],
    // then the offsets as plain doubles [nphis]
    const double2* __restrict__ tab;
    const double* __restrict__ grp;     // per group: x, y, z, wavelength
    const double* __restrict__ gn;      // FEAT bit 4: per group, n of the S+1 materials at its wavelength, then
                                        // per surface n_s / n_s+1, 1 / n_s+1 and host_rcp_ok(n_s+1) (0 / 1)
    const int32_t* __restrict__ gidx;   // single rows: the group of block row y; bundle rows: see rows
    const int32_t* __restrict__ rows;   // bundle rows: (offset into gidx, number of groups) of block row y
    union {
        double* __restrict__ partials;              // spot and focus statistics; kFinalRays: the rays' rows
        const SweepImage* __restrict__ image;       // image mode
        const SweepWave* __restrict__ wave;         // wavefront mode
        const SweepFoot* __restrict__ foot;         // footprint mode
        const SweepEnergy* __restrict__ energy;     // energy mode
        const SweepMap* __restrict__ map;           // wavefront map mode
    };
    // ray j of a group: j % n_thetas indexes the first table, j / n_thetas the second (the beam's n_thetas is its
    // nphis, its nphis its n_disps)
    int64_t n_thetas, nphis, gsize, tiles;
    union {
        struct {
            double c[3], ex[3], ey[3];                  // fan: the axis and its basis, one for the call
        };
        const double* __restrict__ frm;                 // beam: per group normal, n1, n2 (kFrame doubles)
    };
    int32_t nsurf;
    // j / n_thetas as (j * nt_mul) >> nt_shift for j < 2^31 (nt_mul != 0, see sweep_divisor), else int64 division
    uint32_t nt_mul;
    int32_t nt_shift;
};

// The image mode's outputs: they ride in the sweep's one upload, followed by the groups' windows (SweepLayout::img
// and win), so the kernels' argument block keeps its size and layout and the statistics instantiations stay the
// code they were.
struct SweepImage {
    int32_t* image;      // [n_groups][ny][nx]
    int32_t* outside;    // [n_groups]
    int32_t nx, ny;
};
static_assert(sizeof(SweepImage) % sizeof(double) == 0, "the windows follow it");

// The wavefront mode's block of the upload, in the same place: where the tile partials go, followed by the groups'
// references (kWaveRef doubles each, rtpb_stats.h)
struct SweepWave {
    double* partials;
};
static_assert(sizeof(SweepWave) == sizeof(double), "the references follow it");

// The footprint mode's block of the upload, in the same place: where the block partials go, followed by the surfaces'
// frames (kFootFrame doubles each, rtpb_foot.h) -- one per surface of the plan, not per group
struct SweepFoot {
    double* partials;
};
static_assert(sizeof(SweepFoot) == sizeof(double), "the frames follow it");

// The energy mode's block of the upload, in the same place: the outputs and the number of bins, followed by the
// groups' parameters (4 doubles each: cx, cy, scale, 0; rtpb_stats.h energy_bins)
struct SweepEnergy {
    int32_t* hist;       // [n_groups][2][nr]
    int32_t* outside;    // [n_groups][2]
    double* farthest;    // [n_groups][2]
    int32_t nr, pad;
};
static_assert(sizeof(SweepEnergy) % sizeof(double) == 0, "the parameters follow it");

// The wavefront map mode's block of the upload, in the same place: the outputs and the call's sides, scale and limit,
// followed by the groups' references and windows (kWaveRef + kMapWin doubles each; rtpb_wavemap.h wavemap_ray)
struct SweepMap {
    int32_t* count;      // [n_groups][ny][nx]
    long long* sum;      // [n_groups][ny][nx]
    int32_t* outside;    // [n_groups]
    int32_t* clipped;    // [n_groups]
    double* farthest;    // [n_groups][2]
    double scale, w_lim; // scale = 2^q_bits
    int32_t nx, ny;
};
static_assert(sizeof(SweepMap) % sizeof(double) == 0, "the references and windows follow it");
constexpr int kMapPar = kWaveRef + kMapWin;

template <typename TS>
__device__ __forceinline__ double stored(double v) { return static_cast<double>(static_cast<TS>(v)); }

// kSweepRays rays per lane, traced side by side: each surface runs one surface_step instantiation per ray in one
// straight-line region (inside one run of equal surface codes), so independent dependency chains interleave (two:
// -6 % vs one ray per lane); each ray's 256-ray tile is reduced separately, with the same tree as
// spot_partial_kernel.  Single rows: block b covers tiles kSweepRays*b ... of one group.
// BUNDLE rows (round 5): up to kMaxBundle groups of one field point (a multiple of kSweepRays: 2, 4, 6 or 8) -- the same
// fan at several wavelengths.  Block b covers tile b of every group of the bundle: each lane generates its ray once
// and, when the first surface refracts (Flat / Sphere), runs the part of that surface that does not depend on the
// wavelength once (intersection, normal, front-side and on-surface tests, tangent basis: surface_step_pair's split)
// into LDS; then, kSweepRays groups at a time, it refracts the shared state with each group's Snell ratio
// (snell_apply) and traces those rays side by side through the other surfaces.  A field point's leftover groups run
// in single rows.
#ifndef RTPB_SWEEP_RPL
#define RTPB_SWEEP_RPL 2
#endif
constexpr int kSweepRays = RTPB_SWEEP_RPL;         // rays per lane (tiles per block)
// groups per bundle row: a multiple of kSweepRays (each pass of a row traces kSweepRays of its groups)
constexpr int kMaxBundle = 8 - 8 % kSweepRays;
constexpr int kStateRows = 11;                     // bundle state per lane: x y z, N, c, c . d, N . d

// Occupancy: held to >= 6 waves per SIMD (<= 80 VGPRs).  Round 3 measured 7 best (2.4 % faster than the natural
// 83 VGPRs / 5 waves, experiments/ab_sweep_wpe*.log); with round 4's lens instantiation, fixup-free quotients and
// x x + y y carry the sweep runs 0.379 s at 6, 0.384 s at 7, 0.401 s at 8 (profiles/r04/e/, one process,
// bit-identical); round 5's pair rows: 0.345 s at 6, 0.348 s at 5, 0.353 s at 7 (profiles/r05/g).  Bundle rows hold
// 26 KB of LDS per block (the state, and the reduction two statistics at a time), so 6 blocks fit a CU's 160 KB.
// RTPB_SWEEP_WPE overrides it (A/B builds).
#ifndef RTPB_SWEEP_WPE
#define RTPB_SWEEP_WPE 6
#endif
// The wavefront instantiations run the trace kernel's full step with the phase and the whole direction alive to the
// end: RTPB_WAVE_WPE waves per SIMD for them (the registers, scratch and LDS at each setting)
#ifndef RTPB_WAVE_WPE
#define RTPB_WAVE_WPE 4
#endif
#define RTPB_SWEEP_ATTR(NS)                                                                                      \
    __attribute__((amdgpu_waves_per_eu(                                                                          \
        (NS) == kWaveStats || (NS) == kFinalRays || (NS) == kFootStats || (NS) == kMapStats ? RTPB_WAVE_WPE      \
                                                                                             : RTPB_SWEEP_WPE,   \
        8)))
// An optimisation fence on three per-lane values: the compiler moves no computation on them across it
#if defined(__HIP_DEVICE_COMPILE__)
#define RTPB_PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))
#else
#define RTPB_PIN3(a, b, c) ((void)0)
#endif
// NS = kStats: the spot statistics.  NS = kFocusStats (rtpb_focus_sweep): focus_ray of the final state, so the whole
// final direction stays alive to the end.  kPosOnly leaves no part of it unfinished on any surface kind -- snell_apply,
// reflect and lens_step compute dx, dy and dz in full whatever the mode, and a killed row is all NaN (the mode only
// skips the position fill after a NaN direction and the at-plane) -- so the last surface runs the same step as the
// others.  Single rows reduce eight of the sixteen statistics at a time (16 KB of LDS), bundle rows two as before.
// NS = kImageStats (rtpb_image_sweep): no statistics, each counted ray goes into its group's image instead
// (image_bin, wave_image_add); the rule of which rays count is the spot statistics', and there are no red tiles.
// NS = kWaveStats (rtpb_wavefront_sweep; float64, single rows only): wave_ray of the final state against the group's
// reference.  The phase is wanted, so the steps are the final-plane trace kernel's (kNoAt: the full semantics of
// every surface, its roots and square roots included, and no carried x x + y y) and the final state is the one
// rtpb_trace stores, phase and all; eight of the fifteen statistics at a time.
constexpr int kImageStats = 0;
// NS = kEnergyStats (rtpb_energy_sweep; the value is the mode's tag, the two curves): the image mode with another rule
// per ray -- each counted ray goes into its group's circle and square histograms and into the two maxima
// (energy_bins, wave_energy_add).  Everything else is the image mode's: which rays count, the kPosOnly steps, single
// and bundle rows, both storage types, the occupancy class, no red tiles.
constexpr int kEnergyStats = 2;
// NS = kMapStats (rtpb_wavefront_map_sweep; float64, single rows only, no variants; the value is the mode's tag): the
// wavefront mode's steps -- kPhase, the kNoAt full semantics, its occupancy class -- with the counter modes' ending:
// no red tiles and no workspace, each ray's final state goes through wave_ray and wavemap_ray into its group's map
// (wave_map_add), the dead-row and past-the-group lanes as to_image / to_energy handle them.
constexpr int kMapStats = 4;
// NS = kFinalRays (rtpb_final_rays_variants; variants, float64, single rows, groups of at most one tile): no
// reduction, each ray's final state goes to rays_out[group][ray] as the row rtpb_trace stores for the final plane (a
// killed ray's NaN pattern included), so the steps are the wavefront mode's.  Lanes past the group's size store nothing.
constexpr int kFinalRays = 8;
// NS = kFootStats (rtpb_footprint_sweep; float64, single rows only, no variants; the value is the mode's tag, its
// columns are kFootCols): the footprint statistics of EVERY surface (rtpb_foot.h).  They are defined on the history's
// "at" and "after" planes, so the steps are the history kernel's (mode 0: the at-plane formed and handed to emit_at,
// which keeps its position; the TIR fill; no carried x x + y y).  After each surface the lane's rays are combined
// (foot_ray, foot_merge; lanes past the group's size and rays whose tile lies past the group's tiles contribute
// nothing), then the wave's lanes (foot_wave_reduce), and lane 0 of each wave writes the wave's row of that surface
// into the block's LDS table -- its own row, so the surface loop holds no barrier.  After the loop one barrier, and the
// block's threads combine the four waves' rows and store them as the block's partial [group][block][surface][8];
// foot_final_kernel (rtpb_footprint.hip) combines a group's blocks.  nsurf <= RTPB_MAX_SURFACES, the plans' bound.
constexpr int kFootStats = 32;
// SRC = kSrcBeam: the generator of a collimated beam; a bundle row's groups share the beam (pt and frame) as the
// fan's share the field point, and everything after the generator is the same code.
template <typename TS, int FEAT, bool BUNDLE, int NS = kStats, int SRC = kSrcFan>
__global__ __launch_bounds__(kBlock) RTPB_SWEEP_ATTR(NS) void sweep_kernel(SweepArgs a) {
    constexpr int kGen = SRC & ~kSrcVariant;
    constexpr bool kVar = (SRC & kSrcVariant) != 0;
    static_assert(kGen == kSrcFan || kGen == kSrcBeam, "a fan or a beam");
    static_assert(!kVar || ((NS == kFocusStats || NS == kWaveStats || NS == kFinalRays) && (FEAT & 16) != 0 &&
                            (FEAT & 2) == 0),
                  "variants: the focus or wavefront statistics or the final rays, host-evaluated media");
    static_assert(!BUNDLE || (FEAT & 16) != 0, "bundles: host-evaluated media");
    static_assert(NS == kStats || NS == kFocusStats || NS == kImageStats || NS == kWaveStats || NS == kFinalRays ||
                      NS == kFootStats || NS == kEnergyStats || NS == kMapStats,
                  "spot, focus, wavefront or footprint statistics, the image, the energy curves, the wavefront map, or "
                  "the final rays");
    constexpr bool kFoot = NS == kFootStats;
    static_assert(!kFoot || (!kVar && !BUNDLE && sizeof(TS) == 8), "footprints: float64, single rows, no variants");
    constexpr bool kWave = NS == kWaveStats;
    static_assert(!kWave || (!BUNDLE && sizeof(TS) == 8), "wavefront: float64, single rows");
    constexpr bool kRays = NS == kFinalRays;
    static_assert(!kRays || (kVar && !BUNDLE && sizeof(TS) == 8), "final rays: variants, float64, single rows");
    constexpr bool kMap = NS == kMapStats;
    static_assert(!kMap || (!kVar && !BUNDLE && sizeof(TS) == 8), "wavefront map: float64, single rows, no variants");
    constexpr bool kPhase = kWave || kRays || kMap;  // the trace kernel's full steps, the phase kept
    constexpr bool kCounts = NS == kImageStats || NS == kEnergyStats || kMap;     // integer counters, no statistics
    constexpr int kRedRows = kCounts || kRays || kFoot ? 1 : BUNDLE ? 2 : NS == kStats ? kStats : 8;
    __shared__ double red[kRedRows][kBlock];
    __shared__ double state[BUNDLE ? kStateRows : 1][kBlock];
    // footprints: per wave, one row per surface (16 KB)
    double (*foot_tab)[RTPB_MAX_SURFACES][kFootCols] = nullptr;
    if constexpr (kFoot) {
        __shared__ double foot_lds[kBlock / 64][RTPB_MAX_SURFACES][kFootCols];
        foot_tab = foot_lds;
    }
    const int tid = threadIdx.x;
    auto gen = [&](int64_t j, int64_t g) {
        const double* gp = a.grp + 4 * g;
        const int64_t jj = j < a.gsize ? j : 0;
        int64_t it, ip;
        if (a.nt_mul != 0) {
            const uint32_t x = static_cast<uint32_t>(jj);
            const uint32_t qt = static_cast<uint32_t>((uint64_t(x) * a.nt_mul) >> a.nt_shift);
            ip = qt;
            it = x - qt * static_cast<uint32_t>(a.n_thetas);
        } else {
            it = jj % a.n_thetas;
            ip = jj / a.n_thetas;
        }
        Ray<double> r;
        if constexpr (kGen == kSrcBeam) {
            // collimated_kernel's products in its association; the frame is the block's, so scalar loads
            const double* fr = a.frm + kFrame * g;
            const double2 ph = a.tab[it];
            const double oo = reinterpret_cast<const double*>(a.tab + a.n_thetas)[ip];
            const double oc = oo * ph.x, os = oo * ph.y;
            r.x = stored<TS>(gp[0] + fr[3] * oc + fr[6] * os);
            r.y = stored<TS>(gp[1] + fr[4] * oc + fr[7] * os);
            r.z = stored<TS>(gp[2] + fr[5] * oc + fr[8] * os);
            r.dx = stored<TS>(fr[0]); r.dy = stored<TS>(fr[1]); r.dz = stored<TS>(fr[2]);
        } else {
            const double2 t = a.tab[it], ph = a.tab[a.n_thetas + ip];
            const double ct = t.x, st = t.y, cp = ph.x, sp = ph.y;
            r.x = stored<TS>(gp[0]); r.y = stored<TS>(gp[1]); r.z = stored<TS>(gp[2]);
            r.dx = stored<TS>(a.c[0] * ct + a.ex[0] * cp * st + a.ey[0] * sp * st);
            r.dy = stored<TS>(a.c[1] * ct + a.ex[1] * cp * st + a.ey[1] * sp * st);
            r.dz = stored<TS>(a.c[2] * ct + a.ex[2] * cp * st + a.ey[2] * sp * st);
        }
        r.ph = 0.0;
        r.wl = stored<TS>(gp[3]);
        return r;
    };
    cptr<DevSurface<double>> surf = (cptr<DevSurface<double>>)(a.surf);
    if constexpr (kVar) {
        // the block row's variant: that of its first group (a bundle row's groups share it)
        const int32_t g0 = BUNDLE ? a.gidx[a.rows[2 * blockIdx.y]] : a.gidx[blockIdx.y];
        surf += int64_t(((cptr<int32_t>)(a.variant))[g0]) * a.nsurf;
    }
    const cptr<DevMaterial<double>> mats = (cptr<DevMaterial<double>>)(a.mats);
    const cptr<double> table = (cptr<double>)(a.table);
    int64_t grp[kSweepRays], tile[kSweepRays];
    Ray<double> r[kSweepRays];
    // one wavelength per group: with FEAT bit 4 the host has evaluated every material at it (the kernel's own
    // material_n, see rtpb_spot_sweep) and the values arrive as scalar loads; without it (single rows only) every ray
    // of the block has the group's wavelength, so the per-wavelength values of ray 0 serve both
    Rcp<double> iwl[kSweepRays];
    cptr<double> gn[kSweepRays];
    double n_cur[kSweepRays];
    // the group's wavelength (not r[0].wl: a row kill fills the ray's wavelength with NaN too, and the single rows'
    // second ray takes ray 0's n)
    double wl0 = 0.0;
    auto mat_n = [&](int q, int k) -> double {
        if constexpr ((FEAT & 16) != 0) return gn[q][k];
        else return material_n<double, (FEAT & 2) != 0>(load_material<double>(mats + k), wl0, table);
    };
    // the surface's descriptor for ray q: with host-evaluated media, the Snell ratio and 1 / n2 of q's group (IEEE
    // division on the host)
    auto surface_for = [&](int q, int k, const DevSurface<double>& base) {
        DevSurface<double> sd = base;
        if constexpr ((FEAT & 16) != 0) {
            sd.nr = gn[q][a.nsurf + 1 + k];
            sd.rn2 = gn[q][2 * a.nsurf + 1 + k];
            sd.rcp_ok = (sd.rcp_ok & ~(4 | 8)) | 4 | (gn[q][3 * a.nsurf + 1 + k] != 0.0 ? 8 : 0);
        }
        return sd;
    };
    auto code_of = [&](int k) { return surface_code<double>((surf + k)->kind, (surf + k)->rcp_ok); };
    constexpr int kMode = (kFoot ? 0 : kPhase ? kNoAt : kPosOnly) | ((FEAT & 16) != 0 ? kUniMedia : 0);
    // the statistics read only the final positions: the steps run with kPosOnly semantics (no TIR fill of the
    // position -- the next surface's intersection makes it NaN, and the final plane gets the rule in reduce), and a
    // run of axial spheres carries x x + y y of each intersection point into the next sphere's quadratic.
    // Runs of consecutive surfaces of one (kind, axial) code: each run loops inside one instantiation of the surface
    // step, so the rays' registers carry from surface to surface without the copies a per-surface join of the kind
    // branches needs (the ODT path of C5: 12 axial spheres, a lens, a flat = 3 runs).
    double rxy[kSweepRays];
    bool live[kSweepRays];              // footprints: the lane's ray q is one of its group's
    auto trace_from = [&](int s) {
        while (s < a.nsurf) {
            const int code = code_of(s);
            dispatch_code<(FEAT & 1) != 0>(code, [&](auto kind, auto geo) {
                constexpr int K = decltype(kind)::value;
                constexpr int A = decltype(geo)::value;
                constexpr bool kCarry = K == SPHERE && A == kGeoAxial && !kPhase && !kFoot;
                if constexpr (kCarry) {
#pragma unroll
                    for (int q = 0; q < kSweepRays; ++q) rxy[q] = r[q].x * r[q].x + r[q].y * r[q].y;
                }
                do {
                    const DevSurface<double> base = load_surface<double>(surf + s);
                    double n_next[kSweepRays];
#pragma unroll
                    for (int q = 0; q < kSweepRays; ++q) n_next[q] = (BUNDLE || q == 0) ? mat_n(q, s + 1) : n_next[0];
                    auto none = [](const Ray<double>&) {};
                    Ray<double> o[kSweepRays];
                    [[maybe_unused]] double at[kSweepRays][3];
#pragma unroll
                    for (int q = 0; q < kSweepRays; ++q) {
                        const DevSurface<double> sd = (BUNDLE || q == 0) ? surface_for(q, s, base)
                                                                         : surface_for(0, s, base);
                        if constexpr (kFoot) {
                            auto keep = [&](const Ray<double>& p) {
                                at[q][0] = p.x; at[q][1] = p.y; at[q][2] = p.z;
                            };
                            surface_step<double, K, A, kMode>(sd, r[q], n_cur[q], n_next[q], iwl[q], keep, o[q],
                                                              static_cast<GuardBranch*>(nullptr));
                        } else {
                            surface_step<double, K, A, kMode>(sd, r[q], n_cur[q], n_next[q], iwl[q], none, o[q],
                                                              static_cast<GuardBranch*>(nullptr),
                                                              kCarry ? &rxy[q] : nullptr);
                        }
                    }
                    if constexpr (kFoot) {
                        // the surface's frame: the block's, so scalar loads
                        const cptr<double> fp = (cptr<double>)(a.foot + 1) + kFootFrame * s;
                        const double fr[kFootFrame] = {fp[0], fp[1], fp[2], fp[3], fp[4], fp[5], fp[6], fp[7], fp[8]};
                        FootRay acc = foot_none();
#pragma unroll
                        for (int q = 0; q < kSweepRays; ++q) {
                            if (live[q])
                                foot_merge(acc, foot_ray(at[q][0], at[q][1], at[q][2], o[q].x, o[q].y, o[q].z, fr));
                        }
                        foot_wave_reduce(acc);
                        if ((tid & 63) == 0) {
#pragma unroll
                            for (int c = 0; c < kFootCols; ++c) foot_tab[tid >> 6][s][c] = acc.v[c];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < kSweepRays; ++q) {
                        r[q] = o[q];
                        n_cur[q] = n_next[q];
                    }
                    ++s;
                } while (s < a.nsurf && code_of(s) == code);
            });
        }
    };
    // one ray's contribution to its group's tile partial: spot_partial_kernel's tree (block_tree_sum), kRedRows
    // statistics at a time
    auto reduce = [&](const Ray<double>& rr, bool ok, int64_t g, int64_t t) {
        double v[kStats] = {};
        FocusRay f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        WaveRay wv{0.0, 0.0, 0.0, 0.0, 0.0};
        double* out;
        if constexpr (kWave) out = ((cptr<SweepWave>)(a.wave))->partials;
        else out = a.partials;
        // the reference's position rule of the last surface (RT:1221 / RT:1289; a PerfectLens's after-plane
        // propagation gives a NaN position for a NaN direction by itself): NaN direction -> no spot point
        if (ok && !is_nan(rr.dx)) {
            const double x = stored<TS>(rr.x), y = stored<TS>(rr.y), z = stored<TS>(rr.z);
            if constexpr (NS == kStats) {
                if (x - x == 0.0 && y - y == 0.0) {
                    v[0] = 1.0; v[1] = x; v[2] = y; v[3] = z; v[4] = x * x; v[5] = y * y; v[6] = x * y;
                }
            } else if constexpr (kWave) {
                const cptr<double> q = (cptr<double>)(a.wave + 1) + kWaveRef * g;
                const double ref[kWaveRef] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
                wv = wave_ray(x, y, z, rr.dx, rr.dy, rr.dz, rr.ph, ref);
            } else {
                double dx = stored<TS>(rr.dx), dy = stored<TS>(rr.dy), dz = stored<TS>(rr.dz);
                // the slopes' divisions stay behind the trace: without the fence the float64 instantiations spill
                // inside the surface loops (FEAT 17 single rows: 20 spilled VGPRs instead of the spot kernel's 1)
                RTPB_PIN3(dx, dy, dz);
                f = focus_ray(x, y, z, dx, dy, dz);
            }
        }
#pragma unroll
        for (int k0 = 0; k0 < NS; k0 += kRedRows) {
            double u[kRedRows];
#pragma unroll
            for (int j = 0; j < kRedRows; ++j) {
                if constexpr (NS == kStats) u[j] = k0 + j < NS ? v[k0 + j] : 0.0;
                else if constexpr (kWave) u[j] = wave_term(wv, k0 + j);
                else u[j] = focus_term(f, k0 + j);
            }
            block_tree_sum<kRedRows>(u, red);
            if (tid == 0 && t < a.tiles) {
#pragma unroll
                for (int j = 0; j < kRedRows; ++j)
                    if (k0 + j < NS) out[(g * a.tiles + t) * NS + k0 + j] = u[j];
            }
        }
    };
    // the image mode's counterpart: one ray's contribution to its group's image, by the same rule of the last
    // surface; every lane reaches the wave's adds, and g is the same in the whole block
    auto to_image = [&](const Ray<double>& rr, bool ok, int64_t g) {
        const cptr<SweepImage> im = (cptr<SweepImage>)(a.image);
        const cptr<double> win = (cptr<double>)(a.image + 1) + 4 * g;
        const int nx = im->nx, ny = im->ny;
        int bin = kImageSkip;
        if (ok && !is_nan(rr.dx)) {
            const double w[4] = {win[0], win[1], win[2], win[3]};
            bin = image_bin(stored<TS>(rr.x), stored<TS>(rr.y), w, nx, ny);
        }
        wave_image_add(bin, im->image + g * ny * nx, im->outside + g);
    };
    // ... and the energy mode's, by the same rule
    auto to_energy = [&](const Ray<double>& rr, bool ok, int64_t g) {
        const cptr<SweepEnergy> en = (cptr<SweepEnergy>)(a.energy);
        const cptr<double> par = (cptr<double>)(a.energy + 1) + 4 * g;
        const int nr = en->nr;
        EnergyRay e{{kImageSkip, kImageSkip}, {0.0, 0.0}};
        if (ok && !is_nan(rr.dx)) {
            const double p[4] = {par[0], par[1], par[2], par[3]};
            e = energy_bins(stored<TS>(rr.x), stored<TS>(rr.y), p, nr);
        }
        wave_energy_add(e, nr, en->hist + g * 2 * nr, en->outside + 2 * g, en->farthest + 2 * g);
    };
    // ... and the wavefront map mode's: reduce's rule of which final states reach wave_ray, then the map's own
    auto to_map = [&](const Ray<double>& rr, bool ok, int64_t g) {
        const cptr<SweepMap> mp = (cptr<SweepMap>)(a.map);
        const cptr<double> q = (cptr<double>)(a.map + 1) + kMapPar * g;
        const int nx = mp->nx, ny = mp->ny;
        MapRay m{kImageSkip, 0, 0.0, 0.0};
        if (ok && !is_nan(rr.dx)) {
            const double ref[kWaveRef] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
            const double win[kMapWin] = {q[8], q[9], q[10], q[11]};
            m = wavemap_ray(wave_ray(rr.x, rr.y, rr.z, rr.dx, rr.dy, rr.dz, rr.ph, ref), win, nx, ny, mp->scale,
                            mp->w_lim);
        }
        const int64_t cells = int64_t(ny) * nx;
        wave_map_add(m, mp->count + g * cells, mp->sum + g * cells, mp->outside + g, mp->clipped + g,
                     mp->farthest + 2 * g);
    };
    if constexpr (!BUNDLE) {
#pragma unroll
        for (int q = 0; q < kSweepRays; ++q) {
            grp[q] = a.gidx[blockIdx.y];
            tile[q] = kSweepRays * int64_t(blockIdx.x) + q;
            r[q] = gen(tile[q] * kBlock + tid, grp[q]);
            // a beam's positions are complete before the trace begins: without the fence the PerfectLens single rows
            // spill 12 VGPRs instead of the fan's 1
            if constexpr (kGen == kSrcBeam) RTPB_PIN3(r[q].x, r[q].y, r[q].z);
        }
        wl0 = r[0].wl;
#pragma unroll
        for (int q = 0; q < kSweepRays; ++q) {
            iwl[q] = q == 0 ? make_wl_rcp(r[0].wl) : iwl[0];   // every phase update's divisor, 2 pi / wl
            gn[q] = (cptr<double>)(a.gn) + grp[q] * (4 * a.nsurf + 1);
        }
#pragma unroll
        for (int q = 0; q < kSweepRays; ++q) n_cur[q] = q == 0 ? mat_n(0, 0) : n_cur[0];
        if constexpr (kFoot) {
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) live[q] = tile[q] * kBlock + tid < a.gsize;
        }
        trace_from(0);
        if constexpr (kFoot) {
            // the block's partial: the four waves' rows combined, [group][block][surface][kFootCols]
            __syncthreads();
            double* out = ((cptr<SweepFoot>)(a.foot))->partials +
                          (grp[0] * int64_t(gridDim.x) + blockIdx.x) * a.nsurf * kFootCols;
            for (int k = tid; k < a.nsurf * kFootCols; k += kBlock) {
                const int s = k / kFootCols, c = k % kFootCols;
                double v = foot_tab[0][s][c];
#pragma unroll
                for (int w = 1; w < kBlock / 64; ++w) v = foot_col(c, v, foot_tab[w][s][c]);
                out[k] = v;
            }
            return;
        }
#pragma unroll
        for (int q = 0; q < kSweepRays; ++q) {
            if constexpr (NS == kImageStats) {
                to_image(r[q], tile[q] * kBlock + tid < a.gsize, grp[q]);
            } else if constexpr (NS == kEnergyStats) {
                to_energy(r[q], tile[q] * kBlock + tid < a.gsize, grp[q]);
            } else if constexpr (kMap) {
                to_map(r[q], tile[q] * kBlock + tid < a.gsize, grp[q]);
            } else if constexpr (kRays) {
                // a plain per-lane store of the row (four 16-byte stores), inside the group's own rows only
                const int64_t j = tile[q] * kBlock + tid;
                if (j < a.gsize) store_ray<double, RTPB_AOS>(a.partials, grp[q] * a.gsize + j, 0, r[q]);
            } else {
                reduce(r[q], tile[q] * kBlock + tid < a.gsize, grp[q], tile[q]);
            }
        }
    } else {
        const int32_t off = a.rows[2 * blockIdx.y], nb = a.rows[2 * blockIdx.y + 1];
        const int64_t t0 = blockIdx.x;
        const Ray<double> rg = gen(t0 * kBlock + tid, int64_t(a.gidx[off]));
        wl0 = rg.wl;
        const int code0 = a.nsurf > 0 ? code_of(0) : -1;
        using std::integral_constant;
        // fn(kind, geo) on the first surface's code when it is a refracting Flat / Sphere; false otherwise
        auto on_first = [&](auto&& fn) {
            if (code0 == 3 * SPHERE + kGeoAxial) fn(integral_constant<int, SPHERE>(), integral_constant<int, kGeoAxial>());
            else if (code0 == 3 * SPHERE) fn(integral_constant<int, SPHERE>(), integral_constant<int, kGeoGeneral>());
            else if (code0 == 3 * FLAT + kGeoAxial) fn(integral_constant<int, FLAT>(), integral_constant<int, kGeoAxial>());
            else if (code0 == 3 * FLAT + kGeoXZ) fn(integral_constant<int, FLAT>(), integral_constant<int, kGeoXZ>());
            else if (code0 == 3 * FLAT) fn(integral_constant<int, FLAT>(), integral_constant<int, kGeoGeneral>());
            else return false;
            return true;
        };
        // the shared part of the first surface (surface_step_pair): a row that fails the front-side or on-surface
        // test stores a NaN position and c . d, so each refraction of it is all NaN (as the step's kill)
        const bool shared = on_first([&](auto kind, auto geo) {
            constexpr int K = decltype(kind)::value;
            constexpr int A = decltype(geo)::value;
            const DevSurface<double> base = load_surface<double>(surf);
            const Rcp<double> iwl0 = make_wl_rcp(rg.wl);     // (the phase, and with it n1 and iwl0, is not kept)
            double rxy0 = rg.x * rg.x + rg.y * rg.y;
            double Nx, Ny, Nz;
            Ray<double> ri;
            bool fwd = true;
            hit_and_normal<double, K, A>(base, rg, 1.0, iwl0, static_cast<GuardBranch*>(nullptr),
                                         K == SPHERE && A == kGeoAxial ? &rxy0 : nullptr, ri, Nx, Ny, Nz, &fwd);
            const bool front_ok = !front_side_fails<A, true>(rg, base) && fwd;
            constexpr int kBasis = K == FLAT ? A : kGeoGeneral;
            const SnellBasis<double> b = snell_basis<kBasis>(ri, Nx, Ny, Nz, static_cast<GuardBranch*>(nullptr));
            bool ok;
            if constexpr (K == SPHERE) ok = on_sphere<A == kGeoAxial>(ri, base, A == kGeoAxial ? &rxy0 : nullptr) && front_ok;
            else ok = on_flat<A>(ri, base) && front_ok;
            double px = ri.x, py = ri.y, pz = ri.z, cd = b.cd;
            if (!ok) px = py = pz = cd = qnan<double>();
            state[0][tid] = px; state[1][tid] = py; state[2][tid] = pz;
            state[3][tid] = Nx; state[4][tid] = Ny; state[5][tid] = Nz;
            state[6][tid] = b.cx; state[7][tid] = b.cy; state[8][tid] = b.cz;
            state[9][tid] = cd; state[10][tid] = b.nd;
        });
        if (!shared) {
            state[0][tid] = rg.x; state[1][tid] = rg.y; state[2][tid] = rg.z;
            state[3][tid] = rg.dx; state[4][tid] = rg.dy; state[5][tid] = rg.dz;
        }
        for (int p = 0; p < nb; p += kSweepRays) {
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) {
                grp[q] = a.gidx[off + p + q];
                tile[q] = t0;
                gn[q] = (cptr<double>)(a.gn) + grp[q] * (4 * a.nsurf + 1);
                r[q].ph = 0.0;
                r[q].wl = stored<TS>(a.grp[4 * grp[q] + 3]);
            }
            int s0 = 0;
            const bool first = on_first([&](auto kind, auto geo) {
                constexpr int kBasis = decltype(kind)::value == FLAT ? decltype(geo)::value : kGeoGeneral;
                Ray<double> ri;
                ri.x = state[0][tid]; ri.y = state[1][tid]; ri.z = state[2][tid];
                ri.dx = ri.dy = ri.dz = 0.0;
                ri.ph = 0.0;
                const double Nx = state[3][tid], Ny = state[4][tid], Nz = state[5][tid];
                SnellBasis<double> b;
                b.cx = state[6][tid]; b.cy = state[7][tid]; b.cz = state[8][tid];
                b.cd = state[9][tid]; b.nd = state[10][tid];
#pragma unroll
                for (int q = 0; q < kSweepRays; ++q) {
                    ri.wl = r[q].wl;
                    r[q] = snell_apply<kBasis, false>(ri, Nx, Ny, Nz, b, gn[q][a.nsurf + 1],
                                                        static_cast<GuardBranch*>(nullptr));
                }
            });
            if (first) {
                s0 = 1;
            } else {
#pragma unroll
                for (int q = 0; q < kSweepRays; ++q) {
                    r[q].x = state[0][tid]; r[q].y = state[1][tid]; r[q].z = state[2][tid];
                    r[q].dx = state[3][tid]; r[q].dy = state[4][tid]; r[q].dz = state[5][tid];
                }
            }
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) {
                iwl[q] = make_wl_rcp(r[q].wl);
                n_cur[q] = mat_n(q, s0);
            }
            trace_from(s0);
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) {
                if constexpr (NS == kImageStats) to_image(r[q], t0 * kBlock + tid < a.gsize, grp[q]);
                else if constexpr (NS == kEnergyStats) to_energy(r[q], t0 * kBlock + tid < a.gsize, grp[q]);
                else reduce(r[q], t0 * kBlock + tid < a.gsize, grp[q], t0);
            }
        }
    }
}

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
};

inline SweepSource fan_source(int64_t n_thetas, int64_t nphis, const double* center_ray, const double* ex,
                              const double* ey, const double* theta_cos_sin, const double* phi_cos_sin) {
    return SweepSource{n_thetas, nphis, theta_cos_sin, phi_cos_sin, center_ray, ex, ey, nullptr};
}

inline SweepSource beam_source(const double* group_frames, int64_t n_disps, int64_t nphis, const double* offsets,
                               const double* phi_cos_sin) {
    return SweepSource{nphis, n_disps, phi_cos_sin, offsets, nullptr, nullptr, nullptr, group_frames};
}

// rtpb_spot_sweep (NS = kStats), rtpb_focus_sweep (NS = kFocusStats) and rtpb_wavefront_sweep (NS = kWaveStats), and
// their _collimated counterparts (SRC = kSrcBeam): the argument checks ...
template <int NS, int SRC = kSrcFan>
int sweep_check(int64_t n_groups, const double* group_params, const SweepSource& s, double* workspace,
                int64_t workspace_len, double* stats_out) {
    constexpr bool kFocus = NS == kFocusStats, kWave = NS == kWaveStats;
    if (n_groups <= 0 || !s.complete(SRC) || !group_params || !workspace || !stats_out)
        return fail(RTPB_E_INVALID, kWave    ? "bad wavefront-sweep arguments"
                                    : kFocus ? "bad focus-sweep arguments"
                                             : "bad spot-sweep arguments");
    const int64_t tiles = (s.n_a * s.n_b + kBlock - 1) / kBlock;
    if (workspace_len < n_groups * tiles * NS)
        return fail(RTPB_E_INVALID,
                    SRC == kSrcBeam
                        ? (kWave    ? "workspace too small: need n_groups * ceil(n_disps*nphis/256) * 15 doubles"
                           : kFocus ? "workspace too small: need n_groups * ceil(n_disps*nphis/256) * 16 doubles"
                                    : "workspace too small: need n_groups * ceil(n_disps*nphis/256) * 7 doubles")
                    : kWave  ? "workspace too small: need n_groups * ceil(n_thetas*nphis/256) * 15 doubles"
                    : kFocus ? "workspace too small: need n_groups * ceil(n_thetas*nphis/256) * 16 doubles"
                             : "workspace too small: need n_groups * ceil(n_thetas*nphis/256) * 7 doubles");
    if (tiles > 0x7fffffffll || n_groups > 65535) return fail(RTPB_E_LIMIT, "too many groups or rays per group");
    return RTPB_OK;
}

// ... those of the image sweeps (no workspace, no statistics; `what` names the call in the messages) ...
template <int SRC = kSrcFan>
int image_sweep_check(const char* what, const char* too_many, int64_t n_groups, const double* group_params,
                      const SweepSource& s, const double* windows, int32_t nx, int32_t ny, int32_t* image_out,
                      int32_t* outside_out) {
    if (n_groups <= 0 || !s.complete(SRC) || !group_params)
        return fail(RTPB_E_INVALID, SRC == kSrcBeam ? "bad image-sweep-collimated arguments"
                                                    : "bad image-sweep arguments");
    // (n_a * n_b: a product past int64 is past the limit too)
    const int64_t gsize = s.n_a > 0x7fffffffll / s.n_b ? 0x80000000ll : s.n_a * s.n_b;
    int rc = image_check(what, nx, ny, gsize, n_groups, windows, image_out, outside_out);
    if (rc) return rc;
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, too_many);
    return RTPB_OK;
}

// ... those of the final-rays calls (NS = kFinalRays: no workspace; one tile of rays per group at the most) ...
template <int SRC>
int final_rays_check(int64_t n_groups, const double* group_params, const SweepSource& s, const double* rays_out) {
    if (n_groups <= 0 || !s.complete(SRC) || !group_params || !rays_out)
        return fail(RTPB_E_INVALID, "bad final-rays arguments");
    if (s.n_a > kBlock || s.n_b > kBlock || s.n_a * s.n_b > kBlock)
        return fail(RTPB_E_LIMIT, SRC == kSrcBeam ? "final-rays: more than 256 rays per group (n_disps*nphis)"
                                                  : "final-rays: more than 256 rays per group (n_thetas*nphis)");
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, "too many groups or rays per group");
    return RTPB_OK;
}

// ... those of the footprint sweeps (NS = kFootStats: float64 plans, one finite frame per surface of the plan, a
// workspace of one partial per block of two tiles) ...
template <int SRC>
int foot_sweep_check(const rtpb_plan* plan, int64_t n_groups, const double* group_params, const SweepSource& s,
                     const double* frames, int32_t n_frames, double* workspace, int64_t workspace_len,
                     double* stats_out) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    if (plan->dtype != RTPB_F64)
        return fail(RTPB_E_INVALID, "footprint-sweep: float64 plans only (the statistics are defined on the float64 "
                                    "history)");
    if (n_groups <= 0 || !s.complete(SRC) || !group_params || !frames || !workspace || !stats_out)
        return fail(RTPB_E_INVALID, "bad footprint-sweep arguments");
    if (n_frames != plan->nsurf)
        return fail(RTPB_E_INVALID, "footprint-sweep: n_frames (" + std::to_string(n_frames) +
                                        ") is not the plan's number of surfaces (" + std::to_string(plan->nsurf) + ")");
    for (int64_t k = 0; k < int64_t(n_frames) * kFootFrame; ++k)
        if (!(frames[k] - frames[k] == 0.0))
            return fail(RTPB_E_INVALID, "footprint-sweep: frame " + std::to_string(k / kFootFrame) + " is not finite");
    if (plan->nsurf > RTPB_MAX_SURFACES)
        return fail(RTPB_E_LIMIT, "footprint-sweep: more than RTPB_MAX_SURFACES surfaces");
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, "footprint-sweep: too many groups or rays per group");
    // (n_a * n_b: a product past int64 is past the limit too)
    if (s.n_a > (0x7fffffffll * kBlock) / s.n_b)
        return fail(RTPB_E_LIMIT, "footprint-sweep: too many groups or rays per group");
    const int64_t tiles = (s.n_a * s.n_b + kBlock - 1) / kBlock;
    const int64_t blocks = (tiles + kSweepRays - 1) / kSweepRays;
    if (workspace_len / (int64_t(n_frames) * kFootCols) / blocks < n_groups)
        return fail(RTPB_E_INVALID,
                    SRC == kSrcBeam ? "footprint-sweep: workspace too small: need n_groups * ceil(ceil(n_disps*nphis"
                                      "/256)/2) * nsurf * 8 doubles"
                                    : "footprint-sweep: workspace too small: need n_groups * ceil(ceil(n_thetas*nphis"
                                      "/256)/2) * nsurf * 8 doubles");
    return RTPB_OK;
}

// rtpb_image_sweep's own arguments (NS = kImageStats: no workspace, no statistics)
struct ImageCall {
    const double* windows;      // host, n_groups x 4
    int32_t nx, ny;
    int32_t* image_out;
    int32_t* outside_out;
};

// ... those of the energy sweeps (no workspace, no statistics; `what` names the call in the messages) ...
template <int SRC = kSrcFan>
int energy_sweep_check(const char* what, const char* too_many, int64_t n_groups, const double* group_params,
                       const SweepSource& s, const double* params, int32_t nr, int32_t* hist_out,
                       int32_t* outside_out, double* farthest_out) {
    if (n_groups <= 0 || !s.complete(SRC) || !group_params)
        return fail(RTPB_E_INVALID, SRC == kSrcBeam ? "bad energy-sweep-collimated arguments"
                                                    : "bad energy-sweep arguments");
    // (n_a * n_b: a product past int64 is past the limit too)
    const int64_t gsize = s.n_a > 0x7fffffffll / s.n_b ? 0x80000000ll : s.n_a * s.n_b;
    int rc = energy_check(what, nr, gsize, n_groups, params, hist_out, outside_out, farthest_out);
    if (rc) return rc;
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, too_many);
    return RTPB_OK;
}

// rtpb_energy_sweep's own arguments (NS = kEnergyStats: no workspace, no statistics)
struct EnergyCall {
    const double* params;       // host, n_groups x 4
    int32_t nr;
    int32_t* hist_out;
    int32_t* outside_out;
    double* farthest_out;
};

// ... those of the wavefront map sweeps (float64 plans; no workspace, no statistics) ...
template <int SRC = kSrcFan>
int map_sweep_check(const rtpb_plan* plan, int64_t n_groups, const double* group_params, const SweepSource& s,
                    const double* refs, const double* windows, int32_t nx, int32_t ny, int32_t q_bits, double w_lim,
                    const void* count_out, const void* sum_out, const void* outside_out, const void* clipped_out,
                    const void* farthest_out) {
    const char* const what = SRC == kSrcBeam ? "wavefront-map-sweep-collimated" : "wavefront-map-sweep";
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    if (plan->dtype != RTPB_F64)
        return fail(RTPB_E_INVALID, std::string(what) + ": float64 plans only (a float32 phase of 1e4 ... 1e7 rad has "
                                                        "an ulp of a milliradian to a radian: its wavefront is noise)");
    if (n_groups <= 0 || !s.complete(SRC) || !group_params)
        return fail(RTPB_E_INVALID, std::string("bad ") + what + " arguments");
    // (n_a * n_b: a product past int64 is past the limit too)
    const int64_t gsize = s.n_a > 0x7fffffffll / s.n_b ? 0x80000000ll : s.n_a * s.n_b;
    int rc = wavemap_check(what, nx, ny, q_bits, w_lim, gsize, n_groups, refs, windows, count_out, sum_out,
                           outside_out, clipped_out, farthest_out);
    if (rc) return rc;
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, std::string(what) + ": too many groups");
    return RTPB_OK;
}

// rtpb_wavefront_map_sweep's own arguments (NS = kMapStats: no workspace, no statistics)
struct MapCall {
    const double* refs;         // host, n_groups x kWaveRef
    const double* windows;      // host, n_groups x kMapWin
    int32_t nx, ny, q_bits;
    double w_lim;
    int32_t* count_out;
    long long* sum_out;
    int32_t* outside_out;
    int32_t* clipped_out;
    double* farthest_out;
};

// A variant sweep's systems (SRC | kSrcVariant), lowered on the host (lower_variants): no plan and no device blob, the
// descriptors ride in the call's upload.  All variants have nsurf surfaces and nsurf + 1 materials.
struct VariantCall {
    int32_t nsurf = 0, n_variants = 0, dtype = RTPB_F64;
    int feat = 0;                                   // 1: some variant holds a PerfectLens (FEAT 17 for the call)
    const int32_t* group_variant = nullptr;         // host, n_groups, each in [0, n_variants)
    std::vector<DevSurface<double>> desc;           // [n_variants][nsurf], as a plan's blob holds them
    std::vector<DevMaterial<double>> mats;          // [n_variants][nsurf + 1]
    std::vector<std::vector<double>> tables;        // per variant: its TABLE materials' (wavelength, n) pairs
};

// ... and the sweep itself (checked arguments): plan the block rows, fill and send the one upload, launch the sweep
// kernels of the statistics set, then the final reduction -- or, for the image, clear the outputs and launch the
// image kernels.  refs: the wavefront mode's references (host, n_groups x kWaveRef); every group of that mode is a
// single row (the bundle rows' shared first surface keeps no phase) and its storage type is float64.
// vc (SRC | kSrcVariant, and then no plan): the systems of a variant sweep; a group's media are its own variant's, its
// block row is keyed on the variant too, and the descriptors and the groups' variants join the upload.  The wavefront
// mode over variants gives refs and vc both: the two are independent parts of the upload.
// NS = kFinalRays: no workspace and no reduction; stats_out is rays_out, n_groups x gsize x 8, written by the kernel.
// NS = kFootStats: refs is the surfaces' frames (host, nsurf x kFootFrame), the workspace holds the blocks' partials
// (n_groups x ceil(tiles / kSweepRays) x nsurf x kFootCols) and stats_out is n_groups x nsurf x kFootCols.
// NS = kEnergyStats: en holds the call's parameters and outputs, as im does the image's; no workspace, no statistics.
// NS = kMapStats: mp likewise; the references and the windows join the upload group by group.
template <int NS, int SRC = kSrcFan>
int sweep_impl(const rtpb_plan* plan_c, int32_t device, int64_t n_groups, const double* group_params,
               const SweepSource& src, double* workspace, double* stats_out, void* stream,
               const ImageCall* im = nullptr, const double* refs = nullptr, const VariantCall* vc = nullptr,
               const EnergyCall* en = nullptr, const MapCall* mp = nullptr) {
    constexpr bool kEnergy = NS == kEnergyStats, kMap = NS == kMapStats;
    static_assert(!kEnergy || (SRC & kSrcVariant) == 0, "energy curves: no variants");
    static_assert(!kMap || (SRC & kSrcVariant) == 0, "wavefront map: no variants");
    constexpr bool kImage = NS == kImageStats, kWave = NS == kWaveStats, kBeam = (SRC & ~kSrcVariant) == kSrcBeam;
    constexpr bool kVar = (SRC & kSrcVariant) != 0, kRays = NS == kFinalRays, kFoot = NS == kFootStats;
    static_assert(!kFoot || !kVar, "footprints: no variants");
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
    const SweepRows pr = plan_sweep_rows(group_params, n_groups, pre_n && !kWave && !kRays && !kFoot && !kMap, kSweepRays,
                                         kMaxBundle, kBeam ? src.frames : nullptr,
                                         kVar ? vc->group_variant : nullptr);
    // (a beam's second table is its offsets, plain doubles: half as many pair slots; the footprint mode's block is
    // all head: SweepFoot and the surfaces' frames, nothing per group)
    const SweepLayout lay(src.n_a, kBeam ? (src.n_b + 1) / 2 : src.n_b, n_groups, pre_n ? M + 3 * (M - 1) : 0,
                          pr.bundles.size() + pr.singles.size() + pr.rows.size() + (kVar ? size_t(n_groups) : 0),
                          kImage    ? sizeof(SweepImage) / sizeof(double)
                          : kEnergy ? sizeof(SweepEnergy) / sizeof(double)
                          : kMap    ? sizeof(SweepMap) / sizeof(double)
                          : kWave   ? sizeof(SweepWave) / sizeof(double)
                          : kFoot ? sizeof(SweepFoot) / sizeof(double) + size_t(nsurf) * kFootFrame
                                  : 0,
                          kWave ? kWaveRef : kMap ? kMapPar : kFoot ? 0 : 4, kBeam ? kFrame : 0,
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
    if constexpr (kImage) {
        const SweepImage head{im->image_out, im->outside_out, im->nx, im->ny};
        std::memcpy(h + lay.img, &head, sizeof(head));
        std::memcpy(h + lay.win, im->windows, size_t(4 * n_groups) * sizeof(double));
        rc = image_clear(im->image_out, im->outside_out, n_groups, im->nx, im->ny, st);
        if (rc) return rc;
    }
    if constexpr (kEnergy) {
        const SweepEnergy head{en->hist_out, en->outside_out, en->farthest_out, en->nr, 0};
        std::memcpy(h + lay.img, &head, sizeof(head));
        std::memcpy(h + lay.win, en->params, size_t(4 * n_groups) * sizeof(double));
        rc = energy_clear(en->hist_out, en->outside_out, en->farthest_out, n_groups, en->nr, st);
        if (rc) return rc;
    }
    if constexpr (kMap) {
        const SweepMap head{mp->count_out, mp->sum_out, mp->outside_out, mp->clipped_out, mp->farthest_out,
                            std::ldexp(1.0, mp->q_bits), mp->w_lim, mp->nx, mp->ny};
        std::memcpy(h + lay.img, &head, sizeof(head));
        double* const par = reinterpret_cast<double*>(h + lay.win);
        for (int64_t gi = 0; gi < n_groups; ++gi) {
            std::memcpy(par + kMapPar * gi, mp->refs + kWaveRef * gi, kWaveRef * sizeof(double));
            std::memcpy(par + kMapPar * gi + kWaveRef, mp->windows + kMapWin * gi, kMapWin * sizeof(double));
        }
        rc = wavemap_clear(mp->count_out, mp->sum_out, mp->outside_out, mp->clipped_out, mp->farthest_out, n_groups,
                           mp->nx, mp->ny, st);
        if (rc) return rc;
    }
    if constexpr (kWave) {
        const SweepWave head{workspace};
        std::memcpy(h + lay.img, &head, sizeof(head));
        std::memcpy(h + lay.win, refs, size_t(kWaveRef * n_groups) * sizeof(double));
    }
    if constexpr (kFoot) {
        // (refs: the surfaces' frames, nsurf x kFootFrame)
        const SweepFoot head{workspace};
        std::memcpy(h + lay.img, &head, sizeof(head));
        std::memcpy(h + lay.img + sizeof(head), refs, size_t(nsurf) * kFootFrame * sizeof(double));
    }
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
    if constexpr (kImage) a.image = reinterpret_cast<const SweepImage*>(d + lay.img);
    else if constexpr (kEnergy) a.energy = reinterpret_cast<const SweepEnergy*>(d + lay.img);
    else if constexpr (kMap) a.map = reinterpret_cast<const SweepMap*>(d + lay.img);
    else if constexpr (kWave) a.wave = reinterpret_cast<const SweepWave*>(d + lay.img);
    else if constexpr (kFoot) a.foot = reinterpret_cast<const SweepFoot*>(d + lay.img);
    else if constexpr (kRays) a.partials = stats_out;
    else a.partials = workspace;
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
        // (the wavefront, final-rays, footprint and map modes plan no bundle rows)
        if constexpr (!kWave && !kRays && !kFoot && !kMap) {
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
            else if constexpr (!kVar)                                                                        // POLY6 media
                hipLaunchKernelGGL((sweep_kernel<TS, 3, false, NS, SRC>), grid, dim3(kBlock), 0, st, as);
        }
    };
    if constexpr (kWave || kRays || kFoot || kMap) {
        go(double{});
    } else {
        if (dtype == RTPB_F64) go(double{});
        else go(float{});
    }
    HIP_TRY(hipGetLastError());
    if constexpr (kFoot) {
        rc = launch_foot_final(workspace, stats_out, n_groups, (tiles + kSweepRays - 1) / kSweepRays, nsurf, st);
        if (rc) return rc;
    } else if constexpr (!kImage && !kEnergy && !kMap && !kRays) {
        rc = launch_stats_final(NS, workspace, stats_out, n_groups, tiles, st);
        if (rc) return rc;
    }
    return dbuf.release();
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
// arguments, then `own`, the call's checks of its groups, source and outputs (sweep_check, final_rays_check), the range
// of group_variant and the upload bound (extra_upload: what the call's mode adds to variant_upload_bound), then each
// variant through rtpb_plan_create's own lowering (plan_fill, plan_surface, device_material) into vc.  `what` names
// the call in the messages.
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

// rtpb_focus_sweep_variants / _collimated: the prologue, the device, the sweep.
template <int SRC>
int focus_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                         int32_t n_variants, int32_t dtype, int32_t device, int64_t n_groups,
                         const double* group_params, const int32_t* group_variant, const SweepSource& src,
                         double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    VariantCall vc;
    int rc = lower_variant_call<SRC>(
        "focus-sweep-variants", surfaces, nsurf, materials, n_variants, dtype, n_groups, group_variant, src, 0,
        [&] { return sweep_check<kFocusStats, SRC>(n_groups, group_params, src, workspace, workspace_len, stats_out); },
        vc);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kFocusStats, SRC | kSrcVariant>(nullptr, device, n_groups, group_params, src, workspace,
                                                       stats_out, stream, nullptr, nullptr, &vc);
}

// rtpb_wavefront_sweep_variants / _collimated: float64, the references beside the systems.  The upload holds the
// references and the SweepWave word on top of variant_upload_bound.
template <int SRC>
int wavefront_sweep_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                             int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                             const int32_t* group_variant, const SweepSource& src, const double* refs,
                             double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    VariantCall vc;
    const size_t extra = n_groups > 0 ? size_t(n_groups) * kWaveRef * sizeof(double) + sizeof(SweepWave) : 0;
    int rc = lower_variant_call<SRC>(
        "wavefront-sweep-variants", surfaces, nsurf, materials, n_variants, RTPB_F64, n_groups, group_variant, src,
        extra,
        [&] {
            if (!refs) return fail(RTPB_E_INVALID, "bad wavefront-sweep arguments");
            return sweep_check<kWaveStats, SRC>(n_groups, group_params, src, workspace, workspace_len, stats_out);
        },
        vc);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kWaveStats, SRC | kSrcVariant>(nullptr, device, n_groups, group_params, src, workspace,
                                                      stats_out, stream, nullptr, refs, &vc);
}

// rtpb_final_rays_variants / _collimated: float64, at most one tile of rays per group, their final states to rays_out.
template <int SRC>
int final_rays_variants(const rtpb_surface* surfaces, int32_t nsurf, const rtpb_material* materials,
                        int32_t n_variants, int32_t device, int64_t n_groups, const double* group_params,
                        const int32_t* group_variant, const SweepSource& src, double* rays_out, void* stream) {
    VariantCall vc;
    int rc = lower_variant_call<SRC>(
        "final-rays-variants", surfaces, nsurf, materials, n_variants, RTPB_F64, n_groups, group_variant, src, 0,
        [&] { return final_rays_check<SRC>(n_groups, group_params, src, rays_out); }, vc);
    if (rc) return rc;
    rc = check_device(device);
    if (rc) return rc;
    return sweep_impl<kFinalRays, SRC | kSrcVariant>(nullptr, device, n_groups, group_params, src, nullptr, rays_out,
                                                     stream, nullptr, nullptr, &vc);
}

}  // namespace

