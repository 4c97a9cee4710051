// rtpb_sweep_kernel.h -- the fused sweep: generate + trace + reduce in one kernel.  The kernel is a
// template on the SOURCE of a group's rays (a fan, a beam; over a plan or over variants) and on the MODE of what
// becomes of each ray's final state; a mode is described once, by its SweepMode<NS> here (the facts and the device
// ending) and its SweepHost<NS> in rtpb_sweep_call.h (the host hooks of the one driver and the one entry prologue).
// Each row's entry points instantiate kernel and driver in translation units of their own, fan and beam apart, so
// that they compile side by side:
//
//   mode            tag NS            entry points (each also _collimated)           units
//   spot            kStats = 7        rtpb_spot_sweep                                rtpb_sweep[_beam].hip
//   focus           kFocusStats = 16  rtpb_focus_sweep                               rtpb_sweep[_beam].hip
//                                     rtpb_focus_sweep_variants                      rtpb_sweep_variants[_beam].hip
//   wavefront       kWaveStats = 15   rtpb_wavefront_sweep                           rtpb_sweep[_beam].hip
//                                     rtpb_wavefront_sweep_variants                  rtpb_sweep_wave_variants[_beam].hip
//   image           kImageStats = 0   rtpb_image_sweep                               rtpb_sweep[_beam].hip
//   energy          kEnergyStats = 2  rtpb_energy_sweep                              rtpb_sweep_energy[_beam].hip
//   wavefront map   kMapStats = 4     rtpb_wavefront_map_sweep                       rtpb_sweep_wavemap[_beam].hip
//   final rays      kFinalRays = 8    rtpb_final_rays_variants                       rtpb_sweep_wave_variants[_beam].hip
//   footprint       kFootStats = 32   rtpb_footprint_sweep                           rtpb_sweep_foot[_beam].hip
//   transmission    kTransStats = 64  rtpb_transmission_sweep                        rtpb_sweep_trans[_beam].hip
//   polarisation    kPolStats = 128   rtpb_polarisation_sweep                        rtpb_sweep_pol[_beam].hip
//
// What the sweep shares with the plane kernels (the statistics, the counters' contribution rules) is rtpb_stats.h, the
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
// Variant sweep (SRC | kSrcVariant).  Group g traces through the surface descriptors desc + variant[g] * nsurf of the
// call's own upload instead of a plan's blob: many perturbed copies of one system in one launch.  A block row's groups
// share their variant (plan_sweep_rows keys on it), so the base of a block's descriptors is one more block-uniform
// pointer and every descriptor load stays a scalar load; the kinds and geometry codes of a surface may differ from
// variant to variant.  Host-evaluated media only (FEAT 16 / 17), which arrive per group as before.  The flag is folded
// into SRC, so the instantiations without it are the code they were.
constexpr int kSrcFan = 0, kSrcBeam = 1, kSrcVariant = 2;
constexpr int kFrame = 9;               // a beam's frame: normal, n1, n2
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
        double* __restrict__ partials;      // modes without a header: the tile partials, or the final rays' rows
        // modes with one (SweepMode<NS>::Head): the mode's block of the sweep's one upload (SweepLayout::img and
        // win) -- the header, then what follows it per call, then kPerGroup doubles per group
        const void* __restrict__ block;
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
// The modes that run the trace or history kernel's full step with the phase and the whole direction alive to the end:
// RTPB_WAVE_WPE waves per SIMD for them (the registers, scratch and LDS at each setting)
#ifndef RTPB_WAVE_WPE
#define RTPB_WAVE_WPE 4
#endif
// An optimisation fence on three per-lane values: the compiler moves no computation on them across it
#if defined(__HIP_DEVICE_COMPILE__)
#define RTPB_PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))
#else
#define RTPB_PIN3(a, b, c) ((void)0)
#endif

// ---- The modes ----
// SweepMode<NS>: what a mode is, in one place.  NS is the mode's tag -- for the three statistics modes it is also the
// number of columns (rtpb_stats.h), for the others an arbitrary value apart from those.  The facts:
//   kCols       columns of a tile partial (0: no tile partials)
//   kSteps      the surface step's semantics: kPosOnly (final positions only: no TIR fill of the position -- the next
//               surface's intersection makes it NaN, and the final plane gets the rule in the ending -- and a run of
//               axial spheres carries x x + y y), kNoAt (the final-plane trace kernel's: the full semantics of every
//               surface, its roots and square roots included, the phase kept) or kHistorySteps (the history kernel's:
//               the at-plane formed too)
//   kWpe        the occupancy class
//   kBundles    bundle rows allowed (their shared first surface keeps no phase)
//   kF32        float32 storage allowed
//   kPlans, kVariants   the systems it has entry points for
//   kHostMedia  the mode reads the group's indices itself, so only the instantiations with host-evaluated media exist
//               (FEAT bit 4): its entry points refuse the plans that have none (a POLY6 material)
//   red_rows(bundle)    rows of the LDS reduction buffer
//   Head, kPerGroup     the header of the mode's block of the upload (void: none) and the doubles per group behind it
// and, for the modes without tile partials (kCols = 0) and without history steps, the device hook that the kernel
// calls for every ray of the block:
//   end<TS>(a, rr, ok, g, t)   the lane's ray of group g (tile t) ended in state rr; !ok: the lane lies past the group
// The three statistics modes' ending (the kernel's `reduce`) and the footprint mode's per-surface combine and block
// epilogue stay in the kernel body as they were: moved into hooks, every form tried changed those kernels' generated
// code (register allocation and scheduling), and a cleanup leaves the device code as it is (tools/isa_compare.py).
constexpr int kHistorySteps = 0;
constexpr int kImageStats = 0, kEnergyStats = 2, kMapStats = 4, kFinalRays = 8, kFootStats = 32;
constexpr int kTransStats = 64;
constexpr int kPolStats = 128;

template <int NS>
struct SweepMode;       // (only the ten specialisations below exist)

struct SweepModeDefaults {      // (what most modes are)
    static constexpr int kCols = 0;
    static constexpr int kSteps = kPosOnly;
    static constexpr int kWpe = RTPB_SWEEP_WPE;
    static constexpr bool kBundles = true, kF32 = true, kPlans = true, kVariants = false;
    static constexpr bool kHostMedia = false;
    static constexpr int red_rows(bool) { return 1; }
    using Head = void;
    static constexpr int kPerGroup = 0;
};

// A mode with a header: where it and the doubles behind it lie
template <typename H>
struct SweepModeHead : SweepModeDefaults {
    using Head = H;
    static __device__ __forceinline__ cptr<H> head(const SweepArgs& a) { return (cptr<H>)(a.block); }
    static __device__ __forceinline__ cptr<double> tail(const SweepArgs& a) {
        return (cptr<double>)(static_cast<const H*>(a.block) + 1);
    }
};

// Spot statistics (rtpb_spot_sweep).  Single rows reduce all seven at once, bundle rows two at a time.
template <>
struct SweepMode<kStats> : SweepModeDefaults {
    static constexpr int kCols = kStats;
    static constexpr int red_rows(bool bundle) { return bundle ? 2 : kStats; }
};

// Focus statistics (rtpb_focus_sweep, and over variants): focus_ray of the final state, so the whole final direction
// stays alive to the end.  kPosOnly leaves no part of it unfinished on any surface kind -- snell_apply, reflect and
// lens_step compute dx, dy and dz in full whatever the mode, and a killed row is all NaN (the mode only skips the
// position fill after a NaN direction and the at-plane) -- so the last surface runs the same step as the others.
// Single rows reduce eight of the sixteen statistics at a time (16 KB of LDS), bundle rows two.
template <>
struct SweepMode<kFocusStats> : SweepModeDefaults {
    static constexpr int kCols = kFocusStats;
    static constexpr bool kVariants = true;
    static constexpr int red_rows(bool bundle) { return bundle ? 2 : 8; }
};

// Wavefront statistics (rtpb_wavefront_sweep, and over variants): wave_ray of the final state -- the one rtpb_trace
// stores, phase and all -- against the group's reference; eight of the fifteen statistics at a time.  Its block of
// the upload: where the tile partials go, then the groups' references (kWaveRef doubles each, rtpb_stats.h).
struct SweepWave {
    double* partials;
};
static_assert(sizeof(SweepWave) == sizeof(double), "the references follow it");
template <>
struct SweepMode<kWaveStats> : SweepModeHead<SweepWave> {
    static constexpr int kCols = kWaveStats;
    static constexpr int kSteps = kNoAt;
    static constexpr int kWpe = RTPB_WAVE_WPE;
    static constexpr bool kBundles = false, kF32 = false, kVariants = true;
    static constexpr int red_rows(bool) { return 8; }
    static constexpr int kPerGroup = kWaveRef;
};

// Image (rtpb_image_sweep): no statistics and no red tiles, each counted ray goes into its group's image instead
// (image_bin, wave_image_add); the rule of which rays count is the spot statistics'.  Every lane reaches the wave's
// adds, and g is the same in the whole block.  Its block of the upload: the outputs, then the groups' windows (4
// doubles each).
struct SweepImage {
    int32_t* image;      // [n_groups][ny][nx]
    int32_t* outside;    // [n_groups]
    int32_t nx, ny;
};
static_assert(sizeof(SweepImage) % sizeof(double) == 0, "the windows follow it");
template <>
struct SweepMode<kImageStats> : SweepModeHead<SweepImage> {
    static constexpr int kPerGroup = 4;
    template <typename TS>
    static __device__ __forceinline__ void end(const SweepArgs& a, const Ray<double>& rr, bool ok,
                                               int64_t g, int64_t) {
        const cptr<SweepImage> im = head(a);
        const cptr<double> win = tail(a) + 4 * g;
        const int nx = im->nx, ny = im->ny;
        int bin = kImageSkip;
        if (ok && !is_nan(rr.dx)) {
            const double w[4] = {win[0], win[1], win[2], win[3]};
            bin = image_bin(stored<TS>(rr.x), stored<TS>(rr.y), w, nx, ny);
        }
        wave_image_add(bin, im->image + g * ny * nx, im->outside + g);
    }
};

// Energy curves (rtpb_energy_sweep): the image mode with another rule per ray -- each counted ray goes into its
// group's circle and square histograms and into the two maxima (energy_bins, wave_energy_add).  Its block of the
// upload: the outputs and the number of bins, then the groups' parameters (4 doubles each: cx, cy, scale, 0).
struct SweepEnergy {
    int32_t* hist;       // [n_groups][2][nr]
    int32_t* outside;    // [n_groups][2]
    double* farthest;    // [n_groups][2]
    int32_t nr, pad;
};
static_assert(sizeof(SweepEnergy) % sizeof(double) == 0, "the parameters follow it");
template <>
struct SweepMode<kEnergyStats> : SweepModeHead<SweepEnergy> {
    static constexpr int kPerGroup = 4;
    template <typename TS>
    static __device__ __forceinline__ void end(const SweepArgs& a, const Ray<double>& rr, bool ok,
                                               int64_t g, int64_t) {
        const cptr<SweepEnergy> en = head(a);
        const cptr<double> par = tail(a) + 4 * g;
        const int nr = en->nr;
        EnergyRay e{{kImageSkip, kImageSkip}, {0.0, 0.0}};
        if (ok && !is_nan(rr.dx)) {
            const double p[4] = {par[0], par[1], par[2], par[3]};
            e = energy_bins(stored<TS>(rr.x), stored<TS>(rr.y), p, nr);
        }
        wave_energy_add(e, nr, en->hist + g * 2 * nr, en->outside + 2 * g, en->farthest + 2 * g);
    }
};

// Wavefront map (rtpb_wavefront_map_sweep): the wavefront mode's steps and occupancy class with the counter modes'
// ending -- the statistics' rule of which final states reach wave_ray, then wavemap_ray into the group's map
// (wave_map_add).  Its block of the upload: the outputs and the call's sides, scale and limit, then the groups'
// references and windows (kMapPar = kWaveRef + kMapWin doubles each; rtpb_wavemap.h).
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
template <>
struct SweepMode<kMapStats> : SweepModeHead<SweepMap> {
    static constexpr int kSteps = kNoAt;
    static constexpr int kWpe = RTPB_WAVE_WPE;
    static constexpr bool kBundles = false, kF32 = false;
    static constexpr int kPerGroup = kMapPar;
    template <typename TS>
    static __device__ __forceinline__ void end(const SweepArgs& a, const Ray<double>& rr, bool ok,
                                               int64_t g, int64_t) {
        const cptr<SweepMap> mp = head(a);
        const cptr<double> q = tail(a) + kMapPar * g;
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
    }
};

// Final rays (rtpb_final_rays_variants; groups of at most one tile): no reduction, each ray's final state goes to
// rays_out[group][ray] (SweepArgs::partials) as the row rtpb_trace stores for the final plane, a killed ray's NaN
// pattern included, so the steps are the wavefront mode's.  A plain per-lane store of the row (four 16-byte stores),
// inside the group's own rows only: lanes past the group's size store nothing.
template <>
struct SweepMode<kFinalRays> : SweepModeDefaults {
    static constexpr int kSteps = kNoAt;
    static constexpr int kWpe = RTPB_WAVE_WPE;
    static constexpr bool kBundles = false, kF32 = false, kPlans = false, kVariants = true;
    template <typename TS>
    static __device__ __forceinline__ void end(const SweepArgs& a, const Ray<double>& rr, bool ok,
                                               int64_t g, int64_t t) {
        const int64_t j = t * kBlock + threadIdx.x;
        if (j < a.gsize) store_ray<double, RTPB_AOS>(a.partials, g * a.gsize + j, 0, rr);
    }
};

// Footprints (rtpb_footprint_sweep): the footprint statistics of EVERY surface (rtpb_foot.h, kFootCols columns).  They
// are defined on the history's "at" and "after" planes, so the steps are the history kernel's (the at-plane formed and
// handed to emit_at, which keeps its position; the TIR fill; no carried x x + y y).  After each surface the lane's rays
// are combined (foot_ray, foot_merge; lanes past the group's size and rays whose tile lies past the group's tiles
// contribute nothing), then the wave's lanes (foot_wave_reduce), and lane 0 of each wave writes the wave's row of that
// surface into the block's LDS table -- its own row, so the surface loop holds no barrier.  After the loop one
// barrier, and the block's threads combine the four waves' rows and store them as the block's partial
// [group][block][surface][8]; foot_final_kernel (rtpb_footprint.hip) combines a group's blocks.
// nsurf <= RTPB_MAX_SURFACES, the plans' bound.  Its block of the upload: where the block partials go, then the
// surfaces' frames (kFootFrame doubles each) -- one per surface of the plan, nothing per group.
struct SweepFoot {
    double* partials;
};
static_assert(sizeof(SweepFoot) == sizeof(double), "the frames follow it");
template <>
struct SweepMode<kFootStats> : SweepModeHead<SweepFoot> {
    static constexpr int kSteps = kHistorySteps;
    static constexpr int kWpe = RTPB_WAVE_WPE;
    static constexpr bool kBundles = false, kF32 = false;
};

// Transmission (rtpb_transmission_sweep): the transmission statistics of EVERY surface (rtpb_trans.h, kTransCols
// columns) -- the footprint mode with another rule per ray and surface.  The rule reads what the history steps hold
// after a surface anyway: the at-plane with the incoming direction, the ray after the surface with the outgoing one,
// and the two indices n_cur and n_next (host-evaluated: scalar operands).  One cum per ray of the lane is carried
// across the surface runs, as n_cur is.  The combination per surface, the waves' rows in LDS (10 KB) and the block
// epilogue are the footprints', with trans_merge / trans_col.  Its block of the upload: where the block partials go
// and 2^q_bits, then the surfaces' coatings (kTransCoat doubles each) -- nothing per group.
struct SweepTrans {
    double* partials;
    double scale;
};
static_assert(sizeof(SweepTrans) == 2 * sizeof(double), "the coatings follow it");
template <>
struct SweepMode<kTransStats> : SweepModeHead<SweepTrans> {
    static constexpr int kSteps = kHistorySteps;
    static constexpr int kWpe = RTPB_WAVE_WPE;
    static constexpr bool kBundles = false, kF32 = false, kHostMedia = true;
};

// Polarisation (rtpb_polarisation_sweep): the polarisation statistics of EVERY surface (rtpb_pol.h, kPolCols columns)
// -- the transmission mode with a state of kPolState doubles per ray of the lane in cum's place, launched from the
// generated ray's direction and carried across the surface runs.  It reads what the transmission rule reads (the
// at-plane with the incoming direction, the ray after the surface, n_cur and n_next).  The combination per surface, the
// waves' rows in LDS (12 KB) and the block epilogue are the transmission's, with pol_merge (every column a sum).  Its
// block of the upload: where the block partials go, 2^q_bits, the polariser and the analyser axes, then the surfaces'
// coatings as {mode, amplitude} (kTransCoat doubles each) -- nothing per group.  The state is 24 VGPRs a lane on top
// of the transmission mode's, so the mode has an occupancy class of its own (the registers at each).
#ifndef RTPB_POL_WPE
#define RTPB_POL_WPE 3
#endif
struct SweepPol {
    double* partials;
    double scale;
    double u[3], w[3];
};
static_assert(sizeof(SweepPol) == 8 * sizeof(double), "the coatings follow it");
template <>
struct SweepMode<kPolStats> : SweepModeHead<SweepPol> {
    static constexpr int kSteps = kHistorySteps;
    static constexpr int kWpe = RTPB_POL_WPE;
    static constexpr bool kBundles = false, kF32 = false, kHostMedia = true;
};

#define RTPB_SWEEP_ATTR(NS) __attribute__((amdgpu_waves_per_eu(SweepMode<NS>::kWpe, 8)))

// SRC = kSrcBeam: the generator of a collimated beam; a bundle row's groups share the beam (pt and frame) as the
// fan's share the field point, and everything after the generator is the same code.
template <typename TS, int FEAT, bool BUNDLE, int NS = kStats, int SRC = kSrcFan>
__global__ __launch_bounds__(kBlock) RTPB_SWEEP_ATTR(NS) void sweep_kernel(SweepArgs a) {
    using Mode = SweepMode<NS>;
    constexpr int kGen = SRC & ~kSrcVariant;
    constexpr bool kVar = (SRC & kSrcVariant) != 0;
    static_assert(kGen == kSrcFan || kGen == kSrcBeam, "a fan or a beam");
    static_assert(kVar ? Mode::kVariants && (FEAT & 16) != 0 && (FEAT & 2) == 0 : Mode::kPlans,
                  "the mode takes no such systems; variants: host-evaluated media");
    static_assert(!BUNDLE || (Mode::kBundles && (FEAT & 16) != 0),
                  "bundles: a mode that allows them, host-evaluated media");
    static_assert(sizeof(TS) == 8 || Mode::kF32, "the mode's storage is float64");
    static_assert(!Mode::kHostMedia || (FEAT & 16) != 0, "the mode reads host-evaluated media");
    // the at-plane kept: the footprints, the transmission and the polarisation
    constexpr bool kHistory = Mode::kSteps == kHistorySteps;
    constexpr bool kTrans = NS == kTransStats;
    constexpr bool kPol = NS == kPolStats;
    constexpr int kRedRows = Mode::red_rows(BUNDLE);
    __shared__ double red[kRedRows][kBlock];
    __shared__ double state[BUNDLE ? kStateRows : 1][kBlock];
    // footprints: per wave, one row per surface (16 KB); transmission likewise (10 KB)
    double (*foot_tab)[RTPB_MAX_SURFACES][kFootCols] = nullptr;
    [[maybe_unused]] double (*trans_tab)[RTPB_MAX_SURFACES][kTransCols] = nullptr;
    [[maybe_unused]] double (*pol_tab)[RTPB_MAX_SURFACES][kPolCols] = nullptr;      // polarisation: 12 KB
    if constexpr (kPol) {
        __shared__ double pol_lds[kBlock / 64][RTPB_MAX_SURFACES][kPolCols];
        pol_tab = pol_lds;
    } else if constexpr (kTrans) {
        __shared__ double trans_lds[kBlock / 64][RTPB_MAX_SURFACES][kTransCols];
        trans_tab = trans_lds;
    } else if constexpr (kHistory) {
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
    constexpr int kMode = Mode::kSteps | ((FEAT & 16) != 0 ? kUniMedia : 0);
    // Runs of consecutive surfaces of one (kind, axial) code: each run loops inside one instantiation of the surface
    // step, so the rays' registers carry from surface to surface without the copies a per-surface join of the kind
    // branches needs (the ODT path of C5: 12 axial spheres, a lens, a flat = 3 runs).
    double rxy[kSweepRays];
    bool live[kSweepRays];              // history steps: the lane's ray q is one of its group's
    [[maybe_unused]] double cum[kSweepRays];        // transmission: ray q's product over the surfaces so far
    [[maybe_unused]] double pol[kSweepRays][kPolState];     // polarisation: ray q's two field vectors
    auto trace_from = [&](int s) {
        while (s < a.nsurf) {
            const int code = code_of(s);
            dispatch_code<(FEAT & 1) != 0>(code, [&](auto kind, auto geo) {
                constexpr int K = decltype(kind)::value;
                constexpr int A = decltype(geo)::value;
                constexpr bool kCarry = K == SPHERE && A == kGeoAxial && Mode::kSteps == kPosOnly;
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
                    [[maybe_unused]] double at[kSweepRays][kTrans || kPol ? 6 : 3];
#pragma unroll
                    for (int q = 0; q < kSweepRays; ++q) {
                        const DevSurface<double> sd = (BUNDLE || q == 0) ? surface_for(q, s, base)
                                                                         : surface_for(0, s, base);
                        if constexpr (kHistory) {
                            auto keep = [&](const Ray<double>& p) {
                                at[q][0] = p.x; at[q][1] = p.y; at[q][2] = p.z;
                                if constexpr (kTrans || kPol) {
                                    at[q][3] = p.dx; at[q][4] = p.dy; at[q][5] = p.dz;
                                }
                            };
                            surface_step<double, K, A, kMode>(sd, r[q], n_cur[q], n_next[q], iwl[q], keep, o[q],
                                                              static_cast<GuardBranch*>(nullptr));
                        } else {
                            surface_step<double, K, A, kMode>(sd, r[q], n_cur[q], n_next[q], iwl[q], none, o[q],
                                                              static_cast<GuardBranch*>(nullptr),
                                                              kCarry ? &rxy[q] : nullptr);
                        }
                    }
                    if constexpr (kPol) {
                        // the surface's coating, the analyser and the call's 2^q_bits: the block's, so scalar loads
                        const cptr<SweepPol> hd = Mode::head(a);
                        const cptr<double> cp = Mode::tail(a) + kTransCoat * s;
                        const double coat_mode = cp[0], coat_amp = cp[1];
                        const double scale = hd->scale;
                        const double w_an[3] = {hd->w[0], hd->w[1], hd->w[2]};
                        PolRay acc = pol_none();
#pragma unroll
                        for (int q = 0; q < kSweepRays; ++q) {
                            const bool pass = foot_finite3(at[q][0], at[q][1], at[q][2]) &&
                                              foot_finite3(o[q].x, o[q].y, o[q].z);
                            pol_surface(pass, at[q][3], at[q][4], at[q][5], o[q].dx, o[q].dy, o[q].dz, n_cur[q],
                                        n_next[q], coat_mode, coat_amp, pol[q]);
                            if (live[q] && pass) pol_merge(acc, pol_term(pol[q], o[q].dx, o[q].dy, o[q].dz, w_an, scale));
                        }
                        pol_wave_reduce(acc);
                        if ((tid & 63) == 0) {
#pragma unroll
                            for (int c = 0; c < kPolCols; ++c) pol_tab[tid >> 6][s][c] = acc.v[c];
                        }
                    } else if constexpr (kTrans) {
                        // the surface's coating and the call's 2^q_bits: the block's, so scalar loads
                        const cptr<double> cp = Mode::tail(a) + kTransCoat * s;
                        const double coat_mode = cp[0], coat_value = cp[1];
                        const double scale = Mode::head(a)->scale;
                        TransRay acc = trans_none();
#pragma unroll
                        for (int q = 0; q < kSweepRays; ++q) {
                            double t;
                            const bool pass = trans_ray(at[q][0], at[q][1], at[q][2], at[q][3], at[q][4], at[q][5],
                                                        o[q].x, o[q].y, o[q].z, o[q].dx, o[q].dy, o[q].dz, n_cur[q],
                                                        n_next[q], coat_mode, coat_value, t, cum[q]);
                            if (live[q] && pass) trans_merge(acc, trans_term(t, cum[q], scale));
                        }
                        trans_wave_reduce(acc);
                        if ((tid & 63) == 0) {
#pragma unroll
                            for (int c = 0; c < kTransCols; ++c) trans_tab[tid >> 6][s][c] = acc.v[c];
                        }
                    } else if constexpr (kHistory) {
                        // the surface's frame: the block's, so scalar loads
                        const cptr<double> fp = Mode::tail(a) + kFootFrame * s;
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
    // The statistics modes' ending (Mode::kCols > 0; in the kernel, see SweepMode): one ray's contribution to its
    // group's tile partial, spot_partial_kernel's tree (block_tree_sum), kRedRows statistics at a time
    constexpr bool kWave = NS == kWaveStats;
    auto reduce = [&](const Ray<double>& rr, bool ok, int64_t g, int64_t t) {
        double v[kStats] = {};
        FocusRay f{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        WaveRay wv{0.0, 0.0, 0.0, 0.0, 0.0};
        double* out;
        if constexpr (kWave) out = ((cptr<SweepWave>)(static_cast<const SweepWave*>(a.block)))->partials;
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
                const cptr<double> q = (cptr<double>)(static_cast<const SweepWave*>(a.block) + 1) + kWaveRef * g;
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
        if constexpr (kHistory) {
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) live[q] = tile[q] * kBlock + tid < a.gsize;
        }
        if constexpr (kTrans) {
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) cum[q] = 1.0;
        }
        if constexpr (kPol) {
            // the launch, from the generated ray's direction and the call's polariser
            const cptr<SweepPol> hd = Mode::head(a);
            const double u[3] = {hd->u[0], hd->u[1], hd->u[2]};
#pragma unroll
            for (int q = 0; q < kSweepRays; ++q) pol_launch(r[q].dx, r[q].dy, r[q].dz, u, pol[q]);
        }
        trace_from(0);
        if constexpr (kPol) {
            // the block's partial: the four waves' rows combined, [group][block][surface][kPolCols]
            __syncthreads();
            double* out = Mode::head(a)->partials + (grp[0] * int64_t(gridDim.x) + blockIdx.x) * a.nsurf * kPolCols;
            for (int k = tid; k < a.nsurf * kPolCols; k += kBlock) {
                const int s = k / kPolCols, c = k % kPolCols;
                double v = pol_tab[0][s][c];
#pragma unroll
                for (int w = 1; w < kBlock / 64; ++w) v = v + pol_tab[w][s][c];
                out[k] = v;
            }
        } else if constexpr (kTrans) {
            // the block's partial: the four waves' rows combined, [group][block][surface][kTransCols]
            __syncthreads();
            double* out = Mode::head(a)->partials + (grp[0] * int64_t(gridDim.x) + blockIdx.x) * a.nsurf * kTransCols;
            for (int k = tid; k < a.nsurf * kTransCols; k += kBlock) {
                const int s = k / kTransCols, c = k % kTransCols;
                double v = trans_tab[0][s][c];
#pragma unroll
                for (int w = 1; w < kBlock / 64; ++w) v = trans_col(c, v, trans_tab[w][s][c]);
                out[k] = v;
            }
        } else if constexpr (kHistory) {
            // the block's partial: the four waves' rows combined, [group][block][surface][kFootCols]
            __syncthreads();
            double* out = Mode::head(a)->partials + (grp[0] * int64_t(gridDim.x) + blockIdx.x) * a.nsurf * kFootCols;
            for (int k = tid; k < a.nsurf * kFootCols; k += kBlock) {
                const int s = k / kFootCols, c = k % kFootCols;
                double v = foot_tab[0][s][c];
#pragma unroll
                for (int w = 1; w < kBlock / 64; ++w) v = foot_col(c, v, foot_tab[w][s][c]);
                out[k] = v;
            }
        } else {
#pragma unroll
            // (tile partials, or the mode's own ending; the bundle rows below likewise)
            for (int q = 0; q < kSweepRays; ++q)
                if constexpr (Mode::kCols > 0) reduce(r[q], tile[q] * kBlock + tid < a.gsize, grp[q], tile[q]);
                else Mode::template end<TS>(a, r[q], tile[q] * kBlock + tid < a.gsize, grp[q], tile[q]);
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
            for (int q = 0; q < kSweepRays; ++q)
                if constexpr (Mode::kCols > 0) reduce(r[q], t0 * kBlock + tid < a.gsize, grp[q], t0);
                else Mode::template end<TS>(a, r[q], t0 * kBlock + tid < a.gsize, grp[q], t0);
        }
    }
}

}  // namespace
