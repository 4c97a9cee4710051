// rtpb_polarisation.hip -- the polarisation statistics of a stored history (rtpb_polarisation_stats: the unfused path,
// and the way to use the feature on a history one already has), the second pass they share with the fused polarisation
// sweep (launch_pol_final), each ray's two final field vectors (rtpb_ray_polarisation) and the host checks the
// polarisation calls share (pol_check).  The per-ray rule and its combination are rtpb_pol.h's, the wave reduction
// rtpb_stats.h's.
#include "rtpb_stats.h"
#include "rtpb_sweep_host.h"

#include <cstring>

using namespace rtpbi;

namespace {

struct PolArgs {
    const double* __restrict__ hist;        // [1 + 2 nsurf][n_groups * gsize][8]
    const double* __restrict__ media;       // [n_groups][nsurf + 1]
    const double* __restrict__ coat;        // [nsurf][kTransCoat]: {mode, amplitude}
    double* __restrict__ out;               // partials [n_groups][tiles][nsurf][kPolCols], or kPolState doubles per ray
    double scale;                           // 2^q_bits
    double u[3], w[3];                      // the polariser and the analyser
    int64_t gsize, ngroups, tiles;
    int32_t nsurf;
};

// Ray i of the history: its state behind the polariser, from its direction in plane 0
__device__ __forceinline__ void pol_start(const PolArgs& a, int64_t i, double (&e)[kPolState]) {
    const double* R = a.hist + i * 8;
    const double u[3] = {a.u[0], a.u[1], a.u[2]};
    pol_launch(R[3], R[4], R[5], u, e);
}

// Ray i of the history at surface s: the rule's step, the state carried by the caller.  Returns whether the ray
// passes; b is its outgoing direction.
__device__ __forceinline__ bool pol_step(const PolArgs& a, int64_t i, int64_t g, int s, double (&e)[kPolState],
                                         double (&b)[3]) {
    const int64_t n = a.ngroups * a.gsize;
    const double* A = a.hist + ((2 * s + 1) * n + i) * 8;
    const double* B = A + n * 8;
    const double* m = a.media + g * (a.nsurf + 1) + s;
    const double* c = a.coat + kTransCoat * s;
    const bool pass = foot_finite3(A[0], A[1], A[2]) && foot_finite3(B[0], B[1], B[2]);
    b[0] = B[3]; b[1] = B[4]; b[2] = B[5];
    pol_surface(pass, A[3], A[4], A[5], b[0], b[1], b[2], m[0], m[1], c[0], c[1], e);
    return pass;
}

// Block (tile, group): each lane follows its ray through the surfaces in order (the state is carried over them); per
// surface the wave's lanes are combined and lane 0 writes the wave's row -- its own, so the loop holds no barrier --
// and after it the block's threads combine the four waves' rows, as the fused sweep does.
__global__ __launch_bounds__(kBlock) void pol_partial_kernel(PolArgs a) {
    __shared__ double tab[kBlock / 64][RTPB_MAX_SURFACES][kPolCols];
    const int64_t tile = blockIdx.x, g = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t j = tile * kBlock + tid;
    const double w[3] = {a.w[0], a.w[1], a.w[2]};
    double e[kPolState];
    if (j < a.gsize) pol_start(a, g * a.gsize + j, e);
    for (int s = 0; s < a.nsurf; ++s) {
        PolRay f = pol_none();
        if (j < a.gsize) {
            double b[3];
            if (pol_step(a, g * a.gsize + j, g, s, e, b)) f = pol_term(e, b[0], b[1], b[2], w, a.scale);
        }
        pol_wave_reduce(f);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int c = 0; c < kPolCols; ++c) tab[tid >> 6][s][c] = f.v[c];
        }
    }
    __syncthreads();
    double* out = a.out + (g * a.tiles + tile) * a.nsurf * kPolCols;
    for (int k = tid; k < a.nsurf * kPolCols; k += kBlock) {
        const int s = k / kPolCols, c = k % kPolCols;
        double v = tab[0][s][c];
#pragma unroll
        for (int wv = 1; wv < kBlock / 64; ++wv) v = v + tab[wv][s][c];
        out[k] = v;
    }
}

// One thread per ray: the state after the last surface, NaN for a ray without one
__global__ __launch_bounds__(kBlock) void ray_pol_kernel(PolArgs a) {
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= a.ngroups * a.gsize) return;
    const int64_t g = i / a.gsize;
    double e[kPolState], b[3];
    pol_start(a, i, e);
    for (int s = 0; s < a.nsurf; ++s) pol_step(a, i, g, s, e, b);
#pragma unroll
    for (int c = 0; c < kPolState; ++c) a.out[i * kPolState + c] = e[c];
}

struct PolFinalArgs {
    const double* __restrict__ partials;    // [n_groups][blocks][nsurf][kPolCols]
    double* __restrict__ stats;             // [n_groups][nsurf][kPolCols]
    int64_t blocks;
    int32_t nsurf;
};

// Block (surface, group): thread t combines the group's partials t, t + 256, ..., then the wave's lanes and the four
// waves' rows
__global__ __launch_bounds__(kBlock) void pol_final_kernel(PolFinalArgs a) {
    __shared__ double tab[kBlock / 64][kPolCols];
    const int s = blockIdx.x;
    const int64_t g = blockIdx.y;
    const int tid = threadIdx.x;
    PolRay f = pol_none();
    for (int64_t b = tid; b < a.blocks; b += kBlock) {
        const double* p = a.partials + ((g * a.blocks + b) * a.nsurf + s) * kPolCols;
        PolRay o;
#pragma unroll
        for (int c = 0; c < kPolCols; ++c) o.v[c] = p[c];
        pol_merge(f, o);
    }
    pol_wave_reduce(f);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kPolCols; ++c) tab[tid >> 6][c] = f.v[c];
    }
    __syncthreads();
    if (tid < kPolCols) {
        double v = tab[0][tid];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) v = v + tab[w][tid];
        a.stats[(g * a.nsurf + s) * kPolCols + tid] = v;
    }
}

// What rtpb_polarisation_stats and rtpb_ray_polarisation check before the device (`what` names the call)
int pol_history_check(const std::string& what, int32_t dtype, const void* history, int64_t group_size,
                      int64_t n_groups, int32_t nsurf, const double* media, const double* coatings,
                      const double* polariser, const void* out) {
    if (dtype == RTPB_F32)
        return fail(RTPB_E_INVALID, what + ": float64 histories only (the statistics are defined on the float64 "
                                           "history)");
    if (dtype != RTPB_F64) return fail(RTPB_E_INVALID, "bad " + what + " arguments: dtype");
    if (group_size <= 0 || n_groups <= 0 || nsurf <= 0 || !history || !media || !coatings || !polariser || !out)
        return fail(RTPB_E_INVALID, "bad " + what + " arguments");
    if (nsurf > RTPB_MAX_SURFACES) return fail(RTPB_E_LIMIT, what + ": more than RTPB_MAX_SURFACES surfaces");
    return RTPB_OK;
}

// The media and the coatings as {mode, amplitude}: one small stream-ordered upload, media first
int pol_upload_tables(const double* media, const double* coatings, int64_t n_groups, int32_t nsurf, hipStream_t st,
                      StreamScratch& d) {
    const size_t nm = size_t(n_groups) * size_t(nsurf + 1), nc = size_t(nsurf) * kTransCoat;
    const size_t bytes = (nm + nc) * sizeof(double);
    int rc = d.alloc(bytes, st);
    if (rc) return rc;
    PinnedStaging& pin = pinned_staging();
    rc = pin.reserve(bytes);
    if (rc) return rc;
    double* const h = reinterpret_cast<double*>(pin.buf);
    std::memcpy(h, media, nm * sizeof(double));
    for (int32_t s = 0; s < nsurf; ++s) {
        h[nm + kTransCoat * s] = coatings[kTransCoat * s];
        h[nm + kTransCoat * s + 1] = pol_coat_amplitude(coatings[kTransCoat * s], coatings[kTransCoat * s + 1]);
    }
    return pin.upload(d.p, bytes, st);
}

PolArgs pol_args(const void* history, const double* dm, double* out, double scale, const double* u, const double* w,
                 int64_t group_size, int64_t n_groups, int64_t tiles, int32_t nsurf) {
    return PolArgs{static_cast<const double*>(history), dm, dm + n_groups * (nsurf + 1), out, scale,
                   {u[0], u[1], u[2]}, {w[0], w[1], w[2]}, group_size, n_groups, tiles, nsurf};
}

}  // namespace

int rtpbi::launch_pol_final(const double* partials, double* stats, int64_t n_groups, int64_t blocks, int32_t nsurf,
                            hipStream_t st) {
    const PolFinalArgs a{partials, stats, blocks, nsurf};
    hipLaunchKernelGGL(pol_final_kernel, dim3(static_cast<unsigned>(nsurf), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

int rtpbi::pol_check(const char* call, const double* coatings, int32_t nsurf, const double* polariser,
                     const double* analyser, int32_t q_bits, int64_t group_size) {
    const std::string what(call);
    for (int32_t s = 0; s < nsurf; ++s) {
        const double mode = coatings[kTransCoat * s], value = coatings[kTransCoat * s + 1];
        if (!(mode - mode == 0.0 && value - value == 0.0))
            return fail(RTPB_E_INVALID, what + ": coating " + std::to_string(s) + " is not finite");
        if (mode != kCoatConstant && mode != kCoatFresnel && mode != kCoatMirror)
            return fail(RTPB_E_INVALID, what + ": coating " + std::to_string(s) +
                                            " has a mode that is not 0 (CONSTANT), 1 (FRESNEL) or 2 (MIRROR)");
        if (!(value >= 0.0 && value <= 1.0))
            return fail(RTPB_E_INVALID, what + ": coating " + std::to_string(s) + " has a value outside [0, 1]");
    }
    const double* const axes[2] = {polariser, analyser};
    for (int k = 0; k < 2; ++k) {
        const double* v = axes[k];
        if (!v) continue;
        const bool finite = v[0] - v[0] == 0.0 && v[1] - v[1] == 0.0 && v[2] - v[2] == 0.0;
        if (!finite || (v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0))
            return fail(RTPB_E_INVALID, what + ": the " + (k == 0 ? "polariser" : "analyser") +
                                            " axis is not finite or is zero");
    }
    if (q_bits < 1 || q_bits > kTransMaxQBits)
        return fail(RTPB_E_INVALID, what + ": q_bits must be 1 ... " + std::to_string(kTransMaxQBits));
    if (q_bits > trans_max_q_bits(group_size))
        return fail(RTPB_E_LIMIT, what + ": group_size * 2^q_bits exceeds 2^53 (the sums would not be exact); "
                                         "q_bits at most " + std::to_string(trans_max_q_bits(group_size)));
    return RTPB_OK;
}

extern "C" {

int rtpb_polarisation_stats(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                            int32_t nsurf, const double* media, const double* coatings, const double polariser[3],
                            const double analyser[3], int32_t q_bits, double* workspace, int64_t workspace_len,
                            double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    int rc = pol_history_check("polarisation-stats", dtype, history, group_size, n_groups, nsurf, media, coatings,
                               polariser, stats_out);
    if (rc) return rc;
    if (!workspace || !analyser) return fail(RTPB_E_INVALID, "bad polarisation-stats arguments");
    rc = pol_check("polarisation-stats", coatings, nsurf, polariser, analyser, q_bits, group_size);
    if (rc) return rc;
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (tiles > 0x7fffffffll || n_groups > 65535) return fail(RTPB_E_LIMIT, "polarisation-stats: too many groups");
    if (workspace_len / (int64_t(nsurf) * kPolCols) / tiles < n_groups)
        return fail(RTPB_E_INVALID, "polarisation-stats: workspace too small: need n_groups * ceil(group_size/256) * "
                                    "nsurf * 6 doubles");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    StreamScratch d;
    rc = pol_upload_tables(media, coatings, n_groups, nsurf, st, d);
    if (rc) return rc;
    const PolArgs a = pol_args(history, static_cast<const double*>(d.p), workspace, std::ldexp(1.0, q_bits), polariser,
                               analyser, group_size, n_groups, tiles, nsurf);
    hipLaunchKernelGGL(pol_partial_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    rc = launch_pol_final(workspace, stats_out, n_groups, tiles, nsurf, st);
    if (rc) return rc;
    return d.release();
}

int rtpb_ray_polarisation(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                          int32_t nsurf, const double* media, const double* coatings, const double polariser[3],
                          double* out, void* stream) {
    int rc = pol_history_check("ray-polarisation", dtype, history, group_size, n_groups, nsurf, media, coatings,
                               polariser, out);
    if (rc) return rc;
    rc = pol_check("ray-polarisation", coatings, nsurf, polariser, nullptr, 1, 1);   // (no quantisation here)
    if (rc) return rc;
    if (n_groups > 65535 || group_size > (0x7fffffffll * kBlock) / n_groups)
        return fail(RTPB_E_LIMIT, "ray-polarisation: too many groups or rays");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    StreamScratch d;
    rc = pol_upload_tables(media, coatings, n_groups, nsurf, st, d);
    if (rc) return rc;
    const PolArgs a = pol_args(history, static_cast<const double*>(d.p), out, 0.0, polariser, polariser, group_size,
                               n_groups, 0, nsurf);
    const int64_t blocks = (group_size * n_groups + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ray_pol_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return d.release();
}

}  // extern "C"
