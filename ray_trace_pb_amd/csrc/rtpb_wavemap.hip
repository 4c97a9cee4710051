// rtpb_wavemap.hip -- the wavefront map of a stored plane (rtpb_wavefront_map): per group, the optical path difference
// over the exit pupil as integer cell sums and counts, the rays outside the window and past the limit, and the two
// maxima that say which window and limit hold everything.  The contribution rule is rtpb_wavemap.h, the wave's
// aggregated adds rtpb_stats.h, both shared with the fused sweep's map mode (rtpb_sweep_wavemap.hip); the argument
// checks and the clears of both live here.
#include "rtpb_stats.h"

using namespace rtpbi;

namespace {

struct WaveMapArgs {
    const double* __restrict__ plane;
    const double* __restrict__ par;       // per group: the reference (kWaveRef), then the window (kMapWin)
    int32_t* __restrict__ count;          // [ngroups][ny][nx]
    long long* __restrict__ sum;          // [ngroups][ny][nx]
    int32_t* __restrict__ outside;        // [ngroups]
    int32_t* __restrict__ clipped;        // [ngroups]
    double* __restrict__ farthest;        // [ngroups][2]
    int64_t gsize;
    double scale, w_lim;                  // scale = 2^q_bits
    int32_t nx, ny;
};

// spot_energy_kernel's grid: block (tile, g) covers rays 256 tile ... of group g, one ray per lane.  Lanes past the
// group's end carry kImageSkip and +0, so whole waves reach wave_map_add.
__global__ __launch_bounds__(kBlock) void wavefront_map_kernel(WaveMapArgs a) {
    const int64_t g = blockIdx.y;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    MapRay m{kImageSkip, 0, 0.0, 0.0};
    if (j < a.gsize) {
        const double* r = a.plane + (g * a.gsize + j) * 8;
        const double* q = a.par + (kWaveRef + kMapWin) * g;
        const double ref[kWaveRef] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
        const double win[kMapWin] = {q[8], q[9], q[10], q[11]};
        m = wavemap_ray(wave_ray(r[0], r[1], r[2], r[3], r[4], r[5], r[6], ref), win, a.nx, a.ny, a.scale, a.w_lim);
    }
    const int64_t cells = int64_t(a.ny) * a.nx;
    wave_map_add(m, a.count + g * cells, a.sum + g * cells, a.outside + g, a.clipped + g, a.farthest + 2 * g);
}

}  // namespace

int rtpbi::wavemap_check(const char* call, int32_t nx, int32_t ny, int32_t q_bits, double w_lim, int64_t group_size,
                         int64_t n_groups, const void* refs, const void* windows, const void* count_out,
                         const void* sum_out, const void* outside_out, const void* clipped_out,
                         const void* farthest_out) {
    if (nx <= 0 || ny <= 0 || group_size <= 0 || n_groups <= 0 || !refs || !windows || !count_out || !sum_out ||
        !outside_out || !clipped_out || !farthest_out)
        return fail(RTPB_E_INVALID, std::string("bad ") + call + " arguments");
    if (nx > RTPB_MAX_IMAGE_SIDE || ny > RTPB_MAX_IMAGE_SIDE)
        return fail(RTPB_E_LIMIT, std::string(call) + ": nx and ny are at most RTPB_MAX_IMAGE_SIDE (4096)");
    // (before the bound below: it divides by the group's size)
    const int bound = wavemap_bound(q_bits, w_lim, group_size);
    if (bound == 1)
        return fail(RTPB_E_INVALID, std::string(call) + ": q_bits must be 0 ... 52 and w_lim finite and >= 0");
    if (group_size > 0x7fffffffll)
        return fail(RTPB_E_LIMIT, std::string(call) + ": more than 2^31 - 1 rays per group (the counters are int32)");
    if (bound)
        return fail(RTPB_E_LIMIT, std::string(call) + ": a cell's sum could leave int64: need ldexp(w_lim, q_bits) + 1 "
                                                      "<= 2^62 / rays per group; lower q_bits");
    return RTPB_OK;
}

int rtpbi::wavemap_clear(int32_t* count_out, long long* sum_out, int32_t* outside_out, int32_t* clipped_out,
                         double* farthest_out, int64_t n_groups, int32_t nx, int32_t ny, hipStream_t st) {
    const size_t cells = size_t(n_groups) * size_t(ny) * size_t(nx);
    HIP_TRY(hipMemsetAsync(count_out, 0, cells * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(sum_out, 0, cells * sizeof(long long), st));
    HIP_TRY(hipMemsetAsync(outside_out, 0, size_t(n_groups) * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(clipped_out, 0, size_t(n_groups) * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(farthest_out, 0, size_t(n_groups) * 2 * sizeof(double), st));     // (+0.0 is all zero bits)
    return RTPB_OK;
}

extern "C" {

int rtpb_wavefront_map(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                       const double* refs, const double* windows, int32_t nx, int32_t ny, int32_t q_bits,
                       double w_lim, int32_t* count_out, int64_t* sum_out, int32_t* outside_out, int32_t* clipped_out,
                       double* farthest_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (dtype == RTPB_F32)
        return fail(RTPB_E_INVALID, "wavefront-map: float64 planes only (a float32 phase of 1e4 ... 1e7 rad has an "
                                    "ulp of a milliradian to a radian: its wavefront is noise)");
    if (dtype != RTPB_F64) return fail(RTPB_E_INVALID, "bad wavefront-map arguments: dtype");
    if (!plane) return fail(RTPB_E_INVALID, "bad wavefront-map arguments");
    int rc = wavemap_check("wavefront-map", nx, ny, q_bits, w_lim, group_size, n_groups, refs, windows, count_out,
                           sum_out, outside_out, clipped_out, farthest_out);
    if (rc) return rc;
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, "wavefront-map: too many groups");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long* const sum = reinterpret_cast<long long*>(sum_out);
    rc = wavemap_clear(count_out, sum, outside_out, clipped_out, farthest_out, n_groups, nx, ny, st);
    if (rc) return rc;
    // the references and windows: one small stream-ordered upload, as rtpb_wavefront_stats' references
    constexpr int kPar = kWaveRef + kMapWin;
    const size_t bytes = size_t(n_groups) * kPar * sizeof(double);
    StreamScratch dpar;
    rc = dpar.alloc(bytes, st);
    if (rc) return rc;
    PinnedStaging& pin = pinned_staging();
    rc = pin.reserve(bytes);
    if (rc) return rc;
    for (int64_t gi = 0; gi < n_groups; ++gi) {
        std::memcpy(pin.buf + kPar * gi, refs + kWaveRef * gi, kWaveRef * sizeof(double));
        std::memcpy(pin.buf + kPar * gi + kWaveRef, windows + kMapWin * gi, kMapWin * sizeof(double));
    }
    rc = pin.upload(dpar.p, bytes, st);
    if (rc) return rc;
    const WaveMapArgs a{static_cast<const double*>(plane), static_cast<const double*>(dpar.p), count_out, sum,
                        outside_out, clipped_out, farthest_out, group_size, std::ldexp(1.0, q_bits), w_lim, nx, ny};
    hipLaunchKernelGGL(wavefront_map_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return dpar.release();
}

}  // extern "C"
