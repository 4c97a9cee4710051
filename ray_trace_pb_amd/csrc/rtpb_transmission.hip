// rtpb_transmission.hip -- the transmission statistics of a stored history (rtpb_transmission_stats: the unfused path,
// and the way to use the feature on a history one already has), the second pass they share with the fused
// transmission sweep (launch_trans_final), each ray's energy weight (rtpb_ray_transmission) and the indices a plan
// traces with (rtpb_plan_media; host only).  The per-ray rule and its combination are rtpb_trans.h's, the wave
// reduction rtpb_stats.h's.
#include "rtpb_stats.h"
#include "rtpb_sweep_host.h"

#include <cstring>

using namespace rtpbi;

namespace {

struct TransArgs {
    const double* __restrict__ hist;        // [1 + 2 nsurf][n_groups * gsize][8]
    const double* __restrict__ media;       // [n_groups][nsurf + 1]
    const double* __restrict__ coat;        // [nsurf][kTransCoat]
    double* __restrict__ out;               // partials [n_groups][tiles][nsurf][kTransCols], or one double per ray
    double scale;                           // 2^q_bits
    int64_t gsize, ngroups, tiles;
    int32_t nsurf;
};

// Ray i of the history at surface s: the rule's step, cum carried by the caller
__device__ __forceinline__ bool trans_step(const TransArgs& a, int64_t i, int64_t g, int s, double& t, double& cum) {
    const int64_t n = a.ngroups * a.gsize;
    const double* A = a.hist + ((2 * s + 1) * n + i) * 8;
    const double* B = A + n * 8;
    const double* m = a.media + g * (a.nsurf + 1) + s;
    const double* c = a.coat + kTransCoat * s;
    return trans_ray(A[0], A[1], A[2], A[3], A[4], A[5], B[0], B[1], B[2], B[3], B[4], B[5], m[0], m[1], c[0], c[1],
                     t, cum);
}

// Block (tile, group): each lane follows its ray through the surfaces in order (cum is a product over them); per
// surface the wave's lanes are combined and lane 0 writes the wave's row -- its own, so the loop holds no barrier --
// and after it the block's threads combine the four waves' rows, as the fused sweep does.
__global__ __launch_bounds__(kBlock) void trans_partial_kernel(TransArgs a) {
    __shared__ double tab[kBlock / 64][RTPB_MAX_SURFACES][kTransCols];
    const int64_t tile = blockIdx.x, g = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t j = tile * kBlock + tid;
    double cum = 1.0;
    for (int s = 0; s < a.nsurf; ++s) {
        TransRay f = trans_none();
        if (j < a.gsize) {
            double t;
            if (trans_step(a, g * a.gsize + j, g, s, t, cum)) f = trans_term(t, cum, a.scale);
        }
        trans_wave_reduce(f);
        if ((tid & 63) == 0) {
#pragma unroll
            for (int c = 0; c < kTransCols; ++c) tab[tid >> 6][s][c] = f.v[c];
        }
    }
    __syncthreads();
    double* out = a.out + (g * a.tiles + tile) * a.nsurf * kTransCols;
    for (int k = tid; k < a.nsurf * kTransCols; k += kBlock) {
        const int s = k / kTransCols, c = k % kTransCols;
        double v = tab[0][s][c];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) v = trans_col(c, v, tab[w][s][c]);
        out[k] = v;
    }
}

// One thread per ray: cum after the last surface, NaN for a ray that does not pass it
__global__ __launch_bounds__(kBlock) void ray_trans_kernel(TransArgs a) {
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= a.ngroups * a.gsize) return;
    const int64_t g = i / a.gsize;
    double cum = 1.0, t;
    for (int s = 0; s < a.nsurf; ++s) trans_step(a, i, g, s, t, cum);
    a.out[i] = cum;
}

struct TransFinalArgs {
    const double* __restrict__ partials;    // [n_groups][blocks][nsurf][kTransCols]
    double* __restrict__ stats;             // [n_groups][nsurf][kTransCols]
    int64_t blocks;
    int32_t nsurf;
};

// Block (surface, group): thread t combines the group's partials t, t + 256, ..., then the wave's lanes and the four
// waves' rows
__global__ __launch_bounds__(kBlock) void trans_final_kernel(TransFinalArgs a) {
    __shared__ double tab[kBlock / 64][kTransCols];
    const int s = blockIdx.x;
    const int64_t g = blockIdx.y;
    const int tid = threadIdx.x;
    TransRay f = trans_none();
    for (int64_t b = tid; b < a.blocks; b += kBlock) {
        const double* p = a.partials + ((g * a.blocks + b) * a.nsurf + s) * kTransCols;
        TransRay o;
#pragma unroll
        for (int c = 0; c < kTransCols; ++c) o.v[c] = p[c];
        trans_merge(f, o);
    }
    trans_wave_reduce(f);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kTransCols; ++c) tab[tid >> 6][c] = f.v[c];
    }
    __syncthreads();
    if (tid < kTransCols) {
        double v = tab[0][tid];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) v = trans_col(tid, v, tab[w][tid]);
        a.stats[(g * a.nsurf + s) * kTransCols + tid] = v;
    }
}

// What rtpb_transmission_stats and rtpb_ray_transmission check before the device (`what` names the call)
int history_check(const std::string& what, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                  int32_t nsurf, const double* media, const double* coatings, const void* out) {
    if (dtype == RTPB_F32)
        return fail(RTPB_E_INVALID, what + ": float64 histories only (the statistics are defined on the float64 "
                                           "history)");
    if (dtype != RTPB_F64) return fail(RTPB_E_INVALID, "bad " + what + " arguments: dtype");
    if (group_size <= 0 || n_groups <= 0 || nsurf <= 0 || !history || !media || !coatings || !out)
        return fail(RTPB_E_INVALID, "bad " + what + " arguments");
    if (nsurf > RTPB_MAX_SURFACES) return fail(RTPB_E_LIMIT, what + ": more than RTPB_MAX_SURFACES surfaces");
    return RTPB_OK;
}

// The media and the coatings: one small stream-ordered upload, media first
int upload_tables(const double* media, const double* coatings, int64_t n_groups, int32_t nsurf, hipStream_t st,
                  StreamScratch& d) {
    const size_t nm = size_t(n_groups) * size_t(nsurf + 1), nc = size_t(nsurf) * kTransCoat;
    const size_t bytes = (nm + nc) * sizeof(double);
    int rc = d.alloc(bytes, st);
    if (rc) return rc;
    PinnedStaging& pin = pinned_staging();
    rc = pin.reserve(bytes);
    if (rc) return rc;
    std::memcpy(pin.buf, media, nm * sizeof(double));
    std::memcpy(pin.buf + nm, coatings, nc * sizeof(double));
    return pin.upload(d.p, bytes, st);
}

}  // namespace

int rtpbi::launch_trans_final(const double* partials, double* stats, int64_t n_groups, int64_t blocks, int32_t nsurf,
                              hipStream_t st) {
    const TransFinalArgs a{partials, stats, blocks, nsurf};
    hipLaunchKernelGGL(trans_final_kernel, dim3(static_cast<unsigned>(nsurf), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

int rtpbi::trans_check(const char* call, const double* coatings, int32_t nsurf, int32_t q_bits, int64_t group_size) {
    const std::string what(call);
    for (int32_t s = 0; s < nsurf; ++s) {
        const double mode = coatings[kTransCoat * s], value = coatings[kTransCoat * s + 1];
        if (!(mode - mode == 0.0 && value - value == 0.0))
            return fail(RTPB_E_INVALID, what + ": coating " + std::to_string(s) + " is not finite");
        if (mode != kCoatConstant && mode != kCoatFresnel)
            return fail(RTPB_E_INVALID, what + ": coating " + std::to_string(s) +
                                            " has a mode that is neither 0 (CONSTANT) nor 1 (FRESNEL)");
        if (!(value >= 0.0 && value <= 1.0))
            return fail(RTPB_E_INVALID, what + ": coating " + std::to_string(s) + " has a value outside [0, 1]");
    }
    if (q_bits < 1 || q_bits > kTransMaxQBits)
        return fail(RTPB_E_INVALID, what + ": q_bits must be 1 ... " + std::to_string(kTransMaxQBits));
    if (q_bits > trans_max_q_bits(group_size))
        return fail(RTPB_E_LIMIT, what + ": group_size * 2^q_bits exceeds 2^53 (the sums would not be exact); "
                                         "q_bits at most " + std::to_string(trans_max_q_bits(group_size)));
    return RTPB_OK;
}

int rtpbi::trans_plan_check(const char* call, const rtpb_plan* plan) {
    if (plan && (plan->feat & 2) != 0)
        return fail(RTPB_E_INVALID, std::string(call) + ": POLY6 media are not host-evaluated; lower it as RTPB_TABLE");
    return RTPB_OK;
}

extern "C" {

int rtpb_transmission_stats(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                            int32_t nsurf, const double* media, const double* coatings, int32_t q_bits,
                            double* workspace, int64_t workspace_len, double* stats_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    int rc = history_check("transmission-stats", dtype, history, group_size, n_groups, nsurf, media, coatings,
                           stats_out);
    if (rc) return rc;
    if (!workspace) return fail(RTPB_E_INVALID, "bad transmission-stats arguments");
    rc = trans_check("transmission-stats", coatings, nsurf, q_bits, group_size);
    if (rc) return rc;
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (tiles > 0x7fffffffll || n_groups > 65535) return fail(RTPB_E_LIMIT, "transmission-stats: too many groups");
    if (workspace_len / (int64_t(nsurf) * kTransCols) / tiles < n_groups)
        return fail(RTPB_E_INVALID, "transmission-stats: workspace too small: need n_groups * ceil(group_size/256) * "
                                    "nsurf * 5 doubles");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    StreamScratch d;
    rc = upload_tables(media, coatings, n_groups, nsurf, st, d);
    if (rc) return rc;
    const double* dm = static_cast<const double*>(d.p);
    const TransArgs a{static_cast<const double*>(history), dm, dm + n_groups * (nsurf + 1), workspace,
                      std::ldexp(1.0, q_bits), group_size, n_groups, tiles, nsurf};
    hipLaunchKernelGGL(trans_partial_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups)),
                       dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    rc = launch_trans_final(workspace, stats_out, n_groups, tiles, nsurf, st);
    if (rc) return rc;
    return d.release();
}

int rtpb_ray_transmission(int32_t device, int32_t dtype, const void* history, int64_t group_size, int64_t n_groups,
                          int32_t nsurf, const double* media, const double* coatings, double* out, void* stream) {
    int rc = history_check("ray-transmission", dtype, history, group_size, n_groups, nsurf, media, coatings, out);
    if (rc) return rc;
    rc = trans_check("ray-transmission", coatings, nsurf, 1, 1);       // (no quantisation here: the coatings only)
    if (rc) return rc;
    if (n_groups > 65535 || group_size > (0x7fffffffll * kBlock) / n_groups)
        return fail(RTPB_E_LIMIT, "ray-transmission: too many groups or rays");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    StreamScratch d;
    rc = upload_tables(media, coatings, n_groups, nsurf, st, d);
    if (rc) return rc;
    const double* dm = static_cast<const double*>(d.p);
    const TransArgs a{static_cast<const double*>(history), dm, dm + n_groups * (nsurf + 1), out, 0.0, group_size,
                      n_groups, 0, nsurf};
    const int64_t blocks = (group_size * n_groups + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(ray_trans_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return d.release();
}

int rtpb_plan_media(const rtpb_plan* plan, const double* wavelengths, int64_t n, double* out) {
    if (!plan) return fail(RTPB_E_INVALID, "plan is NULL");
    if (!wavelengths || !out || n <= 0) return fail(RTPB_E_INVALID, "bad plan-media arguments");
    if (plan->dtype != RTPB_F64)
        return fail(RTPB_E_INVALID, "plan-media: float64 plans only (a float32 sweep rounds the wavelengths)");
    int rc = trans_plan_check("plan-media", plan);
    if (rc) return rc;
    // fill_group_media: the sweep's own table, of which the indices are the first nsurf + 1 doubles per group
    const size_t M = size_t(plan->nsurf) + 1, row = M + 3 * (M - 1);
    std::vector<DevMaterial<double>> dm(M);
    for (size_t k = 0; k < M; ++k) dm[k] = device_material(*plan, k);
    std::vector<double> params(size_t(n) * 4, 0.0), table(size_t(n) * row);
    for (int64_t i = 0; i < n; ++i) params[size_t(i) * 4 + 3] = wavelengths[i];
    fill_group_media(dm.data(), M, plan->table.data(), params.data(), n, RTPB_F64, table.data());
    for (int64_t i = 0; i < n; ++i)
        std::memcpy(out + size_t(i) * M, table.data() + size_t(i) * row, M * sizeof(double));
    return RTPB_OK;
}

}  // extern "C"
