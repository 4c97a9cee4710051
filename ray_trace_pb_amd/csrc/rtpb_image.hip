// rtpb_image.hip -- the spot image of a stored plane (rtpb_spot_image): per group, a 2-D histogram of the final
// positions.  The contribution rule and the wave's aggregated adds are rtpb_stats.h, shared with the fused sweep's
// image mode (rtpb_sweep.hip).
#include "rtpb_stats.h"

using namespace rtpbi;

namespace {

struct ImageArgs {
    const void* __restrict__ plane;
    const double* __restrict__ windows;   // per group: x_lo, y_lo, x_scale, y_scale
    int32_t* __restrict__ image;          // [ngroups][ny][nx]
    int32_t* __restrict__ outside;        // [ngroups]
    int64_t gsize;
    int32_t nx, ny;
};

// spot_partial_kernel's grid: block (tile, g) covers rays 256 tile ... of group g, one ray per lane.  Lanes past the
// group's end carry kImageSkip, so whole waves reach wave_image_add.
template <typename T>
__global__ __launch_bounds__(kBlock) void spot_image_kernel(ImageArgs a) {
    const int64_t g = blockIdx.y;
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    int bin = kImageSkip;
    if (j < a.gsize) {
        const T* r = static_cast<const T*>(a.plane) + (g * a.gsize + j) * 8;
        const double w[4] = {a.windows[4 * g], a.windows[4 * g + 1], a.windows[4 * g + 2], a.windows[4 * g + 3]};
        bin = image_bin(r[0], r[1], w, a.nx, a.ny);
    }
    wave_image_add(bin, a.image + g * a.ny * a.nx, a.outside + g);
}

}  // namespace

int rtpbi::image_check(const char* call, int32_t nx, int32_t ny, int64_t group_size, int64_t n_groups,
                       const void* windows, const void* image_out, const void* outside_out) {
    if (nx <= 0 || ny <= 0 || group_size <= 0 || n_groups <= 0 || !windows || !image_out || !outside_out)
        return fail(RTPB_E_INVALID, std::string("bad ") + call + " arguments");
    if (nx > RTPB_MAX_IMAGE_SIDE || ny > RTPB_MAX_IMAGE_SIDE)
        return fail(RTPB_E_LIMIT, std::string(call) + ": nx and ny are at most RTPB_MAX_IMAGE_SIDE (4096)");
    if (group_size > 0x7fffffffll)
        return fail(RTPB_E_LIMIT, std::string(call) + ": more than 2^31 - 1 rays per group (the counters are int32)");
    return RTPB_OK;
}

int rtpbi::image_clear(int32_t* image_out, int32_t* outside_out, int64_t n_groups, int32_t nx, int32_t ny,
                       hipStream_t st) {
    HIP_TRY(hipMemsetAsync(image_out, 0, size_t(n_groups) * size_t(ny) * size_t(nx) * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(outside_out, 0, size_t(n_groups) * sizeof(int32_t), st));
    return RTPB_OK;
}

extern "C" {

int rtpb_spot_image(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                    const double* windows, int32_t nx, int32_t ny, int32_t* image_out, int32_t* outside_out,
                    void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (dtype != RTPB_F64 && dtype != RTPB_F32) return fail(RTPB_E_INVALID, "bad spot-image arguments: dtype");
    if (!plane) return fail(RTPB_E_INVALID, "bad spot-image arguments");
    int rc = image_check("spot-image", nx, ny, group_size, n_groups, windows, image_out, outside_out);
    if (rc) return rc;
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, "spot-image: too many groups");
    rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = image_clear(image_out, outside_out, n_groups, nx, ny, st);
    if (rc) return rc;
    const ImageArgs a{plane, windows, image_out, outside_out, group_size, nx, ny};
    const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>(n_groups));
    if (dtype == RTPB_F64) hipLaunchKernelGGL(spot_image_kernel<double>, grid, dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(spot_image_kernel<float>, grid, dim3(kBlock), 0, st, a);
    HIP_TRY(hipGetLastError());
    return RTPB_OK;
}

}  // extern "C"
