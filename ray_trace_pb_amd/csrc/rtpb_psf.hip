// rtpb_psf.hip -- the Huygens point-spread function of a stored plane (rtpb_huygens_psf): per group, the coherent sum
// of the rays' plane wavelets on a grid of image-plane pixels about the group's reference point.  The contribution
// rule is rtpb_stats.h (psf_ray, psf_frac: wave_ray's OPD and direction offset, nothing new about a ray).
//
// The work is rays x pixels double-precision sincospi per group, so the kernel is bound by the float64 VALU and not by
// memory: a block is 256 pixels of one group, one per thread, and the group's rays pass through LDS in tiles of 256 --
// each thread loads one ray, reduces it to (a, w, qx, qy) once, and every thread then walks the tile in ray order.  All
// lanes read the same 32 bytes of a tile entry (reads of one address: a broadcast, no bank conflict), so a ray costs
// each pixel two or three LDS reads beside the seventy-odd VALU operations of its phase, sine and cosine.
//
// A window of a few thousand pixels is a few dozen blocks a group, too few to fill the device (65 x 65 pixels ran at a
// third of the rate of 257 x 257: one wave a SIMD, every dependent float64 operation waiting for the one before), so
// the rays of a group are split into SEGMENTS of whole tiles, a block per (pixel block, segment), and a second kernel
// adds a pixel's partial sums in segment order.  The split is psf_split(group_size, nx, ny) and nothing else, so the
// order of every addition is fixed by those three numbers: no atomics, the same bits from every call.
#include "rtpb_stats.h"

#include <algorithm>
#include <cstring>

using namespace rtpbi;

namespace {

struct PsfArgs {
    const double* __restrict__ plane;      // the first group of this launch
    const double* __restrict__ refwin;     // per group: the reference (8), then the window cx, cy, sx, sy (4)
    const double* __restrict__ weights;    // group_size doubles, or NULL
    double* __restrict__ field;            // nseg == 1: [groups][ny][nx][2]; else the partials [groups][nseg][ny][nx][2]
    double* __restrict__ norm;             // nseg == 1: [groups]; else the partials [groups][nseg]
    int64_t gsize;
    int32_t nx, ny;
    int32_t nseg, seg_tiles;               // segments a group, tiles (of 256 rays) a segment
};

constexpr int kPsfGroupDoubles = kWaveRef + 4;
// the blocks a group is spread over, where its rays allow: four waves on each of the 1024 SIMDs
constexpr int64_t kPsfBlocksPerGroup = 1024;
// the partial sums held at a time, in doubles (256 MiB): more groups than that go in several launches
constexpr int64_t kPsfPartialDoubles = int64_t(1) << 25;

// The split of a group's rays: seg_tiles tiles of 256 rays a segment, nseg segments, none empty.  A function of
// (group_size, nx, ny) alone -- not of the number of groups, nor of the device.
struct PsfSplit {
    int32_t nseg, seg_tiles;
};
PsfSplit psf_split(int64_t group_size, int32_t nx, int32_t ny) {
    const int64_t tiles = (group_size + kBlock - 1) / kBlock;
    const int64_t pblocks = (static_cast<int64_t>(nx) * ny + kBlock - 1) / kBlock;
    const int64_t want = std::min(tiles, std::max<int64_t>(1, kPsfBlocksPerGroup / pblocks));
    const int64_t seg_tiles = (tiles + want - 1) / want;
    return PsfSplit{static_cast<int32_t>((tiles + seg_tiles - 1) / seg_tiles), static_cast<int32_t>(seg_tiles)};
}

// NORM: the block also sums a over its segment's counting rays, in the same ray order (the first pixel block of each
// segment: its thread 0 stores the sum).  Every thread of the block takes every barrier: threads past the last pixel
// compute pixel 0's coordinates and store nothing.
template <bool NORM>
__device__ __forceinline__ void psf_block(const PsfArgs& a, PsfRay* tile) {
    const int64_t g = blockIdx.z, seg = blockIdx.y;
    const int t = threadIdx.x;
    const double* q = a.refwin + kPsfGroupDoubles * g;
    const double ref[kWaveRef] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
    const int64_t npix = static_cast<int64_t>(a.nx) * a.ny;
    const int64_t pix = static_cast<int64_t>(blockIdx.x) * kBlock + t;
    const int64_t p = pix < npix ? pix : 0;
    const double X = (static_cast<double>(p % a.nx) - q[8]) * q[10];
    const double Y = (static_cast<double>(p / a.nx) - q[9]) * q[11];
    const int64_t first = seg * a.seg_tiles * kBlock;
    const int64_t seg_rays = static_cast<int64_t>(a.seg_tiles) * kBlock;
    const int64_t last = a.gsize - first < seg_rays ? a.gsize : first + seg_rays;     // (first < gsize: no empty segment)
    double re = 0.0, im = 0.0, nrm = 0.0;
    for (int64_t j0 = first; j0 < last; j0 += kBlock) {
        const int64_t j = j0 + t;
        if (j < last) {
            const double* r = a.plane + (g * a.gsize + j) * 8;
            tile[t] = psf_ray(r[0], r[1], r[2], r[3], r[4], r[5], r[6], ref, a.weights ? a.weights[j] : 1.0);
        }
        __syncthreads();
        const int n = static_cast<int>(last - j0 < kBlock ? last - j0 : kBlock);
        for (int k = 0; k < n; ++k) {
            const PsfRay f = tile[k];
            if (!psf_counts(f)) continue;           // (the same ray for every thread: the whole block skips it)
            double s, c;
            sincospi(2.0 * psf_frac(f, X, Y), &s, &c);
            re += f.a * c;
            im += f.a * s;
            if (NORM) nrm += f.a;
        }
        __syncthreads();
    }
    const int64_t slot = g * a.nseg + seg;          // (nseg == 1: the group's place in the outputs themselves)
    if (pix < npix) {
        double* o = a.field + (slot * npix + pix) * 2;
        o[0] = re;
        o[1] = im;
    }
    if (NORM && t == 0) a.norm[slot] = nrm;
}

__global__ __launch_bounds__(kBlock) void huygens_psf_kernel(PsfArgs a) {
    __shared__ PsfRay tile[kBlock];
    if (blockIdx.x == 0) psf_block<true>(a, tile);
    else psf_block<false>(a, tile);
}

// The second pass of a split group: element e of its 2 * ny * nx field doubles is the sum of the segments' partials
// 0, 1, ..., nseg - 1 in that order, and so is the norm (thread 0 of the group's first block).
__global__ __launch_bounds__(kBlock) void psf_final_kernel(const double* __restrict__ part_field,
                                                           const double* __restrict__ part_norm,
                                                           double* __restrict__ field, double* __restrict__ norm,
                                                           int64_t elems, int32_t nseg) {
    const int64_t g = blockIdx.y;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e < elems) {
        const double* p = part_field + g * nseg * elems + e;
        double v = p[0];
        for (int s = 1; s < nseg; ++s) v += p[s * elems];
        field[g * elems + e] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double v = part_norm[g * nseg];
        for (int s = 1; s < nseg; ++s) v += part_norm[g * nseg + s];
        norm[g] = v;
    }
}

}  // namespace

extern "C" {

int rtpb_huygens_psf(int32_t device, int32_t dtype, const void* plane, int64_t group_size, int64_t n_groups,
                     const double* refs, const double* windows, const double* weights, int32_t nx, int32_t ny,
                     double* field_out, double* norm_out, void* stream) {
    // (the arguments first: a bad call is RTPB_E_INVALID / RTPB_E_LIMIT with or without a GPU)
    if (dtype == RTPB_F32)
        return fail(RTPB_E_INVALID, "huygens-psf: float64 planes only (a float32 phase of 1e4 ... 1e7 rad has an "
                                    "ulp of a milliradian to a radian: its wavefront is noise)");
    if (dtype != RTPB_F64) return fail(RTPB_E_INVALID, "bad huygens-psf arguments: dtype");
    if (nx <= 0 || ny <= 0 || group_size <= 0 || n_groups <= 0 || !plane || !refs || !windows || !field_out ||
        !norm_out)
        return fail(RTPB_E_INVALID, "bad huygens-psf arguments");
    if (nx > RTPB_MAX_PSF_SIDE || ny > RTPB_MAX_PSF_SIDE)
        return fail(RTPB_E_LIMIT, "huygens-psf: nx and ny are at most RTPB_MAX_PSF_SIDE (2048)");
    if (n_groups > 65535) return fail(RTPB_E_LIMIT, "huygens-psf: too many groups");
    int rc = check_device(device);
    if (rc) return rc;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the references and the windows: one small stream-ordered upload, a group's twelve doubles together
    const size_t bytes = size_t(n_groups) * kPsfGroupDoubles * sizeof(double);
    StreamScratch drw;
    rc = drw.alloc(bytes, st);
    if (rc) return rc;
    PinnedStaging& pin = pinned_staging();
    rc = pin.reserve(bytes);
    if (rc) return rc;
    for (int64_t k = 0; k < n_groups; ++k) {
        std::memcpy(pin.buf + kPsfGroupDoubles * k, refs + kWaveRef * k, kWaveRef * sizeof(double));
        std::memcpy(pin.buf + kPsfGroupDoubles * k + kWaveRef, windows + 4 * k, 4 * sizeof(double));
    }
    rc = pin.upload(drw.p, bytes, st);
    if (rc) return rc;
    const PsfSplit sp = psf_split(group_size, nx, ny);
    const int64_t elems = static_cast<int64_t>(nx) * ny * 2;
    const unsigned pblocks = static_cast<unsigned>((elems / 2 + kBlock - 1) / kBlock);          // <= 16384
    const double* const dplane = static_cast<const double*>(plane);
    const double* const drefwin = static_cast<const double*>(drw.p);
    if (sp.nseg == 1) {
        const PsfArgs a{dplane, drefwin, weights, field_out, norm_out, group_size, nx, ny, 1, sp.seg_tiles};
        hipLaunchKernelGGL(huygens_psf_kernel, dim3(pblocks, 1, static_cast<unsigned>(n_groups)), dim3(kBlock), 0, st,
                           a);
        HIP_TRY(hipGetLastError());
        return drw.release();
    }
    // split groups: the partials of as many groups at a time as kPsfPartialDoubles holds, then their second pass
    const int64_t group_doubles = sp.nseg * (elems + 1);
    const int64_t chunk = std::max<int64_t>(1, std::min(n_groups, kPsfPartialDoubles / group_doubles));
    StreamScratch part;
    rc = part.alloc(size_t(chunk) * size_t(group_doubles) * sizeof(double), st);
    if (rc) return rc;
    double* const part_field = static_cast<double*>(part.p);
    double* const part_norm = part_field + chunk * sp.nseg * elems;
    for (int64_t g0 = 0; g0 < n_groups; g0 += chunk) {
        const unsigned ng = static_cast<unsigned>(std::min(chunk, n_groups - g0));
        const PsfArgs a{dplane + g0 * group_size * 8, drefwin + g0 * kPsfGroupDoubles, weights, part_field, part_norm,
                        group_size, nx, ny, sp.nseg, sp.seg_tiles};
        hipLaunchKernelGGL(huygens_psf_kernel, dim3(pblocks, static_cast<unsigned>(sp.nseg), ng), dim3(kBlock), 0, st,
                           a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(psf_final_kernel, dim3(static_cast<unsigned>((elems + kBlock - 1) / kBlock), ng),
                           dim3(kBlock), 0, st, part_field, part_norm, field_out + g0 * elems, norm_out + g0, elems,
                           sp.nseg);
        HIP_TRY(hipGetLastError());
    }
    rc = part.release();
    if (rc) return rc;
    return drw.release();
}

}  // extern "C"
