// CPU harness of the wavefront map's per-ray rule (ray_trace_pb_amd/csrc/rtpb_wavemap.h: wave_ray, image_bin,
// wavemap_ray, wavemap_bound), built with g++ -ffp-contract=off by tests/wavemap_harness.py.  TEST INFRASTRUCTURE ONLY.
#include "../../ray_trace_pb_amd/csrc/rtpb_wavemap.h"

using namespace rtpb;

extern "C" {

// plane: [n_groups * group_size][8] float64; refs: [n_groups][8]; windows: [n_groups][4]; count, sum:
// [n_groups][ny][nx]; outside, clipped: [n_groups]; farthest: [n_groups][2].  The rays of a group one after another.
int wavemap_harness_map(const double* plane, int64_t group_size, int64_t n_groups, const double* refs,
                        const double* windows, int32_t nx, int32_t ny, int32_t q_bits, double w_lim, int32_t* count,
                        int64_t* sum, int32_t* outside, int32_t* clipped, double* farthest) {
    const double scale = std::ldexp(1.0, q_bits);
    const int64_t cells = int64_t(nx) * ny;
    for (int64_t g = 0; g < n_groups; ++g) {
        const double* q = refs + kWaveRef * g;
        const double* v = windows + kMapWin * g;
        const double ref[kWaveRef] = {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7]};
        const double win[kMapWin] = {v[0], v[1], v[2], v[3]};
        for (int64_t c = 0; c < cells; ++c) count[g * cells + c] = 0, sum[g * cells + c] = 0;
        outside[g] = clipped[g] = 0;
        farthest[2 * g] = farthest[2 * g + 1] = 0.0;
        for (int64_t j = 0; j < group_size; ++j) {
            const double* r = plane + (g * group_size + j) * 8;
            const MapRay m = wavemap_ray(wave_ray(r[0], r[1], r[2], r[3], r[4], r[5], r[6], ref), win, nx, ny, scale,
                                         w_lim);
            if (m.far_e > farthest[2 * g]) farthest[2 * g] = m.far_e;
            if (m.far_w > farthest[2 * g + 1]) farthest[2 * g + 1] = m.far_w;
            if (m.bin == kImageOutside) outside[g] += 1;
            else if (m.bin == kMapClipped) clipped[g] += 1;
            else if (m.bin >= 0) {
                if (m.bin >= cells) return 1;
                count[g * cells + m.bin] += 1;
                sum[g * cells + m.bin] += m.q;
            }
        }
    }
    return 0;
}

int wavemap_harness_bound(int32_t q_bits, double w_lim, int64_t group_size) {
    return wavemap_bound(q_bits, w_lim, group_size);
}

}  // extern "C"
