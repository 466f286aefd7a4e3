// rt_aa.h — the colour-edge criterion of adaptive anti-aliasing
// (rt_render_aa*, rt_aa_edge_mask; include/rt.h). One text for the edge kernel
// (rt_kernel.hip aa_edge_kernel) and the host's rt_aa_edge_mask (rt_api.cpp):
// the subtraction, the absolute value, the maximum and the comparison are
// written here and nowhere else. All float32.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rtamd {

#define RT_AA_HD __host__ __device__ __forceinline__

// Pixels p and q (float4 records, rgb in the first three words) differ:
// max over the channels of |p[c] - q[c]| exceeds the threshold. The maximum
// is IEEE maxNum (fmaxf on either side), so a channel whose difference is NaN
// drops out and a pair all of whose differences are NaN does not differ; an
// infinite difference does, for every threshold below +inf. Symmetric in p, q.
RT_AA_HD bool aa_pair_differs(const float *p, const float *q, float threshold) {
    const float dr = fabsf(p[0] - q[0]), dg = fabsf(p[1] - q[1]), db = fabsf(p[2] - q[2]);
    return fmaxf(fmaxf(dr, dg), db) > threshold;
}

// Pixel (x, y) of a width x height frame of float4 records is flagged: some
// 4-neighbour inside the frame differs from it. The caller has (x, y) inside.
RT_AA_HD bool aa_pixel_flagged(const float *frame, int width, int height, int x, int y, float threshold) {
    const size_t at = static_cast<size_t>(y) * static_cast<size_t>(width) + static_cast<size_t>(x);
    const size_t row = static_cast<size_t>(width);
    const float *p = frame + 4 * at;
    bool f = false;
    if (x > 0) f = f || aa_pair_differs(p, frame + 4 * (at - 1), threshold);
    if (x + 1 < width) f = f || aa_pair_differs(p, frame + 4 * (at + 1), threshold);
    if (y > 0) f = f || aa_pair_differs(p, frame + 4 * (at - row), threshold);
    if (y + 1 < height) f = f || aa_pair_differs(p, frame + 4 * (at + row), threshold);
    return f;
}

// Wave tiles (the render kernels' 8 x 8 units) per frame row, and work-group
// tiles (2 x 2 wave tiles) per frame row and column.
RT_AA_HD int aa_tiles_x(int width) { return (width + 7) / 8; }
RT_AA_HD int aa_tiles_y(int height) { return (height + 7) / 8; }
RT_AA_HD int aa_groups_x(int width) { return (width + 15) / 16; }
RT_AA_HD int aa_groups_y(int height) { return (height + 15) / 16; }
// Where the device keeps wave tile (wx, wy)'s mask: the four masks of a
// work-group tile side by side (32 B, one scalar load), its waves' order
// (wave w at (w % 2, w / 2)). Tiles of the last work-group column / row past
// the frame have a slot too (mask 0).
RT_AA_HD size_t aa_mask_slot(int width, int wx, int wy) {
    const size_t group = static_cast<size_t>(wy >> 1) * static_cast<size_t>(aa_groups_x(width)) + static_cast<size_t>(wx >> 1);
    return group * 4 + static_cast<size_t>((wy & 1) * 2 + (wx & 1));
}

}  // namespace rtamd
