// rt_cull.h — what the scene builder derives from one object: a box's record
// and the data that let a shadow ray skip an object (light_inside, bounding
// ball, separating plane, ShadowCone, mask cone and texel test, BVH box).
// One text for build_scene / build_direction_masks / build_bvh (rt_scene.cpp),
// the animate kernel (rt_anim.hip) and its host run (anim_apply_*_host): every
// inequality and margin is written here and nowhere else. The callers keep
// their loops, the scene-wide `finite` flag and the words of a record that do
// not depend on the object's placement. The culling terms are float64; all of
// them err to the conservative side, so culling changes no pixel.
#pragma once

#include <cmath>

#include "rt_glmath.h"
#include "rt_internal.h"

namespace rtamd {

// (forced inlining, as rt_glmath.h: the animate kernel keeps its registers
// only while every call folds into its caller)
#define RT_HD __host__ __device__ __forceinline__

// The words of a BoxRec that follow from the object's placement and extents:
// the reference GL's transform chain (rt_glmath.h; float32, bit-identical on
// host and device) stored row-major, mins / maxs, w2l_w0 (the kernel adds it
// as is) and translate_only. obj_index, material, light_inside and the
// padding are the caller's.
RT_HD void box_record(const rt_object &o, BoxRec &rec) {
    float L[16], W[16], N[9];
    glf::box_transforms(o.position, o.angles, L, W, N);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            rec.w2l[r * 4 + c] = W[c * 4 + r];
            rec.l2w[r * 4 + c] = L[c * 4 + r];
        }
    // the normal matrix transpose(inverse(mat3(L)))
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) rec.nrm[r * 3 + c] = N[c * 3 + r];
    int translate_only = 1;
    for (int r = 0; r < 3; ++r) {
        rec.mins[r] = o.box_mins[r];
        rec.maxs[r] = o.box_maxs[r];
        rec.w2l_w0[r] = W[12 + r] * 0.0f;
        for (int c = 0; c < 3; ++c)
            if (W[c * 4 + r] != (r == c ? 1.0f : 0.0f)) translate_only = 0;
    }
    rec.translate_only = translate_only;
}

// An object's rotation in float64, R[col][row] (culling only): Rz(yaw)
// Rx(pitch) Ry(roll) (:492-503), each angle the float DEG_TO_RAD * deg the
// shader forms.
RT_HD void rotation64(const float ang[3], double R[3][3]) {
    auto rot = [](int axis, float deg, double r[3][3]) {
        const double a = static_cast<double>(glf::kDegToRad * deg);
        double c, s;
#ifdef __HIP_DEVICE_COMPILE__
        sincos(a, &s, &c);
#else
        c = std::cos(a);
        s = std::sin(a);
#endif
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) r[i][j] = i == j ? 1.0 : 0.0;
        if (axis == 0) { r[1][1] = c; r[1][2] = s; r[2][1] = -s; r[2][2] = c; }
        if (axis == 1) { r[0][0] = c; r[0][2] = -s; r[2][0] = s; r[2][2] = c; }
        if (axis == 2) { r[0][0] = c; r[0][1] = s; r[1][0] = -s; r[1][1] = c; }
    };
    auto mul = [](const double a[3][3], const double b[3][3], double r[3][3]) {
        for (int c = 0; c < 3; ++c)
            for (int w = 0; w < 3; ++w) r[c][w] = a[0][w] * b[c][0] + a[1][w] * b[c][1] + a[2][w] * b[c][2];
    };
    double z[3][3], x[3][3], y[3][3], zx[3][3];
    rot(2, ang[1], z);
    rot(0, ang[0], x);
    rot(1, ang[2], y);
    mul(z, x, zx);
    mul(zx, y, R);
}

// light_inside: the light lies strictly inside the box by a margin. A shadow
// segment that starts inside the box then ends inside it too (its end is the
// light + 0.01 n, :808-809), so the box cannot occlude it. The light in the
// box's frame: the transposed (= inverse) rotation of light - position.
RT_HD bool light_inside_box(const rt_object &o, const double R[3][3], const float light[3]) {
    const double d[3] = {double(light[0]) - double(o.position[0]), double(light[1]) - double(o.position[1]),
                         double(light[2]) - double(o.position[2])};
    bool in = true;
    for (int r = 0; r < 3; ++r) {
        const double lp = R[r][0] * d[0] + R[r][1] * d[1] + R[r][2] * d[2];
        const double m = 0.05 + 1e-4 * (fabs(double(o.box_mins[r])) + fabs(double(o.box_maxs[r])) + fabs(lp));
        in = in && std::isfinite(lp) && double(o.box_mins[r]) + m < lp && lp < double(o.box_maxs[r]) - m;
    }
    return in;
}

// The ball that carries a box's mask bit: (centre, radius). A box that can
// occlude a shadow segment holds a point of it, and so does the ball: the
// spheres' cone test is conservative for it. The radius carries 1e-3 relative
// + 1e-3 (1 + |centre|) of margin over the float64 half diagonal, far above
// the float32 transforms' error; a non-finite box: HUGE_VALF, every direction.
RT_HD float4 box_ball(const rt_object &o, const double R[3][3]) {
    double c[3], h2 = 0.0;
    for (int r = 0; r < 3; ++r) {
        c[r] = 0.5 * (double(o.box_mins[r]) + double(o.box_maxs[r]));
        const double e = 0.5 * (double(o.box_maxs[r]) - double(o.box_mins[r]));
        h2 += e * e;
    }
    double w[3];
    for (int r = 0; r < 3; ++r) w[r] = R[0][r] * c[0] + R[1][r] * c[1] + R[2][r] * c[2] + double(o.position[r]);
    const double wl = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double rad = sqrt(h2) * 1.001 + 1e-3 * (1.0 + wl);
    return make_float4(static_cast<float>(w[0]), static_cast<float>(w[1]), static_cast<float>(w[2]),
                       std::isfinite(rad) ? static_cast<float>(rad * (1.0 + 1e-6)) : HUGE_VALF);
}

// The (box, light) separating plane: the face plane of the box, in the float32
// transform the render kernel uses, with the light farthest beyond it. A
// shadow segment whose start lies beyond that plane too cannot be occluded by
// the box (both of its ends beyond the plane of a face; the exact slab test
// then sees that axis' entry at t > 1 or a miss). (n, w) with the margin m
// folded into w (a start counts as beyond when n . start + w > 0), m = 1e-3 +
// 1e-5 (scene extent + |w|), far above the float32 rounding of n . start and
// of the kernel's transform; kept only if the light lies beyond by more than
// 0.01 (the segment ends at L + 0.01 n, :808-809) + 2 m; else w = -inf (never
// beyond: no_plane, also what a scene with a non-finite object stores). A
// larger extent only lowers w.
RT_HD float4 no_plane() { return make_float4(0.0f, 0.0f, 0.0f, -HUGE_VALF); }
RT_HD float4 box_light_plane(const BoxRec &B, const float light[3], double extent) {
    const double Lp[3] = {light[0], light[1], light[2]};
    double best = -HUGE_VAL, bn[3] = {0, 0, 0}, bw = 0, bm = 0;
    for (int a = 0; a < 3; ++a)
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            const double face = sgn > 0 ? B.maxs[a] : B.mins[a];
            const double r[4] = {B.w2l[4 * a], B.w2l[4 * a + 1], B.w2l[4 * a + 2], B.w2l[4 * a + 3]};
            const double sl = sgn * (r[0] * Lp[0] + r[1] * Lp[1] + r[2] * Lp[2] + r[3] - face);
            if (sl > best) {
                best = sl;
                for (int k = 0; k < 3; ++k) bn[k] = sgn * r[k];
                bw = sgn * (r[3] - face);
                bm = 1e-3 + 1e-5 * (extent + fabs(r[3]) + fabs(face));
            }
        }
    if (std::isfinite(best) && std::isfinite(bw) && best > 0.01 + 2.0 * bm)
        return make_float4(static_cast<float>(bn[0]), static_cast<float>(bn[1]), static_cast<float>(bn[2]),
                           static_cast<float>(bw - bm));
    return no_plane();
}

// A ball (centre c, radius r) seen from a light L, d = |c - L|. A shadow ray
// from shaded point p runs from p + 0.01 n towards L (:808-809): within 0.01
// of the ray from L in the direction of p - L. The ball can block it only if
// that ray passes within rp (r inflated, below) of c: its direction within
// asin(rp / d) of v = (c - L) / d, or any direction when d <= rp (false).
RT_HD bool ball_from_light(const float c[3], float radius, const float light[3], double v[3], double &d, double &rp) {
    for (int k = 0; k < 3; ++k) v[k] = double(c[k]) - double(light[k]);
    d = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    rp = double(radius) + 0.021 + 1e-3 * d;
    return std::isfinite(d) && std::isfinite(rp) && d > rp;
}

// The ShadowCone of a sphere seen from a light (the margins dwarf the float32
// rounding of the stored values).
RT_HD ShadowCone shadow_cone(const SphereRec &s, float abs_radius, const float light[3]) {
    ShadowCone c = {{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float centre[3] = {s.cx, s.cy, s.cz};
    double v[3], d, rp;
    if (!ball_from_light(centre, abs_radius, light, v, d, rp)) {
        c.near = 1.0f;  // always a candidate
        return c;
    }
    for (int r = 0; r < 3; ++r) c.v[r] = static_cast<float>(v[r] / d);
    c.far = static_cast<float>(d - rp);
    const double sp = rp / d;
    c.sph = static_cast<float>(sp);
    c.cph = static_cast<float>(sqrt(fmax(0.0, 1.0 - sp * sp)));
    return c;
}

// The cone of a ball (centre, radius: a sphere, or a box's ball) seen from a
// live light, for the direction masks: axis, cos / sin of the half-angle +
// 1e-3, or every direction; `bit`: the ball's mask bit; *half (optional): the
// half-angle.
struct MaskCone {
    double ax[3], ch, sh;
    int32_t every, bit;
};
static_assert(sizeof(MaskCone) == 48, "MaskCone layout");
RT_HD MaskCone mask_cone(const float ball[4], const float light[3], int bit, double *half = nullptr) {
    MaskCone c = {{0.0, 0.0, 0.0}, 0.0, 0.0, 0, bit};
    double v[3], d, rp, h = 0.0;
    if (!ball_from_light(ball, ball[3], light, v, d, rp)) {
        c.every = 1;
    } else {
        for (int k = 0; k < 3; ++k) c.ax[k] = v[k] / d;
        h = asin(fmin(1.0, rp / d));
        c.ch = cos(h + 1e-3);
        c.sh = sin(h + 1e-3);
    }
    if (half) *half = h;
    return c;
}
// The texel test: w = the texel's centre direction, ca / sa = cos / sin of its
// half-angle alpha (the largest angle to its four corners). angle(w, axis) <=
// alpha + half + 1e-3 on cosines (both angles are below pi; acos is
// decreasing), less 1e-12 for rounding (far below the 1e-3 rad margin).
RT_HD bool texel_hit(const double w[3], double ca, double sa, const MaskCone &c) {
    const double lim = ca * c.ch - sa * c.sh - 1e-12;
    const double dot = w[0] * c.ax[0] + w[1] * c.ax[1] + w[2] * c.ax[2];
    return c.every != 0 || dot >= lim;
}

// A sphere's box in float64 with the BVH margin; r: the radius to cover;
// extent: a bound on |coordinate| of every finite object of the scene (the
// origins of the secondary rays that walk the BVH lie on their surfaces; a
// larger value only widens the box). The render kernel's node test (node_hit)
// has no slack of its own: its error, ~2^-22 (|x| + |o|) / |d|, stays far
// below this margin for every box coordinate x and ray origin o of the scene.
struct SphereBox {
    double lo[3], hi[3];
};
RT_HD SphereBox sphere_box(const SphereRec &s, double r, double extent) {
    const double c[3] = {s.cx, s.cy, s.cz};
    double mag = 0.0;
    for (int a = 0; a < 3; ++a) mag = fmax(mag, fabs(c[a]) + r);
    const double margin = 1e-3 + 1e-4 * fmax(mag, extent);
    SphereBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = c[a] - r - margin;
        b.hi[a] = c[a] + r + margin;
    }
    return b;
}

#undef RT_HD

}  // namespace rtamd
