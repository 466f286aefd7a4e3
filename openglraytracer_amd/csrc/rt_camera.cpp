// rt_camera.cpp — the reference's orbiting camera (raytrace_compute.glsl:
// 334-392, :411-545) evaluated the way the reference's own GL evaluates it.
//
// The reference computes its camera in float32 per invocation; its golden
// renders (tests/golden) come from Mesa llvmpipe. Reproducing that frame
// constant bit for bit needs three things measured on llvmpipe (probe
// shaders built from the reference's own camera functions,
// tests/golden/make_camera_golden.py):
//  * run-time sin / cos are gallivm's polynomials (Cephes range reduction by
//    4/pi, three-part pi/4 subtraction, the two minimax polynomials, every
//    multiply-add fused) — gl_sin / gl_cos (rt_glmath.h);
//  * everything that depends only on constants is folded at compile time in
//    float (tan(45 deg) -> 1, cos(DEG_TO_RAD * 90), the projection terms, the
//    identity pitch / roll rotations);
//  * the compiler's inexact-float rewrites: products and sums with a
//    constant 0 or 1 vanish, a product by a constant times another constant
//    becomes one product by the folded constant ((10 cos s) * c -> cos s *
//    (10 c)), and mod()'s `(x - 360 floor(x/360)) + 90` becomes
//    `(x + 90) - 360 floor(x/360)`; no multiply-add is fused.
// Gf (rt_glmath.h) carries that bookkeeping: a value, whether it is a compile-time
// constant, and whether it is a run-time value times a constant. With it the
// float32 chain — GLSL matrix products (column sums left to right), Mesa's
// inverse(mat4) (2x2 sub-factors, adjugate, determinant, true division) —
// matches llvmpipe's inverse(proj * view) and view matrix exactly
// (tests/test_host.py: 1200 probed times and every golden fixture).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "rt_glmath.h"
#include "rt_internal.h"

namespace rtamd {

// (the float32 chain itself — gallivm_sincos, Gf / Gm, inverse, normal_matrix,
// box_transforms — lives in rt_glmath.h, shared with the animate kernel)
using namespace glf;

float gl_sin(float a) { return gallivm_sincos(a, false); }
float gl_cos(float a) { return gallivm_sincos(a, true); }

// main() :334-364: speed, the orbit position and the yaw angle.
void reference_orbit(float time, float *speed_out, float pos[3], float *yaw_out) {
    const float speed = time * 0.4f + 0.5f;  // :343 (time_scale 0.4, :236)
    pos[0] = 10.0f * gl_cos(speed);
    pos[1] = 10.0f * gl_sin(speed);
    pos[2] = 0.0f;
    // :353 yaw = mod(speed * (180 / 3.1416), 360) + 90, as compiled:
    // (x + 90) - 360 floor(x / 360)
    const float x = speed * (180.0f / 3.1416f);
    const float yaw = (x + 90.0f) - 360.0f * std::floor(x / 360.0f);
    if (speed_out) *speed_out = speed;
    if (yaw_out) *yaw_out = yaw;
}

// inverse(proj_mat * view_mat) (:383) and view_mat (:368) of the reference
// orbit camera at `time`, column-major, as llvmpipe computes them.
void reference_view_gl(float time, float unproj[16], float view[16]) {
    float speed, pos[3], yaw;
    reference_orbit(time, &speed, pos, &yaw);
    const float a = kDegToRad * yaw;
    const Gm Rz = rot(2, run(gl_cos(a)), run(gl_sin(a)));
    // pitch = roll = 0 are constants: cos 0 = 1, sin 0 = 0 folded
    const Gm R = mul(mul(mul(ident(), Rz), rot(0, cst(1.0f), cst(0.0f))), rot(1, cst(1.0f), cst(0.0f)));
    Gm T = ident();
    T.m[3][0] = mul(cst(10.0f), run(gl_cos(speed)));
    T.m[3][1] = mul(cst(10.0f), run(gl_sin(speed)));
    T.m[3][2] = cst(0.0f);
    // flip_y_and_z = rotation_matrix_x(90) (:542), folded at compile time:
    // cos(DEG_TO_RAD * 90) = -4.371139e-8 (0xb33bbd2e), sin = 1
    const Gm flip = rot(0, cst(bits_to_float(0xb33bbd2eu)), cst(1.0f));
    const Gm V = inverse(mul(mul(T, R), flip));
    // calc_projection_matrix (:411-426) folded: q = 1 / tan(45 deg) = 1
    Gm P;
    for (int c = 0; c < 4; ++c)
        for (int w = 0; w < 4; ++w) P.m[c][w] = cst(0.0f);
    P.m[0][0] = cst(1.0f / (16.0f / 9.0f));
    P.m[1][1] = cst(1.0f);
    P.m[2][2] = cst((0.1f + 1000.0f) / (0.1f - 1000.0f));
    P.m[2][3] = cst(-1.0f);
    P.m[3][2] = cst((2.0f * 0.1f * 1000.0f) / (0.1f - 1000.0f));
    const Gm U = inverse(mul(P, V));
    for (int c = 0; c < 4; ++c)
        for (int w = 0; w < 4; ++w) {
            if (unproj) unproj[c * 4 + w] = U.m[c][w].v;
            if (view) view[c * 4 + w] = V.m[c][w].v;
        }
}

// intersect_box_object's transforms (:650-652, :718) as llvmpipe evaluates
// them (rt_glmath.h box_transforms: the text the animate kernel runs too).
void reference_box_transforms(const float pos[3], const float ang[3], float l2w[16], float w2l[16],
                              float nrm[9]) {
    box_transforms(pos, ang, l2w, w2l, nrm);
}

}  // namespace rtamd
