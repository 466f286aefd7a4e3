// rt_glmath.h — the reference GL's float32 arithmetic (run-time sin / cos and
// the matrix chain with the compiler's constant bookkeeping), as one text the
// host (rt_camera.cpp) and the device (rt_anim.hip, the animate kernel) both
// compile: a box's transforms derived on the GPU equal the host's bit for bit.
// Every translation unit is built with -ffp-contract=off; fused multiply-adds
// appear only where they are written (fmaf), divisions are IEEE, float32
// denormals are kept.
//
// The bookkeeping reproduces three things measured on llvmpipe (probe shaders
// built from the reference's own functions, tests/golden/make_camera_golden.py):
//  * run-time sin / cos are gallivm's polynomials (Cephes range reduction by
//    4/pi, three-part pi/4 subtraction, the two minimax polynomials, every
//    multiply-add fused) — gallivm_sincos below;
//  * everything that depends only on constants is folded at compile time in
//    float;
//  * the compiler's inexact-float rewrites: products and sums with a
//    constant 0 or 1 vanish, a product by a constant times another constant
//    becomes one product by the folded constant; no multiply-add is fused.
// Gf carries that: a value, whether it is a compile-time constant, and
// whether it is a run-time value times a constant.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtamd {
namespace glf {

// (forced inlining and unrolling: every flag below is then known at compile
// time and the chain compiles to its straight-line float operations)
#define RT_HD __host__ __device__ __forceinline__

constexpr float kPi = 3.14159265358f;       // raytrace_compute.glsl:13
constexpr float kDegToRad = kPi / 180.0f;    // :17, folded in float

RT_HD float bits_to_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
RT_HD uint32_t float_to_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}

// gallivm's lp_build_sin / lp_build_cos (Mesa llvmpipe, the GL the
// reference's golden renders come from), in float32 with fused multiply-adds.
// The truncation to int limits the argument: |a| * 4/pi < 2^31 (beyond it the
// host's and the device's conversions differ).
RT_HD float gallivm_sincos(float a, bool want_cos) {
    const float x_abs = fabsf(a);
    const float scale_y = x_abs * 1.27323954473516f;  // 4 / pi
    const int emm2_i = static_cast<int>(scale_y);     // truncation
    const int emm2_add = emm2_i + 1;
    const int emm2_and = emm2_add & ~1;  // j = (j + 1) & ~1
    const float y_2 = static_cast<float>(emm2_and);
    uint32_t sign_bit;
    bool poly_mask;
    if (want_cos) {
        const int emm2_2 = emm2_and - 2;
        sign_bit = static_cast<uint32_t>((~emm2_2) & 4) << 29;
        poly_mask = (emm2_2 & 2) == 0;
    } else {
        sign_bit = (static_cast<uint32_t>(emm2_add & 4) << 29) ^ (float_to_bits(a) & 0x80000000u);
        poly_mask = (emm2_and & 2) == 0;
    }
    // extended-precision modular arithmetic: x - j * pi/4 in three parts
    float x = fmaf(y_2, -0.78515625f, x_abs);
    x = fmaf(y_2, -2.4187564849853515625e-4f, x);
    x = fmaf(y_2, -3.77489497744594108e-8f, x);
    const float z = x * x;
    // cosine polynomial
    float yc = fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
    yc = fmaf(yc, z, 4.166664568298827e-2f);
    yc = yc * z;
    yc = yc * z;
    yc = fmaf(z, -0.5f, yc);
    yc = yc + 1.0f;
    // sine polynomial
    float ys = fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
    ys = fmaf(ys, z, -1.6666654611e-1f);
    ys = ys * z;
    ys = fmaf(ys, x, x);
    const float r = poly_mask ? ys : yc;
    return bits_to_float(float_to_bits(r) ^ sign_bit);
}

// A float32 value of the chain with the compiler's constant bookkeeping (see
// the file comment): `konst` — known at compile time; `scaled` — a run-time
// value `base` times the constant `k` (v = base * k).
struct Gf {
    float v;
    bool konst = false;
    bool scaled = false;
    float base = 0.0f, k = 0.0f;
};
RT_HD Gf cst(float v) {
    Gf r;
    r.v = v;
    r.konst = true;
    return r;
}
RT_HD Gf run(float v) {
    Gf r;
    r.v = v;
    return r;
}
RT_HD Gf neg(const Gf &a) {
    Gf r = a;
    r.v = -a.v;
    r.k = -a.k;  // -(b k) == b (-k) exactly
    return r;
}
RT_HD Gf mul(const Gf &a, const Gf &b) {
    if (a.konst && b.konst) return cst(a.v * b.v);
    if (!a.konst && !b.konst) return run(a.v * b.v);
    // (copies, not pointers: the flags stay visible to the optimiser)
    const Gf c = a.konst ? a : b;  // the constant factor
    const Gf x = a.konst ? b : a;
    if (c.v == 0.0f) return cst(0.0f);    // x * 0 -> 0
    if (c.v == 1.0f) return x;            // x * 1 -> x
    if (c.v == -1.0f) return neg(x);      // x * -1 -> -x
    Gf r;
    r.scaled = true;
    if (x.scaled) {  // (base * k) * c -> base * (k c)
        r.base = x.base;
        r.k = x.k * c.v;
    } else {
        r.base = x.v;
        r.k = c.v;
    }
    r.v = r.base * r.k;
    return r;
}
RT_HD Gf add(const Gf &a, const Gf &b) {
    if (a.konst && b.konst) return cst(a.v + b.v);
    if (a.konst && a.v == 0.0f) return b;  // 0 + x -> x
    if (b.konst && b.v == 0.0f) return a;
    return run(a.v + b.v);
}
RT_HD Gf sub(const Gf &a, const Gf &b) { return add(a, neg(b)); }
RT_HD Gf div(const Gf &a, const Gf &b) {
    if (a.konst && b.konst) return cst(a.v / b.v);
    if (a.konst && a.v == 0.0f) return cst(0.0f);
    return run(a.v / b.v);
}

struct Gm {
    Gf m[4][4];  // column-major, m[col][row]
};
RT_HD Gm ident() {
    Gm r;
    #pragma unroll
    for (int c = 0; c < 4; ++c)
        #pragma unroll
        for (int w = 0; w < 4; ++w) r.m[c][w] = cst(c == w ? 1.0f : 0.0f);
    return r;
}
// mat4 * mat4 as GLSL lowers it: column c = A[0] b.x + A[1] b.y + A[2] b.z + A[3] b.w
RT_HD Gm mul(const Gm &a, const Gm &b) {
    Gm r;
    #pragma unroll
    for (int c = 0; c < 4; ++c)
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            Gf acc = mul(a.m[0][w], b.m[c][0]);
            #pragma unroll
            for (int k = 1; k < 4; ++k) acc = add(acc, mul(a.m[k][w], b.m[c][k]));
            r.m[c][w] = acc;
        }
    return r;
}
// rotation_matrix_{x,y,z} (:444-486) from their cosine and sine
RT_HD Gm rot(int axis, const Gf &c, const Gf &s) {
    Gm r = ident();
    if (axis == 0) { r.m[1][1] = c; r.m[1][2] = s; r.m[2][1] = neg(s); r.m[2][2] = c; }
    if (axis == 1) { r.m[0][0] = c; r.m[0][2] = neg(s); r.m[2][0] = s; r.m[2][2] = c; }
    if (axis == 2) { r.m[0][0] = c; r.m[0][1] = s; r.m[1][0] = neg(s); r.m[1][1] = c; }
    return r;
}
RT_HD Gf det2(const Gf &a, const Gf &b, const Gf &c, const Gf &e) { return sub(mul(a, b), mul(c, e)); }
RT_HD Gf term3(const Gf &a, const Gf &x, const Gf &b, const Gf &y, const Gf &c, const Gf &z) {
    return add(sub(mul(a, x), mul(b, y)), mul(c, z));
}
// GLSL inverse(mat4) as Mesa's builtin lowers it: 2x2 sub-factors, the
// adjugate, det = m0.x a0 + (m0.y a1 + (m0.z a2 + m0.w a3)), adj / det.
RT_HD Gm inverse(const Gm &M) {
    const Gf(*m)[4] = M.m;
    const Gf S00 = det2(m[2][2], m[3][3], m[3][2], m[2][3]), S01 = det2(m[2][1], m[3][3], m[3][1], m[2][3]);
    const Gf S02 = det2(m[2][1], m[3][2], m[3][1], m[2][2]), S03 = det2(m[2][0], m[3][3], m[3][0], m[2][3]);
    const Gf S04 = det2(m[2][0], m[3][2], m[3][0], m[2][2]), S05 = det2(m[2][0], m[3][1], m[3][0], m[2][1]);
    const Gf S06 = det2(m[1][2], m[3][3], m[3][2], m[1][3]), S07 = det2(m[1][1], m[3][3], m[3][1], m[1][3]);
    const Gf S08 = det2(m[1][1], m[3][2], m[3][1], m[1][2]), S09 = det2(m[1][0], m[3][3], m[3][0], m[1][3]);
    const Gf S10 = det2(m[1][0], m[3][2], m[3][0], m[1][2]), S11 = det2(m[1][1], m[3][3], m[3][1], m[1][3]);
    const Gf S12 = det2(m[1][0], m[3][1], m[3][0], m[1][1]), S13 = det2(m[1][2], m[2][3], m[2][2], m[1][3]);
    const Gf S14 = det2(m[1][1], m[2][3], m[2][1], m[1][3]), S15 = det2(m[1][1], m[2][2], m[2][1], m[1][2]);
    const Gf S16 = det2(m[1][0], m[2][3], m[2][0], m[1][3]), S17 = det2(m[1][0], m[2][2], m[2][0], m[1][2]);
    const Gf S18 = det2(m[1][0], m[2][1], m[2][0], m[1][1]);
    Gm adj;
    adj.m[0][0] = term3(m[1][1], S00, m[1][2], S01, m[1][3], S02);
    adj.m[1][0] = neg(term3(m[1][0], S00, m[1][2], S03, m[1][3], S04));
    adj.m[2][0] = term3(m[1][0], S01, m[1][1], S03, m[1][3], S05);
    adj.m[3][0] = neg(term3(m[1][0], S02, m[1][1], S04, m[1][2], S05));
    adj.m[0][1] = neg(term3(m[0][1], S00, m[0][2], S01, m[0][3], S02));
    adj.m[1][1] = term3(m[0][0], S00, m[0][2], S03, m[0][3], S04);
    adj.m[2][1] = neg(term3(m[0][0], S01, m[0][1], S03, m[0][3], S05));
    adj.m[3][1] = term3(m[0][0], S02, m[0][1], S04, m[0][2], S05);
    adj.m[0][2] = term3(m[0][1], S06, m[0][2], S07, m[0][3], S08);
    adj.m[1][2] = neg(term3(m[0][0], S06, m[0][2], S09, m[0][3], S10));
    adj.m[2][2] = term3(m[0][0], S11, m[0][1], S09, m[0][3], S12);
    adj.m[3][2] = neg(term3(m[0][0], S08, m[0][1], S10, m[0][2], S12));
    adj.m[0][3] = neg(term3(m[0][1], S13, m[0][2], S14, m[0][3], S15));
    adj.m[1][3] = term3(m[0][0], S13, m[0][2], S16, m[0][3], S17);
    adj.m[2][3] = neg(term3(m[0][0], S14, m[0][1], S16, m[0][3], S18));
    adj.m[3][3] = term3(m[0][0], S15, m[0][1], S17, m[0][2], S18);
    const Gf det = add(mul(m[0][0], adj.m[0][0]),
                       add(mul(m[0][1], adj.m[1][0]), add(mul(m[0][2], adj.m[2][0]), mul(m[0][3], adj.m[3][0]))));
    Gm r;
    #pragma unroll
    for (int c = 0; c < 4; ++c)
        #pragma unroll
        for (int w = 0; w < 4; ++w) r.m[c][w] = div(adj.m[c][w], det);
    return r;
}

// transpose(inverse(mat3(m))) as Mesa's builtin lowers inverse(mat3): the
// three cofactors of the first column, det = (m00 c0 - m01 c1) + m02 c2, the
// adjugate over det; returned column-major (r[col][row]).
RT_HD void normal_matrix(const Gm &M, Gf r[3][3]) {
    const Gf(*m)[4] = M.m;
    const Gf f0 = det2(m[1][1], m[2][2], m[2][1], m[1][2]);
    const Gf f1 = det2(m[1][0], m[2][2], m[2][0], m[1][2]);
    const Gf f2 = det2(m[1][0], m[2][1], m[2][0], m[1][1]);
    const Gf det = add(sub(mul(m[0][0], f0), mul(m[0][1], f1)), mul(m[0][2], f2));
    Gf inv[3][3];  // inv[col][row]
    inv[0][0] = div(f0, det);
    inv[1][0] = div(neg(f1), det);
    inv[2][0] = div(f2, det);
    inv[0][1] = div(neg(det2(m[0][1], m[2][2], m[2][1], m[0][2])), det);
    inv[1][1] = div(det2(m[0][0], m[2][2], m[2][0], m[0][2]), det);
    inv[2][1] = div(neg(det2(m[0][0], m[2][1], m[2][0], m[0][1])), det);
    inv[0][2] = div(det2(m[0][1], m[1][2], m[1][1], m[0][2]), det);
    inv[1][2] = div(neg(det2(m[0][0], m[1][2], m[1][0], m[0][2])), det);
    inv[2][2] = div(det2(m[0][0], m[1][1], m[1][0], m[0][1]), det);
    #pragma unroll
    for (int c = 0; c < 3; ++c)
        #pragma unroll
        for (int w = 0; w < 3; ++w) r[c][w] = inv[w][c];  // transpose
}

// rotation_matrix_{x,y,z} (:444-486) of a run-time angle in degrees
RT_HD Gm rot_deg(int axis, float deg) {
    const float a = mul(cst(kDegToRad), run(deg)).v;
    return rot(axis, run(gallivm_sincos(a, true)), run(gallivm_sincos(a, false)));
}

// intersect_box_object's transforms (:650-652, :718) as llvmpipe evaluates
// them: local_to_world = calc_transform_matrix(position, angles) (:529-532:
// translation_matrix * (mat4(1) * Rz(yaw) * Rx(pitch) * Ry(roll))), its
// Mesa inverse, and transpose(inverse(mat3(local_to_world))). The object's
// fields are run-time values (objects[] is indexed by the loop counter), so
// only the functions' own constants fold. Column-major outputs (m[col][row]
// at col * 4 + row; the normal matrix at col * 3 + row). Probed bit-exact
// against llvmpipe on the shipped scene (tests/golden/make_box_golden.py).
RT_HD void box_transforms(const float pos[3], const float ang[3], float l2w[16], float w2l[16], float nrm[9]) {
    Gm T = ident();
    #pragma unroll
    for (int k = 0; k < 3; ++k) T.m[3][k] = run(pos[k]);
    const Gm R = mul(mul(mul(ident(), rot_deg(2, ang[1])), rot_deg(0, ang[0])), rot_deg(1, ang[2]));
    const Gm L = mul(T, R);
    const Gm W = inverse(L);
    Gf N[3][3];
    normal_matrix(L, N);
    #pragma unroll
    for (int c = 0; c < 4; ++c)
        #pragma unroll
        for (int w = 0; w < 4; ++w) {
            l2w[c * 4 + w] = L.m[c][w].v;
            w2l[c * 4 + w] = W.m[c][w].v;
        }
    #pragma unroll
    for (int c = 0; c < 3; ++c)
        #pragma unroll
        for (int w = 0; w < 3; ++w) nrm[c * 3 + w] = N[c][w].v;
}

#undef RT_HD

}  // namespace glf
}  // namespace rtamd
