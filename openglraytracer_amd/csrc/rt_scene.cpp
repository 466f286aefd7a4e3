// rt_scene.cpp — host side of the hot path: the reference scene / camera
// restated as C++ data, the frame constants (camera unprojection, per-object
// transforms) and the device-resident scene blob.
//
// The reference orbit camera's unprojection is evaluated as the reference's
// GL evaluates it (rt_camera.cpp, bit-identical to llvmpipe). The per-object
// transforms (:650-652, :718) and explicit cameras are evaluated in float64
// and rounded once to float32 ("Parity").
// Everything the kernel evaluates per pixel stays float32 in GLSL order.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "rt_anim.h"
#include "rt_internal.h"

using namespace rtamd;

namespace {

constexpr float kPi = 3.14159265358f;            // raytrace_compute.glsl:13
constexpr float kDegToRad = kPi / 180.0f;         // :17 (folded in float)

struct M4 {
    double m[4][4];  // column-major, m[col][row] as GLSL
};

M4 ident() {
    M4 r{};
    for (int i = 0; i < 4; ++i) r.m[i][i] = 1.0;
    return r;
}

M4 mul(const M4 &a, const M4 &b) {
    M4 r{};
    for (int c = 0; c < 4; ++c)
        for (int row = 0; row < 4; ++row) {
            double acc = 0.0;
            for (int k = 0; k < 4; ++k) acc += a.m[k][row] * b.m[c][k];
            r.m[c][row] = acc;
        }
    return r;
}

// Inverse via the 4x4 adjugate (float64).
M4 inverse(const M4 &a) {
    const double *s = &a.m[0][0];  // column-major linear
    double inv[16];
    inv[0] = s[5] * s[10] * s[15] - s[5] * s[11] * s[14] - s[9] * s[6] * s[15] + s[9] * s[7] * s[14] +
             s[13] * s[6] * s[11] - s[13] * s[7] * s[10];
    inv[4] = -s[4] * s[10] * s[15] + s[4] * s[11] * s[14] + s[8] * s[6] * s[15] - s[8] * s[7] * s[14] -
             s[12] * s[6] * s[11] + s[12] * s[7] * s[10];
    inv[8] = s[4] * s[9] * s[15] - s[4] * s[11] * s[13] - s[8] * s[5] * s[15] + s[8] * s[7] * s[13] +
             s[12] * s[5] * s[11] - s[12] * s[7] * s[9];
    inv[12] = -s[4] * s[9] * s[14] + s[4] * s[10] * s[13] + s[8] * s[5] * s[14] - s[8] * s[6] * s[13] -
              s[12] * s[5] * s[10] + s[12] * s[6] * s[9];
    inv[1] = -s[1] * s[10] * s[15] + s[1] * s[11] * s[14] + s[9] * s[2] * s[15] - s[9] * s[3] * s[14] -
             s[13] * s[2] * s[11] + s[13] * s[3] * s[10];
    inv[5] = s[0] * s[10] * s[15] - s[0] * s[11] * s[14] - s[8] * s[2] * s[15] + s[8] * s[3] * s[14] +
             s[12] * s[2] * s[11] - s[12] * s[3] * s[10];
    inv[9] = -s[0] * s[9] * s[15] + s[0] * s[11] * s[13] + s[8] * s[1] * s[15] - s[8] * s[3] * s[13] -
             s[12] * s[1] * s[11] + s[12] * s[3] * s[9];
    inv[13] = s[0] * s[9] * s[14] - s[0] * s[10] * s[13] - s[8] * s[1] * s[14] + s[8] * s[2] * s[13] +
              s[12] * s[1] * s[10] - s[12] * s[2] * s[9];
    inv[2] = s[1] * s[6] * s[15] - s[1] * s[7] * s[14] - s[5] * s[2] * s[15] + s[5] * s[3] * s[14] +
             s[13] * s[2] * s[7] - s[13] * s[3] * s[6];
    inv[6] = -s[0] * s[6] * s[15] + s[0] * s[7] * s[14] + s[4] * s[2] * s[15] - s[4] * s[3] * s[14] -
             s[12] * s[2] * s[7] + s[12] * s[3] * s[6];
    inv[10] = s[0] * s[5] * s[15] - s[0] * s[7] * s[13] - s[4] * s[1] * s[15] + s[4] * s[3] * s[13] +
              s[12] * s[1] * s[7] - s[12] * s[3] * s[5];
    inv[14] = -s[0] * s[5] * s[14] + s[0] * s[6] * s[13] + s[4] * s[1] * s[14] - s[4] * s[2] * s[13] -
              s[12] * s[1] * s[6] + s[12] * s[2] * s[5];
    inv[3] = -s[1] * s[6] * s[11] + s[1] * s[7] * s[10] + s[5] * s[2] * s[11] - s[5] * s[3] * s[10] -
             s[9] * s[2] * s[7] + s[9] * s[3] * s[6];
    inv[7] = s[0] * s[6] * s[11] - s[0] * s[7] * s[10] - s[4] * s[2] * s[11] + s[4] * s[3] * s[10] +
             s[8] * s[2] * s[7] - s[8] * s[3] * s[6];
    inv[11] = -s[0] * s[5] * s[11] + s[0] * s[7] * s[9] + s[4] * s[1] * s[11] - s[4] * s[3] * s[9] -
              s[8] * s[1] * s[7] + s[8] * s[3] * s[5];
    inv[15] = s[0] * s[5] * s[10] - s[0] * s[6] * s[9] - s[4] * s[1] * s[10] + s[4] * s[2] * s[9] +
              s[8] * s[1] * s[6] - s[8] * s[2] * s[5];
    double det = s[0] * inv[0] + s[1] * inv[4] + s[2] * inv[8] + s[3] * inv[12];
    M4 r;
    double *o = &r.m[0][0];
    for (int i = 0; i < 16; ++i) o[i] = inv[i] / det;
    return r;
}

// rotation_matrix_{x,y,z} (:444-486): the angle enters as the float
// DEG_TO_RAD * deg the shader forms, then cos/sin in float64.
M4 rot(int axis, float deg) {
    const double a = static_cast<double>(kDegToRad * deg);
    const double c = std::cos(a), s = std::sin(a);
    M4 r = ident();
    if (axis == 0) { r.m[1][1] = c; r.m[1][2] = s; r.m[2][1] = -s; r.m[2][2] = c; }
    if (axis == 1) { r.m[0][0] = c; r.m[0][2] = -s; r.m[2][0] = s; r.m[2][2] = c; }
    if (axis == 2) { r.m[0][0] = c; r.m[0][1] = s; r.m[1][0] = -s; r.m[1][1] = c; }
    return r;
}

// calc_transform_matrix (:529-532) = translation (:432) * rotation (:492-503:
// yaw about z, then pitch about x, then roll about y).
M4 transform(const float pos[3], const float ang[3]) {
    M4 t = ident();
    t.m[3][0] = pos[0];
    t.m[3][1] = pos[1];
    t.m[3][2] = pos[2];
    return mul(t, mul(mul(rot(2, ang[1]), rot(0, ang[0])), rot(1, ang[2])));
}

void set4(float *d, float a, float b, float c, float e) {
    d[0] = a; d[1] = b; d[2] = c; d[3] = e;
}
void set4s(float *d, float s) { set4(d, s, s, s, s); }

void set_material(rt_material &m, float amb, const float dif[4], float spe, float shin, float refl, float transp,
                  float ior) {
    set4s(m.ambient, amb);
    std::memcpy(m.diffuse, dif, 16);
    set4s(m.specular, spe);
    m.shininess = shin;
    set4s(m.emissive, 0.0f);
    m.reflectivity = refl;
    m.transparency = transp;
    m.refraction_index = ior;
}

void make_object(rt_object &o, float mn[3], float mx[3], float radius, float p0, float p1, float p2, float a0, float a1,
                 float a2, int mat) {
    std::memcpy(o.box_mins, mn, 12);
    std::memcpy(o.box_maxs, mx, 12);
    o.radius = radius;
    o.position[0] = p0; o.position[1] = p1; o.position[2] = p2;
    o.angles[0] = a0; o.angles[1] = a1; o.angles[2] = a2;
    o.material = mat;
}

// get_closest_collision's type test (:749-771).
int object_kind(const rt_object &o) {
    const bool box = !(o.box_mins[0] == 0.0f && o.box_mins[1] == 0.0f && o.box_mins[2] == 0.0f &&
                       o.box_maxs[0] == 0.0f && o.box_maxs[1] == 0.0f && o.box_maxs[2] == 0.0f);
    if (box) return 1;
    if (o.radius != -1.0f) return 2;
    return 0;
}

uint64_t splitmix64(uint64_t &state) {
    state += 0x9E3779B97F4A7C15ULL;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

float uniform(uint64_t &state, double lo, double hi) {
    const double u = static_cast<double>(splitmix64(state) >> 11) * (1.0 / 9007199254740992.0);
    return static_cast<float>(lo + (hi - lo) * u);
}

}  // namespace

extern "C" {

// raytrace_compute.glsl:74-157
int rt_reference_materials(rt_material out[RT_REFERENCE_MATERIALS]) {
    if (!out) { set_error("rt_reference_materials: null out"); return RT_ERR_INVALID; }
    const float d1[4] = {0.5f, 0.0f, 0.0f, 1.0f}, d2[4] = {0.3f, 0.6f, 0.3f, 1.0f};
    const float dr[4] = {1, 0, 0, 1}, dg[4] = {0, 1, 0, 1}, db[4] = {0, 0, 1, 1};
    const float dm[4] = {0.6f, 0.6f, 0.6f, 1.0f}, dw[4] = {0.4f, 0.4f, 0.4f, 0.4f};
    set_material(out[RT_MAT_MATERIAL1], 1.0f, d1, 1.0f, 4.0f, 1.0f, 0.0f, 1.5f);
    set_material(out[RT_MAT_MATERIAL2], 1.0f, d2, 1.0f, 4.0f, 1.0f, 0.0f, 1.5f);
    set_material(out[RT_MAT_RED_GLASS], 1.0f, dr, 1.0f, 10.0f, 0.8f, 0.4f, 1.5f);
    set_material(out[RT_MAT_GREEN_GLASS], 1.0f, dg, 1.0f, 10.0f, 0.4f, 0.6f, 1.5f);
    set_material(out[RT_MAT_BLUE_GLASS], 1.0f, db, 1.0f, 10.0f, 0.4f, 0.6f, 1.5f);
    set_material(out[RT_MAT_MIRROR], 1.0f, dm, 1.0f, 4.0f, 1.0f, 0.0f, 1.0f);
    set_material(out[RT_MAT_WALL], 0.5f, dw, 0.3f, 3.0f, 0.3f, 0.0f, 1.0f);
    return RT_OK;
}

// raytrace_compute.glsl:199-224
int rt_reference_lights(rt_light out[RT_REFERENCE_LIGHTS]) {
    if (!out) { set_error("rt_reference_lights: null out"); return RT_ERR_INVALID; }
    const float pos[3][3] = {{0.1f, 0.1f, 0.1f}, {7.0f, 7.0f, 2.0f}, {3.0f, -3.0f, 4.0f}};
    for (int i = 0; i < 3; ++i) std::memcpy(out[i].position, pos[i], 12);
    set4s(out[0].ambient, 0.3f); set4s(out[0].diffuse, 0.0f); set4s(out[0].specular, 0.0f);
    set4s(out[1].ambient, 0.05f); set4s(out[1].diffuse, 1.0f); set4s(out[1].specular, 1.0f);
    set4s(out[2].ambient, 0.05f);
    set4(out[2].diffuse, 1.0f, 0.0f, 0.0f, 1.0f);
    set4(out[2].specular, 1.0f, 0.0f, 0.0f, 1.0f);
    return RT_OK;
}

int rt_object_transforms(const rt_object *obj, float l2w[16], float w2l[16], float nrm[9]) {
    if (!obj || !l2w || !w2l || !nrm) {
        set_error("rt_object_transforms: null argument");
        return RT_ERR_INVALID;
    }
    reference_box_transforms(obj->position, obj->angles, l2w, w2l, nrm);
    return RT_OK;
}

// raytrace_compute.glsl:236-237 (scaled_time), :261-321 (objects)
int rt_reference_objects(float time, rt_object out[RT_REFERENCE_OBJECTS]) {
    if (!out) { set_error("rt_reference_objects: null out"); return RT_ERR_INVALID; }
    // scaled_time * k = (time * time_scale) * k, which the reference's GL
    // compiles as time * (time_scale * k) (a product by a constant times
    // another constant folds; probed on llvmpipe)
    auto st = [time](float k) { return time * (0.4f * k); };
    float zero[3] = {0, 0, 0};
    float mn0[3] = {-11, -11, -11}, mx0[3] = {11, 11, 11};
    make_object(out[0], mn0, mx0, -1.0f, 0, 0, 0, 0, 0, 0, RT_MAT_WALL);
    // run-time sin as the reference's GL evaluates it (rt_camera.cpp)
    const float s = 0.5f * gl_sin(st(0.5f)) + 1.5f;
    float mn1[3] = {-1.0f * s, -1.0f * s, -1.0f * s}, mx1[3] = {1.0f * s, 1.0f * s, 1.0f * s};
    make_object(out[1], mn1, mx1, -1.0f, 0, 0, gl_sin(st(3.0f)), 0, st(90.0f), 0, RT_MAT_MIRROR);
    float mn2[3] = {-10, -10, -1}, mx2[3] = {10, 10, 1};
    make_object(out[2], mn2, mx2, -1.0f, 0, 0, -3, gl_sin(st(5.0f)) * 10.0f, 45.0f, 0, RT_MAT_GREEN_GLASS);
    float mn3[3] = {-1, -1, -2}, mx3[3] = {1, 1, 2};
    make_object(out[3], mn3, mx3, -1.0f, 3, 4, 1, 45.0f + st(45.0f), 0, 45.0f + st(180.0f), RT_MAT_BLUE_GLASS);
    make_object(out[4], zero, zero, 2.0f, -3, 4, 1, 0, 0, 0, RT_MAT_RED_GLASS);
    return RT_OK;
}

// rt_reference_objects' rules as channels (include/rt.h): base = the objects
// with the animated fields at their time-0 values.
int rt_reference_animation(rt_object base[RT_REFERENCE_OBJECTS], rt_object_anim anim[RT_REFERENCE_OBJECTS]) {
    if (!base || !anim) { set_error("rt_reference_animation: null argument"); return RT_ERR_INVALID; }
    const int rc = rt_reference_objects(0.0f, base);
    if (rc != RT_OK) return rc;
    std::memset(anim, 0, sizeof(rt_object_anim) * RT_REFERENCE_OBJECTS);
    auto ch = [](int kind, float a, float k, float c) { return rt_anim_channel{kind, a, 0.4f * k, c}; };
    // object 1 (:277-287): the mirror cube, +-1 scaled by 0.5 sin(0.5 st) + 1.5
    for (int i = 0; i < 3; ++i) {
        base[1].box_mins[i] = -1.0f;
        base[1].box_maxs[i] = 1.0f;
    }
    anim[1].scale = ch(RT_ANIM_SIN_OFFSET, 0.5f, 0.5f, 1.5f);
    anim[1].position[2] = ch(RT_ANIM_SIN, 1.0f, 3.0f, 0.0f);
    anim[1].angles[1] = ch(RT_ANIM_RATE, 0.0f, 90.0f, 0.0f);
    // object 2 (:289-297): the glass slab pitching by 10 sin(5 st)
    anim[2].angles[0] = ch(RT_ANIM_SIN, 10.0f, 5.0f, 0.0f);
    // object 3 (:299-307): the blue box turning about two axes
    anim[3].angles[0] = ch(RT_ANIM_RATE_OFFSET, 0.0f, 45.0f, 45.0f);
    anim[3].angles[2] = ch(RT_ANIM_RATE_OFFSET, 0.0f, 180.0f, 45.0f);
    return RT_OK;
}

// rt_animate_objects (radius NULL) and rt_animate_objects2
static int animate_objects(const char *who, const rt_object *base, const rt_object_anim *anim,
                           const rt_anim_channel *radius, int n_objs, float time, rt_object *out) {
    if (n_objs < 0 || (n_objs > 0 && (!base || !anim || !out))) {
        set_error(std::string(who) + ": null argument or negative count");
        return RT_ERR_INVALID;
    }
    for (int i = 0; i < n_objs; ++i) {
        const rt_anim_channel *c = &anim[i].scale;  // 7 channels, contiguous
        for (int k = 0; k < 8; ++k) {
            if (k == 7 && !radius) break;
            const int kind = k < 7 ? c[k].kind : radius[i].kind;
            if (kind < RT_ANIM_NONE || kind > RT_ANIM_SIN_OFFSET) {
                set_error(std::string(who) + ": object " + std::to_string(i) + " has a channel of unknown kind " +
                          std::to_string(kind));
                return RT_ERR_INVALID;
            }
        }
    }
    for (int i = 0; i < n_objs; ++i) {
        const float r = radius ? anim_channel(radius[i], time, base[i].radius) : base[i].radius;
        out[i] = animate_object(base[i], anim[i], time);
        out[i].radius = r;
    }
    return RT_OK;
}

int rt_animate_objects(const rt_object *base, const rt_object_anim *anim, int n_objs, float time, rt_object *out) {
    return animate_objects("rt_animate_objects", base, anim, nullptr, n_objs, time, out);
}

int rt_animate_objects2(const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius, int n_objs,
                        float time, rt_object *out) {
    return animate_objects("rt_animate_objects2", base, anim, radius, n_objs, time, out);
}

// raytrace_compute.glsl:334-364 (run-time sin / cos and mod() as the
// reference's GL evaluates them, rt_camera.cpp)
int rt_reference_camera(float time, rt_camera *out) {
    if (!out) { set_error("rt_reference_camera: null out"); return RT_ERR_INVALID; }
    float yaw;
    reference_orbit(time, nullptr, out->position, &yaw);
    out->angles[0] = 0.0f;
    out->angles[1] = yaw;
    out->angles[2] = 0.0f;
    out->near_plane = 0.1f;
    out->far_plane = 1000.0f;
    out->aspect = 16.0f / 9.0f;
    out->v_fov = 90.0f;
    return RT_OK;
}

int rt_bench_objects(int n_spheres, uint64_t seed, rt_object *out) {
    if (!out || n_spheres < 0 || n_spheres + 1 > RT_MAX_OBJECTS) {
        set_error("rt_bench_objects: bad arguments");
        return RT_ERR_INVALID;
    }
    float mn[3] = {-11, -11, -11}, mx[3] = {11, 11, 11}, zero[3] = {0, 0, 0};
    make_object(out[0], mn, mx, -1.0f, 0, 0, 0, 0, 0, 0, RT_MAT_WALL);
    static const int cycle[6] = {RT_MAT_MATERIAL1, RT_MAT_MATERIAL2, RT_MAT_RED_GLASS,
                                 RT_MAT_GREEN_GLASS, RT_MAT_BLUE_GLASS, RT_MAT_MIRROR};
    uint64_t st = seed;
    for (int i = 0; i < n_spheres; ++i) {
        const float cx = uniform(st, -8.0, 8.0);
        const float cy = uniform(st, -8.0, 8.0);
        const float cz = uniform(st, -4.0, 4.0);
        const float r = uniform(st, 0.3, 1.2);
        make_object(out[i + 1], zero, zero, r, cx, cy, cz, 0, 0, 0, cycle[i % 6]);
    }
    return RT_OK;
}

// main() :366-392 — P (:411-426) and V = inverse(T * R * Rx(90)) (:538-545),
// unprojection = inverse(P * V).
//  cam == NULL: the reference orbit camera at `time`, evaluated as the
//    reference's GL evaluates it (rt_camera.cpp) — bit-identical to llvmpipe;
//  an explicit camera (no counterpart in the reference, which hard-codes its
//    camera): float64, rounded once.
int rt_make_view(const rt_camera *cam_in, float time, rt_view *out) {
    if (!out) { set_error("rt_make_view: null out"); return RT_ERR_INVALID; }
    if (!cam_in) {
        float speed, yaw;
        reference_orbit(time, &speed, out->origin, &yaw);  // ray start = c.position (:391)
        reference_view_gl(time, out->unprojection, nullptr);
        return RT_OK;
    }
    const rt_camera cam = *cam_in;
    const double q = 1.0 / std::tan(static_cast<double>(kDegToRad * 0.5f * cam.v_fov));
    const double n = cam.near_plane, f = cam.far_plane;
    M4 P{};
    P.m[0][0] = q / cam.aspect;
    P.m[1][1] = q;
    P.m[2][2] = (n + f) / (n - f);
    P.m[2][3] = -1.0;
    P.m[3][2] = (2.0 * n * f) / (n - f);
    const M4 V = inverse(mul(transform(cam.position, cam.angles), rot(0, 90.0f)));
    const M4 U = inverse(mul(P, V));
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) out->unprojection[c * 4 + r] = static_cast<float>(U.m[c][r]);
    std::memcpy(out->origin, cam.position, 12);
    return RT_OK;
}

}  // extern "C"

namespace rtamd {

namespace {

// Build a BVH over the spheres with finite centre and radius (the others can
// never produce a valid hit: their quadratic is NaN or its roots infinite),
// reordering `sph`/`smeta` into leaf order. Median split on the widest
// centroid axis, leaves of <= RT_BVH_LEAF spheres, depth-first layout with skip links.
struct BuildItem {
    SphereRec s;
    SphereMeta m;
    double lo[3], hi[3], c[3];
};

int build_node(std::vector<BuildItem> &items, int begin, int end, std::vector<BvhNode> &nodes,
               std::vector<int> &axes) {
    const int id = static_cast<int>(nodes.size());
    nodes.push_back(BvhNode{});
    axes.push_back(0);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    double clo[3] = {1e300, 1e300, 1e300}, chi[3] = {-1e300, -1e300, -1e300};
    for (int i = begin; i < end; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], items[i].lo[a]);
            hi[a] = std::max(hi[a], items[i].hi[a]);
            clo[a] = std::min(clo[a], items[i].c[a]);
            chi[a] = std::max(chi[a], items[i].c[a]);
        }
    BvhNode &n = nodes[id];
    for (int a = 0; a < 3; ++a) {
        n.lo[a] = std::nextafter(static_cast<float>(lo[a]), -INFINITY);
        n.hi[a] = std::nextafter(static_cast<float>(hi[a]), INFINITY);
    }
#ifndef RT_BVH_LEAF  // leaves of up to 6 spheres: config 4 22.04 -> 21.82 ms against 4 (2: 24.7, 3: 22.3, 8: 21.8;
#define RT_BVH_LEAF 6  // SAH leaf termination at 6-8 spheres: 22.3-29.2 ms); config 3 within 0.5 %
#endif
    if (end - begin <= RT_BVH_LEAF) {
        n.leaf = ((end - begin) << 24) | begin;
        return id;
    }
    // surface-area heuristic: over every axis and every split of the
    // centroid-sorted items, minimise A(left) N(left) + A(right) N(right)
    // (a sphere test costs about one node test; ties keep the median split)
    const int cnt = end - begin;
    auto area = [](const double *l, const double *h) {
        const double dx = h[0] - l[0], dy = h[1] - l[1], dz = h[2] - l[2];
        return dx * dy + dy * dz + dz * dx;
    };
    int best_axis = -1, best_mid = (begin + end) / 2;
#ifndef RT_BVH_MEDIAN
    double best = 1e300;
    std::vector<double> left_area(cnt);
    for (int a = 0; a < 3; ++a) {
        std::sort(items.begin() + begin, items.begin() + end,
                  [a](const BuildItem &x, const BuildItem &y) { return x.c[a] < y.c[a]; });
        double l[3] = {1e300, 1e300, 1e300}, h[3] = {-1e300, -1e300, -1e300};
        for (int i = 0; i < cnt; ++i) {
            for (int k = 0; k < 3; ++k) {
                l[k] = std::min(l[k], items[begin + i].lo[k]);
                h[k] = std::max(h[k], items[begin + i].hi[k]);
            }
            left_area[i] = area(l, h);  // items [begin, begin + i]
        }
        double rl[3] = {1e300, 1e300, 1e300}, rh[3] = {-1e300, -1e300, -1e300};
        for (int i = cnt - 1; i >= 1; --i) {  // right = [begin + i, end)
            for (int k = 0; k < 3; ++k) {
                rl[k] = std::min(rl[k], items[begin + i].lo[k]);
                rh[k] = std::max(rh[k], items[begin + i].hi[k]);
            }
            const double cost = left_area[i - 1] * i + area(rl, rh) * (cnt - i);
            if (cost < best) {
                best = cost;
                best_axis = a;
                best_mid = begin + i;
            }
        }
    }
#endif
    int axis = best_axis;
    if (axis < 0) {  // median split on the widest centroid axis
        axis = 0;
        for (int a = 1; a < 3; ++a)
            if (chi[a] - clo[a] > chi[axis] - clo[axis]) axis = a;
    }
    const int mid = best_mid;
    std::sort(items.begin() + begin, items.begin() + end,
              [axis](const BuildItem &x, const BuildItem &y) { return x.c[axis] < y.c[axis]; });
    nodes[id].leaf = 0;
    axes[id] = axis;
    build_node(items, begin, mid, nodes, axes);
    build_node(items, mid, end, nodes, axes);
    return id;
}

// Subtree sizes make the skip links: in depth-first order a subtree rooted at
// id occupies [id, id + size).
int subtree_size(const std::vector<BvhNode> &nodes, int id) {
    if (nodes[id].leaf) return 1;
    const int left = subtree_size(nodes, id + 1);
    return 1 + left + subtree_size(nodes, id + 1 + left);
}

void set_skips(std::vector<BvhNode> &nodes, int id, int next) {
    nodes[id].skip = next;
    if (nodes[id].leaf) return;
    const int left = id + 1, left_size = subtree_size(nodes, left);
    const int right = left + left_size;
    set_skips(nodes, left, right);
    set_skips(nodes, right, next);
}

// The octant's depth-first order (rt_internal.h, kBvhOctants): the children
// of an inner node split on axis a (left: the lower centroids) are entered
// right first when the octant's d[a] < 0.
static_assert(2 * RT_MAX_OBJECTS < 0x8000, "BVH node indices fit the 16-bit links");
void set_links(const std::vector<BvhNode> &nodes, const std::vector<int> &axes, int id, int next, int oct,
               std::vector<uint32_t> &links) {
    auto enc = [](int n) { return static_cast<uint32_t>(n) & 0xFFFFu; };  // -1 -> 0xFFFF
    if (nodes[id].leaf) {
        links[static_cast<size_t>(id) * kBvhOctants + oct] = enc(next) | (enc(next) << 16);
        return;
    }
    const int left = id + 1, right = left + subtree_size(nodes, left);
    const bool flip = (oct >> axes[id]) & 1;
    const int first = flip ? right : left, second = flip ? left : right;
    links[static_cast<size_t>(id) * kBvhOctants + oct] = enc(first) | (enc(next) << 16);
    set_links(nodes, axes, first, second, oct, links);
    set_links(nodes, axes, second, next, oct, links);
}

// extent: a bound on |coordinate| of every finite object of the scene (the
// origins of the secondary rays that walk the BVH lie on their surfaces).
void build_bvh(std::vector<SphereRec> &sph, std::vector<SphereMeta> &smeta, std::vector<BvhNode> &nodes,
               std::vector<uint32_t> &links, double extent) {
    std::vector<BuildItem> finite, other;
    for (size_t i = 0; i < sph.size(); ++i) {
        BuildItem it{sph[i], smeta[i], {}, {}, {}};
        const double c[3] = {sph[i].cx, sph[i].cy, sph[i].cz};
        const double r = std::sqrt(static_cast<double>(sph[i].rr));  // |radius| as the test sees it
        bool ok = std::isfinite(r);
        const SphereBox box = sphere_box(sph[i], r, extent);
        for (int a = 0; a < 3; ++a) {
            ok = ok && std::isfinite(c[a]);
            it.c[a] = c[a];
            it.lo[a] = box.lo[a];
            it.hi[a] = box.hi[a];
        }
        (ok ? finite : other).push_back(it);
    }
    nodes.clear();
    links.clear();
    if (!finite.empty()) {
        std::vector<int> axes;
        build_node(finite, 0, static_cast<int>(finite.size()), nodes, axes);
        set_skips(nodes, 0, -1);
        links.assign(nodes.size() * kBvhOctants, 0u);
        for (int oct = 0; oct < kBvhOctants; ++oct) set_links(nodes, axes, 0, -1, oct, links);
    }
    // leaf order first, then the spheres that cannot be hit (linear loops only)
    sph.clear();
    smeta.clear();
    for (auto *v : {&finite, &other})
        for (const BuildItem &it : *v) {
            sph.push_back(it.s);
            smeta.push_back(it.m);
        }
}

}  // namespace

// proj*view for culling: the float64 inverse of the view's unprojection, and
// whether the view is a consistent pinhole (every pixel's ray, built as the
// kernel builds it, lies on the line through the origin and its NDC point,
// with positive homogeneous w) so that projected footprints bound ray hits.
bool view_projection(const rt_view &v, float proj[16]) {
    M4 U;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) U.m[c][r] = v.unprojection[c * 4 + r];
    const M4 P = inverse(U);
    bool ok = true;
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 4; ++r) {
            proj[c * 4 + r] = static_cast<float>(P.m[c][r]);
            ok = ok && std::isfinite(P.m[c][r]);
        }
    const double o[3] = {v.origin[0], v.origin[1], v.origin[2]};
    const double ndc[5][2] = {{-1, -1}, {1, -1}, {-1, 1}, {1, 1}, {0, 0}};
    for (int i = 0; i < 5 && ok; ++i) {
        double pt[2][3];
        for (int k = 0; k < 2; ++k) {
            const double z = k == 0 ? 0.5 : 1.0;
            double h[4];
            for (int r = 0; r < 4; ++r)
                h[r] = U.m[0][r] * ndc[i][0] + U.m[1][r] * ndc[i][1] + U.m[2][r] * z + U.m[3][r];
            ok = ok && h[3] > 0.0;
            for (int r = 0; r < 3; ++r) pt[k][r] = h[r] / h[3];
        }
        // distance of the origin from the line through the two points
        double d[3], w[3];
        for (int r = 0; r < 3; ++r) {
            d[r] = pt[1][r] - pt[0][r];
            w[r] = o[r] - pt[0][r];
        }
        const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const double cx = d[1] * w[2] - d[2] * w[1], cy = d[2] * w[0] - d[0] * w[2], cz = d[0] * w[1] - d[1] * w[0];
        const double dist = std::sqrt((cx * cx + cy * cy + cz * cz) / dd);
        const double scale = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) + 1e-12;
        ok = ok && dd > 0.0 && dist <= 1e-5 * scale;
    }
    return ok;
}

// Whether the camera ray's six perspective divisions (raytrace_compute.glsl
// :383-390, ws[k] / ws[3] and we[k] / we[3]) may take the short form
// (rt_kernel.hip div_r: the refined reciprocal of the w component and one
// correction, correctly rounded for b normal in [2^-60, 2^60] and a = +0 or
// |a| in [2^-60, 2^60]) for EVERY pixel of a width x height frame, jittered
// samples included. Each component is ((M[k] vx + M[4+k] vy) + M[8+k] z) +
// M[12+k] in float32 with vx in [-1, (width - hw) / hw], vy likewise and z in
// {0.5, 1}:
//  * a numerator's last operation adds c = M[12+k] != 0 to a float y: a
//    nonzero result is at least 2^-26 |c| (if |y| >= |c| / 2 both are
//    multiples of ulp(c) / 2, else |y + c| > |c| / 2), and an exact
//    cancellation gives +0, never -0; so |c| >= 2^-34 keeps every nonzero
//    numerator at or above 2^-60;
//  * the denominators are the linear function w(vx, vy, z) up to rounding:
//    its extremes over the pixel box are at the corners (float64), and the
//    float32 evaluation differs from it by at most 8 * 2^-24 times the sum
//    of the terms' magnitudes; both sit in [2^-20, 2^20] or in the mirror
//    range, every pixel's w does.
bool camera_short_divisions(const float M[16], int width, int height) {
    const int hw = width / 2, hh = height / 2;
    if (hw <= 0 || hh <= 0) return false;
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(M[i]) || std::fabs(M[i]) > 0x1p40f) return false;
    for (int k = 0; k < 4; ++k)
        if (!(std::fabs(M[12 + k]) >= 0x1p-34f)) return false;
    const double vx[2] = {-1.0, static_cast<double>(width - hw) / hw};
    const double vy[2] = {-1.0, static_cast<double>(height - hh) / hh};
    for (const double z : {0.5, 1.0}) {
        const double mag = std::fabs(M[3]) * std::max(std::fabs(vx[0]), std::fabs(vx[1])) +
                           std::fabs(M[7]) * std::max(std::fabs(vy[0]), std::fabs(vy[1])) + std::fabs(M[11]) * z +
                           std::fabs(M[15]);
        const double err = 8.0 * 0x1p-24 * mag + 0x1p-100;
        double lo = INFINITY, hi = -INFINITY;
        for (const double x : vx)
            for (const double y : vy) {
                const double w = double(M[3]) * x + double(M[7]) * y + double(M[11]) * z + double(M[15]);
                lo = std::min(lo, w);
                hi = std::max(hi, w);
            }
        const bool pos = lo - err >= 0x1p-20 && hi + err <= 0x1p20;
        const bool neg = hi + err <= -0x1p-20 && lo - err >= -0x1p20;
        if (!pos && !neg) return false;
    }
    return true;
}

// The view half of the norm proofs (rt_internal.h kNormProofs): for EVERY pixel
// of a width x height frame the camera ray's d = e3 - s3 (camera_ray) has
// finite components and |d|^2 inside inv_sqrt's [2^-96, 2^100], far inside.
// It stands apart from camera_short_divisions (the general depth-0 kernels take
// the room fast path with IEEE divisions too: either quotient is the correctly
// rounded one). On that function's pixel box and corners, float64:
//  * w is affine in (vx, vy): one sign at the eight corners and wmin, the
//    smallest |w| there less the float32 evaluation's 2^-20 Tw, positive;
//  * each point's components are ratios n_k / w of affine functions of
//    (vx, vy) whose denominator keeps its sign, so they take their extremes
//    over the box at the corners: |component| <= Cmax <= 2^40 keeps every
//    |d_k| below 2^42, finite, and |d|^2 below 2^86;
//  * with u the centre pixel's unit direction, u . e3 and u . s3 are such
//    ratios too; G = min |u . e3 - u . s3| from their corner ranges is a lower
//    bound of |d| for the exact points;
//  * a float32 component differs from the exact one by at most eta =
//    2^-20 (T + Cmax Tw) / wmin: at most eight roundings, 2^-21, of the sums
//    of the terms' magnitudes T (numerators) and Tw (w), |w| >= wmin, the
//    short division correctly rounded, and as much again for slack. The far
//    point's w is a cancellation (Tw / wmin is 10^4 for the reference camera),
//    which this carries. So the computed |d| >= G - 4 eta.
// G >= 2^-40 and G >= 8 eta then leave |d|^2 >= 2^-82.
bool camera_norm_range(const float M[16], int width, int height) {
    const int hw = width / 2, hh = height / 2;
    if (hw <= 0 || hh <= 0) return false;
    const double vx[2] = {-1.0, static_cast<double>(width - hw) / hw};
    const double vy[2] = {-1.0, static_cast<double>(height - hh) / hh};
    const double ax = std::max(std::fabs(vx[0]), std::fabs(vx[1])), ay = std::max(std::fabs(vy[0]), std::fabs(vy[1]));
    const auto point = [&](double x, double y, double z, double out[3]) {
        const double w = double(M[3]) * x + double(M[7]) * y + double(M[11]) * z + double(M[15]);
        for (int k = 0; k < 3; ++k)
            out[k] = (double(M[k]) * x + double(M[4 + k]) * y + double(M[8 + k]) * z + double(M[12 + k])) / w;
        return w;
    };
    double T = 0.0, Tw = 0.0, wmin = INFINITY, cmax = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double t = std::fabs(M[k]) * ax + std::fabs(M[4 + k]) * ay + std::fabs(M[8 + k]) + std::fabs(M[12 + k]);
        (k < 3 ? T : Tw) = std::max(k < 3 ? T : Tw, t);
    }
    double s[3], e[3], u[3];
    point(0.0, 0.0, 0.5, s);
    point(0.0, 0.0, 1.0, e);
    double len = 0.0;
    for (int k = 0; k < 3; ++k) {
        u[k] = e[k] - s[k];
        len += u[k] * u[k];
    }
    len = std::sqrt(len);
    if (!(len > 0.0 && std::isfinite(len))) return false;
    for (double &x : u) x /= len;
    double s_lo = INFINITY, s_hi = -INFINITY, e_lo = INFINITY, e_hi = -INFINITY, w_lo = INFINITY, w_hi = -INFINITY;
    for (const double x : vx)
        for (const double y : vy) {
            const double ws = point(x, y, 0.5, s), we = point(x, y, 1.0, e);
            for (const double w : {ws, we}) {
                wmin = std::min(wmin, std::fabs(w));
                w_lo = std::min(w_lo, w);
                w_hi = std::max(w_hi, w);
            }
            for (int k = 0; k < 3; ++k) cmax = std::max(cmax, std::max(std::fabs(s[k]), std::fabs(e[k])));
            const double ps = u[0] * s[0] + u[1] * s[1] + u[2] * s[2], pe = u[0] * e[0] + u[1] * e[1] + u[2] * e[2];
            s_lo = std::min(s_lo, ps);
            s_hi = std::max(s_hi, ps);
            e_lo = std::min(e_lo, pe);
            e_hi = std::max(e_hi, pe);
        }
    const double G = std::max(e_lo - s_hi, s_lo - e_hi);  // (the ranges apart, either way round)
    wmin -= 0x1p-20 * Tw;
    if (!(wmin > 0.0 && (w_lo > 0.0 || w_hi < 0.0))) return false;
    const double eta = 0x1p-20 * (T + cmax * Tw) / wmin;
    return cmax <= 0x1p40 && G >= 0x1p-40 && G >= 8.0 * eta;  // (a NaN fails)
}

// The kernel's frame_setup (rt_kernel.hip) for a one-view launch, on the
// host: every work-group would otherwise derive the same constants (measured
// 7 % of a 1080p depth-0 frame). Camera terms in float32 with the kernel's
// operation order (dot = x*x + (y*y + z*z); xform_point left to right), so the
// LDS image is bit-identical; footprints in float64 with the same inflation
// and 2-pixel margin — closer to the exact projection than the kernel's
// approximate-reciprocal version, and as conservative.
static void view_frame_setup(const LaunchParams &p, const FrameView &V, const float4 *blob, float4 *out);

void host_frame_setup(LaunchParams &p, const float4 *const *blobs) {
    p.n_frame_consts = 0;
    const int per = view_units(p.layout, false);
    if (per == 0 || per > kMaxViewConsts || p.n_views < 1 || p.n_views * per > kMaxFrameConsts) return;
    for (int k = 0; k < p.n_views; ++k)
        if (!blobs[k]) return;
    for (int k = 0; k < p.n_views; ++k) view_frame_setup(p, p.view[k], blobs[k], p.frame_consts + k * per);
    p.n_frame_consts = per;
}

int host_view_consts(const LaunchParams &p, const FrameView &V, const float4 *blob, float4 *out) {
    const int per = view_units(p.layout, false);
    if (per == 0 || per > kMaxViewConsts || !blob) return 0;
    view_frame_setup(p, V, blob, out);
    return per;
}

// One view's records (host_frame_setup).
static void view_frame_setup(const LaunchParams &p, const FrameView &V, const float4 *blob, float4 *out) {
    const SceneLayout &L = p.layout;
    const int ns = L.n_spheres, nb = L.n_boxes;
    const float ox = V.origin[0], oy = V.origin[1], oz = V.origin[2];
    const int hw = p.width / 2, hh = p.height / 2;
    const bool cull = V.cull && hw > 0 && hh > 0;
    const float *P = V.proj;
    const auto *sph = reinterpret_cast<const SphereRec *>(blob + L.off_spheres);
    const auto *meta = reinterpret_cast<const SphereMeta *>(blob + L.off_smeta);
    const auto *box = reinterpret_cast<const BoxRec *>(blob + L.off_boxes);
    float4 *cam = out, *px = out + ns, *bcam = out + 2 * ns;
    for (int s = 0; s < ns; ++s) {
        const SphereRec c = sph[s];
        const float ocx = ox - c.cx, ocy = oy - c.cy, ocz = oz - c.cz;
        const float dd = ocx * ocx + (ocy * ocy + ocz * ocz);
        cam[s] = make_float4(ocx, ocy, ocz, dd - c.rr);
        const float r = meta[s].radius * 1.001f + 1e-3f;
        bool ok = r == r && c.cx == c.cx && c.cy == c.cy && c.cz == c.cz;
        double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
        for (int i = 0; i < 8 && ok; ++i) {
            const double X = c.cx + ((i & 1) ? r : -r), Y = c.cy + ((i & 2) ? r : -r), Z = c.cz + ((i & 4) ? r : -r);
            const double cw = P[3] * X + P[7] * Y + P[11] * Z + P[15];
            const double cx = P[0] * X + P[4] * Y + P[8] * Z + P[12];
            const double cy = P[1] * X + P[5] * Y + P[9] * Z + P[13];
            ok = cw > 1e-4;
            x0 = std::min(x0, cx / cw);
            x1 = std::max(x1, cx / cw);
            y0 = std::min(y0, cy / cw);
            y1 = std::max(y1, cy / cw);
        }
        const double fx0 = std::floor(x0 * hw + hw) - 2.0, fx1 = std::ceil(x1 * hw + hw) + 2.0;
        const double fy0 = std::floor(y0 * hh + hh) - 2.0, fy1 = std::ceil(y1 * hh + hh) + 2.0;
        const double lim = 1.0e9;
        const bool fin = std::fabs(fx0) < lim && std::fabs(fx1) < lim && std::fabs(fy0) < lim && std::fabs(fy1) < lim;
        int32_t rect[4] = {INT32_MIN / 2, INT32_MAX / 2, INT32_MIN / 2, INT32_MAX / 2};
        if (cull && ok && fin) {
            rect[0] = static_cast<int32_t>(fx0);
            rect[1] = static_cast<int32_t>(fx1);
            rect[2] = static_cast<int32_t>(fy0);
            rect[3] = static_cast<int32_t>(fy1);
        }
        std::memcpy(&px[s], rect, sizeof rect);
    }
    for (int b = 0; b < nb; ++b) {
        const float *m = box[b].w2l;
        const float rx = m[0] * ox + m[1] * oy + m[2] * oz + m[3] * 1.0f;
        const float ry = m[4] * ox + m[5] * oy + m[6] * oz + m[7] * 1.0f;
        const float rz = m[8] * ox + m[9] * oy + m[10] * oz + m[11] * 1.0f;
        const BoxRec &B = box[b];
        const bool inside = B.mins[0] < rx && rx < B.maxs[0] && B.mins[1] < ry && ry < B.maxs[1] && B.mins[2] < rz &&
                            rz < B.maxs[2];
        bcam[b] = make_float4(rx, ry, rz, inside ? 1.0f : 0.0f);
    }
}

// The texel and block cones of an n x n cube map (geometry only: computed
// once per n and kept). Texels are grouped in blocks of kMaskBlock x
// kMaskBlock; a block's reach is its own cone's half-angle plus the largest
// half-angle of its texels.
constexpr int kMaskBlock = 8;
struct MaskCones {
    int n = 0;
    std::vector<double> w, ca, sa;  // per texel (face-major): centre direction, cos / sin of the half-angle
    struct Block {
        int face, r0, r1, c0, c1;
        double w[3], reach, cr, sr;  // centre direction, reach and its cos / sin
    };
    std::vector<Block> blocks;
    // per block, its kMaskSubBlock x kMaskSubBlock sub-blocks (same reach rule)
    std::vector<std::vector<Block>> subs;
};
constexpr int kMaskSubBlock = 2;

const MaskCones &mask_cones(int n) {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<MaskCones>> cache;
    std::lock_guard<std::mutex> lock(mu);
    std::unique_ptr<MaskCones> &slot = cache[n];
    if (slot) return *slot;
    auto unit = [](double v[3]) {
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int k = 0; k < 3; ++k) v[k] /= l;
    };
    auto angle = [](const double a[3], const double b[3]) {
        const double c = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
        return std::acos(std::max(-1.0, std::min(1.0, c)));
    };
    auto mc = std::make_unique<MaskCones>();
    mc->n = n;
    const size_t texels = static_cast<size_t>(6) * n * n;
    mc->w.resize(3 * texels);
    mc->ca.resize(texels);
    mc->sa.resize(texels);
    std::vector<double> alpha(texels);
    for (int f = 0; f < 6; ++f) {
        // face f's point (a, b) in the kernel's cube-map coordinates
        // (direction_texel: the cube instructions' sc / |major|, tc / |major|,
        // column from sc, row from tc), as a direction
        auto face_dir = [f](double a, double b, double q[3]) {
            switch (f) {
                case 0: q[0] = 1.0; q[1] = -b; q[2] = -a; break;   // +x: sc = -z, tc = -y
                case 1: q[0] = -1.0; q[1] = -b; q[2] = a; break;   // -x: sc = z, tc = -y
                case 2: q[0] = a; q[1] = 1.0; q[2] = b; break;     // +y: sc = x, tc = z
                case 3: q[0] = a; q[1] = -1.0; q[2] = -b; break;   // -y: sc = x, tc = -z
                case 4: q[0] = a; q[1] = -b; q[2] = 1.0; break;    // +z: sc = x, tc = -y
                default: q[0] = -a; q[1] = -b; q[2] = -1.0; break; // -z: sc = -x, tc = -y
            }
        };
        // a square [a0, a1] x [b0, b1] of the face: its centre direction and
        // the half-angle of the cone through its corners
        auto cone = [&](double a0, double a1, double b0, double b1, double w[3]) {
            face_dir(0.5 * (a0 + a1), 0.5 * (b0 + b1), w);
            unit(w);
            double al = 0.0;
            for (int k = 0; k < 4; ++k) {
                double q[3];
                face_dir((k & 1) ? a1 : a0, (k & 2) ? b1 : b0, q);
                unit(q);
                al = std::max(al, angle(w, q));
            }
            return al;
        };
        for (int row = 0; row < n; ++row)
            for (int col = 0; col < n; ++col) {
                const size_t t = (static_cast<size_t>(f) * n + row) * n + col;
                alpha[t] = cone(-1.0 + 2.0 * col / n, -1.0 + 2.0 * (col + 1) / n, -1.0 + 2.0 * row / n,
                                -1.0 + 2.0 * (row + 1) / n, &mc->w[3 * t]);
                mc->ca[t] = std::cos(alpha[t]);
                mc->sa[t] = std::sin(alpha[t]);
            }
        auto block = [&](int r0, int c0, int size) {
            MaskCones::Block bl;
            bl.face = f;
            bl.r0 = r0;
            bl.c0 = c0;
            bl.r1 = std::min(n, r0 + size);
            bl.c1 = std::min(n, c0 + size);
            bl.reach = cone(-1.0 + 2.0 * bl.c0 / n, -1.0 + 2.0 * bl.c1 / n, -1.0 + 2.0 * bl.r0 / n,
                            -1.0 + 2.0 * bl.r1 / n, bl.w);
            double amax = 0.0;
            for (int row = bl.r0; row < bl.r1; ++row)
                for (int col = bl.c0; col < bl.c1; ++col)
                    amax = std::max(amax, alpha[(static_cast<size_t>(f) * n + row) * n + col]);
            bl.reach += amax;
            bl.cr = std::cos(bl.reach);
            bl.sr = std::sin(bl.reach);
            return bl;
        };
        for (int r0 = 0; r0 < n; r0 += kMaskBlock)
            for (int c0 = 0; c0 < n; c0 += kMaskBlock) {
                mc->blocks.push_back(block(r0, c0, kMaskBlock));
                const MaskCones::Block &bl = mc->blocks.back();
                std::vector<MaskCones::Block> sub;
                for (int r = bl.r0; r < bl.r1; r += kMaskSubBlock)
                    for (int c = bl.c0; c < bl.c1; c += kMaskSubBlock) sub.push_back(block(r, c, kMaskSubBlock));
                mc->subs.push_back(std::move(sub));
            }
    }
    slot = std::move(mc);
    return *slot;
}

// Build the device blob: [spheres][sphere meta][boxes][materials][lights]
// [light x material products]; every section 16-B aligned.
// Shadow direction masks (rt_internal.h, kMaskMaxSpheres): float64 geometry,
// the cone of each sphere from the light and the texel test of rt_cull.h
// (mask_cone, texel_hit). A texel is the spherical image of a square
// of the cube face; it lies inside the cone around its centre direction
// whose half-angle is the largest angle to its four corners (a cone narrower
// than 90 degrees is convex, so holding the corners it holds the square).
// Spheres are tested texel by texel only in the blocks whose reach their
// cone comes within (a texel's centre lies in its block's cone, so every
// texel the texel test accepts lies in an accepted block): the bits set are
// those of the texel-by-texel test alone.
static void build_direction_masks(const std::vector<SphereRec> &sph, const std::vector<SphereMeta> &smeta,
                           const rt_light *lights, const std::vector<LightRec> &lrec, int n,
                           std::vector<uint64_t> &out, int words = 1) {
    const int n_lights = static_cast<int>(lrec.size());
    const MaskCones &mc = mask_cones(n);
    out.clear();
    for (int j = 0; j < n_lights; ++j) {
        if (lrec[j].dead != 0.0f) continue;
        // each sphere's cone from this light (rt_cull.h), with cos / sin of
        // half + 1e-3 per sphere and of alpha per texel: no inverse cosine per
        // (texel, sphere)
        std::vector<MaskCone> cone(sph.size());
        std::vector<double> half(sph.size());
        for (size_t s = 0; s < sph.size(); ++s) {
            const float ball[4] = {sph[s].cx, sph[s].cy, sph[s].cz, smeta[s].radius};
            cone[s] = mask_cone(ball, lights[j].position, static_cast<int>(s), &half[s]);
        }
        const size_t base = out.size();
        out.resize(base + static_cast<size_t>(6) * n * n * words, 0u);
        for (const MaskCones::Block &bl : mc.blocks)
            for (size_t s = 0; s < sph.size(); ++s) {
                const MaskCone &c = cone[s];
                if (!c.every) {
                    // cos(reach + half + 1e-3), less a margin for rounding
                    const double lim = bl.cr * c.ch - bl.sr * c.sh - 1e-9;
                    const double dot = bl.w[0] * c.ax[0] + bl.w[1] * c.ax[1] + bl.w[2] * c.ax[2];
                    if (bl.reach + half[s] + 1e-3 < 3.141592653589793 && dot < lim) continue;
                }
                for (int row = bl.r0; row < bl.r1; ++row)
                    for (int col = bl.c0; col < bl.c1; ++col) {
                        const size_t t = (static_cast<size_t>(bl.face) * n + row) * n + col;
                        if (texel_hit(&mc.w[3 * t], mc.ca[t], mc.sa[t], c))
                            out[base + t * words + s / 64] |= uint64_t{1} << (s % 64);
                    }
            }
    }
}

// Origin-sphere candidate lists of the secondary rays (rt_internal.h,
// kOListSlots): float64 geometry, the spheres in their final (BVH) slot order.
// Every reflection or refraction ray that leaves sphere s starts within
// 0.001 of its surface (:1010-1023: p +- 0.001 n), so inside the ball
// B(c_s, r_s + 0.001); it can hit sphere j only in a direction within
// asin(rin / d) of (c_j - c_s) / d, rin = r_j + r_s + 0.001 + margins, d =
// |c_j - c_s| (any direction when d <= rin) — the shadow masks' cone test
// with the origin ball folded into the target, texel by texel in the blocks
// the sphere's cone reaches. The margins (1e-3 + 1e-4 of the coordinates'
// magnitude, plus 1e-3 rad) dwarf the float32 error of the kernel's hit
// points, offsets and approximate texel lookup. A candidate's bound is a
// lower bound of the ray parameter of any hit on it from that ball: the
// distance between the balls, shrunk by the same margins and by 1e-5 for
// ray directions that are unit vectors only up to rounding; stored rounded
// down in 1/256 units, so a lane that stops on `best t < bound` drops only
// spheres whose hit would lie strictly farther (no tie can be lost).
static void origin_lists_range(const std::vector<SphereRec> &sph, const std::vector<SphereMeta> &smeta, int n,
                               std::vector<uint8_t> &out, size_t s_begin, size_t s_end) {
    const size_t ns = sph.size();
    const MaskCones &mc = mask_cones(n);
    const size_t texels = static_cast<size_t>(6) * n * n;
    std::vector<double> ax(3 * ns), ch(ns), sh(ns), lb(ns), reach(ns);
    std::vector<char> every(ns);
    // the spheres' cone data in list order (o*), a block's candidates (k*) and
    // a sub-block's (s*), contiguous
    std::vector<int> order(ns), kq(ns), sq(ns);
    std::vector<double> ox(ns), oy(ns), oz(ns), oc(ns), osn(ns), orc(ns);
    std::vector<double> kx(ns), ky(ns), kz(ns), kc(ns), ksn(ns), kr(ns);
    std::vector<double> sx(ns), sy(ns), sz(ns), sc(ns), ss(ns);
    std::vector<char> oe(ns), ke(ns), se(ns), keep(ns), hit(ns);
    std::vector<std::pair<double, int>> list;  // one texel's candidates: (bound, slot)
    auto quant = [](double x) -> uint16_t {  // rounded down, saturating (a smaller bound stays a bound)
        if (!(x > 0.0)) return 0;
        const double q = std::floor(x / static_cast<double>(kOListBoundUnit));
        return static_cast<uint16_t>(std::min(q, 65535.0));
    };
    for (size_t s = s_begin; s < s_end; ++s) {
        const double cs[3] = {sph[s].cx, sph[s].cy, sph[s].cz};
        const double rs = smeta[s].radius;
        const double ms = std::sqrt(cs[0] * cs[0] + cs[1] * cs[1] + cs[2] * cs[2]);
        for (size_t j = 0; j < ns; ++j) {
            const double v[3] = {double(sph[j].cx) - cs[0], double(sph[j].cy) - cs[1], double(sph[j].cz) - cs[2]};
            const double d = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            const double cj = std::sqrt(double(sph[j].cx) * sph[j].cx + double(sph[j].cy) * sph[j].cy +
                                        double(sph[j].cz) * sph[j].cz);
            const double rj = smeta[j].radius;
            const double margin = 1e-3 + 1e-4 * (d + ms + cj + rs + rj);
            const double rin = rj + rs + 0.001 + margin;
            const bool ok = std::isfinite(d) && std::isfinite(rin) && std::isfinite(margin);
            lb[j] = j == s ? -1.0 : (ok ? std::max(0.0, (d - rj - rs - 0.001 - 2.0 * margin) * (1.0 - 1e-5)) : 0.0);
            every[j] = !ok || d <= rin;
            if (every[j]) continue;
            for (int k = 0; k < 3; ++k) ax[3 * j + k] = v[k] / d;
            const double half = std::asin(std::min(1.0, rin / d));
            reach[j] = half + 1e-3;
            ch[j] = std::cos(reach[j]);
            sh[j] = std::sin(reach[j]);
        }
        // The spheres in list order, (bound, slot) ascending: every list
        // below is built by walking them in this order, so it comes out
        // sorted. A (sub-)block is skipped for sphere j when j's cone misses
        // the block's reach (every texel the texel test accepts lies in an
        // accepted block and sub-block); the tests run over contiguous
        // arrays of the candidates' cone data.
        for (size_t j = 0; j < ns; ++j) order[j] = static_cast<int>(j);
        std::sort(order.begin(), order.end(), [&](int x, int y) { return lb[x] < lb[y] || (lb[x] == lb[y] && x < y); });
        for (size_t q = 0; q < ns; ++q) {
            const int j = order[q];
            ox[q] = ax[3 * j];
            oy[q] = ax[3 * j + 1];
            oz[q] = ax[3 * j + 2];
            oc[q] = ch[j];
            osn[q] = sh[j];
            orc[q] = reach[j];
            oe[q] = every[j];
        }
        // reach test of a block against candidates [0, m) of (x, y, z, c, sn, r, e): keep[] = 1 if it may reach
        auto reach_test = [](const MaskCones::Block &bl, size_t m, const double *x, const double *y, const double *z,
                             const double *c, const double *sn, const double *r, const char *e, char *keep) {
            for (size_t q = 0; q < m; ++q)
                keep[q] = e[q] | static_cast<char>(bl.reach + r[q] >= 3.141592653589793) |
                          static_cast<char>(bl.w[0] * x[q] + bl.w[1] * y[q] + bl.w[2] * z[q] >=
                                            bl.cr * c[q] - bl.sr * sn[q] - 1e-9);
        };
        for (size_t k = 0; k < mc.blocks.size(); ++k) {
            reach_test(mc.blocks[k], ns, ox.data(), oy.data(), oz.data(), oc.data(), osn.data(), orc.data(), oe.data(),
                       keep.data());
            size_t mk = 0;  // the block's candidates, in list order
            for (size_t q = 0; q < ns; ++q)
                if (keep[q]) {
                    kq[mk] = static_cast<int>(q);
                    kx[mk] = ox[q];
                    ky[mk] = oy[q];
                    kz[mk] = oz[q];
                    kc[mk] = oc[q];
                    ksn[mk] = osn[q];
                    kr[mk] = orc[q];
                    ke[mk] = oe[q];
                    ++mk;
                }
            for (const MaskCones::Block &sb : mc.subs[k]) {
                reach_test(sb, mk, kx.data(), ky.data(), kz.data(), kc.data(), ksn.data(), kr.data(), ke.data(),
                           keep.data());
                size_t m = 0;  // the sub-block's candidates, in list order
                for (size_t q = 0; q < mk; ++q)
                    if (keep[q]) {
                        sq[m] = kq[q];
                        sx[m] = kx[q];
                        sy[m] = ky[q];
                        sz[m] = kz[q];
                        sc[m] = kc[q];
                        ss[m] = ksn[q];
                        se[m] = ke[q];
                        ++m;
                    }
                for (int row = sb.r0; row < sb.r1; ++row)
                    for (int col = sb.c0; col < sb.c1; ++col) {
                        const size_t t = (static_cast<size_t>(sb.face) * n + row) * n + col;
                        const double w0 = mc.w[3 * t], w1 = mc.w[3 * t + 1], w2 = mc.w[3 * t + 2];
                        const double ca = mc.ca[t], sa = mc.sa[t];
                        // (reach < pi / 2 + 1e-3 and a texel's half-angle is small: the summed
                        // angle stays below pi, where the cosine test is exact)
                        for (size_t q = 0; q < m; ++q)
                            hit[q] = se[q] | static_cast<char>(w0 * sx[q] + w1 * sy[q] + w2 * sz[q] >=
                                                               ca * sc[q] - sa * ss[q] - 1e-12);
                        list.clear();  // (list order already)
                        for (size_t q = 0; q < m; ++q)
                            if (hit[q]) list.push_back({lb[order[sq[q]]], order[sq[q]]});
                        uint8_t *rec = out.data() + (s * texels + t) * kOListRecordBytes;
                        const size_t cnt = list.size();
                        rec[0] = static_cast<uint8_t>(std::min<size_t>(cnt, 255));
                        for (size_t i = 0; i < cnt && i < static_cast<size_t>(kOListSlots); ++i)
                            rec[1 + i] = static_cast<uint8_t>(list[i].second);
                        const uint16_t bnd[3] = {cnt > 8 ? quant(list[8].first) : uint16_t{65535},
                                                 cnt > 16 ? quant(list[16].first) : uint16_t{65535},
                                                 cnt > static_cast<size_t>(kOListSlots)
                                                     ? quant(list[kOListSlots].first)
                                                     : uint16_t{65535}};
                        std::memcpy(rec + 1 + kOListSlots, bnd, sizeof bnd);
                    }
            }
        }
    }
}

// The lists of all spheres: independent per origin sphere, built on up to 16
// host threads (256 spheres: about 130 ms of host work on one thread). A
// thread that cannot be started (std::system_error, e.g. a process thread
// limit) leaves its range to the calling thread: nothing throws out of here.
static void build_origin_lists(const std::vector<SphereRec> &sph, const std::vector<SphereMeta> &smeta, int n,
                               std::vector<uint8_t> &out) {
    const size_t ns = sph.size();
    out.assign(ns * static_cast<size_t>(6) * n * n * kOListRecordBytes, 0);
    (void)mask_cones(n);  // (built once, before the workers share it)
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t n_thr = std::min<size_t>({16, hw, (ns + 15) / 16});
    if (n_thr <= 1) {
        origin_lists_range(sph, smeta, n, out, 0, ns);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve(n_thr);
    const size_t per = (ns + n_thr - 1) / n_thr;
    size_t started = 0;  // [0, started) is covered by the running workers
    for (size_t k = 0; k < n_thr; ++k) {
        const size_t a = k * per, b = std::min(ns, a + per);
        if (a >= b) break;
        try {
            pool.emplace_back(origin_lists_range, std::cref(sph), std::cref(smeta), n, std::ref(out), a, b);
        } catch (const std::system_error &) {
            break;
        }
        started = b;
    }
    if (started < ns) origin_lists_range(sph, smeta, n, out, started, ns);
    for (std::thread &t : pool) t.join();
}

// The origin-sphere lists of a built scene, from its host blob (the sphere
// records the kernel stages): empty unless the scene has
// kOListMinSpheres..256 spheres (DeviceScene::olist_eligible).
int build_origin_lists_for(const std::vector<float4> &host, const DeviceScene &ds, std::vector<uint8_t> &olist) {
    olist.clear();
    if (!ds.olist_eligible) return RT_OK;
    const size_t ns = static_cast<size_t>(ds.layout.n_spheres);
    if (host.size() * sizeof(float4) < (static_cast<size_t>(ds.layout.off_smeta) * 16 + ns * sizeof(SphereMeta)) ||
        host.size() * sizeof(float4) < (static_cast<size_t>(ds.layout.off_spheres) * 16 + ns * sizeof(SphereRec))) {
        set_error("origin lists: the scene's host copy is incomplete");
        return RT_ERR_INVALID;
    }
    std::vector<SphereRec> sph(ns);
    std::vector<SphereMeta> smeta(ns);
    const char *base = reinterpret_cast<const char *>(host.data());
    std::memcpy(sph.data(), base + static_cast<size_t>(ds.layout.off_spheres) * 16, ns * sizeof(SphereRec));
    std::memcpy(smeta.data(), base + static_cast<size_t>(ds.layout.off_smeta) * 16, ns * sizeof(SphereMeta));
    try {
        build_origin_lists(sph, smeta, kOListTexels, olist);
    } catch (const std::bad_alloc &) {
        olist.clear();
        set_error("origin lists: out of memory");
        return RT_ERR_NOMEM;
    }
    return RT_OK;
}

int object_kind_of(const rt_object &o) { return object_kind(o); }

double objects_extent(const rt_object *objs, int n_objs) {
    double extent = 0.0;
    for (int i = 0; i < n_objs; ++i) {
        const rt_object &o = objs[i];
        double e = std::sqrt(static_cast<double>(o.position[0]) * o.position[0] +
                             static_cast<double>(o.position[1]) * o.position[1] +
                             static_cast<double>(o.position[2]) * o.position[2]);
        double corner = std::fabs(static_cast<double>(o.radius));
        for (int a = 0; a < 3; ++a)
            corner = std::max(corner, std::max(std::fabs(static_cast<double>(o.box_mins[a])),
                                               std::fabs(static_cast<double>(o.box_maxs[a]))));
        e += corner * std::sqrt(3.0);
        if (std::isfinite(e)) extent = std::max(extent, e);
    }
    return extent;
}

MaskConeTable mask_cone_table(int n) {
    const MaskCones &mc = mask_cones(n);
    return MaskConeTable{n, mc.w.data(), mc.ca.data(), mc.sa.data()};
}

int build_scene(const rt_object *objs, int n_objs, const rt_material *mats, int n_mats, const rt_light *lights,
                int n_lights, std::vector<float4> &blob, DeviceScene &ds, bool with_origin_lists,
                double extent_floor) {
    SceneLayout &lay = ds.layout;
    std::vector<SphereRec> sph;
    std::vector<SphereMeta> smeta;
    std::vector<BoxRec> boxes;
    std::vector<float4> ball;  // the boxes' bounding balls (mask bits)
    for (int i = 0; i < n_objs; ++i) {
        const rt_object &o = objs[i];
        const int kind = object_kind(o);
        if (kind == 0) continue;
        if (o.material < 0 || o.material >= n_mats) {
            set_error("rt_scene_create: object " + std::to_string(i) + " has material index out of range");
            return RT_ERR_INVALID;
        }
        if (kind == 2) {
            sph.push_back({o.position[0], o.position[1], o.position[2], o.radius * o.radius});
            // |radius| for the culling bounds (a negative radius other than -1
            // is a sphere of radius |r|: the test only sees r*r, :588)
            smeta.push_back({i, o.material, std::fabs(o.radius), 0});
        } else {
            // the record and the culling terms, as the animate kernel derives them (rt_cull.h)
            BoxRec b{};
            box_record(o, b);
            b.obj_index = i;
            b.material = o.material;
            double R[3][3];
            rotation64(o.angles, R);
            for (int j = 0; j < n_lights && j < 32; ++j)
                if (light_inside_box(o, R, lights[j].position)) b.light_inside |= 1u << j;
            boxes.push_back(b);
            ball.push_back(box_ball(o, R));
        }
    }
    // |coordinate| bound of the finite objects (BVH margins); an animated
    // scene's template passes the bound over its supported times (any larger
    // value only widens the margins)
    const double extent = std::max(objects_extent(objs, n_objs), extent_floor);
    std::vector<BvhNode> bvh;
    std::vector<uint32_t> blink;
    build_bvh(sph, smeta, bvh, blink, extent);
    std::vector<MatRec> mrec(n_mats);
    std::vector<LightMatRec> lm(static_cast<size_t>(n_mats) * n_lights);
    for (int m = 0; m < n_mats; ++m) {
        MatRec &r = mrec[m];
        for (int k = 0; k < 4; ++k) {
            float acc = 0.0f;  // ambient = vec4(0.0); ambient += La * Ma (:793, :801)
            for (int j = 0; j < n_lights; ++j) acc = acc + lights[j].ambient[k] * mats[m].ambient[k];
            r.amb_sum[k] = acc;
            r.emissive[k] = mats[m].emissive[k];
        }
        r.shininess = mats[m].shininess;
        r.reflectivity = mats[m].reflectivity;
        r.transparency = mats[m].transparency;
        r.refraction_index = mats[m].refraction_index;
        r.eta_in = 1.0f / r.refraction_index;  // the ratio of a ray entering (IEEE division, as the kernel's)
        r.eta_out = 1.0f / r.eta_in;           // and of one leaving the object
        // tame: every product finite and shininess in (0, 1e6): then the
        // diffuse factor max(cos, 0) <= 1 + 2^-20 and pow(max(cos, 0),
        // shininess) are finite (pow is skipped for a zero base; its exp2
        // argument stays below 128 for such bases and exponents) and a light
        // whose products are zero, or whose factor is zero, adds only +-0 to
        // the sums (which start at +0 and so are never -0): its shadow ray
        // cannot change the colour.
        bool tame = mats[m].shininess > 0.0f && mats[m].shininess < 1e6f;
        for (int j = 0; j < n_lights; ++j) {
            LightMatRec &q = lm[m * n_lights + j];
            for (int k = 0; k < 4; ++k) {
                q.ld_md[k] = lights[j].diffuse[k] * mats[m].diffuse[k];   // :830
                q.ls_ms[k] = lights[j].specular[k] * mats[m].specular[k];  // :832
                q.d_nz |= q.ld_md[k] != 0.0f;
                q.s_nz |= q.ls_ms[k] != 0.0f;
                tame = tame && std::isfinite(q.ld_md[k]) && std::isfinite(q.ls_ms[k]);
            }
        }
        for (int j = 0; j < n_lights; ++j) lm[m * n_lights + j].always = tame ? 0 : 1;
    }
    // Shadow culling cones of every (light, sphere) pair (rt_cull.h).
    std::vector<ShadowCone> cones(static_cast<size_t>(n_lights) * sph.size());
    for (int j = 0; j < n_lights; ++j)
        for (size_t s = 0; s < sph.size(); ++s)
            cones[j * sph.size() + s] = shadow_cone(sph[s], smeta[s].radius, lights[j].position);
    // A light with zero diffuse and specular colour (the reference's ambient
    // light, :202-207) adds +-0 to the sums for every finite material with
    // shininess >= 0 (pow then stays finite), so lit and shadowed agree and
    // the kernel may skip it; its ambient term is in amb_sum.
    bool materials_tame = true;
    for (int m = 0; m < n_mats; ++m) {
        // (shininess below 1e6 keeps pow's exp2 argument below 128: finite)
        materials_tame = materials_tame && mats[m].shininess >= 0.0f && mats[m].shininess < 1e6f;
        for (int k = 0; k < 4; ++k)
            materials_tame = materials_tame && std::isfinite(mats[m].diffuse[k]) && std::isfinite(mats[m].specular[k]);
    }
    std::vector<LightRec> lrec(n_lights);
    for (int j = 0; j < n_lights; ++j) {
        std::memcpy(lrec[j].pos, lights[j].position, 12);
        bool zero = true;
        for (int k = 0; k < 4; ++k) zero = zero && lights[j].diffuse[k] == 0.0f && lights[j].specular[k] == 0.0f;
        lrec[j].dead = (zero && materials_tame) ? 1.0f : 0.0f;
    }
    auto units = [](size_t bytes) { return static_cast<int32_t>((bytes + 15) / 16); };
    int32_t off = 0;
    lay.off_spheres = off; off += units(sph.size() * sizeof(SphereRec));
    lay.off_smeta = off;   off += units(smeta.size() * sizeof(SphereMeta));
    lay.off_boxes = off;   off += units(boxes.size() * sizeof(BoxRec));
    lay.off_mats = off;    off += units(mrec.size() * sizeof(MatRec));
    lay.off_lights = off;  off += units(lrec.size() * sizeof(LightRec));
    lay.off_lightmat = off; off += units(lm.size() * sizeof(LightMatRec));
    // Round 6: in a scene of several boxes (chosen by the object kinds alone,
    // as the mask bits), per (box, light) the separating plane (rt_cull.h).
    std::vector<float4> bplane;
    lay.off_bplane = -1;
    if (boxes.size() >= 2) {
        bool finite = true;  // (a non-finite object: no planes; shaded points are bounded by `extent` otherwise)
        for (int i = 0; i < n_objs; ++i)
            for (int k = 0; k < 3; ++k)
                finite = finite && std::isfinite(objs[i].position[k]) && std::isfinite(objs[i].box_mins[k]) &&
                         std::isfinite(objs[i].box_maxs[k]) && std::isfinite(objs[i].radius);
        bplane.assign(boxes.size() * static_cast<size_t>(n_lights), no_plane());
        for (size_t b = 0; b < boxes.size() && finite; ++b)
            for (int j = 0; j < n_lights; ++j)
                bplane[b * n_lights + j] = box_light_plane(boxes[b], lights[j].position, extent);
        lay.off_bplane = off;
        off += units(bplane.size() * sizeof(float4));
    }
    lay.off_bvh = off;     off += units(bvh.size() * sizeof(BvhNode));
    lay.off_blink = off;   off += units(blink.size() * sizeof(uint32_t));
    // The cone table rides in LDS only while the work-group's LDS stays small
    // enough for full occupancy (config 4's 256 spheres x 3 lights would add
    // 24 KB and cut the resident work-groups per CU); without it the kernel
    // derives the cones per wave (off_cone = -1).
    const size_t per_frame = sph.size() * 32 + boxes.size() * 16;
    // Direction masks replace the cone table where they fit (finest texels first).
    int n_live = 0;
    for (int j = 0; j < n_lights; ++j) n_live += lrec[j].dead == 0.0f;
    std::vector<uint64_t> dmask;
    lay.off_dmask = -1;
    lay.dmask_n = 0;
    // Round 6: in a scene of several boxes the boxes get mask bits too (bit
    // n_spheres + b), from their bounding balls (rt_cull.h). The choice depends
    // on the object kinds alone (the blob layout rt_render_batch_scenes
    // requires to be shared by the frames of an animated scene): a one-box
    // scene — the room of configs 2-5 — keeps its box's shortcuts instead.
    const bool box_bits = boxes.size() >= 2;
    const size_t mask_bits = sph.size() + (box_bits ? boxes.size() : 0);
    lay.dmask_box = 0;
    lay.dmask_bytes = 4;  // (without masks)
    bool fixed = false;   // the scene takes its layout class's offsets (below)
    if (!sph.empty() && mask_bits <= static_cast<size_t>(kMaskMaxSpheres) && n_live > 0) {
        lay.dmask_bytes = mask_bits <= 16 ? 2 : (mask_bits <= 32 ? 4 : 8);
#ifndef RT_DMASK_MAXN
#define RT_DMASK_MAXN 12
#endif
        // the finest texels whose masks fit beside `head` units of tables
        const auto texels = [&](int32_t head) {
            for (int n : {32, 24, 16, 12, 8}) {
                if (n > RT_DMASK_MAXN) continue;
                const size_t bytes = static_cast<size_t>(n_live) * 6 * n * n * lay.dmask_bytes;
                if ((static_cast<size_t>(head) + units(bytes)) * 16 + per_frame <= kMaskLdsBudget) return n;
            }
            return 0;
        };
        lay.dmask_n = texels(off);
        // The scene's layout class (rt_internal.h fixed_layout): inside the
        // maxima, and the padding leaves the masks their texels. Then the
        // tables move to the class's offsets, the masks follow them, and the
        // planes, the BVH and its links go behind the masks; else the compact
        // layout above stands.
        if (lay.dmask_n > 0 && fixed_counts(static_cast<int>(sph.size()), static_cast<int>(boxes.size()), n_mats, n_lights)) {
            const FixedLayout f = fixed_layout(boxes.size() == 1);
            const int32_t n_sph = static_cast<int32_t>(sph.size());
            const int32_t tail = off - lay.off_lightmat - units(lm.size() * sizeof(LightMatRec));  // planes, BVH, links
            if (texels(f.off_dmask(n_sph) + tail) == lay.dmask_n) {
                fixed = true;
                lay.off_boxes = f.off_boxes;
                lay.off_mats = f.off_mats;
                lay.off_lights = f.off_lights;
                lay.off_lightmat = f.off_lightmat;
                lay.off_spheres = f.off_spheres;
                lay.off_smeta = f.off_smeta(n_sph);
                off = f.off_dmask(n_sph);
            }
        }
    }
    std::vector<char> dmask_bytes;
    if (lay.dmask_n > 0) {
        if (box_bits) {
            std::vector<SphereRec> bsph(sph);
            std::vector<SphereMeta> bmeta(smeta);
            for (size_t b = 0; b < boxes.size(); ++b) {
                bsph.push_back({ball[b].x, ball[b].y, ball[b].z, 0.0f});
                bmeta.push_back({boxes[b].obj_index, boxes[b].material, ball[b].w, 0});
            }
            build_direction_masks(bsph, bmeta, lights, lrec, lay.dmask_n, dmask);
            lay.dmask_box = 1;
        } else {
            build_direction_masks(sph, smeta, lights, lrec, lay.dmask_n, dmask);
        }
        lay.off_dmask = off;
        dmask_bytes.resize(dmask.size() * lay.dmask_bytes);
        for (size_t i = 0; i < dmask.size(); ++i)  // little-endian: the low bytes of each mask
            std::memcpy(dmask_bytes.data() + i * lay.dmask_bytes, &dmask[i], lay.dmask_bytes);
        off += units(dmask_bytes.size());
        cones.clear();
    }
    if (fixed) {  // (the planes stay right before the BVH, as in the compact layout)
        if (lay.off_bplane >= 0) {
            lay.off_bplane = off;
            off += units(bplane.size() * sizeof(float4));
        }
        lay.off_bvh = off;     off += units(bvh.size() * sizeof(BvhNode));
        lay.off_blink = off;   off += units(blink.size() * sizeof(uint32_t));
    }
    const size_t with_cones = (static_cast<size_t>(off) + units(cones.size() * sizeof(ShadowCone))) * 16 + per_frame;
    if (lay.dmask_n == 0 && with_cones <= kConeLdsBudget) {
        lay.off_cone = off;
        off += units(cones.size() * sizeof(ShadowCone));
    } else {
        lay.off_cone = -1;
        cones.clear();
    }
    lay.n_bvh = static_cast<int32_t>(bvh.size());
    lay.blob_units = off;  // the part every work-group stages into LDS
    // Scenes above RT_GMASK_FROM spheres: wide direction masks (kGMaskMaxSpheres),
    // also beside the LDS masks (depth 0-1 keep those; depth >= 2 reads these),
    // kept in the device blob past the staged part and read through L2.
    std::vector<uint64_t> gmask;
    std::vector<uint8_t> glist;
    lay.off_gmask = -1;
    lay.off_glist = -1;
    lay.gmask_words = 0;
#ifndef RT_GMASK_FROM
#define RT_GMASK_FROM 32  // wide masks above this many spheres at depth >= 2 (tools/ablate.sh flags; config 3, 64 spheres: 1.15 -> 1.11 ms)
#endif
    if (sph.size() > static_cast<size_t>(RT_GMASK_FROM) &&
        sph.size() <= static_cast<size_t>(kGMaskMaxSpheres) && n_live > 0) {
        lay.gmask_words = static_cast<int32_t>((sph.size() + 63) / 64);
        build_direction_masks(sph, smeta, lights, lrec, kGMaskTexels, gmask, lay.gmask_words);
        lay.off_gmask = off;
        off += units(gmask.size() * 8);
        // the candidate lists of the same texels (rt_internal.h kGListMax)
        const size_t n_texels = gmask.size() / static_cast<size_t>(lay.gmask_words);
        glist.assign(n_texels * 16, 0);
        // each live light's order of the spheres: largest angular size seen
        // from the light first (a light inside a sphere's inflated bound, or
        // a non-finite sphere, first of all), so a shadowed query meets its
        // occluder early and its any-hit walk ends (the result is
        // order-independent). CPU model (tools/model/shadow_model.py): the
        // wave's candidate passes per shadow call 2.34 -> 1.47 on config 4,
        // 0.95 -> 0.73 on config 3.
        std::vector<int> live;
        for (int j = 0; j < n_lights; ++j)
            if (lrec[j].dead == 0.0f) live.push_back(j);
        std::vector<std::vector<int>> rank_of(live.size(), std::vector<int>(sph.size()));
        for (size_t k = 0; k < live.size(); ++k) {
            const rt_light &L = lights[live[k]];
            std::vector<double> key(sph.size());
            for (size_t q = 0; q < sph.size(); ++q) {
                const float c[3] = {sph[q].cx, sph[q].cy, sph[q].cz};
                double v[3], d, rp;
                key[q] = ball_from_light(c, smeta[q].radius, L.position, v, d, rp) ? double(smeta[q].radius) / d
                                                                                    : HUGE_VAL;
            }
            std::vector<int> order(sph.size());
            for (size_t q = 0; q < sph.size(); ++q) order[q] = static_cast<int>(q);
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key[x] > key[y]; });
            for (size_t q = 0; q < order.size(); ++q) rank_of[k][order[q]] = static_cast<int>(q);
        }
        const size_t per_light = n_texels / (live.empty() ? 1 : live.size());
        for (size_t t = 0; t < n_texels; ++t) {
            uint8_t *rec = glist.data() + t * 16;
            const std::vector<int> &rk = rank_of[t / per_light];
            int n = 0;
            // the same truncation as the kernel's word walk (occluded: the
            // last word masked to the `rest` = ns - 64 w live slots)
            const int ns = static_cast<int>(sph.size());
            for (int w = 0; w < lay.gmask_words; ++w) {
                uint64_t bits = gmask[t * lay.gmask_words + w];
                const int rest = ns - 64 * w;
                if (rest < 64) bits &= (uint64_t{1} << rest) - 1u;
                for (; bits; bits &= bits - 1) {
                    if (n < kGListMax) rec[1 + n] = static_cast<uint8_t>(64 * w + __builtin_ctzll(bits));
                    ++n;
                }
            }
            rec[0] = n <= kGListMax ? static_cast<uint8_t>(n) : static_cast<uint8_t>(kGListOverflow);
            if (n <= kGListMax)
                std::sort(rec + 1, rec + 1 + n, [&](uint8_t x, uint8_t y) { return rk[x] < rk[y]; });
        }
        lay.off_glist = off;
        off += units(glist.size());
    }
    // The secondary rays' origin-sphere candidate lists (rt_internal.h
    // kOListSlots), past the staged part like the wide masks. Only depth >= 2
    // renders read them, and they cost tens of ms of host work and up to
    // 12.6 MB at 256 spheres: a scene is created without them, and the first
    // render that reads them appends them to the device blob
    // (ensure_origin_lists, rt_api.cpp; never to the host copy).
    // with_origin_lists: built here, at the blob's end (the CPU models'
    // rt_debug_scene_blob).
    std::vector<uint8_t> olist;
    lay.off_olist = -1;
    ds.olist_eligible = sph.size() >= static_cast<size_t>(kOListMinSpheres) && sph.size() <= 256;
    if (ds.olist_eligible && with_origin_lists) {
        build_origin_lists(sph, smeta, kOListTexels, olist);
        lay.off_olist = off;
        off += units(olist.size());
    }
    lay.n_spheres = static_cast<int32_t>(sph.size());
    lay.n_boxes = static_cast<int32_t>(boxes.size());
    ds.room = boxes.size() == 1 && boxes[0].translate_only;
    for (int j = 0; j < n_lights && ds.room; ++j)
        if (lrec[j].dead == 0.0f && (j >= 32 || !((boxes[0].light_inside >> j) & 1u))) ds.room = 0;
    ds.room_fast = ds.room && room_record_identity(boxes[0]);
    ds.norm = NormProof{};
    if (ds.room_fast)
        ds.norm = norm_proof_scene(boxes[0], sph.data(), smeta.data(), static_cast<int>(sph.size()), lrec.data(), n_lights);
    lay.n_mats = n_mats;
    lay.n_lights = n_lights;
    blob.assign(static_cast<size_t>(off > 0 ? off : 1), float4{0, 0, 0, 0});
    auto put = [&](int32_t at, const void *src, size_t bytes) {
        if (bytes) std::memcpy(reinterpret_cast<char *>(blob.data()) + static_cast<size_t>(at) * 16, src, bytes);
    };
    put(lay.off_spheres, sph.data(), sph.size() * sizeof(SphereRec));
    put(lay.off_smeta, smeta.data(), smeta.size() * sizeof(SphereMeta));
    put(lay.off_boxes, boxes.data(), boxes.size() * sizeof(BoxRec));
    put(lay.off_mats, mrec.data(), mrec.size() * sizeof(MatRec));
    put(lay.off_lights, lrec.data(), lrec.size() * sizeof(LightRec));
    put(lay.off_lightmat, lm.data(), lm.size() * sizeof(LightMatRec));
    if (lay.off_bplane >= 0) put(lay.off_bplane, bplane.data(), bplane.size() * sizeof(float4));
    put(lay.off_bvh, bvh.data(), bvh.size() * sizeof(BvhNode));
    put(lay.off_blink, blink.data(), blink.size() * sizeof(uint32_t));
    if (lay.off_cone >= 0) put(lay.off_cone, cones.data(), cones.size() * sizeof(ShadowCone));
    if (lay.off_dmask >= 0) put(lay.off_dmask, dmask_bytes.data(), dmask_bytes.size());
    if (lay.off_gmask >= 0) put(lay.off_gmask, gmask.data(), gmask.size() * 8);
    if (lay.off_glist >= 0) put(lay.off_glist, glist.data(), glist.size());
    if (lay.off_olist >= 0) put(lay.off_olist, olist.data(), olist.size());
    return RT_OK;
}

// ---- animated scenes: the host's side of rt_anim_create / rt_anim_create2 ----
namespace {

// largest |value| a channel takes over the supported times
double channel_bound(const rt_anim_channel &ch, double base) {
    const double T = kAnimTimeBound;
    switch (ch.kind) {
        case RT_ANIM_RATE: return std::fabs(double(ch.k)) * T;
        case RT_ANIM_RATE_OFFSET: return std::fabs(double(ch.c)) + std::fabs(double(ch.k)) * T;
        case RT_ANIM_SIN: return std::fabs(double(ch.a)) * 1.0001;  // (the polynomial sin stays within 1 + 2^-20)
        case RT_ANIM_SIN_OFFSET: return std::fabs(double(ch.a)) * 1.0001 + std::fabs(double(ch.c));
        default: return std::fabs(base);
    }
}
bool channel_grows(const rt_anim_channel &ch) { return ch.kind == RT_ANIM_RATE || ch.kind == RT_ANIM_RATE_OFFSET; }
bool channel_finite(const rt_anim_channel &ch) {
    return ch.kind == RT_ANIM_NONE || (std::isfinite(ch.a) && std::isfinite(ch.k) && std::isfinite(ch.c));
}
// (first slot, count) of every node's subtree, from the leaf words
AnimNodeRange node_ranges(const BvhNode *nodes, int id, std::vector<AnimNodeRange> &out) {
    if (nodes[id].leaf) return out[id] = AnimNodeRange{nodes[id].leaf & 0xFFFFFF, nodes[id].leaf >> 24};
    const AnimNodeRange l = node_ranges(nodes, id + 1, out);
    int right = id + 1;  // the node after the left subtree
    right = nodes[right].skip;
    const AnimNodeRange r = node_ranges(nodes, right, out);
    return out[id] = AnimNodeRange{l.first, l.count + r.count};
}

}  // namespace

int anim_plan(const char *who_c, const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius,
              int n_objs, const rt_material *mats, int n_mats, const rt_light *lights, int n_lights, int max_frames,
              bool spheres, AnimPlan &plan) {
    const std::string who(who_c);
    if (!base || !anim || n_objs <= 0 || n_objs > RT_MAX_OBJECTS || !mats || n_mats <= 0 || n_mats > RT_MAX_MATERIALS ||
        n_lights < 0 || n_lights > RT_MAX_LIGHTS || (n_lights > 0 && !lights)) {
        set_error(who + ": bad arguments");
        return RT_ERR_INVALID;
    }
    if (max_frames < 1 || max_frames > RT_MAX_BATCH) {
        set_error(who + ": max_frames outside [1, " + std::to_string(RT_MAX_BATCH) + "]");
        return RT_ERR_INVALID;
    }
    const rt_anim_channel none{};
    std::vector<rt_object> bound(base, base + n_objs);  // every object where it reaches farthest
    std::vector<char> moving_sphere(n_objs, 0);
    int n_sph = 0, n_moving = 0;
    bool time_bound = false, box_moves = false;
    for (int i = 0; i < n_objs; ++i) {
        const rt_anim_channel *c = &anim[i].scale;  // 7 channels, contiguous
        const rt_anim_channel &rad = radius ? radius[i] : none;
        for (int k = 0; k < 8; ++k) {
            const int kind = k < 7 ? c[k].kind : rad.kind;
            if (kind < RT_ANIM_NONE || kind > RT_ANIM_SIN_OFFSET) {
                set_error(who + ": object " + std::to_string(i) + " has a channel of unknown kind " +
                          std::to_string(kind));
                return RT_ERR_INVALID;
            }
        }
        const int kind = object_kind(base[i]);
        n_sph += kind == 2;
        if (anim_is_static(anim[i]) && rad.kind == RT_ANIM_NONE) continue;
        if (kind != 1 && !spheres) {
            set_error(who + ": object " + std::to_string(i) +
                      " is not a box: channels are supported on box objects only (static spheres are fine)");
            return RT_ERR_UNSUPPORTED;
        }
        if (kind == 0) {
            set_error(who + ": object " + std::to_string(i) +
                      " is a null object: channels are supported on boxes and spheres only");
            return RT_ERR_UNSUPPORTED;
        }
        if (kind == 1) {  // (a radius channel on a box moves nothing the render reads)
            if (anim_is_static(anim[i])) continue;
            box_moves = true;
            const double s = channel_bound(anim[i].scale, 1.0) * (1.0 + 1e-6);
            for (int k = 0; k < 3; ++k) {
                bound[i].box_mins[k] = static_cast<float>(std::fabs(double(base[i].box_mins[k])) * s * (1.0 + 1e-6));
                bound[i].box_maxs[k] = static_cast<float>(std::fabs(double(base[i].box_maxs[k])) * s * (1.0 + 1e-6));
                bound[i].position[k] =
                    static_cast<float>(channel_bound(anim[i].position[k], base[i].position[k]) * (1.0 + 1e-6));
                time_bound = time_bound || channel_grows(anim[i].position[k]);
            }
            time_bound = time_bound || channel_grows(anim[i].scale);
            continue;
        }
        // a sphere moves by its position and radius channels (the render never
        // reads a sphere's angles or box extents)
        bool moves = rad.kind != RT_ANIM_NONE, finite = std::isfinite(base[i].radius) && channel_finite(rad) &&
                                                        std::isfinite(base[i].radius * base[i].radius);
        for (int k = 0; k < 3; ++k) {
            moves = moves || anim[i].position[k].kind != RT_ANIM_NONE;
            finite = finite && std::isfinite(base[i].position[k]) && channel_finite(anim[i].position[k]);
        }
        if (!moves) continue;
        if (!finite) {
            set_error(who + ": object " + std::to_string(i) +
                      " is a moving sphere whose base position, radius or channel constants are not finite");
            return RT_ERR_INVALID;
        }
        moving_sphere[i] = 1;
        ++n_moving;
        for (int k = 0; k < 3; ++k) {
            bound[i].position[k] =
                static_cast<float>(channel_bound(anim[i].position[k], base[i].position[k]) * (1.0 + 1e-6));
            time_bound = time_bound || channel_grows(anim[i].position[k]);
        }
        bound[i].radius = static_cast<float>(channel_bound(rad, base[i].radius) * (1.0 + 1e-6));
        time_bound = time_bound || channel_grows(rad);
    }
    const std::string limit = " has a moving sphere and " + std::to_string(n_sph) + " spheres: at most " +
                              std::to_string(RT_GMASK_FROM) +
                              " spheres may share a scene with a moving one (more need wide masks and candidate "
                              "lists, which are not rebuilt on the device)";
    if (n_moving > 0 && n_sph > RT_GMASK_FROM) {
        set_error(who + ": the scene" + limit);
        return RT_ERR_UNSUPPORTED;
    }
    const double extent = objects_extent(bound.data(), n_objs) * (1.0 + 1e-6);
    std::vector<float4> &blob = plan.blob;
    DeviceScene &ds = plan.ds;
    int rc = build_scene(base, n_objs, mats, n_mats, lights, n_lights, blob, ds, true, extent);
    if (rc != RT_OK) return rc;
    const SceneLayout &L = ds.layout;
    if ((static_cast<size_t>(L.blob_units) + view_units(L, false)) * sizeof(float4) > kMaxLds) {
        set_error(who + ": scene needs more than 160 KiB of LDS");
        return RT_ERR_UNSUPPORTED;
    }
    if (n_moving > 0 && (L.off_gmask >= 0 || ds.olist_eligible)) {  // (the layout's own word on the limit above)
        set_error(who + ": the scene" + limit);
        return RT_ERR_UNSUPPORTED;
    }
    // The room shape reads the one box's record and the lights (DeviceScene::
    // room): a box without channels keeps the host's record (the kernel leaves
    // it alone), so build_scene's decision stands; a moving box never claims it.
    const bool static_room = L.n_boxes == 1 && !box_moves;
    if (!static_room) ds.room = ds.room_fast = 0;
    // (norm_proof_scene read the spheres at their base places: no proof of a frame the device moves them in)
    if (!static_room || n_moving > 0) ds.norm = NormProof{};
    // the kernel's static table
    AnimTable T{};
    T.n_boxes = static_room ? 0 : L.n_boxes;
    T.n_lights = n_lights;
    T.n_spheres = L.n_spheres;
    T.dmask_n = L.dmask_n;
    T.dmask_bytes = L.dmask_bytes;
    T.dmask_box = L.dmask_box;
    T.extent = extent;
    T.finite = 1;
    T.n_bvh = L.n_bvh;
    T.blob_spheres = L.off_spheres;
    T.blob_smeta = L.off_smeta;
    T.blob_bvh = L.off_bvh;
    T.blob_cone = L.off_cone;
    std::vector<rt_object> tb;
    std::vector<rt_object_anim> ta;
    for (int i = 0; i < n_objs; ++i) {
        const bool box = object_kind(base[i]) == 1;
        bool fin = std::isfinite(base[i].radius);
        for (int k = 0; k < 3 && !box; ++k)
            fin = fin && std::isfinite(base[i].position[k]) && std::isfinite(base[i].box_mins[k]) &&
                  std::isfinite(base[i].box_maxs[k]);
        if (!fin) T.finite = 0;
        if (box && !static_room) {
            tb.push_back(base[i]);
            ta.push_back(anim[i]);
        }
    }
    // the moving spheres, by their slot in the template's leaf order
    std::vector<AnimSphere> ts;
    const SphereMeta *smeta = reinterpret_cast<const SphereMeta *>(blob.data() + L.off_smeta);
    uint64_t moving_bits = 0;
    // spheres the BVH covers: the finite ones, first in slot order (build_bvh)
    const BvhNode *nodes = reinterpret_cast<const BvhNode *>(blob.data() + L.off_bvh);
    std::vector<AnimNodeRange> ranges(std::max(L.n_bvh, 1), AnimNodeRange{0, 0});
    if (L.n_bvh > 0) node_ranges(nodes, 0, ranges);
    const int n_in_bvh = L.n_bvh > 0 ? ranges[0].count : 0;
    for (int s = 0; s < L.n_spheres && n_moving > 0; ++s) {
        const int i = smeta[s].obj_index;
        if (!moving_sphere[i]) continue;
        if (s >= n_in_bvh) {  // (unreachable: a moving sphere's base is finite)
            set_error(who + ": object " + std::to_string(i) + " is a moving sphere outside the BVH");
            return RT_ERR_INVALID;
        }
        AnimSphere a{};
        std::memcpy(a.position, base[i].position, 12);
        a.radius = base[i].radius;
        for (int k = 0; k < 3; ++k) a.ch[k] = anim[i].position[k];
        a.ch[3] = radius ? radius[i] : none;
        a.slot = s;
        ts.push_back(a);
        moving_bits |= uint64_t{1} << s;
    }
    T.n_msph = static_cast<int32_t>(ts.size());
    T.moving_slots = static_cast<uint32_t>(moving_bits);
    std::vector<float4> tl(std::max(n_lights, 1));
    const LightRec *lrec = reinterpret_cast<const LightRec *>(blob.data() + L.off_lights);
    for (int j = 0; j < n_lights; ++j) {
        const int32_t live = lrec[j].dead == 0.0f ? T.n_live++ : -1;
        tl[j] = make_float4(lights[j].position[0], lights[j].position[1], lights[j].position[2], 0.0f);
        std::memcpy(&tl[j].w, &live, 4);
    }
    std::vector<double> tc;
    std::vector<unsigned char> tm;
    if (L.dmask_n > 0 && (L.dmask_box || !ts.empty())) {
        const MaskConeTable mc = mask_cone_table(L.dmask_n);
        const size_t texels = static_cast<size_t>(6) * L.dmask_n * L.dmask_n;
        tc.resize(5 * texels);
        for (size_t t = 0; t < texels; ++t) {
            for (int k = 0; k < 3; ++k) tc[5 * t + k] = mc.w[3 * t + k];
            tc[5 * t + 3] = mc.ca[t];
            tc[5 * t + 4] = mc.sa[t];
        }
        // the template masks: the static spheres' bits alone
        tm.resize(static_cast<size_t>(T.n_live) * texels * L.dmask_bytes);
        unsigned char *m = reinterpret_cast<unsigned char *>(blob.data() + L.off_dmask);
        uint64_t keep = L.n_spheres >= 64 ? ~uint64_t{0} : ((uint64_t{1} << L.n_spheres) - 1u);
        keep &= ~moving_bits;
        for (size_t t = 0; t < static_cast<size_t>(T.n_live) * texels; ++t) {
            uint64_t v = 0;
            std::memcpy(&v, m + t * L.dmask_bytes, L.dmask_bytes);
            v &= keep;
            std::memcpy(m + t * L.dmask_bytes, &v, L.dmask_bytes);
        }
        std::memcpy(tm.data(), m, tm.size());
    }
    auto align16 = [](size_t x) { return (x + 15) / 16 * 16; };
    size_t at = align16(sizeof(AnimTable));
    T.off_base = static_cast<int32_t>(at);  at = align16(at + tb.size() * sizeof(rt_object));
    T.off_anim = static_cast<int32_t>(at);  at = align16(at + ta.size() * sizeof(rt_object_anim));
    T.off_light = static_cast<int32_t>(at); at = align16(at + tl.size() * sizeof(float4));
    T.off_cone = static_cast<int32_t>(at);  at = align16(at + tc.size() * sizeof(double));
    T.off_mask = static_cast<int32_t>(at);  at = align16(at + tm.size());
    T.off_msph = static_cast<int32_t>(at);  at = align16(at + ts.size() * sizeof(AnimSphere));
    T.off_node = static_cast<int32_t>(at);  at = align16(at + ranges.size() * sizeof(AnimNodeRange));
    std::vector<unsigned char> &table = plan.table;
    table.assign(at + 16, 0);
    std::memcpy(table.data(), &T, sizeof T);
    if (!tb.empty()) std::memcpy(table.data() + T.off_base, tb.data(), tb.size() * sizeof(rt_object));
    if (!ta.empty()) std::memcpy(table.data() + T.off_anim, ta.data(), ta.size() * sizeof(rt_object_anim));
    std::memcpy(table.data() + T.off_light, tl.data(), tl.size() * sizeof(float4));
    if (!tc.empty()) std::memcpy(table.data() + T.off_cone, tc.data(), tc.size() * sizeof(double));
    if (!tm.empty()) std::memcpy(table.data() + T.off_mask, tm.data(), tm.size());
    if (!ts.empty()) std::memcpy(table.data() + T.off_msph, ts.data(), ts.size() * sizeof(AnimSphere));
    std::memcpy(table.data() + T.off_node, ranges.data(), ranges.size() * sizeof(AnimNodeRange));
    plan.tab = T;
    plan.time_bound = time_bound;
    return RT_OK;
}

// Phase 3 of the animate kernel for one (ball, live light li): the cone's bit
// ORed into the light's masks, texel by texel.
static void or_cone_bits(const AnimPlan &plan, std::vector<float4> &blob, int li, const MaskCone &c) {
    const AnimTable &T = plan.tab;
    const size_t texels = static_cast<size_t>(6) * T.dmask_n * T.dmask_n;
    const double *w = reinterpret_cast<const double *>(plan.table.data() + T.off_cone);
    unsigned char *dmask = reinterpret_cast<unsigned char *>(blob.data() + plan.ds.layout.off_dmask);
    for (size_t t = 0; t < texels; ++t) {
        if (!texel_hit(w + 5 * t, w[5 * t + 3], w[5 * t + 4], c)) continue;
        unsigned char *m = dmask + (static_cast<size_t>(li) * texels + t) * T.dmask_bytes;
        uint64_t v = 0;
        std::memcpy(&v, m, T.dmask_bytes);
        v |= uint64_t{1} << c.bit;
        std::memcpy(m, &v, T.dmask_bytes);
    }
}

void anim_apply_boxes_host(const AnimPlan &plan, float time, std::vector<float4> &blob) {
    const AnimTable &T = plan.tab;
    const SceneLayout &L = plan.ds.layout;
    const unsigned char *table = plan.table.data();
    const rt_object *base = reinterpret_cast<const rt_object *>(table + T.off_base);
    const rt_object_anim *anim = reinterpret_cast<const rt_object_anim *>(table + T.off_anim);
    const float4 *light = reinterpret_cast<const float4 *>(table + T.off_light);
    BoxRec *boxes = reinterpret_cast<BoxRec *>(blob.data() + L.off_boxes);
    const int nb = T.n_boxes, nl = T.n_lights, n_mask_boxes = anim_mask_boxes(T);
    // 1. records, light_inside and balls
    std::vector<float4> ball(n_mask_boxes);
    bool finite = T.finite != 0;
    for (int b = 0; b < nb; ++b) {
        const rt_object o = animate_object(base[b], anim[b], time);
        box_record(o, boxes[b]);
        for (int r = 0; r < 3; ++r)
            finite = finite && std::isfinite(o.position[r]) && std::isfinite(o.box_mins[r]) &&
                     std::isfinite(o.box_maxs[r]);
        double R[3][3];
        rotation64(o.angles, R);
        uint32_t inside = 0;
        for (int j = 0; j < nl && j < 32; ++j)
            if (light_inside_box(o, R, &light[j].x)) inside |= 1u << j;
        boxes[b].light_inside = inside;
        if (b < n_mask_boxes) ball[b] = box_ball(o, R);
    }
    // 2. the separating planes; 3. the boxes' mask bits
    float4 *bplane = L.off_bplane >= 0 ? blob.data() + L.off_bplane : nullptr;
    for (int i = 0; bplane && i < nb * nl; ++i)
        bplane[i] = finite ? box_light_plane(boxes[i / nl], &light[i % nl].x, T.extent) : no_plane();
    for (int i = 0; i < n_mask_boxes * nl; ++i) {
        const int b = i / nl, j = i % nl;
        int32_t li;
        std::memcpy(&li, &light[j].w, 4);
        if (li >= 0) or_cone_bits(plan, blob, li, mask_cone(&ball[b].x, &light[j].x, T.n_spheres + b));
    }
}

void anim_apply_spheres_host(const AnimPlan &plan, float time, std::vector<float4> &blob) {
    const AnimTable &T = plan.tab;
    if (T.n_msph == 0) return;
    const unsigned char *table = plan.table.data();
    const AnimSphere *msph = reinterpret_cast<const AnimSphere *>(table + T.off_msph);
    const float4 *light = reinterpret_cast<const float4 *>(table + T.off_light);
    SphereRec *sph = reinterpret_cast<SphereRec *>(blob.data() + T.blob_spheres);
    SphereMeta *smeta = reinterpret_cast<SphereMeta *>(blob.data() + T.blob_smeta);
    // 1. records
    for (int i = 0; i < T.n_msph; ++i) {
        float rad;
        anim_sphere_records(msph[i], time, sph[msph[i].slot], rad);
        smeta[msph[i].slot].radius = rad;
    }
    // 2. the BVH's bounds and the ShadowCone entries
    const AnimNodeRange *range = reinterpret_cast<const AnimNodeRange *>(table + T.off_node);
    BvhNode *bvh = reinterpret_cast<BvhNode *>(blob.data() + T.blob_bvh);
    std::vector<SphereBox> sbox(T.n_spheres);
    for (int s = 0; s < T.n_spheres; ++s) sbox[s] = anim_sphere_box(sph[s], smeta[s].radius, T.extent);
    for (int n = 0; n < T.n_bvh; ++n) anim_node_bounds(sbox.data(), range[n], bvh[n].lo, bvh[n].hi);
    if (T.blob_cone >= 0) {
        ShadowCone *scone = reinterpret_cast<ShadowCone *>(blob.data() + T.blob_cone);
        for (int i = 0; i < T.n_msph; ++i)
            for (int j = 0; j < T.n_lights; ++j) {
                const int slot = msph[i].slot;
                scone[j * T.n_spheres + slot] = shadow_cone(sph[slot], smeta[slot].radius, &light[j].x);
            }
    }
    // 3. the moving spheres' mask bits
    if (T.dmask_n <= 0) return;
    for (int j = 0; j < T.n_lights; ++j) {
        int32_t li;
        std::memcpy(&li, &light[j].w, 4);
        if (li < 0) continue;
        for (int i = 0; i < T.n_msph; ++i) {
            const SphereRec &s = sph[msph[i].slot];
            const float ball[4] = {s.cx, s.cy, s.cz, smeta[msph[i].slot].radius};
            or_cone_bits(plan, blob, li, mask_cone(ball, &light[j].x, msph[i].slot));
        }
    }
}

}  // namespace rtamd

extern "C" {

// Development hook (host only, not part of include/rt.h): the code and
// message rt_anim_create2 would return for this description (rt_anim_create
// when `boxes_only`), without a device.
int rt_debug_anim_validate(const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius, int n_objs,
                           const rt_material *mats, int n_mats, const rt_light *lights, int n_lights, int max_frames,
                           int boxes_only) {
    AnimPlan plan;
    return anim_plan(boxes_only ? "rt_anim_create" : "rt_anim_create2", base, anim, boxes_only ? nullptr : radius,
                     n_objs, mats, n_mats, lights, n_lights, max_frames, !boxes_only, plan);
}

// Development hook (host only, not part of include/rt.h): the slot blob of
// rt_anim_create2's scene at `time` as the host makes it (rt_debug_anim_blob's
// layout): the animate kernel's phases in plain loops over the plan's table
// (anim_apply_boxes_host, anim_apply_spheres_host; the arithmetic is the
// kernel's own text, rt_cull.h and rt_anim.h) applied to the template. meta
// (24 ints): rt_debug_scene_blob's. Returns the blob's bytes (copied when
// they fit in cap), or a negative RT_ERR_*.
long long rt_debug_anim_host_blob(const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius,
                                  int n_objs, const rt_material *mats, int n_mats, const rt_light *lights,
                                  int n_lights, float time, void *out, long long cap, int32_t *meta) {
    AnimPlan plan;
    const int rc =
        anim_plan("rt_anim_create2", base, anim, radius, n_objs, mats, n_mats, lights, n_lights, 1, true, plan);
    if (rc != RT_OK) return rc;
    if (plan.time_bound && !(std::fabs(time) <= kAnimTimeBound)) {
        set_error("rt_debug_anim_host_blob: time outside the scene's range");
        return RT_ERR_UNSUPPORTED;
    }
    std::vector<float4> blob = plan.blob;
    anim_apply_boxes_host(plan, time, blob);
    anim_apply_spheres_host(plan, time, blob);
    const SceneLayout &L = plan.ds.layout;
    const long long bytes = static_cast<long long>(blob.size() * sizeof(float4));
    if (out && cap >= bytes) std::memcpy(out, blob.data(), static_cast<size_t>(bytes));
    if (meta) {
        const int32_t m[24] = {L.blob_units, L.off_spheres, L.off_smeta, L.off_boxes, L.off_mats,
                               L.off_lights, L.off_lightmat, L.off_bvh, L.n_bvh, L.off_blink, L.off_cone,
                               L.off_dmask, L.dmask_n, L.dmask_bytes, L.off_gmask, L.gmask_words,
                               L.off_glist, L.n_spheres, L.n_boxes, L.n_mats, L.n_lights, L.off_olist,
                               0, 0};
        std::memcpy(meta, m, sizeof m);
    }
    return bytes;
}

}  // extern "C"
