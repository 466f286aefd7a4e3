// rt_anim.h — a scene as a function of `time` (include/rt.h, rt_anim): the
// channel arithmetic the host (rt_animate_objects, rt_scene.cpp) and the
// animate kernel (rt_anim.hip) share, and the kernel's argument block.
#pragma once

#include <cmath>
#include <vector>

#include "rt_glmath.h"
#include "rt_internal.h"

namespace rtamd {

// One channel at `time`: float32, the written operation order, no fused
// multiply-add (-ffp-contract=off); `base` for RT_ANIM_NONE.
__host__ __device__ inline float anim_channel(const rt_anim_channel &ch, float time, float base) {
    switch (ch.kind) {
        case RT_ANIM_RATE: return time * ch.k;
        case RT_ANIM_RATE_OFFSET: {
            const float r = time * ch.k;
            return ch.c + r;
        }
        case RT_ANIM_SIN: {
            const float s = glf::gallivm_sincos(time * ch.k, false);
            return s * ch.a;
        }
        case RT_ANIM_SIN_OFFSET: {
            const float s = glf::gallivm_sincos(time * ch.k, false);
            const float p = ch.a * s;
            return p + ch.c;
        }
        default: return base;
    }
}
// An object at `time`: the scale multiplies box_mins / box_maxs componentwise,
// the position and angle channels replace their components.
__host__ __device__ inline rt_object animate_object(const rt_object &base, const rt_object_anim &an, float time) {
    rt_object o = base;
    if (an.scale.kind != RT_ANIM_NONE) {
        const float s = anim_channel(an.scale, time, 1.0f);
        for (int i = 0; i < 3; ++i) {
            o.box_mins[i] = base.box_mins[i] * s;
            o.box_maxs[i] = base.box_maxs[i] * s;
        }
    }
    for (int i = 0; i < 3; ++i) {
        o.position[i] = anim_channel(an.position[i], time, base.position[i]);
        o.angles[i] = anim_channel(an.angles[i], time, base.angles[i]);
    }
    return o;
}
inline bool anim_is_static(const rt_object_anim &an) {
    bool st = an.scale.kind == RT_ANIM_NONE;
    for (int i = 0; i < 3; ++i) st = st && an.position[i].kind == RT_ANIM_NONE && an.angles[i].kind == RT_ANIM_NONE;
    return st;
}

// A scene laid out for |time| <= kAnimTimeBound when a position, the scale or
// a radius has a RATE channel (include/rt.h).
constexpr float kAnimTimeBound = 1.0e4f;

// ---- moving spheres (rt_anim_create2) ---------------------------------------
// One text for the host (rt_animate_objects2, the host hook
// rt_debug_anim_host_blob) and the animate kernel's sphere phases.
//
// A moving sphere: its base centre and radius, the channels that move it
// (x, y, z, radius) and its slot in the template's leaf order (fixed at
// creation from the base objects).
struct AnimSphere {
    float position[3], radius;
    rt_anim_channel ch[4];
    int32_t slot, pad[3];
};
static_assert(sizeof(AnimSphere) == 96, "AnimSphere layout");
// The records build_scene makes of the sphere at `time`: centre, the float32
// product radius * radius, and |radius| (SphereMeta::radius).
__host__ __device__ inline void anim_sphere_records(const AnimSphere &s, float time, SphereRec &rec, float &abs_radius) {
    rec.cx = anim_channel(s.ch[0], time, s.position[0]);
    rec.cy = anim_channel(s.ch[1], time, s.position[1]);
    rec.cz = anim_channel(s.ch[2], time, s.position[2]);
    const float r = anim_channel(s.ch[3], time, s.radius);
    rec.rr = r * r;
    abs_radius = fabsf(r);
}
// A BVH node's subtree: a contiguous range of sphere slots.
struct AnimNodeRange {
    int32_t first, count;
};
// A sphere's box in float64 with build_bvh's margin (the table's extent bound
// stands in for the scene's: a larger margin only widens the box). The radius
// is the larger of sqrt(rr), what the intersection sees, and |radius|.
struct AnimSphereBox {
    double lo[3], hi[3];
};
__host__ __device__ inline AnimSphereBox anim_sphere_box(const SphereRec &s, float abs_radius, double extent) {
    const double c[3] = {s.cx, s.cy, s.cz};
    const double r = fmax(sqrt(static_cast<double>(s.rr)), static_cast<double>(abs_radius));
    double mag = 0.0;
    for (int a = 0; a < 3; ++a) mag = fmax(mag, fabs(c[a]) + r);
    const double margin = 1e-3 + 1e-4 * fmax(mag, extent);
    AnimSphereBox b;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = c[a] - r - margin;
        b.hi[a] = c[a] + r + margin;
    }
    return b;
}
// The node's bounds, refitted: the union of its subtree's sphere boxes (one
// per sphere slot), rounded outward to float32.
__host__ __device__ inline void anim_node_bounds(const AnimSphereBox *box, AnimNodeRange nr, float lo[3], float hi[3]) {
    double l[3] = {1e300, 1e300, 1e300}, h[3] = {-1e300, -1e300, -1e300};
    for (int s = nr.first; s < nr.first + nr.count; ++s)
        for (int a = 0; a < 3; ++a) {
            l[a] = fmin(l[a], box[s].lo[a]);
            h[a] = fmax(h[a], box[s].hi[a]);
        }
    for (int a = 0; a < 3; ++a) {
        lo[a] = nextafterf(static_cast<float>(l[a]), -HUGE_VALF);
        hi[a] = nextafterf(static_cast<float>(h[a]), HUGE_VALF);
    }
}
// build_scene's ShadowCone of a sphere seen from a light (float64).
__host__ __device__ inline ShadowCone anim_shadow_cone(const SphereRec &s, float abs_radius, const float light[3]) {
    ShadowCone c = {{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const double v[3] = {double(s.cx) - light[0], double(s.cy) - light[1], double(s.cz) - light[2]};
    const double d = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double rp = double(abs_radius) + 0.021 + 1e-3 * d;
    if (!(std::isfinite(d) && std::isfinite(rp)) || d <= rp) {
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
// The cone of a ball (centre, radius: a sphere, or a box's bounding sphere)
// seen from a live light, for the direction masks (build_direction_masks):
// axis, cos / sin of the half-angle + 1e-3, or every direction; `bit`: the
// ball's mask bit.
struct MaskCone {
    double ax[3], ch, sh;
    int32_t every, bit;
};
static_assert(sizeof(MaskCone) == 48, "MaskCone layout");
__host__ __device__ inline MaskCone anim_mask_cone(const float ball[4], const float light[3], int bit) {
    MaskCone c = {{0.0, 0.0, 0.0}, 0.0, 0.0, 0, bit};
    const double v[3] = {double(ball[0]) - double(light[0]), double(ball[1]) - double(light[1]),
                         double(ball[2]) - double(light[2])};
    const double d = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double rp = double(ball[3]) + 0.021 + 1e-3 * d;
    if (!(std::isfinite(d) && std::isfinite(rp)) || d <= rp) {
        c.every = 1;
    } else {
        for (int k = 0; k < 3; ++k) c.ax[k] = v[k] / d;
        const double half = asin(fmin(1.0, rp / d));
        c.ch = cos(half + 1e-3);
        c.sh = sin(half + 1e-3);
    }
    return c;
}
// The texel test (build_direction_masks): w = the texel's centre direction,
// cos / sin of its half-angle (5 doubles).
__host__ __device__ inline bool anim_texel_hit(const double *w, const MaskCone &c) {
    // cos(alpha + half + 1e-3), less 1e-12 for rounding
    const double lim = w[3] * c.ch - w[4] * c.sh - 1e-12;
    const double dot = w[0] * c.ax[0] + w[1] * c.ax[1] + w[2] * c.ax[2];
    return c.every != 0 || dot >= lim;
}

// The animate kernel's static table (device memory, built by rt_anim_create):
// what does not depend on `time`. Offsets in bytes from the table's start,
// every section 16-B aligned.
struct AnimTable {
    int32_t n_boxes, n_lights, n_live;
    int32_t dmask_n, dmask_bytes, dmask_box;  // the slots' LDS direction masks (SceneLayout)
    int32_t n_spheres;
    int32_t finite;     // 1: every time-independent field the plane test looks at is finite
    double extent;      // bound of the scene's extent over the supported times (rt_scene.cpp objects_extent)
    int32_t off_base;   // n_boxes rt_object: the boxes' base objects, in BoxRec order
    int32_t off_anim;   // n_boxes rt_object_anim
    int32_t off_light;  // n_lights x (3 float position, int32 live index or -1 for a dead light)
    int32_t off_cone;   // 6 n n texels x 5 double: centre direction, cos / sin of the half-angle (mask_cones)
    int32_t off_mask;   // n_live x 6 n n masks of dmask_bytes: the static spheres' bits
    uint32_t moving_slots;  // bit s: the sphere in slot s moves (a scene with a moving sphere has at most 32)
    // moving spheres (0 of them: the box phases alone)
    int32_t n_msph;
    int32_t off_msph;   // n_msph AnimSphere
    int32_t n_bvh;
    int32_t off_node;   // n_bvh AnimNodeRange
    // the sections of a slot the sphere phases rewrite, 16-B units (SceneLayout);
    // blob_cone -1: the layout has no ShadowCone table
    int32_t blob_spheres, blob_smeta, blob_bvh, blob_cone;
};
static_assert(sizeof(AnimTable) == 96, "AnimTable layout");
// balls with a bit in the LDS direction masks that the kernel recomputes:
// the boxes (scenes with box bits), then the moving spheres
inline int anim_mask_boxes(const AnimTable &t) { return t.dmask_box ? t.n_boxes : 0; }
inline int anim_mask_balls(const AnimTable &t) { return anim_mask_boxes(t) + (t.dmask_n > 0 ? t.n_msph : 0); }

// Kernel arguments: frame f (blockIdx.x) rewrites slot (first_slot + f) %
// n_slots at times[f].
struct AnimParams {
    const unsigned char *table;
    unsigned char *blobs;      // slot s at blobs + s * slot_bytes
    unsigned long long slot_bytes;
    int32_t first_slot, n_slots;
    int32_t off_boxes, off_bplane, off_dmask;  // 16-B units in a slot (SceneLayout)
    int32_t pad;
    float times[RT_MAX_BATCH];
};

// rt_anim.hip
// (spheres: the instance with the sphere phases, for a table with moving spheres)
hipError_t launch_animate(const AnimParams &p, bool spheres, int n_frames, size_t lds, hipStream_t stream);
// LDS bytes of an animate launch
size_t animate_lds(const AnimTable &t);

// rt_scene.cpp
// What rt_anim_create / rt_anim_create2 lay out on the host, no device needed:
// the template blob every slot starts as, its layout, and the kernel's table.
struct AnimPlan {
    std::vector<float4> blob;
    DeviceScene ds;
    AnimTable tab{};
    std::vector<unsigned char> table;
    bool time_bound = false;
};
// Validates the description and fills `plan`; the code and message are the
// entry point's (`who`: its name; spheres: rt_anim_create2's rules, else
// channels on boxes only).
int anim_plan(const char *who, const rt_object *base, const rt_object_anim *anim, const rt_anim_channel *radius,
              int n_objs, const rt_material *mats, int n_mats, const rt_light *lights, int n_lights, int max_frames,
              bool spheres, AnimPlan &plan);
// The sphere phases of the animate kernel on the host: rewrites, in `blob` (a
// copy of plan.blob), what the kernel rewrites for the moving spheres.
void anim_apply_spheres_host(const AnimPlan &plan, float time, std::vector<float4> &blob);
int object_kind_of(const rt_object &o);
// bound on |coordinate| of the finite objects (build_scene's BVH and plane margins)
double objects_extent(const rt_object *objs, int n_objs);
struct MaskConeTable {
    int n;
    const double *w, *ca, *sa;  // per texel (face-major): 3 doubles, 1, 1
};
MaskConeTable mask_cone_table(int n);

}  // namespace rtamd
