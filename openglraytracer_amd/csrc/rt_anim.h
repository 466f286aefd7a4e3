// rt_anim.h — a scene as a function of `time` (include/rt.h, rt_anim): the
// channel arithmetic the host (rt_animate_objects, rt_scene.cpp) and the
// animate kernel (rt_anim.hip) share, and the kernel's argument block. What
// follows from an object once it is placed — records, culling data — is
// rt_cull.h's, the text the scene builder runs too.
#pragma once

#include <cmath>
#include <vector>

#include "rt_cull.h"
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
// One text for the host (rt_animate_objects2, anim_apply_spheres_host) and
// the animate kernel's sphere phases.
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
// The box the refit gives a sphere: its radius the larger of sqrt(rr), what
// the intersection sees, and |radius|; the table's extent bound stands in for
// the scene's.
__host__ __device__ inline SphereBox anim_sphere_box(const SphereRec &s, float abs_radius, double extent) {
    return sphere_box(s, fmax(sqrt(static_cast<double>(s.rr)), static_cast<double>(abs_radius)), extent);
}
// The node's bounds, refitted: the union of its subtree's sphere boxes (one
// per sphere slot), rounded outward to float32.
__host__ __device__ inline void anim_node_bounds(const SphereBox *box, AnimNodeRange nr, float lo[3], float hi[3]) {
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
// The animate kernel's phases on the host, in plain loops over the plan's
// table: rewrite, in `blob` (a copy of plan.blob), what the kernel rewrites
// for the boxes and for the moving spheres.
void anim_apply_boxes_host(const AnimPlan &plan, float time, std::vector<float4> &blob);
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
