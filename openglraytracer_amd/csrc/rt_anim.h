// rt_anim.h — a scene as a function of `time` (include/rt.h, rt_anim): the
// channel arithmetic the host (rt_animate_objects, rt_scene.cpp) and the
// animate kernel (rt_anim.hip) share, and the kernel's argument block.
#pragma once

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

// A scene laid out for |time| <= kAnimTimeBound when a position or the scale
// has a RATE channel (include/rt.h).
constexpr float kAnimTimeBound = 1.0e4f;

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
    int32_t pad;
};

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
hipError_t launch_animate(const AnimParams &p, int n_frames, size_t lds, hipStream_t stream);
// LDS bytes of an animate launch
size_t animate_lds(const AnimTable &t);

// rt_scene.cpp
int object_kind_of(const rt_object &o);
// bound on |coordinate| of the finite objects (build_scene's BVH and plane margins)
double objects_extent(const rt_object *objs, int n_objs);
struct MaskConeTable {
    int n;
    const double *w, *ca, *sa;  // per texel (face-major): 3 doubles, 1, 1
};
MaskConeTable mask_cone_table(int n);

}  // namespace rtamd
